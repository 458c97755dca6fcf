"""The yardstick of tests/test_gpu_vort_diag.py checked without a GPU: the dense restatement of Euler::HorizPotVort and
HorizSolve::diagVertVort (tests/vort_diag_case.py) solves its own systems to round-off, its interface density is the reference's two-AXPY
form bit for bit, and its diagVertVort really sits at level 0."""
import numpy as np
import pytest

from tests import vort_diag_case as vc


@pytest.fixture(scope="module")
def case(oracle):
    return vc.make_case()


def test_restatement_is_self_consistent(case):
    gd, F = case["gd"], case["F"]
    uz, r1 = vc.horiz_pot_vort(gd, F["u1"], F["h1"])
    dwdx, r2 = vc.vert_vort(gd, F["velz1"], F["h1"])
    print("residuals  HorizPotVort: %s   diagVertVort: %s" % (" ".join("%.1e" % v for v in r1), " ".join("%.1e" % v for v in r2)))
    assert uz.shape == (vc.NK - 1, gd.N1) and dwdx.shape == (vc.NK - 1, gd.N1)
    assert np.isfinite(uz).all() and np.isfinite(dwdx).all()
    assert max(r1) < 1e-12 and max(r2) < 1e-12


def test_interface_density_is_the_two_axpy_form(case):
    rho = case["F"]["h1"]
    assert np.array_equal(vc.rho_bar(rho), vc.rho_bar_two_axpy(rho))
    assert (vc.rho_bar(rho) > 0.0).all()


def test_the_level_shows(case):
    """the mesh's thickness differs between levels, so an operator assembled at the wrong level is visible in the restatement"""
    gd, F = case["gd"], case["F"]
    rb = vc.rho_bar(F["h1"])
    a0, a1 = gd.mat("UHMAT", 0, flag=0, field=rb[1]), gd.mat("UHMAT", 1, flag=0, field=rb[1])
    m0, m1 = gd.mat("WMAT", 0, flag=1), gd.mat("WMAT", 1, flag=1)
    assert np.linalg.norm(a0 - a1) > 1e-3 * np.linalg.norm(a0) and np.linalg.norm(m0 - m1) > 1e-3 * np.linalg.norm(m0)
