"""CPU checks of the restatement of Euler::diagnostics (tests/energetics_case.py) that the GPU tests of mimsem_amd/energetics.py compare with, and
of Energetics.write_line.  No GPU."""
import numpy as np
import pytest

from tests import energetics_case as ec


@pytest.fixture(scope="module")
def case(oracle):
    return ec.make_case()


def test_mass_is_the_sum_of_the_density_dofs(case):
    """the edge functions integrate to one under GLL quadrature, so int2 of a 2-form is the sum of its DoFs"""
    from mimsem_amd import energetics  # noqa: F401  (the module under test exists)
    mass, s_abs = ec.restate_horizontal(case)["mass"]
    want = float(case["rho"].sum())
    print("mass %.16g  rho.sum() %.16g  relative difference %.2e" % (mass, want, abs(mass - want) / want))
    assert abs(mass - want) <= 1e-13 * want
    assert abs(s_abs - mass) <= 1e-13 * mass                   # a positive density: no cancellation


def test_matrix_route_equals_the_quadrature_point_formulas(case):
    """pins the formulas csrc/energetics.inc is written from: the assembled Uhmat / Wmat route of the reference against a plain evaluation at
    the quadrature points, to 1e-12 of S_abs"""
    from mimsem_amd import energetics  # noqa: F401
    mat, plain = ec.restate_horizontal(case), ec.plain_quadrature(case)
    for n in ("keh", "ie", "entr"):
        err = abs(mat[n][0] - plain[n][0]) / mat[n][1]
        print("%-5s matrix route %.16g  quadrature points %.16g  |difference| / S_abs %.2e" % (n, mat[n][0], plain[n][0], err))
        assert mat[n][0] > 0 and err <= 1e-12


def test_column_restatement_is_finite_and_signed(case):
    col = ec.restate_column(case)
    for n in ec.COLUMN:
        s, a = col[n]
        assert np.isfinite(s) and a > 0 and abs(s) <= a * (1 + 1e-15)
    assert col["kev"][0] != 0 and col["pe"][0] > 0


def test_write_line_format(tmp_path):
    """every value as %.16g and a tab, then a newline: what `file.precision(16); file << v << "\\t"; ... << endl` writes (eul/Euler_2.cpp:716-734).
    The double nearest 1e-20 is 9.99999999999999945e-21, which 16 significant digits print as 9.999999999999999e-21 (the reference's stream
    does too); 1e-22 is a small value that prints short."""
    from mimsem_amd.energetics import FIELDS, Energetics
    vals = [0.5, 1.0 / 3.0, 1e-20, -2.0, 123456789.125, 0.0, 1e300, -1e-300, 3.0, 0.1, 5.13e18, 1e-22]
    want = ("0.5\t0.3333333333333333\t9.999999999999999e-21\t-2\t123456789.125\t0\t1e+300\t-1e-300\t3\t0.1\t5.13e+18\t1e-22\t\n").encode()
    p = tmp_path / "energetics.dat"
    Energetics.write_line(str(p), vals)
    assert p.read_bytes() == want
    Energetics.write_line(str(p), vals)                         # appends
    assert p.read_bytes() == want + want
    assert len(FIELDS) == 12 and FIELDS[0] == "keh" and FIELDS[10] == "mass" and FIELDS[11] == "entr"
    with pytest.raises(ValueError):
        Energetics.write_line(str(p), vals[:11])
