"""Pins tests/box_schur2_case.py, the numpy restatement that tests/test_gpu_box_schur2.py checks the device against, on the CPU: the upwinded
theta diagnosis of box/VertSolve.cpp:499-531 against the lumped one where they must agree, the partition of unity of its shape functions, the
size of the seeded inputs, and that the box loop is far from the eul loop on them (so a device loop that ignored theta_up or the recomputed
uuz could not pass the GPU test)."""
import numpy as np
import pytest

from tests import box_schur2_case as bc
from tests.helpers import rel_l2

TOL = 1e-10                 # the parity bar of tests/test_gpu_schur2.py
# the shapes of tests/test_gpu_box_schur2.py: the column entry, then the loop
THETA_BOXES = [(1, 2, 2), (2, 2, 3), (3, 2, 5), (4, 2, 4), (2, 3, 3)]
LOOP_BOXES = [(3, 2, 5), (4, 2, 4)]
_CASES = {}


def case(oracle, shape, sphere=False):
    key = shape + (sphere,)
    if key not in _CASES:
        _CASES[key] = (bc.make_sphere if sphere else bc.make_box)(oracle, *shape)
    return _CASES[key]


def all_cases(oracle):
    return [case(oracle, s) for s in THETA_BOXES] + [case(oracle, (3, 2, 4), sphere=True)]


def test_zero_velocity_gives_the_lumped_theta(oracle):
    """velz = 0: N0b = N1t = 1, N1b = N0t = 0, VA2_up is the block-diagonal VA2 of AssembleLinearWithRho2 and theta equals Patch.diag_theta2"""
    for c in all_cases(oracle):
        P, st = c["P"], c["st"]
        zero = np.zeros_like(st["velz"])
        got = bc.diag_theta2_up_all(P, st["rho"], st["rt"], zero, bc.DTW)
        want = np.stack([P.diag_theta2(e % P.nElsX, e // P.nElsX, st["rho"][e], st["rt"][e]) for e in range(P.nEl)])
        err = rel_l2(got, want)
        print(P.n2e, P.nk, "%.3e" % err)
        assert err < 1e-12


def test_block_column_sums_do_not_depend_on_the_velocity(oracle):
    """N0 + N1 = 1 at both ends of a level: the sum of the two block rows of a level's block column of VAB2_up, and the sums over the block rows
    of every block column of VA2_up taken level by level, are those of velz = 0, to round-off"""
    for c in all_cases(oracle):
        P, st = c["P"], c["st"]
        nk, n2 = P.nk, P.n2e
        for e in (0, P.nEl - 1):
            AB, A = bc.upwind_matrices(P, e, st["rho"][e], st["velz"][e], bc.DTW)
            AB0, A0 = bc.upwind_matrices(P, e, st["rho"][e], 0.0 * st["velz"][e], bc.DTW)
            colsum = lambda M: M.reshape(nk + 1, n2, -1).sum(axis=0)
            for M, M0, name in ((AB, AB0, "VAB2_up"), (A, A0, "VA2_up")):
                err = np.abs(colsum(M) - colsum(M0)).max() / np.abs(colsum(M0)).max()
                print(name, n2, nk, "%.3e" % err)
                assert err < 1e-14, name
            assert np.abs(A - A0).max() > 0.01 * np.abs(A0).max()          # (the matrices themselves do move)


def test_inputs_upwind_enough_and_stay_block_dominant(oracle):
    """0.1 <= max_q |dtw w| <= 0.5 for the seeded velocities: the upwinding matters, and the off-diagonal blocks stay below the diagonal ones
    (the condition of use of mimsem_column_diag_theta_wup)"""
    for c in all_cases(oracle) + [case(oracle, s) for s in LOOP_BOXES]:
        m = bc.max_upwind(c["P"], c["st"]["velz"], bc.DTW)
        print("%.3f" % m)
        assert 0.1 <= m <= 0.5


def test_upwinded_theta_is_far_from_the_lumped_one(oracle):
    for c in all_cases(oracle):
        P, st = c["P"], c["st"]
        up = bc.diag_theta2_up_all(P, st["rho"], st["rt"], st["velz"], bc.DTW)
        lumped = np.stack([P.diag_theta2(e % P.nElsX, e // P.nElsX, st["rho"][e], st["rt"][e]) for e in range(P.nEl)])
        d = rel_l2(up, lumped)
        print(P.n2e, P.nk, "%.3e" % d)
        assert d > 100 * TOL


@pytest.mark.parametrize("shape", LOOP_BOXES, ids=lambda s: "p%d_ne%d_nk%d" % s)
def test_box_loop_is_far_from_the_eul_loop(oracle, shape):
    """three iterations: the box loop (upwinded theta, recomputed uuz) against the same loop with the lumped theta and dt udwdx; every compared
    field differs by more than 100 x the bar.  Each of the two differences alone moves them too"""
    c = case(oracle, shape)
    P, st = c["P"], c["st"]
    gd = bc.box_dense(c)
    uuz = lambda velz_j: bc.vert_mom_vort(c, gd, c["ul"], velz_j)
    args = (P, bc.DT, st["velz"], st["rho"], st["rt"], st["exner"], st["zv"], 3)
    box = bc.solve_schur_2_box(*args, udwdx=c["udwdx"], uuz=uuz)
    m = bc.max_upwind(P, box["velz"], bc.DTW)
    print("max |dtw w_j| after three iterations: %.3f" % m)
    assert m < 0.6                                       # the iterate stays where the unpivoted sweep of the device entry is safe
    for name, kw in (("eul", dict(theta_up=False)), ("theta only", dict(uuz=uuz, theta_up=False)), ("uuz only", dict(theta_up=True))):
        other = bc.solve_schur_2_box(*args, udwdx=c["udwdx"], **kw)
        moved = {k: rel_l2(box[k], other[k]) for k in ("velz", "rho", "rt", "exner", "theta_h", "exner_h")}
        print(name, {k: "%.2e" % v for k, v in moved.items()})
        assert all(np.isfinite(box[k]).all() for k in moved)
        small = [k for k, v in moved.items() if not v > 100 * TOL]
        assert not small, (name, small, moved)
