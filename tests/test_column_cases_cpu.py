"""The builder behind tests/test_gpu_column_every_column.py, checked without a GPU: the map from a context column to (oracle patch, element),
the inputs (the oracle alone is well-posed on them; no two columns carry the same row) and the per-column comparison, which must name a
single wrong interior column by its index."""
import numpy as np
import pytest

from tests import column_cases as cc
from tests.helpers import _rel_ld, ld_solve

CASES = cc.all_cases()
COLUMNS = dict(S1=1, S3=3, S5=5, S6=6, S9=9, S18=18, B9=9, B4=4)


def test_the_case_list_is_the_one_of_the_table():
    by_order = {}
    for name, pn, nk in CASES:
        by_order.setdefault(pn, set()).add((name, nk))
    both = lambda *names: {(n, nk) for n in names for nk in (4, 5)}
    assert by_order[1] == {("B9", 5), ("B4", 4)}
    assert by_order[2] == both("S3", "S5", "S6", "S9", "S18")
    assert by_order[3] == by_order[4] == both("S3", "S5", "S6", "S9")
    assert by_order[5] == by_order[6] == both("S1", "S3", "S5")
    assert len(CASES) == len(set(CASES)) == 40


@pytest.fixture(scope="module", params=CASES, ids=cc.case_id)
def case(request, oracle):
    return cc.build_case(oracle, *request.param)


def test_column_map_and_geometry(case):
    """dm.det[e] and dm.thick[:, e] are the oracle patch's det and thick of the mapped element.  thick: bit for bit everywhere (both sides
    halve the same level differences).  det: bit for bit on the box (the oracle is handed the package's array, Patch.set_metric); on the sphere
    the oracle evaluates the Jacobian itself in C and the package in numpy, in another order of operations: rtol 1e-14"""
    dm = case.dm
    assert dm.nEl == COLUMNS[case.name] == len(case.where)
    assert case.numbering == ("local" if case.one_patch else "global")
    seen = set()
    for e in range(dm.nEl):
        i, le = case.where[e]
        assert e == case.el0[i] + le and (i, le) not in seen
        seen.add((i, le))
        P, ex, ey = case.col(e)
        assert (ex, ey) == (le % P.nElsX, le // P.nElsX) and P.nk == case.nk and P.n2e == case.n2e
        iq = P.elinds("q")[le]
        assert np.array_equal(dm.thick[:, e], P.thick[:, iq]), e
        assert np.array_equal(dm.thickInv[:, e], P.thickInv[:, iq]), e
        if case.name in cc.BOXES:
            assert np.array_equal(dm.det[e], P.det[le]), e
        else:
            assert np.allclose(dm.det[e], P.det[le], rtol=1e-14, atol=0.0), e
    if case.one_patch:                                   # the 1-form row of the entries that take uh is the patch's own
        P = case.P0
        assert dm.n1 == P.n1 and np.array_equal(dm.inds1x, P.elinds("n1x")) and np.array_equal(dm.inds1y, P.elinds("n1y"))
        assert np.array_equal(dm.indsq, P.elinds("q"))
        lat = case.latitudes()
        assert lat.shape == (dm.nEl, (case.pn + 1) ** 2) and (np.abs(lat) <= np.pi / 2).all() and np.ptp(lat) > 0.0
        assert case.name not in cc.BOXES or (np.abs(lat) < np.pi / 2).all()     # (a polar face holds the pole itself at even orders)
        assert np.array_equal(lat, P.sq[:, 1][P.elinds("q")])


def _distinct_rows(a):
    a = np.asarray(a)
    return len({r.tobytes() for r in a}) == a.shape[0]


def test_no_two_columns_share_an_input_row(case):
    """a kernel that reads the wrong column cannot pass: every field and every right-hand side differs between any two columns, and so does
    the geometry a column operator is built from (thick: the perturbed levels)"""
    F = case.fields()
    for k, v in F.items():
        assert v.shape[0] == case.nEl and _distinct_rows(v), k
    for seed in (9, 29):
        for v in case.rhs(seed):
            assert _distinct_rows(v)
    assert _distinct_rows(case.dm.thick.transpose(1, 0, 2).reshape(case.nEl, -1))


def test_the_oracle_alone_is_well_posed_on_these_inputs(case):
    """conditions on the inputs, not measurements of the device: every oracle solve is finite, the oracle solves its own system to 1e-11
    (oracle_vs_own_system of helpers.solve_error_budget: the oracle's solution against the extended-precision solve of the oracle's system)
    and cond(L) < 1e8, for solve_schur_column_eta and solve_schur_column_3 with flags 0 and 3, on every column"""
    F = case.fields()
    worst = dict(own=0.0, cond=0.0)
    for e in range(case.nEl):
        P, ex, ey = case.col(e)
        Fs = [f[e] for f in case.rhs(9)]
        refs = [(P.solve_schur_column_eta(ex, ey, 75.0, F["thetaL"][e], F["rho"][e], F["eta"][e], F["pi"][e], *Fs), "L_pi", "F_pi", "d_pi")]
        Fs = [f[e] for f in case.rhs(29)]
        for flags in (0, 3):
            refs.append((P.solve_schur_column_3(ex, ey, 75.0, F["theta"][e], F["velz"][e], F["rho"][e], F["rt"][e], F["pi"][e], *Fs, flags=flags),
                         "L", "F_rt", "d_rt"))
        for ref, kL, kF, kd in refs:
            for k, v in ref.items():
                assert np.isfinite(v).all(), (e, k)
            own = _rel_ld(ref[kd], ld_solve(ref[kL], ref[kF]))
            cond = float(np.linalg.cond(ref[kL]))
            worst = dict(own=max(worst["own"], own), cond=max(worst["cond"], cond))
            assert own < 1e-11 and cond < 1e8, (e, kL, own, cond)
    print("oracle on %s: own-system error %.1e, cond(L) %.1e" % (case.label, worst["own"], worst["cond"]))


@pytest.mark.parametrize("param", [c for c in CASES if c[0] in cc.ONE_PATCH], ids=cc.case_id)
def test_the_upwinded_theta_system_is_well_posed(oracle, param):
    """the oracle is a reference for diagTheta_up at 1e-10 only where its own solve is far below that: on every column of the one-patch shapes,
    with the velocities of Case.uh, the oracle's theta is within 1e-12 of the extended-precision solution of VA2_up theta = VAB2_up rt and the
    diagonal blocks of VA2_up have cond < 1e8 (the bound of the Schur systems above).  A condition on the inputs; the device is not involved"""
    case = cc.build_case(oracle, *param)
    F = case.fields()
    dt, n2, nk = 60.0, case.n2e, case.nk
    uh = case.uh(np.random.default_rng(21), dt)                    # the draw of test_gpu_column_every_column.test_diag_theta_up_and_temp_forcing
    worst = dict(own=0.0, cond=0.0)
    for e in range(case.nEl):
        P, ex, ey = case.col(e)
        A = P.colop_dense_ex("LINEAR_RHO2_UP", ex, ey, param=dt, f1=F["rho"][e], uh=uh)
        b = P.colop_dense_ex("LINCON2_UP", ex, ey, param=dt, uh=uh) @ F["rt"][e]
        th = P.diag_theta_up(ex, ey, dt, F["rho"][e], F["rt"][e], uh)
        assert np.isfinite(th).all()
        own = _rel_ld(th, ld_solve(A, b))
        cond = max(float(np.linalg.cond(A[k * n2:(k + 1) * n2, k * n2:(k + 1) * n2])) for k in range(nk + 1))
        worst = dict(own=max(worst["own"], own), cond=max(worst["cond"], cond))
        assert own < 1e-12 and cond < 1e8, (e, own, cond)
    assert np.abs(uh).max() > 0.0
    print("oracle diag_theta_up on %s: own-system error %.1e, cond of the worst VA2_up block %.1e" % (case.label, worst["own"], worst["cond"]))


# ---- the comparison helper can fail, and says where -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nEl,bad", [(3, 1), (5, 2), (6, 4), (9, 7), (18, 16)])
def test_one_wrong_interior_column_is_reported_by_index(nEl, bad):
    """a device result in which exactly ONE interior column (not 0, not nEl - 1: the two the suite used to look at) carries a relative error
    of 1e-8, and that column is small beside the others, so a whole-array norm would pass it"""
    assert 0 < bad < nEl - 1
    r = np.random.default_rng(nEl)
    want = r.standard_normal((nEl, 40)) * 1e8
    want[bad] *= 1e-6                                                        # small beside its neighbours
    got = want.copy()
    d = r.standard_normal(40)
    got[bad] += 1e-8 * np.linalg.norm(want[bad]) * d / np.linalg.norm(d)
    assert cc.rel_l2(got, want) < cc.TOL                                     # the whole-array norm does not see it
    assert cc.rel_l2(got[[0, nEl - 1]], want[[0, nEl - 1]]) == 0.0           # nor do the first and the last column
    cols, err = cc.failing_columns(got, want)
    assert cols == [bad] and abs(err[bad] / 1e-8 - 1.0) < 1e-6 and (np.delete(err, bad) == 0.0).all()
    with pytest.raises(AssertionError, match=r"column %d above" % bad):
        cc.assert_columns("self-check", got, want)
    assert cc.assert_columns("self-check", want.copy(), want) == 0.0
    got[bad] = np.nan                                                        # a NaN column fails too
    assert cc.failing_columns(got, want)[0] == [bad]
