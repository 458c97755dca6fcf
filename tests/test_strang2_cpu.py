"""The numpy restatement of Euler::Strang (tests/strang2_case.py), pinned on the CPU against the restatements it is composed from: the
point-wise mass-flux right-hand side of csrc/flux_rhs.inc against the four-term GlobalDense.uvec_hu sum, its vertical stage against
schur2_case.solve_schur_2, its momentum updates against the dense M1 lines, and the two sensitivity conditions the GPU bars of
tests/test_gpu_strang2.py rest on.  No GPU."""
import numpy as np
import pytest

from tests import schur2_case as s2
from tests import strang2_case as s2c
from tests import strang_case as sc
from tests.helpers import rel_l2

FIELDS = ("velx", "velz", "rho", "rt", "exner")


@pytest.fixture(scope="module")
def case(oracle):
    return sc.make_case()


@pytest.fixture(scope="module")
def two_steps(case):
    """two steps of the restatement; after each the state, the predictor, Fu of stage 1 and the carried vectors"""
    R = s2c.Restatement2(case)
    st, rec = case["state"], []
    for _ in range(2):
        u_in = st[0]
        st = R.step(*st)
        rec.append(dict(state=st, u_in=u_in, velx_p=R.velx_p, Fu_1=R.Fu_1, u_prev=R.u_prev, u_curr=R.u_curr, uz=R.uz, uz_prev=R.uz_prev,
                        k2i=(R.k2i, R.k2i_abs)))
    return R, rec


def test_pointwise_flux_rhs_is_the_four_term_uvec_hu_sum(case):
    """1e-13: the two sides add the same ~ 4 x 16 products per entry in another order, round-off ~ 1e-16 sqrt(64); two orders of margin"""
    c, gd, nk = case, case["gd"], case["nk"]
    r = np.random.default_rng(7)
    u1 = c["velx"]; u2 = u1 * (1 + 0.05 * r.standard_normal(u1.shape))
    h1 = c["rho"]; h2 = h1 * (1 + 0.01 * r.standard_normal(h1.shape))
    for k in range(nk):
        want = s2c.flux_rhs(gd, k, u1[k], u2[k], h1[k], h2[k])
        got = np.zeros(gd.N1)
        for t, g, P in c["patches"]:
            np.add.at(got, t.loc1, s2c.flux_rhs_pointwise(P, k, gd.l1(t, u1[k]), gd.l1(t, u2[k]), gd.l2(t, h1[k]), gd.l2(t, h2[k])))
        err = rel_l2(got, want)
        print("level %d: |point-wise - sum of uvec_hu| / |sum| = %.2e" % (k, err))
        assert err < 1e-13, k
        # the aliased call of stage 1 is the plain product: weights 1/3 + 1/6 + 1/6 + 1/3 = 1
        assert rel_l2(s2c.flux_rhs(gd, k, u1[k], u1[k], h1[k], h1[k]), gd.uvec_hu(k, u1[k], h1[k], 1.0)) < 1e-13


def test_interface_rows_change_layout_like_the_level_rows(case):
    c, nk = case, case["nk"]
    assert np.array_equal(s2c.to_horiz(c, sc.to_vert(c, c["rho"]), nk), c["rho"])
    assert np.array_equal(s2c.to_horiz(c, c["velz_v"], nk - 1), sc.to_horiz(c, c["velz_v"], nk - 1))


def test_stage_2_without_wind_is_solve_schur_2_patch_by_patch(case):
    """zero velx: Fk = Gk = 0, the forcing vanishes and the stage is schur2_case.solve_schur_2 on every patch, same iteration count"""
    c = case
    velx, velz_v, rho, rt, exner = c["state"]
    R = s2c.Restatement2(c)
    zero = np.zeros_like(velx)
    got = R.stage2(zero, zero, velz_v, rho, rt, exner)
    assert not R.Fk.any()
    rho_v, rt_v, exner_v = (sc.to_vert(c, a) for a in (rho, rt, exner))
    e0 = 0
    for t, g, P in c["patches"]:
        s = slice(e0, e0 + P.nEl)
        want = s2.solve_schur_2(P, sc.DT, velz_v[s], rho_v[s], rt_v[s], exner_v[s], c["zv_v"][s], sc.NITS)
        for a, name in zip(got, ("velz", "rho", "rt", "exner")):
            assert np.all(np.isfinite(want[name])), name
            assert rel_l2(a[s], want[name]) < 1e-13, (t.pi, name, rel_l2(a[s], want[name]))
        e0 += P.nEl
    assert rel_l2(got[1], rho_v) > 1e-9                        # the loop did move the state


def test_stage_1_is_the_forward_then_the_leapfrog_line(case, two_steps):
    """first step: M1 velx = M1 velx_0 - dt Fu; second step: M1 velx = M1 u_prev - 2 dt Fu with u_prev the velx the FIRST step started from
    (eul/Euler_2.cpp:1214-1226), on the dense M1 of tests/hmomentum_case.py"""
    R, rec = two_steps
    dense, dt = R.dense, sc.DT
    assert np.array_equal(rec[0]["u_curr"], case["velx"]) and rec[0]["u_prev"] is None
    assert np.array_equal(rec[1]["u_prev"], case["velx"]) and np.array_equal(rec[1]["u_curr"], rec[0]["state"][0])
    assert np.array_equal(rec[0]["uz_prev"], sc.vc.horiz_pot_vort(case["gd"], case["velx"], case["rho"])[0])      # :1205
    assert not np.array_equal(rec[1]["uz_prev"], rec[0]["uz_prev"]) and not np.array_equal(rec[1]["uz_prev"], rec[1]["uz"])     # :1187-1189
    for step, (cfac, u_a) in enumerate(((1.0, rec[0]["u_in"]), (2.0, rec[0]["u_in"]))):
        for k in range(case["nk"]):
            M = dense.m1(k)
            b = M @ u_a[k] - cfac * dt * rec[step]["Fu_1"][k]
            assert rel_l2(M @ rec[step]["velx_p"][k], b) < 1e-13, (step, k)
    assert rel_l2(rec[1]["u_in"], rec[0]["u_in"]) > 1e-6       # (so the second line is told apart from M1 velx_0 - 2 dt Fu)
    assert all(r["k2i"][1] > 0 and np.isfinite(r["k2i"][0]) for r in rec)


def test_two_steps_stay_finite_and_move(case, two_steps):
    R, rec = two_steps
    for s in rec:
        assert all(np.all(np.isfinite(a)) for a in s["state"])
    for a, b in zip(rec[0]["state"], case["state"]):
        assert rel_l2(a, b) > 1e-12
    assert not R.first_step


def test_the_transport_forcing_moves_every_stage_2_field(case, two_steps):
    """the GPU step test can only see a wrong advection_rhs if the forcing moves the fields of stage 2 by far more than their bars: a first
    step with and without it, relative L2 of the difference against 100 x the bar of step 1"""
    R, rec = two_steps
    off = s2c.Restatement2(case, transport=False).step(*case["state"])
    moved = {n: rel_l2(a, b) for n, a, b in zip(FIELDS, rec[0]["state"], off)}
    print("transport forcing on / off, step 1: " + "  ".join("%s %.2e" % kv for kv in moved.items()))
    for n in ("velz", "rho", "rt", "exner"):
        assert moved[n] > 100 * s2c.BARS[1][n], (n, moved[n], s2c.BARS[1][n])


def test_strang_differs_from_strang_ec_in_every_field(case, two_steps):
    """the restated Strang step against the restated Strang_ec step: more than 100 x the bar in every field that carries one, so a device
    step that took an _ec routine by mistake cannot pass tests/test_gpu_strang2.py"""
    R, rec = two_steps
    ec = sc.Restatement(case).step(*case["state"])
    moved = {n: rel_l2(a, b) for n, a, b in zip(FIELDS, rec[0]["state"], ec)}
    print("Strang against Strang_ec, step 1: " + "  ".join("%s %.2e" % kv for kv in moved.items()))
    for n in FIELDS:
        assert moved[n] > 100 * s2c.BARS[1][n], (n, moved[n], s2c.BARS[1][n])
