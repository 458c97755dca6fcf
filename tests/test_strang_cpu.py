"""The numpy restatement of Euler::Strang_ec (tests/strang_case.py), pinned on the CPU against the restatements it is composed from: its
vertical stage against oracle/vert_oracle.py, its momentum updates against the dense M1 / M1ray lines of tests/hmomentum_case.py, and the
point-wise Bernoulli formula of csrc/bernoulli.inc against HorizOracle.diagnose_Phi.  No GPU."""
import numpy as np
import pytest

from tests import strang_case as sc
from tests.helpers import rel_l2


@pytest.fixture(scope="module")
def case(oracle):
    return sc.make_case()


@pytest.fixture(scope="module")
def two_steps(case):
    """two steps of the restatement; after each the state, the predictor, Fu of stage 1 and the carried vectors"""
    R = sc.Restatement(case)
    st, rec = case["state"], []
    for _ in range(2):
        u_in = st[0]
        st = R.step(*st)
        rec.append(dict(state=st, u_in=u_in, velx_p=R.velx_p, Fu_1=R.Fu_1, u_prev=R.u_prev, u_curr=R.u_curr, uz=R.uz, uz_prev=R.uz_prev))
    return R, rec


def test_stage_2_without_wind_is_the_oracle_newton_loop(case):
    """zero velx: the transport tendencies vanish and the stage is vert_oracle.solve_schur_eta patch by patch, same iteration count"""
    from oracle import vert_oracle
    c = case
    velx, velz_v, rho, rt, exner = c["state"]
    R = sc.Restatement(c)
    zero = np.zeros_like(velx)
    got = R.stage2(zero, zero, velz_v, rho, rt, exner)
    rho_v, rt_v, exner_v = (sc.to_vert(c, a) for a in (rho, rt, exner))
    e0 = 0
    for t, g, P in c["patches"]:
        s = slice(e0, e0 + P.nEl)
        want = vert_oracle.solve_schur_eta(P, sc.DT, velz_v[s], rho_v[s], rt_v[s], exner_v[s], c["zv_v"][s], sc.NITS)
        for a, b, name in zip(got, want[:4], ("velz", "rho", "rt", "exner")):
            assert np.all(np.isfinite(b)), name
            assert rel_l2(a[s], b) < 1e-13, (t.pi, name, rel_l2(a[s], b))
        e0 += P.nEl
    assert rel_l2(got[1], rho_v) > 1e-9                        # the loop did move the state


def test_stage_1_is_the_forward_then_the_leapfrog_line(case, two_steps):
    """first step: M1 velx = M1 velx_0 - dt Fu; second step: M1 velx = M1 u_prev - 2 dt Fu with u_prev the velx the FIRST step started from
    (eul/Euler_2.cpp:1433-1445), on the dense M1 of tests/hmomentum_case.py"""
    R, rec = two_steps
    dense, dt = R.dense, sc.DT
    assert np.array_equal(rec[0]["u_curr"], case["velx"]) and rec[0]["u_prev"] is None
    assert np.array_equal(rec[1]["u_prev"], case["velx"]) and np.array_equal(rec[1]["u_curr"], rec[0]["state"][0])
    assert np.array_equal(rec[0]["uz_prev"], sc.vc.horiz_pot_vort(case["gd"], case["velx"], case["rho"])[0])      # :1425
    assert not np.array_equal(rec[1]["uz_prev"], rec[0]["uz_prev"]) and not np.array_equal(rec[1]["uz_prev"], rec[1]["uz"])     # :1407-1409
    for step, (cfac, u_a) in enumerate(((1.0, rec[0]["u_in"]), (2.0, rec[0]["u_in"]))):
        for k in range(case["nk"]):
            M = dense.m1(k)
            b = M @ u_a[k] - cfac * dt * rec[step]["Fu_1"][k]
            assert rel_l2(M @ rec[step]["velx_p"][k], b) < 1e-13, (step, k)
    assert rel_l2(rec[1]["u_in"], rec[0]["u_in"]) > 1e-6       # (so the second line is told apart from M1 velx_0 - 2 dt Fu)


def test_stage_1_with_friction_solves_m1_plus_m1ray(case):
    c = case
    velx, velz_v, rho, rt, exner = c["state"]
    R = sc.Restatement(c, hs_forcing=True)
    p = R.stage1(velx, sc.to_horiz(c, velz_v, c["nk"] - 1), rho, rt, exner)
    plain = sc.momentum_update(R.dense, R.hz.M1, sc.DT, velx, R.Fu_1, 1.0, None)
    for k in range(c["nk"]):
        A = R.dense.m1(k) + R.dense.m1ray(k, sc.DT, R.dense.local2(exner[k]), R.dense.local2(exner[0]))
        assert rel_l2(A @ p[k], R.dense.m1(k) @ velx[k] - sc.DT * R.Fu_1[k]) < 1e-13, k
    assert rel_l2(p, plain) > 1e-12                             # the friction is felt


def test_pointwise_bernoulli_is_diagnose_phi(case):
    c, gd, nk = case, case["gd"], case["nk"]
    hz = c["ho"].HorizOracle(gd)
    r = np.random.default_rng(7)
    u1 = c["velx"]; u2 = u1 * (1 + 0.05 * r.standard_normal(u1.shape))
    z1 = sc.to_horiz(c, c["velz_v"], nk - 1); z2 = z1 * (1 + 0.05 * r.standard_normal(z1.shape))
    for k in range(nk):
        want = hz.diagnose_Phi(k, u1[k], u2[k], z1, z2)
        got = np.zeros(gd.N2)
        for t, g, P in c["patches"]:
            own = t.pi * t.n2 + np.arange(t.n2)
            got[own] = sc.bernoulli_pointwise(P, t, k, nk, gd.l1(t, u1[k]), gd.l1(t, u2[k]), np.ascontiguousarray(z1[:, own]), np.ascontiguousarray(z2[:, own]))
        err = rel_l2(got, want)
        print("level %d: |point-wise - diagnose_Phi| / |diagnose_Phi| = %.2e" % (k, err))
        assert err < 1e-13, k


def test_k2i_of_stage_3_is_the_oracles(case, two_steps):
    """Restatement.k2i (from dp restated after eul/HorizSolve.cpp:699-708) is what HorizOracle.momentum_rhs_ec returns with Fk"""
    R, rec = two_steps
    c, nk = case, case["nk"]
    velx_0, velz_v0 = rec[0]["state"][0], rec[0]["state"][1]
    velz_hn = sc.to_horiz(c, rec[1]["state"][1], nk - 1); velz_h0 = sc.to_horiz(c, velz_v0, nk - 1)
    k2i = 0.0
    for k in range(nk):
        k2i += R.hz.momentum_rhs_ec(k, R.theta_l2_h[k], R.uz, R.uz_prev, velz_hn, velz_h0, R.exner_h[k], velx_0[k], R.velx_p[k],
                                    rec[0]["state"][2][k], rec[1]["state"][2][k], Fk=R.Fk[k])[1]
    assert R.k2i_abs > 0 and abs(k2i - R.k2i) < 1e-13 * R.k2i_abs, (k2i, R.k2i, R.k2i_abs)


def test_two_steps_stay_finite_and_move(case, two_steps):
    R, rec = two_steps
    for s in rec:
        assert all(np.all(np.isfinite(a)) for a in s["state"])
    for a, b in zip(rec[0]["state"], case["state"]):
        assert rel_l2(a, b) > 1e-12
    assert not R.first_step
