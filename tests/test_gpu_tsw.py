"""The thermal shallow-water step on the device (mimsem_tsw_diagnose / mimsem_tsw_update, mimsem_amd.thermalsw) against the numpy oracle
of ThermalSW_EEC_2::solve_rk (tests/tsw_oracle.py): the two kernels per output at every built order, the fused stage against the one
composed from the existing applies, whole RK3 steps against the dense oracle, and the entries' argument errors."""
import numpy as np
import pytest

from tests.helpers import rel_l2
from tests.test_tsw_oracle import galewsky_state, tsw_sphere

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = -1, -2


def device_sphere(pn, ne, sparse=False):
    from mimsem_amd.device import DeviceMesh, Engine
    cs, topos, geoms, coords, O = tsw_sphere(pn, ne, sparse)
    dm = DeviceMesh(topos, geoms, nk=1, numbering="global")
    eng = Engine(dm)
    xq = np.zeros((dm.nq, 3))
    for g in geoms:
        xq[g.loc0] = coords[g.loc0]
    return eng, O, xq[dm.gidq]


def to_eng(eng, form, x):
    g = {1: eng.mesh.gid1, 2: eng.mesh.gid2}[form]
    return eng.tensor(np.asarray(x)[g])


def from_eng(eng, form, t):
    g = {1: eng.mesh.gid1, 2: eng.mesh.gid2}[form]
    out = np.zeros(g.size); out[g] = t.detach().cpu().numpy().ravel()
    return out


@pytest.mark.parametrize("pn", [2, 3, 4, 5])
def test_kernels_match_oracle(oracle, pn):
    """every output of the two kernels against the oracle's assembled matrices and direct solves (the sphere has det > 0 everywhere:
    tests/test_tsw_oracle.py::test_sphere_has_no_negative_determinant -- there is no negative-det geometry in the src flavour to test)"""
    eng, O, _ = device_sphere(pn, 2)
    assert (eng.mesh.det > 0).all()
    u, h, S = galewsky_state(O)
    r = np.random.default_rng(pn)
    u = u * (1 + 0.1 * r.standard_normal(u.size)); h = h * (1 + 1e-2 * r.standard_normal(h.size)); S = S * (1 + 1e-2 * r.standard_normal(S.size))
    m2inv = eng.element_matrices("WMATINV")
    s, Phi, h2 = eng.tsw_diagnose(to_eng(eng, 2, h), to_eng(eng, 2, S), to_eng(eng, 1, u), m2inv)
    s_ref = np.linalg.solve(O.M2h(h), O.M2 @ S)
    Phi_ref = O.K(u) @ u + 0.5 * (O.M2 @ S) + 0.25 * (O.M2h(s_ref) @ h)
    h2_ref = np.linalg.solve(O.M2, O.M2h(h) @ h)
    errs = dict(s=rel_l2(from_eng(eng, 2, s), s_ref), Phi=rel_l2(from_eng(eng, 2, Phi), Phi_ref), h2=rel_l2(from_eng(eng, 2, h2), h2_ref))
    # the update: F, G, grad s of the oracle's stage, (alpha, beta) of stage 2
    d = O.diagnose(u, h, S)
    hi, Si = h * (1 + 1e-3 * r.standard_normal(h.size)), S * (1 + 1e-3 * r.standard_normal(S.size))
    al, be, dt = 0.75, 0.25, 30.0
    hj_t, Sj_t = to_eng(eng, 2, h), to_eng(eng, 2, S)
    eng.tsw_update(to_eng(eng, 1, d["F"]), to_eng(eng, 1, d["G"]), to_eng(eng, 1, d["grad_s"]), to_eng(eng, 2, d["s"]), m2inv,
                   to_eng(eng, 2, hi), to_eng(eng, 2, Si), hj_t, Sj_t, al, be, dt)
    hj_ref = al * hi + be * (h - dt * (O.E21 @ d["F"]))
    Sj_ref = al * Si + be * S - be * dt * np.linalg.solve(O.M2, d["fS"])
    errs.update(hj=rel_l2(from_eng(eng, 2, hj_t), hj_ref), Sj=rel_l2(from_eng(eng, 2, Sj_t), Sj_ref))
    # fS through S_j: the increment alone (S_j - alpha S_i - beta S_j = -beta dt M2^-1 fS)
    dS = from_eng(eng, 2, Sj_t) - (al * Si + be * S)
    errs["fS"] = rel_l2(dS, -be * dt * np.linalg.solve(O.M2, d["fS"]))
    print("p=%d kernels vs oracle: " % pn + "  ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) < 1e-10, errs


@pytest.fixture(scope="module")
def ne2():
    from mimsem_amd.thermalsw import ThermalSW, galewsky_tsw
    import torch
    eng, O, xq = device_sphere(3, 2)
    T = ThermalSW(eng, xq)
    uq, hq, sq = galewsky_tsw(torch.as_tensor(xq, device=eng.device))
    return eng, O, xq, T, T.init(uq, hq, sq)


def test_fused_matches_composed(ne2):
    from mimsem_amd.thermalsw import ThermalSW
    eng, O, xq, T, (u, h, S) = ne2
    C = ThermalSW(eng, xq, fused=False)
    a, b = T.solve_rk(u, h, S, 30.0), C.solve_rk(u, h, S, 30.0)
    errs = [rel_l2(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a, b)]
    print("fused vs composed, one step: u %.1e  h %.1e  S %.1e" % tuple(errs))
    assert max(errs) < 1e-13


def test_missed_m1h_check_redoes_the_step_adaptively(ne2):
    """an M1h PCG forced to ONE iteration misses its true-residual check: the step is redone with the adaptive PCG and equals the step of an
    object that was adaptive from the start.  Tolerance: after the miss both objects run the same solvers (adaptive M1h PCG, the mass solver in
    its fixed-length mode) on the same state, so the 1e-13 this file asks between two device evaluations of one step is asked here too"""
    from mimsem_amd.thermalsw import ThermalSW
    eng, O, xq, T, (u, h, S) = ne2
    A, B = ThermalSW(eng, xq), ThermalSW(eng, xq)
    for t in (A, B):
        t.solve_M1(eng.apply("UTQ", eng.zeros(1, eng.sizes["q2"]) + 1.0))           # (the mass solver's one-time calibration, as init() triggers it)
        assert t.mass.verify(t.rtol) and t.mass.chebyshev
    A.m1h_its = 1
    B.m1h_its = 0
    a, b = A.solve_rk(u, h, S, 30.0), B.solve_rk(u, h, S, 30.0)
    assert A.redone == 1 and A.m1h_its == 0 and A.mass.chebyshev and A.mass.solves_missed == 0
    assert B.redone == 0 and B.mass.chebyshev
    errs = [rel_l2(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a, b)]
    print("redone after a missed M1h check vs adaptive from the start: u %.1e  h %.1e  S %.1e" % tuple(errs))
    assert max(errs) < 1e-13


def test_step_matches_dense_oracle(ne2):
    eng, O, xq, T, (u, h, S) = ne2
    uo, ho, So = galewsky_state(O)
    e0 = [rel_l2(from_eng(eng, 1, u), uo), rel_l2(from_eng(eng, 2, h), ho), rel_l2(from_eng(eng, 2, S), So)]
    a = T.solve_rk(u, h, S, 30.0)
    b = O.solve_rk(uo, ho, So, 30.0)
    errs = [rel_l2(from_eng(eng, f, x), y) for f, x, y in zip((1, 2, 2), a, b)]
    inv_d, inv_o = T.invariants(*a), O.invariants(*b)
    print("initial state vs oracle: u %.1e  h %.1e  S %.1e" % tuple(e0))
    print("one step vs dense oracle: u %.1e  h %.1e  S %.1e" % tuple(errs))
    print("invariants device / oracle: " + "  ".join("%s %.3e" % (k, (inv_d[k] - inv_o[k]) / max(abs(inv_o[k]), 1e-300)) for k in inv_o))
    assert max(e0) < 1e-10 and max(errs) < 1e-10
    for k in ("mass", "buoyancy", "energy", "entropy", "enstrophy"):
        assert abs(inv_d[k] - inv_o[k]) <= 1e-10 * abs(inv_o[k]), k


def test_ten_steps_ne4(oracle):
    import torch
    from mimsem_amd.thermalsw import ThermalSW, galewsky_tsw
    eng, O, xq = device_sphere(3, 4, sparse=True)
    T = ThermalSW(eng, xq)
    uq, hq, sq = galewsky_tsw(torch.as_tensor(xq, device=eng.device))
    x = T.init(uq, hq, sq)
    y = galewsky_state(O)
    for _ in range(10):
        x = T.solve_rk(*x, 30.0)
        y = O.solve_rk(*y, 30.0)
    errs = [rel_l2(from_eng(eng, f, a), b) for f, a, b in zip((1, 2, 2), x, y)]
    i0, i1 = O.invariants(*galewsky_state(O)), T.invariants(*x)
    print("10 steps ne=4 vs oracle: u %.1e  h %.1e  S %.1e   (%d steps redone)" % (*errs, T.redone))
    print("drift over 10 steps (device): " + "  ".join("%s %.2e" % (k, (i1[k] - i0[k]) / abs(i0[k])) for k in ("mass", "buoyancy", "energy", "entropy")))
    assert max(errs) < 1e-9
    assert abs(i1["mass"] - i0["mass"]) <= 1e-12 * abs(i0["mass"])


def test_argument_errors(ne2, oracle):
    eng, O, xq, T, (u, h, S) = ne2
    L, ctx = eng.L, eng.ctx
    ph, pu, pm = h.data_ptr(), u.data_ptr(), T.m2inv.data_ptr()
    o = [eng.zeros(eng.sizes[2]) for _ in range(3)]
    po = [t.data_ptr() for t in o]
    assert L.mimsem_tsw_diagnose(ctx, ph, ph, pu, pm, *po) == 0
    assert L.mimsem_tsw_diagnose(None, ph, ph, pu, pm, *po) == ERR_ARG
    assert L.mimsem_tsw_diagnose(ctx, None, ph, pu, pm, *po) == ERR_ARG
    assert L.mimsem_tsw_diagnose(ctx, ph, ph, pu, None, *po) == ERR_ARG
    assert L.mimsem_tsw_diagnose(ctx, ph, ph, pu, pm, po[0], None, po[2]) == ERR_ARG
    assert L.mimsem_tsw_update(ctx, pu, pu, pu, ph, pm, ph, ph, po[0], po[1], 0.0, 1.0, 30.0) == 0
    assert L.mimsem_tsw_update(ctx, pu, None, pu, ph, pm, ph, ph, po[0], po[1], 0.0, 1.0, 30.0) == ERR_ARG
    assert L.mimsem_tsw_update(None, pu, pu, pu, ph, pm, ph, ph, po[0], po[1], 0.0, 1.0, 30.0) == ERR_ARG
    eng.sync()
    # an engine with nk != 1, and an order without a built kernel
    from mimsem_amd.device import DeviceMesh, Engine
    from tests.helpers import make_patch
    cs, topo, geom, P, rng = make_patch(oracle, 3, 2, 6, 0, nk=2, seed=5)
    e2 = Engine(DeviceMesh([topo], [geom], nk=2, numbering="local"))
    x1, x2 = e2.zeros(e2.sizes[1]), e2.zeros(e2.sizes[2])
    assert e2.L.mimsem_tsw_diagnose(e2.ctx, x2.data_ptr(), x2.data_ptr(), x1.data_ptr(), x2.data_ptr(), x2.data_ptr(), x2.data_ptr(), x2.data_ptr()) == ERR_ARG
    cs, topo, geom, P, rng = make_patch(oracle, 6, 2, 6, 0, nk=1, seed=5)
    e6 = Engine(DeviceMesh([topo], [geom], nk=1, numbering="local"))
    y1, y2 = e6.zeros(e6.sizes[1]), e6.zeros(e6.sizes[2])
    assert e6.L.mimsem_tsw_update(e6.ctx, y1.data_ptr(), y1.data_ptr(), y1.data_ptr(), y2.data_ptr(), y2.data_ptr(), y2.data_ptr(),
                                  y2.data_ptr(), y2.data_ptr(), y2.data_ptr(), 0.0, 1.0, 1.0) == ERR_UNSUPPORTED
    from mimsem_amd._lib import MimsemError
    with pytest.raises(MimsemError):
        eng.tsw_diagnose(h[0][:-1].contiguous(), S[0], u[0], T.m2inv)                # a short row is refused before the launch


def test_kernels_on_mirrored_geometry(oracle):
    """det < 0 everywhere (the sphere with the first column of J negated): the Whmat and Wmat blocks are negative definite for a positive
    physical depth, and the unpivoted LU of k_tsw_diagnose must still give what the engine's pivoted element inverses (WHMATINV) give"""
    import torch
    from mimsem_amd.device import DeviceMesh, Engine
    _, topos, geoms, coords, O = tsw_sphere(3, 2)
    dm = DeviceMesh(topos, geoms, nk=1, numbering="global")
    u0, h0, S0 = galewsky_state(O)
    dm.J = np.ascontiguousarray(dm.J.copy()); dm.J[..., 0] *= -1.0; dm.J[..., 2] *= -1.0
    dm.det = np.ascontiguousarray(-dm.det)
    eng = Engine(dm)
    assert (eng.mesh.det < 0).all()
    r = np.random.default_rng(7)
    # a physical state on the mirrored elements: 2-form DoFs carry det, so positive depth and buoyancy have negative DoFs
    h, S = to_eng(eng, 2, -h0)[None], to_eng(eng, 2, -S0)[None]
    u = to_eng(eng, 1, u0 * (1 + 0.1 * r.standard_normal(u0.size)))[None]
    Wh = eng.element_matrices("WHMAT", f=h[0]).view(eng.nEl, eng.n2e, eng.n2e)
    assert bool((torch.linalg.eigvalsh(Wh) < 0).all())                              # negative definite blocks
    m2inv = eng.element_matrices("WMATINV")
    s, Phi, h2 = eng.tsw_diagnose(h[0], S[0], u[0], m2inv)
    M2S = eng.apply("WMAT", S)
    s_ref = eng.apply("WHMATINV", M2S, f=h)
    Phi_ref = eng.apply("WTQUMAT", u, f=u) + 0.5 * M2S + 0.25 * eng.apply("WHMAT", h, f=s_ref)
    h2_ref = eng.blocks_apply(2, m2inv.view(eng.nEl, eng.n2e, eng.n2e), eng.apply("WHMAT", h, f=h))
    F = to_eng(eng, 1, r.standard_normal(u0.size))[None]; G = to_eng(eng, 1, r.standard_normal(u0.size))[None]
    gs = to_eng(eng, 1, r.standard_normal(u0.size))[None]
    hi, Si = h * 1.001, S * 0.999
    hj, Sj = h.clone(), S.clone()
    eng.tsw_update(F[0], G[0], gs[0], s_ref[0], m2inv, hi[0], Si[0], hj[0], Sj[0], 0.75, 0.25, 30.0)
    divF = eng.incidence("E21", F)
    fS = 0.5 * eng.apply("WMAT", eng.incidence("E21", G)) + 0.5 * eng.apply("WHMAT", divF, f=s_ref) + eng.apply("WTQUMAT", F, f=gs)
    hj_ref = 0.75 * hi + 0.25 * (h - 30.0 * divF)
    Sj_ref = 0.75 * Si + 0.25 * S - 0.25 * 30.0 * eng.blocks_apply(2, m2inv.view(eng.nEl, eng.n2e, eng.n2e), fS)
    c = lambda t: t.cpu().numpy()
    errs = dict(s=rel_l2(c(s), c(s_ref)), Phi=rel_l2(c(Phi), c(Phi_ref)), h2=rel_l2(c(h2), c(h2_ref)), hj=rel_l2(c(hj), c(hj_ref)),
                Sj=rel_l2(c(Sj), c(Sj_ref)))
    print("det < 0: kernels vs the engine's applies: " + "  ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) < 1e-10, errs


INVARIANTS = ("mass", "buoyancy", "energy", "enstrophy", "vorticity", "entropy")


def test_config3_step_matches_fixture(golden_dir):
    """one solve_rk(30 s) of the GalewskyTSW_2 state at config 3 (24x24x6, p = 3) against tests/golden/tsw_galewsky_p3_ne24.npz"""
    import os
    import torch
    from mimsem_amd.thermalsw import ThermalSW, galewsky_tsw
    from tests.helpers import sketch_rel_err
    z = np.load(os.path.join(golden_dir, "tsw_galewsky_p3_ne24.npz"))
    eng, O, xq = device_sphere(3, 24, sparse=True)
    T = ThermalSW(eng, xq)
    uq, hq, sq = galewsky_tsw(torch.as_tensor(xq, device=eng.device))
    x0 = T.init(uq, hq, sq)
    x1 = T.solve_rk(*x0, float(z["dt"]))
    errs = {}
    for name, form, a in zip(("u0", "h0", "S0", "u1", "h1", "S1"), (1, 2, 2, 1, 2, 2), (*x0, *x1)):
        y = from_eng(eng, form, a)
        errs[name] = max(sketch_rel_err(y, z[name + "_sketch"], float(z[name + "_norm"])),
                         abs(np.linalg.norm(y) - float(z[name + "_norm"])) / float(z[name + "_norm"]))
    inv = T.invariants(*x1)
    ierr = {k: abs(inv[k] - z["inv1"][i]) / abs(z["inv1"][i]) for i, k in enumerate(INVARIANTS) if k != "vorticity"}
    print("config 3 vs fixture: " + "  ".join("%s %.1e" % kv for kv in errs.items()))
    print("invariants after the step vs fixture: " + "  ".join("%s %.1e" % kv for kv in ierr.items())
          + "  vorticity %.2e (fixture %.2e: zero to round-off)" % (inv["vorticity"], z["inv1"][4]))
    assert max(errs.values()) < 1e-10, errs
    assert max(ierr.values()) <= 1e-12, ierr


def test_galewsky_200_steps_ne8(oracle):
    """200 steps at ne = 8: mass to round-off; energy, entropy and buoyancy drift held to twice the sparse oracle's drift over the first
    20 steps at the same size (the reference publishes no bound), both reported"""
    import torch
    from mimsem_amd.thermalsw import ThermalSW, galewsky_tsw
    eng, O, xq = device_sphere(3, 8, sparse=True)
    T = ThermalSW(eng, xq)
    uq, hq, sq = galewsky_tsw(torch.as_tensor(xq, device=eng.device))
    x = T.init(uq, hq, sq)
    y = galewsky_state(O)
    d0, o0 = T.invariants(*x), O.invariants(*y)
    for _ in range(20):
        x = T.solve_rk(*x, 30.0)
        y = O.solve_rk(*y, 30.0)
    d20, o20 = T.invariants(*x), O.invariants(*y)
    for _ in range(180):
        x = T.solve_rk(*x, 30.0)
    d200 = T.invariants(*x)
    rel = lambda a, b, k: (a[k] - b[k]) / abs(b[k])
    for k in ("mass", "buoyancy", "energy", "entropy"):
        print("%-9s drift: device 20 steps %+.3e  oracle 20 steps %+.3e  device 200 steps %+.3e" % (k, rel(d20, d0, k), rel(o20, o0, k), rel(d200, d0, k)))
    print("steps redone: %d" % T.redone)
    assert abs(rel(d200, d0, "mass")) <= 1e-12
    for k in ("buoyancy", "energy", "entropy"):
        assert abs(rel(d20, d0, k)) <= 2.0 * abs(rel(o20, o0, k)) + 1e-15, k
