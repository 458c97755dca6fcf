"""Euler's explicit horizontal momentum update with Held-Suarez friction (eul/Euler_2.cpp:1431-1456, :1477-1492) on the device:
MIMSEM_OP_UMAT_FRIC (M1 + M1ray(tau) in one element pass), mimsem_fric_chebyshev_solve through MassSolver.solve_fric, and the step's wiring
in HorizMomentum -- against the dense M1 + M1ray of the oracle's element matrices on a small cubed sphere (tests/hmomentum_case.py)."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import SCALE, rel_l2
from tests.hmomentum_case import K_F, NK, Sphere

pytestmark = pytest.mark.gpu
TOL = 1e-10
TAUS = (240.0, 1.0 / K_F)

_CASES = {}


def _case(oracle, pn):
    """sphere, engine and one set of exner rows per order, built once: rows 0..2 with sigma in [0.5, 1] per element, es = level 0's own field"""
    if pn not in _CASES:
        from mimsem_amd.device import Engine
        S = Sphere(oracle, pn)
        eng = Engine(S.dm)
        r = np.random.default_rng(97 + pn)
        rows, es = [], None
        for k in range(NK):
            ek, es = S.exner(r, k)
            rows.append(ek)
        _CASES[pn] = (S, eng, rows, es)
    return _CASES[pn]


def _dev(S, eng, rows, es):
    return eng.tensor(np.stack([S.to_device(f) for f in rows])), eng.tensor(S.to_device(es))


def _dense(S, k, tau, ek, es):
    return S.m1(k) + S.m1ray(k, tau, ek, es)


# ---- 1. the operator --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn", [2, 3, 4])
def test_umat_fric_matches_umat_plus_umat_ray(oracle, pn):
    from mimsem_amd._lib import FLAG_ACCUM
    S, eng, rows, es = _case(oracle, pn)
    tau = 240.0
    r = np.random.default_rng(5)
    x = r.standard_normal((NK, S.n1))
    ex, exs = _dev(S, eng, rows, es)
    A = [_dense(S, k, tau, rows[k], es) for k in range(NK)]
    for k in range(NK):
        assert np.abs(S.ray_elmats(k, tau, rows[k], es)).max() > 0                 # sigma > 0.7 somewhere on every level
    # all levels in one call
    got = eng.apply_fric(eng.tensor(x), ex, exs, tau, lev0=0, scale=SCALE).cpu().numpy()
    for k in range(NK):
        assert rel_l2(got[k], A[k] @ x[k]) < TOL, k
    # one level, not the first
    got2 = eng.apply_fric(eng.tensor(x[2:3]), ex[2:3], exs, tau, lev0=2, scale=SCALE).cpu().numpy()
    assert rel_l2(got2[0], A[2] @ x[2]) < TOL
    # accumulate
    y0 = r.standard_normal((NK, S.n1)) * np.abs(A[0] @ x[0]).mean()
    y = eng.tensor(y0)
    eng.apply_fric(eng.tensor(x), ex, exs, tau, lev0=0, scale=SCALE, flags=FLAG_ACCUM, out=y)
    for k in range(NK):
        assert rel_l2(y[k].cpu().numpy(), y0[k] + A[k] @ x[k]) < TOL, k
    # element matrices: the sum of the two oracle blocks
    for k in range(NK):
        gm = S._blocks(eng.element_matrices_fric(ex[k], exs, tau, lev=k, scale=SCALE).cpu().numpy())
        assert rel_l2(gm, S.m1_elmats(k) + S.ray_elmats(k, tau, rows[k], es)) < TOL, k


@pytest.mark.parametrize("pn", [2, 3, 4])
def test_umat_fric_without_friction_is_umat(oracle, pn):
    """a level whose sigma stays below 0.7 on every element (k_v = 0 at every point): the Umat apply, to round-off"""
    S, eng, rows, es = _case(oracle, pn)
    lev, tau = 1, 240.0
    ek, _ = S.exner(np.random.default_rng(11), lev, lo=0.5, hi=0.6)
    assert np.abs(S.ray_elmats(lev, tau, ek, es)).max() == 0.0
    x = eng.tensor(np.random.default_rng(6).standard_normal((1, S.n1)))
    got = eng.apply_fric(x, eng.tensor(S.to_device(ek)[None]), eng.tensor(S.to_device(es)), tau, lev0=lev, scale=SCALE)
    want = eng.apply("UMAT", x, lev0=lev, scale=SCALE, flags=1)
    assert rel_l2(got.cpu().numpy(), want.cpu().numpy()) < 1e-13


# ---- 2. the solve -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn", [3, 4])
def test_solve_fric_matches_dense_solve(oracle, pn):
    from mimsem_amd.krylov import MassSolver
    S, eng, rows, es = _case(oracle, pn)
    ex, exs = _dev(S, eng, rows, es)
    ms = MassSolver(eng, SCALE, True)
    b = np.random.default_rng(7).standard_normal((NK, S.n1)) * 1e9
    steps = {}
    for tau in TAUS:
        x, steps[tau] = ms.solve_fric(eng.tensor(b), tau, ex, exs)
        assert ms.chebyshev and steps[tau] == ms._cheb_fric[tau].steps == len(ms._cheb_fric[tau].coef)      # the fixed-length mode ran
        checked = ms.solves_checked
        assert ms.verify() and ms.solves_checked == checked + 1 and ms.solves_missed == 0
        for k in range(NK):
            ref = np.linalg.solve(_dense(S, k, tau, rows[k], es), b[k])
            err = rel_l2(x[k].cpu().numpy(), ref)
            print("p %d tau %g level %d: %d steps, error %.2e" % (pn, tau, k, steps[tau], err))
            assert err < TOL, (tau, k)
    assert steps[TAUS[1]] > steps[TAUS[0]]                                          # the interval rule at work


# ---- 3. degenerate cases --------------------------------------------------------------------------------------------------------------
def test_degenerate_cases(oracle):
    import torch
    from mimsem_amd.hmomentum import HorizMomentum
    from mimsem_amd.horizsolve import HorizSolve
    S, eng, rows, es = _case(oracle, 3)
    ex, exs = _dev(S, eng, rows, es)
    hz = HorizSolve(eng)
    ms = hz.m1
    r = np.random.default_rng(8)
    b = eng.tensor(r.standard_normal((NK, S.n1)) * 1e9)
    x0, _ = ms.solve(b)                                                             # (the one-time calibration of the step count happens here)
    x0, _ = ms.solve(b)
    # tau = 0, or no exner: MassSolver.solve, bit for bit -- through the class and through the C entry
    assert torch.equal(ms.solve_fric(b, 0.0, ex, exs)[0], x0)
    assert torch.equal(ms.solve_fric(b, 240.0, None, None)[0], x0)
    cm, coef = ms._blocks_cm, ms._cheb.coef
    want = eng.block_chebyshev_solve("UMAT", cm, b, coef, elem_scale=ms.escale, scale=SCALE, flags=1)
    assert torch.equal(eng.fric_chebyshev_solve(cm, b, coef, 0.0, ex, exs, elem_scale=ms.escale, scale=SCALE), want)
    assert torch.equal(eng.fric_chebyshev_solve(cm, b, coef, 240.0, None, None, elem_scale=ms.escale, scale=SCALE), want)
    # hs_forcing = False: MassSolver.solve of b = M1 u_a - c dt Fu
    dt = 120.0
    u_a = eng.tensor(r.standard_normal((NK, S.n1))); Fu = eng.tensor(r.standard_normal((NK, S.n1)) * 1e7)
    hm = HorizMomentum(eng, hz, dt, hs_forcing=False)
    rhs = eng.combine(Fu, -2.0 * dt)
    eng.apply("UMAT", u_a, lev0=0, scale=SCALE, flags=1 | 2, out=rhs)
    assert torch.equal(hm.update(u_a, Fu, 2.0, ex), ms.solve(rhs)[0])
    assert torch.equal(hm.update(u_a, Fu, 2.0), ms.solve(rhs)[0])
    for k in range(NK):
        assert rel_l2(rhs[k].cpu().numpy(), S.m1(k) @ u_a[k].cpu().numpy() - 2.0 * dt * Fu[k].cpu().numpy()) < TOL
    assert ms.verify()
    # one level; a level range that does not start at level 0
    tau = 240.0
    bn = b.cpu().numpy()
    x1, _ = ms.solve_fric(b[0:1], tau, ex[0:1], exs)
    assert ms.verify()
    assert rel_l2(x1[0].cpu().numpy(), np.linalg.solve(_dense(S, 0, tau, rows[0], es), bn[0])) < TOL
    x12, _ = ms.solve_fric(b[1:], tau, ex[1:], exs, lev0=1)
    assert ms.verify() and ms.solves_missed == 0
    for k in (1, 2):
        assert rel_l2(x12[k - 1].cpu().numpy(), np.linalg.solve(_dense(S, k, tau, rows[k], es), bn[k])) < TOL, k
    with pytest.raises(Exception):
        eng.fric_chebyshev_solve(cm, b, coef, 240.0, ex, exs, elem_scale=ms.escale, scale=SCALE, flags=0)      # M1 + M1ray carries the thickness


# ---- 4. recorded ------------------------------------------------------------------------------------------------------------------------
def test_recorded_solve_fric_replays_the_eager_bits(oracle):
    import torch
    from mimsem_amd._lib import check
    from mimsem_amd.krylov import MassSolver
    S, eng, rows, es = _case(oracle, 3)
    ex, exs = _dev(S, eng, rows, es)
    L = eng.L
    ms = MassSolver(eng, SCALE, True)
    tau = 240.0
    b = eng.tensor(np.random.default_rng(9).standard_normal((NK, S.n1)) * 1e9)
    out = torch.full_like(b, float("nan"))
    ms.solve_fric(b, tau, ex, exs, out=out)                                       # the first call: spectral bounds, workspaces, the check log
    assert ms.verify()
    torch.cuda.synchronize()
    check(L.mimsem_ctx_use_own_stream(eng.ctx), "use_own_stream")
    try:
        ms.solve_fric(b, tau, ex, exs, out=out); eng.sync()
        want = out.clone()
        assert ms.verify() and bool(torch.isfinite(want).all())
        torch.cuda.synchronize()
        g = C.c_void_p()
        check(L.mimsem_graph_begin(eng.ctx), "graph_begin")
        ms.solve_fric(b, tau, ex, exs, out=out)
        check(L.mimsem_graph_end(eng.ctx, C.byref(g)), "graph_end")
        for _ in range(2):
            out.fill_(float("nan")); torch.cuda.synchronize()
            check(L.mimsem_graph_launch(g), "graph_launch"); eng.sync()
            assert torch.equal(out, want)
        assert ms.verify() and ms.solves_missed == 0                                # the replays wrote their check norms into the log
        L.mimsem_graph_destroy(g)
    finally:
        eng.use_stream(torch.cuda.current_stream(eng.device))


# ---- 5. the step's wiring ------------------------------------------------------------------------------------------------------------------
def test_predictor_and_corrector_against_the_reference_lines(oracle):
    from mimsem_amd.hmomentum import HorizMomentum
    from mimsem_amd.horizsolve import HorizSolve
    S, eng, rows, es = _case(oracle, 3)
    dt = 120.0
    r = np.random.default_rng(10)

    def field(seed):
        """an exner field of the step: row 0 is level 0 (sigma near 1: it is also exner_s), rows 1, 2 with sigma in [0.5, 1]"""
        rr = np.random.default_rng(seed)
        f1, f0 = S.exner(rr, 1)
        f2, _ = S.exner(rr, 2)
        return [f0, f1, f2]
    ex0, exh = field(21), field(22)
    dev = lambda F: eng.tensor(np.stack([S.to_device(f) for f in F]))
    velx, u_prev, velx_0 = (r.standard_normal((NK, S.n1)) for _ in range(3))
    Fu = np.stack([S.m1(k) @ r.standard_normal(S.n1) for k in range(NK)]) / dt          # dt Fu of the size of M1 u
    hm = HorizMomentum(eng, HorizSolve(eng), dt, hs_forcing=True)
    t = eng.tensor
    cases = (("predictor, first step", hm.predictor(t(velx), t(u_prev), t(Fu), dev(ex0), True), velx, 1.0, ex0),      # :1433-1438
             ("predictor", hm.predictor(t(velx), t(u_prev), t(Fu), dev(ex0), False), u_prev, 2.0, ex0),               # :1439-1445
             ("corrector", hm.corrector(t(velx_0), t(Fu), dev(exh)), velx_0, 1.0, exh))                               # :1477-1489
    assert hm.verify()
    for name, got, u_a, c, F in cases:
        for k in range(NK):
            A = _dense(S, k, c * dt, F[k], F[0])
            ref = np.linalg.solve(A, S.m1(k) @ u_a[k] - c * dt * Fu[k])
            assert rel_l2(got[k].cpu().numpy(), ref) < TOL, (name, k)
