"""The reference's PCBJACOBI (PCBJacobiSetTotalBlocks(size*nElsX*nElsX), eul/HorizSolve.cpp:77-96, src/SWEqn_Picard.cpp:85-113) on the GPU:
exact inverses of the assembled diagonal blocks of the edges each element owns (mimsem_owned_blocks_*, mimsem_ksp_set_pc_bjacobi_owned,
mimsem_owned_block_chebyshev_solve) against the dense assembled matrices of the oracle (oracle/sw_oracle.py) and a numpy GMRES."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sphere(pn, ne=2, nk=1, seed=None):
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from mimsem_amd.workloads import z_levels
    cs = CubedSphere(pn, ne, 6); coords = sphere_coords(pn, ne)
    topos = [Topo(cs, p, nk) for p in range(6)]
    geoms = [Geom(t, cs, coords, nk, signed_det=True) for t in topos]
    rng = np.random.default_rng(seed)
    for g in geoms:
        g.set_levels(np.stack([np.zeros(g.n0), np.ones(g.n0)]) if seed is None else z_levels(nk, g.n0, rng))
    dm = DeviceMesh(topos, geoms, nk=nk, numbering="global")
    assert np.array_equal(dm.gid1, np.arange(cs.nDofs1G))
    return cs, topos, geoms, coords, dm, Engine(dm)


_CASES = {}


def _case(pn):
    """the p = pn, 2 x 2 x 6 sphere with the oracle's dense assembled M1 / M2 (src/ flavour: unit scale and thickness)"""
    if pn not in _CASES:
        from oracle import sw_oracle
        cs, topos, geoms, coords, dm, eng = _sphere(pn)
        O = sw_oracle.SWOracle(cs, topos, geoms, coords)
        _CASES[pn] = (eng, O)
    return _CASES[pn]


def _chunks(M, nd):
    return np.stack([M[k * nd:(k + 1) * nd, k * nd:(k + 1) * nd] for k in range(M.shape[0] // nd)])


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("pn", [2, 3, 4])
def test_owned_blocks_equal_assembled_chunks(pn):
    eng, O = _case(pn)
    nd = 2 * pn * pn
    B = eng.owned_blocks("UMAT")
    assert B.shape == (1, eng.nEl, nd, nd)
    assert _rel(B[0].cpu().numpy(), _chunks(np.asarray(O.M1), nd)) < 1e-13
    assert torch.equal(B, eng.owned_blocks("UMAT"))                      # fixed summation order: the same bits
    # Uhmat with a thickness field (a 2-form)
    h = 1.0 + 0.3 * np.random.default_rng(pn).random(O.N2)
    Bh = eng.owned_blocks("UHMAT", f=eng.tensor(h[None]))
    assert _rel(Bh[0].cpu().numpy(), _chunks(np.asarray(O._assemble1("UHMAT", h, 2)), nd)) < 1e-13
    assert torch.equal(Bh, eng.owned_blocks("UHMAT", f=eng.tensor(h[None])))
    # 2-forms: the element's own block
    B2 = eng.owned_blocks("WMAT")
    assert _rel(B2[0].cpu().numpy(), _chunks(np.asarray(O.M2), pn * pn)) < 1e-13


@pytest.mark.parametrize("pn", [2, 3, 4])
def test_owned_blocks_apply(pn):
    eng, O = _case(pn)
    nd, nlev = 2 * pn * pn, 3
    ref = np.linalg.inv(_chunks(np.asarray(O.M1), nd))                       # [nEl, nd, nd]
    Binv = eng.owned_blocks("UMAT", invert=True)[0].contiguous()
    x = np.random.default_rng(7).standard_normal((nlev, O.N1))
    want = np.einsum("kij,lkj->lki", ref, x.reshape(nlev, -1, nd)).reshape(nlev, -1)
    # one set of blocks for every level (blocks_level_stride = 0), output pre-filled with NaN: every slot is written
    y = torch.full((nlev, O.N1), float("nan"), dtype=torch.float64, device=eng.device)
    eng.owned_blocks_apply(1, Binv, eng.tensor(x), out=y)
    y = y.cpu().numpy()
    assert np.isfinite(y).all()
    for lev in range(nlev):
        assert np.linalg.norm(y[lev] - want[lev]) / np.linalg.norm(want[lev]) < 1e-12
    # a set per level
    B4 = torch.stack([(1.0 + lev) * Binv for lev in range(nlev)]).contiguous()
    y4 = torch.full((nlev, O.N1), float("nan"), dtype=torch.float64, device=eng.device)
    eng.owned_blocks_apply(1, B4, eng.tensor(x), out=y4)
    y4 = y4.cpu().numpy()
    assert np.isfinite(y4).all()
    for lev in range(nlev):
        assert np.linalg.norm(y4[lev] - (1.0 + lev) * want[lev]) / np.linalg.norm(want[lev]) < 1e-12


def _np_gmres(A, P, b, rtol, restart, maxit):
    """left-preconditioned restarted GMRES from x = 0 (classical Gram-Schmidt twice, Givens rotations): x and the history of
    |P r| / |P b| per iteration"""
    n = b.size
    x = np.zeros(n); pb = P @ b; bn = np.linalg.norm(pb); hist = []; its = 0
    while its < maxit:
        r = P @ (b - A @ x); beta = np.linalg.norm(r)
        if beta <= rtol * bn:
            break
        m = restart
        V = np.zeros((m + 1, n)); H = np.zeros((m + 1, m)); g = np.zeros(m + 1); cs = np.zeros(m); sn = np.zeros(m)
        V[0] = r / beta; g[0] = beta; kk = 0; done = False
        for j in range(m):
            w = P @ (A @ V[j])
            h = V[:j + 1] @ w; w = w - V[:j + 1].T @ h
            h2 = V[:j + 1] @ w; w = w - V[:j + 1].T @ h2; h = h + h2
            H[:j + 1, j] = h; H[j + 1, j] = np.linalg.norm(w); V[j + 1] = w / H[j + 1, j]
            for i in range(j):
                a_, b_ = H[i, j], H[i + 1, j]
                H[i, j], H[i + 1, j] = cs[i] * a_ + sn[i] * b_, -sn[i] * a_ + cs[i] * b_
            d = np.hypot(H[j, j], H[j + 1, j]); cs[j], sn[j] = H[j, j] / d, H[j + 1, j] / d
            H[j, j], H[j + 1, j] = d, 0.0
            g[j + 1], g[j] = -sn[j] * g[j], cs[j] * g[j]
            its += 1; kk = j + 1
            hist.append(abs(g[j + 1]) / bn)
            if abs(g[j + 1]) <= rtol * bn or its >= maxit:
                done = True; break
        y = np.linalg.solve(np.triu(H[:kk, :kk]), g[:kk])
        x = x + V[:kk].T @ y
        if done:
            break
    return x, hist


@pytest.mark.parametrize("pn", [2, 3, 4])
def test_ksp_gmres_owned_matches_dense_and_numpy_gmres(pn):
    from mimsem_amd.krylov import KSP
    eng, O = _case(pn)
    nd = 2 * pn * pn
    M1 = np.asarray(O.M1)
    b = np.random.default_rng(11).standard_normal(O.N1)
    xd = np.linalg.solve(M1, b)
    bt = eng.tensor(b[None])
    k = KSP(eng, "gmres").set_operator("UMAT", 1).set_pc("bjacobi_owned")
    k.set_tolerances(rtol=1e-15, atol=1e-50, maxit=500, restart=30)
    x = k.solve(bt).cpu().numpy()[0]
    assert np.linalg.norm(x - xd) / np.linalg.norm(xd) < 1e-12
    # the preconditioned residual history of the library's GMRES (its estimate after j iterations: maxit = j) against numpy's
    P = np.zeros_like(M1)
    inv = np.linalg.inv(_chunks(M1, nd))
    for kb in range(M1.shape[0] // nd):
        P[kb * nd:(kb + 1) * nd, kb * nd:(kb + 1) * nd] = inv[kb]
    rtol = 1e-12
    _, hist = _np_gmres(M1, P, b, rtol, 30, 500)
    k.set_tolerances(rtol=rtol, atol=1e-50, maxit=500, restart=30)
    k.solve(bt)
    assert k.iterations == len(hist), (k.iterations, len(hist))
    for j, h in enumerate(hist):
        if h <= 1e-12:
            break
        k.set_tolerances(rtol=rtol, atol=1e-50, maxit=j + 1, restart=30)
        k.solve(bt)
        assert abs(k.rnorm - h) <= 1e-8 * h, (j, k.rnorm, h)
    # the element-block preconditioner is a different one: a different count
    ke = KSP(eng, "gmres").set_operator("UMAT", 1).set_pc("bjacobi")
    ke.set_tolerances(rtol=rtol, atol=1e-50, maxit=500, restart=30)
    ke.solve(bt)
    print("GMRES iterations to 1e-12: owned blocks %d, element blocks %d" % (len(hist), ke.iterations))
    assert ke.iterations != len(hist)


def test_owned_chebyshev_mass_solve_config3():
    """the owned-block Chebyshev solve (coefficients from its Lanczos interval) on M1 of the config-3 sphere (p = 3, 24 x 24 x 6): it passes
    the MassSolver checks and agrees with the element-block Chebyshev solve"""
    from mimsem_amd.krylov import MassSolver
    *_, dm, eng = _sphere(3, ne=24)
    b = eng.tensor(np.random.default_rng(3).standard_normal((1, dm.n1)))
    own = MassSolver(eng, scale=1.0, vert_scale=False, precond="owned")
    x, steps = own.solve(b)
    assert own.chebyshev and own.verify()                              # one-time true-residual check and the logged check both hold
    res = float(torch.linalg.vector_norm(b - own.apply(x)) / torch.linalg.vector_norm(b))
    ref = MassSolver(eng, scale=1.0, vert_scale=False)
    xr, steps_ref = ref.solve(b)
    assert ref.chebyshev and ref.verify()
    err = float(torch.linalg.vector_norm(x - xr) / torch.linalg.vector_norm(xr))
    print("config 3 Chebyshev steps: owned %d (bound %s), element blocks %d; true residual %.2e, difference %.2e"
          % (steps, own.cheb_calibration.get("bound_steps"), steps_ref, res, err))
    assert res < 1e-11 and err < 1e-10


def test_owned_multilevel_horizsolve_like():
    """M1 with layer thickness on 4 levels (eul/HorizSolve.cpp's ksp1 solves): one set of owned blocks per level, solved by the KSP's CG and by
    the owned-block Chebyshev solve, against the element-block solver"""
    from mimsem_amd.krylov import KSP, MassSolver
    from mimsem_amd.workloads import SCALE
    nk = 4
    *_, dm, eng = _sphere(3, ne=2, nk=nk, seed=5)
    b = eng.tensor(np.random.default_rng(9).standard_normal((nk, dm.n1)))
    ref = MassSolver(eng, scale=SCALE, vert_scale=True)
    xr, _ = ref.solve(b)
    own = MassSolver(eng, scale=SCALE, vert_scale=True, precond="owned")
    assert own.blocks_owned.shape == (nk, eng.nEl, 18, 18)
    x, _ = own.solve(b)
    assert own.chebyshev and own.verify()
    for lev in range(nk):
        assert float(torch.linalg.vector_norm(x[lev] - xr[lev]) / torch.linalg.vector_norm(xr[lev])) < 1e-10
    k = KSP(eng, "cg").set_operator("UMAT", nk, scale=SCALE, flags=1).set_pc("bjacobi_owned")
    k.set_tolerances(rtol=1e-14, atol=1e-300, maxit=300)
    xc = k.solve(b)
    for lev in range(nk):
        assert float(torch.linalg.vector_norm(xc[lev] - xr[lev]) / torch.linalg.vector_norm(xr[lev])) < 1e-10


def test_owned_entry_errors():
    from mimsem_amd import _lib
    eng, O = _case(2)
    L = eng.L
    out = eng.zeros(1, eng.nEl * 64)
    assert L.mimsem_owned_blocks_build(eng.ctx, _lib.OPS["PMAT"], 0, 1, 1.0, 0, None, 0, out.data_ptr()) == -2        # 0-forms
    assert L.mimsem_owned_blocks_build(eng.ctx, _lib.OPS["ROTMAT"], 0, 1, 1.0, 0, None, 0, out.data_ptr()) == -1      # not a mass-like operator
    assert L.mimsem_owned_blocks_apply(eng.ctx, 0, 1, out.data_ptr(), 0, out.data_ptr(), 0, out.data_ptr(), 0) == -2
    from mimsem_amd.krylov import KSP
    k = KSP(eng, "gmres")
    assert L.mimsem_ksp_set_pc_bjacobi_owned(k.h) == -4                                                               # no operator yet
    k.set_operator("PMAT", 1)
    assert L.mimsem_ksp_set_pc_bjacobi_owned(k.h) == -2


_BIG = {}


def _big():
    """the config-4 sphere (p = 3, 24 x 24 x 6, 30 levels): 3 456 blocks of 18 rows, 8 per workgroup -- enough work items that a call with shared
    blocks keeps 2 (12 levels), 4 (16 levels) or 8 (30 levels) levels per work item"""
    if not _BIG:
        *_, dm, eng = _sphere(3, ne=24, nk=30, seed=13)
        _BIG["eng"] = eng
        _BIG["Binv"] = eng.owned_blocks("UMAT", invert=True)[0].contiguous()
    return _BIG["eng"], _BIG["Binv"]


@pytest.mark.parametrize("nlev", [12, 16, 30])
def test_owned_apply_several_levels_per_work_item(nlev):
    eng, Binv = _big()
    nd = Binv.shape[1]
    g = torch.Generator(device="cpu"); g.manual_seed(nlev)
    x = torch.randn(nlev, eng.sizes[1], generator=g, dtype=torch.float64).to(eng.device)
    y = torch.full_like(x, float("nan"))
    eng.owned_blocks_apply(1, Binv, x, out=y)                            # one set of blocks for every level: chunks of 2 / 4 / 8 levels
    assert bool(torch.isfinite(y).all())
    want = torch.einsum("kij,lkj->lki", Binv, x.view(nlev, -1, nd)).reshape(nlev, -1)      # chunk k = block k's rows (global numbering)
    err = torch.linalg.vector_norm(y - want, dim=1) / torch.linalg.vector_norm(want, dim=1)
    assert float(err.max()) < 1e-13
    # the same blocks once per level (one level per work item) give the same result
    y1 = torch.full_like(x, float("nan"))
    eng.owned_blocks_apply(1, Binv.expand(nlev, *Binv.shape).contiguous(), x, out=y1)
    assert float((torch.linalg.vector_norm(y1 - y, dim=1) / torch.linalg.vector_norm(y, dim=1)).max()) < 1e-14


@pytest.mark.parametrize("nlev", [12, 16])
def test_owned_chebyshev_several_levels_per_work_item(nlev):
    """the solve's first-step and later-step passes with chunks of levels (shared blocks) against one level per work item (per-level blocks)"""
    eng, Binv = _big()
    g = torch.Generator(device="cpu"); g.manual_seed(100 + nlev)
    b = torch.randn(nlev, eng.sizes[1], generator=g, dtype=torch.float64).to(eng.device)
    coef = [(1.2, 0.0)] + [(1.0, 0.05)] * 7
    pb, upd = torch.zeros_like(b), torch.zeros_like(b)
    x = eng.owned_block_chebyshev_solve(Binv, b, coef, pb=pb, upd=upd)
    pb1, upd1 = torch.zeros_like(b), torch.zeros_like(b)
    x1 = eng.owned_block_chebyshev_solve(Binv.expand(nlev, *Binv.shape).contiguous(), b, coef, pb=pb1, upd=upd1)
    for a, r in ((x, x1), (pb, pb1), (upd, upd1)):
        assert float((torch.linalg.vector_norm(a - r, dim=1) / torch.linalg.vector_norm(r, dim=1)).max()) < 1e-13


def test_owned_mass_solve_30_levels_shared_blocks():
    """MassSolver(precond="owned") without thickness on the 30 levels of the config-4 sphere: one set of blocks, chunks of 8 levels in every pass
    of the solve; it passes its checks and agrees with the element-block solver"""
    from mimsem_amd.krylov import MassSolver
    eng, _ = _big()
    b = eng.tensor(np.random.default_rng(17).standard_normal((eng.nk, eng.sizes[1])))
    own = MassSolver(eng, scale=1.0, vert_scale=False, precond="owned")
    assert own.blocks_owned.dim() == 3
    x, _ = own.solve(b)
    assert own.chebyshev and own.verify()
    ref = MassSolver(eng, scale=1.0, vert_scale=False)
    xr, _ = ref.solve(b)
    err = torch.linalg.vector_norm(x - xr, dim=1) / torch.linalg.vector_norm(xr, dim=1)
    assert float(err.max()) < 1e-10


def test_owned_python_paths_refuse_uncovered_slots():
    """a rank-local layout (one patch, ghosts on the east / north sides): the ghosts lie outside every block -- owned_blocks_apply leaves them
    zero when it allocates the output, MassSolver(precond="owned") refuses the layout as the C paths do"""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom
    from mimsem_amd.krylov import MassSolver
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    cs = CubedSphere(3, 4, 6); coords = sphere_coords(3, 4)
    t = Topo(cs, 0, 1); g = Geom(t, cs, coords, 1, signed_det=True)
    g.set_levels(np.stack([np.zeros(g.n0), np.ones(g.n0)]))
    eng = Engine(DeviceMesh([t], [g], nk=1, numbering="local"))
    assert not eng.owned_covers_all(1) and eng.owned_covers_all(2)
    Binv = eng.owned_blocks("UMAT", invert=True)[0].contiguous()
    y = eng.owned_blocks_apply(1, Binv, eng.tensor(np.ones((1, eng.sizes[1]))))
    n = 3
    l = np.arange(n * (n + 1))
    owned = np.unique(np.concatenate([t.all_inds1x_l()[:, l % (n + 1) < n], t.all_inds1y_l()[:, l // n < n]], axis=1))
    ghosts = np.setdiff1d(np.arange(eng.sizes[1]), owned)
    yc = y.cpu().numpy()[0]
    assert ghosts.size == 2 * t.nDofsX and (yc[ghosts] == 0.0).all() and np.isfinite(yc).all() and (yc[owned] != 0.0).any()
    with pytest.raises(ValueError):
        MassSolver(eng, scale=1.0, vert_scale=False, precond="owned")
