""" "Next" rows (SURVEY 8(f) N1/N2 first pieces): device CG mass solve and the weak-form grad/curl built on it,
checked against a dense assembly of the oracle's element matrices on the whole (small) cubed sphere."""
import numpy as np
import pytest

from mimsem_amd.workloads import SCALE, z_levels

pytestmark = pytest.mark.gpu
MOMENTUM_TOL = 1e-10    # HorizSolve::momentum_rhs_ec per level, relative L2 (and the kinetic-to-internal exchange term)


@pytest.fixture(scope="module")
def sphere(oracle):
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    pn, ne, nk = 3, 2, 2
    cs = CubedSphere(pn, ne, 6); coords = sphere_coords(pn, ne)
    topos = [Topo(cs, p, nk) for p in range(6)]
    geoms = [Geom(t, cs, coords, nk) for t in topos]
    rng = np.random.default_rng(3)
    levs = z_levels(nk, geoms[0].n0)
    for g in geoms:
        g.set_levels(levs)
    eng = Engine(DeviceMesh(topos, geoms, nk=nk, numbering="global"))
    # oracle: global dense M1, M2 at every level from the per-patch element matrices
    mats = []
    for k in range(nk):
        M1 = np.zeros((cs.nDofs1G, cs.nDofs1G)); M2 = np.zeros((cs.nDofs2G, cs.nDofs2G))
        for t, g in zip(topos, geoms):
            P = oracle.Patch(pn, pn, cs.nel, nk)
            P.set_sphere_geometry(coords[cs.patches[t.pi].loc0]); P.set_levels(levs)
            em = P.op_elmats("UMAT", k, SCALE, 1).reshape(P.nEl, 4, P.n1e, P.n1e)
            gx, gy = t.all_inds1x_g(), t.all_inds1y_g()
            for e in range(P.nEl):
                for b, (r, c) in enumerate(((gx, gx), (gx, gy), (gy, gx), (gy, gy))):
                    M1[np.ix_(r[e], c[e])] += em[e, b]
            em2 = P.op_elmats("WMAT", k, SCALE, 1).reshape(P.nEl, P.n2e, P.n2e)
            g2 = t.all_inds2_g()
            for e in range(P.nEl):
                M2[np.ix_(g2[e], g2[e])] += em2[e]
        mats.append((M1, M2))
    return cs, eng, mats, rng


def test_device_cg_mass_solve(sphere):
    from mimsem_amd.krylov import MassSolver
    cs, eng, mats, rng = sphere
    ms = MassSolver(eng, SCALE, True)
    b = rng.standard_normal((eng.nk, cs.nDofs1G)) * 1e9
    x, its = ms.solve(eng.tensor(b), rtol=1e-15)
    assert its < 300
    for k, (M1, _) in enumerate(mats):
        ref = np.linalg.solve(M1, b[k])
        assert np.linalg.norm(x[k].cpu().numpy() - ref) / np.linalg.norm(ref) < 1e-10


def test_c_abi_ksp_mass_solves(sphere):
    """mimsem_ksp_* (csrc/ksp.hip): the CG and GMRES loops of the C ABI with the library-built PCBJACOBI-per-element preconditioner
    (mimsem_ksp_set_pc_bjacobi) on M1 u = b for all levels, against dense solves of the oracle-assembled matrices; the preconditioner
    the library builds equals MassSolver's; tolerances / iteration counts / reasons come back through mimsem_ksp_get_info"""
    import torch
    from mimsem_amd.krylov import KSP, MassSolver
    cs, eng, mats, rng = sphere
    b = rng.standard_normal((eng.nk, cs.nDofs1G)) * 1e9
    bt = eng.tensor(b)
    for kind, rtol in (("cg", 1e-15), ("gmres", 1e-15)):
        ksp = KSP(eng, kind).set_operator("UMAT", eng.nk, scale=SCALE, flags=1)
        ksp.set_pc("bjacobi").set_tolerances(rtol=rtol, atol=1e-300, maxit=400, restart=40)
        x = ksp.solve(bt)
        assert ksp.reason in ("rtol", "atol") and 0 < ksp.iterations < 200, (kind, ksp.reason, ksp.iterations)
        for k, (M1, _) in enumerate(mats):
            ref = np.linalg.solve(M1, b[k])
            assert np.linalg.norm(x[k].cpu().numpy() - ref) / np.linalg.norm(ref) < 1e-10, (kind, k)
    # no preconditioner: more iterations, the same solution; the iteration limit is reported, not hidden
    ksp = KSP(eng, "cg").set_operator("UMAT", eng.nk, scale=SCALE, flags=1)
    ksp.set_pc("none").set_tolerances(rtol=1e-14, atol=1e-300, maxit=3)
    ksp.solve(bt)
    assert ksp.reason == "diverged_its" and ksp.iterations == 3
    # MassSolver's PCG path runs through the same C loop (MIMSEM_PCG=c, the default) and agrees with its Python composition
    ms = MassSolver(eng, SCALE, True)
    ms.chebyshev = False
    x_c, its_c = ms.solve(bt, rtol=1e-15)
    import os
    os.environ["MIMSEM_PCG"] = "python"
    try:
        x_p, its_p = ms.solve(bt, rtol=1e-15)
    finally:
        del os.environ["MIMSEM_PCG"]
    assert abs(its_c - its_p) <= 2
    assert float(torch.linalg.vector_norm(x_c - x_p) / torch.linalg.vector_norm(x_p)) < 1e-12


def test_c_abi_ksp_ritz_and_pc_blocks(sphere):
    """mimsem_ksp_ritz (round 5): the Ritz values of P M1 after m Arnoldi steps inside the library against the eigenvalues of the dense
    P M1 -- P applied column by column through mimsem_elem_blocks_apply on the blocks mimsem_ksp_get_pc_blocks hands out.  Ritz values lie
    inside the spectrum's hull and reach its ends (that is what the fixed-length Chebyshev solves of the C++ hosts rely on)."""
    import ctypes as C
    import torch
    from mimsem_amd.krylov import KSP
    cs, eng, mats, rng = sphere
    n1 = cs.nDofs1G
    ksp = KSP(eng, "cg").set_operator("UMAT", eng.nk, scale=SCALE, flags=1)
    ksp.set_pc("bjacobi")
    blocks, escale, nd = ksp.pc_blocks()
    assert blocks and escale and nd == 2 * eng.n1e                      # thickness flag + 1-forms: one inverse per element and a per-level factor
    # dense P per level: the preconditioner applied to the identity
    eye = torch.eye(n1, dtype=torch.float64, device=eng.device)
    lam = []
    for k, (M1, _) in enumerate(mats):
        Pk = np.zeros((n1, n1))
        for j0 in range(0, n1, 64):
            cols = eye[j0:j0 + 64].contiguous()                          # rows = unit vectors; one "level" each, all with the factors of level k
            out = torch.zeros_like(cols)
            for r in range(cols.shape[0]):
                rc = eng.L.mimsem_elem_blocks_apply(eng.ctx, 1, 1, 0, C.c_void_p(blocks), 0, C.c_void_p(escale + 8 * k * eng.nEl), eng.nEl,
                                                    C.c_void_p(cols[r].data_ptr()), n1, C.c_void_p(out[r].data_ptr()), n1, 1.0)
                assert rc == 0
            Pk[:, j0:j0 + 64] = out.cpu().numpy().T
        ev = np.linalg.eigvals(Pk @ M1)
        assert np.abs(ev.imag).max() < 1e-8 * np.abs(ev.real).max()       # P and M1 symmetric positive definite
        lam.append(ev.real)
    lam = np.concatenate(lam)
    lo, hi, im = ksp.ritz(25)
    assert im < 1e-6
    assert lam.min() * (1 - 1e-8) <= lo <= lam.min() * 1.10 and lam.max() * 0.95 <= hi <= lam.max() * (1 + 1e-8), (lo, hi, lam.min(), lam.max())
    # a non-symmetric case: the packed shallow-water operator under its coupled blocks has (nearly) real Ritz values in (0, 2)
    kA = KSP(eng, "gmres")
    with pytest.raises(Exception):
        kA.ritz(10)                                                       # no operator yet
    lo2, hi2, im2 = ksp.ritz(2)                                           # the shortest recurrence still gives values inside the hull
    assert lam.min() * (1 - 1e-8) <= lo2 <= hi2 <= lam.max() * (1 + 1e-8)


def test_chebyshev_mass_solver(sphere):
    """the default mass solver on one rank: fixed-length Chebyshev semi-iteration on the fused block sweep
    (mimsem_block_chebyshev_sweep) -- one sweep against its composition, the Lanczos spectral bounds, the solve against PCG"""
    import torch
    from mimsem_amd.krylov import MassSolver
    cs, eng, mats, rng = sphere
    ms = MassSolver(eng, SCALE, True)
    assert ms.chebyshev
    b = eng.tensor(rng.standard_normal((eng.nk, cs.nDofs1G)) * 1e9)
    x1, steps = ms.solve(b)
    ch = ms._cheb
    assert 0.3 < ch.lmin < 1.0 < ch.lmax < 2.5 and steps == ch.steps and 4 <= steps <= 30
    ms.chebyshev = False
    x2, its = ms.solve(b, rtol=1e-15)
    assert float(torch.linalg.vector_norm(x1 - x2) / torch.linalg.vector_norm(x2)) < 1e-12
    # one sweep: z = P (b - M1 x); p = z + beta p; x += alpha p
    x = eng.tensor(rng.standard_normal((eng.nk, cs.nDofs1G))); p = eng.tensor(rng.standard_normal((eng.nk, cs.nDofs1G)))
    z = ms.precond(b - ms.apply(x))
    pref = z + 0.37 * p; xref = x + 1.9 * pref
    upd = torch.zeros_like(x)
    eng.block_chebyshev_sweep("UMAT", ms.blocks.transpose(1, 2).contiguous(), x, b, p, 1.9, 0.37, elem_scale=ms.escale,
                              scale=SCALE, flags=ms.flags, upd=upd)
    for got, want in ((upd, z), (p, pref), (x, xref)):
        assert float(torch.linalg.vector_norm(got - want) / torch.linalg.vector_norm(want)) < 1e-13


def test_chebyshev_whole_solve_equals_the_sweeps(sphere):
    """mimsem_block_chebyshev_solve (round 6: the whole fixed-length solve from x = 0 as one call, no element pass for the first step, x and
    p written rather than updated there) against the same steps as mimsem_block_chebyshev_sweep calls from x = 0: the same bits, for one
    step, two, an even and an odd count (the experiments build's two-launch form -- MIMSEM_CHEB_PEND=1 -- alternates the iterate between two
    buffers and must end in the caller's), with and without the check vectors; then through MassSolver (the default path of HorizSolve's
    mass solves) against PCG"""
    import torch
    from mimsem_amd.krylov import MassSolver
    cs, eng, mats, rng = sphere
    ms = MassSolver(eng, SCALE, True)
    cm = ms.blocks.transpose(1, 2).contiguous()
    b = eng.tensor(rng.standard_normal((eng.nk, cs.nDofs1G)) * 1e3)
    ms.solve(b)                                                             # (calibration, workspaces)
    ch = ms._cheb
    for n in (1, 2, 5, 8, len(ch.coef)):
        coef = ch.coef[:n]
        x = torch.zeros_like(b); p = torch.full_like(b, 7.0); u_last = torch.zeros_like(b); u_first = torch.zeros_like(b)
        for k, (al, be) in enumerate(coef):
            eng.block_chebyshev_sweep("UMAT", cm, x, b, p, al, be, elem_scale=ms.escale, scale=SCALE, flags=ms.flags,
                                      upd=u_first if k == 0 else (u_last if k == n - 1 else None))
        if n == 1:
            u_last = u_first
        pb = torch.full_like(b, float("nan")); upd = torch.full_like(b, float("nan")); y = torch.full_like(b, float("nan"))
        eng.block_chebyshev_solve("UMAT", cm, b, coef, x=y, elem_scale=ms.escale, scale=SCALE, flags=ms.flags, pb=pb, upd=upd)
        assert torch.equal(y, x), (n, float((y - x).abs().max()))
        assert torch.equal(pb, u_first) and torch.equal(upd, u_last), n
        y2 = eng.block_chebyshev_solve("UMAT", cm, b, coef, elem_scale=ms.escale, scale=SCALE, flags=ms.flags)      # no check vectors, own output
        assert torch.equal(y2, x)
    # a sub-range of levels, strided rows
    big = eng.tensor(rng.standard_normal((eng.nk, cs.nDofs1G + 5)))
    bb = big[1:, :cs.nDofs1G]
    x = torch.zeros(eng.nk - 1, cs.nDofs1G, dtype=torch.float64, device=eng.device); p = torch.zeros_like(x)
    for al, be in ch.coef[:4]:
        eng.block_chebyshev_sweep("UMAT", cm, x, bb, p, al, be, elem_scale=ms.escale[1:], lev0=1, scale=SCALE, flags=ms.flags)
    y = eng.block_chebyshev_solve("UMAT", cm, bb, ch.coef[:4], elem_scale=ms.escale[1:], lev0=1, scale=SCALE, flags=ms.flags)
    assert torch.equal(y, x)
    # the solver class uses it (one context) and agrees with PCG
    assert ch.whole is not None
    x1, _ = ms.solve(b)
    assert ms.verify()
    ms.chebyshev = False
    x2, _ = ms.solve(b, rtol=1e-15)
    assert float(torch.linalg.vector_norm(x1 - x2) / torch.linalg.vector_norm(x2)) < 1e-12
    import ctypes as C
    assert eng.L.mimsem_block_chebyshev_solve(eng.ctx, 2, 0, eng.nk, SCALE, 1, None, 0, C.c_void_p(cm.data_ptr()), None, 0, C.c_void_p(b.data_ptr()), b.stride(0),
                                              2, (C.c_double * 4)(1, 0, 1, 0), C.c_void_p(y.data_ptr()), y.stride(0), None, 0, None, 0) == -2      # only Umat


def test_rowdot_short_and_long_rows(sphere):
    """mimsem_krylov_rowdot: one launch for up to 8 rows (the last block of a row reduces it), two launches above; rows longer than 262 144 entries
    get more than 32 blocks (round 6).  Against float64 sums in extended order (torch) on every branch, and run-to-run identical bits."""
    import torch
    cs, eng, mats, rng = sphere
    for nrows, n in ((1, 1), (1, 1000), (2, 93312), (3, 262144), (2, 262145), (2, 1866240), (8, 300001), (9, 300001), (60, 62208), (70, 1500)):
        A = torch.randn(nrows, n, dtype=torch.float64, device=eng.device)
        B = torch.randn(nrows, n, dtype=torch.float64, device=eng.device)
        got = eng.rowdot(A, B)
        want = (A.double() * B).sum(dim=1)
        scale = (A.abs() * B.abs()).sum(dim=1)
        assert bool(((got - want).abs() <= 1e-14 * scale + 1e-300).all()), (nrows, n)
        for _ in range(3):
            assert torch.equal(eng.rowdot(A, B), got), (nrows, n)                       # (the arrival counters are left clean: every call the same)


def test_chebyshev_start_and_axpy_dots(sphere):
    """the two one-launch helpers around the [u|h] Chebyshev solve of a Picard iteration (round 6): mimsem_krylov_chebyshev_start (r = s c;
    d = r / theta; x = 0, also in place on c) and mimsem_krylov_axpy_dots (x += dx with both norms of the stopping test: the bits of the update
    followed by two rowdot calls)"""
    import torch
    cs, eng, mats, rng = sphere
    for nrows, n in ((1, 93312), (3, 1000), (1, 7)):
        c = torch.randn(nrows, n, dtype=torch.float64, device=eng.device)
        r, d, x = (torch.full_like(c, float("nan")) for _ in range(3))
        eng.chebyshev_start(c, -1.0, 0.77, r, d, x)
        assert torch.equal(r, -c) and torch.equal(d, (-c) * (1.0 / 0.77)) and not bool(x.any())
        c2 = c.clone()
        eng.chebyshev_start(c2, 1.0, 1.3, c2, d, x)                        # in place on c
        assert torch.equal(c2, c) and torch.equal(d, c * (1.0 / 1.3))
    # mimsem_krylov_chebyshev_px: the vector algebra of a Chebyshev step on a sharded mesh (z = dinv (b - y) or z = y; p = z + beta p; x += alpha p)
    for nrows, n in ((1, 5000), (3, 777)):
        y, b, dinv, p0, x0 = (torch.randn(nrows, n, dtype=torch.float64, device=eng.device) for _ in range(5))
        for diag in (False, True):
            p, x, upd = p0.clone(), x0.clone(), torch.full_like(x0, float("nan"))
            eng.chebyshev_px(0.8, 0.3, y, p, x, b=b if diag else None, dinv=dinv if diag else None, upd=upd)
            z = dinv * (b - y) if diag else y
            pn = torch.addcmul(z, p0, torch.tensor(0.3, dtype=torch.float64, device=eng.device))
            assert torch.equal(upd, z)
            assert float((p - pn).abs().max()) <= 1e-15 * float(pn.abs().max()) and float((x - (x0 + 0.8 * pn)).abs().max()) <= 1e-15 * float(x0.abs().max() + pn.abs().max())
    for n in (1, 1000, 93312, 300001, 1866240):
        dx = torch.randn(1, n, dtype=torch.float64, device=eng.device); x0 = torch.randn(1, n, dtype=torch.float64, device=eng.device)
        x = x0.clone(); out = torch.full((2,), float("nan"), dtype=torch.float64, device=eng.device)
        eng.axpy_dots(dx, x, out)
        want_x = x0 + dx
        assert torch.equal(x, want_x)
        assert torch.equal(out[0:1], eng.rowdot(dx, dx)) and torch.equal(out[1:2], eng.rowdot(want_x, want_x)), n
        x = x0.clone(); out2 = torch.zeros_like(out)
        eng.axpy_dots(dx, x, out2)
        assert torch.equal(out2, out)                                       # (the arrival counter is left clean)


def test_weak_gradient_matches_dense(sphere):
    from mimsem_amd.horizsolve import HorizSolve
    cs, eng, mats, rng = sphere
    hs = HorizSolve(eng)
    phi = rng.standard_normal((eng.nk, cs.nDofs2G))
    u = hs.grad(eng.tensor(phi)).cpu().numpy()
    E21 = np.zeros((cs.nDofs2G, cs.nDofs1G))
    e21 = eng.incidence("E21", eng.tensor(np.eye(cs.nDofs1G))).cpu().numpy()     # rows = unit vectors -> E21 columns
    E21[:] = e21.T
    for k, (M1, M2) in enumerate(mats):
        ref = np.linalg.solve(M1, -E21.T @ (M2 @ phi[k]))
        assert np.linalg.norm(u[k] - ref) / np.linalg.norm(ref) < 1e-9
    # mimetic identity on the whole sphere: E21 E10 = 0
    w = eng.incidence("E21", eng.incidence("E10", eng.tensor(rng.standard_normal((1, cs.nDofs0G)))))
    assert float(w.abs().max()) < 1e-12


def test_periodic_box_p4_global_apply(oracle):
    """BASELINE config 5 flavour: p=4 doubly periodic box (constant Jacobian, periodic wrap in the numbering), 4 patches on
    one GPU in global numbering; Umat / Wmat / WtQUmat applies vs a dense assembly of the oracle's element matrices"""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import BoxGeom
    from mimsem_amd.mesh import PeriodicBox, box_coords
    from mimsem_amd.topo import Topo
    pn, ne, npr, nk = 4, 4, 4, 2
    bx = PeriodicBox(pn, ne, npr); coords = box_coords(pn, ne, 1000.0)
    topos = [Topo(bx, p, nk) for p in range(npr)]
    geoms = [BoxGeom(t, bx, coords, nk, 1000.0) for t in topos]
    rng = np.random.default_rng(17)
    levs = z_levels(nk, geoms[0].n0, rng, ztop=1500.0)
    for g in geoms:
        g.set_levels(levs)                        # same level heights on every patch-local grid position
    eng = Engine(DeviceMesh(topos, geoms, nk=nk, numbering="global"))
    lev = 1
    M1 = np.zeros((bx.nDofs1G, bx.nDofs1G)); K = np.zeros((bx.nDofs2G, bx.nDofs1G))
    u1 = rng.standard_normal(bx.nDofs1G) * 10.0
    for t, g in zip(topos, geoms):
        P = oracle.Patch(pn, pn, bx.nel, nk)
        P.set_metric(g.det, g.J); P.set_levels(levs)
        gx, gy, g2 = t.all_inds1x_g(), t.all_inds1y_g(), t.all_inds2_g()
        em = P.op_elmats("UMAT", lev, SCALE, 1).reshape(P.nEl, 4, P.n1e, P.n1e)
        ul = np.zeros(P.n1); ul[t.all_inds1x_l().ravel()] = u1[gx.ravel()]; ul[t.all_inds1y_l().ravel()] = u1[gy.ravel()]
        ek = P.op_elmats("WTQUMAT", lev, SCALE, 0, ul).reshape(P.nEl, 2, P.n2e, P.n1e)
        for e in range(P.nEl):
            for b, (r, c) in enumerate(((gx, gx), (gx, gy), (gy, gx), (gy, gy))):
                M1[np.ix_(r[e], c[e])] += em[e, b]
            K[np.ix_(g2[e], gx[e])] += ek[e, 0]; K[np.ix_(g2[e], gy[e])] += ek[e, 1]
    x = rng.standard_normal(bx.nDofs1G)
    xt = eng.tensor(np.stack([x, x])); ut = eng.tensor(np.stack([u1, u1]))
    y = eng.apply("UMAT", xt, lev0=0, scale=SCALE, flags=1)[lev].cpu().numpy()
    assert np.linalg.norm(y - M1 @ x) / np.linalg.norm(M1 @ x) < 1e-10
    y2 = eng.apply("WTQUMAT", xt, f=ut, lev0=0, scale=SCALE)[lev].cpu().numpy()
    assert np.linalg.norm(y2 - K @ x) / np.linalg.norm(K @ x) < 1e-10


def test_krylov_mdot_maxpy(sphere):
    """the Gram-Schmidt building blocks of the device GMRES: h = V w and w += alpha V^T h, bitwise reproducible"""
    import torch
    cs, eng, mats, rng = sphere
    n, m = 93312, 31
    V = eng.tensor(rng.standard_normal((m, n))); w = eng.tensor(rng.standard_normal(n))
    for k in (1, 7, m):
        h = eng.mdot(V, w, k=k)
        ref = (V[:k].double() @ w)
        assert float((h - ref).abs().max() / ref.abs().max()) < 1e-13
        assert torch.equal(h, eng.mdot(V, w, k=k))
        w2 = w.clone(); eng.maxpy(V, h, w2, alpha=-0.5, k=k)
        ref2 = w - 0.5 * (h @ V[:k])
        assert float((w2 - ref2).abs().max()) < 1e-10 * float(ref2.abs().max())


def test_krylov_cgs2_three_launches(sphere):
    """mimsem_krylov_cgs2 (round 4: both Gram-Schmidt passes, normalisation and Hessenberg column in three launches -- the update of
    pass 1 and the dots of pass 2 share a kernel) against the four-launch composition orthogonalize + reorthonormalize_ex on an
    ORTHONORMAL basis (what Arnoldi hands it), bitwise reproducible, flag word down; sizes that are not multiples of its 512-entry blocks"""
    import torch
    cs, eng, mats, rng = sphere
    for n, m in ((93312, 31), (5003, 9)):
        Q, _ = torch.linalg.qr(eng.tensor(rng.standard_normal((n, m))))
        V = Q.T.contiguous()
        w0 = eng.tensor(rng.standard_normal(n))
        for k in (1, 6, m - 1):
            flag = torch.zeros(1, dtype=torch.int32).pin_memory()
            out = []
            for which in ("cgs2", "four", "cgs2"):
                w = w0.clone(); v = torch.empty_like(w)
                h1 = torch.zeros(m + 1, dtype=torch.float64, device=eng.device); h2 = torch.zeros_like(h1)
                col = torch.zeros(m + 2, dtype=torch.float64).pin_memory()
                if which == "cgs2":
                    eng.cgs2(V, w, v, k, h1, h2, col, m + 1, flag=flag)
                else:
                    eng.orthogonalize(V, w, h1, k=k)
                    eng.reorthonormalize(V, w, v, k, h1, h2, col, m + 1, fused=True, flag=flag)
                torch.cuda.synchronize()
                out.append((w.clone(), v.clone(), col.clone()))
            assert int(flag[0]) == 0
            (wa, va, ca), (wb, vb, cb), (wc, vc, cc) = out
            assert torch.equal(wa, wc) and torch.equal(va, vc) and torch.equal(ca, cc)                   # run-to-run bitwise
            scale = float(w0.abs().max())
            assert float((wa - wb).abs().max()) < 1e-13 * scale and float((va - vb).abs().max()) < 1e-12
            assert float((ca[:k] - cb[:k]).abs().max()) < 1e-12 * scale and abs(float(ca[m + 1] - cb[m + 1])) < 1e-12 * float(cb[m + 1])
            href = V[:k] @ w0
            assert float((ca[:k].to(eng.device) - href).abs().max()) < 1e-12 * scale
            assert float((V[:k] @ va).abs().max()) < 1e-14 and abs(float(torch.linalg.vector_norm(va)) - 1.0) < 1e-13


def test_krylov_fused_gram_schmidt_and_normalize(sphere):
    """mimsem_krylov_orthogonalize (h = V w, w -= V^T h in two launches) and mimsem_krylov_normalize (v = w/|w| plus the finished
    Hessenberg column written to device or pinned host memory) against torch, bitwise reproducible"""
    import torch
    cs, eng, mats, rng = sphere
    n, m = 93312, 61
    V = eng.tensor(rng.standard_normal((m, n))); w0 = eng.tensor(rng.standard_normal(n))
    for k in (1, 5, 60):
        w = w0.clone(); h = torch.zeros(m, dtype=torch.float64, device=eng.device)
        eng.orthogonalize(V, w, h, k=k)
        href = V[:k] @ w0
        assert float((h[:k] - href).abs().max() / href.abs().max()) < 1e-13
        wref = w0 - href @ V[:k]
        assert float((w - wref).abs().max()) < 1e-11 * float(wref.abs().max())
        wb = w0.clone(); hb = torch.zeros_like(h); eng.orthogonalize(V, wb, hb, k=k)
        assert torch.equal(w, wb) and torch.equal(h, hb)
        h2 = eng.tensor(rng.standard_normal(m))
        for col in (torch.zeros(m + 2, dtype=torch.float64, device=eng.device), torch.zeros(m + 2, dtype=torch.float64).pin_memory()):
            v = torch.empty_like(w)
            eng.normalize(w, v, k, h, h2, col, m + 1)
            torch.cuda.synchronize()
            nrm = float(torch.linalg.vector_norm(w))
            assert abs(float(col[m + 1]) - nrm) < 1e-13 * nrm
            assert float((v - w / col[m + 1].item()).abs().max()) < 1e-15 * float(v.abs().max())
            assert torch.equal(col[:k].to(eng.device), (h + h2)[:k])
            assert float(col[k:m + 1].abs().max()) == 0.0 if k < m + 1 else True


def test_horizsolve_right_hand_sides(oracle):
    """N2: HorizSolve::advection_rhs_ec / momentum_rhs_ec (eul/HorizSolve.cpp:380-417, 637-786) for all levels at once vs
    the dense restatement oracle/horiz_oracle.py (per-level dense matrices, LU for the KSP solves)"""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom
    from mimsem_amd.horizsolve import HorizSolve
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from oracle import horiz_oracle as ho
    pn, ne, nk = 3, 2, 3
    cs = CubedSphere(pn, ne, 6); coords = sphere_coords(pn, ne)
    topos = [Topo(cs, p, nk) for p in range(6)]
    geoms = [Geom(t, cs, coords, nk) for t in topos]
    levs = z_levels(nk, geoms[0].n0)
    for g in geoms:
        g.set_levels(levs)
    dm = DeviceMesh(topos, geoms, nk=nk, numbering="global")
    eng = Engine(dm)
    gd = ho.GlobalDense(cs, topos, geoms, coords, levs)
    H = ho.HorizOracle(gd)
    hs = HorizSolve(eng, quad_coords=gd.xq[dm.gidq])
    assert abs(hs.del2 - H.del2) < 1e-6 * abs(H.del2)
    assert np.linalg.norm(hs.fg.cpu().numpy() - H.fg) / np.linalg.norm(H.fg) < 1e-10
    r = np.random.default_rng(31)
    # physically scaled fields: 2-form dofs ~ value * area * thickness, 1-form dofs ~ value * edge length * thickness
    area = np.mean([P.det.mean() for P in gd.P]) * 4.0 / (pn * pn); dz = np.mean([P.thick.mean() for P in gd.P]); ln = np.sqrt(area)
    N1, N2 = gd.N1, gd.N2
    u1 = r.standard_normal((nk, N1)) * 20.0 * ln * dz; u2 = u1 * (1 + 0.05 * r.standard_normal((nk, N1)))
    h1 = r.uniform(0.8, 1.2, (nk, N2)) * area * dz; h2 = h1 * (1 + 0.01 * r.standard_normal((nk, N2)))
    th = r.uniform(290, 310, (nk, N2)) * area * dz; Pi = r.uniform(900, 1000, (nk, N2)) * area * dz
    velz = r.standard_normal((nk - 1, N2)) * area; velz2 = velz * (1 + 0.05 * r.standard_normal(velz.shape))
    dudz = r.standard_normal((nk - 1, N1)) * 1e-3 * ln; dudz2 = dudz * 1.1
    t = eng.tensor
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    dF, dG, Fk, Gk = H.advection_rhs_ec(u1, u2, h1, h2, th)
    gF, gG, gFk, gGk = hs.advection_rhs_ec(t(u1), t(u2), t(h1), t(h2), t(th))
    assert rel(gFk.cpu().numpy(), Fk) < 1e-10 and rel(gGk.cpu().numpy(), Gk) < 1e-10
    assert rel(gF.cpu().numpy(), dF) < 1e-9 and rel(gG.cpu().numpy(), dG) < 1e-9
    for lev in range(nk):
        assert rel(hs.diagnose_Phi(t(u1), t(u2), t(velz), t(velz2))[lev].cpu().numpy(), H.diagnose_Phi(lev, u1[lev], u2[lev], velz, velz2)) < 1e-10
        assert rel(hs.diagnose_q(t(h1), t(u1))[lev].cpu().numpy(), H.diagnose_q(lev, h1[lev], u1[lev])) < 1e-10
    dwdx = r.standard_normal((nk - 1, N1)) * 2e-4 * ln; dwdx2 = dwdx * 0.9          # horizontal gradient of the vertical velocity on the interfaces (:704-712)
    for kwargs in (dict(), dict(use_F=True), dict(use_F=True, dwdx=True)):
        Fx = Fk if kwargs.get("use_F") else None
        Fz = (velz * 0.7) if kwargs.get("use_F") else None
        w1, w2 = (dwdx, dwdx2) if kwargs.get("dwdx") else (None, None)
        got = hs.momentum_rhs_ec(t(th), t(dudz), t(dudz2), t(velz), t(velz2), t(Pi), t(u1), t(u2), t(h1), t(h2),
                                 Fx=None if Fx is None else t(Fx), Fz=None if Fz is None else t(Fz), Fk=t(Fk),
                                 dwdx1=None if w1 is None else t(w1), dwdx2=None if w2 is None else t(w2)).cpu().numpy()
        k2i, errs = 0.0, []
        for lev in range(nk):
            want, k = H.momentum_rhs_ec(lev, th[lev], dudz, dudz2, velz, velz2, Pi[lev], u1[lev], u2[lev], h1[lev], h2[lev],
                                        Fx=None if Fx is None else Fx[lev], Fz=Fz, Fk=Fk[lev], dwdx1=w1, dwdx2=w2)
            k2i += k
            errs.append(rel(got[lev], want))
        ek2i = abs(hs.k2i - k2i) / abs(k2i)
        print("momentum_rhs_ec %s vs oracle per level: %s  k2i %.2e" % (kwargs, " ".join("%.2e" % e for e in errs), ek2i))
        for lev, e in enumerate(errs):
            assert e < MOMENTUM_TOL, (lev, kwargs)
        assert ek2i < MOMENTUM_TOL
    # grad(theta) of advection_rhs_ec handed to momentum_rhs_ec (one mass solve less): the same bits as the call that solves it again
    again = hs.momentum_rhs_ec(t(th), t(dudz), t(dudz2), t(velz), t(velz2), t(Pi), t(u1), t(u2), t(h1), t(h2), Fx=t(Fk), Fz=t(velz * 0.7), Fk=t(Fk),
                               dwdx1=t(dwdx), dwdx2=t(dwdx2), dTheta=hs.dTheta).cpu().numpy()
    assert np.array_equal(again, got)
    # every fixed-length mass solve above logged its check norms on the device: one read, all met, none skipped
    assert hs.verify() and hs.m1.solves_missed == 0 and (hs.m1.solves_checked >= 15 or not hs.m1.chebyshev)


def test_krylov_batched_cg_kernels(sphere):
    """rowdot / cg_update / cg_direction: per-row scalars read from device memory, bitwise reproducible reductions"""
    import torch
    cs, eng, mats, rng = sphere
    nr, n = 5, 62208
    A, B = eng.tensor(rng.standard_normal((nr, n))), eng.tensor(rng.standard_normal((nr, n)))
    d = eng.rowdot(A, B)
    ref = (A * B).sum(dim=1)
    assert float(((d - ref) / ref.abs().max()).abs().max()) < 1e-13 and torch.equal(d, eng.rowdot(A, B))
    num, den = eng.tensor(rng.uniform(1, 2, nr)), eng.tensor(rng.uniform(1, 2, nr))
    x, r = A.clone(), B.clone(); p, Ap = eng.tensor(rng.standard_normal((nr, n))), eng.tensor(rng.standard_normal((nr, n)))
    eng.cg_update(num, den, p, Ap, x, r)
    al = (num / den)[:, None]
    assert torch.allclose(x, A + al * p, rtol=1e-13, atol=1e-13) and torch.allclose(r, B - al * Ap, rtol=1e-13, atol=1e-13)
    z = eng.tensor(rng.standard_normal((nr, n))); p2 = p.clone()
    eng.cg_direction(num, den, z, p2)
    assert torch.allclose(p2, z + al * p, rtol=1e-13, atol=1e-13)


def test_vertical_newton_loop_with_horizontal_transport():
    """VertSolve::solve_schur_eta with HorizSolve::advection_rhs_ec re-evaluated in every Newton iteration (eul/VertSolve.cpp:1798-1799)
    on a whole (small) sphere: a hydrostatic column state plus a weak horizontal wind -- the iteration contracts and stays finite;
    without wind the horizontal tendencies vanish identically"""
    import torch
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom, gll_points
    from mimsem_amd.horizsolve import HorizSolve
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from mimsem_amd.vertsolve import VertSolve
    pn, ne, nk = 3, 3, 8
    cs = CubedSphere(pn, ne, 6); coords = sphere_coords(pn, ne)
    topos = [Topo(cs, p, nk) for p in range(6)]
    geoms = [Geom(t, cs, coords, nk) for t in topos]
    for g in geoms:
        g.set_levels(z_levels(nk, g.n0))
    dm = DeviceMesh(topos, geoms, nk=nk, numbering="global")
    eng = Engine(dm)
    rng = np.random.default_rng(41)
    nEl, n2 = dm.nEl, eng.n2e
    wd = np.diff(gll_points(pn)); wj = np.outer(wd, wd).ravel()
    cell = dm.det.mean(axis=1)[:, None, None] * dm.thick.mean(axis=2).T[:, :, None] * wj[None, None, :]
    zl = np.mean([g.levs.mean(axis=1) for g in geoms], axis=0); zm = 0.5 * (zl[:-1] + zl[1:])
    th_v = 300.0 + 0.004 * zm
    pi_v = 1004.5 - (9.80616 / 0.004) * np.log(th_v / 300.0)
    rho_v = (1.0e5 / 287.0) * (pi_v / 1004.5) ** (717.5 / 287.0) / th_v
    colv = lambda v: eng.tensor((cell * v[None, :, None]).reshape(nEl, nk * n2))
    vs = VertSolve(eng, 30.0)
    levs = np.zeros((nk + 1, dm.nq))
    for g in geoms:
        levs[:, np.searchsorted(dm.gidq, g.loc0[np.arange(g.n0)])] = g.levs
    zv = vs.init_gz(levs)
    st = (eng.zeros(nEl, (nk - 1) * n2), colv(rho_v), colv(rho_v * th_v), colv(pi_v))
    hs = HorizSolve(eng)
    zero = eng.zeros(nk, dm.n1)
    f0 = vs.horiz_forcing_from(hs, zero, zero)(st[1], st[1], eng.diag_theta(0, st[1], st[2]))
    assert float(f0[0].abs().max()) == 0.0 and float(f0[1].abs().max()) == 0.0
    # a weak wind: a smooth 1-form = weak gradient of a smooth scalar, ~1 m/s
    xq = np.zeros((dm.nq, 3))
    for g in geoms:
        xq[g.loc0] = coords[g.loc0]
    phi_q = torch.as_tensor(xq[dm.gidq][:, 2] / 6371220.0, device=eng.device).repeat(nk, 1).contiguous()
    phi = eng.apply("WTQ", phi_q)                                     # sin(latitude), as a weak 2-form on every level
    velx = hs.grad(phi / float(phi.abs().max()) * float(st[1].abs().mean()) * 1e-6)
    forcing = vs.horiz_forcing_from(hs, velx, velx)
    out = vs.solve_schur_eta(*st, zv, horiz_forcing=forcing, maxit=4, tol=0.0)
    assert all(bool(torch.isfinite(o).all()) for o in out)
    h = vs.history
    assert h[-1]["exner"] < 0.2 * h[0]["exner"] and h[-1]["rho"] < h[0]["rho"] and h[-1]["exner"] < 1e-3, h


def test_c_abi_ksp_bjacobi_on_every_context_and_form(oracle):
    """round-4 advisor: (a) PCBJACOBI took the edge multiplicities from host copies only the wave-eligible contexts kept -- a p = 5 context
    or MIMSEM_WAVE=0 got MIMSEM_ERR_STATE; (b) a level window outside the context's levels reached the kernels unchecked; (c) 0- and 2-form
    operators (ksp0, ksp2 of the reference) were refused.  Each case: the call's return code and the solve against a dense solve."""
    import os
    import torch
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom
    from mimsem_amd.krylov import KSP
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo

    def build(pn, ne, nk, env=None):
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            cs = CubedSphere(pn, ne, 6); coords = sphere_coords(pn, ne)
            topos = [Topo(cs, p, nk) for p in range(6)]; geoms = [Geom(t, cs, coords, nk) for t in topos]
            levs = z_levels(nk, geoms[0].n0)
            for g in geoms:
                g.set_levels(levs)
            return cs, Engine(DeviceMesh(topos, geoms, nk=nk, numbering="global"))
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    def dense(eng, op, n, nlev, flags):
        """column j = the operator applied to e_j (per level)"""
        I = eng.tensor(np.eye(n))
        out = []
        for k in range(nlev):
            cols = [eng.apply(op, I[j:j + 1].contiguous(), lev0=k, scale=SCALE, flags=flags).cpu().numpy()[0] for j in range(n)]
            out.append(np.array(cols).T)
        return out

    rng = np.random.default_rng(12)
    for pn, ne, env in ((5, 1, None), (3, 2, {"MIMSEM_WAVE": "0"})):
        cs, eng = build(pn, ne, 2, env)
        b = rng.standard_normal((2, cs.nDofs1G)) * 1e9
        ksp = KSP(eng, "cg").set_operator("UMAT", 2, scale=SCALE, flags=1)
        ksp.set_pc("bjacobi").set_tolerances(rtol=1e-15, atol=1e-300, maxit=400)
        x = ksp.solve(eng.tensor(b)).cpu().numpy()
        assert ksp.reason in ("rtol", "atol"), (pn, ksp.reason)
        its_pc = ksp.iterations
        for k, A in enumerate(dense(eng, "UMAT", cs.nDofs1G, 2, 1)):
            ref = np.linalg.solve(A, b[k])
            assert np.linalg.norm(x[k] - ref) / np.linalg.norm(ref) < 1e-10, (pn, k)
        ksp = KSP(eng, "cg").set_operator("UMAT", 2, scale=SCALE, flags=1)
        ksp.set_pc("none").set_tolerances(rtol=1e-15, atol=1e-300, maxit=400)
        ksp.solve(eng.tensor(b))
        assert ksp.iterations > its_pc, (pn, its_pc, ksp.iterations)
        # the level window is checked where it is given
        L, h = eng.L, KSP(eng, "cg")
        from mimsem_amd.device import OPS
        assert L.mimsem_ksp_set_operator(h.h, OPS["UMAT"], 1, 2, SCALE, 1, None, 0) == -1          # levels 1..2 of 2: MIMSEM_ERR_ARG
        assert L.mimsem_ksp_set_operator(h.h, OPS["UMAT"], 1, 2, SCALE, 0, None, 0) == 0           # without the thickness factor no table is read
        assert L.mimsem_ksp_set_pc_bjacobi(h.h) == 0
        # 2-forms: block-diagonal mass matrix, the element blocks are its inverse; 0-forms: diagonal (collocated) mass matrix, likewise
        for op, n, flags, form in (("WMAT", cs.nDofs2G, 1, 2), ("PMAT", cs.nDofs0G, 0, 0)):
            bb = rng.standard_normal((1, n)) * 1e9
            ksp = KSP(eng, "gmres").set_operator(op, 1, lev0=1, scale=SCALE, flags=flags)
            ksp.set_pc("bjacobi").set_tolerances(rtol=1e-15, atol=1e-300, maxit=50)
            xx = ksp.solve(eng.tensor(bb)).cpu().numpy()
            assert ksp.iterations <= 2 and ksp.reason in ("rtol", "atol"), (op, ksp.iterations, ksp.reason)
            I = eng.tensor(np.eye(n))
            A = np.array([eng.apply(op, I[j:j + 1].contiguous(), lev0=1, scale=SCALE, flags=flags).cpu().numpy()[0] for j in range(n)]).T
            ref = np.linalg.solve(A, bb[0])
            assert np.linalg.norm(xx[0] - ref) / np.linalg.norm(ref) < 1e-10, op
        del eng
        torch.cuda.empty_cache()
