"""Euler::HorizPotVort, HorizSolve::diagVertVort and Euler::VertMassFlux on the device (mimsem_amd/vortdiag.py) and the ABI entries under
them: mimsem_elem_block_pc_build_levels (csrc/elem_block_pc.inc) and mimsem_op_apply_levels (csrc/api.hip).  The case and the dense
restatement are tests/vort_diag_case.py (checked on the CPU by tests/test_vort_diag_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import vort_diag_case as vc

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = -1, -2
OP_UMAT, OP_WMAT, OP_UHMAT, OP_ROTMAT, OP_UTMAT_H = 0, 1, 2, 6, 9
SCALE, VERT = 1.0e8, 1
BLOCK_TOL = 1e-14        # tests/test_gpu_elem_block_pc.py::test_matches_bjacobi_and_python: largest relative Frobenius difference of a block
SOLVE_TOL = 1e-9         # tests/test_gpu_next_rows.py::test_horizsolve_right_hand_sides: the bar of the mass-solve outputs dF, dG
FZ_TOL = 1e-10           # tests/test_gpu_column.py::test_residual_compositions (TOL): its diagnose_F_z comparison
MOMENTUM_TOL = 1e-10     # tests/test_gpu_next_rows.py (MOMENTUM_TOL): HorizSolve::momentum_rhs_ec per level, relative L2


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def block_rel(a, b):
    """largest relative difference of one block (Frobenius norm per element block), as tests/test_gpu_elem_block_pc.py"""
    return float((np.linalg.norm((a - b).reshape(a.shape[0], -1), axis=1) / np.linalg.norm(b.reshape(b.shape[0], -1), axis=1)).max())


def order_6_engine():
    """one element per face at order 6 (no builder kernel), nk = 1, unit thickness"""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    cs = CubedSphere(6, 1, 6); coords = sphere_coords(6, 1)
    topos = [Topo(cs, p, 1) for p in range(6)]
    geoms = [Geom(t, cs, coords, 1, signed_det=True) for t in topos]
    for g in geoms:
        g.set_levels(np.stack([np.zeros(g.n0), np.ones(g.n0)]))
    return Engine(DeviceMesh(topos, geoms, nk=1, numbering="global"))


def engine_of(case):
    from mimsem_amd.device import DeviceMesh, Engine
    dm = DeviceMesh(case["topos"], case["geoms"], nk=vc.NK, numbering="global")
    return Engine(dm), dm


@pytest.fixture(scope="module")
def case(oracle):
    c = vc.make_case()
    c["eng"], c["dm"] = engine_of(c)
    c["t"] = {k: c["eng"].tensor(v) for k, v in c["F"].items() if isinstance(v, np.ndarray)}
    return c


@pytest.fixture(scope="module")
def two_pass(case):
    """a second engine on the same mesh whose operators take the two-pass form (element pass + gather): MIMSEM_WAVE=0 at its creation"""
    old = os.environ.get("MIMSEM_WAVE")
    os.environ["MIMSEM_WAVE"] = "0"
    try:
        eng, _ = engine_of(case)
    finally:
        if old is None:
            del os.environ["MIMSEM_WAVE"]
        else:
            os.environ["MIMSEM_WAVE"] = old
    return eng


@pytest.fixture(scope="module")
def dense(case):
    """the dense restatement's outputs, computed once"""
    gd, F = case["gd"], case["F"]
    d = {}
    d["uz1"], _ = vc.horiz_pot_vort(gd, F["u1"], F["h1"]); d["uz2"], _ = vc.horiz_pot_vort(gd, F["u2"], F["h2"])
    d["dw1"], _ = vc.vert_vort(gd, F["velz1"], F["h1"]); d["dw2"], _ = vc.vert_vort(gd, F["velz2"], F["h2"])
    d["Fz"] = vc.vert_mass_flux(gd, F["velz1"], F["velz2"], F["h1"], F["h2"])
    return d


@pytest.fixture(scope="module")
def run(case):
    """the device diagnoses, once: a first (adaptive, count-finding) call of each solve, then the fixed-length calls and ONE check()"""
    from mimsem_amd.horizsolve import HorizSolve
    from mimsem_amd.vortdiag import VortDiag
    eng, t = case["eng"], case["t"]
    hs = HorizSolve(eng, quad_coords=case["gd"].xq[case["dm"].gidq])
    vd = VortDiag(eng, hs)
    r = dict(hs=hs, vd=vd)
    r["uz_first"] = vd.horiz_pot_vort(t["u1"], t["h1"]); r["dw_first"] = vd.vert_vort(t["velz1"], t["h1"])
    r["fixed_first"], r["its_first"], r["m_its"] = dict(vd.fixed_its), dict(vd.its), vd.m_its
    r["uz1"] = vd.horiz_pot_vort(t["u1"], t["h1"]); r["fixed_uz"] = vd.fixed_its["uz"]
    r["dw1"] = vd.vert_vort(t["velz1"], t["h1"]); r["fixed_dw"] = vd.fixed_its["dwdx"]
    r["uz2"] = vd.horiz_pot_vort(t["u2"], t["h2"]); r["dw2"] = vd.vert_vort(t["velz2"], t["h2"])
    r["logged"] = vd.logged
    r["check"] = vd.check()
    r["Fz"] = vd.vert_mass_flux(t["velz1"], t["velz2"], t["h1"], t["h2"])
    return r


def rho_bar_dev(case):
    eng, t = case["eng"], case["t"]
    return eng.combine(t["h1"][:-1], 0.5, beta=0.5, c=t["h1"][1:])


# ---- 1. build_levels against the single-level builder ---------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["UMAT", "UHMAT"])
def test_build_levels_rows_are_the_single_level_blocks(case, op):
    eng = case["eng"]
    rb = rho_bar_dev(case)
    assert np.array_equal(rb.cpu().numpy(), vc.rho_bar_two_axpy(case["F"]["h1"]))      # 0.5 a + 0.5 b: the two-AXPY bits
    f = rb if op == "UHMAT" else None
    for lev0, step in ((0, 1), (1, 1), (0, 0), (1, 0)):
        got = eng.elem_block_pc_levels(op, 2, f=f, lev0=lev0, lev_step=step, scale=SCALE)
        assert got.shape == (2, eng.nEl, 2 * eng.n1e, 2 * eng.n1e) and bool(torch.isfinite(got).all())
        for r in range(2):
            want = eng.elem_block_pc(op, f=None if f is None else f[r], lev=lev0 + r * step, scale=SCALE)
            assert torch.equal(got[r], want), (op, lev0, step, r)
    if op == "UHMAT":       # (the thickness of level 1 differs from level 0's: a builder that ignored the step would be seen)
        a, b = eng.elem_block_pc_levels(op, 2, f=f, lev0=0, lev_step=1, scale=SCALE), eng.elem_block_pc_levels(op, 2, f=f, lev0=0, lev_step=0, scale=SCALE)
        assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])


# ---- 2. UTMAT_H ------------------------------------------------------------------------------------------------------------------------
def test_build_levels_utmat_h(case):
    from mimsem_amd.device import check
    from mimsem_amd.krylov import KSP
    eng, gd = case["eng"], case["gd"]
    rb = rho_bar_dev(case)
    rbn = rb.cpu().numpy()
    ni, nd, n1e = vc.NK - 1, 2 * eng.n1e, eng.n1e
    got = eng.elem_block_pc_levels("UTMAT_H", ni, f=rb, lev0=0, lev_step=1, scale=SCALE)
    gotn = got.cpu().numpy()
    idx = np.concatenate([eng.mesh.inds1x, eng.mesh.inds1y], axis=1)
    d = 1.0 / np.bincount(idx.ravel(), minlength=eng.sizes[1])[idx]                                 # D_e: 1 / (elements sharing the edge)
    for i in range(ni):
        ksp = KSP(eng, "cg").set_operator("UTMAT_H", 1, lev0=i, scale=SCALE, f=rb[i:i + 1])
        ksp.set_pc("bjacobi")
        ptr, esc, nd_ = ksp.pc_blocks()
        assert ptr and not esc and nd_ == nd
        ref = np.empty((eng.nEl, nd, nd))
        eng.sync()
        check(eng.L.mimsem_memcpy_d2h(eng.ctx, ref.ctypes.data, ptr, ref.nbytes), "d2h")
        eng.sync()
        same = bool(np.array_equal(gotn[i], ref))
        em = np.concatenate([P.op_elmats("UTMAT_H", i, SCALE, 0, gd.l2(t, rbn[i])) for t, P in zip(gd.topos, gd.P)]).reshape(eng.nEl, 2, 2, n1e, n1e)
        A = em.transpose(0, 1, 3, 2, 4).reshape(eng.nEl, nd, nd)
        want = d[:, :, None] * np.linalg.inv(A) * d[:, None, :]
        e_orc = block_rel(gotn[i], want)
        print("UTMAT_H interface %d: bit-equal to mimsem_ksp_set_pc_bjacobi: %s (%.1e)   vs D inv(A_e) D of the oracle: %.2e" % (i, same, block_rel(gotn[i], ref), e_orc))
        assert same
        assert e_orc <= BLOCK_TOL


# ---- 3. error paths -------------------------------------------------------------------------------------------------------------------
def test_build_levels_argument_errors(case):
    eng = case["eng"]
    L, nd = eng.L, 2 * eng.n1e
    rb = rho_bar_dev(case)
    out = torch.zeros(2, eng.nEl, nd, nd, dtype=torch.float64, device=eng.device)
    fp, op_, fs = C.c_void_p(rb.data_ptr()), C.c_void_p(out.data_ptr()), rb.stride(0)
    B = L.mimsem_elem_block_pc_build_levels
    assert B(eng.ctx, OP_WMAT, 0, 1, 2, SCALE, 0, None, 0, op_) == ERR_UNSUPPORTED         # a 2-form operator
    assert B(eng.ctx, OP_ROTMAT, 0, 1, 2, SCALE, 0, fp, fs, op_) == ERR_UNSUPPORTED
    assert B(eng.ctx, OP_UHMAT, 0, 1, 2, SCALE, 1, fp, fs, op_) == ERR_UNSUPPORTED         # thickness flag, as the single-level entry
    assert B(None, OP_UMAT, 0, 1, 2, SCALE, 0, None, 0, op_) == ERR_ARG
    assert B(eng.ctx, OP_UMAT, 0, 1, 2, SCALE, 0, None, 0, None) == ERR_ARG
    assert B(eng.ctx, OP_UTMAT_H, 0, 1, 2, SCALE, 0, None, 0, op_) == ERR_ARG              # without its density
    assert B(eng.ctx, OP_UHMAT, 0, 1, 2, SCALE, 0, None, 0, op_) == ERR_ARG
    assert B(eng.ctx, OP_UMAT, 2, 1, 2, SCALE, 0, None, 0, op_) == ERR_ARG                 # rows at levels 2, 3 of nk = 3
    assert B(eng.ctx, OP_UMAT, 3, 0, 2, SCALE, 0, None, 0, op_) == ERR_ARG                 # level 3 of nk = 3
    assert B(eng.ctx, OP_UMAT, -1, 1, 2, SCALE, 0, None, 0, op_) == ERR_ARG
    assert B(eng.ctx, OP_UMAT, 0, 2, 2, SCALE, 0, None, 0, op_) == ERR_ARG                 # a step other than 0 or 1
    assert B(eng.ctx, OP_UMAT, 0, -1, 2, SCALE, 0, None, 0, op_) == ERR_ARG
    assert B(eng.ctx, OP_UMAT, 0, 1, -1, SCALE, 0, None, 0, op_) == ERR_ARG
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                                                     # nothing written
    assert B(eng.ctx, OP_UMAT, 2, 0, 2, SCALE, 0, None, 0, op_) == 0                         # step 0 at the last level: in range
    e6 = order_6_engine()
    o6 = torch.zeros(1, e6.nEl, 2 * e6.n1e, 2 * e6.n1e, dtype=torch.float64, device=e6.device)
    assert e6.L.mimsem_elem_block_pc_build_levels(e6.ctx, OP_UMAT, 0, 1, 1, 1.0, 0, None, 0, C.c_void_p(o6.data_ptr())) == ERR_UNSUPPORTED
    # mimsem_op_apply_levels
    x = case["t"]["u1"]; y = torch.zeros_like(x)
    A = L.mimsem_op_apply_levels
    xp, yp = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    assert A(eng.ctx, OP_UMAT, 0, 0, 3, SCALE, 0, None, 0, xp, x.stride(0), yp, y.stride(0), 1.0) == ERR_UNSUPPORTED
    assert A(eng.ctx, OP_UMAT, 0, 2, 3, SCALE, 0, None, 0, xp, x.stride(0), yp, y.stride(0), 1.0) == ERR_ARG
    assert A(eng.ctx, OP_UHMAT, 3, 0, 3, SCALE, 0, fp, fs, xp, x.stride(0), yp, y.stride(0), 1.0) == ERR_ARG


# ---- 4. op_apply_levels ---------------------------------------------------------------------------------------------------------------
def test_op_apply_levels(case, two_pass):
    eng, t = case["eng"], case["t"]
    u, h = t["u1"], t["h1"]
    for op, x, f, flags in (("UMAT", u, None, VERT), ("WMAT", h, None, VERT), ("UHMAT", u, h, VERT), ("UHMAT", u, h, 0)):
        assert torch.equal(eng.apply_levels(op, x, 1, f=f, lev0=0, scale=SCALE, flags=flags), eng.apply(op, x, f=f, lev0=0, scale=SCALE, flags=flags)), op
    for op, x, f, flags in (("WMAT", h, None, VERT), ("UHMAT", u, h, 0)):
        y0 = eng.apply_levels(op, x, 0, f=f, lev0=0, scale=SCALE, flags=flags)
        assert y0.shape[0] == vc.NK and bool(torch.isfinite(y0).all())
        for r in range(vc.NK):
            fr = None if f is None else f[r:r + 1]
            one = two_pass.apply(op, x[r:r + 1], f=fr, lev0=0, scale=SCALE, flags=flags)            # one row, level 0, the two-pass form
            assert torch.equal(y0[r:r + 1], one), (op, r)
            dflt = eng.apply(op, x[r:r + 1], f=fr, lev0=0, scale=SCALE, flags=flags)                 # the engine's default form of the operator
            e = rel(y0[r].cpu().numpy(), dflt[0].cpu().numpy())
            print("%s step 0 row %d vs the default one-row apply at level 0: %.1e" % (op, r, e))
            if op == "WMAT":
                assert torch.equal(y0[r:r + 1], dflt)                                               # (k_elem_apply either way)
            assert e < 1e-13                                 # another order of the same ~16-term sums: a few units of 1.1e-16
            if r >= 1:                                       # the level is visible: the same row at its own level is another vector
                own = eng.apply(op, x[r:r + 1], f=fr, lev0=r, scale=SCALE, flags=flags)
                assert rel(y0[r].cpu().numpy(), own[0].cpu().numpy()) > 1e-3, (op, r)
        # a lev0 other than 0
        y1 = eng.apply_levels(op, x[:2], 0, f=None if f is None else f[:2], lev0=1, scale=SCALE, flags=flags)
        assert torch.equal(y1[1:2], two_pass.apply(op, x[1:2], f=None if f is None else f[1:2], lev0=1, scale=SCALE, flags=flags))


def test_blocks_apply_takes_a_block_set_per_row(case):
    """mimsem_elem_blocks_apply already has a level stride on `blocks` (the preconditioner of the batched solves): row r uses set r"""
    eng, t = case["eng"], case["t"]
    P = eng.elem_block_pc_levels("UTMAT_H", 2, f=rho_bar_dev(case), lev0=0, lev_step=1, scale=SCALE)
    x = t["u1"][:2].contiguous()
    y = eng.blocks_apply(1, P, x, transpose=True)
    for r in range(2):
        assert torch.equal(y[r:r + 1], eng.blocks_apply(1, P[r], x[r:r + 1], transpose=True))
    assert not torch.equal(y[1:2], eng.blocks_apply(1, P[0], x[1:2], transpose=True))


# ---- 5. the two solves against the dense restatement ----------------------------------------------------------------------------------
def test_solves_match_the_dense_restatement(case, run, dense):
    for name, got, want in (("uz(1)", run["uz1"], dense["uz1"]), ("uz(2)", run["uz2"], dense["uz2"]),
                            ("dwdx(1)", run["dw1"], dense["dw1"]), ("dwdx(2)", run["dw2"], dense["dw2"]),
                            ("uz first call", run["uz_first"], dense["uz1"]), ("dwdx first call", run["dw_first"], dense["dw1"])):
        g = got.cpu().numpy()
        errs = [rel(g[i], want[i]) for i in range(vc.NK - 1)]
        print("%-16s relative L2 error per interface: %s" % (name, " ".join("%.2e" % e for e in errs)))
        assert g.shape == want.shape and np.isfinite(g).all()
        assert max(errs) < SOLVE_TOL, name
    assert run["check"] is True


# ---- 6. the fixed-length path -----------------------------------------------------------------------------------------------------------
def test_fixed_length_path_and_its_check(case, run, dense):
    from mimsem_amd.vortdiag import VortDiag
    eng, t = case["eng"], case["t"]
    print("first calls: fixed_its %s iterations %s -> m_its %s; second calls launched with fixed_its uz %d dwdx %d; %d solves logged" %
          (run["fixed_first"], run["its_first"], run["m_its"], run["fixed_uz"], run["fixed_dw"], run["logged"]))
    assert run["fixed_first"] == {"uz": 0, "dwdx": 0}                        # the first call of each solve finds its count adaptively
    assert run["fixed_uz"] > 0 and run["fixed_dw"] > 0 and run["logged"] == 4
    assert run["check"] is True and run["vd"].missed == 0
    vd = VortDiag(eng, run["hs"])
    vd.m_its = 1                                                             # deliberately too short
    vd.horiz_pot_vort(t["u1"], t["h1"]); vd.vert_vort(t["velz1"], t["h1"])
    assert vd.fixed_its == {"uz": 1, "dwdx": 1}
    assert vd.check() is False and vd.m_its == 0 and vd.missed == 1
    uz, dw = vd.horiz_pot_vort(t["u1"], t["h1"]).cpu().numpy(), vd.vert_vort(t["velz1"], t["h1"]).cpu().numpy()      # the retry: adaptive
    assert vd.fixed_its == {"uz": 0, "dwdx": 0}
    errs = [rel(uz[i], dense["uz1"][i]) for i in range(vc.NK - 1)] + [rel(dw[i], dense["dw1"][i]) for i in range(vc.NK - 1)]
    print("retry after the missed check: %s" % " ".join("%.2e" % e for e in errs))
    assert max(errs) < SOLVE_TOL
    assert vd.check() is True


# ---- 7. vert_mass_flux ----------------------------------------------------------------------------------------------------------------
def test_vert_mass_flux(case, run, dense):
    got, want = run["Fz"].cpu().numpy(), dense["Fz"]
    assert got.shape == want.shape == (vc.NK - 1, case["gd"].N2)
    gd = case["gd"]
    worst = 0.0
    for t, P in zip(gd.topos, gd.P):                                         # column by column, in the oracle's vertical layout
        own = t.pi * t.n2 + np.arange(t.n2)
        pad = lambda a: P.horiz_to_vert(np.ascontiguousarray(np.vstack([a[:, own], np.zeros((1, t.n2))])))
        gv, wv = pad(got), pad(want)
        for e in range(P.nEl):
            worst = max(worst, rel(gv[e], wv[e]))
    print("vert_mass_flux vs the oracle's diagnose_F_z: worst column %.2e, whole field %.2e" % (worst, rel(got, want)))
    assert worst < FZ_TOL


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------------------
def test_momentum_rhs_ec_from_the_diagnoses(case, run, dense):
    t, F, hs = case["t"], case["F"], run["hs"]
    H = case["ho"].HorizOracle(case["gd"])
    got = hs.momentum_rhs_ec(t["th"], run["uz1"], run["uz2"], t["velz1"], t["velz2"], t["Pi"], t["u1"], t["u2"], t["h1"], t["h2"],
                             Fz=run["Fz"], dwdx1=run["dw1"], dwdx2=run["dw2"]).cpu().numpy()
    errs = []
    for lev in range(vc.NK):
        want = H.momentum_rhs_ec(lev, F["th"][lev], dense["uz1"], dense["uz2"], F["velz1"], F["velz2"], F["Pi"][lev], F["u1"][lev], F["u2"][lev],
                                 F["h1"][lev], F["h2"][lev], Fz=dense["Fz"], dwdx1=dense["dw1"], dwdx2=dense["dw2"])
        errs.append(rel(got[lev], want))
    print("momentum_rhs_ec fed the device diagnoses vs the oracle fed the dense ones, per level: %s" % " ".join("%.2e" % e for e in errs))
    assert max(errs) < MOMENTUM_TOL
    assert hs.verify()
