"""mimsem_elem_block_pc_build (csrc/elem_block_pc.inc): the element-block preconditioner D_e (A_e)^-1 D_e of UMAT / UHMAT(h) in one
capturable launch, against the blocks mimsem_ksp_set_pc_bjacobi builds (PCSetUp of ksp1h, src/ThermalSW_EEC_2.cpp:253-268), against the
Python composition of ThermalSW.solve_M1h, recorded and replayed with a changed depth field, and its argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = -1, -2
OP_UMAT, OP_WMAT, OP_UHMAT = 0, 1, 2


def sphere_engine(pn, ne):
    """the whole cubed sphere on one engine (global numbering, nk = 1, unit thickness) and the quadrature points in its numbering"""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    cs = CubedSphere(pn, ne, 6); coords = sphere_coords(pn, ne)
    topos = [Topo(cs, p, 1) for p in range(6)]
    geoms = [Geom(t, cs, coords, 1, signed_det=True) for t in topos]
    for g in geoms:
        g.set_levels(np.stack([np.zeros(g.n0), np.ones(g.n0)]))
    dm = DeviceMesh(topos, geoms, nk=1, numbering="global")
    eng = Engine(dm)
    xq = np.zeros((dm.nq, 3))
    for g in geoms:
        xq[g.loc0] = coords[g.loc0]
    return eng, xq[dm.gidq]


def galewsky_depth(eng, xq, seed):
    """the Galewsky depth as a 2-form (M2^-1 WtQ hq), times 1 + 1e-2 noise"""
    from mimsem_amd.sweqn import galewsky
    _, hq = galewsky(torch.as_tensor(xq, device=eng.device))
    m2inv = eng.element_matrices("WMATINV").view(eng.nEl, eng.n2e, eng.n2e)
    h = eng.blocks_apply(2, m2inv, eng.apply("WTQ", hq.reshape(1, -1).contiguous()))
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    return (h * (1.0 + 1e-2 * torch.randn(h.shape, generator=g, dtype=torch.float64).to(h.device))).contiguous()


def bjacobi_blocks(eng, op, h):
    """the blocks of mimsem_ksp_set_pc_bjacobi on the same operator, read back with mimsem_ksp_get_pc_blocks"""
    from mimsem_amd.device import check
    from mimsem_amd.krylov import KSP
    ksp = KSP(eng, "cg").set_operator(op, 1, f=h if op == "UHMAT" else None)
    ksp.set_pc("bjacobi")
    ptr, esc, nd = ksp.pc_blocks()
    assert ptr and not esc and nd == 2 * eng.n1e
    out = np.empty((eng.nEl, nd, nd))
    eng.sync()
    check(eng.L.mimsem_memcpy_d2h(eng.ctx, out.ctypes.data, ptr, out.nbytes), "d2h")
    eng.sync()
    return out


def python_blocks(eng, op, h):
    """ThermalSW.solve_M1h's composition: element matrices, permute, block_inverse, edge weights"""
    n1e = eng.n1e
    idx = torch.cat([torch.as_tensor(eng.mesh.inds1x, device=eng.device), torch.as_tensor(eng.mesh.inds1y, device=eng.device)], dim=1).long()
    mult = torch.zeros(eng.sizes[1], dtype=torch.float64, device=eng.device)
    mult.index_add_(0, idx.reshape(-1), torch.ones(idx.numel(), dtype=torch.float64, device=eng.device))
    d1 = 1.0 / mult[idx]
    em = eng.element_matrices(op, f=h[0] if op == "UHMAT" else None).view(eng.nEl, 2, 2, n1e, n1e)
    B = em.permute(0, 1, 3, 2, 4).reshape(eng.nEl, 2 * n1e, 2 * n1e)
    return (d1[:, :, None] * eng.block_inverse(B) * d1[:, None, :]).cpu().numpy()


def block_rel(a, b):
    """largest relative difference of one block (Frobenius norm per element block)"""
    return float((np.linalg.norm((a - b).reshape(a.shape[0], -1), axis=1) / np.linalg.norm(b.reshape(b.shape[0], -1), axis=1)).max())


@pytest.mark.parametrize("ne", [2, 4])
@pytest.mark.parametrize("pn", [2, 3, 4, 5])
def test_matches_bjacobi_and_python(pn, ne):
    eng, xq = sphere_engine(pn, ne)
    h = galewsky_depth(eng, xq, 7 * pn + ne)
    for op in ("UMAT", "UHMAT"):
        got = eng.elem_block_pc(op, f=h[0] if op == "UHMAT" else None).cpu().numpy()
        ref = bjacobi_blocks(eng, op, h)
        py = python_blocks(eng, op, h)
        e_ref, e_py = block_rel(got, ref), block_rel(got, py)
        same = bool(np.array_equal(got, ref))
        print("p=%d ne=%d %-5s  vs mimsem_ksp_set_pc_bjacobi: %.1e (bit-equal: %s)  vs Python composition: %.1e" % (pn, ne, op, e_ref, same, e_py))
        assert np.isfinite(got).all()
        assert e_ref <= 1e-14 and e_py <= 1e-14
        assert same, "the same operations in the same order as mimsem_ksp_set_pc_bjacobi: the same bits"


def test_recorded_build_follows_the_depth_field():
    """built inside mimsem_graph_begin / _end, h changed in place, the graph replayed: the blocks of the NEW h"""
    from mimsem_amd.device import check
    eng, xq = sphere_engine(3, 4)
    L = eng.L
    h = galewsky_depth(eng, xq, 1)
    h2 = galewsky_depth(eng, xq, 2)
    nd = 2 * eng.n1e
    out = torch.zeros(eng.nEl, nd, nd, dtype=torch.float64, device=eng.device)
    first = eng.elem_block_pc("UHMAT", f=h[0]).clone()          # (eager: the context makes its edge weights)
    eng.sync(); torch.cuda.synchronize()
    g = C.c_void_p()
    check(L.mimsem_graph_begin(eng.ctx), "graph_begin")
    rc = L.mimsem_elem_block_pc_build(eng.ctx, OP_UHMAT, 0, 1.0, 0, C.c_void_p(h.data_ptr()), C.c_void_p(out.data_ptr()))
    check(L.mimsem_graph_end(eng.ctx, C.byref(g)), "graph_end")
    check(rc, "mimsem_elem_block_pc_build (captured)")
    try:
        assert L.mimsem_graph_num_nodes(g) == 1
        torch.cuda.synchronize()
        assert float(out.abs().max()) == 0.0                    # (recording executes nothing)
        h.copy_(h2)
        torch.cuda.synchronize()
        check(L.mimsem_graph_launch(g), "graph_launch")
        torch.cuda.synchronize()
        want = eng.elem_block_pc("UHMAT", f=h2[0])
        torch.cuda.synchronize()
        got, want, first = out.cpu().numpy(), want.cpu().numpy(), first.cpu().numpy()
        print("replayed vs eager with the new h: max |diff| %.1e; vs the old h: %.1e" % (np.abs(got - want).max(), np.abs(got - first).max()))
        assert np.array_equal(got, want)
        assert not np.array_equal(got, first)
    finally:
        L.mimsem_graph_destroy(g)


def test_argument_errors():
    eng, xq = sphere_engine(3, 2)
    L = eng.L
    nd = 2 * eng.n1e
    h = galewsky_depth(eng, xq, 3)
    out = torch.zeros(eng.nEl, nd, nd, dtype=torch.float64, device=eng.device)
    hp, op_ = C.c_void_p(h.data_ptr()), C.c_void_p(out.data_ptr())
    assert L.mimsem_elem_block_pc_build(eng.ctx, OP_WMAT, 0, 1.0, 0, None, op_) == ERR_UNSUPPORTED
    assert L.mimsem_elem_block_pc_build(eng.ctx, 6, 0, 1.0, 0, hp, op_) == ERR_UNSUPPORTED          # ROTMAT
    assert L.mimsem_elem_block_pc_build(eng.ctx, OP_UHMAT, 0, 1.0, 1, hp, op_) == ERR_UNSUPPORTED   # thickness flag
    assert L.mimsem_elem_block_pc_build(eng.ctx, OP_UMAT, 0, 1.0, 2, None, op_) == ERR_UNSUPPORTED
    assert L.mimsem_elem_block_pc_build(None, OP_UMAT, 0, 1.0, 0, None, op_) == ERR_ARG
    assert L.mimsem_elem_block_pc_build(eng.ctx, OP_UMAT, 0, 1.0, 0, None, None) == ERR_ARG
    assert L.mimsem_elem_block_pc_build(eng.ctx, OP_UHMAT, 0, 1.0, 0, None, op_) == ERR_ARG        # UHMAT without its depth
    assert L.mimsem_elem_block_pc_build(eng.ctx, OP_UMAT, 1, 1.0, 0, None, op_) == ERR_ARG         # level outside nk = 1
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                                                             # nothing written
    for pn in (6, 7):                                                                                # orders without a built kernel
        e2, _ = sphere_engine(pn, 1)
        o2 = torch.zeros(e2.nEl, 2 * e2.n1e, 2 * e2.n1e, dtype=torch.float64, device=e2.device)
        assert e2.L.mimsem_elem_block_pc_build(e2.ctx, OP_UMAT, 0, 1.0, 0, None, C.c_void_p(o2.data_ptr())) == ERR_UNSUPPORTED
