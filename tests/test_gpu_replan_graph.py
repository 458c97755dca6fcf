"""The retirement contract of the wave-level plan (mimsem_amd/csrc/api.hip: setup_wave, mimsem_ctx::alloc): a recording made through
mimsem_graph_* has the addresses of the plan's device tables baked into its kernel arguments.  mimsem_ctx_set_halo_slots builds a NEW plan;
the tables of the old one are retired -- the context stops naming them, its list of allocations keeps them until mimsem_ctx_destroy -- so
the old recording keeps computing what it computed, while eager applies run under the new plan.

Per order: record -> replay -> re-plan with marked slots -> scribble -> replay the OLD recording (same bits) -> eager under the new plan
(same bits: a 1-form slot has at most two contributors, as tests/test_gpu_halo_abi.py asserts for a re-planned apply) -> un-mark -> eager
(same bits) -> destroy the context under the live recording, then the recording."""
import ctypes as C

import numpy as np
import pytest

from mimsem_amd.workloads import SCALE, z_levels

pytestmark = pytest.mark.gpu

NK = 4


def _engine(pn):
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    cs = CubedSphere(pn, 2, 6); coords = sphere_coords(pn, 2)
    topos = [Topo(cs, p, NK) for p in range(6)]
    geoms = [Geom(t, cs, coords, NK) for t in topos]
    for g in geoms:
        g.set_levels(z_levels(NK, g.n0))
    dm = DeviceMesh(topos, geoms, nk=NK, numbering="global")
    return dm, Engine(dm)


@pytest.mark.parametrize("pn", [3, 2])
def test_old_recording_survives_a_new_wave_plan(pn):
    import torch
    from mimsem_amd._lib import check
    dm, eng = _engine(pn)
    L = eng.L
    st = (C.c_int * 5)()
    assert L.mimsem_op_wave_stats(eng.ctx, NK, st) == 1, "no wave-level plan: the test no longer tests anything"
    # p = 3: the owner-computes form (no perimeter slots); p = 2: the wave kernel with the perimeter pass
    assert (st[3] == 0) == (pn == 3), list(st)
    rng = np.random.default_rng(50 + pn)
    x = eng.tensor(rng.standard_normal((NK, dm.n1))); h = eng.tensor(rng.uniform(0.5, 1.5, (NK, dm.n2)) * 1e6)
    yu = eng.zeros(NK, dm.n1); yh = eng.zeros(NK, dm.n1)

    def seq():
        eng.apply("UMAT", x, lev0=0, scale=SCALE, flags=1, out=yu)
        eng.apply("UHMAT", x, f=h, lev0=0, scale=SCALE, flags=1, out=yh)
    # (1) record, (2) replay and keep
    check(L.mimsem_ctx_use_own_stream(eng.ctx), "use_own_stream")
    torch.cuda.synchronize()
    seq(); eng.sync()                                       # (workspaces reach their size outside the recording)
    g = C.c_void_p()
    check(L.mimsem_graph_begin(eng.ctx), "graph_begin"); seq(); check(L.mimsem_graph_end(eng.ctx, C.byref(g)), "graph_end")
    yu.zero_(); yh.zero_(); torch.cuda.synchronize()
    check(L.mimsem_graph_launch(g), "graph_launch"); eng.sync()
    want_u, want_h = yu.clone(), yh.clone()
    assert float(want_u.abs().max()) > 0 and float(want_h.abs().max()) > 0
    ws0 = L.mimsem_ctx_workspace_bytes(eng.ctx)
    # (3) a new plan: the old tables are retired, and stay counted
    marked = np.sort(rng.choice(dm.n1, 12, replace=False)).astype(np.int32)
    eng.set_halo_slots(1, marked)
    assert L.mimsem_ctx_workspace_bytes(eng.ctx) > ws0
    assert L.mimsem_op_wave_stats(eng.ctx, NK, st) == 1 and st[3] > 0, list(st)      # (a plan with a halo split has its perimeter pass)
    # (4) scribble, (5) the OLD recording
    yu.fill_(float("nan")); yh.fill_(float("nan")); torch.cuda.synchronize()
    check(L.mimsem_graph_launch(g), "graph_launch"); eng.sync()
    assert torch.equal(yu, want_u) and torch.equal(yh, want_h)
    # (6) eager under the new plan
    yu.fill_(float("nan")); yh.fill_(float("nan")); torch.cuda.synchronize()
    seq(); eng.sync()
    assert torch.equal(yu, want_u) and torch.equal(yh, want_h)
    # (7) un-marked: a third plan
    eng.set_halo_slots(1, np.zeros(0, np.int32))
    yu.fill_(float("nan")); yh.fill_(float("nan")); torch.cuda.synchronize()
    seq(); eng.sync()
    assert torch.equal(yu, want_u) and torch.equal(yh, want_h)
    # (8) the context goes first, its recording afterwards
    L.mimsem_ctx_destroy(eng.ctx); eng.ctx = C.c_void_p()
    assert L.mimsem_graph_launch(g) != 0, "a recording whose context is gone must refuse to launch"
    L.mimsem_graph_destroy(g)
