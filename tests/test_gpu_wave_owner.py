"""The owner-computes form of the headline operator (Umat at p = 3, k_apply_wave<3, UMAT, ..., OWN>): every store pair is
written finished by one owner wave-group, which computes the neighbour element's contribution across its ghost sides itself -- one launch,
no partial sums, no perimeter pass.  It must give the bits of today's two-launch form (MIMSEM_WAVE_OWN=0) for every level range, both
flags, the accumulate form and inputs that change from launch to launch; numberings it does not fit keep the two launches."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.helpers import SCALE, z_levels

pytestmark = pytest.mark.gpu


def _mesh(pn, ne, npatch, nk):
    from mimsem_amd.device import DeviceMesh
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    cs = CubedSphere(pn, ne, npatch); coords = sphere_coords(pn, ne)
    topos = [Topo(cs, p, nk) for p in range(npatch)]
    geoms = [Geom(t, cs, coords, nk) for t in topos]
    for g in geoms:
        g.set_levels(z_levels(nk, g.n0))
    return DeviceMesh(topos, geoms, nk=nk, numbering="global")


def _stats(eng, nk):
    st = (C.c_int * 5)()
    return eng.L.mimsem_op_wave_stats(eng.ctx, nk, st), list(st)


# the meshes of test_gpu_wave.py's fixture, and the benchmark sphere (config 4: p = 3, 24 x 24 x 6, 30 levels)
MESHES = [(2, 4, 6, 11), (3, 4, 6, 11), (4, 2, 6, 11), (3, 3, 6, 11), (2, 5, 6, 11), (3, 24, 24, 30)]


@pytest.fixture(scope="module", params=MESHES, ids=lambda m: "p%d_ne%d_nk%d" % (m[0], m[1], m[3]))
def pair(request):
    from mimsem_amd.device import Engine
    pn, ne, npatch, nk = request.param
    dm = _mesh(pn, ne, npatch, nk)
    own = Engine(dm)
    os.environ["MIMSEM_WAVE_OWN"] = "0"
    try:
        old = Engine(dm)
    finally:
        del os.environ["MIMSEM_WAVE_OWN"]
    return request.param, dm, own, old


def test_owner_computes_equals_two_launch_form(pair):
    import torch
    (pn, ne, npatch, nk), dm, own, old = pair
    r = np.random.default_rng(7)
    if nk <= 11:
        ranges = [(l0, n) for l0 in range(nk) for n in range(1, nk - l0 + 1)]      # every (lev0, nlev)
    else:
        ranges = [(0, nk), (0, 8), (0, 16), (1, 29), (3, 17), (7, 9), (12, 1), (nk - 1, 1), (5, 24)]
    for it in range(2):
        x = own.tensor(r.standard_normal((nk, dm.n1)) * (1.0 + it))
        for fl in (0, 1):
            for lev0, nl in ranges:
                a = own.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl)
                b = old.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl)
                assert torch.equal(a, b), (pn, ne, it, fl, lev0, nl, int((a != b).sum()))
            base = own.tensor(r.standard_normal((nk, dm.n1)))
            ya, yb = base.clone(), base.clone()
            own.apply("UMAT", x, lev0=0, scale=SCALE, flags=fl | 2, alpha=0.25, out=ya)
            old.apply("UMAT", x, lev0=0, scale=SCALE, flags=fl | 2, alpha=0.25, out=yb)
            assert torch.equal(ya, yb), (pn, ne, it, fl, "accumulate", int((ya != yb).sum()))
    # the other operators of the wave kernel keep their two-launch form in both contexts: same results
    h = own.tensor(r.uniform(0.5, 1.5, (nk, dm.n2)) * 1e6)
    x = own.tensor(r.standard_normal((nk, dm.n1)))
    assert torch.equal(own.apply("UHMAT", x, f=h, lev0=0, scale=SCALE, flags=1), old.apply("UHMAT", x, f=h, lev0=0, scale=SCALE, flags=1))


def test_owner_plan_invariants(pair):
    """Through the statistics bench.py prices the launch with: the new form writes every slot once, straight into y (each pair by its one
    owner), with no partial sum and no perimeter record; where it does not apply the two-launch numbers stay"""
    (pn, ne, npatch, nk), dm, own, old = pair
    ok, st = _stats(own, nk)
    ok0, st0 = _stats(old, nk)
    assert ok == 1 and ok0 == 1, (st, st0)
    assert st0[3] > 0 and st0[2] > 0, st0                       # today's form: perimeter records and partial sums
    assert st[0] == st0[0] and st[4] == st0[4]
    if_own = st[1] == dm.n1 and st[2] == 0 and st[3] == 0
    if pn == 3 and ne in (4, 24):
        assert if_own, (st, dm.n1)
    elif pn != 3:                                               # Umat at p = 3 only: the two launches, unchanged
        assert st == st0, (st, st0)
    else:                                                       # (a group that would need more than 4 ghost sides: the two launches)
        assert if_own or st == st0, (st, st0)


def test_benchmark_sphere_gets_owner_form_reference_local_layout_does_not():
    """Config 4's sphere (the bench.py workload) gets the new form; the reference's rank-local layout (no slot-pair plan at all) keeps
    the two-pass kernels, and its results do not depend on the switch"""
    import torch
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    dm = _mesh(3, 24, 24, 4)
    ok, st = _stats(Engine(dm), 4)
    assert ok == 1 and st[1] == dm.n1 and st[2] == 0 and st[3] == 0, st
    cs = CubedSphere(3, 8, 6); coords = sphere_coords(3, 8)
    t = Topo(cs, 2, 4)
    g = Geom(t, cs, coords, 4); g.set_levels(z_levels(4, g.n0))
    dml = DeviceMesh([t], [g], nk=4, numbering="local")
    ref = Engine(dml)
    assert _stats(ref, 4)[0] == 0
    os.environ["MIMSEM_WAVE_OWN"] = "0"
    try:
        ref0 = Engine(dml)
    finally:
        del os.environ["MIMSEM_WAVE_OWN"]
    x = ref.tensor(np.random.default_rng(3).standard_normal((4, dml.n1)))
    assert torch.equal(ref.apply("UMAT", x, lev0=0, scale=SCALE, flags=1), ref0.apply("UMAT", x, lev0=0, scale=SCALE, flags=1))
