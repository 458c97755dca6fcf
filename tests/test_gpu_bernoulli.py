"""mimsem_horiz_bernoulli (csrc/bernoulli.inc): HorizSolve::diagnose_Phi (eul/HorizSolve.cpp:419-470) for every level in one launch, through
Engine.bernoulli and HorizSolve(fused_phi=True), against HorizOracle.diagnose_Phi / the oracle's element matrices per level and against the
composed route (three WtQUmat applies, two interface averages, three Whmat applies).  Bar: relative L2 < 1e-10 per level, the bar
tests/test_gpu_next_rows.py::test_horizsolve_right_hand_sides sets for this quantity."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import energetics_case as ec
from tests import vort_diag_case as vc
from tests.euler_fused_cases import phi_from_element_matrices            # (moved there: shared with tests/test_gpu_euler_fused_orders.py)
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-10
MOMENTUM_TOL = 1e-10     # tests/test_gpu_next_rows.py (MOMENTUM_TOL): HorizSolve::momentum_rhs_ec per level, relative L2
SCALE = 1.0e8
ERR_ARG, ERR_UNSUPPORTED = -1, -2


def _engine(c, nk):
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.horizsolve import HorizSolve
    dm = DeviceMesh(c["topos"], c["geoms"], nk=nk, numbering="global")
    eng = Engine(dm)
    gd = c.get("gd")
    c["eng"] = eng
    c["hs"] = HorizSolve(eng, quad_coords=None if gd is None else gd.xq[dm.gidq])
    return c


def _fields(c, nk, seed):
    """u1, u2 [nk, N1] and velz1, velz2 [nk-1, N2] of a case (the second of each pair a 5 % perturbation of the first)"""
    r = np.random.default_rng(seed)
    F = c["F"]
    u1, z1 = F["u1"], F["velz1"]
    u2 = F["u2"] if "u2" in F else u1 * (1 + 0.05 * r.standard_normal(u1.shape))
    z2 = F["velz2"] if "velz2" in F else z1 * (1 + 0.05 * r.standard_normal(z1.shape))
    c["np"] = (u1, u2, z1, z2)
    c["t"] = tuple(c["eng"].tensor(a) for a in c["np"])
    return c


def _fused(c, *a):
    return c["eng"].bernoulli(*(a or c["t"]), scale=SCALE)


def _composed(c):
    hs = c["hs"]
    assert hs.fused_phi is False                     # the default: every existing caller keeps the composed route
    return hs.diagnose_Phi(*c["t"])


def _check(label, got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    want = want.cpu().numpy() if torch.is_tensor(want) else want
    errs = [rel_l2(got[k], want[k]) for k in range(want.shape[0])]
    print("%s: relative L2 per level  %s" % (label, "  ".join("%.2e" % e for e in errs)))
    assert np.all(np.isfinite(got)) and max(errs) < TOL, (label, errs)


@pytest.fixture(scope="module")
def sphere(oracle):
    """p = 3, ne = 2, nk = 3: 72 units of 16 lanes, 16 to a block -- the last block is partial"""
    c = _fields(_engine(vc.make_case(), vc.NK), vc.NK, 3)
    H = c["ho"].HorizOracle(c["gd"])
    u1, u2, z1, z2 = c["np"]
    c["H"], c["ref"] = H, np.stack([H.diagnose_Phi(k, u1[k], u2[k], z1, z2) for k in range(vc.NK)])
    return c


@pytest.fixture(scope="module")
def box(oracle):
    """p = 4, ne = 3, nk = 2 periodic box: 25 points on 32 lanes, and both levels are boundary levels (one interface each)"""
    c = ec.make_box_case(oracle)
    c = _fields(_engine(c, c["nk"]), c["nk"], 4)
    c["ref"] = phi_from_element_matrices(c, c["nk"])
    return c


def test_sphere_against_the_oracle_and_the_composed_route(sphere):
    got = _fused(sphere)
    _check("p3 sphere, kernel vs HorizOracle.diagnose_Phi", got, sphere["ref"])
    _check("p3 sphere, kernel vs composed route", got, _composed(sphere))


def test_p4_box_against_the_element_matrices_and_the_composed_route(box):
    got = _fused(box)
    _check("p4 box, kernel vs element matrices", got, box["ref"])
    _check("p4 box, kernel vs composed route", got, _composed(box))


def test_order_6_against_the_composed_route():
    """one element per lane group of 64 (49 points); no dense restatement at this order: the composed device route is the reference"""
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from tests.helpers import z_levels
    pn, nk = 6, 2
    cs = CubedSphere(pn, 1, 6); coords = sphere_coords(pn, 1)
    topos = [Topo(cs, p, nk) for p in range(6)]
    geoms = [Geom(t, cs, coords, nk) for t in topos]
    r = np.random.default_rng(5)
    levs = z_levels(nk, geoms[0].n0, r)
    for g in geoms:
        g.set_levels(levs)
    c = dict(topos=topos, geoms=geoms, F=dict(u1=r.standard_normal((nk, cs.nDofs1G)), velz1=r.standard_normal((nk - 1, cs.nDofs2G))))
    c = _fields(_engine(c, nk), nk, 6)
    _check("order 6, kernel vs composed route", _fused(c), _composed(c))


def test_same_bits_aliased_repeated_replayed_and_strided(sphere):
    eng = sphere["eng"]
    u1, u2, z1, z2 = sphere["t"]
    a = _fused(sphere)
    assert torch.equal(a, _fused(sphere))                                        # two calls
    # stage 1 of the step: velx1 is velx2, velz1 is velz2 -- the bits of the call on copies
    same = _fused(sphere, u1, u1, z1, z1)
    assert torch.equal(same, _fused(sphere, u1, u1.clone(), z1, z1.clone())) and not torch.equal(same, a)
    # recorded and replayed
    g, out = eng.capture(lambda: _fused(sphere))
    out.zero_()
    g.replay(); torch.cuda.synchronize()
    assert torch.equal(out, a)
    # rows 0, 2, 4 of a wider array, the rows between hold garbage; the output strided as well
    wide = []
    for x in sphere["t"]:
        big = torch.full((2 * x.shape[0], x.shape[1]), 1.0e30, dtype=torch.float64, device=x.device)
        big[::2] = x
        wide.append(big[::2])
        assert not wide[-1].is_contiguous() or x.shape[0] == 1
    assert torch.equal(_fused(sphere, *wide), a)
    obig = torch.full((2 * a.shape[0], a.shape[1]), -3.0, dtype=torch.float64, device=a.device)
    eng.bernoulli(*sphere["t"], scale=SCALE, out=obig[::2])
    assert torch.equal(obig[::2], a) and bool((obig[1::2] == -3.0).all())


def test_argument_errors_write_nothing(sphere):
    eng, nk = sphere["eng"], vc.NK
    fn = eng.L.mimsem_horiz_bernoulli
    u1, u2, z1, z2 = sphere["t"]
    out = torch.full((nk, eng.sizes[2]), 7.0, dtype=torch.float64, device=eng.device)
    p = dict(u1=u1, u2=u2, z1=z1, z2=z2, out=out)

    def call(ctx=eng.ctx, nk_=nk, ldu=u1.stride(0), ldz=z1.stride(0), ldo=out.stride(0), **null):
        q = {k: (None if k in null else C.c_void_p(v.data_ptr())) for k, v in p.items()}
        return fn(ctx, nk_, q["u1"], q["u2"], ldu, q["z1"], q["z2"], ldz, SCALE, q["out"], ldo)
    assert call(ctx=None) == ERR_ARG
    for k in p:
        assert call(**{k: True}) == ERR_ARG, k
    for bad in (1, 0, -1, nk + 1):
        assert call(nk_=bad) == ERR_ARG, bad
    assert call(ldu=-1) == ERR_ARG and call(ldz=-1) == ERR_ARG and call(ldo=-1) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))                           # the poisoned output stays poisoned
    # an order above 7 cannot reach the entry: no context of that order exists (its switch answers MIMSEM_ERR_UNSUPPORTED as
    # mimsem_ctx_create does)
    from mimsem_amd._lib import MeshDesc, MimsemError
    d = MeshDesc(); d.elOrd = d.quadOrd = 8; d.nEl = 1; d.nk = 2
    h = C.c_void_p()
    assert eng.L.mimsem_ctx_create(C.byref(d), 0, C.byref(h)) == ERR_UNSUPPORTED and not h.value
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, _fused(sphere))
    with pytest.raises(MimsemError):
        eng.bernoulli(u1, u2[:2], z1, z2)                                        # row counts differ: caught before the C call
    with pytest.raises(MimsemError):
        eng.bernoulli(u1[:1], u2[:1], z1[:0], z2[:0])                            # nk < 2


def test_momentum_rhs_with_the_fused_bernoulli(sphere):
    """HorizSolve.momentum_rhs_ec with fused_phi = True against HorizOracle.momentum_rhs_ec, per level"""
    from mimsem_amd.horizsolve import HorizSolve
    c, F, H, eng = sphere, sphere["F"], sphere["H"], sphere["eng"]
    nk, t = vc.NK, sphere["eng"].tensor
    hs = HorizSolve(eng, quad_coords=c["gd"].xq[eng.mesh.gidq])
    hs.fused_phi = True
    r = np.random.default_rng(11)
    dudz = r.standard_normal((nk - 1, c["gd"].N1)) * 1e-3 * F["ln"]; dudz2 = dudz * 1.1
    u1, u2, z1, z2 = c["np"]
    args = (F["th"], dudz, dudz2, z1, z2, F["Pi"], u1, u2, F["h1"], F["h2"])
    got = hs.momentum_rhs_ec(*[t(a) for a in args]).cpu().numpy()
    errs = []
    for k in range(nk):
        want = H.momentum_rhs_ec(k, F["th"][k], dudz, dudz2, z1, z2, F["Pi"][k], u1[k], u2[k], F["h1"][k], F["h2"][k])
        errs.append(rel_l2(got[k], want))
    print("momentum_rhs_ec with the fused Bernoulli vs oracle per level: %s" % " ".join("%.2e" % e for e in errs))
    assert max(errs) < MOMENTUM_TOL
    assert hs.verify()
