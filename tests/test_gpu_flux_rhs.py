"""mimsem_horiz_flux_rhs (csrc/flux_rhs.inc): the assembled mass-flux right-hand side sum_ab c_ab Uvec::assemble_hu(u_a, h_b) of
HorizSolve::diagnose_fluxes / momentum_rhs (eul/HorizSolve.cpp:298-306, :538-547) for every level in two launches, through Engine.flux_rhs,
against the four-term GlobalDense.uvec_hu sum / the point-wise restatement of tests/strang2_case.py per level and against the composed route
(HorizSolve._uvec_hu4: four accumulated Uhmat applies).  Bar: relative L2 < 1e-10 per level, the bar of tests/test_gpu_bernoulli.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import energetics_case as ec
from tests import strang2_case as s2c
from tests import vort_diag_case as vc
from tests.euler_fused_cases import flux_rhs_scattered                   # (moved there: shared with tests/test_gpu_euler_fused_orders.py)
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-10
SCALE = 1.0e8
ERR_ARG, ERR_UNSUPPORTED = -1, -2


def _engine(c, nk):
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.horizsolve import HorizSolve
    eng = Engine(DeviceMesh(c["topos"], c["geoms"], nk=nk, numbering="global"))
    c["eng"], c["hs"] = eng, HorizSolve(eng)
    return c


def _fields(c, seed):
    """u1, u2 [nk, N1] and h1, h2 [nk, N2] of a case (the second of each pair a perturbation of the first)"""
    r = np.random.default_rng(seed)
    F = c["F"]
    u1, h1 = F["u1"], F["h1"]
    u2 = F["u2"] if "u2" in F else u1 * (1 + 0.05 * r.standard_normal(u1.shape))
    h2 = F["h2"] if "h2" in F else h1 * (1 + 0.01 * r.standard_normal(h1.shape))
    c["np"] = (u1, u2, h1, h2)
    c["t"] = tuple(c["eng"].tensor(a) for a in c["np"])
    return c


def _fused(c, *a, **kw):
    return c["eng"].flux_rhs(*(a or c["t"]), scale=SCALE, **kw)


def _composed(c):
    assert c["hs"].fused_hu is False                 # the default: every existing caller keeps the composed route
    return c["hs"]._uvec_hu4(*c["t"])


def _check(label, got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    want = want.cpu().numpy() if torch.is_tensor(want) else want
    assert got.shape == want.shape
    errs = [rel_l2(got[k], want[k]) for k in range(want.shape[0])]
    print("%s: relative L2 per level  %s" % (label, "  ".join("%.2e" % e for e in errs)))
    assert np.all(np.isfinite(got)) and max(errs) < TOL, (label, errs)


@pytest.fixture(scope="module")
def sphere(oracle):
    """p = 3, ne = 2, nk = 3: 72 units of 16 lanes, 16 to a block -- the last block is partial"""
    c = _fields(_engine(vc.make_case(), vc.NK), 3)
    u1, u2, h1, h2 = c["np"]
    c["ref"] = np.stack([s2c.flux_rhs(c["gd"], k, u1[k], u2[k], h1[k], h2[k]) for k in range(vc.NK)])
    return c


@pytest.fixture(scope="module")
def box(oracle):
    """p = 4, ne = 3, nk = 2 periodic box: 25 points on 32 lanes, one patch whose edges wrap around"""
    c = ec.make_box_case(oracle)
    c = _fields(_engine(c, c["nk"]), 4)
    c["ref"] = flux_rhs_scattered(c, c["nk"], c["np"])
    return c


def test_sphere_against_the_uvec_hu_sum_and_the_composed_route(sphere):
    got = _fused(sphere)
    _check("p3 sphere, kernel vs sum of GlobalDense.uvec_hu", got, sphere["ref"])
    _check("p3 sphere, kernel vs composed route", got, _composed(sphere))


def test_p4_box_against_the_pointwise_restatement_and_the_composed_route(box):
    got = _fused(box)
    _check("p4 box, kernel vs point-wise restatement", got, box["ref"])
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
    c = dict(topos=topos, geoms=geoms, F=dict(u1=r.standard_normal((nk, cs.nDofs1G)), h1=r.uniform(0.8, 1.2, (nk, cs.nDofs2G))))
    c = _fields(_engine(c, nk), 6)
    _check("order 6, kernel vs composed route", _fused(c), _composed(c))


def test_one_level(sphere):
    """nk = 1: the first rows alone, as [1, n] and as [n]; the result is level 0 of the full call"""
    u1, u2, h1, h2 = sphere["t"]
    a = _fused(sphere)
    one = _fused(sphere, u1[:1], u2[:1], h1[:1], h2[:1])
    assert one.shape == (1, u1.shape[1]) and torch.equal(one[0], a[0])
    _check("nk = 1", one, sphere["ref"][:1])
    flat = _fused(sphere, u1[0], u2[0], h1[0], h2[0])
    assert torch.equal(flat.reshape(-1), a[0])


def test_same_bits_aliased_repeated_replayed_and_strided(sphere):
    eng = sphere["eng"]
    u1, u2, h1, h2 = sphere["t"]
    a = _fused(sphere)
    assert torch.equal(a, _fused(sphere))                                        # two calls
    # stage 1 of the step: u1 is u2, h1 is h2 -- the bits of the call on copies
    same = _fused(sphere, u1, u1, h1, h1)
    assert torch.equal(same, _fused(sphere, u1, u1.clone(), h1, h1.clone())) and not torch.equal(same, a)
    # recorded and replayed (the calls above have sized the workspace)
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
        assert not wide[-1].is_contiguous()
    assert torch.equal(_fused(sphere, *wide), a)
    obig = torch.full((2 * a.shape[0], a.shape[1]), -3.0, dtype=torch.float64, device=a.device)
    _fused(sphere, out=obig[::2])
    assert torch.equal(obig[::2], a) and bool((obig[1::2] == -3.0).all())


def test_argument_errors_write_nothing(sphere):
    eng, nk = sphere["eng"], vc.NK
    fn = eng.L.mimsem_horiz_flux_rhs
    u1, u2, h1, h2 = sphere["t"]
    out = torch.full((nk, eng.sizes[1]), 7.0, dtype=torch.float64, device=eng.device)
    p = dict(u1=u1, u2=u2, h1=h1, h2=h2, out=out)

    def call(ctx=eng.ctx, nk_=nk, ldu=u1.stride(0), ldh=h1.stride(0), ldo=out.stride(0), alias=None, **null):
        q = {k: (None if k in null else C.c_void_p(v.data_ptr())) for k, v in p.items()}
        if alias:
            q["out"] = q[alias]                                                  # (refused before anything is launched)
        return fn(ctx, nk_, q["u1"], q["u2"], ldu, q["h1"], q["h2"], ldh, SCALE, q["out"], ldo)
    assert call(ctx=None) == ERR_ARG
    for k in p:
        assert call(**{k: True}) == ERR_ARG, k
    for bad in (0, -1, nk + 1):
        assert call(nk_=bad) == ERR_ARG, bad
    assert call(ldu=-1) == ERR_ARG and call(ldh=-1) == ERR_ARG and call(ldo=-1) == ERR_ARG
    ins = [x.clone() for x in (u1, u2, h1, h2)]
    for k in ("u1", "u2", "h1", "h2"):
        assert call(alias=k) == ERR_ARG, k
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))                           # the poisoned output stays poisoned
    assert all(torch.equal(a, b) for a, b in zip(ins, (u1, u2, h1, h2)))         # and no input was taken for the output
    # an order above 7 cannot reach the entry: no context of that order exists
    from mimsem_amd._lib import MeshDesc, MimsemError
    d = MeshDesc(); d.elOrd = d.quadOrd = 8; d.nEl = 1; d.nk = 2
    h = C.c_void_p()
    assert eng.L.mimsem_ctx_create(C.byref(d), 0, C.byref(h)) == ERR_UNSUPPORTED and not h.value
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, _fused(sphere))
    poisoned = torch.full_like(out, 7.0)
    for bad in (lambda: eng.flux_rhs(u1, u2[:2], h1, h2, out=poisoned),                       # row counts differ
                lambda: eng.flux_rhs(u1, u2, h1[:, :-1], h2[:, :-1], out=poisoned),           # rows too short
                lambda: eng.flux_rhs(u1, u2, h1, h2.float(), out=poisoned),                   # dtype
                lambda: eng.flux_rhs(u1, u2, h1, None, out=poisoned),                         # a missing operand
                lambda: eng.flux_rhs(u1, u2, h1, h2, out=poisoned[:2]),                       # out too small
                lambda: eng.flux_rhs(u1, u2, h1, h2, out=u1)):                                # out is an input
        with pytest.raises(MimsemError):
            bad()
    torch.cuda.synchronize()
    assert torch.equal(poisoned, torch.full_like(out, 7.0))
