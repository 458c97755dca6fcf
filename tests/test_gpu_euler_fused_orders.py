"""The fused element kernels on the default path of the 3-D Euler step at EVERY order they are built for, against the CPU oracle:

    Engine.bernoulli            k_horiz_bernoulli<1..7>     (csrc/bernoulli.inc)
    Engine.flux_rhs             k_horiz_flux_rhs<1..7>      (csrc/flux_rhs.inc) and the 1-form gather
    Energetics.horizontal       k_energetics_horiz<1..7>    (csrc/energetics.inc)
    Engine.energetics_column    k_energetics_column<1..4>   (csrc/energetics.inc); orders 5 .. 7 answer MIMSEM_ERR_UNSUPPORTED

on the cases of tests/euler_fused_cases.py (checked on the CPU by tests/test_euler_fused_cases_cpu.py): a periodic box at every order 1 .. 7 and
a 3 x 3 sphere patch with a full Jacobian at orders 2 .. 7, 27 or 75 units of three levels -- full blocks and a partial last one in each of the
five lane layouts.  One more test sends k_energetics_horiz round its fixed-stride walk a second time.

Bars (none of them from what the device gives): relative L2 < 1e-10 per level and per (level, element) for the two vector results
(tests/test_gpu_bernoulli.py, tests/test_gpu_flux_rhs.py), plus, for the 1-form result, max |error| < 1e-10 max |value| per level;
|error| / S_abs <= 1e-10 for the sums (PARITY of tests/test_gpu_energetics.py).  The references agree among themselves to 1e-12."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import energetics_case as ec
from tests import euler_fused_cases as fc
from tests.test_gpu_energetics import route_two

pytestmark = pytest.mark.gpu
TOL = fc.TOL                 # relative L2, per level and per element
PARITY = 1e-10               # sums, relative to S_abs
SCALE = fc.SCALE
ERR_UNSUPPORTED = -2
EN_MAX_BLOCKS = 2048         # csrc/energetics.inc

BOXES_FUSED = [k for k in fc.CASES if k[0] == "box" and k[1] in fc.COLUMN_ORDERS]
BOXES_COMPOSED = [k for k in fc.CASES if k[0] == "box" and k[1] not in fc.COLUMN_ORDERS]


def _composed_host(eng):
    """HorizSolve's composed routes (diagnose_Phi with fused_phi = False, _uvec_hu4) without the 1-form mass solver its constructor builds:
    both are sequences of operator applies and read nothing else of the object"""
    from mimsem_amd.horizsolve import HorizSolve

    class ComposedOnly(HorizSolve):
        def __init__(self, eng):
            self.eng, self.nk, self.fused_phi, self.fused_hu = eng, eng.nk, False, False
    return ComposedOnly(eng)


def _build(c):
    """the engine of a case (the box in the global numbering, the patch in its local one), the hosts and the device copies of the inputs"""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.energetics import Energetics
    from mimsem_amd.vertsolve import VertSolve
    eng = Engine(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering=c["numbering"]))
    (t, g, P), = c["patches"]
    assert eng.nEl == c["nEl"] and eng.sizes[1] == c["velx"].shape[1] and eng.sizes[2] == c["rho"].shape[1]
    b = types.SimpleNamespace(c=c, eng=eng, hs=_composed_host(eng), en=Energetics(eng, VertSolve(eng, 0.0)), i2=t.all_inds2_g())
    b.bern = tuple(eng.tensor(a) for a in c["bern"])
    b.flux = tuple(eng.tensor(a) for a in c["flux"])
    # what tests/test_gpu_energetics.py::horizontal and route_two read
    b.en_case = dict(eng=eng, en=b.en, t={k: eng.tensor(c[k]) for k in ("velx", "rho", "rt", "exner", "velz_v", "rho_v", "zv_v")})
    b.en_case["t"]["theta"] = eng.tensor(np.array(c["ref"]["theta"]))
    return b


@pytest.fixture(scope="module")
def built(oracle):
    """key -> the built case; every engine is made once per module"""
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = _build(fc.case(oracle, key))
        return cache[key]
    yield get
    cache.clear()


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _levels(label, got, want):
    """relative L2 per level below TOL; returns the worst"""
    got, want = _np(got), _np(want)
    errs = fc.level_errors(got, want)
    assert np.all(np.isfinite(got)) and max(errs) < TOL, (label, errs)
    return max(errs)


def _entries(label, got, want):
    """the largest absolute error of a level below TOL of the level's largest absolute value; returns the worst ratio"""
    got, want = _np(got), _np(want)
    errs = [float(np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()) for k in range(want.shape[0])]
    assert max(errs) < TOL, (label, errs)
    return max(errs)


# ---- Engine.bernoulli ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", fc.CASES, ids=fc.case_id)
def test_bernoulli(built, key):
    b = built(key)
    c, ref = b.c, b.c["ref"]
    got = b.eng.bernoulli(*b.bern, scale=SCALE)
    again = b.eng.bernoulli(*b.bern, scale=SCALE)
    composed = b.hs.diagnose_Phi(*b.bern)
    assert b.hs.fused_phi is False
    worst = {}
    for name, want in (("element matrices", ref["phi_mat"]), ("point-wise", ref["phi_pt"]), ("composed route", composed)):
        label = "bernoulli %s vs %s" % (c["label"], name)
        worst[name] = (_levels(label, got, want), fc.assert_elements(label, _np(got), _np(want), b.i2, tol=TOL))
    print("bernoulli  %-9s order %d: worst relative L2 per level / per (level, element)  %s" % (
        c["id"], c["pn"], "  ".join("%s %.2e / %.2e" % (n, l, e) for n, (l, e) in worst.items())))
    assert torch.equal(got, again)


# ---- Engine.flux_rhs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", fc.CASES, ids=fc.case_id)
def test_flux_rhs(built, key):
    b = built(key)
    c, ref = b.c, b.c["ref"]
    got = b.eng.flux_rhs(*b.flux, scale=SCALE)
    again = b.eng.flux_rhs(*b.flux, scale=SCALE)
    composed = b.hs._uvec_hu4(*b.flux)
    assert b.hs.fused_hu is False and tuple(got.shape) == ref["flux"].shape
    worst = {}
    for name, want in (("point-wise", ref["flux"]), ("composed route", composed)):
        label = "flux_rhs %s vs %s" % (c["label"], name)
        worst[name] = (_levels(label, got, want), _entries(label, got, want))
    print("flux_rhs   %-9s order %d: worst relative L2 per level / max |error| over max |value| per level  %s" % (
        c["id"], c["pn"], "  ".join("%s %.2e / %.2e" % (n, l, e) for n, (l, e) in worst.items())))
    assert torch.equal(got, again)


# ---- Energetics.horizontal ------------------------------------------------------------------------------------------------------------------
def _horizontal(b):
    t = b.en_case["t"]
    return b.en.horizontal(t["velx"], t["rho"], t["rt"], t["exner"], t["theta"])


@pytest.mark.parametrize("key", fc.CASES, ids=fc.case_id)
def test_energetics_horizontal(built, key):
    b = built(key)
    c, ref = b.c, b.c["ref"]["horiz"]
    got = _horizontal(b)
    again = _horizontal(b)
    two = route_two(b.en_case)
    vals = got.tolist()
    e_ref = {n: abs(v - ref[n][0]) / ref[n][1] for n, v in zip(ec.HORIZ, vals)}
    e_two = {n: abs(v - w) / ref[n][1] for n, v, w in zip(ec.HORIZ, vals, two)}
    print("energetics %-9s order %d: |device - reference| / S_abs  vs restatement %s   vs composed route %s" % (
        c["id"], c["pn"], " ".join("%s %.2e" % (n, e_ref[n]) for n in ec.HORIZ), " ".join("%s %.2e" % (n, e_two[n]) for n in ec.HORIZ)))
    for n, v in zip(ec.HORIZ, vals):
        assert np.isfinite(v) and ref[n][1] > 0, n
        assert e_ref[n] <= PARITY and e_two[n] <= PARITY, (n, v, ref[n], e_ref[n], e_two[n])
    assert torch.equal(got, again)


# ---- Engine.energetics_column -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", BOXES_FUSED, ids=fc.case_id)
def test_energetics_column_fused(built, key):
    """orders 1 .. 4: 25 = 16 + 9 columns at order 1, 9 = 4 + 4 + 1 at orders 2 and 3, 9 = 4 x 2 + 1 at order 4"""
    b = built(key)
    c, ref, t = b.c, b.c["ref"]["column"], b.en_case["t"]
    args = (t["velz_v"], t["rho_v"], t["zv_v"])
    assert b.eng.mesh.n <= b.en.FUSED_MAX_ORDER
    got = b.eng.energetics_column(*args)
    again = b.eng.energetics_column(*args)
    comp = b.en.column_composed(*args)
    vals = got.tolist()
    e_ref = {n: abs(v - ref[n][0]) / ref[n][1] for n, v in zip(ec.COLUMN, vals)}
    e_cmp = {n: abs(v - w) / ref[n][1] for n, v, w in zip(ec.COLUMN, vals, comp.tolist())}
    print("column     %-9s order %d: |device - reference| / S_abs  vs restatement %s   vs composed route %s" % (
        c["id"], c["pn"], " ".join("%s %.2e" % (n, e_ref[n]) for n in ec.COLUMN), " ".join("%s %.2e" % (n, e_cmp[n]) for n in ec.COLUMN)))
    for n, v in zip(ec.COLUMN, vals):
        assert np.isfinite(v) and ref[n][1] > 0, n
        assert e_ref[n] <= PARITY and e_cmp[n] <= PARITY, (n, v, ref[n], e_ref[n], e_cmp[n])
    assert torch.equal(got, again)
    b.en.fused = True
    assert torch.equal(b.en.column(*args), got)                                          # the host takes the kernel at these orders


@pytest.mark.parametrize("key", BOXES_COMPOSED, ids=fc.case_id)
def test_energetics_column_orders_without_a_kernel(built, key):
    """orders 5, 6, 7: the entry answers MIMSEM_ERR_UNSUPPORTED and writes nothing; Energetics.column with fused = True is the composed route"""
    from mimsem_amd._lib import MimsemError
    b = built(key)
    c, eng, t = b.c, b.eng, b.en_case["t"]
    args = (t["velz_v"], t["rho_v"], t["zv_v"])
    out = torch.full((4,), 7.0, dtype=torch.float64, device=eng.device)
    blocks = torch.full((eng.nEl * (eng.nk - 1) * eng.n2e * eng.n2e,), 7.0, dtype=torch.float64, device=eng.device)   # (never read)
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = eng.L.mimsem_euler_energetics_column(eng.ctx, p(args[0]), p(args[1]), p(args[2]), p(blocks), p(out))
    torch.cuda.synchronize()
    assert rc == ERR_UNSUPPORTED and torch.equal(out, torch.full_like(out, 7.0))
    with pytest.raises(MimsemError):
        eng.energetics_column(*args, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))
    assert eng.mesh.n > b.en.FUSED_MAX_ORDER
    b.en.fused = True
    got, comp = b.en.column(*args), b.en.column_composed(*args)
    print("column     %-9s order %d: MIMSEM_ERR_UNSUPPORTED, nothing written; Energetics.column = column_composed bit for bit: %s" % (
        c["id"], c["pn"], " ".join("%s %.6e" % nv for nv in zip(ec.COLUMN, comp.tolist()))))
    assert bool(torch.isfinite(comp).all()) and torch.equal(got, comp)


# ---- the fixed-stride walk of k_energetics_horiz ----------------------------------------------------------------------------------------------
def test_energetics_horizontal_blocks_walk_several_units():
    """More units than the grid's 2 048 blocks hold at once: p = 5 has 4 units per block, so the 53 x 53 x 3 = 8 427 units of this periodic box
    send blocks 0 .. 58 round the fixed-stride walk a second time (block 58 with three of its four units), where the two wave_lds_sync() of
    the loop keep a unit's LDS rows apart from the next unit's.  No dense restatement at this size: the composed device route is the
    reference, and S_abs is the sum itself (all four terms are sums of positive contributions)."""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.energetics import Energetics
    from mimsem_amd.geom import BoxGeom
    from mimsem_amd.mesh import PeriodicBox, box_coords
    from mimsem_amd.topo import Topo
    from mimsem_amd.vertsolve import VertSolve
    from tests.helpers import z_levels
    pn, ne, nk, EPB = 5, 53, 3, 4
    bx = PeriodicBox(pn, ne, 1); coords = box_coords(pn, ne, 1000.0)
    t = Topo(bx, 0, nk)
    g = BoxGeom(t, bx, coords, nk, 1000.0)
    r = np.random.default_rng(13)
    g.set_levels(z_levels(nk, g.n0, r, ztop=1500.0))
    eng = Engine(DeviceMesh([t], [g], nk=nk, numbering="global"))
    units = eng.nEl * nk
    assert eng.nEl == ne * ne and units > EN_MAX_BLOCKS * EPB
    assert 256 // 64 == EPB and (pn + 1) ** 2 > 32                                        # the 64-lane layout
    second = units - EN_MAX_BLOCKS * EPB
    assert (second // EPB, second % EPB) == (58, 3)                                         # blocks 0 .. 57 full, block 58 partial
    c = dict(eng=eng, en=Energetics(eng, VertSolve(eng, 0.0)))
    F = dict(velx=r.standard_normal((nk, eng.sizes[1])))
    for k, (lo, hi) in dict(rho=(0.8, 1.2), rt=(290, 310), exner=(900, 1000), theta=(290, 310)).items():
        F[k] = r.uniform(lo, hi, (nk, eng.sizes[2]))
    c["t"] = {k: eng.tensor(v) for k, v in F.items()}
    tt = c["t"]
    run = lambda: c["en"].horizontal(tt["velx"], tt["rho"], tt["rt"], tt["exner"], tt["theta"])
    got, again, two = run(), run(), route_two(c)
    errs = [abs(v - w) / abs(w) for v, w in zip(got.tolist(), two)]
    print("energetics walk p=5 ne=53 nk=3 (%d units, %d in the second trip): fused kernel vs composed route, relative  %s" % (
        units, second, "  ".join("%s %.2e" % ne_ for ne_ in zip(ec.HORIZ, errs))))
    assert all(w > 0 for w in two) and max(errs) <= PARITY
    assert torch.equal(got, again)
