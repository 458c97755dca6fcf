"""mimsem_horiz_momentum_forcing (csrc/momentum_forcing.inc): the element-local forcing of HorizSolve::momentum_rhs
    out_k (+)= R(q_k) a_k + F(th_k) g_k + 1/2 sum_{i in {k-1, k}} Rh(dz_i) v_i
for every level in two launches, through Engine.momentum_forcing, against the oracle's dense ROTMAT / UHMAT / UTQWMAT matrices
(tests/box_strang_case.py forcing_dense) per level and against the composed route (one Engine.apply per operator and the interface-to-level
sums).  Bar: relative L2 < 1e-10 per level, the bar of tests/test_gpu_bernoulli.py and tests/test_gpu_flux_rhs.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import box_strang_case as bc
from tests import vort_diag_case as vc
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-10
SCALE = bc.SCALE
VERT, ACCUM = 1, 2
ERR_ARG, ERR_UNSUPPORTED = -1, -2


def _engine(c, nk):
    from mimsem_amd.device import DeviceMesh, Engine
    c["eng"] = Engine(DeviceMesh(c["topos"], c["geoms"], nk=nk, numbering="global"))
    return c


def _tensors(eng, F):
    return {t: tuple(eng.tensor(np.array(x)) for x in F[t]) for t in bc.TERMS if t in F}      # (the case's arrays are read-only: copies)


def _case(c):
    c = _engine(c, c["nk"])
    c["T"] = _tensors(c["eng"], c["FF"])
    return c


def _fused(eng, T, terms=bc.TERMS, flags=0, out=None):
    return eng.momentum_forcing(rot=T.get("rot") if "rot" in terms else None, pgf=T.get("pgf") if "pgf" in terms else None,
                                vor=T.get("vor") if "vor" in terms else None, scale=SCALE, flags=flags, out=out)


def _composed(eng, T, terms=bc.TERMS, vert=False):
    """the route momentum_rhs takes without the kernel: one apply per operator, every interface's Rh v added to its two levels"""
    nk = (T["rot"][1] if "rot" in T else T["pgf"][1]).shape[0]
    out = eng.zeros(nk, eng.sizes[1])
    if "rot" in terms and "rot" in T:
        out += eng.apply("ROTMAT", T["rot"][1], f=T["rot"][0], scale=SCALE)
    if "pgf" in terms and "pgf" in T:
        out += eng.apply("UHMAT", T["pgf"][1], f=T["pgf"][0], scale=SCALE, flags=VERT if vert else 0)
    if "vor" in terms and "vor" in T:
        t = eng.apply("UTQWMAT", T["vor"][1], f=T["vor"][0], lev0=0, scale=SCALE)
        out[1:] += 0.5 * t
        out[:-1] += 0.5 * t
    return out


def _check(label, got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    want = want.cpu().numpy() if torch.is_tensor(want) else want
    assert got.shape == want.shape, (got.shape, want.shape)
    errs = [rel_l2(got[k], want[k]) for k in range(want.shape[0])]
    print("%s: relative L2 per level  %s" % (label, "  ".join("%.2e" % e for e in errs)))
    assert np.all(np.isfinite(got)) and all(np.linalg.norm(w) > 0 for w in want) and max(errs) < TOL, (label, errs)


@pytest.fixture(scope="module")
def sphere(oracle):
    """p = 3, ne = 2, nk = 3, a full Jacobian: 72 units of 16 lanes, 16 to a block -- the last block is partial"""
    return _case(bc.sphere_forcing_case())


@pytest.fixture(scope="module")
def box(oracle):
    """p = 4, ne = 3, nk = 2 periodic box: 25 points on 32 lanes, one interface feeding both levels"""
    return _case(bc.box_forcing_case(oracle))


@pytest.fixture(scope="module")
def cases(sphere, box):
    return dict(sphere=sphere, box=box)


@pytest.mark.parametrize("vert", [False, True], ids=["no_const_vert", "const_vert"])
@pytest.mark.parametrize("which", ["sphere", "box"])
def test_summed_against_the_dense_matrices_and_the_composed_route(which, vert, cases):
    c = cases[which]
    got = _fused(c["eng"], c["T"], flags=VERT if vert else 0)
    _check("%s, kernel vs dense matrices" % which, got, bc.forcing_dense(c["gd"], c["FF"], vert=vert))
    _check("%s, kernel vs composed route" % which, got, _composed(c["eng"], c["T"], vert=vert))


@pytest.mark.parametrize("term", bc.TERMS)
@pytest.mark.parametrize("which", ["sphere", "box"])
def test_each_term_alone_against_its_operator(which, term, cases):
    """the other two pairs NULL.  vor alone on the sphere (nk = 3): level 0 takes interface 0 only, level 2 interface 1 only, level 1 both"""
    c = cases[which]
    got = _fused(c["eng"], c["T"], (term,))
    _check("%s %s alone, kernel vs dense matrix" % (which, term), got, bc.forcing_dense(c["gd"], c["FF"], (term,)))
    _check("%s %s alone, kernel vs one apply" % (which, term), got, _composed(c["eng"], c["T"], (term,)))
    if term == "vor":
        t = 0.5 * c["eng"].apply("UTQWMAT", c["T"]["vor"][1], f=c["T"]["vor"][0], lev0=0, scale=SCALE)
        _check("%s first and last level: one interface each" % which, torch.stack([got[0], got[-1]]), torch.stack([t[0], t[-1]]))


def test_one_and_two_levels(sphere):
    """nk = 1: no interface, the third pair must be absent; nk = 2: one interface feeding both levels.  Rows 0 .. nk-1 of the same arrays"""
    eng, gd = sphere["eng"], sphere["gd"]
    one = bc.sub_levels(sphere["FF"], 1)
    T1 = _tensors(eng, one)
    got = _fused(eng, T1)
    assert got.shape == (1, eng.sizes[1])
    _check("nk = 1", got, bc.forcing_dense(gd, one))
    flat = eng.momentum_forcing(rot=tuple(x[0] for x in T1["rot"]), pgf=tuple(x[0] for x in T1["pgf"]), scale=SCALE)    # [n] rows
    assert torch.equal(flat.reshape(-1), got[0])
    two = bc.sub_levels(sphere["FF"], 2)
    _check("nk = 2", _fused(eng, _tensors(eng, two)), bc.forcing_dense(gd, two))
    # a strided view is made contiguous by the wrapper: the bits of the packed call
    wide = {}
    for t, pair in sphere["T"].items():
        big = [torch.full((2 * x.shape[0], x.shape[1]), 1.0e30, dtype=torch.float64, device=x.device) for x in pair]
        for b, x in zip(big, pair):
            b[::2] = x
        wide[t] = tuple(b[::2] for b in big)
        assert not wide[t][0].is_contiguous()
    assert torch.equal(_fused(eng, wide), _fused(eng, sphere["T"]))


def test_two_element_periodic_box(oracle):
    """ne = 2: an element's two neighbours in a direction are the same element, every edge of the box wraps around"""
    c = _case(bc.box_forcing_case(oracle, pn=3, ne=2, nk=2, seed=91))
    got = _fused(c["eng"], c["T"])
    _check("2 x 2 box, kernel vs dense matrices", got, bc.forcing_dense(c["gd"], c["FF"]))
    _check("2 x 2 box, kernel vs composed route", got, _composed(c["eng"], c["T"]))


def _random_tensors(eng, nk, seed):
    r = np.random.default_rng(seed)
    n0, n1, n2 = eng.sizes[0], eng.sizes[1], eng.sizes[2]
    draw = lambda rows, n: eng.tensor(r.standard_normal((rows, n)))
    return dict(rot=(draw(nk, n0), draw(nk, n1)), pgf=(draw(nk, n2), draw(nk, n1)), vor=(draw(nk - 1, n1), draw(nk - 1, n2)))


@pytest.mark.parametrize("pn", [1, 2, 5, 6, 7])
def test_other_orders_against_the_composed_route(pn):
    """the 4-lane layout (order 1, a 5 x 5 box: 75 units, 64 + 11) and, on a one-element-per-face sphere (18 units), orders 2 and 5 (9 and 36
    live lanes of 16 and 64) and the 64-lane orders 6 and 7 (49 and 64 live lanes): with the fixtures' orders 3 and 4 every built order runs;
    no dense restatement at these orders: the composed device route is the reference"""
    from mimsem_amd.geom import BoxGeom, Geom
    from mimsem_amd.mesh import CubedSphere, PeriodicBox, box_coords, sphere_coords
    from mimsem_amd.topo import Topo
    from tests.helpers import z_levels
    nk = 3
    r = np.random.default_rng(50 + pn)
    if pn == 1:
        bx = PeriodicBox(pn, 5, 1)
        topos = [Topo(bx, 0, nk)]
        geoms = [BoxGeom(topos[0], bx, box_coords(pn, 5, 1000.0), nk, 1000.0)]
    else:
        cs = CubedSphere(pn, 1, 6); coords = sphere_coords(pn, 1)
        topos = [Topo(cs, p, nk) for p in range(6)]
        geoms = [Geom(t, cs, coords, nk) for t in topos]
    levs = z_levels(nk, geoms[0].n0, r)
    for g in geoms:
        g.set_levels(levs)
    c = _engine(dict(topos=topos, geoms=geoms), nk)
    T = _random_tensors(c["eng"], nk, 60 + pn)
    for vert in (False, True):
        _check("order %d vert=%d, kernel vs composed route" % (pn, vert), _fused(c["eng"], T, flags=VERT if vert else 0), _composed(c["eng"], T, vert=vert))


def test_accumulates_onto_a_set_output(sphere):
    eng, T = sphere["eng"], sphere["T"]
    a = _fused(eng, T)
    out = torch.full_like(a, float("nan"))                                       # poisoned, then set: ACCUM adds to what is there, nothing else
    base = torch.linspace(-1.0, 1.0, a.numel(), dtype=torch.float64, device=a.device).reshape(a.shape) * float(a.abs().mean())
    out.copy_(base)
    got = _fused(eng, T, flags=ACCUM, out=out)
    assert got is out and torch.equal(out, base + a)
    # without ACCUM a poisoned output is overwritten
    out.fill_(float("nan"))
    assert torch.equal(_fused(eng, T, out=out), a)
    # all three pairs absent: zero, or untouched with ACCUM
    out.copy_(base)
    assert torch.equal(_fused(eng, T, (), flags=ACCUM, out=out), base)
    assert torch.equal(_fused(eng, T, (), out=out), torch.zeros_like(a))


def test_same_bits_repeated_and_replayed(sphere):
    eng, T = sphere["eng"], sphere["T"]
    a = _fused(eng, T)
    assert torch.equal(a, _fused(eng, T))                                        # two calls
    g, out = eng.capture(lambda: _fused(eng, T))                                 # (the calls above have sized the workspace)
    out.zero_()
    g.replay(); torch.cuda.synchronize()
    assert torch.equal(out, a)


def test_argument_errors_write_nothing(sphere):
    eng, nk, T = sphere["eng"], vc.NK, sphere["T"]
    fn = eng.L.mimsem_horiz_momentum_forcing
    out = torch.full((nk, eng.sizes[1]), 7.0, dtype=torch.float64, device=eng.device)
    p = dict(q=T["rot"][0], a=T["rot"][1], th=T["pgf"][0], g=T["pgf"][1], dz=T["vor"][0], v=T["vor"][1], out=out)
    names = ("q", "a", "th", "g", "dz", "v")

    def call(ctx=eng.ctx, nk_=nk, flags=0, alias=None, **null):
        x = {k: (None if k in null else C.c_void_p(t.data_ptr())) for k, t in p.items()}
        if alias:
            x["out"] = x[alias]                                                  # (refused before anything is launched)
        return fn(ctx, nk_, flags, SCALE, *[x[k] for k in names], x["out"])
    assert call(ctx=None) == ERR_ARG and call(out=True) == ERR_ARG
    for k in names:                                                              # one NULL of a pair
        assert call(**{k: True}) == ERR_ARG, k
    for bad in (0, -1, nk + 1):
        assert call(nk_=bad) == ERR_ARG, bad
    assert call(nk_=1) == ERR_ARG                                                # one level has no interface
    assert call(flags=4) == ERR_ARG and call(flags=8) == ERR_ARG                 # only VERT and ACCUM
    ins = [p[k].clone() for k in names]
    for k in names:
        assert call(alias=k) == ERR_ARG, k
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))                           # the poisoned output stays poisoned
    assert all(torch.equal(a, p[k]) for a, k in zip(ins, names))                 # and no input was taken for the output
    assert call() == 0 and call(nk_=1, dz=True, v=True) == 0
    torch.cuda.synchronize()
    want = _fused(eng, T)
    assert torch.equal(out[1:], want[1:])                                        # (row 0 rewritten by the one-level call)
    from mimsem_amd._lib import MimsemError
    poisoned = torch.full_like(out, 7.0)
    rot, pgf, vor = T["rot"], T["pgf"], T["vor"]
    mf = eng.momentum_forcing
    for bad in (lambda: mf(rot=(rot[0], None), pgf=pgf, vor=vor, out=poisoned),                     # one of a pair missing
                lambda: mf(rot=(rot[0], rot[1][:2]), pgf=pgf, vor=vor, out=poisoned),               # row counts differ
                lambda: mf(rot=rot, pgf=pgf, vor=(vor[0], vor[1][:1]), out=poisoned),               # interface rows differ
                lambda: mf(rot=rot, pgf=pgf, vor=(vor[1], vor[0]), out=poisoned),                   # spaces swapped
                lambda: mf(rot=rot, pgf=(pgf[0][:, :-1], pgf[1]), vor=vor, out=poisoned),           # rows too short
                lambda: mf(rot=rot, pgf=(pgf[0].float(), pgf[1]), vor=vor, out=poisoned),           # dtype
                lambda: mf(rot=(rot[0][:1], rot[1][:1]), vor=vor, out=poisoned[:1]),                # an interface with one level
                lambda: mf(rot=rot, pgf=pgf, vor=vor, out=poisoned[:2]),                            # out too small
                lambda: mf(rot=rot, pgf=pgf, vor=vor, flags=4, out=poisoned),                       # unknown flag
                lambda: mf(rot=rot, pgf=pgf, vor=vor, flags=ACCUM),                                 # ACCUM without out
                lambda: mf(rot=rot, pgf=pgf, vor=vor, out=rot[1])):                                 # out is an input
        with pytest.raises(MimsemError):
            bad()
    torch.cuda.synchronize()
    assert torch.equal(poisoned, torch.full_like(out, 7.0))
