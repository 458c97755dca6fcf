"""mimsem_zonal_plan_build / mimsem_euler_zonal_moments (csrc/zonal_stats.inc) through Engine.zonal_plan / zonal_moments and ZonalStats
(mimsem_amd/zonalstats.py), and the Held-Suarez driver around them, against the fsum restatement of tests/zonal_case.py and against
ZonalStats.composed.  Bar: 1e-10 per (moment, level, band) entry on |got - want| / S_abs, S_abs the sum of the absolute values of the
entry's terms (the bar and the measure of tests/test_gpu_energetics.py).

Observed on an MI355X (max over the entries): see DESIGN.md 8, "Zonal-mean statistics"."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import energetics_case as ec
from tests import zonal_case as zc

pytestmark = pytest.mark.gpu
TOL = 1e-10
ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_MOMENTS = [3, 7, 8]                    # the moments that hold T


def _engine(c, nk):
    from mimsem_amd.device import DeviceMesh, Engine
    return Engine(DeviceMesh(c["topos"], c["geoms"], nk=nk, numbering="global"))


def _state(eng, c):
    """(velx, None, rho, rt, exner) of an energetics case on the device"""
    return (eng.tensor(np.array(c["velx"])), None, eng.tensor(np.array(c["rho"])), eng.tensor(np.array(c["rt"])), eng.tensor(np.array(c["exner"])))


def _sample(eng, st, band, nb, nlev=None, acc=None):
    """one sample into zeros (or onto acc) with the plan of `band`"""
    eng.zonal_plan(band, nb)
    nlev = st[0].shape[0] if nlev is None else nlev
    acc = eng.zeros(9, nlev, nb) if acc is None else acc
    eng.zonal_moments(st[0][:nlev], st[2][:nlev], st[3][:nlev], st[4][:nlev], acc)
    torch.cuda.synchronize()
    return acc


def _check(label, got, want, s_abs):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape, (got.shape, want.shape)
    errs = [zc.rel_err(got[m], want[m], s_abs[m]) for m in range(9)]
    print("%s: max |got - want| / S_abs per moment  %s" % (label, "  ".join("%s %.1e" % (n, e) for n, e in zip(zc.MOMENTS, errs))))
    assert np.isfinite(got).all() and max(errs) < TOL, (label, errs)


@pytest.fixture(scope="module")
def sphere(oracle):
    """p = 3, ne = 2, nk = 3 cubed sphere (24 elements, 384 points), a full Jacobian; positive rho, rt, exner, random velx; the point values
    of the restatement are made once and shared"""
    c = ec.make_case()
    c["eng"] = _engine(c, c["nk"])
    c["st"] = _state(c["eng"], c)
    c["fields"], c["weight"] = zc.point_fields(c["patches"], c["velx"], c["rho"], c["rt"], c["exner"])
    return c


def _random_band(c, nb, seed, empty=None, out_fraction=0.1):
    r = np.random.default_rng(seed)
    eng = c["eng"]
    keep = [b for b in range(nb) if b != empty]
    band = r.choice(keep, size=(eng.nEl, eng.mp12)).astype(np.int32)
    band[r.random(band.shape) < out_fraction] = -1
    return band


def test_nine_moments_against_the_fsum_restatement(sphere):
    """random band table, nb = 5, about a tenth of the points left out, band 2 empty"""
    c, eng = sphere, sphere["eng"]
    band = _random_band(c, 5, 1, empty=2)
    assert (band == -1).any() and not (band == 2).any() and all((band == b).any() for b in (0, 1, 3, 4))
    want, s_abs = zc.moments(c["fields"], c["weight"], band, 5)
    got = _sample(eng, c["st"], band, 5).cpu().numpy()
    _check("sphere p = 3, nb = 5", got, want, s_abs)
    assert not got[:, :, 2].any() and not np.signbit(got[:, :, 2]).any()                   # the empty band: exactly 0.0
    kept = float(c["weight"][band >= 0].sum())
    assert abs(got[0, 0].sum() / kept - 1.0) < 1e-12 and kept < 0.95 * c["weight"].sum()   # the points left out are not in acc[0]
    assert np.array_equal(got[0, 0], got[0, 1])                                            # the weights do not depend on the level


@pytest.mark.parametrize("pn", [1, 2, 3, 4, 5, 6, 7])
def test_every_order_against_the_composed_route(pn):
    """the smallest mesh of each order (order 1: a 5 x 5 periodic box; above: a sphere of one element per face), three levels, three
    bands with a point left out: kernel against ZonalStats.composed at the same bar.  Orders 3 and 4 meet the fsum restatement in
    test_nine_moments_against_the_fsum_restatement and test_periodic_box"""
    from mimsem_amd.geom import BoxGeom, Geom, gll_points
    from mimsem_amd.mesh import CubedSphere, PeriodicBox, box_coords, sphere_coords
    from mimsem_amd.topo import Topo
    from mimsem_amd.zonalstats import ZonalStats
    from tests.helpers import z_levels
    nk = 3
    r = np.random.default_rng(70 + pn)
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
    eng = _engine(dict(topos=topos, geoms=geoms), nk)
    # positive 2-forms: a constant has the DoFs c (cell width x) (cell width y); half a per cent of noise on them keeps the interpolant positive
    # at every order (5 % does not at order 6: the end cells are narrow), the factor per element and level makes the fields differ
    wd = np.diff(gll_points(pn)); cell = np.outer(wd, wd).ravel()
    two = lambda lo, hi: eng.tensor(r.uniform(lo, hi, (nk, eng.nEl, 1)) * cell[None, None, :] * (1.0 + 0.005 * r.standard_normal((nk, eng.nEl, pn * pn)))
                                    ).reshape(nk, -1)
    st = (eng.tensor(r.standard_normal((nk, eng.sizes[1]))), None, two(0.8, 1.2), two(290.0, 310.0), two(900.0, 1000.0))
    lat = r.uniform(-0.5 * np.pi, 0.5 * np.pi, (eng.nEl, eng.mp12))
    zs = ZonalStats(eng, lat, 3)
    zs.band[0, 0] = -1                                                                       # one point left out
    eng.zonal_plan(zs.band, 3)
    want, s_abs = zs.composed(st).cpu().numpy(), zs.composed(st, absolute=True).cpu().numpy()
    assert np.isfinite(want).all() and (want[0] > 0).all() and (want[3] > 0).all()           # every band holds points, r > 0 everywhere
    zs.sample(st); torch.cuda.synchronize()
    assert zs.count == 1
    _check("order %d, kernel vs composed" % pn, zs.moments(), want, s_abs)


def test_periodic_box(oracle):
    """p = 4, 2 x 2 periodic box (a diagonal Jacobian, 25 points per element, every edge wraps), nk = 2, levels perturbed per point;
    an arbitrary band table: the kernel takes no sphere for granted"""
    c = ec.make_box_case(oracle, pn=4, ne=2, nk=2, seed=47)
    c["eng"] = eng = _engine(c, 2)
    band = _random_band(c, 4, 5)
    want, s_abs = zc.restate(c["patches"], c["velx"], c["rho"], c["rt"], c["exner"], band, 4)
    _check("box p = 4", _sample(eng, _state(eng, c), band, 4), want, s_abs)


def test_list_shapes(sphere):
    """nb = 1: the 384 points cross one block stride of 256; a band of exactly 1 point and one of exactly 257; nk = 1"""
    c, eng = sphere, sphere["eng"]
    one = np.zeros((eng.nEl, eng.mp12), dtype=np.int32)
    want, s_abs = zc.moments(c["fields"], c["weight"], one, 1)
    _check("nb = 1", _sample(eng, c["st"], one, 1), want, s_abs)
    shapes = np.full(eng.nEl * eng.mp12, 2, dtype=np.int32)
    order = np.random.default_rng(9).permutation(shapes.size)
    shapes[order[0]] = 0; shapes[order[1:258]] = 1
    shapes = shapes.reshape(eng.nEl, eng.mp12)
    assert [(shapes == b).sum() for b in range(3)] == [1, 257, 126]
    want, s_abs = zc.moments(c["fields"], c["weight"], shapes, 3)
    got = _sample(eng, c["st"], shapes, 3)
    _check("bands of 1, 257 and 126 points", got, want, s_abs)
    e, q = np.argwhere(shapes == 0)[0]
    assert float(got[0, 0, 0]) == c["weight"][e, q]                                          # one term: no sum at all
    got1 = _sample(eng, c["st"], shapes, 3, nlev=1)
    assert tuple(got1.shape) == (9, 1, 3) and torch.equal(got1[:, 0], got[:, 0])             # nk = 1: the bits of level 0 of the full call
    _check("nk = 1", got1, want[:, :1], s_abs[:, :1])


@pytest.mark.parametrize("nb", [7, 64])
def test_zonal_stats_bands(sphere, nb):
    """the latitude bands of ZonalStats on the 384 points: nb = 7, and nb = 64 with most bands empty"""
    from mimsem_amd.zonalstats import ZonalStats, band_index
    c, eng = sphere, sphere["eng"]
    lat = zc.latitudes(c)
    zs = ZonalStats(eng, eng.tensor(lat), nb)
    assert np.array_equal(zs.band, band_index(lat, nb)) and zs.band.min() >= 0 and zs.band.max() < nb
    want, s_abs = zc.moments(c["fields"], c["weight"], zs.band, nb)
    zs.sample(c["st"]); torch.cuda.synchronize()
    empty = s_abs[0, 0] == 0.0
    print("nb = %d: %d bands empty" % (nb, int(empty.sum())))
    assert nb != 64 or empty.sum() > nb // 2
    _check("ZonalStats, nb = %d" % nb, zs.moments(), want, s_abs)
    m = zs.means()
    assert np.isnan(m["T"][:, empty]).all() and np.isfinite(m["T"][:, ~empty]).all() and m["T"].shape == (c["nk"], nb)
    assert np.allclose(m["T"][:, ~empty], want[3][:, ~empty] / want[0][:, ~empty], rtol=1e-10, atol=0.0)
    assert np.array_equal(zs.composed(c["st"]).cpu().numpy()[:, :, empty], np.zeros((9, c["nk"], int(empty.sum()))))
    _check("ZonalStats.composed, nb = %d" % nb, zs.composed(c["st"]), want, s_abs)
    zs.FUSED = False                                                                         # (an instance attribute: the class default stays)
    zs.sample(c["st"])
    assert zs.count == 2
    _check("kernel + composed sample, nb = %d" % nb, zs.moments(), 2.0 * want, 2.0 * s_abs)


def test_accumulates_reproducibly_and_replays(sphere):
    from mimsem_amd.device import check
    c, eng, st = sphere, sphere["eng"], sphere["st"]
    band = _random_band(c, 5, 2, empty=4)
    s = _sample(eng, st, band, 5)
    acc = torch.full_like(s, float("nan"))                                                   # poisoned, then set to a base
    base = torch.linspace(-1.0, 1.0, s.numel(), dtype=torch.float64, device=s.device).reshape(s.shape) * float(s.abs().mean())
    acc.copy_(base)
    got = _sample(eng, st, band, 5, acc=acc)
    assert got is acc and torch.equal(acc, base + s)                                         # the sample is formed first, added once
    assert torch.equal(acc[:, :, 4], base[:, :, 4])                                          # the empty band: untouched
    assert torch.equal(_sample(eng, st, band, 5), s)                                         # two calls: the same bits
    L, g = eng.L, C.c_void_p()
    rec = eng.zeros(9, c["nk"], 5)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    check(L.mimsem_graph_begin(eng.ctx), "graph_begin")
    rc = L.mimsem_euler_zonal_moments(eng.ctx, c["nk"], ptr(st[0]), ptr(st[2]), ptr(st[3]), ptr(st[4]), ptr(rec))
    check(L.mimsem_graph_end(eng.ctx, C.byref(g)), "graph_end")
    check(rc, "mimsem_euler_zonal_moments (captured)")
    try:
        assert L.mimsem_graph_num_nodes(g) == 1                                              # one launch: a chain with no parallel branch
        torch.cuda.synchronize()
        assert not rec.any()                                                                 # (recording executes nothing)
        check(L.mimsem_graph_launch(g), "graph_launch"); torch.cuda.synchronize()
        assert torch.equal(rec, s)
        check(L.mimsem_graph_launch(g), "graph_launch"); torch.cuda.synchronize()
        assert torch.equal(rec, s + s)                                                       # a running sum without a read-back
    finally:
        L.mimsem_graph_destroy(g)


def test_nan_is_contained(sphere):
    """a NaN in one DoF of rho in element 5 on level 1: NaN in the T moments of exactly the bands that element's points fall into on that
    level, finite everywhere else -- the velocity moments of those bands included, which do not hold rho.  r <= 0 reads the same: the
    element's rho with its sign turned is negative at every one of its points"""
    c, eng, st = sphere, sphere["eng"], sphere["st"]
    nb = 40                                                                                  # more bands than an element has points
    band = _random_band(c, nb, 3, out_fraction=0.3)
    hit = np.zeros(nb, dtype=bool)
    hit[band[5][band[5] >= 0]] = True
    assert hit.any() and not hit.all()
    for bad in ("nan", "negative"):
        rho = st[2].clone()
        if bad == "nan":
            rho[1, 5 * eng.n2e + 2] = float("nan")
        else:
            rho[1, 5 * eng.n2e:6 * eng.n2e] *= -1.0
        got = _sample(eng, (st[0], None, rho, st[3], st[4]), band, nb).cpu().numpy()
        nan = np.isnan(got)
        want = np.zeros_like(nan)
        want[np.ix_(T_MOMENTS, [1], np.flatnonzero(hit))] = True
        assert np.array_equal(nan, want) and np.isfinite(got[~want]).all(), bad
    clean = _sample(eng, st, band, nb).cpu().numpy()
    assert np.array_equal(got[~want], clean[~want])                                          # and nothing else moved


def test_argument_errors_change_nothing(sphere):
    from mimsem_amd._lib import MimsemError
    c, eng, st, nk = sphere, sphere["eng"], sphere["st"], sphere["nk"]
    band = _random_band(c, 5, 4)
    s = _sample(eng, st, band, 5)
    L = eng.L
    acc = torch.full_like(s, 7.0)
    p = dict(velx=st[0], rho=st[2], rt=st[3], exner=st[4], acc=acc)
    names = ("velx", "rho", "rt", "exner", "acc")

    def call(ctx=eng.ctx, nlev=nk, alias=None, **null):
        x = {k: (None if k in null else C.c_void_p(t.data_ptr())) for k, t in p.items()}
        if alias:
            x["acc"] = x[alias]                                                              # (refused before anything is launched)
        return L.mimsem_euler_zonal_moments(ctx, nlev, *[x[k] for k in names])
    other = _engine(c, nk)                                                                   # a context without a plan
    assert call(ctx=other.ctx) == ERR_ARG and call(ctx=None) == ERR_ARG
    for k in names:
        assert call(**{k: True}) == ERR_ARG, k
    for bad in (0, -1, nk + 1):
        assert call(nlev=bad) == ERR_ARG, bad
    ins = [p[k].clone() for k in names[:4]]
    for k in names[:4]:
        assert call(alias=k) == ERR_ARG, k
    inside = C.c_void_p(st[2].data_ptr() + 8 * (st[2].numel() - 1))                          # acc beginning in the last entry of rho: an overlap
    assert L.mimsem_euler_zonal_moments(eng.ctx, nk, *[C.c_void_p(p[k].data_ptr()) for k in names[:4]], inside) == ERR_ARG
    # a band table out of range, nb <= 0, a null table: refused, the old plan stays
    tbl = np.ascontiguousarray(band)
    for value, nb in ((5, 5), (-2, 5), (0, 0), (0, -3)):
        t = tbl.copy(); t[3, 7] = value
        assert L.mimsem_zonal_plan_build(eng.ctx, C.c_void_p(t.ctypes.data), nb) == ERR_ARG, (value, nb)
    assert L.mimsem_zonal_plan_build(eng.ctx, None, 5) == ERR_ARG and L.mimsem_zonal_plan_build(None, C.c_void_p(tbl.ctypes.data), 5) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(acc, torch.full_like(acc, 7.0))                                       # the poisoned acc stays poisoned
    assert all(torch.equal(a, p[k]) for a, k in zip(ins, names))
    acc.zero_()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(acc, s)                                                               # the old plan, bit for bit
    poisoned = torch.full_like(s, 7.0)
    zm = eng.zonal_moments
    for bad in (lambda: zm(st[0], st[2], st[3], None, poisoned),                             # an operand missing
                lambda: zm(st[0], st[2][:2], st[3], st[4], poisoned),                        # row counts differ
                lambda: zm(st[2], st[0], st[3], st[4], poisoned),                            # spaces swapped
                lambda: zm(st[0], st[2][:, :-1], st[3], st[4], poisoned),                    # rows too short
                lambda: zm(st[0], st[2].float(), st[3], st[4], poisoned),                    # dtype
                lambda: zm(st[0], st[2], st[3], st[4], poisoned[:, :2]),                     # acc of another level count
                lambda: zm(st[0], st[2], st[3], st[4], poisoned[:, :, :4]),                  # acc of another band count
                lambda: zm(st[0], st[2], st[3], st[4], None),
                lambda: other.zonal_moments(st[0], st[2], st[3], st[4], poisoned),           # no plan
                lambda: eng.zonal_plan(band[:5], 5),                                         # a table of another shape
                lambda: eng.zonal_plan(band, 4),                                             # a value beyond nb
                lambda: eng.zonal_plan(np.full_like(band, -2), 5)):
        with pytest.raises(MimsemError):
            bad()
    torch.cuda.synchronize()
    assert torch.equal(poisoned, torch.full_like(s, 7.0))
    wide = torch.full((2 * nk, st[2].shape[1]), 1.0e30, dtype=torch.float64, device=eng.device)
    wide[::2] = st[2]
    assert not wide[::2].is_contiguous()
    out = eng.zeros(9, nk, 5)
    zm(st[0], wide[::2], st[3], st[4], out); torch.cuda.synchronize()
    assert torch.equal(out, s)                                                               # a strided view is made contiguous by the wrapper


@pytest.fixture(scope="module")
def strang(oracle):
    """the case of tests/test_gpu_cpp_euler.py (tests/strang_case.py: p = 3, ne = 2, nk = 4) under Held-Suarez forcing"""
    from tests import strang_case as sc
    from tests.test_gpu_strang2 import make_euler
    c = sc.make_case()
    c["eng"] = _engine(c, c["nk"])
    c["t0"] = tuple(c["eng"].tensor(a) for a in c["state"])
    c["eu"] = make_euler(c, hs_forcing=True)
    return c


def test_two_strang_steps_sampled_through_run(strang, tmp_path):
    from mimsem_amd.zonalstats import ZonalStats
    c, eng, eu = strang, strang["eng"], strang["eu"]
    lat = zc.latitudes(c)
    stats, states = ZonalStats(eng, lat, 4), []

    def on_state(step, state):
        states.append(state)
        stats.sample(step, state)                                                            # the hook form of sample
    eu.run(c["t0"], 2, outdir=str(tmp_path / "out"), integrator="strang", on_state=on_state)
    assert stats.count == 2 and len(states) == 2 and eu.steps == 2
    host = lambda a: a.detach().cpu().numpy()
    want, s_abs = np.zeros((9, c["nk"], 4)), np.zeros((9, c["nk"], 4))
    for st in states:
        S, A = zc.restate(c["patches"], host(st[0]), host(st[2]), host(st[3]), host(st[4]), stats.band, 4)
        want += S; s_abs += A
    _check("two strang steps under Held-Suarez forcing", stats.moments(), want, s_abs)
    assert 150.0 < np.nanmin(stats.means()["T"]) and np.nanmax(stats.means()["T"]) < 350.0
    # save, a fresh object, load, a third sample: the bits of three samples uninterrupted
    path = str(tmp_path / "zonal_stats.npz")
    stats.save(path)
    stats.sample(states[1]); torch.cuda.synchronize()
    again = ZonalStats(eng, lat, 4)
    again.load(path)
    assert again.count == 2
    again.sample(states[1]); torch.cuda.synchronize()
    assert again.count == stats.count == 3 and torch.equal(again.acc, stats.acc)


def test_driver_writes_the_statistics_of_a_held_suarez_run(tmp_path):
    """scripts/run_umjs14.py --case held-suarez --ne 2 --nsteps 2 --zonal-stats 8 as a fresh child process under a time limit"""
    out = str(tmp_path / "hs")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "run_umjs14.py"), "--case", "held-suarez", "--ne", "2", "--nsteps", "2", "--zonal-stats", "8",
           "--outdir", out, "--time-limit", "240"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:]); print(r.stderr[-2000:])
    assert r.returncode == 0
    assert "Held-Suarez case" in r.stdout and "16 levels, dt = 120 s, Euler.strang, Held-Suarez forcing" in r.stdout
    assert "zonal statistics: 8 bands, 2 samples" in r.stdout and "ms per sample" in r.stdout
    with np.load(os.path.join(out, "zonal_stats.npz")) as z:
        acc, count, nb = z["acc"], int(z["count"]), int(z["nbands"])
    assert count == 2 and nb == 8 and acc.shape == (9, 16, 8)
    full = acc[0, 0] > 0.0
    assert full.sum() >= 4 and np.isfinite(acc).all() and not acc[:, :, ~full].any()
    T = acc[3][:, full] / acc[0][:, full]
    print("zonal-mean T after two steps: %.1f .. %.1f K" % (T.min(), T.max()))
    assert 150.0 < T.min() and T.max() < 350.0
