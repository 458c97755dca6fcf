"""Euler::diagnostics on the device (mimsem_amd/energetics.py) and the entry under it, mimsem_euler_energetics_horiz (csrc/energetics.inc),
against the oracle restatement of tests/energetics_case.py (checked on the CPU by tests/test_energetics_cpu.py).  Errors are taken relative
to S_abs, the sum of the absolute per-element (per-column) contributions -- k2p and p2k are signed and may cancel -- and held to the
project's parity bar."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import energetics_case as ec

pytestmark = pytest.mark.gpu
PARITY = 1e-10           # README "N3 parity bar", SURVEY 8(c)
ERR_ARG = -1
SCALE, VERT = ec.SCALE, 1


def build(c):
    """engine, Energetics and the device copies of a case's inputs (theta: the oracle's diagTheta_L2, an INPUT of horizontal())"""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.energetics import Energetics
    from mimsem_amd.vertsolve import VertSolve
    eng = Engine(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering="global"))
    c["eng"], c["en"] = eng, Energetics(eng, VertSolve(eng, 0.0))
    c["theta"] = ec.theta_L2(c)
    c["t"] = {k: eng.tensor(c[k]) for k in ("velx", "rho", "rt", "exner", "theta", "velz_v", "rho_v", "zv_v")}
    return c


def horizontal(c, **kw):
    t = c["t"]
    a = {k: kw.get(k, t[k]) for k in ("velx", "rho", "rt", "exner", "theta")}
    return c["en"].horizontal(a["velx"], a["rho"], a["rt"], a["exner"], a["theta"])


def compare(label, names, got, ref):
    errs = {n: abs(float(g) - ref[n][0]) / ref[n][1] for n, g in zip(names, got)}
    print("%s: |device - restatement| / S_abs  %s" % (label, "  ".join("%s %.2e" % (n, errs[n]) for n in names)))
    for n, g in zip(names, got):
        assert np.isfinite(float(g)) and ref[n][1] > 0, n
        assert errs[n] <= PARITY, (n, float(g), ref[n])
    return errs


def route_two(c):
    """the route the device could already take: eng.apply(UHMAT / WMAT, flags = VERT) followed by rowdot, interp_quad for int2"""
    from mimsem_amd.geom import gll_weights
    eng, t = c["eng"], c["t"]
    w = gll_weights(eng.mesh.n)
    ap = lambda op, x, f=None: eng.apply(op, x, f=f, lev0=0, scale=SCALE, flags=VERT)
    keh = 0.5 * eng.rowdot(ap("UHMAT", t["velx"], t["rho"]), t["velx"]).sum() / SCALE
    ie = (ec.CV / ec.CP) * eng.rowdot(t["rt"], ap("WMAT", t["exner"])).sum() / SCALE
    entr = 0.5 * eng.rowdot(ap("WMAT", t["rt"]), t["theta"]).sum() / SCALE
    wd = eng.tensor(eng.mesh.det * np.outer(w, w).ravel()[None, :])                     # det w_qx w_qy
    mass = (eng.interp_quad(2, t["rho"]) * wd[None]).sum()
    return [float(v) for v in (keh, ie, entr, mass)]


@pytest.fixture(scope="module")
def case(oracle):
    c = build(ec.make_case())
    c["ref_h"], c["ref_c"] = ec.restate_horizontal(c), ec.restate_column(c)
    return c


@pytest.fixture(scope="module")
def box(oracle):
    c = build(ec.make_box_case(oracle))
    c["ref_h"], c["ref_c"] = ec.restate_horizontal(c), ec.restate_column(c)
    return c


# ---- 1. the eight sums against the restatement (p = 3 sphere: 72 units, the last block partial) ----------------------------------------
def test_eight_sums_match_the_restatement(case):
    t = case["t"]
    compare("horizontal p3 sphere", ec.HORIZ, horizontal(case).tolist(), case["ref_h"])
    compare("column     p3 sphere", ec.COLUMN, case["en"].column(t["velz_v"], t["rho_v"], t["zv_v"]).tolist(), case["ref_c"])


# ---- 2. the fused horizontal sums against apply + rowdot / interp_quad -----------------------------------------------------------------
def test_fused_sums_match_the_composed_route(case):
    got, two = horizontal(case).tolist(), route_two(case)
    errs = [abs(g - w) / case["ref_h"][n][1] for n, g, w in zip(ec.HORIZ, got, two)]
    print("fused kernel vs apply + rowdot / interp_quad, / S_abs: %s" % "  ".join("%s %.2e" % (n, e) for n, e in zip(ec.HORIZ, errs)))
    assert max(errs) <= PARITY
    compare("composed route p3 sphere", ec.HORIZ, two, case["ref_h"])


# ---- 3. determinism, one level, strided rows ---------------------------------------------------------------------------------------------
def test_same_bits_one_level_and_strided_rows(case):
    t, nk = case["t"], case["nk"]
    a = horizontal(case)
    assert torch.equal(a, horizontal(case))
    one = {k: t[k][:1] for k in ("velx", "rho", "rt", "exner", "theta")}
    compare("level 0 alone", ec.HORIZ, horizontal(case, **one).tolist(), ec.restate_horizontal(case, levels=[0]))
    assert not torch.equal(horizontal(case, **one), a)
    wide = {}
    for k in one:                                    # rows 0, 2, 4 of a 2 nk-row array: level stride 2 n, the rows between hold garbage
        big = torch.full((2 * nk, t[k].shape[1]), 1.0e30, dtype=torch.float64, device=t[k].device)
        big[::2] = t[k]
        wide[k] = big[::2]
        assert not wide[k].is_contiguous() and wide[k].stride(0) == 2 * t[k].shape[1]
    assert torch.equal(horizontal(case, **wide), a)
    col = lambda: case["en"].column(t["velz_v"], t["rho_v"], t["zv_v"])
    assert torch.equal(col(), col())


# ---- 4. another lane layout: p = 4 periodic box (25 points per element on 32 lanes, 18 units in 3 blocks) --------------------------------
def test_eight_sums_on_a_p4_box(box):
    """the restatement comes from the oracle patch built on the box metric (element matrices; the case has no dense global matrices)"""
    t = box["t"]
    compare("horizontal p4 box", ec.HORIZ, horizontal(box).tolist(), box["ref_h"])
    compare("column     p4 box", ec.COLUMN, box["en"].column(t["velz_v"], t["rho_v"], t["zv_v"]).tolist(), box["ref_c"])
    errs = [abs(g - w) / box["ref_h"][n][1] for n, g, w in zip(ec.HORIZ, horizontal(box).tolist(), route_two(box))]
    print("p4 box, fused kernel vs composed route / S_abs: %s" % "  ".join("%.2e" % e for e in errs))
    assert max(errs) <= PARITY


def test_order_6_against_the_composed_route():
    """one element per lane group of 64 (49 points): the header says every order works; no dense restatement at this order, so the composed
    device route is the reference here and S_abs is the sum itself (all four horizontal terms are sums of positive contributions)"""
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
    c = dict(topos=topos, geoms=geoms, nk=nk)
    c["velx"] = r.standard_normal((nk, cs.nDofs1G))
    for k, (lo, hi) in dict(rho=(0.8, 1.2), rt=(290, 310), exner=(900, 1000), theta=(290, 310)).items():
        c[k] = r.uniform(lo, hi, (nk, cs.nDofs2G))
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.energetics import Energetics
    from mimsem_amd.vertsolve import VertSolve
    eng = Engine(DeviceMesh(topos, geoms, nk=nk, numbering="global"))
    c["eng"], c["en"] = eng, Energetics(eng, VertSolve(eng, 0.0))
    c["t"] = {k: eng.tensor(c[k]) for k in ("velx", "rho", "rt", "exner", "theta")}
    got, two = horizontal(c).tolist(), route_two(c)
    errs = [abs(g - w) / abs(w) for g, w in zip(got, two)]
    print("order 6, fused kernel vs composed route, relative: %s" % "  ".join("%.2e" % e for e in errs))
    assert all(w > 0 for w in two) and max(errs) <= PARITY


# ---- 5. error paths ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(case):
    eng, t, nk = case["eng"], case["t"], case["nk"]
    fn = eng.L.mimsem_euler_energetics_horiz
    out = torch.full((4,), 7.0, dtype=torch.float64, device=eng.device)
    names = ("velx", "rho", "rt", "exner", "theta")
    p = {k: C.c_void_p(t[k].data_ptr()) for k in names}
    s = {k: t[k].stride(0) for k in names}
    op = C.c_void_p(out.data_ptr())

    def call(ctx=eng.ctx, nlev=nk, out_=op, **null):
        a = []
        for k in names:
            a += [None if k in null else p[k], s[k]]
        return fn(ctx, nlev, *a, out_)
    assert call(ctx=None) == ERR_ARG
    assert call(out_=None) == ERR_ARG
    for k in names:
        assert call(**{k: True}) == ERR_ARG, k
    for nlev in (0, -1, nk + 1):
        assert call(nlev=nlev) == ERR_ARG, nlev
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))                                       # nothing written
    assert call() == 0 and call(nlev=1) == 0
    torch.cuda.synchronize()
    assert float(out[3]) > 0 and not torch.equal(out, torch.full_like(out, 7.0))
    from mimsem_amd._lib import MimsemError
    with pytest.raises(MimsemError):
        case["en"].horizontal(t["velx"], t["rho"][:2], t["rt"], t["exner"], t["theta"])     # row counts differ: caught before the C call


# ---- 6. diagnostics: recorded and replayed, the twelve numbers ---------------------------------------------------------------------------
def test_diagnostics_eager_and_replayed(case):
    from mimsem_amd.energetics import FIELDS, Energetics
    from mimsem_amd.horizsolve import HorizSolve
    from mimsem_amd.vertsolve import VertSolve
    eng, t, nk = case["eng"], case["t"], case["nk"]
    hs, vs = HorizSolve(eng), VertSolve(eng, 0.0)
    hs.k2i_dev = eng.tensor(np.array([3.25]))[0]                     # what momentum_rhs_ec / solve_schur_eta leave behind
    vs.k2i_z = -1.5
    en = Energetics(eng, vs, hs).set_geopotential(t["zv_v"])
    velx = t["velx"].clone()
    args = (velx, t["velz_v"], t["rho"], t["rt"], t["exner"])
    vals = en.diagnostics(*args)
    assert isinstance(vals, list) and len(vals) == 12 and all(isinstance(v, float) for v in vals)
    d = dict(zip(FIELDS, vals))
    ref = dict(case["ref_h"]); ref.update(case["ref_c"])
    compare("diagnostics (theta diagnosed on the device)", ec.HORIZ + ec.COLUMN, [d[n] for n in ec.HORIZ + ec.COLUMN], ref)
    assert d["k2i"] == 3.25 and d["k2i_z"] == -1.5 and d["i2k"] == 0.0 and d["i2k_z"] == 0.0
    want = float(case["rho"].sum())
    print("mass %.16g  rho.sum() %.16g  relative difference %.2e" % (vals[10], want, abs(vals[10] - want) / want))
    assert abs(vals[10] - want) <= 1e-13 * want
    eager = en.diagnostics(*args, read=False).clone()
    assert eager.tolist() == vals
    g, out = eng.capture(lambda: en.diagnostics(*args, read=False))
    out.zero_()
    g.replay(); torch.cuda.synchronize()
    assert torch.equal(out, eager)
    velx.mul_(2.0)                                                    # the recording reads its inputs anew: keh is quadratic in velx
    g.replay(); torch.cuda.synchronize()
    assert torch.equal(out, en.diagnostics(*args, read=False))
    assert abs(float(out[0]) / float(eager[0]) - 4.0) < 1e-12 and torch.equal(out[1:], eager[1:])
    assert Energetics.write_line is not None
