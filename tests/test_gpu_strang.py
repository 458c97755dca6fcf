"""Euler.strang_ec (mimsem_amd/euler.py) against the numpy restatement of Euler::Strang_ec in tests/strang_case.py (pinned on the CPU by
tests/test_strang_cpu.py): two steps (the second takes the leapfrog branch and a uz_prev that differs from uz), a first step with the
Held-Suarez forcing, a step that misses a check and redoes itself, and the fused against the composed Bernoulli function.

Both sides run a FIXED Newton count (strang_case.NITS iterations, tol = 0).  A step chains about two dozen component evaluations, each held
to 1e-10 against LU-solved restatements, so the bars are not derived: each is the observed relative L2 error x 10 rounded up to a power
of ten, and none may exceed 1e-8 (CAP).  Observed on an MI355X (relative L2 against the restatement; dt = 0.5 moves rho by a small fraction
of itself, so most of its entries agree to the last bit):
                          velx      velz      rho       rt        exner
    step 1                6.32e-16  2.25e-15  7.53e-18  2.51e-15  4.33e-16
    step 2                1.15e-15  3.14e-15  1.98e-17  4.61e-15  1.05e-15
    step 1, Held-Suarez   6.64e-16  2.35e-15  5.02e-18  2.58e-15  4.45e-16     (held to the bars of step 1)
    step 2, forced miss   1.15e-15  3.14e-15  1.98e-17  4.61e-15  1.05e-15     (held to the bars of step 2)
    energetics / S_abs    step 1: keh 7.3e-16 ie 6.5e-16 entr 1.2e-15, pe = mass = 0; step 2: keh 1.3e-15 ie 1.3e-15 entr 2.3e-15
    k2i / S_abs           step 1: 9.7e-16, step 2: 4.8e-15 (bar 1e-10, that of the energetics sums)
    fused vs composed Bernoulli, step 1: velx 4.1e-19, velz 9.8e-18, rho = rt = exner = 0
"""
import numpy as np
import pytest
import torch

from tests import strang_case as sc
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
FIELDS = ("velx", "velz", "rho", "rt", "exner")
CAP = 1e-8
BARS = {1: dict(velx=1e-14, velz=1e-13, rho=1e-16, rt=1e-13, exner=1e-14),        # observed x 10, rounded up to a power of ten
        2: dict(velx=1e-13, velz=1e-13, rho=1e-15, rt=1e-13, exner=1e-13)}
ENERGY = ("keh", "ie", "pe", "mass", "entr")
PARITY = 1e-10           # tests/test_gpu_energetics.py (PARITY): sums relative to S_abs


def make_euler(c, **kw):
    from mimsem_amd.euler import Euler
    eng, dm = c["eng"], c["eng"].mesh
    levs = np.zeros((c["nk"] + 1, dm.nq))
    for g in c["geoms"]:
        levs[:, np.searchsorted(dm.gidq, g.loc0[np.arange(g.n0)])] = g.levs
    if kw.get("hs_forcing"):
        kw["hs_lat"] = eng.tensor(np.ascontiguousarray(c["lat"]))
    return Euler(eng, sc.DT, levs, c["gd"].xq[dm.gidq], newton_maxit=sc.NITS, newton_tol=0.0, **kw)


def compare(label, got, want, bars):
    errs = {n: rel_l2(g.cpu().numpy(), w) for n, g, w in zip(FIELDS, got, want)}
    print("%s: |device - restatement| / |restatement|  %s" % (label, "  ".join("%s %.2e" % (n, errs[n]) for n in FIELDS)))
    for n, g in zip(FIELDS, got):
        assert bool(torch.isfinite(g).all()), n
        assert bars[n] <= CAP and errs[n] < bars[n], (label, n, errs[n], bars[n])
    return errs


@pytest.fixture(scope="module")
def case(oracle):
    """the case, its engine, two restated steps (with the energetics of each new state) and two device steps"""
    from mimsem_amd.device import DeviceMesh, Engine
    c = sc.make_case()
    c["eng"] = Engine(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering="global"))
    R, st = sc.Restatement(c), c["state"]
    c["ref"] = []
    c["ref_k2i"] = []
    for _ in range(2):
        st = R.step(*st)
        c["ref"].append(st)
        c["ref_k2i"].append((R.k2i, R.k2i_abs))
    c["t0"] = tuple(c["eng"].tensor(a) for a in c["state"])
    eu, st, c["dev"] = make_euler(c), c["t0"], []
    for _ in range(2):
        out = eu.strang_ec(*st)
        st = out[:5]
        c["dev"].append(dict(state=st, values=out[5], u_prev=eu.u_prev, u_curr=eu.u_curr, uz=eu.uz, uz_prev=eu.uz_prev,
                             again=eu.energetics.diagnostics(*st)))
    c["euler"] = eu
    return c


def test_two_steps_match_the_restatement(case):
    eu = case["euler"]
    assert eu.steps == 2 and eu.redone == 0 and not eu.first_step and eu.horiz.fused_phi == type(eu).FUSED_PHI
    for i in (0, 1):
        compare("step %d" % (i + 1), case["dev"][i]["state"], case["ref"][i], BARS[i + 1])
    d = case["dev"]
    assert d[0]["u_prev"] is None and torch.equal(d[0]["u_curr"], case["t0"][0])
    assert torch.equal(d[1]["u_prev"], case["t0"][0]) and torch.equal(d[1]["u_curr"], d[0]["state"][0])     # the leapfrog's u_prev
    assert torch.equal(d[1]["uz_prev"], d[0]["uz"]) and not torch.equal(d[1]["uz_prev"], d[1]["uz"])          # :1407-1409
    assert len(eu.vert.history) == sc.NITS                                # the fixed Newton count


def test_energetics_line_of_each_step(case):
    from mimsem_amd.energetics import FIELDS as LINE
    for i in (0, 1):
        vals = case["dev"][i]["values"]
        assert isinstance(vals, list) and len(vals) == 12
        assert vals == case["dev"][i]["again"]                                                   # the same bits as a call right after
        ref = sc.energetics(case, case["ref"][i])
        d = dict(zip(LINE, vals))
        bar = max(BARS[i + 1].values())
        errs = {n: abs(d[n] - ref[n][0]) / ref[n][1] for n in ENERGY}
        print("step %d energetics: |device - restatement| / S_abs  %s" % (i + 1, "  ".join("%s %.2e" % (n, errs[n]) for n in ENERGY)))
        for n in ENERGY:
            assert ref[n][1] > 0 and errs[n] < bar, (i, n, d[n], ref[n])
        assert d["i2k"] == 0.0 and d["i2k_z"] == 0.0 and np.isfinite(d["k2i_z"])
        # k2i is that of stage 3's momentum_rhs_ec with Fk of the last transport evaluation (eul/HorizSolve.cpp:704-708): a signed sum, so
        # relative to S_abs, at the bar tests/test_gpu_energetics.py holds such sums to
        k2i, k2i_abs = case["ref_k2i"][i]
        e = abs(d["k2i"] - k2i) / k2i_abs
        print("step %d k2i %.6e, restated %.6e, |difference| / S_abs %.2e" % (i + 1, d["k2i"], k2i, e))
        assert k2i != 0.0 and e < PARITY


def test_first_step_with_held_suarez_forcing(case):
    R = sc.Restatement(case, hs_forcing=True)
    want = R.step(*case["state"])
    eu = make_euler(case, hs_forcing=True)
    out = eu.strang_ec(*case["t0"], diagnostics=False)
    assert out[5] is None
    compare("step 1, Held-Suarez", out[:5], want, BARS[1])
    assert rel_l2(want[0], case["ref"][0][0]) > 1e-9                     # the forcing is felt


def test_a_missed_check_redoes_the_step(case):
    eu = make_euler(case)
    st = eu.strang_ec(*case["t0"], diagnostics=False)[:5]
    assert eu.redone == 0 and eu.vort.m_its > 1
    eu.vort.m_its = 1                                                    # one PCG iteration: the check of the step must fail
    out = eu.strang_ec(*st, diagnostics=False)
    assert eu.redone == 1 and eu.vort.missed == 1 and eu.vort.m_its == 0 and eu.steps == 2
    compare("step 2 after a forced miss", out[:5], case["ref"][1], BARS[2])
    d = case["dev"][1]                                                   # the unforced run
    assert torch.equal(eu.u_prev, d["u_prev"]) and torch.equal(eu.u_curr, st[0])
    for name in ("uz", "uz_prev"):
        e = rel_l2(getattr(eu, name).cpu().numpy(), d[name].cpu().numpy())
        print("forced miss: %s against the unforced run %.2e" % (name, e))
        assert e < max(BARS[2].values()), name


def test_fused_and_composed_bernoulli_give_the_same_step(case):
    outs = {}
    for fused in (True, False):
        eu = make_euler(case)
        eu.horiz.fused_phi = fused
        outs[fused] = eu.strang_ec(*case["t0"], diagnostics=False)[:5]
        compare("step 1, fused_phi = %s" % fused, outs[fused], case["ref"][0], BARS[1])
    for n, a, b in zip(FIELDS, outs[True], outs[False]):
        e = rel_l2(a.cpu().numpy(), b.cpu().numpy())
        print("fused vs composed %s %.2e" % (n, e))
        assert e < BARS[1][n], n
    assert not torch.equal(outs[True][0], outs[False][0])                # two routes, not one


def test_sharded_engines_are_refused(case):
    from mimsem_amd.euler import Euler

    class Sharded:
        halo = object()
    with pytest.raises(NotImplementedError):
        Euler(Sharded(), sc.DT, None, None)
