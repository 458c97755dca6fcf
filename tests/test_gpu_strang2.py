"""Euler.strang (mimsem_amd/euler.py) against the numpy restatement of Euler::Strang in tests/strang2_case.py (pinned on the CPU by
tests/test_strang2_cpu.py): two steps (the second takes the leapfrog branch and a uz_prev that differs from uz), a first step with the
Held-Suarez forcing, a step that misses a check and redoes itself, the fused against the composed mass-flux right-hand side, and
Euler.run(integrator="strang") against the calls.

Both sides run a FIXED Newton count (strang_case.NITS iterations, tol = 0).  As in tests/test_gpu_strang.py the bars are not derived: each
is the relative L2 error observed against the restatement x 10 rounded up to a power of ten, and none may exceed 1e-8 (CAP); they live in
strang2_case.BARS because tests/test_strang2_cpu.py states its sensitivity conditions against them (the transport forcing moves the
stage-2 fields by 4.9e-6 .. 2.4e-5 and the step differs from Strang_ec's by 7.2e-6 .. 9.2e-2 per field: far above 100 x any bar).
Observed on an MI355X (relative L2 against the restatement):
                          velx      velz      rho       rt        exner
    step 1                6.32e-16  2.35e-15  1.55e-17  9.05e-18  3.64e-16
    step 2                1.13e-15  2.26e-15  2.34e-17  1.55e-17  3.78e-16
    step 1, Held-Suarez   6.38e-16  2.56e-15  1.12e-17  1.23e-17  3.56e-16     (held to the bars of step 1)
    step 2, forced miss   1.13e-15  2.26e-15  2.34e-17  1.55e-17  3.78e-16     (held to the bars of step 2)
    (rho and rt move by a small fraction of themselves at dt = 0.5, so most of their entries agree to the last bit)
    energetics / S_abs    step 1: keh 6.1e-16 ie 1.3e-16 mass 1.9e-16 entr 2.6e-16, pe = 0; step 2: keh 1.1e-15 ie 1.3e-16 entr 2.6e-16
    k2i / S_abs           step 1: 6.2e-16, step 2: 9.7e-16 (bar 1e-10, that of the energetics sums)
    FUSED_HU True vs False, step 1: velx 7.9e-18, velz = rho = rt = exner = 0 (the same bars; velx differs in bits)
"""
import numpy as np
import pytest
import torch

from tests import strang2_case as s2c
from tests import strang_case as sc
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
FIELDS = ("velx", "velz", "rho", "rt", "exner")
CAP, BARS = s2c.CAP, s2c.BARS
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
    """the case, its engine, two restated steps (with k2i of each) and two device steps"""
    from mimsem_amd.device import DeviceMesh, Engine
    c = sc.make_case()
    c["eng"] = Engine(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering="global"))
    R, st = s2c.Restatement2(c), c["state"]
    c["ref"], c["ref_k2i"] = [], []
    for _ in range(2):
        st = R.step(*st)
        c["ref"].append(st)
        c["ref_k2i"].append((R.k2i, R.k2i_abs))
    c["t0"] = tuple(c["eng"].tensor(a) for a in c["state"])
    eu, st, c["dev"] = make_euler(c), c["t0"], []
    for _ in range(2):
        out = eu.strang(*st)
        st = out[:5]
        c["dev"].append(dict(state=st, values=out[5], u_prev=eu.u_prev, u_curr=eu.u_curr, uz=eu.uz, uz_prev=eu.uz_prev,
                             again=eu.energetics.diagnostics(*st)))
    c["euler"] = eu
    return c


def test_two_steps_match_the_restatement(case):
    eu = case["euler"]
    assert eu.steps == 2 and eu.redone == 0 and not eu.first_step and eu.horiz.fused_hu == type(eu).FUSED_HU
    for i in (0, 1):
        compare("step %d" % (i + 1), case["dev"][i]["state"], case["ref"][i], BARS[i + 1])
    d = case["dev"]
    assert d[0]["u_prev"] is None and torch.equal(d[0]["u_curr"], case["t0"][0])
    assert torch.equal(d[1]["u_prev"], case["t0"][0]) and torch.equal(d[1]["u_curr"], d[0]["state"][0])     # the leapfrog's u_prev
    assert torch.equal(d[1]["uz_prev"], d[0]["uz"]) and not torch.equal(d[1]["uz_prev"], d[1]["uz"])          # :1187-1189
    assert len(eu.vert.history) == sc.NITS and "rt" in eu.vert.history[-1]                                   # solve_schur_2, the fixed count
    assert eu.vert.theta_h.shape[1] == (case["nk"] + 1) * case["eng"].n2e                                    # theta on the interfaces


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
        # k2i is that of stage 3's momentum_rhs with Fk of the last advection_rhs (eul/HorizSolve.cpp:560-563): a signed sum, so relative
        # to the sum of magnitudes, at the bar tests/test_gpu_energetics.py holds such sums to
        k2i, k2i_abs = case["ref_k2i"][i]
        e = abs(d["k2i"] - k2i) / k2i_abs
        print("step %d k2i %.6e, restated %.6e, |difference| / S_abs %.2e" % (i + 1, d["k2i"], k2i, e))
        assert k2i != 0.0 and e < PARITY


def test_first_step_with_held_suarez_forcing(case):
    R = s2c.Restatement2(case, hs_forcing=True)
    want = R.step(*case["state"])
    eu = make_euler(case, hs_forcing=True)
    out = eu.strang(*case["t0"], diagnostics=False)
    assert out[5] is None
    compare("step 1, Held-Suarez", out[:5], want, BARS[1])
    assert rel_l2(want[0], case["ref"][0][0]) > 1e-9 and rel_l2(want[3], case["ref"][0][3]) > 100 * BARS[1]["rt"]    # both forcings are felt


def test_a_missed_check_redoes_the_step(case):
    eu = make_euler(case)
    st = eu.strang(*case["t0"], diagnostics=False)[:5]
    assert eu.redone == 0 and eu.vort.m_its > 1
    eu.vort.m_its = 1                                                    # one PCG iteration: the check of the step must fail
    out = eu.strang(*st, diagnostics=False)
    assert eu.redone == 1 and eu.vort.missed == 1 and eu.vort.m_its == 0 and eu.steps == 2
    compare("step 2 after a forced miss", out[:5], case["ref"][1], BARS[2])
    d = case["dev"][1]                                                   # the unforced run
    assert torch.equal(eu.u_prev, d["u_prev"]) and torch.equal(eu.u_curr, st[0])
    for name in ("uz", "uz_prev"):
        e = rel_l2(getattr(eu, name).cpu().numpy(), d[name].cpu().numpy())
        print("forced miss: %s against the unforced run %.2e" % (name, e))
        assert e < max(BARS[2].values()), name


def test_fused_and_composed_flux_rhs_give_the_same_step(case, monkeypatch):
    from mimsem_amd.euler import Euler
    outs = {}
    for fused in (True, False):
        monkeypatch.setattr(Euler, "FUSED_HU", fused)
        eu = make_euler(case)
        outs[fused] = eu.strang(*case["t0"], diagnostics=False)[:5]
        assert eu.horiz.fused_hu is fused
        compare("step 1, FUSED_HU = %s" % fused, outs[fused], case["ref"][0], BARS[1])
    for n, a, b in zip(FIELDS, outs[True], outs[False]):
        print("fused vs composed %s %.2e" % (n, rel_l2(a.cpu().numpy(), b.cpu().numpy())))
    assert not torch.equal(outs[True][0], outs[False][0])                # two routes, not one


def test_run_with_the_strang_integrator_is_the_calls(case, tmp_path):
    eu = make_euler(case)
    st = eu.run(case["t0"], 2, outdir=str(tmp_path), integrator="strang")
    for n, a, d in zip(FIELDS, st, case["dev"][1]["state"]):
        assert torch.equal(a, d), n
    assert eu.steps == 2 and len((tmp_path / "energetics.dat").read_text().splitlines()) == 2
    with pytest.raises(ValueError):
        eu.run(case["t0"], 1, outdir=str(tmp_path), integrator="trapazoidal")
    # strang_ec stays the default of run(), and a different step
    ec = make_euler(case).run(case["t0"], 1, outdir=str(tmp_path / "ec"))
    assert rel_l2(ec[1].cpu().numpy(), case["ref"][0][1]) > 100 * BARS[1]["velz"]
