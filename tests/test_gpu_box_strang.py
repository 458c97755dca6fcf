"""BoxEuler.strang (mimsem_amd/euler.py) against the numpy restatement of the box twin's Euler::Strang in tests/box_strang_case.py (pinned on
the CPU by tests/test_box_strang_cpu.py): two consecutive steps with do_visc = False -- the first with uuz = 0 and the forward predictor, the
second with the leapfrog predictor, uuz from the carried velocity and a uz_prev that differs from uz -- every field and the twelve
diagnostics; the fused against the composed forcing; and the pieces of scripts/run_bubble.py on a small bubble.

Both sides run a FIXED Newton count (box_strang_case.NITS iterations, tol = 0).  The bars per field live in box_strang_case.BARS (relative
L2 observed on an MI355X against the restatement x 10, rounded up to a power of ten, none above CAP = 1e-8); the sums of the diagnostics are
held to the largest field bar of their step relative to S_abs, k2i and k2i_z -- signed sums -- to 1e-10 relative to the sum of the
magnitudes, the bar of tests/test_gpu_energetics.py for such sums."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import box_strang_case as bc
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
FIELDS, CAP, BARS = bc.FIELDS, bc.CAP, bc.BARS
SUMS = ("keh", "kev", "pe", "ie", "k2p", "p2k", "mass", "entr")
PARITY = 1e-10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_euler(c, **kw):
    from mimsem_amd.euler import BoxEuler
    eng, dm = c["eng"], c["eng"].mesh
    g, = c["geoms"]
    levs = np.zeros((c["nk"] + 1, dm.nq))
    levs[:, np.searchsorted(dm.gidq, g.loc0[np.arange(g.n0)])] = g.levs
    return BoxEuler(eng, bc.DT, levs, c["coords"][dm.gidq], lx=c["lx"], newton_maxit=bc.NITS, newton_tol=0.0, do_visc=False, **kw)


def compare(label, got, want, bars):
    errs = {n: rel_l2(g.cpu().numpy(), w) for n, g, w in zip(FIELDS, got, want)}
    print("%s: |device - restatement| / |restatement|  %s" % (label, "  ".join("%s %.2e" % (n, errs[n]) for n in FIELDS)))
    for n, g in zip(FIELDS, got):
        assert bool(torch.isfinite(g).all()), n
        assert bars[n] <= CAP and errs[n] < bars[n], (label, n, errs[n], bars[n])
    return errs


@pytest.fixture(scope="module")
def case(oracle):
    """the case, its engine, two restated steps (with the twelve numbers of each) and two device steps"""
    from mimsem_amd.device import DeviceMesh, Engine
    c = bc.make_case(oracle)
    c["eng"] = Engine(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering="global"))
    R, st = bc.BoxRestatement(c), c["state"]
    c["ref"], c["ref_diag"] = [], []
    for _ in range(2):
        st = R.step(*st)
        c["ref"].append(st)
        c["ref_diag"].append(R.diagnostics(st))
    c["t0"] = tuple(c["eng"].tensor(np.array(a)) for a in c["state"])
    eu, st, c["dev"] = make_euler(c), c["t0"], []
    for _ in range(2):
        out = eu.strang(*st)
        st = out[:5]
        c["dev"].append(dict(state=st, values=out[5], u_prev=eu.u_prev, u_curr=eu.u_curr, uz=eu.uz, uz_prev=eu.uz_prev))
    c["euler"] = eu
    return c


def test_two_steps_match_the_restatement(case):
    eu = case["euler"]
    assert eu.steps == 2 and eu.redone == 0 and not eu.first_step and eu.horiz.fused_forcing == type(eu).FUSED_FORCING
    for i in (0, 1):
        compare("box step %d" % (i + 1), case["dev"][i]["state"], case["ref"][i], BARS[i + 1])
    d = case["dev"]
    assert d[0]["u_prev"] is None and torch.equal(d[0]["u_curr"], case["t0"][0])
    assert torch.equal(d[1]["u_prev"], case["t0"][0]) and torch.equal(d[1]["u_curr"], d[0]["state"][0])     # the leapfrog's u_prev
    assert torch.equal(d[1]["uz_prev"], d[0]["uz"]) and not torch.equal(d[1]["uz_prev"], d[1]["uz"])          # :1347-1349
    assert len(eu.vert.history) == bc.NITS and "rt" in eu.vert.history[-1]                                   # solve_schur_2, the fixed count
    assert eu.vert.theta_h.shape[1] == (case["nk"] + 1) * case["eng"].n2e                                    # theta on the interfaces


def test_the_twelve_diagnostics_of_each_step(case):
    from mimsem_amd.energetics import FIELDS as LINE
    for i in (0, 1):
        vals = case["dev"][i]["values"]
        assert isinstance(vals, list) and len(vals) == 12
        d, ref = dict(zip(LINE, vals)), case["ref_diag"][i]
        bar = max(BARS[i + 1].values())
        errs = {n: abs(d[n] - ref[n][0]) / ref[n][1] for n in SUMS}
        print("box step %d diagnostics: |device - restatement| / S_abs  %s" % (i + 1, "  ".join("%s %.2e" % (n, errs[n]) for n in SUMS)))
        for n in SUMS:
            assert ref[n][1] > 0 and errs[n] < bar, (i, n, d[n], ref[n])
        for n in ("k2i", "k2i_z"):                                               # signed sums: relative to the sum of the magnitudes
            e = abs(d[n] - ref[n][0]) / ref[n][1]
            print("box step %d %s %.6e, restated %.6e, |difference| / S_abs %.2e" % (i + 1, n, d[n], ref[n][0], e))
            assert ref[n][0] != 0.0 and e < PARITY, (i, n)
        assert d["i2k"] == 0.0 and d["i2k_z"] == 0.0
    # the entropy is the box's own, of stage 1's theta_0: not the sphere's 1/2 theta . M2 rt that Energetics puts in that slot
    eu, st = case["euler"], case["dev"][1]["state"]
    assert abs(eu.energetics.diagnostics(*st)[11] - case["dev"][1]["values"][11]) > 1e-6 * abs(case["dev"][1]["values"][11])


def test_fused_and_composed_forcing_give_the_same_step(case, monkeypatch):
    from mimsem_amd.euler import BoxEuler
    outs = {}
    for fused in (True, False):
        monkeypatch.setattr(BoxEuler, "FUSED_FORCING", fused)
        eu = make_euler(case)
        assert eu.horiz.fused_forcing is fused
        st = case["t0"]
        for i in (0, 1):
            st = eu.strang(*st, diagnostics=False)[:5]
            compare("box step %d, FUSED_FORCING = %s" % (i + 1, fused), st, case["ref"][i], BARS[i + 1])
        outs[fused] = st
    for n, a, b in zip(FIELDS, outs[True], outs[False]):
        print("fused vs composed %s %.2e" % (n, rel_l2(a.cpu().numpy(), b.cpu().numpy())))
    assert not torch.equal(outs[True][0], outs[False][0])                        # two routes, not one


def test_orders_above_four_and_strang_ec_are_refused(case):
    from mimsem_amd.euler import BoxEuler
    with pytest.raises(NotImplementedError):
        case["euler"].strang_ec(*case["t0"])

    class Five:                                                                  # (the order is read before anything else)
        class mesh:
            n = 5
    with pytest.raises(NotImplementedError):
        BoxEuler(Five, bc.DT, None, None)


def test_run_dump_and_load(case, tmp_path):
    eu = make_euler(case)
    st = eu.run(case["t0"], 2, dump_every=2, outdir=str(tmp_path))
    for n, a, d in zip(FIELDS, st, case["dev"][1]["state"]):
        assert torch.equal(a, d), n
    assert eu.steps == 2 and eu.step == 1 and len((tmp_path / "energetics.dat").read_text().splitlines()) == 2
    nk = case["nk"]
    names = sorted(p.name for p in tmp_path.iterdir() if p.suffix == ".vec")
    want = {"velocity_h": nk, "density": nk, "rhoTheta": nk, "exner": nk, "velocity_z": nk - 1, "theta": nk + 1}
    assert len(names) == sum(want.values()) and not [p for p in tmp_path.iterdir() if p.suffix == ".npy"]
    assert all(sum(n.startswith(f + "_") for n in names) == k for f, k in want.items())
    back = make_euler(case).load(1, str(tmp_path))
    for n, a, b in zip(FIELDS, back, st):
        assert torch.equal(a, b), n


def test_a_small_bubble_runs(tmp_path):
    """the pieces of scripts/run_bubble.py on a p = 3, 2 x 2, nk = 6 bubble for two steps at the driver's dt: finite fields, Newton converged,
    mass conserved to round-off, at most one step redone"""
    spec = importlib.util.spec_from_file_location("run_bubble", os.path.join(ROOT, "scripts", "run_bubble.py"))
    rb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rb)
    from mimsem_amd.energetics import FIELDS as LINE
    eng, eu = rb.make_box_euler(3, 2, 6, 0.01)
    assert eu.horiz.do_visc is False and eu.horiz.thickness == 250.0
    state = eu.initial_state()
    assert not bool(state[0].any()) and not bool(state[1].any())                 # at rest
    lines, its = [], []
    st = eu.run(state, 2, outdir=str(tmp_path), on_step=lambda step, v: (lines.append(v), its.append(len(eu.vert.history))))
    assert all(bool(torch.isfinite(a).all()) for a in st)
    assert eu.steps == 2 and eu.redone <= 1
    h = eu.vert.history[-1]
    print("bubble: Newton iterations %s, last norms %s" % (its, "  ".join("%s %.2e" % kv for kv in h.items())))
    assert max(its) < eu.newton_maxit and all(h[k] < eu.newton_tol for k in ("exner", "rho", "rt"))
    im = LINE.index("mass")
    drift = abs(lines[1][im] - lines[0][im]) / lines[0][im]
    print("bubble: mass %.16e -> %.16e, relative drift %.2e" % (lines[0][im], lines[1][im], drift))
    assert drift < 1e-13
    assert bool(st[1].abs().max() > 0)                                           # the bubble rises
