"""Euler::Strang with its host in C++ (mimsem_amd/host/mimsem_euler.hpp: mimsem_host::eul::Euler::Strang over VortDiag, HorizMomentum, Energetics,
HorizSolve's momentum_rhs / advection_rhs and VertSolve2, driven by tests/cpp/test_euler2.cpp) on the case of tests/strang_case.py (p = 3, ne = 2,
nk = 4, dt = 0.5, a fixed count of NITS Newton iterations): against the numpy restatement of the step (tests/strang2_case.py Restatement2),
against the Python host (Euler.strang) on the same two steps, the state the step carries, the energetics line with k2i, a first step with
Held-Suarez forcing, and a forced missed check that redoes the step.

Bars: relative L2 against the restatement per field and per step, 10 x the error observed on the MI355X rounded up to a power of ten (the
rule of tests/test_gpu_cpp_euler.py), none above CAP.  Between the two hosts: the sum of their bars.

CPU (not marked gpu): the driver compiles with plain g++ -std=c++17 -Wall -Werror, no HIP headers, and links against the C ABI."""
import os
import subprocess

import numpy as np
import pytest

from tests import strang2_case as s2c
from tests import strang_case as sc
from tests.helpers import rel_l2

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("velx", "velz", "rho", "rt", "exner")
CAP = 1e-8
PARITY = 1e-10           # tests/test_gpu_energetics.py (PARITY): sums relative to S_abs; k2i as tests/test_gpu_strang2.py holds it
# observed on the MI355X (|C++ host - restatement| / |restatement|):
#                         velx      velz      rho       rt        exner
#   step 1                6.32e-16  2.35e-15  1.55e-17  9.05e-18  3.64e-16
#   step 2                1.13e-15  2.26e-15  2.34e-17  1.55e-17  3.78e-16
#   step 1, Held-Suarez   6.44e-16  2.56e-15  1.12e-17  1.23e-17  3.56e-16     (held to the bars of step 1)
#   forced miss           the figures of steps 1 and 2 to the digits shown; all three switches on: velx 6.30e-16, the rest as step 1
#   the two hosts differ by at most 2.3e-16 (velx), rho = rt = exner bit-equal
#   energetics / S_abs    step 1: keh 6.1e-16 ie 1.3e-16 mass 1.9e-16 entr 2.6e-16, pe = 0; step 2: keh 1.1e-15; k2i / S_abs 6.2e-16, 9.5e-16
BARS = {1: dict(velx=1e-14, velz=1e-13, rho=1e-15, rt=1e-16, exner=1e-14),
        2: dict(velx=1e-13, velz=1e-13, rho=1e-15, rt=1e-15, exner=1e-14)}
ENERGY = ("keh", "ie", "pe", "mass", "entr")


def _build(out):
    from mimsem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "test_euler2.cpp"), "-o", out,
                           "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip", "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_driver_compiles_and_links(tmp_path):
    assert os.path.exists(_build(str(tmp_path / "test_euler2")))
    text = open(os.path.join(ROOT, "mimsem_amd", "host", "mimsem_euler.hpp")).read()
    assert "hip/hip_runtime" not in text and "void Strang(" in text


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("euler2") / "test_euler2"))


def run_cpp(exe, tmp, c, nsteps, tag, hs=False, vort_its=0, switches="phi"):
    """one run of test_euler2 from the start state of the case; switches: HorizSolve's during the step ("phi": the Python host's defaults,
    FUSED_PHI on and FUSED_HU off)"""
    from mimsem_amd.workloads import read_arrays, write_euler_case
    eng, dm = c["eng"], c["eng"].mesh
    levs = np.zeros((c["nk"] + 1, dm.nq))
    for g in c["geoms"]:
        levs[:, np.searchsorted(dm.gidq, g.loc0[np.arange(g.n0)])] = g.levs
    case, res = str(tmp / (tag + ".case")), str(tmp / (tag + ".out"))
    write_euler_case(case, dm, levs, c["gd"].xq[dm.gidq], c["state"], sc.DT, nsteps, hs_lat=c["lat"] if hs else None,
                     newton_maxit=sc.NITS, newton_tol=0.0, vort_its=vort_its, eng=eng)
    p = subprocess.run([exe, case, res, switches], capture_output=True, text=True, timeout=300)
    print(p.stdout.strip(), p.stderr.strip())
    assert p.returncode == 0 and "OK" in p.stdout
    r = read_arrays(res)
    shape = {"velx": (c["nk"], -1), "rho": (c["nk"], -1), "rt": (c["nk"], -1), "exner": (c["nk"], -1), "velz": c["state"][1].shape}
    for s in range(1, nsteps + 1):
        for n in FIELDS:
            r[n + str(s)] = r[n + str(s)].reshape(shape[n])
    return r


def state_of(r, s):
    return tuple(r[n + str(s)] for n in FIELDS)


def compare(label, got, want, bars):
    errs = {n: rel_l2(g, w) for n, g, w in zip(FIELDS, got, want)}
    print("%s: |C++ host - restatement| / |restatement|  %s" % (label, "  ".join("%s %.2e" % (n, errs[n]) for n in FIELDS)))
    for n, g in zip(FIELDS, got):
        assert np.isfinite(g).all(), n
        assert bars[n] <= CAP and errs[n] < bars[n], (label, n, errs[n], bars[n])
    return errs


@pytest.fixture(scope="module")
def case(oracle, exe, tmp_path_factory):
    """the case, its engine, two restated steps (with k2i of each), two steps of the Python host and two of the C++ host"""
    from mimsem_amd.device import DeviceMesh, Engine
    from tests.test_gpu_strang2 import make_euler
    c = sc.make_case()
    c["eng"] = Engine(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering="global"))
    R, st = s2c.Restatement2(c), c["state"]
    c["ref"], c["ref_k2i"] = [], []
    for _ in range(2):
        st = R.step(*st)
        c["ref"].append(st)
        c["ref_k2i"].append((R.k2i, R.k2i_abs))
    eu, st, c["py"] = make_euler(c), tuple(c["eng"].tensor(a) for a in c["state"]), []
    for _ in range(2):
        st = eu.strang(*st, diagnostics=False)[:5]
        c["py"].append(tuple(t.cpu().numpy() for t in st))
    c["tmp"] = tmp_path_factory.mktemp("euler2_runs")
    c["cpp"] = run_cpp(exe, c["tmp"], c, 2, "two")
    return c


@gpu
def test_two_steps_match_the_restatement(case):
    r = case["cpp"]
    for s in (1, 2):
        compare("step %d" % s, state_of(r, s), case["ref"][s - 1], BARS[s])
    assert list(r["counters"][:2]) == [2, 0]                              # two steps, no spurious redo
    assert r["counters"][2] > 1 and r["counters"][3] > 1 and r["counters"][4] == 0 and r["counters"][6] == 0
    for s in (1, 2):                                                      # solve_schur_2, the fixed count
        assert r["newton" + str(s)].size == 4 * sc.NITS and np.isfinite(r["newton" + str(s)]).all()
    assert list(r["per_step"].reshape(2, 4)[:, 0]) == [sc.NITS, sc.NITS]


@gpu
def test_same_fields_as_the_python_host(case):
    """two hosts, the same launches: each within its own bars of the restatement, so within their sum of each other"""
    for s in (1, 2):
        for n, a, b in zip(FIELDS, state_of(case["cpp"], s), case["py"][s - 1]):
            e = rel_l2(a, b)
            print("step %d  C++ host vs Python host  %s %.2e" % (s, n, e))
            assert e < BARS[s][n] + s2c.BARS[s][n], (s, n, e)


@gpu
def test_leapfrog_and_uz_prev_carry(case):
    r = case["cpp"]
    assert "u_prev1" not in r and np.array_equal(r["u_curr1"], case["state"][0].ravel())
    assert np.array_equal(r["u_prev2"], case["state"][0].ravel()) and np.array_equal(r["u_curr2"], r["velx1"].ravel())
    assert np.array_equal(r["uz_prev2"], r["uz1"]) and not np.array_equal(r["uz_prev2"], r["uz2"])            # :1187-1189


@gpu
def test_energetics_line_of_each_step(case):
    from mimsem_amd.energetics import FIELDS as LINE
    for s in (1, 2):
        vals = case["cpp"]["values" + str(s)]
        assert vals.size == 12 and np.isfinite(vals).all()
        d = dict(zip(LINE, vals))
        ref = sc.energetics(case, case["ref"][s - 1])
        bar = max(BARS[s].values())
        errs = {n: abs(d[n] - ref[n][0]) / ref[n][1] for n in ENERGY}
        print("step %d energetics: |C++ host - restatement| / S_abs  %s" % (s, "  ".join("%s %.2e" % (n, errs[n]) for n in ENERGY)))
        for n in ENERGY:
            assert ref[n][1] > 0 and errs[n] < bar, (s, n, d[n], ref[n])
        assert d["i2k"] == 0.0 and d["i2k_z"] == 0.0 and np.isfinite(d["k2i_z"]) and d["k2i_z"] != 0.0
        k2i, k2i_abs = case["ref_k2i"][s - 1]
        e = abs(d["k2i"] - k2i) / k2i_abs
        print("step %d k2i %.6e, restated %.6e, |difference| / S_abs %.2e" % (s, d["k2i"], k2i, e))
        assert k2i != 0.0 and e < PARITY


@gpu
def test_first_step_with_held_suarez_forcing(case, exe):
    want = s2c.Restatement2(case, hs_forcing=True).step(*case["state"])
    r = run_cpp(exe, case["tmp"], case, 1, "hs", hs=True)
    compare("step 1, Held-Suarez", state_of(r, 1), want, BARS[1])
    assert list(r["counters"][:2]) == [1, 0]
    assert rel_l2(r["velx1"], case["cpp"]["velx1"]) > 1e-9 and rel_l2(r["rt1"], case["cpp"]["rt1"]) > 100 * BARS[1]["rt"]   # both forcings are felt


@gpu
def test_a_forced_miss_redoes_the_step(case, exe):
    r = run_cpp(exe, case["tmp"], case, 2, "miss", vort_its=1)           # one PCG iteration: the check of step 1 must fail
    assert list(r["counters"][:2]) == [2, 1] and r["counters"][4] == 1
    assert r["counters"][2] == 0 and r["counters"][3] == 0               # adaptive afterwards
    for s in (1, 2):
        compare("step %d after a forced miss" % s, state_of(r, s), case["ref"][s - 1], BARS[s])


@gpu
def test_every_switch_gives_the_same_step(case, exe):
    """composed (no switch) and all three fused: the first step within the same bars"""
    for sw in ("none", "hu phi forcing"):
        r = run_cpp(exe, case["tmp"], case, 1, "sw_" + sw.replace(" ", "_"), switches=sw)
        compare("step 1, switches: %s" % sw, state_of(r, 1), case["ref"][0], BARS[1])
