"""Euler::Strang_ec with its host in C++ (mimsem_amd/host/mimsem_euler.hpp: mimsem_host::eul::Euler over VortDiag, HorizMomentum, Energetics,
HorizSolve and VertSolveEta, driven by tests/cpp/test_euler.cpp) on the case of tests/strang_case.py (p = 3, ne = 2, nk = 4, dt = 0.5, a fixed
count of NITS Newton iterations): against the numpy restatement of the step, against the Python host (mimsem_amd/euler.py) on the same two
steps, the state the step carries, the energetics line, Held-Suarez forcing, and a forced missed check.

Bars: relative L2 against the restatement per field and per step, 10 x the error observed on the MI355X rounded up to a power of ten (the
rule of tests/test_gpu_strang.py; the margin covers the reordering of sums between builds), none above CAP.  They are this host's own: its
composed Bernoulli function and its Chebyshev step counts are not the Python host's."""
import os
import subprocess

import numpy as np
import pytest

from tests import strang_case as sc
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("velx", "velz", "rho", "rt", "exner")
CAP = 1e-8
# observed on the MI355X (|C++ host - restatement| / |restatement|):
#   step 1  velx 6.25e-16  velz 2.25e-15  rho 7.53e-18  rt 2.51e-15  exner 4.33e-16
#   step 2  velx 1.14e-15  velz 3.13e-15  rho 1.98e-17  rt 4.62e-15  exner 1.05e-15
# (step 1 with Held-Suarez forcing: 6.59e-16  2.35e-15  5.02e-18  2.58e-15  4.42e-16; the two hosts differ by at most 2.3e-16)
BARS = {1: dict(velx=1e-14, velz=1e-13, rho=1e-16, rt=1e-13, exner=1e-14),
        2: dict(velx=1e-13, velz=1e-13, rho=1e-15, rt=1e-13, exner=1e-13)}
SUMS = ("keh", "ie", "entr", "mass", "kev", "k2p", "p2k", "pe")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from mimsem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    out = str(tmp_path_factory.mktemp("euler") / "test_euler")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "test_euler.cpp"), "-o", out,
                           "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip", "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return out


def run_cpp(exe, tmp, c, nsteps, tag, hs=False, vort_its=0, m1_steps=0):
    """one run of test_euler from the start state of the case: the arrays it wrote, in the engine's (global) numbering"""
    from mimsem_amd.workloads import read_arrays, write_euler_case
    eng, dm = c["eng"], c["eng"].mesh
    levs = np.zeros((c["nk"] + 1, dm.nq))
    for g in c["geoms"]:
        levs[:, np.searchsorted(dm.gidq, g.loc0[np.arange(g.n0)])] = g.levs
    case, res = str(tmp / (tag + ".case")), str(tmp / (tag + ".out"))
    write_euler_case(case, dm, levs, c["gd"].xq[dm.gidq], c["state"], sc.DT, nsteps, hs_lat=c["lat"] if hs else None,
                     newton_maxit=sc.NITS, newton_tol=0.0, vort_its=vort_its, m1_steps=m1_steps, eng=eng)
    p = subprocess.run([exe, case, res], capture_output=True, text=True, timeout=300)
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
    """the case, its engine, two restated steps, two steps of the Python host and two of the C++ host"""
    from mimsem_amd.device import DeviceMesh, Engine
    from tests.test_gpu_strang import make_euler
    c = sc.make_case()
    c["eng"] = Engine(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering="global"))
    R, st = sc.Restatement(c), c["state"]
    c["ref"], c["ref_k2i"] = [], []
    for _ in range(2):
        st = R.step(*st)
        c["ref"].append(st)
        c["ref_k2i"].append((R.k2i, R.k2i_abs))
    eu, st, c["py"] = make_euler(c), tuple(c["eng"].tensor(a) for a in c["state"]), []
    for _ in range(2):
        st = eu.strang_ec(*st, diagnostics=False)[:5]
        c["py"].append(tuple(t.cpu().numpy() for t in st))
    c["tmp"] = tmp_path_factory.mktemp("euler_runs")
    c["cpp"] = run_cpp(exe, c["tmp"], c, 2, "two")
    return c


def test_two_steps_match_the_restatement(case):
    r = case["cpp"]
    for s in (1, 2):
        compare("step %d" % s, state_of(r, s), case["ref"][s - 1], BARS[s])
    assert list(r["counters"][:2]) == [2, 0]                              # two steps, no spurious redo
    assert r["counters"][2] > 1 and r["counters"][3] > 1 and r["counters"][4] == 0 and r["counters"][6] == 0
    per = r["per_step"].reshape(2, 4)
    assert per[1, 2] == r["counters"][2] and per[1, 3] == r["counters"][3]      # step 2 ended on fixed-length interface solves


def test_same_fields_as_the_python_host(case):
    """two hosts, the same launches: each within its own bars of the restatement, so within their sum of each other"""
    from tests.test_gpu_strang import BARS as PY_BARS
    for s in (1, 2):
        for n, a, b in zip(FIELDS, state_of(case["cpp"], s), case["py"][s - 1]):
            e = rel_l2(a, b)
            print("step %d  C++ host vs Python host  %s %.2e" % (s, n, e))
            assert e < BARS[s][n] + PY_BARS[s][n], (s, n, e)


def test_leapfrog_carry(case):
    r = case["cpp"]
    assert "u_prev1" not in r and np.array_equal(r["u_curr1"], case["state"][0].ravel())
    assert np.array_equal(r["u_prev2"], case["state"][0].ravel()) and np.array_equal(r["u_curr2"], r["velx1"].ravel())
    assert np.array_equal(r["uz_prev2"], r["uz1"]) and not np.array_equal(r["uz_prev2"], r["uz2"])            # :1407-1409


def test_fixed_newton_count(case):
    r = case["cpp"]
    for s in (1, 2):
        assert r["newton" + str(s)].size == 4 * sc.NITS and np.isfinite(r["newton" + str(s)]).all()
    assert list(r["per_step"].reshape(2, 4)[:, 0]) == [sc.NITS, sc.NITS]


def test_energetics_line_of_each_step(case):
    from mimsem_amd.energetics import FIELDS as LINE
    for s in (1, 2):
        vals = case["cpp"]["values" + str(s)]
        assert vals.size == 12 and np.isfinite(vals).all()
        d = dict(zip(LINE, vals))
        ref = sc.energetics(case, case["ref"][s - 1])
        bar = max(BARS[s].values())
        errs = {n: abs(d[n] - ref[n][0]) / ref[n][1] for n in SUMS if ref[n][0] != 0.0}
        print("step %d energetics: |C++ host - restatement| / S_abs  %s" % (s, "  ".join("%s %.2e" % (n, e) for n, e in errs.items())))
        assert len(errs) >= 5
        for n, e in errs.items():
            assert e < bar, (s, n, d[n], ref[n])
        assert d["i2k"] == 0.0 and d["i2k_z"] == 0.0 and np.isfinite(d["k2i_z"])
        k2i, k2i_abs = case["ref_k2i"][s - 1]
        e = abs(d["k2i"] - k2i) / k2i_abs
        print("step %d k2i %.6e, restated %.6e, |difference| / S_abs %.2e" % (s, d["k2i"], k2i, e))
        assert k2i != 0.0 and e < bar


def hs_reference(case):
    """the restated first step under Held-Suarez forcing, made once"""
    if "hs_ref" not in case:
        case["hs_ref"] = sc.Restatement(case, hs_forcing=True).step(*case["state"])
    return case["hs_ref"]


def test_first_step_with_held_suarez_forcing(case, exe):
    want = hs_reference(case)
    r = run_cpp(exe, case["tmp"], case, 1, "hs", hs=True)
    compare("step 1, Held-Suarez", state_of(r, 1), want, BARS[1])
    assert list(r["counters"][:2]) == [1, 0]
    assert rel_l2(r["velx1"], case["cpp"]["velx1"]) > 1e-9               # the forcing is felt


def test_held_suarez_step_after_a_missed_m1_check(case, exe):
    """M1 cut to 4 Chebyshev steps: its check misses and the step is run again with the CG solvers -- under the forcing the CG on
    M1 + M1ray (MIMSEM_OP_UMAT_FRIC).  The CG stops at a relative residual of 1e-14 where the Chebyshev solves reach ~1e-16, so velx has a bar
    of its own by the same rule (observed 5.11e-15); the other fields (2.34e-15  5.02e-18  2.59e-15  4.41e-16) keep the step's"""
    want = hs_reference(case)
    r = run_cpp(exe, case["tmp"], case, 1, "hs_miss", hs=True, m1_steps=4)
    assert list(r["counters"][:2]) == [1, 1] and r["counters"][6] >= 1
    compare("step 1, Held-Suarez, after a missed M1 check", state_of(r, 1), want, dict(BARS[1], velx=1e-13))


def test_a_forced_miss_redoes_the_step(case, exe):
    r = run_cpp(exe, case["tmp"], case, 2, "miss", vort_its=1)           # one PCG iteration: the check of step 1 must fail
    assert list(r["counters"][:2]) == [2, 1] and r["counters"][4] == 1
    assert r["counters"][2] == 0 and r["counters"][3] == 0               # adaptive afterwards
    per = r["per_step"].reshape(2, 4)
    assert list(per[:, 1]) == [1, 1] and list(per[:, 2]) == [0, 0] and list(per[:, 3]) == [0, 0]
    for s in (1, 2):
        compare("step %d after a forced miss" % s, state_of(r, s), case["ref"][s - 1], BARS[s])
