"""The thermal shallow-water step with its host in C++ (mimsem_amd/host/mimsem_thermalsw.hpp: src::ThermalSW_EEC_2, driven by
tests/cpp/test_tsw.cpp, GalewskyTSW_2's main): against the dense oracle, the config-3 fixture, the Python host (mimsem_amd.thermalsw),
recorded against eager, a forced missed check, and the invariants over 20 steps."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.helpers import rel_l2
from tests.test_gpu_elem_block_pc import sphere_engine
from tests.test_gpu_tsw import INVARIANTS, device_sphere, from_eng

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from mimsem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    out = str(tmp_path_factory.mktemp("tsw") / "test_tsw")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "test_tsw.cpp"), "-o", out,
                           "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip", "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return out


def run_cpp(exe, tmp_path, eng, T, dt, nsteps, tag="run", use_graph=True, m1h_its=16, quad=None, state=None):
    """one run of test_tsw on the engine's mesh (global numbering): the results as numpy arrays in the engine's numbering"""
    from mimsem_amd.workloads import read_arrays, write_tsw_case
    case, res = str(tmp_path / (tag + ".case")), str(tmp_path / (tag + ".out"))
    c = lambda t: t.detach().cpu().numpy()
    write_tsw_case(case, eng.mesh, c(T.fg), dt, nsteps, use_graph=use_graph, m1h_its=m1h_its,
                   quad=None if quad is None else [c(x) for x in quad], state=None if state is None else [c(x) for x in state])
    p = subprocess.run([exe, case, res], capture_output=True, text=True, timeout=600)
    print(p.stdout.strip(), p.stderr.strip())
    assert p.returncode == 0 and "OK" in p.stdout
    r = read_arrays(res)
    r["inv"] = r["inv"].reshape(-1, 6)
    return r


def python_host(pn, ne):
    from mimsem_amd.thermalsw import ThermalSW, galewsky_tsw
    eng, xq = sphere_engine(pn, ne)
    T = ThermalSW(eng, xq)
    quad = galewsky_tsw(torch.as_tensor(xq, device=eng.device))
    return eng, T, quad


def inv_dict(row):
    return dict(zip(INVARIANTS, row))


def test_one_step_against_dense_oracle(exe, tmp_path, oracle):
    """ne = 2, p = 3: init() and one solve_rk(30 s) against tests/tsw_oracle.py (dense matrices, direct solves)"""
    from mimsem_amd.thermalsw import ThermalSW, galewsky_tsw
    from tests.test_tsw_oracle import galewsky_state
    eng, O, xq = device_sphere(3, 2)
    T = ThermalSW(eng, xq)
    r = run_cpp(exe, tmp_path, eng, T, 30.0, 1, quad=galewsky_tsw(torch.as_tensor(xq, device=eng.device)))
    y0 = galewsky_state(O)
    y1 = O.solve_rk(*y0, 30.0)
    g = lambda name, form: from_eng(eng, form, torch.as_tensor(r[name]))
    errs = {n: rel_l2(g(n, f), want) for n, f, want in zip(("u0", "h0", "S0", "u1", "h1", "S1"), (1, 2, 2, 1, 2, 2), (*y0, *y1))}
    i_o = O.invariants(*y1)
    ierr = {k: abs(v - i_o[k]) / abs(i_o[k]) for k, v in inv_dict(r["inv"][1]).items() if k != "vorticity"}
    print("C++ host vs dense oracle: " + "  ".join("%s %.1e" % kv for kv in errs.items()))
    print("invariants after the step: " + "  ".join("%s %.1e" % kv for kv in ierr.items()))
    assert max(errs.values()) <= 1e-10, errs
    assert max(ierr.values()) <= 1e-10, ierr


def test_config3_step_matches_fixture(exe, tmp_path, golden_dir):
    """config 3 (24 x 24 x 6, p = 3): init() and one step against tests/golden/tsw_galewsky_p3_ne24.npz with the sketch comparison and the
    bars of tests/test_gpu_tsw.py::test_config3_step_matches_fixture"""
    from tests.helpers import sketch_rel_err
    z = np.load(os.path.join(golden_dir, "tsw_galewsky_p3_ne24.npz"))
    eng, T, quad = python_host(3, 24)
    r = run_cpp(exe, tmp_path, eng, T, float(z["dt"]), 1, quad=quad)
    errs = {}
    for name, form in zip(("u0", "h0", "S0", "u1", "h1", "S1"), (1, 2, 2, 1, 2, 2)):
        y = from_eng(eng, form, torch.as_tensor(r[name]))
        errs[name] = max(sketch_rel_err(y, z[name + "_sketch"], float(z[name + "_norm"])),
                         abs(np.linalg.norm(y) - float(z[name + "_norm"])) / float(z[name + "_norm"]))
    inv = inv_dict(r["inv"][1])
    ierr = {k: abs(inv[k] - z["inv1"][i]) / abs(z["inv1"][i]) for i, k in enumerate(INVARIANTS) if k != "vorticity"}
    print("C++ host, config 3 vs fixture: " + "  ".join("%s %.1e" % kv for kv in errs.items()))
    print("invariants vs fixture: " + "  ".join("%s %.1e" % kv for kv in ierr.items()))
    assert max(errs.values()) < 1e-10, errs
    assert max(ierr.values()) <= 1e-12, ierr


def test_ten_steps_match_python_host(exe, tmp_path):
    eng, T, quad = python_host(3, 4)
    x = T.init(*quad)
    for _ in range(10):
        x = T.solve_rk(*x, 30.0)
    r = run_cpp(exe, tmp_path, eng, T, 30.0, 10, quad=quad)
    errs = {n: rel_l2(r[n], t[0].cpu().numpy()) for n, t in zip(("u1", "h1", "S1"), x)}
    print("10 steps ne=4, C++ host vs Python host: " + "  ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) <= 1e-12, errs


def test_recorded_step_is_the_eager_step(exe, tmp_path):
    """three steps recorded (one eager warm-up, one recording, replays) and three eager: the same bits; one read per step"""
    eng, T, quad = python_host(3, 4)
    g = run_cpp(exe, tmp_path, eng, T, 30.0, 3, tag="graph", use_graph=True, quad=quad)
    e = run_cpp(exe, tmp_path, eng, T, 30.0, 3, tag="eager", use_graph=False, quad=quad)
    steps, reads, redone, recordings, nodes, _ = g["counters"]
    print("recorded step: %d graph nodes" % nodes)
    for n in ("u1", "h1", "S1"):
        assert np.array_equal(g[n], e[n]), n
    assert np.array_equal(g["inv"], e["inv"])
    assert nodes > 0 and recordings == 1 and reads == steps == 3 and redone == 0
    assert e["counters"][3] == 0 and e["counters"][4] == 0 and e["counters"][1] == 3


def test_forced_miss_redoes_the_step(exe, tmp_path):
    """m1h_its = 2 cannot reach the M1h tolerance: the first step misses its check and is redone by the adaptive solvers"""
    eng, T, quad = python_host(3, 4)
    a = run_cpp(exe, tmp_path, eng, T, 30.0, 1, tag="normal", quad=quad)
    b = run_cpp(exe, tmp_path, eng, T, 30.0, 1, tag="miss", m1h_its=2, quad=quad)
    errs = {n: rel_l2(b[n], a[n]) for n in ("u1", "h1", "S1")}
    print("forced miss vs normal run: " + "  ".join("%s %.1e" % kv for kv in errs.items()))
    assert b["counters"][2] == 1 and a["counters"][2] == 0
    assert max(errs.values()) <= 1e-10, errs


def test_invariants_over_20_steps_ne8(exe, tmp_path):
    """20 steps at ne = 8: mass drift at round-off; buoyancy, energy and entropy drift within twice the Python host's"""
    eng, T, quad = python_host(3, 8)
    x = T.init(*quad)
    d0 = T.invariants(*x)
    for _ in range(20):
        x = T.solve_rk(*x, 30.0)
    d20 = T.invariants(*x)
    r = run_cpp(exe, tmp_path, eng, T, 30.0, 20, quad=quad)
    c0, c20 = inv_dict(r["inv"][0]), inv_dict(r["inv"][-1])
    rel = lambda a, b, k: (a[k] - b[k]) / abs(b[k])
    for k in ("mass", "buoyancy", "energy", "entropy"):
        print("%-9s drift over 20 steps: C++ host %+.3e  Python host %+.3e" % (k, rel(c20, c0, k), rel(d20, d0, k)))
    assert abs(rel(c20, c0, "mass")) <= 1e-12
    for k in ("buoyancy", "energy", "entropy"):
        assert abs(rel(c20, c0, k)) <= 2.0 * abs(rel(d20, d0, k)) + 1e-15, k
