"""The whole shallow-water step and the HorizSolve right-hand sides at the benchmark's mesh sizes against the sparse mode of the numpy
oracles, through the fixtures tests/golden/make_step_fixtures.py wrote:

  * SWEqn::solve on bench.py's config 2 (Williamson-2, 16x16x6, dt 600 s, q from the mean state, 4 Picard iterations) and config 3
    (the Galewsky jet, 24x24x6, dt 360 s, upwinded q, 2 iterations): the Python host (mimsem_amd/sweqn.py, the timed fixed-length
    graphed path) and the C++ host (tests/cpp/test_sw.cpp, all four modes), from the device's start state, every field compared
    through its stored sketch (tests/helpers.py::sketch_rel_err).
  * HorizSolve on the config-4 sphere with 10 levels (nk * n1 = 622 080 rows in the C++ host's check-norm reductions): every output
    compared through its stored sketch (tests/helpers.py::sketch_rel_err), the inputs rebuilt bit for bit from the integer hash.

At these sizes the fixed-length Chebyshev solves run with the spectral intervals and lengths fitted to the mesh, which the ne = 2
parity tests never reach."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import sketch_rel_err

pytestmark = pytest.mark.gpu
SW_TOL = 1e-10          # fg, the start state and the state after the step: sketched relative L2 (tests/test_gpu_sweqn.py's tolerance)
STEP_TOL = 1e-8         # the step's increment u1 - u0, h1 - h0 (|du| / |u| ~ 3e-5 at config 3: SW_TOL on the state allows ~3e-6 here)
HIST_RTOL = 1e-6        # the Picard history |dx| / |x| per entry: a ratio of norms of increments ~1e-5 .. 1e-9 of the state
RHS_TOL = 1e-10         # HorizSolve outputs, sketched relative L2
HORIZ_FIXTURE = "horiz_p3_ne24_nk10.npz"


@pytest.fixture(scope="module", params=["sw2", "sw3"], ids=["config2", "config3"])
def sw_case(request, golden_dir):
    """one SW fixture and the Python host's step on its sphere.  The start state is the device's own init1 / init2 of the case's analytic
    fields (checked against the oracle's through the sketches); the oracle's start differs from it by round-off, which one step carries
    into u1 at about that size, far below SW_TOL"""
    import torch
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.sweqn import SWEqn
    from tests.golden.make_step_fixtures import SW_CASES, sw_initial_fields, sw_sphere
    fname, ne, dt, nits, q_exact, ic = SW_CASES[request.param]
    d = dict(np.load(os.path.join(golden_dir, fname)))
    assert (int(d["ne"]), float(d["dt"]), int(d["nits"]), bool(d["q_exact"])) == (ne, dt, nits, q_exact)
    cs, coords, topos, geoms = sw_sphere(ne)
    dm = DeviceMesh(topos, geoms, nk=1, numbering="global")
    assert np.array_equal(dm.gid1, np.arange(cs.nDofs1G)) and np.array_equal(dm.gid0, np.arange(cs.nDofs0G))
    xq = np.zeros((dm.nq, 3))
    for g in geoms:
        xq[g.loc0] = coords[g.loc0]
    eng = Engine(dm)
    S = SWEqn(eng, xq[dm.gidq])
    uq, hq = sw_initial_fields(torch.as_tensor(xq[dm.gidq], device=eng.device), ic)
    u0, h0 = S.init1(uq), S.init2(hq)
    start = {"fg": S.fg[0].cpu().numpy(), "u0": u0[0].cpu().numpy(), "h0": h0[0].cpu().numpy()}
    u1, h1 = S.solve(u0, h0, dt, nits=nits, q_exact=q_exact)
    step = {"u1": u1[0].cpu().numpy(), "h1": h1[0].cpu().numpy()}
    counters = (S.fixed_iterations, S.adaptive_iterations, S.recalibrations)
    return {"sw2": "config2", "sw3": "config3"}[request.param], d, dm, start, step, np.array(S.history), counters


def _check_sw(label, d, start, step, hist):
    f = dict(start, **step)
    f["du"], f["dh"] = f["u1"] - f["u0"], f["h1"] - f["h0"]
    errs = {k: sketch_rel_err(f[k], d["S_" + k], float(d["norm_" + k])) for k in ("fg", "u0", "h0", "u1", "h1", "du", "dh")}
    ehist = float(np.abs(hist / d["history"] - 1.0).max()) if hist.size == d["history"].size else float("inf")
    print("%s vs sparse oracle (sketched relative L2): %s  history %.2e (device %s, oracle %s)" % (
        label, "  ".join("%s %.2e" % kv for kv in errs.items()), ehist, np.array2string(hist, precision=6),
        np.array2string(d["history"], precision=6)))
    for k in ("fg", "u0", "h0", "u1", "h1"):
        assert errs[k] < SW_TOL, (k, errs[k])
    for k in ("du", "dh"):
        assert errs[k] < STEP_TOL, (k, errs[k])
    assert ehist < HIST_RTOL


def test_sw_step_python_host(sw_case):
    case, d, dm, start, step, hist, (fixed, adaptive, recal) = sw_case
    print("%s Python host: fixed/adaptive iterations %d/%d, recalibrations %d" % (case, fixed, adaptive, recal))
    _check_sw("%s Python host" % case, d, start, step, hist)
    assert fixed == int(d["nits"]) and adaptive == 0 and recal == 0          # the timed, graphed fixed-length path


def test_sw_step_cpp_host(tmp_path, oracle, sw_case):
    """tests/cpp/test_sw.cpp in its four modes, from the same start state and Coriolis 0-form as the Python host"""
    from mimsem_amd.workloads import write_sw_case
    from tests.test_gpu_cpp_shim import _build
    case, d, dm, start, _, _, _ = sw_case
    dt, nits, q_exact = float(d["dt"]), int(d["nits"]), bool(d["q_exact"])
    fin, fout = str(tmp_path / "sw_in.bin"), str(tmp_path / "sw_out.bin")
    write_sw_case(fin, dm, start["fg"], start["u0"], start["h0"], dt, 1, nits, q_exact)
    out = subprocess.run([_build(str(tmp_path), "test_sw"), fin, fout, "no-half-step"], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "ALL OK" in out.stdout
    res = np.fromfile(fout, dtype=np.float64).reshape(4, dm.n1 + dm.n2)
    for mode in range(4):
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("mode %d step 0:" % mode)]
        assert len(line) == 1, mode
        hist = np.array([float(v) for v in line[0].split(":")[1].split()])
        _check_sw("%s C++ host mode %d" % (case, mode), d, start, {"u1": res[mode, :dm.n1], "h1": res[mode, dm.n1:]}, hist)


@pytest.fixture(scope="module")
def horiz(golden_dir):
    """the config-4 sphere with the fixture's 10 levels, its inputs rebuilt from the hash, and the Python host's results"""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.horizsolve import HorizSolve
    from tests.golden.make_step_fixtures import MOMENTUM_CASES, horiz_inputs, horiz_sphere
    d = dict(np.load(os.path.join(golden_dir, HORIZ_FIXTURE)))
    nk = int(d["nk"])
    cs, coords, topos, geoms, levs = horiz_sphere(int(d["ne"]), nk)
    dm = DeviceMesh(topos, geoms, nk=nk, numbering="global")
    assert np.array_equal(dm.gid1, np.arange(cs.nDofs1G)) and np.array_equal(dm.gid0, np.arange(cs.nDofs0G))
    assert nk * dm.n1 > 524288                          # past both rowdot thresholds (262 144 and 64 x 8 192 entries)
    xq = np.zeros((dm.nq, 3))
    for g in geoms:
        xq[g.loc0] = coords[g.loc0]
    f = horiz_inputs(nk, dm.n1, dm.n2, float(d["area"]), float(d["dz"]))
    eng = Engine(dm)
    hs = HorizSolve(eng, quad_coords=xq[dm.gidq])
    t = eng.tensor
    got = {"fg": hs.fg.cpu().numpy()}
    got["dF"], got["dG"], got["Fk"], got["Gk"] = (a.cpu().numpy() for a in hs.advection_rhs_ec(t(f["u1"]), t(f["u2"]), t(f["h1"]), t(f["h2"]), t(f["theta"])))
    got["Phi"] = hs.diagnose_Phi(t(f["u1"]), t(f["u2"]), t(f["velz1"]), t(f["velz2"])).cpu().numpy()
    got["q"] = hs.diagnose_q(t(f["h1"]), t(f["u1"])).cpu().numpy()
    k2i = {}
    Fk = t(got["Fk"])
    for name, use_F, use_w in MOMENTUM_CASES:
        got[name] = hs.momentum_rhs_ec(t(f["theta"]), t(f["dudz1"]), t(f["dudz2"]), t(f["velz1"]), t(f["velz2"]), t(f["Pi"]), t(f["u1"]),
                                       t(f["u2"]), t(f["h1"]), t(f["h2"]), Fx=Fk if use_F else None, Fz=t(f["Fz"]) if use_F else None, Fk=Fk,
                                       dwdx1=t(f["dwdx1"]) if use_w else None, dwdx2=t(f["dwdx2"]) if use_w else None).cpu().numpy()
        k2i[name] = float(hs.k2i)
    verified = (hs.verify(), hs.m1.chebyshev, hs.m1.solves_checked, hs.m1.solves_missed)
    return d, dm, f, got, k2i, float(hs.del2), verified


OUTPUTS = ("fg", "dF", "dG", "Fk", "Gk", "Phi", "q", "fuA", "fuB", "fuC")


def _check_horiz(label, d, got, k2i, del2):
    errs = {k: sketch_rel_err(got[k], d["S_" + k], float(d["norm_" + k])) for k in OUTPUTS if k in got}
    ek2i = {k: abs(k2i[k] - float(d["k2i_" + k])) / abs(float(d["k2i_" + k])) for k in k2i}
    print("%s vs sparse oracle (sketched relative L2): %s   k2i: %s   del2 %.2e" % (
        label, "  ".join("%s %.2e" % kv for kv in errs.items()), "  ".join("%s %.2e" % kv for kv in ek2i.items()),
        abs(del2 - float(d["del2"])) / abs(float(d["del2"]))))
    assert abs(del2 - float(d["del2"])) < 1e-6 * abs(float(d["del2"]))
    for k, e in errs.items():
        assert e < RHS_TOL, (k, e)
    for k, e in ek2i.items():
        assert e < RHS_TOL, (k, e)


def test_horizsolve_python_host(horiz):
    d, dm, f, got, k2i, del2, (ok, cheb, checked, missed) = horiz
    print("Python host: fixed-length mass solves %s, %d checked, %d missed" % (cheb, checked, missed))
    _check_horiz("HorizSolve Python host nk=10", d, got, k2i, del2)
    assert ok and cheb and missed == 0 and checked >= 15


def test_horizsolve_cpp_host(tmp_path, oracle, horiz):
    """tests/cpp/test_horiz.cpp (Chebyshev mode): the C++ host's check norms reduce rows of nk * n1 = 622 080 entries"""
    from mimsem_amd.workloads import mesh_arrays, write_arrays
    from tests.test_gpu_cpp_shim import _build
    d, dm, f, pyhost, _, _, _ = horiz
    nk, N0, N1, N2 = int(d["nk"]), dm.n0, dm.n1, dm.n2
    arrays = mesh_arrays(dm)
    arrays.update(fg=pyhost["fg"], **f)                  # (the device's Coriolis 0-form: the Python host's, checked against the oracle's sketch)
    fin, fout = str(tmp_path / "horiz_in.arr"), str(tmp_path / "horiz_out.bin")
    write_arrays(fin, arrays)
    out = subprocess.run([_build(str(tmp_path), "test_horiz"), fin, fout], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "DONE" in out.stdout and "fixed-length Chebyshev" in out.stdout
    res = np.fromfile(fout, dtype=np.float64)
    got, pos = {}, 0
    for k, rows, n in (("dF", nk, N2), ("dG", nk, N2), ("Fk", nk, N1), ("Gk", nk, N1), ("Phi", nk, N2), ("q", nk, N0), ("fuA", nk, N1),
                       ("fuB", nk, N1), ("fuC", nk, N1)):
        got[k] = res[pos:pos + rows * n].reshape(rows, n); pos += rows * n
    k2iA, k2iB, del2 = res[pos:pos + 3]
    assert pos + 3 == res.size
    _check_horiz("HorizSolve C++ host nk=10", d, got, {"fuA": k2iA, "fuB": k2iB}, del2)


@pytest.mark.parametrize("n", [262144, 262145, 524288, 622080, 1000003, 9000000])
def test_rowdot_long_rows(n):
    """mimsem_krylov_rowdot on rows past 262 144 entries (a block per 8 192 entries) and past 524 288 (more than 64 partial sums per row,
    up to the cap of 1 024 blocks) -- the C++ HorizSolve's check norms reduce one row of nk * n1 entries -- against an extended-precision
    sum, in the one-launch form (up to 8 rows) and the two-launch form (more rows): the same bits from both"""
    import torch
    from mimsem_amd.device import DeviceMesh, Engine
    from tests.golden.make_step_fixtures import sw_sphere
    cs, coords, topos, geoms = sw_sphere(2)
    eng = Engine(DeviceMesh(topos, geoms, nk=1, numbering="global"))
    g = torch.Generator(device=eng.device).manual_seed(n)
    nrows = 9
    A = torch.rand((nrows, n), dtype=torch.float64, device=eng.device, generator=g) + 0.5
    B = torch.rand((nrows, n), dtype=torch.float64, device=eng.device, generator=g) + 0.5
    B[1::2] -= 1.0                                                  # odd rows: signed products, a sum far below the sum of magnitudes
    many = eng.rowdot(A, B).cpu().numpy()                           # 9 rows: the two launches
    few = eng.rowdot(A[:2], B[:2]).cpu().numpy()                    # 2 rows: the one-launch form
    a, b = A.cpu().numpy().astype(np.longdouble), B.cpu().numpy().astype(np.longdouble)
    exact = (a * b).sum(axis=1)
    mag = np.abs(a * b).sum(axis=1)
    err = np.abs(many.astype(np.longdouble) - exact) / mag
    print("rowdot n=%d: worst |d - exact| / sum|a b| = %.2e (positive rows %.2e)" % (n, float(err.max()), float(err[0::2].max())))
    assert float(err.max()) < 1e-14                                 # a partial sum lost or counted twice is ~1e-3 of the row at least
    assert np.array_equal(few, many[:2])
