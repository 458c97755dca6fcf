"""The box twin's Euler::Strang with its host in C++ (mimsem_amd/host/mimsem_euler.hpp: mimsem_host::box::Euler over the box-mode HorizSolve,
VortDiag with vert_mom_vort, VertSolve2's box loop and mimsem_euler_log_entropy, driven by tests/cpp/test_box_euler.cpp) on the case of
tests/box_strang_case.py (p = 3, 3 x 3 box, nk = 4, do_visc off, a fixed count of NITS Newton iterations): two steps against BoxRestatement
and against the Python host (BoxEuler.strang), the twelve diagnostics of each step, the first-step uuz = 0 and the carried state, fused
against composed forcing, a forced missed check, and the two meshes the host refuses (order 5, layers that differ).

Bars: relative L2 against the restatement per field and per step, 10 x the error observed on the MI355X rounded up to a power of ten (the
rule of tests/test_gpu_cpp_euler.py), none above CAP.  Between the two hosts: the sum of their bars.  Sums of the diagnostics: the step's
largest field bar over S_abs; k2i and k2i_z: PARITY = 1e-10 over the sum of the magnitudes of their terms (tests/test_gpu_box_strang.py).

CPU (not marked gpu): the driver compiles with plain g++ -std=c++17 -Wall -Werror, no HIP headers, and links against the C ABI."""
import os
import subprocess

import numpy as np
import pytest

from tests import box_strang_case as bc
from tests.helpers import rel_l2

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = bc.FIELDS
CAP = 1e-8
PARITY = 1e-10
SUMS = ("keh", "kev", "pe", "ie", "k2p", "p2k", "mass", "entr")
# observed on the MI355X (|C++ host - restatement| / |restatement|):
#                         velx      velz      rho       rt        exner
#   step 1                1.10e-12  1.67e-13  1.41e-16  1.50e-16  4.01e-16
#   step 2                2.06e-12  2.52e-13  5.29e-16  5.42e-16  4.86e-16
#   composed forcing and the steps after a forced miss: the same to the digits shown; the two hosts differ by at most 1.3e-12 (velx)
#   (velx: the horizontal pressure gradient of an exner field that is uniform to PERT is a difference of nearly equal numbers on both sides)
#   diagnostics / S_abs   at most 3.9e-14 (keh, step 1); k2i 5.8e-14 / 6.4e-14, k2i_z 4.8e-15 / 1.2e-15; slot 11: the kernel's bits on both steps
BARS = {1: dict(velx=1e-10, velz=1e-11, rho=1e-14, rt=1e-14, exner=1e-14),
        2: dict(velx=1e-10, velz=1e-11, rho=1e-14, rt=1e-14, exner=1e-14)}


def _build(out):
    from mimsem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "test_box_euler.cpp"), "-o", out,
                           "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip", "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_driver_compiles_and_links(tmp_path):
    assert os.path.exists(_build(str(tmp_path / "test_box_euler")))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("box_euler") / "test_box_euler"))


def _levs(c, dm):
    g, = c["geoms"]
    levs = np.zeros((c["nk"] + 1, dm.nq))
    levs[:, np.searchsorted(dm.gidq, g.loc0[np.arange(g.n0)])] = g.levs
    return levs


def run_cpp(exe, tmp, c, nsteps, tag, vort_its=0, switches="", eng=None, state=None, expect_ok=True):
    from mimsem_amd.workloads import read_arrays, write_euler_case
    eng = c["eng"] if eng is None else eng
    dm = eng.mesh
    case, res = str(tmp / (tag + ".case")), str(tmp / (tag + ".out"))
    write_euler_case(case, dm, _levs(c, dm), None, c["state"] if state is None else state, bc.DT, nsteps, newton_maxit=bc.NITS, newton_tol=0.0,
                     vort_its=vort_its, do_visc=False, eng=eng, box_lx=c["lx"])
    p = subprocess.run([exe, case, res, switches], capture_output=True, text=True, timeout=300)
    print(p.stdout.strip(), p.stderr.strip())
    if not expect_ok:
        return p
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
    """the case, its engine, two restated steps (with the twelve numbers of each), two steps of the Python host and two of the C++ host"""
    from mimsem_amd.device import DeviceMesh, Engine
    from tests.test_gpu_box_strang import make_euler
    c = bc.make_case(oracle)
    c["eng"] = Engine(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering="global"))
    R, st = bc.BoxRestatement(c), c["state"]
    c["ref"], c["ref_diag"] = [], []
    for _ in range(2):
        st = R.step(*st)
        c["ref"].append(st)
        c["ref_diag"].append(R.diagnostics(st))
    eu, st, c["py"], c["py_entropy"] = make_euler(c), tuple(c["eng"].tensor(np.array(a)) for a in c["state"]), [], []
    for _ in range(2):
        out = eu.strang(*st)
        st = out[:5]
        c["py"].append(tuple(t.cpu().numpy() for t in st))
        c["py_entropy"].append(float(c["eng"].log_entropy(eu._theta_0, eu._lz, bc.ec.CP)[0]))      # the kernel on the Python host's theta_0
    c["tmp"] = tmp_path_factory.mktemp("box_euler_runs")
    c["cpp"] = run_cpp(exe, c["tmp"], c, 2, "two")
    return c


@gpu
def test_two_steps_match_the_restatement(case):
    r = case["cpp"]
    for s in (1, 2):
        compare("box step %d" % s, state_of(r, s), case["ref"][s - 1], BARS[s])
    assert list(r["counters"][:2]) == [2, 0] and r["counters"][4] == 0 and r["counters"][6] == 0
    for s in (1, 2):
        assert r["newton" + str(s)].size == 4 * bc.NITS and np.isfinite(r["newton" + str(s)]).all()
        assert list(r["fused_forcing" + str(s)]) == [0.0, 1.0]            # fused during the step (the default), the host's switch restored


@gpu
def test_same_fields_as_the_python_host(case):
    """two hosts, the same launches: each within its own bars of the restatement, so within their sum of each other"""
    for s in (1, 2):
        for n, a, b in zip(FIELDS, state_of(case["cpp"], s), case["py"][s - 1]):
            e = rel_l2(a, b)
            print("box step %d  C++ host vs Python host  %s %.2e" % (s, n, e))
            assert e < BARS[s][n] + bc.BARS[s][n], (s, n, e)


@gpu
def test_first_step_uuz_is_zero_then_carried(case, exe):
    """the carried state: the leapfrog's u_prev and uz_prev as on the sphere.  uuz: the restatement WITHOUT the first-step zero (lose =
    "uuz_first") moves velz by 1.3e-4 on step 1, far above the bar the C++ step meets against the restatement that has it; and step 2 of the
    C++ host meets its bar only with the carried vert_mom_vort(velx, velz_0), which the restatement without it ("dwdx" apart) does not share"""
    r = case["cpp"]
    assert "u_prev1" not in r and np.array_equal(r["u_curr1"], case["state"][0].ravel())
    assert np.array_equal(r["u_prev2"], case["state"][0].ravel()) and np.array_equal(r["u_curr2"], r["velx1"].ravel())
    assert np.array_equal(r["uz_prev2"], r["uz1"]) and not np.array_equal(r["uz_prev2"], r["uz2"])            # :1347-1349
    lost = bc.BoxRestatement(case, lose="uuz_first").step(*case["state"])
    e = rel_l2(r["velz1"], lost[1])
    print("velz of step 1 against the restatement with uuz != 0 on the first step: %.2e" % e)
    assert e > 100 * BARS[1]["velz"]


@gpu
def test_the_twelve_diagnostics_of_each_step(case):
    from mimsem_amd.energetics import FIELDS as LINE
    for s in (1, 2):
        vals = case["cpp"]["values" + str(s)]
        assert vals.size == 12 and np.isfinite(vals).all()
        d, ref = dict(zip(LINE, vals)), case["ref_diag"][s - 1]
        bar = max(BARS[s].values())
        errs = {n: abs(d[n] - ref[n][0]) / ref[n][1] for n in SUMS}
        print("box step %d diagnostics: |C++ host - restatement| / S_abs  %s" % (s, "  ".join("%s %.2e" % (n, errs[n]) for n in SUMS)))
        for n in SUMS:
            assert ref[n][1] > 0 and errs[n] < bar, (s, n, d[n], ref[n])
        for n in ("k2i", "k2i_z"):                                               # signed sums: relative to the sum of the magnitudes
            e = abs(d[n] - ref[n][0]) / ref[n][1]
            print("box step %d %s %.6e, restated %.6e, |difference| / S_abs %.2e" % (s, n, d[n], ref[n][0], e))
            assert ref[n][0] != 0.0 and e < PARITY, (s, n)
        assert d["i2k"] == 0.0 and d["i2k_z"] == 0.0
    # slot 11 is the kernel's value: on step 1 both hosts diagnose theta_0 from the same input with the same kernel, so the same bits
    assert case["cpp"]["values1"][11] == case["py_entropy"][0]
    e = abs(case["cpp"]["values2"][11] - case["py_entropy"][1]) / abs(case["py_entropy"][1])
    print("slot 11 of step 2 against the kernel on the Python host's theta_0: %.2e" % e)
    assert e < max(BARS[2].values())
    # ... and not the sphere's 1/2 theta . M2 rt that Energetics puts in that slot
    from tests.test_gpu_box_strang import make_euler
    st = tuple(case["eng"].tensor(a) for a in state_of(case["cpp"], 2))
    sphere = make_euler(case).energetics.diagnostics(*st)[11]
    assert abs(sphere - case["cpp"]["values2"][11]) > 1e-6 * abs(case["cpp"]["values2"][11])


@gpu
def test_fused_and_composed_forcing_within_the_same_bars(case, exe):
    r = run_cpp(exe, case["tmp"], case, 2, "composed", switches="composed")
    for s in (1, 2):
        compare("box step %d, composed forcing" % s, state_of(r, s), case["ref"][s - 1], BARS[s])
        assert list(r["fused_forcing" + str(s)]) == [0.0, 0.0]
    e = rel_l2(r["velx2"], case["cpp"]["velx2"])
    print("fused vs composed velx after two steps %.2e" % e)
    assert not np.array_equal(r["velx2"], case["cpp"]["velx2"])          # two routes, not one


@gpu
def test_a_forced_miss_redoes_the_step(case, exe):
    r = run_cpp(exe, case["tmp"], case, 2, "miss", vort_its=1)           # one PCG iteration: the check of step 1 must fail
    assert list(r["counters"][:2]) == [2, 1] and r["counters"][4] == 1
    assert r["counters"][2] == 0 and r["counters"][3] == 0               # adaptive afterwards
    for s in (1, 2):
        compare("box step %d after a forced miss" % s, state_of(r, s), case["ref"][s - 1], BARS[s])


@gpu
def test_refused_meshes_end_in_an_exception_and_a_nonzero_exit(case, exe, oracle):
    """an order-5 box and the box of box_schur2_case with its perturbed levels: the constructor's message on stderr, exit status 1, no crash"""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import BoxGeom
    from mimsem_amd.mesh import PeriodicBox, box_coords
    from mimsem_amd.topo import Topo
    nk = case["nk"]
    bx = PeriodicBox(5, 2, 1)
    t = Topo(bx, 0, nk)
    g = BoxGeom(t, bx, box_coords(5, 2, case["lx"]), nk, case["lx"])
    g.set_levels(np.outer(bc.DZ * np.arange(nk + 1), np.ones(g.n0)))
    eng5 = Engine(DeviceMesh([t], [g], nk=nk, numbering="global"))
    c5 = dict(case, geoms=[g])
    z = lambda *shape: np.ones(shape)
    st5 = (z(nk, eng5.sizes[1]), z(eng5.nEl, (nk - 1) * 25), z(nk, eng5.sizes[2]), z(nk, eng5.sizes[2]), z(nk, eng5.sizes[2]))
    p = run_cpp(exe, case["tmp"], c5, 1, "order5", eng=eng5, state=st5, expect_ok=False)
    assert p.returncode == 1 and "orders 1..4" in p.stderr and "OK" not in p.stdout
    cn = bc.make_case(oracle, uniform=False)
    engn = Engine(DeviceMesh([cn["topo"]], [cn["geom"]], nk=nk, numbering="global"))
    cnn = dict(case, geoms=[cn["geom"]])
    p = run_cpp(exe, case["tmp"], cnn, 1, "nonuniform", eng=engn, expect_ok=False)
    assert p.returncode == 1 and "uniform layers only" in p.stderr and "OK" not in p.stdout
