"""mimsem_host::HorizSolve::advection_rhs / momentum_rhs (mimsem_amd/host/mimsem_horizsolve.hpp; eul/HorizSolve.cpp:330-375, :496-635) and the
switches fused_hu / fused_forcing / fused_phi, driven from C++ (tests/cpp/test_horiz2.cpp), against the numpy restatements of
tests/strang2_case.py on the p = 3, ne = 2, nk = 3 sphere of tests/vort_diag_case.py: the case, the references and the bar of the Python
host's test, tests/test_gpu_horiz_rhs2.py -- relative L2 per level below MOMENTUM_TOL = 1e-10, k2i relative to the sum of the magnitudes of
its terms at the same bar; every observed value is printed.  The switches are off by default (the _ec routines keep their bits:
tests/test_gpu_cpp_shim.py and tests/test_gpu_cpp_euler.py run unchanged).

CPU: the driver compiles with plain g++ -std=c++17 -Wall -Werror, no HIP headers, and links against the C ABI."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOMENTUM_TOL = 1e-10
MODES = ("composed", "fused_hu", "fused_forcing", "fused_phi", "all three")


def _build(tmp):
    from mimsem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exe = os.path.join(tmp, "test_horiz2")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "test_horiz2.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip", "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_driver_compiles_and_links(tmp_path):
    assert os.path.exists(_build(str(tmp_path)))
    assert "hip/hip_runtime" not in open(os.path.join(ROOT, "mimsem_amd", "host", "mimsem_horizsolve.hpp")).read()


@pytest.mark.gpu
def test_right_hand_sides_driven_from_cpp(tmp_path, oracle):
    from mimsem_amd.device import DeviceMesh
    from mimsem_amd.workloads import mesh_arrays, write_arrays
    from tests import strang2_case as s2c
    from tests import vort_diag_case as vc
    c = vc.make_case()
    F, gd, nk = c["F"], c["gd"], vc.NK
    dm = DeviceMesh(c["topos"], c["geoms"], nk=nk, numbering="global")
    r = np.random.default_rng(17)
    theta_i = r.uniform(290, 310, (nk + 1, gd.N2)) * F["area"]                         # theta on the nk+1 interfaces (no thickness)
    dudz1 = r.standard_normal((nk - 1, gd.N1)) * 1e-3 * F["ln"]; dudz2 = dudz1 * 1.1
    dwdx1 = r.standard_normal((nk - 1, gd.N1)) * 1e-4 * F["ln"]; dwdx2 = dwdx1 * 0.9
    hz = c["ho"].HorizOracle(gd)
    adv = s2c.advection_rhs(hz, F["u1"], F["u2"], F["h1"], F["h2"], theta_i)
    margs = lambda k: (theta_i, dudz1, dudz2, F["velz1"], F["velz2"], F["Pi"][k], F["u1"][k], F["u2"][k], F["h1"][k], F["h2"][k])
    mom = [s2c.momentum_rhs(hz, k, *margs(k), dwdx1=dwdx1, dwdx2=dwdx2, Fk=adv[2][k]) for k in range(nk)]
    want_mom = np.stack([m[0] for m in mom])
    k2i, k2i_abs = sum(m[1] for m in mom), sum(m[2] for m in mom)
    want_plain = np.stack([s2c.momentum_rhs(hz, k, *margs(k)) for k in range(nk)])
    assert k2i != 0.0 and k2i_abs > 0 and rel_l2(want_mom, want_plain) > 1e-6          # the optional terms are felt
    fg = np.broadcast_to(hz.fg, (nk, dm.n0)) if np.ndim(hz.fg) == 1 else hz.fg
    arrays = mesh_arrays(dm)
    arrays.update(fg=fg, u1=F["u1"], u2=F["u2"], h1=F["h1"], h2=F["h2"], theta_i=theta_i, Pi=F["Pi"], velz1=F["velz1"], velz2=F["velz2"],
                  dudz1=dudz1, dudz2=dudz2, dwdx1=dwdx1, dwdx2=dwdx2)
    fin, fout = str(tmp_path / "horiz2_in.arr"), str(tmp_path / "horiz2_out.bin")
    write_arrays(fin, arrays)
    out = subprocess.run([_build(str(tmp_path)), fin, fout], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "DONE" in out.stdout
    res = np.fromfile(fout, dtype=np.float64)
    pos = [0]

    def take(rows, n):
        a = res[pos[0]:pos[0] + rows * n].reshape(rows, n); pos[0] += rows * n
        return a
    N1, N2 = gd.N1, gd.N2
    for mode in MODES:
        got = dict(dF=take(nk, N2), dG=take(nk, N2), Fk=take(nk, N1), Gk=take(nk, N1), mom=take(nk, N1), plain=take(nk, N1))
        want = dict(dF=adv[0], dG=adv[1], Fk=adv[2], Gk=adv[3], mom=want_mom, plain=want_plain)
        for name in got:
            errs = [rel_l2(got[name][k], want[name][k]) for k in range(nk)]
            print("C++ %-13s %-5s relative L2 per level  %s" % (mode, name, "  ".join("%.2e" % e for e in errs)))
            assert np.all(np.isfinite(got[name])) and max(errs) < MOMENTUM_TOL, (mode, name, errs)
        e = abs(take(1, 1)[0, 0] - k2i) / k2i_abs
        print("C++ %-13s k2i   |difference| / sum of magnitudes %.2e" % (mode, e))
        assert e < MOMENTUM_TOL, (mode, e)
    assert pos[0] == res.size
