"""mimsem_host::Euler::log_entropy (mimsem_amd/host/mimsem_shim.hpp), the C++ face of mimsem_euler_log_entropy: what a torch-free host needs
for slot 11 of the box's energetics line (box/Euler_2.cpp:979-997).

CPU: tests/cpp/test_box_entropy.cpp compiles with plain g++ -std=c++17 -Wall -Werror, no HIP headers, and links against the C ABI.
GPU: the driver runs on the mesh of tests/box_strang_case.py (p = 3, 3 x 3 box, nk = 4; theta on the 5 interfaces, rows padded to an odd
pitch) in a process of its own; its value is Engine.log_entropy's bit for bit (one library, one grid, one order of summation) and within
PARITY = 1e-10 of S_abs of the numpy sum from the oracle's tables (the bar of tests/test_gpu_box_entropy.py)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = 1e-10


def _build(tmp):
    from mimsem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exe = os.path.join(tmp, "test_box_entropy")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "test_box_entropy.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip", "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_driver_compiles_and_links(tmp_path):
    assert os.path.exists(_build(str(tmp_path)))
    src = open(os.path.join(ROOT, "tests", "cpp", "test_box_entropy.cpp")).read() + open(os.path.join(ROOT, "mimsem_amd", "host", "mimsem_shim.hpp")).read()
    assert "hip/hip_runtime" not in src and "mimsem_euler_log_entropy" in src


@pytest.mark.gpu
def test_cpp_value_is_the_engines(tmp_path, oracle):
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.workloads import mesh_arrays, write_arrays
    from tests import box_strang_case as bc
    from tests.test_gpu_box_entropy import CP, draw_theta, numpy_sum
    c = bc.make_case(oracle)
    eng = Engine(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering="global"))
    nrows, n2 = c["nk"] + 1, eng.sizes[2]
    theta = draw_theta(3, nrows, eng.nEl, 111)
    lz = np.full(nrows, bc.DZ); lz[0] *= 0.5; lz[-1] *= 0.5
    pitch = n2 + 3
    wide = np.full((nrows, pitch), np.nan)                                            # (a word read from the padding poisons the sum)
    wide[:, :n2] = theta
    arrays = mesh_arrays(eng.mesh)
    arrays.update(theta=wide.ravel(), lz=lz, dims=np.array([float(nrows), float(pitch), CP]))
    fin, fout = str(tmp_path / "ent_in.arr"), str(tmp_path / "ent_out.bin")
    write_arrays(fin, arrays)
    out = subprocess.run([_build(str(tmp_path)), fin, fout], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "DONE" in out.stdout
    got = np.fromfile(fout, dtype=np.float64)
    assert got.shape == (2,) and got[0] == got[1]                                      # two calls, the same bits
    want = float(eng.log_entropy(eng.tensor(theta), eng.tensor(lz), CP)[0])
    val, s_abs = numpy_sum(oracle, 3, theta, lz, CP)
    print("C++ % .16e  Engine % .16e  numpy % .16e  |C++ - numpy| / S_abs = %.2e" % (got[0], want, val, abs(got[0] - val) / s_abs))
    assert got[0] == want
    assert abs(got[0] - val) / s_abs <= PARITY
