"""CPU checks of the C++ host of the 3-D Euler step (no GPU needed): mimsem_amd/host/mimsem_euler.hpp with tests/cpp/test_euler.cpp and
mimsem_amd/host/euler_call.cpp compile with plain g++ -std=c++17 -Wall against the header and link against the built library, and the
library's binding declares the two entries the host needs beyond those of the other hosts: the fixed-length mode of the batched PCG
(mimsem_ksp_set_fixed_iterations) and its device-side check log (mimsem_krylov_ratio_max)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mimsem_ksp_set_fixed_iterations", "mimsem_krylov_ratio_max")


@pytest.fixture(scope="module")
def lib_path():
    from mimsem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.LIB_PATH


def _build(tmp, src, name):
    exe = os.path.join(tmp, name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", src, "-o", exe, "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_host_and_call_sites_compile_and_link(tmp_path, lib_path):
    assert os.path.exists(_build(str(tmp_path), os.path.join(ROOT, "tests", "cpp", "test_euler.cpp"), "test_euler"))
    assert os.path.exists(_build(str(tmp_path), os.path.join(ROOT, "mimsem_amd", "host", "euler_call.cpp"), "euler_call"))


def test_host_sits_on_the_shared_pieces():
    text = open(os.path.join(ROOT, "mimsem_amd", "host", "mimsem_euler.hpp")).read()
    for inc in ('#include "mimsem_horizsolve.hpp"', '#include "mimsem_vertsolve.hpp"'):
        assert inc in text
    assert "hip/hip_runtime" not in text and "release()" not in text
    for name in NEW[:1] + ("mimsem_elem_block_pc_build_levels", "mimsem_op_apply_levels", "mimsem_fric_chebyshev_solve", "mimsem_ksp_ritz",
                       "mimsem_euler_energetics_horiz", "mimsem_euler_energetics_column"):
        assert name in text, name


def test_new_entries_declared_and_exported(lib_path):
    from mimsem_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "mimsem_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bT %s$" % name, out, re.M), name
        assert name in _lib.exported_symbols()
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert "MIMSEM_KSP_FIXED_ITS" in hdr


def test_case_writer_is_there():
    from mimsem_amd import workloads
    assert callable(workloads.write_euler_case) and callable(workloads.read_arrays)
