"""CPU checks of the thermal shallow-water C++ host and its preconditioner builder (no GPU needed): mimsem_amd/host/mimsem_thermalsw.hpp with
tests/cpp/test_tsw.cpp and mimsem_amd/host/tsw_call.cpp -- and every other C++ host on the shared pieces of mimsem_mass.hpp -- compile and link
with plain g++ against the built library, the library exports
mimsem_elem_block_pc_build, and the builder's kernel (k_elem_block_pc, csrc/elem_block_pc.inc) uses no scratch at any built order."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


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
    assert os.path.exists(_build(str(tmp_path), os.path.join(ROOT, "tests", "cpp", "test_tsw.cpp"), "test_tsw"))
    assert os.path.exists(_build(str(tmp_path), os.path.join(ROOT, "mimsem_amd", "host", "tsw_call.cpp"), "tsw_call"))


def test_every_host_compiles_on_the_shared_mass_pieces(tmp_path, lib_path):
    """mimsem_mass.hpp through all four host headers (-Wall -Werror): the call programs of SWEqn, HorizSolve, VertSolveEta and ThermalSW_EEC_2
    (above) and the driver of the shared pieces on their own; no host keeps a release() list or a constructor try / catch"""
    host = os.path.join(ROOT, "mimsem_amd", "host")
    for name in ("mimsem_sweqn.hpp", "mimsem_horizsolve.hpp", "mimsem_thermalsw.hpp", "mimsem_vertsolve.hpp"):
        text = open(os.path.join(host, name)).read()
        assert '#include "mimsem_mass.hpp"' in text, name
        assert "release()" not in text and "catch (...) { release" not in text, name
    for name in ("sw_call", "horiz_call", "vert_call"):
        assert os.path.exists(_build(str(tmp_path), os.path.join(host, name + ".cpp"), name))
    assert os.path.exists(_build(str(tmp_path), os.path.join(ROOT, "tests", "cpp", "test_mass.cpp"), "test_mass"))


def test_builder_symbol_exported(lib_path):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT mimsem_elem_block_pc_build$", out, re.M)
    from mimsem_amd import _lib
    assert "mimsem_elem_block_pc_build" in _lib.exported_symbols()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_builder_kernel_fits_without_scratch(tmp_path):
    asm = tmp_path / "elem_kernels.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Wno-unused-function",
                        "-Wno-unused-variable", os.path.join(ROOT, "mimsem_amd", "csrc", "elem_kernels.hip"), "-o", str(asm)],
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    s = asm.read_text()
    md = s[s.index("amdgpu_metadata"):]
    got = {}
    for e in md.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", e).group(1)
        g = lambda k: int(re.search(k + r":\s+(\d+)", e).group(1))
        m = re.search(r"k_elem_block_pcILi(\d)ELi(\d+)E", name)
        if m:
            got[(int(m.group(1)), int(m.group(2)))] = dict(vgpr=g(r"\.vgpr_count"), spill=g(r"\.vgpr_spill_count"),
                                                           scratch=g(r"\.private_segment_fixed_size"), lds=g(r"\.group_segment_fixed_size"))
    assert sorted(got) == [(p, op) for p in (2, 3, 4, 5) for op in (0, 2)], sorted(got)      # UMAT (0) and UHMAT (2) at orders 2..5
    for k, v in sorted(got.items()):
        print(k, v)
        assert v["scratch"] == 0 and v["spill"] == 0, (k, v)
        assert v["vgpr"] <= 256 and v["lds"] <= 64 * 1024, (k, v)
