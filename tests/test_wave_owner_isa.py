"""The owner-computes instantiations of the headline kernel (k_apply_wave<3, UMAT, LCT, ACCUM, TILE = false, OWN = true>) in
the gfx950 code hipcc produces (device side only, no GPU needed): no scratch memory, the register budget their waves-per-EU bound
promises, straight-line level batches (exact vmcnt counts keep loads in flight), no workgroup barrier, no atomics."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def elem_asm(tmp_path_factory):
    """elem_kernels.hip compiled ONCE to gfx950 ISA (device side only)"""
    asm = tmp_path_factory.mktemp("isa") / "elem_kernels.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Wno-unused-function",
                        "-Wno-unused-variable", os.path.join(ROOT, "mimsem_amd", "csrc", "elem_kernels.hip"), "-o", str(asm)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return asm.read_text()


def _metadata(s):
    md = s[s.index("amdgpu_metadata"):]
    out = {}
    for e in md.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", e).group(1)
        g = lambda k: int(re.search(k + r":\s+(\d+)", e).group(1))
        out[name] = {"spill": g(r"\.vgpr_spill_count"), "scratch": g(r"\.private_segment_fixed_size"), "vgpr": g(r"\.vgpr_count"),
                     "lds": g(r"\.group_segment_fixed_size")}
    return out


def _body(s, name):
    i = s.index("\n" + name + ":")
    return s[i:s.index(".Lfunc_end", i)]


OWN = re.compile(r"k_apply_waveILi3ELi0ELi(1|8)ELb([01])ELb0ELb1E")       # <3, UMAT, LCT, ACCUM, false, true>


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_owner_instantiations_fit_without_scratch(elem_asm):
    md = _metadata(elem_asm)
    own = {k: v for k, v in md.items() if OWN.search(k)}
    assert len(own) == 4, sorted(k for k in md if "k_apply_wave" in k)            # LCT 1 | 8, plain | accumulate
    base = [v for k, v in md.items() if re.search(r"k_apply_waveILi3ELi0ELi8ELb0ELb0ELb0E", k)]
    assert len(base) == 1
    for k, v in own.items():
        assert v["scratch"] == 0 and v["spill"] == 0, (k, v)
        assert v["vgpr"] <= 168, (k, v)                          # >= 3 waves per SIMD (the hot launch holds 1.7 per SIMD)
        assert v["lds"] <= 32768, (k, v)                         # five workgroups of four waves still fit a CU's LDS
    assert base[0]["scratch"] == 0 and base[0]["vgpr"] <= 128, base    # today's form keeps its 4 waves per SIMD


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_owner_kernel_is_straight_line(elem_asm):
    names = [n for n in _metadata(elem_asm) if OWN.search(n) and OWN.search(n).group(1) == "8"]
    assert len(names) == 2
    for n in names:
        body = _body(elem_asm, n)
        assert "s_barrier" not in body, n                         # no workgroup barrier: hand-offs stay inside the wavefront
        assert "buffer_wbl2" not in body and "global_atomic" not in body, n      # no cross-wave traffic, no atomics
        assert "v_mov_b32_dpp" in body or "row_ror" in body, n    # the ghost rows run the element's DPP algebra
        waits = re.findall(r"s_waitcnt vmcnt\((\d+)\)", body)
        assert waits and sum(1 for w in waits if int(w) > 0) >= 4, (n, waits[:40])      # exact counts: loads stay in flight
        assert re.search(r"global_load_dwordx4", body) and re.search(r"global_store_dwordx4", body), n
