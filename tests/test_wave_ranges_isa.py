"""The level-range form of the owner-computes kernel (k_apply_wave<3, UMAT, LCT, ACCUM, TILE = false, OWN = true>) in the gfx950
code hipcc produces (device side only, no GPU needed).  A wavefront ends at the first batch boundary at or beyond its item's last level;
that exit must cost the level loop nothing: no scratch, the register budget of 3 waves per SIMD, no workgroup barrier, no cache
write-back or invalidate, and no `s_waitcnt vmcnt(0)` beyond those the kernel had before the exit existed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# `s_waitcnt vmcnt(0)` in the whole kernel, recorded from the build of the parent commit (chunks of 8 levels, no early exit), by
# (LCT, ACCUM): the set-up waits for the lane tables once; the accumulate form reads y before it adds to it
PARENT_VMCNT0 = {(1, 0): 1, (1, 1): 2, (8, 0): 2, (8, 1): 10}
VGPR_BOUND = 168                          # 512 / 3 waves per SIMD, in allocation granules of 8


@pytest.fixture(scope="module")
def elem_asm(tmp_path_factory):
    asm = tmp_path_factory.mktemp("isa") / "elem_kernels.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Wno-unused-function",
                        "-Wno-unused-variable", os.path.join(ROOT, "mimsem_amd", "csrc", "elem_kernels.hip"), "-o", str(asm)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return asm.read_text()


OWN = re.compile(r"k_apply_waveILi3ELi0ELi(1|8)ELb([01])ELb0ELb1E")       # <3, UMAT, LCT, ACCUM, false, true>


def _kernels(s):
    md = s[s.index("amdgpu_metadata"):]
    out = {}
    for e in md.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", e).group(1)
        m = OWN.search(name)
        if not m:
            continue
        g = lambda k: int(re.search(k + r":\s+(\d+)", e).group(1))
        i = s.index("\n" + name + ":")
        out[(int(m.group(1)), int(m.group(2)))] = {"spill": g(r"\.vgpr_spill_count"), "scratch": g(r"\.private_segment_fixed_size"),
                                                   "vgpr": g(r"\.vgpr_count"), "body": s[i:s.index(".Lfunc_end", i)]}
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_early_exit_costs_the_level_loop_nothing(elem_asm):
    ks = _kernels(elem_asm)
    assert sorted(ks) == sorted(PARENT_VMCNT0), sorted(ks)
    for key, k in ks.items():
        body = k["body"]
        assert k["scratch"] == 0 and k["spill"] == 0 and "scratch_" not in body, (key, k["scratch"], k["spill"])
        assert k["vgpr"] <= VGPR_BOUND, (key, k["vgpr"])
        assert "s_barrier" not in body, key
        assert "buffer_wbl2" not in body and "buffer_inv" not in body, key
        n0 = len(re.findall(r"s_waitcnt vmcnt\(0\)", body))
        assert n0 <= PARENT_VMCNT0[key], (key, n0, PARENT_VMCNT0[key])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_exit_follows_the_batch_stores(elem_asm):
    """LCT = 8: one exit behind each of the ring's first three batches, each after that batch's two 16-byte stores and with no wait in
    front of it; the fourth batch leaves through the loop"""
    for key, k in _kernels(elem_asm).items():
        if key[0] != 8:
            continue
        lines = k["body"].split("\n")
        ends = [i for i, l in enumerate(lines) if "s_endpgm" in l]
        assert len(ends) == 4, (key, len(ends))                     # three exits and the kernel's end
        stores = [i for i, l in enumerate(lines) if "global_store_dwordx4" in l]
        assert len(stores) == 8, (key, len(stores))
        for b, e in enumerate(ends[:3]):
            assert stores[2*b + 1] < e < stores[2*b + 2], (key, b, e, stores)
            between = "\n".join(lines[stores[2*b + 1]:e])
            assert "s_waitcnt vmcnt" not in between, (key, b)        # nothing waits for the abandoned requests
