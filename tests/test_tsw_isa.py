"""The thermal shallow-water kernels (k_tsw_diagnose, k_tsw_update, csrc/tsw_kernels.hip) in the gfx950 code hipcc produces (device side only,
no GPU needed): no scratch memory and at most 128 VGPRs at every built order, so four waves fit per SIMD."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_tsw_kernels_fit_without_scratch(tmp_path):
    asm = tmp_path / "tsw_kernels.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Wno-unused-function",
                        "-Wno-unused-variable", os.path.join(ROOT, "mimsem_amd", "csrc", "tsw_kernels.hip"), "-o", str(asm)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    s = asm.read_text()
    md = s[s.index("amdgpu_metadata"):]
    got = {}
    for e in md.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", e).group(1)
        g = lambda k: int(re.search(k + r":\s+(\d+)", e).group(1))
        m = re.search(r"k_tsw_(diagnose|update)ILi(\d)E", name)
        if m:
            got[(m.group(1), int(m.group(2)))] = dict(vgpr=g(r"\.vgpr_count"), spill=g(r"\.vgpr_spill_count"),
                                                      scratch=g(r"\.private_segment_fixed_size"))
    assert sorted(got) == [(k, p) for k in ("diagnose", "update") for p in (2, 3, 4, 5)], sorted(got)
    for k, v in got.items():
        print(k, v)
        assert v["scratch"] == 0 and v["spill"] == 0, (k, v)
        assert v["vgpr"] <= 128, (k, v)
