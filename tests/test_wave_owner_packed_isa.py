"""Instruction counts of the owner-computes Umat kernel with packed ghost lanes (k_apply_wave<3, UMAT, 8, ACCUM, false, true>,
DESIGN 4.8, round 9) in the gfx950 code hipcc produces (device side only, no GPU needed), against the same kernel without ghost work
(OWN = false, the element kernel of the two-launch form).  Whole LCT = 8 bodies (4 lock-step batches of 2 levels), plain form:

                          ghost rows (round 7)   packed ghost lanes   element kernel
    global_load*                  46                    46                 28
    ds_read*                      70                    73                 70
    ds_write*                     69                    64                 55
    ds_read_b128                   0                     8                  0
    v_mov_b32_dpp                416                   312                208

The ghost work's DPP moves halve (one pass of 13 dpp64 per batch of 2 levels instead of one per level), its LDS staging stores pair up,
its operand reads become two ds_read_b128 per batch, its result stores one per batch."""
import os
import re
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def elem_asm(tmp_path_factory):
    asm = tmp_path_factory.mktemp("isa") / "elem_kernels.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Wno-unused-function",
                        "-Wno-unused-variable", os.path.join(ROOT, "mimsem_amd", "csrc", "elem_kernels.hip"), "-o", str(asm)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return asm.read_text()


def _counts(s, own, accum):
    name = "k_apply_waveILi3ELi0ELi8ELb%dELb0ELb%dE" % (accum, own)
    m = re.search(r"\n(_Z\w*" + name + r"\w*):", s)
    assert m, name
    body = s[m.start():s.index(".Lfunc_end", m.start())]
    ops = Counter(l.split()[0] for l in body.splitlines() if l.startswith("\t") and not l.lstrip().startswith((".", ";")))
    pick = lambda p: sum(v for k, v in ops.items() if k.startswith(p))
    return {"gload": pick("global_load"), "dsr": pick("ds_read"), "dsw": pick("ds_write"), "b128": ops["ds_read_b128"],
            "dpp": ops["v_mov_b32_dpp"]}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("accum", [0, 1])
def test_packed_ghost_share_of_the_owner_body(elem_asm, accum):
    own, base = _counts(elem_asm, 1, accum), _counts(elem_asm, 0, accum)
    ghost = {k: own[k] - base[k] for k in own}
    assert ghost["dpp"] == 104, (own, base)                  # 4 passes x (dpp_rows + dpp_quad<3> + dpp_rows + dpp_quad<4>) x 2 halves
    assert own["b128"] == 8, own                              # the quadruples: two 16-byte reads per pass
    assert ghost["dsw"] <= 9, (own, base)                     # round 7: 14 (a staging store and a result store per level)
    assert ghost["dsr"] <= 3, (own, base)                     # round 7: 0 with 16 b64 operand reads hidden in the element's count
    assert ghost["gload"] <= 18, (own, base)                  # as round 7: a gather per level, a thickInv load per pass, the tables
