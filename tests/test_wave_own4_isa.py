"""The owner-computes Umat kernel with one ghost pass per four levels (own4::k_apply_wave<3, UMAT, 8, ACCUM>) in the gfx950
code hipcc produces (device side only, no GPU needed), against the same kernel without ghost work (OWN = false, the element kernel of
the two-launch form) and against the pass per batch of two levels (k_apply_wave<3, UMAT, 8, ACCUM, false, true>).  Whole LCT = 8
bodies (4 lock-step batches of 2 levels):

                          pass per batch   pass per four levels   element kernel
    v_mov_b32_dpp              312                 260                 208
    ds_read_b128                 8                   4                   0

The ghost work runs at two of the ring's four batches, so its DPP moves and its quadruple reads halve; the kernel stays straight-line
(the ring is one block with its three wave-uniform exits), keeps its registers and its LDS budget, and has no barrier and no atomic."""
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


def _kernel(s, name):
    m = re.search(r"\n(_Z\w*" + name + r"\w*):", s)
    assert m, name
    sym = m.group(1)
    body = s[m.start():s.index(".Lfunc_end", m.start())]
    lines = [l.split()[0] for l in body.splitlines() if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]
    full = [l.strip() for l in body.splitlines() if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]
    return sym, lines, full


def _meta(s, sym, key):
    m = re.search(r"\.set " + re.escape(sym) + r"\." + key + r", (\d+)", s)
    assert m, (sym, key)
    return int(m.group(1))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("accum", [0, 1])
def test_four_level_ghost_pass_of_the_owner_body(elem_asm, accum):
    sym, ops, full = _kernel(elem_asm, "own412k_apply_waveILi3ELi0ELi8ELb%dEEEv" % accum)
    _, base_ops, _ = _kernel(elem_asm, "k_apply_waveILi3ELi0ELi8ELb%dELb0ELb0E" % accum)
    _, old_ops, _ = _kernel(elem_asm, "k_apply_waveILi3ELi0ELi8ELb%dELb0ELb1E" % accum)
    new, base, old = Counter(ops), Counter(base_ops), Counter(old_ops)
    # registers, scratch, LDS
    assert _meta(elem_asm, sym, "private_seg_size") == 0 and not any(o.startswith("scratch_") for o in new), "scratch"
    assert _meta(elem_asm, sym, "num_vgpr") <= 168 and _meta(elem_asm, sym, "num_agpr") == 0
    desc = elem_asm[elem_asm.index(".amdhsa_kernel " + sym):]
    desc = desc[:desc.index(".end_amdhsa_kernel")]
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1)) <= 32*1024
    assert "vgpr_spill_count: 0" in elem_asm[elem_asm.index(".name:           " + sym) - 1500:elem_asm.index(".name:           " + sym) + 1500] or \
        not re.search(r"; (ScratchSize|SGPRSpill|VGPRSpill)[^\n]*: [1-9]", elem_asm[elem_asm.index(sym + ":"):elem_asm.index(".amdhsa_kernel " + sym)][-3000:])
    # no barrier, no atomic
    assert new["s_barrier"] == 0 and not any(o.startswith(("global_atomic", "flat_atomic", "buffer_atomic", "ds_add", "ds_cmpst")) for o in new)
    # two 16-byte stores per batch, three exits inside the ring and the kernel's end
    assert new["global_store_dwordx4"] == 8 and sum(v for k, v in new.items() if k.startswith("global_store")) == 8, new
    assert new["s_endpgm"] == 4, new
    # no wait for loads between a batch's stores and its exit: the requests in flight are abandoned, not waited for
    ends = [i for i, o in enumerate(ops) if o == "s_endpgm"]
    for e in ends[:3]:
        st = max(i for i in range(e) if ops[i] == "global_store_dwordx4")
        assert not any("vmcnt" in l for l in full[st + 1:e]), full[st:e + 1]
    # the ghost share: 2 passes x (dpp_rows + dpp_quad<3> + dpp_rows + dpp_quad<4>) x 2 halves; two 16-byte quadruple reads per pass
    assert new["v_mov_b32_dpp"] - base["v_mov_b32_dpp"] == 52, (new["v_mov_b32_dpp"], base["v_mov_b32_dpp"])
    assert old["v_mov_b32_dpp"] - base["v_mov_b32_dpp"] == 104
    assert old["ds_read_b128"] == 8 and new["ds_read_b128"] == 4, (old["ds_read_b128"], new["ds_read_b128"])
