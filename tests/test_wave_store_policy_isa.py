"""The cache policy of each stream of the owner-computes Umat kernel (own4::k_apply_wave and own4::k_apply_wave_list <3, UMAT, 8, ACCUM>,
DESIGN 4.8) in the gfx950 code hipcc produces (device side only, no GPU needed).  A ring of LCT = 8 levels is four lock-step batches:

    stream                               instructions per kernel                          policy
    y                                    8 global_store_dwordx4 (one per level)           STORE_MOD
    thickInv pairs of the element        6 global_load_dwordx4 (2 prologue + 4 ring)      THICK_MOD
    thickInv of the ghost lanes          3 global_load_dwordx2 (1 prologue + 2 ring)      THICK_MOD
    x pairs, gathered ghost DoFs         12 global_load_dwordx4, 12 global_load_dwordx2   default
    tables, metric, y read by ACCUM      the rest                                         default

x is re-read by the neighbouring groups, by the ghost gathers and by the sibling item of the group, so it must keep the default
policy whatever the other streams carry; thickInv is read once per launch and by nobody else.  Changing a policy may not cost the
kernel its registers, its straight-line ring or the exits that leave without waiting for the loads in flight."""
import os
import re
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
MODS = ("nt", "sc0", "sc1")
STORE_MOD = ("nt",)            # the policy the y stores ship with (a tuple of modifiers; () = the default policy)
THICK_MOD = ()                 # ... and the thickInv loads: `nt` there was measured 3 us per launch slower (profiles/umat_store_policy_ab.txt)


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
    full = [l.strip() for l in body.splitlines() if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]
    return sym, [l.split()[0] for l in full], full


def _meta(s, sym, key):
    m = re.search(r"\.set " + re.escape(sym) + r"\." + key + r", (\d+)", s)
    assert m, (sym, key)
    return int(m.group(1))


def _mods(line):
    return tuple(w for w in line.split() if w in MODS)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("entry", ["own412k_apply_waveILi3ELi0ELi8ELb%dEEEv", "own417k_apply_wave_listILi3ELi0ELi8ELb%dEEEv"], ids=["default_rule", "item_list"])
@pytest.mark.parametrize("accum", [0, 1])
def test_policy_per_stream(elem_asm, entry, accum):
    sym, ops, full = _kernel(elem_asm, entry % accum)
    new = Counter(ops)
    # registers, scratch, barrier, atomic
    assert _meta(elem_asm, sym, "private_seg_size") == 0 and not any(o.startswith("scratch_") for o in new), "scratch"
    assert _meta(elem_asm, sym, "num_vgpr") <= 168 and _meta(elem_asm, sym, "num_agpr") == 0
    assert new["s_barrier"] == 0 and not any(o.startswith(("global_atomic", "flat_atomic", "buffer_atomic", "ds_add", "ds_cmpst")) for o in new)
    assert not any(o.startswith(("flat_", "buffer_")) for o in new), "every access of the kernel is a global_ one"
    # y: one 16-byte store per level of the ring, nothing else is stored, all with the shipped policy
    stores = [l for l in full if l.startswith("global_store")]
    assert len(stores) == 8 and all(l.startswith("global_store_dwordx4") for l in stores), stores
    assert all(_mods(l) == STORE_MOD for l in stores), stores
    # loads: the thickInv pairs (16 bytes) and the ghost lanes' thickInv (8 bytes) carry theirs; every other load carries none
    loads = [l for l in full if l.startswith("global_load")]
    marked = Counter(l.split()[0] for l in loads if _mods(l))
    if THICK_MOD:
        assert marked == {"global_load_dwordx4": 6, "global_load_dwordx2": 3}, marked
        assert all(_mods(l) == THICK_MOD for l in loads if _mods(l)), [l for l in loads if _mods(l)]
    else:
        assert not marked, marked
    plain = Counter(l.split()[0] for l in loads if not _mods(l))
    # x pairs: 2 batches of 2 levels ahead + 8 in the ring (ACCUM reads y with 8 more, default policy); gathers likewise, 8 bytes each
    assert plain["global_load_dwordx4"] >= 12 + (8 if accum else 0) and plain["global_load_dwordx2"] >= 12, plain
    assert len(loads) - sum(marked.values()) == sum(plain.values())
    first = full.index(stores[0])                        # (the ring's loads of its last three batches stand behind its first store)
    assert sum(1 for l in full[first:] if l.startswith("global_load_dwordx4") and not _mods(l)) >= 6 + (6 if accum else 0), "the ring's x pairs"
    # the exits: three inside the ring and the kernel's end; no wait for loads between a batch's stores and its exit
    assert new["s_endpgm"] == 4, new
    ends = [i for i, o in enumerate(ops) if o == "s_endpgm"]
    for e in ends[:3]:
        st = max(i for i in range(e) if ops[i].startswith("global_store"))
        assert not any("vmcnt" in l for l in full[st + 1:e]), full[st:e + 1]
