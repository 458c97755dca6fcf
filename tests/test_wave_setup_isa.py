"""The set-up of the owner-computes Umat kernel (own4::k_apply_wave / k_apply_wave_list <3, UMAT, 8, ACCUM>) in the gfx950
code hipcc produces (device side only, no GPU needed): what a wavefront executes once per work item, before its first DPP move.

Before the change, as compiled from the default rule's kernel with ACCUM = false (the counts stand below as constants): 651
instructions in front of the first v_mov_b32_dpp, 12 exec-mask branches around conditional LDS reads of the coefficient registers and
around the two candidates of the write pointer, 9 single ds_read_b64 each behind its own s_waitcnt lgkmcnt(0), 62 scalar
multiplications (row addresses formed from the level, a runtime unsigned division), and the same row arithmetic again in every batch of
the ring.  Now the rows are stepped, the coefficients are read unconditionally and zeroed by selects, group and part of an item come
from a multiplication by a reciprocal the host passes, and the write pointer is a select of two scalar rows."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# the parent's set-up (own4::k_apply_wave<3, UMAT, 8, false>)
PARENT_SETUP_INSTRUCTIONS = 651
PARENT_EXEC_BRANCHES = 12
PARENT_SINGLE_READ_WAITS = 9
PARENT_SETUP_SCALAR_MULS = 62

KERNELS = ["own412k_apply_waveILi3ELi0ELi8ELb%dEEEv", "own417k_apply_wave_listILi3ELi0ELi8ELb%dEEEv"]


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
    body = s[m.start():s.index(".Lfunc_end", m.start())]
    full = [l.strip() for l in body.splitlines() if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]
    return [l.split()[0] for l in full], full


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("kernel", KERNELS, ids=["default_rule", "planned_list"])
def test_set_up_of_the_owner_body(elem_asm, kernel, accum):
    ops, full = _kernel(elem_asm, kernel % accum)
    dpp = ops.index("v_mov_b32_dpp")                     # the first batch's algebra begins
    load = next(i for i, o in enumerate(ops) if o.startswith("global_load"))
    store = next(i for i, o in enumerate(ops) if o.startswith("global_store"))
    assert load < dpp < store
    setup = ops[:dpp]
    branches = [l for l in full[:dpp] if l.startswith(("s_cbranch_execz", "s_cbranch_execnz"))]
    waits = [i for i in range(load, dpp) if "lgkmcnt(0)" in full[i]]
    muls = sum(o in ("s_mul_i32", "s_mul_hi_u32") for o in setup)
    print("%s: %d instructions before the first DPP move (parent %d), %d exec-mask branches (%d), %d lgkmcnt(0) waits behind the first "
          "load (%d single-read ones), %d scalar multiplications (%d)" % (kernel % accum, dpp, PARENT_SETUP_INSTRUCTIONS, len(branches),
          PARENT_EXEC_BRANCHES, len(waits), PARENT_SINGLE_READ_WAITS, muls, PARENT_SETUP_SCALAR_MULS))
    # the coefficient registers and the write pointer: selects, not exec-mask regions
    assert not branches, branches
    # the LDS reads of the set-up go out together: at most two full waits between the first load and the first batch
    assert len(waits) <= 2, [full[i - 1:i + 1] for i in waits]
    # stepped rows: no address multiplication in the ring (only the start pointers, in the set-up, are products)
    late = [l for l in full[store:] if l.split()[0] in ("s_mul_i32", "s_mul_hi_u32")]
    assert not late, late[:8]
    assert muls < PARENT_SETUP_SCALAR_MULS
    # no runtime division
    assert not any(o.startswith("v_rcp_iflag_f32") for o in ops)
    # ... and the set-up is shorter by what those four cost, less the selects that replace the branches
    assert dpp <= PARENT_SETUP_INSTRUCTIONS - 100, dpp
    # the default rule's kernel still waits ONCE for its first kernel arguments before the exit test (the note at ElemArgs, ctx.hpp)
    first_branch = next(i for i, o in enumerate(ops) if o.startswith("s_cbranch"))
    assert sum(o == "s_waitcnt" for o in ops[:first_branch]) == 1, full[:first_branch + 1]
