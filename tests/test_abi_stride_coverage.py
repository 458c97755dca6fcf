"""Every entry point of include/mimsem_hip.h that takes a row stride has a case in tests/test_gpu_abi_strides.py or a stated reason not to.
A function counts when one of its parameters is a `long long` whose name ends in `stride` or starts with `ld`.  A new strided entry point
fails here until someone gives it a case."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAY_BE_EXCLUDED = {"mimsem_ksp_set_operator", "mimsem_ksp_set_operator_sw", "mimsem_ksp_set_pc_jacobi", "mimsem_ksp_set_pc_elem_blocks", "mimsem_ksp_solve",
                   "mimsem_halo_begin", "mimsem_sw_chebyshev_step2", "mimsem_sw_chebyshev_flush"}


def strided_entries():
    with open(os.path.join(ROOT, "include", "mimsem_hip.h")) as fh:
        src = fh.read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    found = set()
    for m in re.finditer(r"\b(mimsem_\w+)\s*\(([^;{}()]*)\)\s*;", src):
        params = [" ".join(p.split()) for p in m.group(2).split(",")]
        if any(re.fullmatch(r"long long (\w*stride|ld\w*)", p) for p in params):
            found.add(m.group(1))
    return found


def test_every_strided_entry_has_a_case_or_a_reason():
    from tests.test_gpu_abi_strides import COVERED, EXCLUDED
    found = strided_entries()
    assert len(found) == 55, sorted(found)
    assert isinstance(EXCLUDED, dict) and set(EXCLUDED) <= MAY_BE_EXCLUDED and len(EXCLUDED) <= 8 and all(EXCLUDED.values())
    assert not COVERED & set(EXCLUDED), sorted(COVERED & set(EXCLUDED))
    assert COVERED | set(EXCLUDED) == found, (sorted(found - COVERED - set(EXCLUDED)), sorted((COVERED | set(EXCLUDED)) - found))


def test_layouts_give_distinct_strides_inside_their_buffers():
    """the harness itself (tests/stride_case.py), on the host: all strides of a call differ (shared groups apart), the even layout keeps
    16-byte alignment and the odd one breaks it, and a row walked with the LARGEST stride of the call still ends inside the buffer"""
    import numpy as np
    from tests import stride_case as sc
    ops = [sc.Operand("a", np.zeros((3, 10))), sc.Operand("b", np.zeros((3, 12))), sc.Operand("c", np.zeros((2, 10)), "out", share="g"),
           sc.Operand("d", np.zeros((2, 10)), "out", share="g"), sc.Operand("e", np.zeros((1, 10)), broadcast=True), sc.Operand("w", np.zeros((1, 40)), flat=True)]
    case = sc.Case("x", ops, None)
    for mode, parity in (("even", 0), ("odd", 1)):
        place, size = sc.layout(case, mode)
        strides = [place[n][1] for n in "abc"]
        assert len(set(strides)) == 3 and place["c"] == place["d"] and place["e"][1] == 0
        assert all(s % 2 == parity and s >= o.n for s, o in zip(strides, ops)) and all(lead % 2 == parity for lead, _ in place.values())
        S = max(strides)
        assert all(place[o.name][0] + (o.rows - 1) * S + max(p.n for p in ops) <= size for o in ops)
