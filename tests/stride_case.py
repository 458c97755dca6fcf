"""One C-ABI call under three memory layouts (tests/test_gpu_abi_strides.py).

include/mimsem_hip.h addresses a multi-row operand as base + k*stride with a stride of its own per operand.  A Case names the operands
of one call and a function that issues it through eng.L from {name: (address, stride)}; run_case() places the operands

  "contiguous"  every operand [rows, n] at the start of a buffer of its own (what the rest of the suite does),
  "even"        operand i in a buffer of its own at row stride n_i + 2 (i + 1), 2 doubles into the allocation: all strides of the call
                differ, every 16-byte alignment of the contiguous call is kept,
  "odd"         operand i at row stride n_i + 2 i + 1, 1 double in: every 16-byte alignment is broken,

and check_strided() compares a strided run with the contiguous one: return code 0, every result row the same BITS, every word around
the rows untouched, every input unchanged.

The buffers make the test safe against the bug it hunts.  Every buffer of a case has lead + rows_max * S + n_max + 64 doubles, S the
LARGEST stride of the call and rows_max / n_max the most rows / the longest row of any operand: a kernel that walks operand a with
operand b's stride stays inside a's own allocation and shows up as a mismatch, not as a stray access.  The words of an input buffer
outside its rows are NaN (a read of them poisons the result), those of a result buffer hold SENTINEL."""
import numpy as np
import torch

SENTINEL = -7.25e300                      # the guard value of tests/test_gpu_wave_own4.py
TAIL = 64


class Operand:
    """rows x n doubles of one argument.  role "in" | "out" | "inout"; data: the initial [rows, n] array (results too: a kernel that leaves
    part of its result alone must leave the same values in every layout).  broadcast: one row at stride 0.  flat: an argument without a
    stride of its own (a vector, a block array): one row, placed like the others.  share: operands that the ABI gives ONE stride
    argument name the same group and get the same stride (each still in a buffer of its own)."""

    def __init__(self, name, data, role="in", broadcast=False, flat=False, share=None):
        data = np.ascontiguousarray(np.atleast_2d(np.asarray(data, dtype=np.float64)))
        assert data.ndim == 2 and role in ("in", "out", "inout")
        assert not (broadcast or flat) or data.shape[0] == 1
        self.name, self.data, self.role, self.broadcast, self.flat, self.share = name, data, role, broadcast, flat, share
        self.rows, self.n = data.shape


class Case:
    """entry: the ABI function under test; operands: [Operand]; call(eng, a) -> return code, a[name] = (address, stride), a(name) =
    the address alone, (None, 0) for an operand the case left out; ref(ins, outs): the comparison with the entry's reference on host
    arrays {name: [rows, n]} (raises AssertionError); bitwise=False: an entry that may legitimately differ between layouts -- then
    ref() is applied to every strided run instead (the reason belongs in the case's comment)."""

    def __init__(self, entry, operands, call, ref=None, bitwise=True):
        self.entry, self.operands, self.call, self.ref, self.bitwise = entry, operands, call, ref, bitwise
        names = [o.name for o in operands]
        assert len(set(names)) == len(names)
        strided = [o for o in operands if not (o.broadcast or o.flat)]
        assert all(o.rows >= 2 for o in strided), "row 0 lies at offset 0 for any stride: a one-row operand cannot see a crossed stride"


class Args(dict):
    def __call__(self, name):
        return self[name][0]

    def __missing__(self, name):
        return (None, 0)


def layout(case, mode):
    """{name: (lead, stride)} and the size of every buffer of the case.  The contiguous layout puts every operand at the start of its buffer
    with stride n, as a fresh [rows, n] tensor lies; its buffer is sized by the same rule"""
    rows_max, n_max = max(o.rows for o in case.operands), max(o.n for o in case.operands)
    if mode == "contiguous":
        return {o.name: (0, 0 if o.broadcast else o.n) for o in case.operands}, rows_max * n_max + n_max + TAIL
    odd = mode == "odd"
    lead = 1 if odd else 2
    place, used, groups, i = {}, set(), {}, 0
    for o in case.operands:
        if o.broadcast or o.flat:
            place[o.name] = (lead, 0 if o.broadcast else o.n)
            continue
        if o.share is not None and o.share in groups:
            place[o.name] = (lead, groups[o.share])
            continue
        s = o.n + (2 * i + 1 if odd else 2 * (i + 1))
        while s in used:                                   # rows of different lengths: keep every stride of the call distinct (same parity)
            s += 2
        used.add(s); i += 1
        place[o.name] = (lead, s)
        if o.share is not None:
            groups[o.share] = s
    S = max([s for _, s in place.values()] + [1])
    size = lead + rows_max * S + n_max + TAIL
    return place, size


class Run:
    """one execution: rc, the buffers, {name: 2-D view of the operand's rows}"""


def run_case(eng, case, mode):
    place, size = layout(case, mode)
    run = Run()
    run.mode, run.buf, run.view, run.init, run.place = mode, {}, {}, {}, place
    args = Args()
    for o in case.operands:
        lead, s = place[o.name]
        buf = torch.full((size,), float("nan") if o.role == "in" else SENTINEL, dtype=torch.float64, device=eng.device)
        view = torch.as_strided(buf, (o.rows, o.n), (s if o.rows > 1 else o.n, 1), lead)
        view.copy_(torch.from_numpy(o.data).to(eng.device))
        run.buf[o.name], run.view[o.name], run.init[o.name] = buf, view, buf.clone()
        args[o.name] = (view.data_ptr(), s)
    torch.cuda.synchronize(eng.device)
    run.rc = case.call(eng, args)
    eng.sync()
    torch.cuda.synchronize(eng.device)
    return run


def host(run, case, roles):
    return {o.name: run.view[o.name].cpu().numpy().copy() for o in case.operands if o.role in roles}


def check_reference(case, run):
    if case.ref is not None:
        case.ref({o.name: o.data for o in case.operands}, host(run, case, ("out", "inout")))


def check_strided(case, base, run):
    """(a) .. (d) of a strided run against the contiguous one"""
    assert base.rc == 0 and run.rc == 0, (case.entry, base.rc, run.rc)                                        # (a)
    for o in case.operands:
        buf, view = run.buf[o.name], run.view[o.name]
        if o.role == "in":                                                                                     # (d) NaN != NaN: compare the bits
            assert torch.equal(buf.view(torch.int64), run.init[o.name].view(torch.int64)), (case.entry, run.mode, o.name, "an input was written")
            continue
        if case.bitwise:                                                                                       # (b)
            same = view == base.view[o.name]
            assert torch.equal(view, base.view[o.name]), (case.entry, run.mode, o.name, "rows differ from the contiguous call",
                                                           int((~same).sum()), [int((~same[r]).sum()) for r in range(o.rows)])
        rest = buf.clone()                                                                                     # (c)
        torch.as_strided(rest, view.shape, view.stride(), view.storage_offset()).fill_(SENTINEL)
        bad = rest != SENTINEL
        assert not bool(bad.any()), (case.entry, run.mode, o.name, "words outside the rows were written", bad.nonzero().flatten()[:8].tolist(),
                                     run.place[o.name])
    if not case.bitwise:
        check_reference(case, run)
