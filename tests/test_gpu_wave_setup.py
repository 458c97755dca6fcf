"""The set-up of the owner-computes Umat kernel (own4::apply_wave_body, csrc/elem_wave.inc): the rows of x and of the
thickInv pair table are STEPPED from one batch to the next instead of computed from the level, the coefficient registers are read
at clamped indices and zeroed by selects, the default rule splits an item into group and part by a multiplication (ElemArgs::wcpp
carries the reciprocal) and the write pointer is chosen per lane between two scalar rows.  None of that may change a bit of y or touch
a word beside it: on the 4 x 4 x 6 sphere (24 wave-groups) with 17 levels of geometry the form is compared BIT FOR BIT with the
two-launch form (MIMSEM_WAVE_OWN=0) for level counts around every batch, pass, ring and item boundary, at lev0 = 0, 1 and the largest
that fits (the last pair row of the table and the clamp behind the last level are reached with both parities), with both flags,
accumulating twice in a row, alpha and scale off 1 (alpha negative: an unused coefficient stays +0.0), x and y as row slices of wider
arrays with different strides, guard rows before and behind y, requested parts of 2, 6 and 10 levels in both item orders, the planned
list under pretended chips, and one captured graph replayed three times."""
import numpy as np
import pytest

from tests.helpers import SCALE
from tests.test_gpu_wave_own4 import SENTINEL, _engine, _mesh

pytestmark = pytest.mark.gpu

NK = 17
NLEVS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17]
SC, ALPHA = 0.75*SCALE, -0.375
UMAT = 0


def _lev0s(nl):
    return sorted({0, 1, NK - nl} & set(range(NK - nl + 1)))


def _call(eng, xv, yv, lev0, fl, acc):
    """mimsem_op_apply(UMAT) on 2-D views with unit inner stride: each with its own row stride"""
    assert xv.stride(1) == 1 and yv.stride(1) == 1 and xv.shape == yv.shape
    rc = eng.L.mimsem_op_apply(eng.ctx, UMAT, lev0, xv.shape[0], SC, fl | (2 if acc else 0), None, 0,
                               xv.data_ptr(), xv.stride(0), yv.data_ptr(), yv.stride(0), ALPHA)
    assert rc == 0, (rc, lev0, fl, acc)


def _run(eng, x, base, nl, lev0, fl, acc):
    """rows 1 .. nl of a sentinel-filled array (acc: y = base, then accumulated `acc` times)"""
    import torch
    y = torch.full((nl + 3, x.shape[1]), SENTINEL, dtype=torch.float64, device=x.device)
    if acc:
        y[1:1 + nl] = base[:nl]
    for _ in range(max(acc, 1)):
        _call(eng, x[:nl], y[1:1 + nl], lev0, fl, acc)
    return y


CASES = [(nl, lev0, fl, acc) for nl in NLEVS for lev0 in _lev0s(nl) for fl in (0, 1) for acc in (0, 2)]


@pytest.fixture(scope="module")
def small():
    """the mesh, the inputs and the two-launch form's result of every case, computed once"""
    import torch
    dm = _mesh(3, 4, 6, NK)
    old = _engine(dm, MIMSEM_WAVE_OWN="0")
    r = np.random.default_rng(61)
    x = old.tensor(r.standard_normal((NK, dm.n1)))
    base = old.tensor(r.standard_normal((NK, dm.n1)))
    ref = {c: _run(old, x, base, *c) for c in CASES}
    for c, y in ref.items():
        assert bool((y[0] == SENTINEL).all()) and bool((y[1 + c[0]:] == SENTINEL).all()), c
    torch.cuda.synchronize()
    return dm, x, base, ref


def _check_all(eng, small, what):
    import torch
    dm, x, base, ref = small
    for c in CASES:
        y = _run(eng, x, base, *c)
        assert torch.equal(y, ref[c]), (what, c, int((y != ref[c]).sum()))      # (the guard rows are part of the comparison)


def test_default_rule_equals_the_two_launch_form_bit_for_bit(small):
    _check_all(_engine(small[0], MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE="0"), small, "default rule")


def test_row_slices_of_wider_arrays_with_different_strides(small):
    """x at row stride n1 + 5, 1 double in (every 16-byte alignment broken); y at n1 + 12, 2 doubles in; every word beside y stays"""
    import torch
    dm, x, base, ref = small
    eng = _engine(dm, MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE="0")
    n1 = dm.n1
    xw = torch.full((NK, n1 + 5), SENTINEL, dtype=torch.float64, device=x.device)
    xw[:, 1:1 + n1] = x
    for c in CASES:
        nl, lev0, fl, acc = c
        yw = torch.full((nl + 3, n1 + 12), SENTINEL, dtype=torch.float64, device=x.device)
        if acc:
            yw[1:1 + nl, 2:2 + n1] = base[:nl]
        for _ in range(max(acc, 1)):
            _call(eng, xw[:nl, 1:1 + n1], yw[1:1 + nl, 2:2 + n1], lev0, fl, acc)
        assert torch.equal(yw[:, 2:2 + n1], ref[c]), (c, int((yw[:, 2:2 + n1] != ref[c]).sum()))
        assert bool((yw[:, :2] == SENTINEL).all()) and bool((yw[:, 2 + n1:] == SENTINEL).all()), (c, "words beside the rows of y")
    assert bool((xw[:, :1] == SENTINEL).all()) and bool((xw[:, 1 + n1:] == SENTINEL).all()) and torch.equal(xw[:, 1:1 + n1], x)


@pytest.mark.parametrize("plev", [2, 6, 10], ids=["part2", "part6", "part10"])
@pytest.mark.parametrize("order", [1, 3], ids=["part_major", "group_major"])
def test_requested_parts(small, plev, order):
    eng = _engine(small[0], MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE="0")
    assert eng.L.mimsem_ctx_set_wave_split(eng.ctx, plev, order) == 0
    _check_all(eng, small, "parts of %d levels, order %d" % (plev, order))


@pytest.mark.parametrize("ncu,k", [(5, 2), (7, 2)], ids=["5cu_x2", "7cu_x2"])
def test_planned_list_under_a_pretended_chip(small, ncu, k):
    eng = _engine(small[0], MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE=None)
    eng.set_wave_balance(ncu, k)
    _check_all(eng, small, "%d CUs x %d" % (ncu, k))
    assert int(eng.L.mimsem_ctx_wave_balance_launches(eng.ctx)) > 0, "the list kernel never ran"


def test_one_captured_graph_replayed_three_times(small):
    import torch
    dm, x, base, ref = small
    eng = _engine(dm, MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE="0")
    old = _engine(dm, MIMSEM_WAVE_OWN="0")
    nl, lev0, fl = 15, 2, 1
    want = _run(old, x, base, nl, lev0, fl, 3)
    y = torch.full((nl + 3, dm.n1), SENTINEL, dtype=torch.float64, device=x.device)
    g, _ = eng.capture(lambda: _call(eng, x[:nl], y[1:1 + nl], lev0, fl, 1))
    y.fill_(SENTINEL); y[1:1 + nl] = base[:nl]
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want), int((y != want).sum())
