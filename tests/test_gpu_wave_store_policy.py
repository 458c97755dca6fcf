"""Cache policies of the owner-computes Umat kernel's streams and the level clamp of its loads (own4::apply_wave_body):
which policy a store or a load carries, and which level a load past an item's end re-reads, may not change a bit of y.  On the
4 x 4 x 6 sphere (24 wave-groups, all three mixes of ghost sides) the default path is compared BIT FOR BIT with the two-launch form
(MIMSEM_WAVE_OWN=0) for level counts around every batch, pass, ring and item boundary, geometry sub-ranges with lev0 odd and even, both
values of the vertical flag, the accumulate form TWICE in a row (the second call reads the y the first one stored), guard rows on
either side of the range, requested parts of 2, 6 and 10 levels (items that end inside the call: their loads past the end re-read the
item's own last level), the planned item list, and a captured graph replayed three times."""
import numpy as np
import pytest

from tests.helpers import SCALE
from tests.test_gpu_wave_own4 import NK, SENTINEL, _engine, _mesh

pytestmark = pytest.mark.gpu

NLEVS = [2, 3, 5, 8, 9, 16, 17, 30, 31]
LEV0S = (0, 1, 3)
CASES = [(nl, lev0, fl) for nl in NLEVS for lev0 in LEV0S for fl in (0, 1)]       # (NK = 36: every count fits from every lev0)
PARTS = [2, 6, 10]


def _run(eng, x, base, nl, lev0, fl):
    """(plain result, the accumulate form applied twice onto `base`), each in rows 1 .. nl of a sentinel-filled buffer"""
    import torch
    y = torch.full((nl + 3, x.shape[1]), SENTINEL, dtype=torch.float64, device=x.device)
    eng.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl, out=y[1:1 + nl])
    z = torch.full((nl + 3, x.shape[1]), SENTINEL, dtype=torch.float64, device=x.device)
    z[1:1 + nl] = base[:nl]
    for _ in range(2):
        eng.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl | 2, alpha=0.25, out=z[1:1 + nl])
    return y, z


@pytest.fixture(scope="module")
def small():
    """the mesh, the inputs and the two-launch form's results, computed once: {case: (y, z) with their guard rows}"""
    import torch
    dm = _mesh(3, 4, 6, NK)
    old = _engine(dm, MIMSEM_WAVE_OWN="0")
    r = np.random.default_rng(47)
    x = old.tensor(r.standard_normal((NK, dm.n1)))
    base = old.tensor(r.standard_normal((NK, dm.n1)))
    ref = {c: _run(old, x, base, *c) for c in CASES}
    torch.cuda.synchronize()
    for c, (y, z) in ref.items():
        for t in (y, z):
            assert bool((t[0] == SENTINEL).all()) and bool((t[1 + c[0]:] == SENTINEL).all()), c
            assert bool(torch.isfinite(t[1:1 + c[0]]).all()) and bool((t[1:1 + c[0]] != SENTINEL).all()), c
    return dm, x, base, ref, old


def _check(eng, x, base, ref):
    import torch
    for c in CASES:
        y, z = _run(eng, x, base, *c)
        assert torch.equal(y, ref[c][0]), (c, int((y != ref[c][0]).sum()))        # (the guard rows are part of the comparison)
        assert torch.equal(z, ref[c][1]), (c, "accumulate twice", int((z != ref[c][1]).sum()))


def test_default_path_equals_two_launch_form_bit_for_bit(small):
    dm, x, base, ref, _ = small
    _check(_engine(dm, MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE=None), x, base, ref)


@pytest.mark.parametrize("plev", PARTS, ids=["part%d" % p for p in PARTS])
@pytest.mark.parametrize("order", [1, 3], ids=["part_major", "group_major"])
def test_items_that_end_inside_the_call(small, plev, order):
    dm, x, base, ref, _ = small
    eng = _engine(dm, MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE=None)
    assert eng.L.mimsem_ctx_set_wave_split(eng.ctx, plev, order) == 0
    _check(eng, x, base, ref)


def test_planned_item_list(small):
    """own4::k_apply_wave_list shares the body: a pretended chip of 11 CUs x 3 workgroups engages it on the long calls"""
    dm, x, base, ref, _ = small
    eng = _engine(dm, MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE=None)
    eng.set_wave_balance(11, 3)
    _check(eng, x, base, ref)
    assert int(eng.L.mimsem_ctx_wave_balance_launches(eng.ctx)) > 0


def test_captured_graph_replayed_three_times(small):
    import torch
    from mimsem_amd.device import no_gc
    dm, x, base, _, old = small
    nl, lev0, fl = 30, 1, 1
    eng = _engine(dm, MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE=None)
    z = torch.full((nl + 3, dm.n1), SENTINEL, dtype=torch.float64, device=x.device)
    z[1:1 + nl] = base[:nl]
    eng.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl | 2, alpha=0.25, out=z[1:1 + nl])      # workspaces reach their size
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with no_gc(), torch.cuda.graph(g), eng.on_current_stream():
        eng.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl | 2, alpha=0.25, out=z[1:1 + nl])
    torch.cuda.synchronize()
    z.fill_(SENTINEL); z[1:1 + nl] = base[:nl]
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    want = torch.full((nl + 3, dm.n1), SENTINEL, dtype=torch.float64, device=x.device)
    want[1:1 + nl] = base[:nl]
    for _ in range(3):
        old.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl | 2, alpha=0.25, out=want[1:1 + nl])
    assert torch.equal(z, want), int((z != want).sum())
