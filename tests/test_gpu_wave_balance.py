"""Balanced level ranges of the owner-computes Umat kernel (own4::k_apply_wave with a planned item list: csrc/wave_balance.hpp,
mimsem_ctx_set_wave_balance).  Which ranges exist and which four share a workgroup may not change a bit of the result: on
the small sphere (24 wave-groups) the planner is engaged through the setter with pretended chips -- 5 and 7 CUs at 2 workgroups per
CU, 3 CUs at 3 (whose 9 workgroups the default rule's 6, 12, 18 or 24 never leave room for: the default rule stays), and 13 CUs at 2
and 11 at 3, which reach the long calls -- and compared BIT FOR BIT with the two-launch form (MIMSEM_WAVE_OWN=0) and with the default
split (MIMSEM_WAVE_BALANCE=0) for level counts around every pass, batch, ring and item boundary, geometry sub-ranges with lev0 odd
and even, both flags and the accumulate form, with guard rows around the range.  What the context reports (mimsem_op_wave_stats
out[4]) is the longest item of the list tests/cpp/wave_balance_cli.cpp prints for the same call, or the default rule's where the
planner has nothing to do or refuses, and the launches that ran from a list are counted where the kernel is launched
(mimsem_ctx_wave_balance_launches: exactly the calls the rule engages, none else); a call captured before the list exists keeps the default rule, one captured after it uses the
list, and both replay bit-equal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import SCALE
from tests.test_gpu_wave_own4 import NK, SENTINEL, _engine, _mesh
from tests.test_wave_balance_cpu import default_longest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLEVS = [2, 3, 4, 5, 7, 8, 9, 14, 16, 17, 30, 31]
LEV0S = (0, 1, 3)
CHIPS = [(5, 2), (7, 2), (3, 3), (13, 2), (11, 3)]       # (pretended CUs, workgroups per CU)
WNW, NGROUPS = 4, 24


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wave_balance") / "wave_balance_cli")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "wave_balance_cli.cpp"), "-o", exe])
    return exe


def _planned_longest(cli, ngroups, nlev, ncu, k):
    """the longest item (levels) a context must report once its list is made: the rule of csrc/api.hip (wave_balance_workgroups)
    restated, the plan from the CLI"""
    dl = default_longest(ngroups, nlev)
    parts = -(-((nlev + 1) // 2) // ((dl + 1) // 2))      # parts per group of the default rule
    wgs = -(-ngroups * parts // WNW)
    if nlev < 2 or wgs > 3 * ncu or wgs % ncu == 0:
        return dl, False
    out = subprocess.run([cli] + [str(v) for v in (ngroups, nlev, WNW, k * ncu, dl)], capture_output=True, text=True, check=True).stdout.split()
    if int(out[0]) != 0:
        return dl, False
    return max(int(v) for v in out[4::3]), True


def _longest(eng, nlev):
    st = (C.c_int * 5)()
    assert eng.L.mimsem_op_wave_stats(eng.ctx, nlev, st) == 1, list(st)
    return int(st[4])


def _listed(eng):
    """launches of the list kernel on this context so far, counted at the launch site"""
    return int(eng.L.mimsem_ctx_wave_balance_launches(eng.ctx))


def _apply(eng, x, base, nl, lev0, fl, acc):
    """UMAT into rows 1 .. nl of a sentinel-filled buffer (accumulate form: onto `base`)"""
    import torch
    y = torch.full((nl + 3, x.shape[1]), SENTINEL, dtype=torch.float64, device=x.device)
    if acc:
        y[1:1 + nl] = base[:nl]
        eng.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl | 2, alpha=0.25, out=y[1:1 + nl])
    else:
        eng.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl, out=y[1:1 + nl])
    return y


CASES = [(nl, lev0, fl, acc) for nl in NLEVS for lev0 in LEV0S if lev0 + nl <= NK for fl in (0, 1) for acc in (0, 1)]


@pytest.fixture(scope="module")
def small():
    """the mesh, the inputs and the results of the default split, computed once: {case: rows with their guard rows}"""
    import torch
    dm = _mesh(3, 4, 6, NK)
    off = _engine(dm, MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE="0")
    r = np.random.default_rng(41)
    x = off.tensor(r.standard_normal((NK, dm.n1)))
    base = off.tensor(r.standard_normal((NK, dm.n1)))
    ref = {c: _apply(off, x, base, *c) for c in CASES}
    for c, y in ref.items():
        assert bool((y[0] == SENTINEL).all()) and bool((y[1 + c[0]:] == SENTINEL).all()), c
    torch.cuda.synchronize()
    return dm, x, base, ref, off


def test_default_split_equals_two_launch_form(small):
    import torch
    dm, x, base, ref, off = small
    old = _engine(dm, MIMSEM_WAVE_OWN="0")
    for c in CASES:
        assert torch.equal(_apply(old, x, base, *c), ref[c]), c
    for nl in NLEVS:                                     # MIMSEM_WAVE_BALANCE=0: the default rule's figure, before and after calls
        assert _longest(off, nl) == default_longest(NGROUPS, nl), nl
    assert _listed(off) == 0 and _listed(old) == 0       # ... and its kernel


@pytest.mark.parametrize("ncu,k", CHIPS, ids=["%dcu_x%d" % c for c in CHIPS])
def test_planned_ranges_equal_the_default_split_bit_for_bit(small, cli, ncu, k):
    import torch
    dm, x, base, ref, _ = small
    eng = _engine(dm, MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE=None)
    eng.set_wave_balance(ncu, k)
    plans = {nl: _planned_longest(cli, NGROUPS, nl, ncu, k) for nl in NLEVS}
    engaged = [nl for nl in NLEVS if plans[nl][1]]
    for nl in NLEVS:
        assert _longest(eng, nl) == default_longest(NGROUPS, nl), nl      # no list yet
    assert _listed(eng) == 0
    for c in CASES:
        n0 = _listed(eng)
        y = _apply(eng, x, base, *c)
        assert torch.equal(y, ref[c]), (c, int((y != ref[c]).sum()))      # (the guard rows are part of the comparison)
        assert _listed(eng) - n0 == (1 if c[0] in engaged else 0), (c, "the list kernel ran exactly where the rule engages it")
    for nl in NLEVS:
        assert _longest(eng, nl) == plans[nl][0], (nl, _longest(eng, nl), plans[nl])
    print("%d CUs x %d: planner engaged at %s levels" % (ncu, k, engaged))
    assert bool(engaged) == ((ncu, k) != (3, 3)), engaged
    for _ in range(10):                                  # the same call again and again
        c = (engaged[-1] if engaged else 30, 1, 1, 1)
        assert torch.equal(_apply(eng, x, base, *c), ref[c])


def test_long_calls_are_engaged_on_the_small_sphere(cli):
    """the pretended chips of 13 and 11 CUs reach the 30- and 31-level calls (the issue's three chips do not: the default rule's 24
    workgroups are more than 3 per CU of theirs)"""
    assert all(_planned_longest(cli, NGROUPS, nl, 13, 2)[1] and _planned_longest(cli, NGROUPS, nl, 11, 3)[1] for nl in (30, 31))


def test_capture_before_and_after_the_list_exists(small, cli):
    import torch
    from mimsem_amd.device import no_gc
    dm, x, base, ref, _ = small
    eng = _engine(dm, MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE=None)
    assert eng.L.mimsem_ctx_set_wave_balance(eng.ctx, 11, 3) == 0
    nl, lev0, fl = 30, 1, 1
    want, on = _planned_longest(cli, NGROUPS, nl, 11, 3)
    assert on and want != default_longest(NGROUPS, nl)   # (6 against 8: the two rules can be told apart)
    _apply(eng, x, base, 31, 0, 0, 0)                    # another level count: the workspace reaches its size, no list for 30 levels
    y = torch.full((nl + 3, dm.n1), SENTINEL, dtype=torch.float64, device=x.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    n0 = _listed(eng)
    with no_gc(), torch.cuda.graph(g), eng.on_current_stream():
        eng.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl, out=y[1:1 + nl])
    torch.cuda.synchronize()
    assert _listed(eng) == n0                            # the default rule's kernel was recorded
    assert _longest(eng, nl) == default_longest(NGROUPS, nl)      # captured without a list: the default rule, and no list was made
    y.fill_(SENTINEL); g.replay(); torch.cuda.synchronize()
    assert torch.equal(y, ref[(nl, lev0, fl, 0)])
    assert torch.equal(_apply(eng, x, base, nl, lev0, fl, 0), ref[(nl, lev0, fl, 0)])      # eager: plans and uploads the list
    assert _longest(eng, nl) == want and _listed(eng) == n0 + 1
    y2 = torch.full((nl + 3, dm.n1), SENTINEL, dtype=torch.float64, device=x.device)
    g2, _ = eng.capture(lambda: eng.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl, out=y2[1:1 + nl]))
    assert _listed(eng) == n0 + 3                        # the warm-up call and the recorded one both ran from the list
    y2.fill_(SENTINEL); g2.replay(); torch.cuda.synchronize()
    assert torch.equal(y2, ref[(nl, lev0, fl, 0)])
    y.fill_(SENTINEL); g.replay(); torch.cuda.synchronize()      # the first recording still replays its own launch
    assert torch.equal(y, ref[(nl, lev0, fl, 0)])


def test_setter_argument_errors_change_nothing(small, cli):
    import torch
    dm, x, base, ref, _ = small
    eng = _engine(dm, MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE=None)
    L = eng.L
    assert L.mimsem_ctx_set_wave_balance(eng.ctx, 7, 2) == 0
    c = (17, 0, 0, 0)
    assert torch.equal(_apply(eng, x, base, *c), ref[c])
    want, on = _planned_longest(cli, NGROUPS, 17, 7, 2)
    assert on and want != default_longest(NGROUPS, 17) and _longest(eng, 17) == want
    for ncu, k in [(7, 0), (7, 4), (0, -1), (0, 7), ((1 << 20) + 1, 2)]:
        assert L.mimsem_ctx_set_wave_balance(eng.ctx, ncu, k) == -1, (ncu, k)
    assert L.mimsem_ctx_set_wave_balance(None, 7, 2) == -1
    from mimsem_amd._lib import MimsemError
    for ncu, k in [(7, 0), (0, 4)]:                      # the Engine's wrapper refuses the same before it reaches the library
        with pytest.raises(MimsemError):
            eng.set_wave_balance(ncu, k)
    assert _longest(eng, 17) == want                     # the list and the setting are what they were
    n0 = _listed(eng)
    assert torch.equal(_apply(eng, x, base, *c), ref[c]) and _listed(eng) == n0 + 1      # ... and still in force
    eng.set_wave_balance(-1, 0)                          # off: wgs_per_cu is not looked at
    assert torch.equal(_apply(eng, x, base, *c), ref[c]) and _longest(eng, 17) == default_longest(NGROUPS, 17)
    assert _listed(eng) == n0 + 1


def test_benchmark_sphere_on_the_device_own_cus(cli):
    """the bench.py workload (p = 3, 24 x 24 x 6, 864 wave-groups, 30 levels) with the device's CU count against MIMSEM_WAVE_BALANCE=0"""
    import torch
    dm = _mesh(3, 24, 24, NK)
    new = _engine(dm, MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE=None)
    off = _engine(dm, MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE="0")
    new.set_wave_balance(0, 2)                           # engaged whatever the library's default is
    r = np.random.default_rng(43)
    x = new.tensor(r.standard_normal((NK, dm.n1))); base = new.tensor(r.standard_normal((NK, dm.n1)))
    for c in [(30, 0, 0, 0), (30, 3, 1, 1)]:
        ya, yb = _apply(new, x, base, *c), _apply(off, x, base, *c)
        assert torch.equal(ya, yb), (c, int((ya != yb).sum()))
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    want, on = _planned_longest(cli, 864, 30, ncu, 2)
    assert on and _longest(new, 30) == want and _longest(off, 30) == 16, (_longest(new, 30), want, on)
    assert _listed(new) == 2 and _listed(off) == 0
    assert new.L.mimsem_ctx_set_wave_balance(new.ctx, 0, 3) == 0      # three workgroups per CU: shorter items
    c = (30, 1, 0, 1)
    ya, yb = _apply(new, x, base, *c), _apply(off, x, base, *c)
    assert torch.equal(ya, yb), (c, int((ya != yb).sum()))
    assert _longest(new, 30) == _planned_longest(cli, 864, 30, ncu, 3)[0]
