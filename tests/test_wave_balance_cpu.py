"""The host planner of the owner form's level ranges (csrc/wave_balance.hpp, DESIGN 4.8: which (group, first level, levels) items a
launch has and which four share a workgroup) through tests/cpp/wave_balance_cli.cpp, a plain C++ program: every (group, level) in
exactly one item, items inside a group, from an even level over whole pairs, exactly WNW x workgroups of them, a group's items
neighbours, workgroup totals at most 2 pairs apart, no item longer than the default rule's longest plus a pair, no single pair unless
the call has fewer than 4 levels -- and a workgroup count the call cannot fill is refused with a status, not met with empty items.
The checker itself is checked on plans spoilt by one level."""
import os
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WNW = 4
OK, ARG, INFEASIBLE = 0, 1, 2


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wave_balance") / "wave_balance_cli")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "wave_balance_cli.cpp"), "-o", exe])
    return exe


def default_longest(ngroups, nlev):
    """the longest item of the default rule (csrc/api.hip: wave_level_parts without a requested split), restated"""
    lch = max(1, min(8, nlev))
    nch = -(-nlev // lch)
    cpp = 1
    if lch == 8 and nch > 1:
        nparts = min(nch, max(1, -(-1536 // ngroups)))
        nparts = next(n for n in range(nparts, nch + 1) if nch % n == 0)
        cpp = -(-nch // nparts)
    return min(nlev, 2 * ((lch * cpp + 1) // 2))


def plan(cli, ngroups, nlev, nwg, fault=None, wnw=WNW):
    args = [cli] + [str(v) for v in (ngroups, nlev, wnw, nwg, default_longest(ngroups, nlev))] + ([fault] if fault else [])
    out = subprocess.run(args, capture_output=True, text=True, check=True).stdout.split()
    rc, n = int(out[0]), int(out[1])
    v = [int(t) for t in out[2:]]
    assert len(v) == 3 * n
    return rc, [tuple(v[3 * i:3 * i + 3]) for i in range(n)]


def check(items, ngroups, nlev, nwg, wnw=WNW):
    """the hard properties; returns the histogram of item lengths in pairs"""
    assert len(items) == wnw * nwg, (len(items), wnw * nwg)
    seen = Counter()
    for g, l0, n in items:
        assert 0 <= g < ngroups and n >= 1 and l0 >= 0 and l0 + n <= nlev, (g, l0, n)
        assert l0 % 2 == 0, (g, l0, n)
        assert n % 2 == 0 or l0 + n == nlev, ("a half pair inside a group", g, l0, n)      # whole pairs, but for an odd nlev's last level
        for lev in range(l0, l0 + n):
            seen[(g, lev)] += 1
    assert len(seen) == ngroups * nlev, ("levels missing", ngroups * nlev - len(seen))
    assert max(seen.values()) == 1, ("levels computed twice", [k for k, c in seen.items() if c > 1][:4])
    # a group's items are neighbours in the order, and ascend
    last = {}
    for i, (g, l0, n) in enumerate(items):
        if g in last:
            assert last[g][0] == i - 1 and last[g][1] == l0, ("a group's items apart or out of order", g, i)
        else:
            assert l0 == 0
        last[g] = (i, l0 + n)
    pairs = [(n + 1) // 2 for _, _, n in items]
    totals = [sum(pairs[w * wnw:(w + 1) * wnw]) for w in range(nwg)]
    assert max(totals) - min(totals) <= 2, (min(totals), max(totals))
    assert max(pairs) <= (default_longest(ngroups, nlev) + 1) // 2 + 1, (max(pairs), default_longest(ngroups, nlev))
    assert nlev < 4 or min(pairs) >= 2, min(pairs)
    return Counter(pairs)


# (groups, levels, workgroups): the benchmark sphere around its level count on 2 and 3 workgroups per CU of 256, a short call, the small
# sphere of the GPU tests on pretended chips, one group
FEASIBLE = [(864, nl, nwg) for nwg in (512, 768) for nl in (29, 30, 31)] + [(864, 12, 512)] + \
           [(24, 4, 6), (24, 5, 6), (24, 7, 6), (24, 7, 10)]
# too few cells: 40 items of at least 2 pairs where 24 groups have 2 or 3 pairs each; 8 items in 15 pairs; 256 items in 24 pairs.
# Too many: 24 x 15 pairs in 24 or 40 items of at most 5 (the default rule cuts the small sphere into parts of 8 levels)
REFUSED = [(24, 4, 10), (24, 5, 10), (1, 30, 2), (24, 2, 64), (24, 30, 6), (24, 30, 10)]


@pytest.mark.parametrize("ngroups,nlev,nwg", FEASIBLE, ids=["%dx%d_on_%d" % s for s in FEASIBLE])
def test_plan_has_the_hard_properties(cli, ngroups, nlev, nwg):
    rc, items = plan(cli, ngroups, nlev, nwg)
    assert rc == OK, rc
    hist = check(items, ngroups, nlev, nwg)
    print("%d groups x %d levels on %d workgroups: items of (pairs: count) %s" % (ngroups, nlev, nwg, dict(sorted(hist.items()))))


@pytest.mark.parametrize("ngroups,nlev,nwg", REFUSED, ids=["%dx%d_on_%d" % s for s in REFUSED])
def test_a_count_the_call_cannot_fill_is_refused(cli, ngroups, nlev, nwg):
    lo = 1 if nlev < 4 else 2
    hi = (default_longest(ngroups, nlev) + 1) // 2 + 1
    per_group = ((nlev + 1) // 2) // lo                  # items a group can be cut into at most
    assert ngroups * per_group < WNW * nwg or WNW * nwg * hi < ngroups * ((nlev + 1) // 2)      # (the case is what it claims to be)
    rc, items = plan(cli, ngroups, nlev, nwg)
    assert rc == INFEASIBLE and items == [], (rc, len(items))


def test_bad_arguments_are_refused(cli):
    for ngroups, nlev, nwg in [(0, 30, 2), (24, 0, 2), (24, 30, 0)]:
        args = [cli, str(ngroups), str(nlev), "4", str(nwg), "8"]
        out = subprocess.run(args, capture_output=True, text=True, check=True).stdout.split()
        assert out[:2] == [str(ARG), "0"], out[:2]


@pytest.mark.parametrize("fault", ["drop", "double"])
@pytest.mark.parametrize("ngroups,nlev,nwg", [(864, 30, 512), (24, 7, 10)])
def test_the_checker_notices_a_dropped_or_doubled_level(cli, ngroups, nlev, nwg, fault):
    rc, items = plan(cli, ngroups, nlev, nwg, fault=fault)
    assert rc == OK
    with pytest.raises(AssertionError):
        check(items, ngroups, nlev, nwg)
