"""Level ranges of the owner-computes kernel (k_apply_wave<3, UMAT, ..., OWN>; csrc/api.hip wave_level_parts): a work item is
(wave-group, first level, number of levels), the parts of a group are whole level pairs (by default the chunk form's items, 11 levels
as 8 + 3; a requested part length is dealt evenly, lengths at most one pair apart), and a
wavefront leaves the level loop at the first batch boundary at or beyond its last level.  Which levels a wavefront walks must not change
a bit of the result: the owner form is compared BIT FOR BIT with the two-launch form (MIMSEM_WAVE_OWN=0, whose items are the chunks of 8
levels) for level counts around every batch, ring and part boundary, with geometry sub-ranges (lev0 > 0), both flags and the accumulate
form, and the rows of y next to the range must keep what they held.  The default split follows the chunk form's items; every other
split -- 10 + 10 + 10, 8 + 8 + 8 + 6, parts of one batch, a single part -- and the part-major item order are reached through
mimsem_ctx_set_wave_split, in the library every build makes (MIMSEM_WAVE_LCH / MIMSEM_WAVE_CPP ask for the same in an experiments build)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.helpers import SCALE, z_levels

pytestmark = pytest.mark.gpu

NLEVS = [1, 2, 3, 7, 8, 9, 14, 15, 16, 17, 29, 30, 31, 32, 33]
NK = 36                                   # levels of the geometry: every count above from lev0 = 0 .. 3
SENTINEL = -7.25e300                      # what the guard rows around the range hold


def _mesh(pn, ne, npatch, nk):
    from mimsem_amd.device import DeviceMesh
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    cs = CubedSphere(pn, ne, npatch); coords = sphere_coords(pn, ne)
    topos = [Topo(cs, p, nk) for p in range(npatch)]
    geoms = [Geom(t, cs, coords, nk) for t in topos]
    for g in geoms:
        g.set_levels(z_levels(nk, g.n0))
    return DeviceMesh(topos, geoms, nk=nk, numbering="global")


def _engine(dm, **env):
    from mimsem_amd.device import Engine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Engine(dm)                 # the switches are read at context creation
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _longest(eng, nlev):
    st = (C.c_int * 5)()
    assert eng.L.mimsem_op_wave_stats(eng.ctx, nlev, st) == 1, list(st)
    assert st[1] == eng.mesh.n1 and st[2] == 0 and st[3] == 0, list(st)          # the owner form is what runs
    return int(st[4])


def _ngroups(eng):
    st = (C.c_int * 5)()
    assert eng.L.mimsem_op_wave_stats(eng.ctx, 1, st) == 1
    return int(st[0])


def _even_longest(nlev, part_levels):
    """What the issue's rule fixes without looking at the code: the fewest parts of at most `part_levels` levels (in whole level pairs),
    lengths even and at most one pair apart, together exactly nlev levels -- then the longest part holds ceil(pairs / parts) pairs, cut
    to nlev where an odd count leaves a single part one level short."""
    pairs = (nlev + 1) // 2
    nparts = -(-pairs // ((part_levels + 1) // 2))
    return min(nlev, 2 * -(-pairs // nparts))


@pytest.fixture(scope="module")
def small():
    dm = _mesh(3, 4, 6, NK)               # 24 wave-groups: the default rule cuts as fine as it ever does (parts of 6 and 8 levels)
    return dm, _engine(dm), _engine(dm, MIMSEM_WAVE_OWN="0")


def _compare(dm, own, old, nlevs, lev0s, seed):
    import torch
    r = np.random.default_rng(seed)
    x = own.tensor(r.standard_normal((NK, dm.n1)))
    base = own.tensor(r.standard_normal((NK, dm.n1)))
    for nl in nlevs:
        for lev0 in lev0s:
            if lev0 + nl > NK:
                continue
            for fl in (0, 1):
                ya = torch.full((nl + 3, dm.n1), SENTINEL, dtype=torch.float64, device=x.device)
                yb = ya.clone()
                own.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl, out=ya[1:1 + nl])
                old.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl, out=yb[1:1 + nl])
                assert torch.equal(ya[1:1 + nl], yb[1:1 + nl]), (nl, lev0, fl, int((ya != yb).sum()))
                assert bool((ya[0] == SENTINEL).all()) and bool((ya[1 + nl:] == SENTINEL).all()), (nl, lev0, fl, "rows beyond the range")
                ya[1:1 + nl] = base[:nl]; yb[1:1 + nl] = base[:nl]
                own.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl | 2, alpha=0.25, out=ya[1:1 + nl])
                old.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl | 2, alpha=0.25, out=yb[1:1 + nl])
                assert torch.equal(ya[1:1 + nl], yb[1:1 + nl]), (nl, lev0, fl, "accumulate", int((ya != yb).sum()))
                assert bool((ya[0] == SENTINEL).all()) and bool((ya[1 + nl:] == SENTINEL).all()), (nl, lev0, fl, "accumulate: rows beyond")


def test_default_split_equals_two_launch_form_bit_for_bit(small):
    dm, own, old = small
    st = (C.c_int * 5)()
    for nl in NLEVS:
        assert old.L.mimsem_op_wave_stats(old.ctx, nl, st) == 1
        assert _longest(own, nl) == st[4] <= nl, (nl, _longest(own, nl), list(st))       # one number per context, whichever form runs
    _compare(dm, own, old, NLEVS, (0, 1, 3), seed=11)


# levels of a part asked for: 2 (one batch), 3 (rounded up to 2 pairs), 8 (the ring), 10, 16, 32 (a single part for most counts)
PART_LEVELS = [2, 3, 8, 10, 16, 32]


@pytest.mark.parametrize("plev", PART_LEVELS, ids=["part%d" % p for p in PART_LEVELS])
@pytest.mark.parametrize("order", [1, 3], ids=["part_major", "group_major"])
def test_requested_splits_equal_two_launch_form_bit_for_bit(small, plev, order):
    dm, own, old = small
    alt = _engine(dm)
    assert alt.L.mimsem_ctx_set_wave_split(alt.ctx, plev, order) == 0
    for nl in NLEVS:
        assert _longest(alt, nl) == _even_longest(nl, plev), (nl, plev, _longest(alt, nl))
    _compare(dm, alt, old, NLEVS, (0, 2), seed=13)
    assert alt.L.mimsem_ctx_set_wave_split(alt.ctx, 0, -1) == 0                           # back to the library's rule, the order kept
    assert [_longest(alt, nl) for nl in NLEVS] == [_longest(own, nl) for nl in NLEVS]
    assert alt.L.mimsem_ctx_set_wave_split(alt.ctx, -1, 3) == -1 and alt.L.mimsem_ctx_set_wave_split(alt.ctx, 8, 4) == -1


def test_benchmark_sphere_split():
    """the bench.py workload (p = 3, 24 x 24 x 6, 864 wave-groups): 30 levels in two parts of 16 + 14, and the counts around them;
    then the split that measured fastest there (10 + 10 + 10), which is not the default"""
    dm = _mesh(3, 24, 24, NK)
    own, old = _engine(dm), _engine(dm, MIMSEM_WAVE_OWN="0")
    assert _ngroups(own) == 864 and _longest(own, 30) == 16
    _compare(dm, own, old, [1, 15, 16, 17, 29, 30, 31, 32, 33], (0, 3), seed=17)
    assert own.L.mimsem_ctx_set_wave_split(own.ctx, 10, -1) == 0 and _longest(own, 30) == 10
    _compare(dm, own, old, [29, 30, 31], (0, 3), seed=19)
