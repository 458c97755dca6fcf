"""The owner-computes Umat kernel with one ghost pass per FOUR levels (own4::k_apply_wave<3, UMAT, 8, ACCUM>; csrc/api.hip
build_wave_own, gh4): ghost side b is DPP row b, the four levels of a double batch lie across it, the pass runs at the even batches of
the ring and a lane of the second batch hands its result over one batch later.  None of that may change a bit of the result: the form
is compared BIT FOR BIT with the two-launch form (MIMSEM_WAVE_OWN=0) and with the pass per batch of two levels (MIMSEM_WAVE_OWN=1) for
level counts around every pass, batch, ring and item boundary (odd and even batch counts, a half-empty last pass), geometry sub-ranges
with lev0 odd and even, both flags and the accumulate form, with guard rows around the range, and for requested parts in both item
orders.  The small sphere holds all three mixes of ghost sides (2 + 2, 4 + 0, 0 + 4 x-normal + y-normal), which the plan line of
MIMSEM_VERBOSE reports."""
import os
import re

import numpy as np
import pytest

from tests.helpers import SCALE, z_levels

pytestmark = pytest.mark.gpu

NLEVS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 14, 16, 17, 29, 30, 31]
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
    """an Engine made under the given switches (None: unset); they are read at context creation"""
    from mimsem_amd.device import Engine
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return Engine(dm)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _forms(dm):
    return (_engine(dm, MIMSEM_WAVE_OWN=None), _engine(dm, MIMSEM_WAVE_OWN="1"), _engine(dm, MIMSEM_WAVE_OWN="0"))


@pytest.fixture(scope="module")
def small():
    dm = _mesh(3, 4, 6, NK)               # 24 wave-groups
    return (dm,) + _forms(dm)


def _compare(dm, new, refs, nlevs, lev0s, seed):
    import torch
    r = np.random.default_rng(seed)
    x = new.tensor(r.standard_normal((NK, dm.n1)))
    base = new.tensor(r.standard_normal((NK, dm.n1)))
    for nl in nlevs:
        for lev0 in lev0s:
            if lev0 + nl > NK:
                continue
            for fl in (0, 1):
                ya = torch.full((nl + 3, dm.n1), SENTINEL, dtype=torch.float64, device=x.device)
                new.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl, out=ya[1:1 + nl])
                assert bool((ya[0] == SENTINEL).all()) and bool((ya[1 + nl:] == SENTINEL).all()), (nl, lev0, fl, "rows beyond the range")
                za = ya.clone(); za[1:1 + nl] = base[:nl]
                new.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl | 2, alpha=0.25, out=za[1:1 + nl])
                assert bool((za[0] == SENTINEL).all()) and bool((za[1 + nl:] == SENTINEL).all()), (nl, lev0, fl, "accumulate: rows beyond")
                for k, ref in enumerate(refs):
                    yb = torch.full((nl + 3, dm.n1), SENTINEL, dtype=torch.float64, device=x.device)
                    ref.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl, out=yb[1:1 + nl])
                    assert torch.equal(ya, yb), (nl, lev0, fl, k, int((ya != yb).sum()))
                    yb[1:1 + nl] = base[:nl]
                    ref.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl | 2, alpha=0.25, out=yb[1:1 + nl])
                    assert torch.equal(za, yb), (nl, lev0, fl, k, "accumulate", int((za != yb).sum()))


def test_plan_reports_all_three_side_mixes(capfd):
    """every group of the small sphere has 4 ghost sides: 2 + 2, 4 + 0 and 0 + 4 all occur, nothing else; the default is the new pass"""
    dm = _mesh(3, 4, 6, NK)
    capfd.readouterr()
    _engine(dm, MIMSEM_VERBOSE="1", MIMSEM_WAVE_OWN=None)
    err = capfd.readouterr().err
    m = re.search(r"(\d+) groups 2 \+ 2, (\d+) groups 4 \+ 0, (\d+) groups 0 \+ 4, (\d+) other; ghost pass per four levels", err)
    assert m, err[-1500:]
    n22, n40, n04, other = map(int, m.groups())
    assert n22 > 0 and n40 > 0 and n04 > 0 and other == 0 and n22 + n40 + n04 == 24, m.groups()
    _engine(dm, MIMSEM_VERBOSE="1", MIMSEM_WAVE_OWN="1")
    assert "ghost pass per batch" in capfd.readouterr().err


def test_default_split_equals_both_other_forms_bit_for_bit(small):
    dm, new, own1, old = small
    _compare(dm, new, (old, own1), NLEVS, (0, 1, 3), seed=23)


PART_LEVELS = [2, 4, 6, 10, 32]


@pytest.mark.parametrize("plev", PART_LEVELS, ids=["part%d" % p for p in PART_LEVELS])
@pytest.mark.parametrize("order", [1, 3], ids=["part_major", "group_major"])
def test_requested_splits_equal_both_other_forms_bit_for_bit(small, plev, order):
    dm, _, own1, old = small
    alt = _engine(dm, MIMSEM_WAVE_OWN=None)
    assert alt.L.mimsem_ctx_set_wave_split(alt.ctx, plev, order) == 0
    _compare(dm, alt, (old, own1), NLEVS, (0, 1, 3), seed=29)


def test_benchmark_sphere():
    """the bench.py workload (p = 3, 24 x 24 x 6, 864 wave-groups): 30 levels as 16 + 14, and the counts next to it"""
    dm = _mesh(3, 24, 24, NK)
    new, own1, old = _forms(dm)
    _compare(dm, new, (old, own1), [29, 30, 31], (0, 1, 3), seed=31)
