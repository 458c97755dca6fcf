"""Packed ghost lanes of the owner-computes Umat kernel (k_apply_wave<3, UMAT, ..., OWN>): the neighbour's side
terms run on one DPP row of x-normal sides and one of y-normal sides per level, and must still give the bits of the two-launch form
(MIMSEM_WAVE_OWN=0).  Sphere meshes of several sizes: groups with four ghost sides of both kinds, sides across cube-panel edges (the
neighbour's orientation rotated), ragged level counts for the lock-step batches."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import SCALE
from tests.test_gpu_wave_owner import _mesh, _stats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (p, ne, patches, levels): every cube-panel edge of the sphere is a ghost side somewhere; odd level counts leave ragged batches
MESHES = [(3, 2, 6, 5), (3, 6, 6, 9), (3, 8, 6, 7), (3, 12, 6, 3)]


def _plan_line(pn, ne, npatch, nk):
    """the owner plan's summary line (MIMSEM_VERBOSE), from a fresh process"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests.test_gpu_wave_owner import _mesh\n"
            "from mimsem_amd.device import Engine\n"
            "Engine(_mesh(%d, %d, %d, %d))\n") % (ROOT, pn, ne, npatch, nk)
    env = dict(os.environ, MIMSEM_VERBOSE="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stderr.splitlines() if "owner-computes form" in l]
    return lines[-1] if lines else ""


def test_some_groups_have_four_ghost_sides_of_both_kinds():
    full = 0
    for m in MESHES[1:3]:
        line = _plan_line(*m)
        assert "owner-computes form" in line, (m, line)
        full += int(line.split("per group; ")[1].split(" groups")[0])
    assert full > 0


@pytest.fixture(scope="module", params=MESHES, ids=lambda m: "p%d_ne%d_nk%d" % (m[0], m[1], m[3]))
def pair(request):
    from mimsem_amd.device import Engine
    pn, ne, npatch, nk = request.param
    dm = _mesh(pn, ne, npatch, nk)
    own = Engine(dm)
    os.environ["MIMSEM_WAVE_OWN"] = "0"
    try:
        old = Engine(dm)
    finally:
        del os.environ["MIMSEM_WAVE_OWN"]
    return request.param, dm, own, old


def test_packed_ghost_lanes_equal_two_launch_form(pair):
    import torch
    (pn, ne, npatch, nk), dm, own, old = pair
    ok, st = _stats(own, nk)
    assert ok == 1 and st[1] == dm.n1 and st[2] == 0 and st[3] == 0, st      # the owner form applies
    r = np.random.default_rng(11)
    ranges = [(l0, n) for l0 in range(nk) for n in range(1, nk - l0 + 1)]
    x = own.tensor(r.standard_normal((nk, dm.n1)))
    for fl in (0, 1):
        for lev0, nl in ranges:
            a = own.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl)
            b = old.apply("UMAT", x[:nl], lev0=lev0, scale=SCALE, flags=fl)
            assert torch.equal(a, b), (ne, fl, lev0, nl, int((a != b).sum()))
        base = own.tensor(r.standard_normal((nk, dm.n1)))
        ya, yb = base.clone(), base.clone()
        own.apply("UMAT", x, lev0=0, scale=SCALE, flags=fl | 2, alpha=0.5, out=ya)
        old.apply("UMAT", x, lev0=0, scale=SCALE, flags=fl | 2, alpha=0.5, out=yb)
        assert torch.equal(ya, yb), (ne, fl, "accumulate", int((ya != yb).sum()))
    # signed zeros and exact zeros survive as the neighbour's own chains leave them
    z = own.tensor(np.zeros((nk, dm.n1))) * -1.0
    assert torch.equal(own.apply("UMAT", z, lev0=0, scale=SCALE, flags=1).view(torch.int64),
                       old.apply("UMAT", z, lev0=0, scale=SCALE, flags=1).view(torch.int64))
