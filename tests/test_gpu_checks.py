"""The check log of the Python hosts (mimsem_amd/checks.py) on the device: a full MassSolver log, a full CheckLog that must not be
overrun, and what _PicardGraph logs and how it judges a degenerate slot.  The ne = 2 cubed sphere at p = 3 (24 elements): the smallest
mesh on which shared edges, two kinds of solves and more than one level all occur."""
import numpy as np
import pytest

from mimsem_amd.workloads import SCALE, z_levels

pytestmark = pytest.mark.gpu
PN, NE = 3, 2


def _sphere(nk, **geom_kw):
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    cs = CubedSphere(PN, NE, 6); coords = sphere_coords(PN, NE)
    topos = [Topo(cs, p, nk) for p in range(6)]
    return cs, coords, topos, [Geom(t, cs, coords, nk, **geom_kw) for t in topos]


@pytest.fixture(scope="module")
def levels3():
    """an engine with three levels (the eul flavour: MassSolver)"""
    from mimsem_amd.device import DeviceMesh, Engine
    cs, coords, topos, geoms = _sphere(3)
    levs = z_levels(3, geoms[0].n0)
    for g in geoms:
        g.set_levels(levs)
    return Engine(DeviceMesh(topos, geoms, nk=3, numbering="global"))


@pytest.fixture(scope="module")
def sw_step():
    """the shallow-water host after ONE step (q_exact=False, nits=2) from a perturbed Williamson-2 state"""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.sweqn import SWEqn
    cs, coords, topos, geoms = _sphere(1, signed_det=True)
    for g in geoms:
        g.set_levels(np.stack([np.zeros(g.n0), np.ones(g.n0)]))       # unit thickness: the src/ flavour has no vertical
    dm = DeviceMesh(topos, geoms, nk=1, numbering="global")
    eng = Engine(dm)
    xq = np.zeros((dm.nq, 3))
    for g in geoms:
        xq[g.loc0] = coords[g.loc0]
    xq = xq[dm.gidq]
    S = SWEqn(eng, xq)
    th = np.arcsin(xq[:, 2] / 6371220.0); lam = np.arctan2(xq[:, 1], xq[:, 0])
    U0, H0 = 38.61068276698372, 2998.1154702758267
    uq = np.stack([U0 * np.cos(th) + 3.0 * np.sin(2 * lam) * np.cos(th), 2.0 * np.cos(lam) * np.cos(th) ** 2], axis=1)
    hq = H0 - (6371220.0 * 7.292e-5 * U0 + 0.5 * U0 * U0) * np.sin(th) ** 2 / 9.80616 + 40.0 * np.cos(th) * np.sin(lam)
    u0, h0 = S.init1(eng.tensor(uq)), S.init2(eng.tensor(hq))
    u1, h1 = S.solve(u0, h0, 360.0, nits=2, q_exact=False)
    return eng, S, (u1, h1)


def test_mass_solver_log_overflow(levels3):
    """18 fixed-length solves without verify(): the log has 16 slots, the 17th and 18th solve overwrite the last one -- they are counted"""
    from mimsem_amd.krylov import MassSolver
    eng = levels3
    ms = MassSolver(eng, SCALE, True)
    b = eng.tensor(np.random.default_rng(11).standard_normal((eng.nk, eng.sizes[1])) * 1e9)
    ms.solve(b)                                                            # (the one-time calibration of the step count logs twice)
    assert ms.chebyshev and ms.verify() and ms.solves_unchecked == 0
    checked, missed = ms.solves_checked, ms.solves_missed
    for _ in range(18):
        ms.solve(b)
    assert ms.chebyshev and ms.check_log.capacity == 16 and ms.check_log.size == 16 and ms.check_log.shared == 2
    assert ms.verify() is True
    assert ms.solves_checked - checked == 16 and ms.solves_unchecked == 2 and ms.solves_missed == missed
    worst = ms.worst_check
    assert ms.verify() is True                                             # nothing logged: nothing read, nothing counted
    assert ms.solves_checked - checked == 16 and ms.solves_unchecked == 2 and ms.solves_missed == missed and ms.worst_check == worst
    assert ms.check_log.size == 0 and ms.check_log.shared == 0 and not bool(ms.check_log.dev.any())


def test_check_log_capacity_is_an_error_not_an_overrun(levels3):
    import torch
    from mimsem_amd._lib import MimsemError
    from mimsem_amd.checks import CheckLog
    eng = levels3
    log = CheckLog(eng, 2)
    sentinel = torch.full((512,), 7.0, dtype=torch.float64, device=eng.device)      # allocated after the log
    v = eng.tensor(np.arange(1.0, 9.0).reshape(2, 4))
    log.pair(v, "M1")
    log.two(v[0], v[1], "q")
    assert (log.size, log.capacity, log.kind(0), log.kind(1)) == (2, 2, "M1", "q")
    assert not torch.cuda.is_current_stream_capturing()
    with pytest.raises(MimsemError):
        log.claim("A")
    with pytest.raises(MimsemError):
        log.pair(v, "A")                                                   # (refused before the launch)
    torch.cuda.synchronize()
    assert log.dev.shape == (2, 2) and log.size == 2 and log.kind(1) == "q"
    host, = CheckLog.read(log)
    assert host.tolist() == [[30.0, 174.0], [30.0, 174.0]]
    assert bool((sentinel == 7.0).all())
    log.rewind()
    assert log.size == 0 and log.claim("A").data_ptr() == log.dev.data_ptr()      # rewound: the same slots again


def test_picard_graph_logs_the_same_kinds_in_both_bodies(sw_step):
    eng, S, _ = sw_step
    assert S.fixed_iterations == 2 and S.adaptive_iterations == 0 and S.recalibrations == 0
    pg = S._pg
    assert sorted(pg.graphs) == [False, True]                              # the first iteration of a step and the later ones
    for first in (True, False):
        g, kinds, nslots = pg.graphs[first]
        assert g is not None and nslots == 4 and list(kinds)[:nslots] == ["M1", "q", "A", "picard"], (first, kinds, nslots)
    assert pg.log.capacity == pg.NSLOT and pg.log.size == 4
    assert len(S.history) == 2 and all(0.0 < n < 1.0 for n in S.history)


@pytest.mark.parametrize("slot", [0, 1, 2], ids=["M1", "q", "A"])
def test_picard_graph_rejects_a_residual_against_a_zero_reference(sw_step, slot):
    """a hand-made host vector: no device work"""
    eng, S, _ = sw_step
    pg = S._pg
    kinds = pg.graphs[True][1]
    vals = np.zeros((pg.NSLOT, 2))
    vals[3] = (1e-24, 1.0)                                                 # picard: |dx| / |x| = 1e-12
    pg.last_miss = None
    assert pg.verify(vals, first=True) == (True, 1e-12) and pg.last_miss is None      # (0, 0) slots: accepted
    vals[slot] = (1e-3, 0.0)
    ok, norm = pg.verify(vals.reshape(-1).tolist(), first=True)
    assert ok is False and norm == 1e-12
    assert pg.last_miss[0] == kinds[slot] == ("M1", "q", "A")[slot]
    for bad in ((1e-40, -1.0), (1e-40, float("nan")), (float("nan"), 1.0)):
        vals[slot] = bad
        pg.last_miss = None
        assert pg.verify(vals, first=True)[0] is False and pg.last_miss[0] == kinds[slot], bad
