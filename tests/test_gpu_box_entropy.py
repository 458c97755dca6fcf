"""mimsem_euler_log_entropy (csrc/log_entropy.inc): the entropy of the box twin's energetics line (box/Euler_2.cpp:979-997)
    out = factor sum_rows lz[row] sum_e sum_q Q_q log((W theta_row)_q)
through Engine.log_entropy, against the numpy sum written from the oracle's W / Q tables (the sum BoxRestatement.diagnostics makes,
tests/box_strang_case.py entropy) and against the composed route (Engine.interp_quad, torch.log, a weighted torch sum).

Bar: |difference| <= PARITY S_abs with S_abs = |factor| sum lz Q |log| and PARITY = 1e-10, the project's bar for such sums
(tests/test_gpu_energetics.py).  What to expect: log(theta) ~ 5.7 has one sign, so S_abs = |sum| and the bar is a relative 1e-10; every term
carries a few ulp (the interpolation's n^2 products, the logarithm, two weights) and N terms summed in trees add O(sqrt(N)) ulp at worst --
1e-14 to 1e-13 of S_abs at these sizes, three orders inside the bar.  The observed value of every comparison is printed.

theta is drawn around 300: DoF j of an element is T_j dx_jx dy_jy with T_j uniform in [290, 310] and dx the GLL node spacings -- the 2-form
DoFs of a field near 300 (the interpolant of equal T_j is T exactly), positive at every point; each reference checks that it is."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import box_strang_case as bc
from tests import strang_case as sc

pytestmark = pytest.mark.gpu
PARITY = 1e-10
CP = bc.ec.CP
ERR_ARG = -1


# ---- inputs and the two references ---------------------------------------------------------------------------------------------------
def draw_theta(pn, nrows, nel, seed):
    from mimsem_amd.geom import gll_points
    d = np.diff(gll_points(pn))
    T = np.random.default_rng(seed).uniform(290.0, 310.0, (nrows, nel, pn * pn))
    return (T * np.outer(d, d).ravel()).reshape(nrows, nel * pn * pn)


def draw_lz(nrows, seed):
    """every row its own weight (a wrong row index must show), the two ends halved as :988 has them"""
    lz = np.random.default_rng(seed).uniform(200.0, 400.0, nrows)
    lz[0] *= 0.5; lz[-1] *= 0.5
    return lz


def numpy_sum(oracle, pn, theta, lz, factor):
    """(sum, S_abs) from the oracle's tables; 2-form slots are element-contiguous (Topo.all_inds2_g): [nrows, nEl, n2e]"""
    tab = oracle.tables(pn, pn)
    W, Q = tab["W"], tab["Q"]
    tq = theta.reshape(theta.shape[0], -1, pn * pn) @ W.T                               # [nrows, nEl, mp12]
    assert tq.min() > 0.0
    terms = factor * lz[:, None, None] * (Q[None, None, :] * np.log(tq))
    return float(terms.sum()), float(np.abs(terms).sum())


def composed(eng, theta, lz, factor):
    """(sum, S_abs) as BoxEuler.entropy composes it: interp_quad, torch.log, a weighted sum"""
    from mimsem_amd.geom import gll_weights
    w = torch.as_tensor(gll_weights(eng.mesh.m), dtype=torch.float64, device=eng.device)
    Q = (w[:, None] * w[None, :]).reshape(-1)
    tq = eng.interp_quad(2, theta, push_forward=False)
    tq = tq if tq.dim() == 3 else tq[None]
    assert float(tq.min()) > 0.0
    terms = factor * (lz[:, None, None] * Q[None, None, :] * torch.log(tq))
    return float(terms.sum()), float(terms.abs().sum())


def check(label, got, want):
    val, s_abs = want
    err = abs(got - val) / s_abs
    print("%-58s kernel % .16e  reference % .16e  |difference| / S_abs = %.2e" % (label, got, val, err))
    assert np.isfinite(got) and s_abs > 0.0 and err <= PARITY, (label, got, val, err)
    return err


# ---- engines ---------------------------------------------------------------------------------------------------------------------------
def box_engine(pn, ne, nk, lx=1000.0, seed=5):
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import BoxGeom
    from mimsem_amd.mesh import PeriodicBox, box_coords
    from mimsem_amd.topo import Topo
    from tests.helpers import z_levels
    bx = PeriodicBox(pn, ne, 1)
    t = Topo(bx, 0, nk)
    g = BoxGeom(t, bx, box_coords(pn, ne, lx), nk, lx)
    g.set_levels(z_levels(nk, g.n0, np.random.default_rng(seed), ztop=1500.0))
    return Engine(DeviceMesh([t], [g], nk=nk, numbering="global"))


def run(eng, theta, lz, factor=CP):
    th, l = eng.tensor(theta), eng.tensor(lz)
    return float(eng.log_entropy(th, l, factor)[0]), th, l


@pytest.fixture(scope="module")
def box3(oracle):
    """tests/box_strang_case.py make_case: p = 3, 3 x 3 box, nk = 4 -- 5 rows x 9 elements = 45 units of 16 lanes, 16 to a block: two full
    blocks and a last one with 13 live units and 3 idle ones"""
    from mimsem_amd.device import DeviceMesh, Engine
    c = bc.make_case(oracle)
    c["eng"] = Engine(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering="global"))
    return c


def test_box_step_shape_against_the_restatement_and_both_switch_positions(box3, oracle):
    """the shape and the call of the box step: theta on the nk + 1 = 5 interfaces of a context with nk = 4, lz half a layer at both ends,
    factor CP.  BoxEuler.entropy gives the kernel's value with FUSED_ENTROPY on and the composed one with it off"""
    from mimsem_amd.euler import BoxEuler
    c, eng = box3, box3["eng"]
    nk, P = c["nk"], c["P"]
    assert eng.nEl * (nk + 1) == 45 and eng.mesh.n == 3
    theta = draw_theta(3, nk + 1, eng.nEl, 11)
    lz = np.full(nk + 1, bc.DZ); lz[0] *= 0.5; lz[-1] *= 0.5
    got, th, l = run(eng, theta, lz)
    check("p=3 3x3 nk=4 (45 units), numpy sum", got, numpy_sum(oracle, 3, theta, lz, CP))
    theta_v = np.ascontiguousarray(theta.reshape(nk + 1, eng.nEl, P.n2e).transpose(1, 0, 2)).reshape(eng.nEl, -1)
    check("p=3 3x3 nk=4, BoxRestatement's entropy()", got, bc.entropy(c, theta_v))
    check("p=3 3x3 nk=4, composed route", got, composed(eng, th, l, CP))
    dm = eng.mesh
    g, = c["geoms"]
    levs = np.zeros((nk + 1, dm.nq))
    levs[:, np.searchsorted(dm.gidq, g.loc0[np.arange(g.n0)])] = g.levs
    eu = BoxEuler(eng, bc.DT, levs, c["coords"][dm.gidq], lx=c["lx"], newton_maxit=bc.NITS, newton_tol=0.0, do_visc=False)
    assert np.allclose(eu._lz.cpu().numpy(), lz, rtol=1e-14, atol=0.0)
    eu.FUSED_ENTROPY = True
    fused = eu.entropy(th)
    assert fused.dim() == 0 and float(fused) == got                                    # the kernel's bits
    eu.FUSED_ENTROPY = False
    off = eu.entropy(th)
    assert off.dim() == 0
    check("BoxEuler.entropy, FUSED_ENTROPY on against off", float(fused), (float(off), abs(float(off))))


@pytest.mark.parametrize("pn,ne,nk", [(4, 2, 2), (1, 5, 3), (2, 3, 3)], ids=["p4_25_points_on_32_lanes", "p1_64_elements_a_block", "p2_16_elements_a_wave"])
def test_other_box_orders_against_the_numpy_sum(oracle, pn, ne, nk):
    """p = 4, 2 x 2 box, nk = 2: 25 points on 32 lanes, 12 units in one block of 8.  p = 1 (4 lanes an element, 16 elements a wave; 5 x 5 x 4
    rows = 100 units: a block of 64 and a partial one) and p = 2 (16 lanes, 4 elements a wave; 9 x 4 = 36 units: two full blocks and a
    partial one): several elements share a wave, and the wave's tree sums across them"""
    eng = box_engine(pn, ne, nk)
    theta, lz = draw_theta(pn, nk + 1, eng.nEl, 20 + pn), draw_lz(nk + 1, 30 + pn)
    got, th, l = run(eng, theta, lz)
    check("p=%d %dx%d box, %d rows, numpy sum" % (pn, ne, ne, nk + 1), got, numpy_sum(oracle, pn, theta, lz, CP))
    check("p=%d %dx%d box, %d rows, composed route" % (pn, ne, ne, nk + 1), got, composed(eng, th, l, CP))


@pytest.mark.parametrize("pn", [5, 6, 7])
def test_high_orders_against_the_composed_route(pn):
    """the 64-lane layouts: 36, 49 and 64 live lanes, 4 units to a block; a 2 x 2 box with 3 rows is 12 units, three blocks.  No table of the
    restatement is pinned at these orders: the composed device route is the reference"""
    eng = box_engine(pn, 2, 2)
    theta, lz = draw_theta(pn, 3, eng.nEl, 40 + pn), draw_lz(3, 50 + pn)
    got, th, l = run(eng, theta, lz, -2.5)                                             # (a factor that is not CP, and negative)
    check("p=%d 2x2 box, 3 rows, composed route" % pn, got, composed(eng, th, l, -2.5))


def test_one_row(box3, oracle):
    """nrows = 1 (9 units: one partial block); a [n2] tensor is one row"""
    eng = box3["eng"]
    theta, lz = draw_theta(3, 1, eng.nEl, 61), np.array([123.0])
    got, th, l = run(eng, theta, lz)
    check("nrows = 1, numpy sum", got, numpy_sum(oracle, 3, theta, lz, CP))
    assert float(eng.log_entropy(th[0], l, CP)[0]) == got


def test_sphere(oracle):
    """the mesh of tests/strang_case.py make_case: the p = 3, ne = 2 cubed sphere (24 elements in six patches), nk = 4 and 5 rows: 120 units,
    7 full blocks and a half one.  The quantity has no metric: the same tables as on the box"""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from tests.helpers import z_levels
    cs = CubedSphere(sc.PN, sc.NE, 6); coords = sphere_coords(sc.PN, sc.NE)
    topos = [Topo(cs, p, sc.NK) for p in range(6)]
    geoms = [Geom(t, cs, coords, sc.NK) for t in topos]
    for g in geoms:
        g.set_levels(z_levels(sc.NK, geoms[0].n0))
    eng = Engine(DeviceMesh(topos, geoms, nk=sc.NK, numbering="global"))
    assert eng.nEl == 24 and eng.sizes[2] == 24 * 9
    theta, lz = draw_theta(3, sc.NK + 1, eng.nEl, 71), draw_lz(sc.NK + 1, 72)
    got, th, l = run(eng, theta, lz)
    check("p=3 ne=2 sphere, 5 rows, numpy sum", got, numpy_sum(oracle, 3, theta, lz, CP))
    check("p=3 ne=2 sphere, 5 rows, composed route", got, composed(eng, th, l, CP))


def test_every_reduction_loop_runs_more_than_once(oracle):
    """The reduction has two loops.  (1) The block's fixed-stride walk over its units: the grid is capped at 2048 blocks, so a block takes a
    second unit only past 2048 EPB units -- at p = 3 (EPB = 16) past 32 768.  (2) The final pass, where lane l sums partials l, l + 64, ..:
    more than one trip needs more than 64 blocks.  nrows is not bound by the context's nk, so a small mesh reaches both: a p = 3, 2 x 2 box
    (4 elements) with 16 421 rows is 65 684 units = 2 x 32 768 + 148 -- every block walks twice, blocks 0 .. 9 a third time, block 9 with 4
    live units of 16 on that trip, blocks 10 .. 2047 not at all (an uneven trip count between blocks); the final pass makes 32 trips per
    lane.  theta is 4.7 MB.  Bar as everywhere; N = 1.05e6 terms"""
    eng = box_engine(3, 2, 2)
    nrows = 16421
    assert eng.nEl * nrows == 2 * 2048 * 16 + 148
    theta, lz = draw_theta(3, nrows, eng.nEl, 81), draw_lz(nrows, 82)
    got, th, l = run(eng, theta, lz)
    check("p=3 2x2 box, 16421 rows (65684 units), numpy sum", got, numpy_sum(oracle, 3, theta, lz, CP))
    check("p=3 2x2 box, 16421 rows (65684 units), composed route", got, composed(eng, th, l, CP))


@pytest.mark.parametrize("pad", [1, 6], ids=["odd_pitch", "even_pitch"])
def test_strided_rows(box3, pad):
    """theta as a slice of a wider array whose other words are NaN (a word read from there poisons the sum), at an odd and an even pitch;
    and one row for every level (pitch 0, as expand() makes)"""
    eng = box3["eng"]
    n2, nrows = eng.sizes[2], 5
    theta, lz = draw_theta(3, nrows, eng.nEl, 91), draw_lz(nrows, 92)
    want, th, l = run(eng, theta, lz)
    wide = torch.full((nrows, pad + n2 + pad), float("nan"), dtype=torch.float64, device=eng.device)
    view = wide[:, pad:pad + n2]
    view.copy_(th)
    assert view.stride(0) == n2 + 2 * pad and not view.is_contiguous()
    assert float(eng.log_entropy(view, l, CP)[0]) == want                              # the bits of the packed call
    same = th[2:3].expand(nrows, n2)
    assert same.stride(0) == 0
    assert float(eng.log_entropy(same, l, CP)[0]) == float(eng.log_entropy(th[2:3].repeat(nrows, 1), l, CP)[0])


def test_same_bits_repeated_and_replayed(box3):
    eng = box3["eng"]
    theta, lz = draw_theta(3, 5, eng.nEl, 95), draw_lz(5, 96)
    a, th, l = run(eng, theta, lz)
    assert float(eng.log_entropy(th, l, CP)[0]) == a                                   # two calls
    g, out = eng.capture(lambda: eng.log_entropy(th, l, CP))                           # (the calls above have sized the workspace)
    out.fill_(float("nan"))
    g.replay(); torch.cuda.synchronize()
    assert float(out[0]) == a


def test_argument_errors_write_nothing(box3):
    from mimsem_amd._lib import MimsemError
    eng = box3["eng"]
    nrows, n2 = 5, eng.sizes[2]
    theta, lz = draw_theta(3, nrows, eng.nEl, 97), draw_lz(nrows, 98)
    want, th, l = run(eng, theta, lz)
    out = torch.full((1,), 7.0, dtype=torch.float64, device=eng.device)
    fn = eng.L.mimsem_euler_log_entropy
    p = dict(theta=th, lz=l, out=out)

    def call(ctx=eng.ctx, n=nrows, pitch=n2, **null):
        x = {k: (None if k in null else C.c_void_p(t.data_ptr())) for k, t in p.items()}
        return fn(ctx, n, x["theta"], pitch, x["lz"], CP, x["out"])
    assert call(ctx=None) == ERR_ARG
    for k in p:
        assert call(**{k: True}) == ERR_ARG, k
    for bad in (0, -1):
        assert call(n=bad) == ERR_ARG, bad
    assert call(pitch=-1) == ERR_ARG
    for bad in (1, n2 - 1):                                                            # rows that overlap
        assert call(pitch=bad) == ERR_ARG, bad
    torch.cuda.synchronize()
    assert float(out[0]) == 7.0                                                        # the poisoned output stays poisoned
    assert call() == 0
    torch.cuda.synchronize()
    assert float(out[0]) == want
    poisoned = torch.full((1,), 7.0, dtype=torch.float64, device=eng.device)
    le = eng.log_entropy
    for bad in (lambda: le(None, l, CP, out=poisoned), lambda: le(th, None, CP, out=poisoned),
                lambda: le(th[:, :-1], l, CP, out=poisoned),                           # rows too short
                lambda: le(th, l[:-1], CP, out=poisoned),                              # lz shorter than the rows
                lambda: le(th[:0], l[:0], CP, out=poisoned),                           # no row
                lambda: le(th.float(), l, CP, out=poisoned),                           # dtype
                lambda: le(torch.cat([th, th], 1)[:, ::2], l, CP, out=poisoned),           # inner stride 2
                lambda: le(th, l, CP, out=torch.full((2,), 7.0, dtype=torch.float64, device=eng.device))):   # out is one double
        with pytest.raises(MimsemError):
            bad()
    torch.cuda.synchronize()
    assert float(poisoned[0]) == 7.0
