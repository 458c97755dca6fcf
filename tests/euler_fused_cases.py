"""tests/euler_fused_cases.py -- the meshes, inputs and oracle references of tests/test_gpu_euler_fused_orders.py: the fused element kernels of the
3-D Euler step (k_horiz_bernoulli, k_horiz_flux_rhs, k_energetics_horiz, k_energetics_column) at every order they are built for.
TEST INFRASTRUCTURE ONLY; no GPU is touched here (tests/test_euler_fused_cases_cpu.py checks all of it on the CPU).

The unit counts are chosen against the kernels' mapping, not against a workload: a work item is one (level, element), a block of 256 threads
holds EPB = 64, 16, 16, 8, 4, 4, 4 of them at orders 1 .. 7 (4, 16, 16, 32, 64, 64, 64 lanes each), and every case has full blocks AND a
partial last one.  Every case has nk = 3: level 1 has both interfaces, levels 0 and 2 one each (the Bernoulli interface average).

    kind    mesh                                        orders    units   blocks          what it reaches
    box     PeriodicBox(pn, 5, 1), global numbering        1        75    64 + 11         the 4-lane layout; edges that wrap around
    box     PeriodicBox(pn, 3, 1), global numbering      2, 3       27    16 + 11         the 16-lane layout at both of its orders
    box     same                                           4        27    3 x 8 + 3       the 32-lane layout
    box     same                                        5, 6, 7     27    6 x 4 + 3       the 64-lane layout, 36 / 49 / 64 live lanes
    patch   CubedSphere(pn, 3, 6), one patch, local      2 .. 7     27    as the boxes    a FULL Jacobian: J01, J10 at least 0.1 of J00, J11

The box metric is diagonal, so a swapped J01 / J10 or a wrong Gab cannot show on it; the sphere patch is there for those.  On patches 0 and 5
of the cube J01 stays at 0.02 of the diagonal entries (tests/test_euler_fused_cases_cpu.py prints the figures); on patches 1 .. 4 both J01
and J10 pass the 0.1 condition, which build_case asserts, and those four take the orders in turn (six orders, four patches: orders 6 and 7
reuse patches 1 and 2).  Order 1 has no sphere coordinates (mesh.sphere_coords raises) and stays box-only.  The column kernel (16, 4, 4, 2
columns per 64-thread block at orders 1 .. 4) sees 25 = 16 + 9 columns on the order-1 box and 9 on the others: a partial last block at
every order.

A patch case lives in the patch's LOCAL vector layout (DeviceMesh(numbering="local")): edges shared by two elements of the patch receive two
contributions of the flux right-hand side, edges on the patch boundary one, in the reference scatter as on the device.

References, oracle only (c["ref"], made once by references() and never changed):
    phi_mat   diagnose_Phi from the oracle's WTQUMAT / WHMAT element matrices per level (phi_from_element_matrices)
    phi_pt    the same from Patch.interp, J, det, thickInv and W: the point-wise form in the header of csrc/bernoulli.inc (phi_pointwise)
    flux      strang2_case.flux_rhs_pointwise scattered with the patch's edge map (flux_rhs_scattered)
    horiz     energetics_case.restate_horizontal; plain: energetics_case.plain_quadrature; theta: energetics_case.theta_L2 (an INPUT of the kernel)
    column    energetics_case.restate_column, on the boxes of orders 1 .. 4 (the orders the column kernel is built for)
"""
import numpy as np

from tests import energetics_case as ec
from tests import strang2_case as s2c
from tests.helpers import make_patch, rel_l2

TOL = 1e-10                  # the bar of tests/test_gpu_bernoulli.py and tests/test_gpu_flux_rhs.py: relative L2 against the oracle
SCALE = ec.SCALE
NK = 3
ORDERS = (1, 2, 3, 4, 5, 6, 7)
BOX_NE = {1: 5, 2: 3, 3: 3, 4: 3, 5: 3, 6: 3, 7: 3}
PATCH_NE = 3
PATCH_PI = {2: 1, 3: 2, 4: 3, 5: 4, 6: 1, 7: 2}
COLUMN_ORDERS = (1, 2, 3, 4)             # mimsem_euler_energetics_column
JACOBIAN_MIN = 0.1

CASES = [("box", pn) for pn in ORDERS] + [("patch", pn) for pn in ORDERS if pn in PATCH_PI]
case_id = lambda key: "%s_p%d" % key


class LocalView:
    """a Topo seen through its LOCAL maps: the *_g maps of the helpers in tests/energetics_case.py and tests/strang2_case.py answer with the patch-local
    slots, so those helpers work unchanged on vectors in the local layout (patch 0 of a one-patch world)"""

    def __init__(self, topo):
        self._t, self.pi, self.n2 = topo, 0, topo.n2

    def all_inds1x_g(self): return self._t.all_inds1x_l()
    def all_inds1y_g(self): return self._t.all_inds1y_l()
    def all_inds2_g(self): return self._t.all_inds2_l()

    def __getattr__(self, name):
        return getattr(self._t, name)


def jacobian_ratio(P):
    """the smaller of max |J01| and max |J10| over the largest |diagonal| entry of the patch's Jacobian (J = [J00, J01, J10, J11] per
    quadrature point): at least JACOBIAN_MIN means BOTH off-diagonal entries count, which implies that the largest one does"""
    J = np.abs(np.array(P.J))
    return float(min(J[..., 1].max(), J[..., 2].max()) / max(J[..., 0].max(), J[..., 3].max()))


def build_case(oracle, kind, pn):
    """one case of the table above: the dict of tests/energetics_case.py (topos, geoms, patches, velx, rho, rt, exner, velz_v, rho_v, zv_v, ...) plus
    bern = (u1, u2, velz1, velz2) and flux = (u1, u2, h1, h2) -- the second of each pair a perturbation of the first, every level its own draw"""
    if kind == "box":
        c = ec.make_box_case(oracle, pn=pn, ne=BOX_NE[pn], nk=NK, seed=100 + pn)
        c["numbering"] = "global"
    else:
        pi = PATCH_PI[pn]
        cs, topo, geom, P, _ = make_patch(oracle, pn, ne=PATCH_NE, nprocs=6, pi=pi, nk=NK, seed=200 + 10 * pn + pi)
        r = np.random.default_rng(300 + pn)
        F = ec.state_fields(P, r, pn, NK, topo.n1, topo.n2)
        c = dict(topos=[topo], geoms=[geom], levs=geom.levs, gd=None, patches=[(LocalView(topo), geom, P)], F=F)
        c = ec._finish(c, NK, F)
        c["numbering"] = "local"
    (t, g, P), = c["patches"]
    c["kind"], c["pn"], c["id"] = kind, pn, case_id((kind, pn))
    c["nEl"], c["units"] = P.nEl, P.nEl * NK
    c["label"] = "%s p=%d (%d units)" % (kind, pn, c["units"])
    c["jacobian_ratio"] = jacobian_ratio(P)
    if kind == "patch":
        assert c["jacobian_ratio"] >= JACOBIAN_MIN, "%s: off-diagonal Jacobian entries only %.3f of the diagonal ones" % (c["label"], c["jacobian_ratio"])
    r = np.random.default_rng(400 + pn + (50 if kind == "patch" else 0))
    F = c["F"]
    u1, z1, h1 = F["u1"], F["velz1"], F["h1"]
    u2 = u1 * (1 + 0.05 * r.standard_normal(u1.shape))
    z2 = z1 * (1 + 0.05 * r.standard_normal(z1.shape))
    h2 = h1 * (1 + 0.01 * r.standard_normal(h1.shape))
    c["bern"], c["flux"] = (u1, u2, z1, z2), (u1, u2, h1, h2)
    c["np"] = c["bern"]
    for a, b in ((z1, z2), (h1, h2)):                   # a wrong level index must show: no two levels share a row
        for x in (a, b):
            assert all(not np.array_equal(x[i], x[j]) for i in range(x.shape[0]) for j in range(i))
    return c


_CASES = {}


def case(oracle, key):
    """the case of key = (kind, order) with its references: built once, never changed"""
    if key not in _CASES:
        c = build_case(oracle, *key)
        c["ref"] = references(c)
        _CASES[key] = c
    return _CASES[key]


# ---- references -----------------------------------------------------------------------------------------------------------------------------
def _level_average(z, k, nk):
    """1/2 z[k-1] (k > 0) + 1/2 z[k] (k < nk-1): the boundary levels have one interface (eul/HorizSolve.cpp:451-459)"""
    a = np.zeros(z.shape[1])
    if k > 0: a += 0.5 * z[k - 1]
    if k < nk - 1: a += 0.5 * z[k]
    return a


def phi_from_element_matrices(c, nk, fields=None):
    """diagnose_Phi per level from the oracle's WtQUmat / Whmat element matrices of one patch (a case without dense global matrices)"""
    (t, g, P), = c["patches"]
    u1, u2, z1, z2 = c["np"] if fields is None else fields
    gx, gy, g2 = t.all_inds1x_g(), t.all_inds1y_g(), t.all_inds2_g()
    own = ec._own(t)
    out = np.zeros((nk, z1.shape[1]))
    for k in range(nk):
        zb = [_level_average(z, k, nk) for z in (z1, z2)]
        K = [P.op_elmats("WTQUMAT", k, SCALE, 0, ec._patch_local_1form(t, P, u[k])).reshape(P.nEl, 2, P.n2e, P.n1e) for u in (u1, u2)]
        W = [P.op_elmats("WHMAT", k, SCALE, 0, np.ascontiguousarray(a[own])).reshape(P.nEl, P.n2e, P.n2e) for a in zb]
        for e in range(P.nEl):
            ap = lambda Ke, u: Ke[0] @ u[k, gx[e]] + Ke[1] @ u[k, gy[e]]
            out[k, g2[e]] = (ap(K[0][e], u1) + ap(K[0][e], u2) + ap(K[1][e], u2)) / 3.0 \
                + (W[0][e] @ zb[0][g2[e]] + W[0][e] @ zb[1][g2[e]] + W[1][e] @ zb[1][g2[e]]) / 6.0
    return out


def phi_pointwise(c, nk, fields=None):
    """diagnose_Phi per level from the point-wise form csrc/bernoulli.inc is written from: with t = thickInv, d = det, J the Jacobian, Q the
    weight, U_a = J (u_a, v_a)^T / d the Piola-mapped interpolant of velx_a (interp1_l) and r_a the interpolant of the level average of velz_a
    over d (interp2_g),   c_q = SCALE Q [t^2/6 (U1.U1 + U1.U2 + U2.U2) + t/6 (r1^2 + r1 r2 + r2^2)],   Phi[e, j] = sum_q W[q][j] c_q"""
    (t, g, P), = c["patches"]
    u1, u2, z1, z2 = c["np"] if fields is None else fields
    W, Q, iq, g2 = P.arr("W", (P.mp12, P.n2e)), P.arr("Q", (P.mp12,)), P.elinds("q"), t.all_inds2_g()
    own = ec._own(t)
    out = np.zeros((nk, z1.shape[1]))
    for k in range(nk):
        ul = [ec._patch_local_1form(t, P, u[k]) for u in (u1, u2)]
        zl = [np.ascontiguousarray(_level_average(z, k, nk)[own]) for z in (z1, z2)]
        for e in range(P.nEl):
            ex, ey = e % P.nElsX, e // P.nElsX
            cq = np.zeros(P.mp12)
            for q in range(P.mp12):
                px, py = q % P.mp1, q // P.mp1
                J = np.array(P.J[e, q]).reshape(2, 2); d = P.det[e, q]; ti = P.thickInv[k, iq[e, q]]
                U1, U2 = (J @ np.array(P.interp("1l", ex, ey, px, py, u)) / d for u in ul)
                r1, r2 = (P.interp("2g", ex, ey, px, py, z)[0] for z in zl)
                cq[q] = SCALE * Q[q] * (ti * ti / 6.0 * (U1 @ U1 + U1 @ U2 + U2 @ U2) + ti / 6.0 * (r1 * r1 + r1 * r2 + r2 * r2))
            out[k, g2[e]] = W.T @ cq
    return out


def edge_slot_map(t, P):
    """patch-local 1-form slot -> slot of the case's vectors (the global id on a box, the slot itself in the local layout)"""
    gmap = np.full(P.n1, -1, dtype=np.int64)
    gmap[t.all_inds1x_l().ravel()] = t.all_inds1x_g().ravel()
    gmap[t.all_inds1y_l().ravel()] = t.all_inds1y_g().ravel()
    assert (gmap >= 0).all()
    return gmap


def edge_contributions(c):
    """how many elements contribute to each 1-form slot of the case's vectors"""
    (t, g, P), = c["patches"]
    n = np.zeros(c["velx"].shape[1], dtype=np.int64)
    np.add.at(n, np.concatenate([t.all_inds1x_g().ravel(), t.all_inds1y_g().ravel()]), 1)
    return n


def flux_rhs_scattered(c, nk, fields):
    """strang2_case.flux_rhs_pointwise per level, its patch-local vector (one contribution per element and edge, added up) scattered
    with ADD into the case's slots: an edge that wraps around a periodic box collects both of its elements"""
    (t, g, P), = c["patches"]
    u1, u2, h1, h2 = fields
    gmap, own = edge_slot_map(t, P), ec._own(t)
    ref = np.zeros_like(u1)
    for k in range(nk):
        loc = s2c.flux_rhs_pointwise(P, k, ec._patch_local_1form(t, P, u1[k]), ec._patch_local_1form(t, P, u2[k]),
                                     np.ascontiguousarray(h1[k][own]), np.ascontiguousarray(h2[k][own]))
        np.add.at(ref[k], gmap, loc)
    return ref


def references(c):
    nk = c["nk"]
    ref = dict(phi_mat=phi_from_element_matrices(c, nk, c["bern"]), phi_pt=phi_pointwise(c, nk, c["bern"]),
               flux=flux_rhs_scattered(c, nk, c["flux"]), theta=ec.theta_L2(c), horiz=ec.restate_horizontal(c), plain=ec.plain_quadrature(c))
    if c["kind"] == "box" and c["pn"] in COLUMN_ORDERS:
        ref["column"] = ec.restate_column(c)
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            assert np.isfinite(v).all(), (c["label"], k)
            v.setflags(write=False)
    return ref


# ---- the comparison -------------------------------------------------------------------------------------------------------------------------
def level_errors(got, want):
    """relative L2 error of every level (row) on its own"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return [float(rel_l2(got[k], want[k])) for k in range(want.shape[0])]


def element_errors(got, want, index):
    """[levels, elements]: relative L2 error of every (level, element) on that element's own norm; index [nEl, dofs] maps an element to its slots"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.array([[rel_l2(got[k, index[e]], want[k, index[e]]) for e in range(index.shape[0])] for k in range(want.shape[0])])


def assert_elements(label, got, want, index, tol=TOL):
    """every (level, element) below tol on its own norm: a wrong element cannot hide in a level norm.  Returns the worst error; the failure
    names the (level, element) pairs"""
    err = element_errors(got, want, index)
    bad = [(int(k), int(e)) for k, e in zip(*np.nonzero(~(err < tol)))]             # (a NaN fails)
    assert not bad, "%s: %d (level, element) above %.1e: %s (worst %.3e)" % (
        label, len(bad), tol, ", ".join("(%d, %d) %.3e" % (k, e, err[k, e]) for k, e in bad[:12]) + (" ..." if len(bad) > 12 else ""),
        float(np.nanmax(err)))
    return float(err.max())
