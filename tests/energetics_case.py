"""The cases and the restatement of Euler::diagnostics (eul/Euler_2.cpp:600-744) shared by tests/test_energetics_cpu.py and
tests/test_gpu_energetics.py.

make_case():      the p = 3, ne = 2, nk = 3 cubed sphere of tests/vort_diag_case.py (24 x 3 = 72 units: the last block of the kernel is partial)
                  with rt, exner, the weak-form geopotential zv of VertSolve::initGZ (eul/VertSolve.cpp:89-175) and velz in the vertical layout
make_box_case():  a p = 4, ne = 3, nk = 2 doubly periodic box (25 quadrature points per element: the 32-lane layout; 18 units in 3 blocks), its
                  oracle patch built from the box metric as tests/test_gpu_next_rows.py::test_periodic_box_p4_global_apply builds it, levels
                  perturbed per quadrature point

restate() evaluates every sum with the oracle only -- the Uhmat / Wmat matrices (the dense global ones of GlobalDense.mat where the case has
them, the element matrices otherwise), Patch.interp("2g") for int2, Patch.colop_dense for CONLIN_W / LINEAR_RT / LINEAR_INV,
Patch.diag_theta_L2 and the +-I incidence for V10 / V01 -- and returns beside each sum S_abs, the sum of the absolute values of its
per-element (per-column) contributions: k2p and p2k are signed and may cancel, so errors are taken relative to S_abs.
plain_quadrature() evaluates keh, ie, entr from the quadrature-point formulas the kernel is written from (csrc/energetics.inc)."""
import numpy as np

from tests import vort_diag_case as vc
from tests.helpers import z_levels

SCALE = 1.0e8
CV, CP = 717.5, 1004.5               # eul/Euler_2.cpp:29-30
GRAVITY = 9.80616
HORIZ = ("keh", "ie", "entr", "mass")
COLUMN = ("kev", "k2p", "p2k", "pe")


def _patch_local_1form(t, P, u):
    ul = np.zeros(P.n1)
    ul[t.all_inds1x_l().ravel()] = u[t.all_inds1x_g().ravel()]
    ul[t.all_inds1y_l().ravel()] = u[t.all_inds1y_g().ravel()]
    return ul


def _own(t):
    return t.pi * t.n2 + np.arange(t.n2)


def init_gz(patches, levs, nk):
    """zv [nEl, nk n2e] of VertSolve::initGZ: zv_k = W^T (SCALE w_q / 2) (g z_k + g z_{k+1}) per element, as tests/test_gpu_column.py states it"""
    out = []
    for t, g, P in patches:
        W, Q = P.arr("W", (P.mp12, P.n2e)), P.arr("Q", (P.mp12,))
        inds0 = g.all_inds0_l()
        zv = np.zeros((P.nEl, nk * P.n2e))
        for e in range(P.nEl):
            for k in range(nk):
                gz = GRAVITY * (levs[k, inds0[e]] + levs[k + 1, inds0[e]])
                zv[e, k * P.n2e:(k + 1) * P.n2e] = W.T @ (SCALE * 0.5 * Q * gz)
        out.append(zv)
    return np.concatenate(out)


def to_vert(patches, a, nk):
    """[nk or nk - 1, N2] horizontal -> [nEl, rows n2e] vertical, patch by patch (L2Vecs::HorizToVert; interface fields ride in the first
    nk - 1 rows of an nk-row array)"""
    out = []
    for t, g, P in patches:
        b = a[:, _own(t)]
        rows = b.shape[0]
        if rows < nk:
            b = np.vstack([b, np.zeros((nk - rows, t.n2))])
        out.append(P.horiz_to_vert(np.ascontiguousarray(b))[:, :rows * P.n2e])
    return np.concatenate(out)


def _finish(c, nk, F):
    patches = c["patches"]
    c["nk"] = nk
    c["velx"], c["rho"], c["rt"], c["exner"] = F["u1"], F["h1"], F["th"], F["Pi"]
    c["velz_v"] = to_vert(patches, F["velz1"], nk)
    c["rho_v"] = to_vert(patches, c["rho"], nk)
    c["zv_v"] = init_gz(patches, c["levs"], nk)
    return c


def make_case():
    c = vc.make_case()
    c["patches"] = list(zip(c["topos"], c["geoms"], c["gd"].P))
    return _finish(c, vc.NK, c["F"])


def make_box_case(oracle, pn=4, ne=3, nk=2, seed=43):
    from mimsem_amd.geom import BoxGeom
    from mimsem_amd.mesh import PeriodicBox, box_coords
    from mimsem_amd.topo import Topo
    bx = PeriodicBox(pn, ne, 1); coords = box_coords(pn, ne, 1000.0)
    t = Topo(bx, 0, nk)
    g = BoxGeom(t, bx, coords, nk, 1000.0)
    r = np.random.default_rng(seed)
    levs = z_levels(nk, g.n0, r, ztop=1500.0)
    g.set_levels(levs)
    P = oracle.Patch(pn, pn, bx.nel, nk)
    P.set_metric(g.det, g.J); P.set_levels(levs)
    F = state_fields(P, r, pn, nk, bx.nDofs1G, bx.nDofs2G)
    c = dict(topos=[t], geoms=[g], levs=levs, gd=None, patches=[(t, g, P)], F=F)
    return _finish(c, nk, F)


def state_fields(P, r, pn, nk, N1, N2):
    """a physically scaled 3-D state on the one patch P, every level its own draw: u1 [nk, N1], h1 (density), th (density-weighted potential
    temperature), Pi (Exner) [nk, N2] and velz1 [nk-1, N2] as DoFs (fluxes and cell integrals: the area and thickness factors)"""
    area = P.det.mean() * 4.0 / (pn * pn); dz = P.thick.mean(); ln = np.sqrt(area)
    return dict(u1=r.standard_normal((nk, N1)) * 20.0 * ln * dz, h1=r.uniform(0.8, 1.2, (nk, N2)) * area * dz,
                th=r.uniform(290, 310, (nk, N2)) * area * dz, Pi=r.uniform(900, 1000, (nk, N2)) * area * dz,
                velz1=r.standard_normal((nk - 1, N2)) * area)


def theta_L2(c, rho=None, rt=None):
    """VertSolve::diagTheta_L2 in the horizontal layout [nk, N2] (HorizToVert, per column, VertToHoriz: eul/Euler_2.cpp:699-704)"""
    rho = c["rho"] if rho is None else rho
    rt = c["rt"] if rt is None else rt
    out = np.zeros_like(rho)
    for t, g, P in c["patches"]:
        own = _own(t)
        rv, tv = P.horiz_to_vert(np.ascontiguousarray(rho[:, own])), P.horiz_to_vert(np.ascontiguousarray(rt[:, own]))
        th = np.stack([P.diag_theta_L2(e % P.nElsX, e // P.nElsX, rv[e], tv[e]) for e in range(P.nEl)])
        out[:, own] = P.vert_to_horiz(th)
    return out


def restate_horizontal(c, levels=None):
    """{name: (sum, S_abs)} of keh, ie, entr, mass over `levels` (default: all) plus the per-level sums under name + "_k" """
    nk, gd = c["nk"], c["gd"]
    levels = range(nk) if levels is None else levels
    velx, rho, rt, exner = c["velx"], c["rho"], c["rt"], c["exner"]
    theta = theta_L2(c)
    S = {n: 0.0 for n in HORIZ}; A = {n: 0.0 for n in HORIZ}
    for k in levels:
        per = {n: [] for n in HORIZ}
        for t, g, P in c["patches"]:
            own = _own(t)
            gx, gy, g2 = t.all_inds1x_g(), t.all_inds1y_g(), t.all_inds2_g()
            rl = np.ascontiguousarray(rho[k, own])
            Fe = P.op_elmats("UHMAT", k, SCALE, 1, rl).reshape(P.nEl, 4, P.n1e, P.n1e)      # F->assemble(rho_k, k, true, SCALE)
            Me = P.op_elmats("WMAT", k, SCALE, 1).reshape(P.nEl, P.n2e, P.n2e)              # M2->assemble(k, SCALE, true)
            Q = P.arr("Q", (P.mp12,))
            for e in range(P.nEl):
                xx, xy = velx[k, gx[e]], velx[k, gy[e]]
                per["keh"].append(0.5 * (xx @ (Fe[e, 0] @ xx + Fe[e, 1] @ xy) + xy @ (Fe[e, 2] @ xx + Fe[e, 3] @ xy)) / SCALE)
                per["ie"].append((CV / CP) * (rt[k, g2[e]] @ (Me[e] @ exner[k, g2[e]])) / SCALE)
                per["entr"].append(0.5 * (theta[k, g2[e]] @ (Me[e] @ rt[k, g2[e]])) / SCALE)
                ex, ey = e % P.nElsX, e // P.nElsX
                per["mass"].append(sum(P.det[e, q] * Q[q] * P.interp("2g", ex, ey, q % P.mp1, q // P.mp1, rl)[0] for q in range(P.mp12)))   # int2
        sums = {n: float(np.sum(per[n])) for n in HORIZ}
        if gd is not None:                       # the matrix route of the reference: assembled global matrices
            Fk, Mk = gd.mat("UHMAT", k, flag=1, field=rho[k]), gd.mat("WMAT", k, flag=1)
            sums["keh"] = 0.5 * float(velx[k] @ (Fk @ velx[k])) / SCALE
            sums["ie"] = (CV / CP) * float(rt[k] @ (Mk @ exner[k])) / SCALE
            sums["entr"] = 0.5 * float((Mk @ rt[k]) @ theta[k]) / SCALE
        for n in HORIZ:
            S[n] += sums[n]; A[n] += float(np.abs(per[n]).sum())
    return {n: (S[n], A[n]) for n in HORIZ}


def incidence_V10(nk, n2):
    V = np.zeros((nk * n2, (nk - 1) * n2))
    for k in range(nk):
        for i in range(n2):
            if k > 0: V[k * n2 + i, (k - 1) * n2 + i] = -1.0
            if k < nk - 1: V[k * n2 + i, k * n2 + i] = +1.0
    return V


def restate_column(c):
    """{name: (sum, S_abs)} of kev, k2p, p2k, pe (eul/Euler_2.cpp:638-664, :675-684), column by column"""
    nk = c["nk"]
    velz, rho, zv = c["velz_v"], c["rho_v"], c["zv_v"]
    per = {n: [] for n in COLUMN}
    e0 = 0
    for t, g, P in c["patches"]:
        V10 = incidence_V10(nk, P.n2e); V01 = -V10.T
        for e in range(P.nEl):
            ex, ey = e % P.nElsX, e // P.nElsX
            w, r, z = velz[e0 + e], rho[e0 + e], zv[e0 + e]
            BA = P.colop_dense("CONLIN_W", ex, ey, f1=w)
            per["kev"].append(0.5 * (r @ (BA @ w)) / SCALE)
            gi = P.colop_dense("LINEAR_INV", ex, ey) @ (P.colop_dense("LINEAR_RT", ex, ey, flag=1, f1=r) @ w)
            per["k2p"].append((gi @ (V01 @ z)) / SCALE)
            per["p2k"].append(((V10 @ gi) @ z) / SCALE)
            per["pe"].append((z @ r) / SCALE)
        e0 += P.nEl
    return {n: (float(np.sum(per[n])), float(np.abs(per[n]).sum())) for n in COLUMN}


def plain_quadrature(c):
    """{name: (sum, S_abs)} of keh, ie, entr from the quadrature-point formulas: with t = thickInv, w = w_qx w_qy, d = det, J = [[a, b], [c, e]],
    (u, v) the LOCAL interpolants of velx and rho_q, Theta_q, Pi_q, theta_q = interp2_g (which holds the 1/d),
      keh  = 1/2 sum rho_q t [(a^2 + c^2) u^2 + 2 (a b + c e) u v + (b^2 + e^2) v^2] w/d t
      ie   = CV/CP sum (Theta_q d) (Pi_q d) w/d t          entr = 1/2 sum (theta_q d) (Theta_q d) w/d t"""
    nk = c["nk"]
    velx, rho, rt, exner = c["velx"], c["rho"], c["rt"], c["exner"]
    theta = theta_L2(c)
    names = ("keh", "ie", "entr")
    S = {n: 0.0 for n in names}; A = {n: 0.0 for n in names}
    for k in range(nk):
        for t, g, P in c["patches"]:
            own = _own(t)
            ul = _patch_local_1form(t, P, velx[k])
            f2 = [np.ascontiguousarray(a[k, own]) for a in (rho, rt, exner, theta)]
            Q, iq, J, det = P.arr("Q", (P.mp12,)), P.elinds("q"), P.J, P.det
            for e in range(P.nEl):
                ex, ey = e % P.nElsX, e // P.nElsX
                v = {n: 0.0 for n in names}
                for q in range(P.mp12):
                    px, py = q % P.mp1, q // P.mp1
                    uq, vq = P.interp("1l", ex, ey, px, py, ul)
                    rq, Tq, Pq, hq = (P.interp("2g", ex, ey, px, py, f)[0] for f in f2)
                    a, b, cc, ee = J[e, q]
                    d, ti, w = det[e, q], P.thickInv[k, iq[e, q]], Q[q]
                    v["keh"] += 0.5 * rq * ti * ((a * a + cc * cc) * uq * uq + 2.0 * (a * b + cc * ee) * uq * vq + (b * b + ee * ee) * vq * vq) * w / d * ti
                    v["ie"] += (CV / CP) * (Tq * d) * (Pq * d) * w / d * ti
                    v["entr"] += 0.5 * (hq * d) * (Tq * d) * w / d * ti
                for n in names:
                    S[n] += v[n]; A[n] += abs(v[n])
    return {n: (S[n], A[n]) for n in names}
