"""tests/box_schur2_case.py -- numpy restatement of the box twin's vertical Newton loop, VertSolve::solve_schur_2 of box/VertSolve.cpp:1264-1458,
and of the two operators it has beyond the eul loop (tests/schur2_case.py):

  upwind_matrices / diag_theta2_up   diagTheta2 (box/VertSolve.cpp:499-531) with AssembleLinCon_up and AssembleLinearWithRho_up
                                     (box/VertOps.cpp:2601-2741): both matrices dense per column from the pyoracle.Patch tables, a dense solve
  vert_mom_vort                      AssembleVertMomVort (box/VertSolve.cpp:1460-1499) on the dense global matrices of the horizontal oracle
  solve_schur_2_box                  the loop, written after schur2_case.solve_schur_2 with flags = 3 and rayleigh = 0

TEST INFRASTRUCTURE ONLY: the checker of Engine.diag_theta_wup, VortDiag.vert_mom_vort and VertSolve.solve_schur_2(theta_up=True, ...); nothing in
the product imports it.  Also the periodic boxes and the start states the tests share."""
import numpy as np

from oracle.horiz_oracle import GlobalDense
from oracle.vert_oracle import _v10
from tests import schur2_case as sc
from tests.energetics_case import to_vert
from tests.helpers import z_levels

SCALE = sc.SCALE
DT = 0.1                    # time step of the loop tests; the theta diagnosis upwinds over DTW
DTW = 0.25 * DT             # box/VertSolve.cpp:521
UPWIND = 0.3                # max_q |DTW w| of the seeded vertical velocities (0.1 <= . <= 0.5: tests/test_box_schur2_cpu.py)


# ---- the two upwinded matrices -------------------------------------------------------------------------------------------------
def shape_functions(P, velz, dtw):
    """N0b, N1b, N0t, N1t [nk, mp12] of one column: phi_0 / phi_1 at -1 + dtw wb and +1 + dtw wt (box/VertOps.cpp:2601-2602, :2630-2639)"""
    nk, n2 = P.nk, P.n2e
    W = P.arr("W", (P.mp12, n2))
    wi = np.zeros((nk + 1, P.mp12))                    # w at the nk + 1 interfaces: 0 at the ground and the lid
    for i in range(nk - 1):
        wi[i + 1] = W @ velz[i * n2:(i + 1) * n2]
    zb, zt = -1.0 + dtw * wi[:-1], 1.0 + dtw * wi[1:]
    return 0.5 * (1.0 - zb), 0.5 * (1.0 + zb), 0.5 * (1.0 - zt), 0.5 * (1.0 + zt)


def upwind_matrices(P, e, rho, velz, dtw):
    """VAB2_up [(nk+1) n2, nk n2] and VA2_up [(nk+1) n2, (nk+1) n2] of column e, dense"""
    nk, n2 = P.nk, P.n2e
    W, Q, det = P.arr("W", (P.mp12, n2)), P.arr("Q", (P.mp12,)), P.det[e]
    N0b, N1b, N0t, N1t = shape_functions(P, velz, dtw)
    AB, A = np.zeros(((nk + 1) * n2, nk * n2)), np.zeros(((nk + 1) * n2, (nk + 1) * n2))
    blk = lambda c: W.T @ (c[:, None] * W)
    q0 = Q * (SCALE / det)
    for k in range(nk):
        a, b = slice(k * n2, (k + 1) * n2), slice((k + 1) * n2, (k + 2) * n2)
        AB[a, a] += blk(0.5 * (N0b[k] + N0t[k]) * q0)
        AB[b, a] += blk(0.5 * (N1b[k] + N1t[k]) * q0)
        rk = (W @ rho[a]) * (0.5 / det)
        A[a, a] += blk(rk * N0b[k] * q0); A[a, b] += blk(rk * N0t[k] * q0)
        A[b, a] += blk(rk * N1b[k] * q0); A[b, b] += blk(rk * N1t[k] * q0)
    return AB, A


def diag_theta2_up(P, e, rho, rt, velz, dtw):
    AB, A = upwind_matrices(P, e, rho, velz, dtw)
    return np.linalg.solve(A, AB @ rt)


def diag_theta2_up_all(P, rho, rt, velz, dtw):
    return np.stack([diag_theta2_up(P, e, rho[e], rt[e], velz[e], dtw) for e in range(P.nEl)])


def max_upwind(P, velz, dtw):
    """max over columns, interfaces and quadrature points of |dtw w|"""
    W = P.arr("W", (P.mp12, P.n2e))
    return float(np.abs(dtw * np.einsum("qj,eij->eiq", W, velz.reshape(P.nEl, P.nk - 1, P.n2e))).max())


# ---- AssembleVertMomVort -------------------------------------------------------------------------------------------------------
def box_dense(c):
    """the horizontal oracle's dense global matrices on the one-patch periodic box of a case"""
    gd = GlobalDense.__new__(GlobalDense)
    gd.cs, gd.topos, gd.geoms, gd.sparse, gd.nk = c["bx"], [c["topo"]], [c["geom"]], False, c["P"].nk
    gd.N0, gd.N1, gd.N2 = c["bx"].nDofs0G, c["bx"].nDofs1G, c["bx"].nDofs2G
    gd.P = [c["P"]]
    gd.E21 = gd._e21()
    gd.E12 = -gd.E21.T
    return gd


def vert_mom_vort(c, gd, ul, velz_v):
    """uuz [nEl, (nk-1) n2e] (vertical layout) from ul [nk, N1] and velz in the vertical layout: for every interface
    dwdx = M1o^-1 E12 M2o w, uuz = Rz(1/2 u_k + 1/2 u_{k+1}; SCALE) dwdx (M1o, M2o: level 0, SCALE, no thickness), then HorizToVert"""
    P, nk = c["P"], c["P"].nk
    if "M1o" not in c:
        c["M1o"], c["M2o"] = gd.mat("UMAT", 0, 0), gd.mat("WMAT", 0, 0)
    wh = to_horiz(c, velz_v, nk - 1)
    uuz = np.zeros((nk - 1, gd.N2))
    for k in range(nk - 1):
        dwdx = np.linalg.solve(c["M1o"], gd.E12 @ (c["M2o"] @ wh[k]))
        uuz[k] = gd.mat("WTQDUDZ", 0, 0, 0.5 * ul[k] + 0.5 * ul[k + 1]) @ dwdx
    return to_vert([(c["topo"], c["geom"], P)], uuz, nk)


def to_horiz(c, vz, rows):
    """[nEl, rows n2e] vertical -> [rows, N2] horizontal on the one-patch box (L2Vecs::VertToHoriz)"""
    P = c["P"]
    pad = np.zeros((P.nEl, P.nk * P.n2e)); pad[:, :rows * P.n2e] = vz
    return P.vert_to_horiz(pad)[:rows]


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def solve_schur_2_box(P, dt, velz_i, rho_i, rt_i, exner_i, zv, nits, tol=0.0, udwdx=None, uuz=None, theta_up=True):
    """at most `nits` iterations of box/VertSolve.cpp:1328-1418 for every column: schur2_case.solve_schur_2 with flags = 3, rayleigh = 0, no
    Held-Suarez forcing, theta_i / theta_j from diag_theta2_up over 0.25 dt (theta_up=False: the lumped diagTheta2 of the eul loop) and, with
    udwdx and uuz = callable(velz_j) -> [nEl, (nk-1) n2e], F_w += 0.5 dt udwdx + 0.5 dt uuz_j, uuz_j = udwdx at first (:1326), = uuz(velz_j)
    at the end of every iteration (:1403).  Returns dict(velz, rho, rt, exner, theta_h, exner_h, history)."""
    nEl, nk, n2 = P.nEl, P.nk, P.n2e
    V10 = _v10(nk, n2)
    velz_j, rho_j, rt_j, exner_j = velz_i.copy(), rho_i.copy(), rt_i.copy(), exner_i.copy()

    def theta(rho, rt, velz):
        if theta_up:
            return diag_theta2_up_all(P, rho, rt, velz, 0.25 * dt)
        return np.stack([P.diag_theta2(e % P.nElsX, e // P.nElsX, rho[e], rt[e]) for e in range(nEl)])
    theta_i = theta(rho_i, rt_i, velz_i)
    theta_h = theta_i.copy()
    exner_h, velz_h, rho_h, rt_h = exner_i.copy(), velz_i.copy(), rho_i.copy(), rt_i.copy()
    uuz_j = None if udwdx is None else udwdx.copy()
    hist = []
    for it in range(nits):
        mx = dict(exner=0.0, w=0.0, rho=0.0, rt=0.0)
        for e in range(nEl):
            ex, ey = e % P.nElsX, e // P.nElsX
            F_w, F_z, G_z, _, _ = sc.assemble_residual(P, ex, ey, dt, theta_h[e], exner_h[e], velz_i[e], velz_j[e], rho_i[e], rho_j[e], zv[e], V10, 0.0)
            if udwdx is not None:
                F_w = F_w + 0.5 * dt * udwdx[e] + 0.5 * dt * uuz_j[e]
            F_exner = P.eos_residual(ex, ey, rt_j[e], exner_j[e])
            VB = P.colop_dense("CONST", ex, ey)
            F_rho = VB @ (rho_j[e] + dt * (V10 @ F_z) - rho_i[e])
            F_rt = VB @ (rt_j[e] + dt * (V10 @ G_z) - rt_i[e])
            sol = P.solve_schur_column_3(ex, ey, dt, theta_h[e], velz_h[e], rho_h[e], rt_h[e], exner_h[e], F_w, F_rho, F_rt, F_exner, flags=3)
            d_w, d_rho, d_rt, d_exner = sol["d_u"], sol["d_rho"], sol["d_rt"], sol["d_pi"]
            velz_j[e] += d_w; rho_j[e] += d_rho; rt_j[e] += d_rt; exner_j[e] += d_exner
            for k, (dx, x) in dict(exner=(d_exner, exner_j[e]), w=(d_w, velz_j[e]), rho=(d_rho, rho_j[e]), rt=(d_rt, rt_j[e])).items():
                ratio = np.linalg.norm(dx) / np.linalg.norm(x)
                mx[k] = ratio if ratio > mx[k] else mx[k]
            exner_h[e] = 0.5 * exner_i[e] + 0.5 * exner_j[e]; velz_h[e] = 0.5 * velz_i[e] + 0.5 * velz_j[e]
            rho_h[e] = 0.5 * rho_i[e] + 0.5 * rho_j[e]; rt_h[e] = 0.5 * rt_i[e] + 0.5 * rt_j[e]
        theta_h = 0.5 * theta(rho_j, rt_j, velz_j) + 0.5 * theta_i
        if udwdx is not None and uuz is not None:
            uuz_j = uuz(velz_j)
        hist.append(mx)
        if mx["exner"] < tol and mx["rho"] < tol and mx["rt"] < tol:
            break
    return dict(velz=velz_j, rho=rho_j, rt=rt_j, exner=exner_j, theta_h=theta_h, exner_h=exner_h, history=hist)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def make_box(oracle, pn, ne, nk, seed=None):
    """a one-patch doubly periodic box (box/ flavour: constant diagonal Jacobian) with perturbed levels, its oracle patch, the start state of
    schur2_case.state_at_rest with a seeded vertical velocity of max_q |DTW w| = UPWIND, a seeded horizontal velocity and a seeded udwdx"""
    from mimsem_amd.geom import BoxGeom
    from mimsem_amd.mesh import PeriodicBox, box_coords
    from mimsem_amd.topo import Topo
    seed = 100 * pn + 10 * ne + nk if seed is None else seed
    lx = 2.0 * ne                                       # det = (lx / (2 ne))^2 = 1: the 2-form dofs of velz are velocities (see finish_case)
    bx = PeriodicBox(pn, ne, 1); coords = box_coords(pn, ne, lx)
    t = Topo(bx, 0, nk)
    g = BoxGeom(t, bx, coords, nk, lx)
    r = np.random.default_rng(seed)
    levs = z_levels(nk, g.n0, r, ztop=300.0 * nk)
    g.set_levels(levs)
    P = oracle.Patch(pn, pn, bx.nel, nk)
    P.set_metric(g.det, g.J); P.set_levels(levs)
    return finish_case(dict(bx=bx, topo=t, geom=g, P=P, N1=bx.nDofs1G), r)


def make_sphere(oracle, pn, ne, nk, seed=None):
    """one face of a cubed sphere (varying det) with the same start state: the column entry only"""
    from tests.helpers import make_patch
    seed = 100 * pn + 10 * ne + nk + 1 if seed is None else seed
    cs, topo, geom, P, r = make_patch(oracle, pn, ne, 6, 1, nk=nk, seed=seed)
    return finish_case(dict(bx=None, topo=topo, geom=geom, P=P, N1=None), r)


def finish_case(c, r):
    """The reference upwinds with w NOT divided by det, so |DTW w| < 1 bounds the dofs of velz themselves.  The loop must stay there too:
    the start state is at rest but not in hydrostatic balance, the first iteration adds ~ g DT to w / det, and with det = 1 and DT = 0.1 that
    moves |DTW w| by 0.025; udwdx (0.1 m/s^2 in the weak form of F_w) and uuz (u ~ 1 m/s) move it by less."""
    P, geom = c["P"], c["geom"]
    st = sc.state_at_rest(P, geom, seed=int(r.integers(1 << 30)))
    w = r.standard_normal(st["velz"].shape)
    st["velz"] = w * (UPWIND / max_upwind(P, w, DTW))
    c["st"] = st
    Q = P.arr("Q", (P.mp12,))
    c["udwdx"] = 1e-1 * r.standard_normal(st["velz"].shape) * SCALE * float(Q.mean() * P.thick.mean() / P.det.mean())
    if c["N1"] is not None:
        c["ul"] = np.sqrt(P.det.mean()) * r.standard_normal((P.nk, c["N1"]))
    return c
