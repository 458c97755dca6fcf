"""tests/schur2_case.py -- numpy restatement of the vertical Newton loop VertSolve::solve_schur_2 (eul/VertSolve.cpp:1059-1246) with its
residual assembly (assemble_residual :386-430, diagnose_F_z :237-260, diagnose_Phi_z :262-286), column by column as the reference does,
on the dense column matrices and vector functions of the C oracle (pyoracle.Patch).  TEST INFRASTRUCTURE ONLY: the checker of
mimsem_amd/vertsolve.py::VertSolve.solve_schur_2; nothing in the product imports it.  Also the start states the tests share."""
import numpy as np

from oracle.vert_oracle import _v10

SCALE = 1.0e8               # eul/VertOps.cpp:21
RAYLEIGH = 4.0 / 120.0      # eul/VertSolve.cpp:32
GRAVITY = 9.80616
CP, CV, RD, P0 = 1004.5, 717.5, 287.0, 1.0e5


def assemble_residual(P, ex, ey, dt, theta, Pi, velz1, velz2, rho1, rho2, zv, V10, rayleigh=RAYLEIGH):
    """:386-430 -> fw, F, G, the pressure-gradient term dt VA(theta) VA^-1 V01 VB Pi alone, and F * tA1 entry by entry (:415)"""
    D = lambda op, **kw: P.colop_dense(op, ex, ey, **kw)
    V01 = -V10.T
    VAinv = D("LINEAR_INV")
    F = VAinv @ D("LINEAR_RT", flag=1, f1=rho1) @ (velz1 / 3 + velz2 / 6) + VAinv @ D("LINEAR_RT", flag=1, f1=rho2) @ (velz1 / 6 + velz2 / 3)
    W1, W2 = D("CONLIN_W", f1=velz1), D("CONLIN_W", f1=velz2)
    Phi = (W1 @ velz1 + W1 @ velz2 + W2 @ velz2) / 6 + zv
    VA, VB = D("LINEAR"), D("CONST")
    fw = VA @ velz2 - VA @ velz1 + dt * (V01 @ Phi)
    tA2 = VAinv @ (V01 @ (VB @ Pi))
    VAt = D("LINEAR_THETA", f1=theta)                 # theta on the nk+1 interfaces
    tA1 = VAt @ tA2
    fw = fw + dt * tA1
    G = VAinv @ (VAt @ F)
    if rayleigh:
        VR = D("RAYLEIGH")
        fw = fw + 0.5 * dt * rayleigh * (VR @ velz2 + VR @ velz1)
    return fw, F, G, dt * tA1, F * tA1


def solve_schur_2(P, dt, velz_i, rho_i, rt_i, exner_i, zv, nits, tol=0.0, dFx=None, dGx=None, udwdx=None, hs_forcing=False, columns=None,
                  rayleigh=RAYLEIGH, flags=0):
    """at most `nits` Newton iterations of :1119-1207 for every column of the patch (or of `columns`: the others keep their input state and
    the max-norms run over the subset); arrays [nEl][slots*n2e].  dFx / dGx: the horizontal forcing of :1124, either arrays [nEl][nk n2e]
    or a callable (rho_i, rho_j, theta_h) -> (dFx, dGx).  Stops when exner, rho and rt are all below tol (:1202).
    Returns a dict: velz, rho, rt, exner, theta_h, exner_h, history, k2i_z, k2i_abs (sum of |F tA1| / SCALE: the scale of k2i_z's round-off),
    F_w1 / pgrad1 (F_w and its pressure-gradient term at iteration 1)."""
    nEl, nk, n2 = P.nEl, P.nk, P.n2e
    cols = list(range(nEl)) if columns is None else [int(c) for c in columns]
    V10 = _v10(nk, n2)
    velz_j, rho_j, rt_j, exner_j = velz_i.copy(), rho_i.copy(), rt_i.copy(), exner_i.copy()

    def col(f):
        out = np.zeros((nEl, (nk + 1) * n2))
        for e in cols:
            out[e] = f(e % P.nElsX, e // P.nElsX, e)
        return out
    theta_i = col(lambda ex, ey, e: P.diag_theta2(ex, ey, rho_i[e], rt_i[e]))
    theta_h = theta_i.copy()
    exner_h, velz_h, rho_h, rt_h = exner_i.copy(), velz_i.copy(), rho_i.copy(), rt_i.copy()
    hist = []
    k2i_z = k2i_abs = 0.0
    F_w1 = np.zeros_like(velz_i); pgrad1 = np.zeros_like(velz_i)
    for it in range(nits):
        mx = dict(exner=0.0, w=0.0, rho=0.0, rt=0.0)
        k2i_z = k2i_abs = 0.0
        fx, gx = dFx(rho_i, rho_j, theta_h) if callable(dFx) else (dFx, dGx)
        for e in cols:
            ex, ey = e % P.nElsX, e // P.nElsX
            F_w, F_z, G_z, pg, k2 = assemble_residual(P, ex, ey, dt, theta_h[e], exner_h[e], velz_i[e], velz_j[e], rho_i[e], rho_j[e], zv[e], V10,
                                                      rayleigh)
            k2i_z += k2.sum() / SCALE; k2i_abs += np.abs(k2).sum() / SCALE
            if udwdx is not None:
                F_w = F_w + dt * udwdx[e]
            if it == 0:
                F_w1[e] = F_w; pgrad1[e] = pg
            F_exner = P.eos_residual(ex, ey, rt_j[e], exner_j[e])
            VB = P.colop_dense("CONST", ex, ey)
            dF_z = rho_j[e] + dt * (V10 @ F_z) - rho_i[e]
            dG_z = rt_j[e] + dt * (V10 @ G_z) - rt_i[e]
            if fx is not None:
                dF_z = dF_z + dt * fx[e]
                dG_z = dG_z + dt * gx[e]
            F_rho = VB @ dF_z
            F_rt = VB @ dG_z
            if hs_forcing:
                F_rt = F_rt + dt * P.temp_forcing_hs(ex, ey, exner_h[e], theta_h[e], rho_h[e])
            sol = P.solve_schur_column_3(ex, ey, dt, theta_h[e], velz_h[e], rho_h[e], rt_h[e], exner_h[e], F_w, F_rho, F_rt, F_exner, flags=flags)
            d_w, d_rho, d_rt, d_exner = sol["d_u"], sol["d_rho"], sol["d_rt"], sol["d_pi"]
            velz_j[e] += d_w; rho_j[e] += d_rho; rt_j[e] += d_rt; exner_j[e] += d_exner
            for k, (dx, x) in dict(exner=(d_exner, exner_j[e]), w=(d_w, velz_j[e]), rho=(d_rho, rho_j[e]), rt=(d_rt, rt_j[e])).items():
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.linalg.norm(dx) / np.linalg.norm(x)
                mx[k] = ratio if ratio > mx[k] else mx[k]                 # MaxNorm :233 (a NaN ratio loses the comparison)
            exner_h[e] = 0.5 * exner_i[e] + 0.5 * exner_j[e]; velz_h[e] = 0.5 * velz_i[e] + 0.5 * velz_j[e]
            rho_h[e] = 0.5 * rho_i[e] + 0.5 * rho_j[e]; rt_h[e] = 0.5 * rt_i[e] + 0.5 * rt_j[e]
        theta_h = 0.5 * col(lambda ex, ey, e: P.diag_theta2(ex, ey, rho_j[e], rt_j[e])) + 0.5 * theta_i
        hist.append(mx)
        if mx["exner"] < tol and mx["rho"] < tol and mx["rt"] < tol:
            break
    return dict(velz=velz_j, rho=rho_j, rt=rt_j, exner=exner_j, theta_h=theta_h, exner_h=exner_h, history=hist, k2i_z=k2i_z, k2i_abs=k2i_abs,
                F_w1=F_w1, pgrad1=pgrad1)


# ---- the start states ----------------------------------------------------------------------------------------------------------
def geopotential(P, geom):
    """VertSolve::initGZ (:89-175): zv_k = W^T diag(SCALE w_q / 2) (g z_k + g z_{k+1}) in the vertical layout"""
    nEl, nk, n2 = P.nEl, P.nk, P.n2e
    W, Q = P.arr("W", (P.mp12, n2)), P.arr("Q", (P.mp12,))
    inds0, levs = geom.all_inds0_l(), geom.levs
    zv = np.zeros((nEl, nk * n2))
    for e in range(nEl):
        for k in range(nk):
            zv[e, k * n2:(k + 1) * n2] = W.T @ (SCALE * 0.5 * Q * GRAVITY * (levs[k, inds0[e]] + levs[k + 1, inds0[e]]))
    return zv


def _two_form(P, geom, v):
    """a value v[k] per level as the 2-form with DoF_j = v * (area of sub-cell j) * det * thickness (the edge functions histopolate)"""
    nEl, nk, n2 = P.nEl, P.nk, P.n2e
    inds0 = geom.all_inds0_l()
    wd = np.diff(P.arr("qx", (P.mp1,)))
    wj = np.outer(wd, wd).ravel()
    detm = P.det.mean(axis=1)
    out = np.zeros((nEl, nk * n2))
    for e in range(nEl):
        for k in range(nk):
            out[e, k * n2:(k + 1) * n2] = v[k] * wj * detm[e] * P.thick[k, inds0[e]].mean()
    return out


def state_at_rest(P, geom, seed=29, pert=1e-4):
    """the state of tests/test_gpu_column.py::test_vertical_newton_loop_matches_oracle: an EOS-consistent column at rest with `pert`
    relative perturbations, velz = 0 -> dict(velz, rho, rt, exner, zv)"""
    r = np.random.default_rng(seed)
    nEl, nk, n2 = P.nEl, P.nk, P.n2e
    rho_v, th_v = np.linspace(1.2, 0.5, nk), np.linspace(290.0, 330.0, nk)
    pi_v = CP * (RD * rho_v * th_v / P0) ** (RD / CV)
    p = lambda: 1.0 + pert * r.standard_normal((nEl, nk * n2))
    rho, rt, exner = _two_form(P, geom, rho_v) * p(), _two_form(P, geom, rho_v * th_v) * p(), _two_form(P, geom, pi_v) * p()
    return dict(velz=np.zeros((nEl, (nk - 1) * n2)), rho=rho, rt=rt, exner=exner, zv=geopotential(P, geom))


def hydrostatic_state(P, geom, theta0=300.0):
    """an unperturbed isentropic column in hydrostatic balance: theta = theta0, Pi(z) = cp - g z / theta0 (so that theta dPi/dz = -g) at the
    mid-height of every level and quadrature point, rho from the equation of state, each projected onto the 2-forms through the level mass
    matrix (dof = VB^-1 W^T Q SCALE v: VB dof reproduces the pointwise values exactly); velz = 0"""
    nEl, nk, n2 = P.nEl, P.nk, P.n2e
    W, Q = P.arr("W", (P.mp12, n2)), P.arr("Q", (P.mp12,))
    inds0, levs = geom.all_inds0_l(), geom.levs
    rho, rt, exner = (np.zeros((nEl, nk * n2)) for _ in range(3))
    for e in range(nEl):
        VBinv = P.colop_dense("CONST_INV", e % P.nElsX, e // P.nElsX)
        zmid = 0.5 * (levs[:-1, inds0[e]] + levs[1:, inds0[e]])                  # [nk, mp12]
        pi_q = CP - GRAVITY * zmid / theta0
        rho_q = P0 / (RD * theta0) * (pi_q / CP) ** (CV / RD)
        proj = lambda vq: VBinv @ np.concatenate([W.T @ (SCALE * Q * vq[k]) for k in range(nk)])
        rho[e], exner[e] = proj(rho_q), proj(pi_q)
        rt[e] = theta0 * rho[e]
    return dict(velz=np.zeros((nEl, (nk - 1) * n2)), rho=rho, rt=rt, exner=exner, zv=geopotential(P, geom))


def extras(P, st, dt, seed=41):
    """the optional inputs, all on: latitude of the quadrature points (Held-Suarez), a u dw/dx term (0.1 m/s^2 as a 1-form: large enough to move
    every field by more than 100 x the parity bar within three iterations at dt = 30), and a seeded random horizontal forcing of the
    size of (rho_j - rho_i)/dt of the unforced loop (1e-4 relative perturbations relax within a few iterations: ~ 1e-4 rho / dt)"""
    r = np.random.default_rng(seed)
    nEl, nk, n2 = P.nEl, P.nk, P.n2e
    lat = np.ascontiguousarray(P.sq[:, 1][P.elinds("q")])
    udwdx = 1e-1 * r.standard_normal((nEl, (nk - 1) * n2)) * float(np.abs(st["zv"]).mean()) / GRAVITY / 1.5e4
    dFx = 1e-4 * r.standard_normal((nEl, nk * n2)) * st["rho"] / dt
    dGx = 1e-4 * r.standard_normal((nEl, nk * n2)) * st["rt"] / dt
    return dict(lat=lat, udwdx=udwdx, dFx=dFx, dGx=dGx)
