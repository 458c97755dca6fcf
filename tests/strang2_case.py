"""The numpy restatement of Euler::Strang (eul/Euler_2.cpp:1146-1364) and of the two right-hand sides it adds to Strang_ec's --
HorizSolve::advection_rhs (eul/HorizSolve.cpp:330-375, with diagnose_fluxes' theta_in_Wt = true branch :313-317) and
HorizSolve::momentum_rhs (:496-635) -- shared by tests/test_strang2_cpu.py, tests/test_gpu_flux_rhs.py, tests/test_gpu_horiz_rhs2.py and
tests/test_gpu_strang2.py, and the point-wise form of the mass-flux right-hand side csrc/flux_rhs.inc is written from.
TEST INFRASTRUCTURE ONLY.

Case: strang_case.make_case() (p = 3, ne = 2, nk = 4, DT = 0.5, NITS = 3 Newton iterations on both sides, no convergence test).

Restatement: oracle.horiz_oracle.GlobalDense / HorizOracle (dense LU for every KSPSolve) for the horizontal operators, the functions of
tests/vort_diag_case.py, the dense M1 (+ M1ray) of strang_case, and newton2(): the Newton loop of VertSolve::solve_schur_2 over ALL patches
with the horizontal forcing re-evaluated once per iteration (eul/VertSolve.cpp:1123-1124), written after strang_case.newton with
schur2_case.assemble_residual (schur2_case.solve_schur_2 itself is per patch).

Layouts as in strang_case; theta of the non-_ec routines lies on the nk+1 interfaces: [nk+1, N2] horizontal, [nEl, (nk+1) n2e] vertical.

Not restated, as in mimsem_amd/euler.py: :1180 (vert->theta_h filled on the first step, overwritten by solve_schur_2 before any read) and
the order of the local velocity copies at :1269 (each velocity is paired with itself)."""
import numpy as np

from tests import schur2_case as s2
from tests import strang_case as sc
from tests import vort_diag_case as vc

SCALE = sc.SCALE
CAP = 1e-8
# the bars of a device step against Restatement2 per field (tests/test_gpu_strang2.py: relative L2; the error observed on an MI355X x 10,
# rounded up to a power of ten, none above CAP); the sensitivity conditions of tests/test_strang2_cpu.py are stated against them
BARS = {1: dict(velx=1e-14, velz=1e-13, rho=1e-15, rt=1e-16, exner=1e-14),
        2: dict(velx=1e-13, velz=1e-13, rho=1e-15, rt=1e-15, exner=1e-14)}


def flux_rhs_pointwise(P, lev, u1, u2, h1, h2, scale=SCALE):
    """the point-wise form of sum_ab c_ab Uvec::assemble_hu(lev, scale, u_a, h_b, false, c_ab) (eul/Assembly.cpp:2198-2279; c_11 = c_22 = 1/3,
    c_12 = c_21 = 1/6) on one patch: with t = thickInv, d = det, J the Jacobian, Q the weight, (u_a, v_a) the local interpolants of u_a
    (interp1_l) and r_b the interpolant of h_b over d (interp2_g),
        m = scale Q t^2 / d,  (U, V) = r1 (u1/3 + u2/6, v1/3 + v2/6) + r2 (u1/6 + u2/3, v1/6 + v2/3)
        c_x = m (Gaa U + Gab V), c_y = m (Gab U + Gbb V),  out_x[e] = Ut c_x, out_y[e] = Vt c_y, summed over the elements of the patch.
    u1, u2, h1, h2: patch-local vectors of the level.  Returns the patch-local 1-form vector (Uvec's vl)"""
    U, V, Q = P.arr("U", (P.mp12, P.n1e)), P.arr("V", (P.mp12, P.n1e)), P.arr("Q", (P.mp12,))
    iq, ix, iy = P.elinds("q"), P.elinds("n1x"), P.elinds("n1y")
    out = np.zeros(P.n1)
    for e in range(P.nEl):
        ex, ey = e % P.nElsX, e // P.nElsX
        cx, cy = np.zeros(P.mp12), np.zeros(P.mp12)
        for q in range(P.mp12):
            px, py = q % P.mp1, q // P.mp1
            J = np.array(P.J[e, q]).reshape(2, 2); d = P.det[e, q]; ti = P.thickInv[lev, iq[e, q]]
            a1, a2 = (np.array(P.interp("1l", ex, ey, px, py, u)) for u in (u1, u2))
            r1, r2 = (P.interp("2g", ex, ey, px, py, h)[0] for h in (h1, h2))
            UV = r1 * (a1 / 3.0 + a2 / 6.0) + r2 * (a1 / 6.0 + a2 / 3.0)
            G = J.T @ J                                                              # [[Gaa, Gab], [Gab, Gbb]]
            cx[q], cy[q] = (scale * Q[q] * ti * ti / d) * (G @ UV)
        np.add.at(out, ix[e], U.T @ cx)
        np.add.at(out, iy[e], V.T @ cy)
    return out


def flux_rhs(gd, lev, u1, u2, h1, h2):
    """the assembled four-term sum of a level from GlobalDense.uvec_hu (:300-305)"""
    return gd.uvec_hu(lev, u1, h1, 1.0 / 3.0) + gd.uvec_hu(lev, u1, h2, 1.0 / 6.0) \
        + gd.uvec_hu(lev, u2, h1, 1.0 / 6.0) + gd.uvec_hu(lev, u2, h2, 1.0 / 3.0)


def diagnose_fluxes(hz, lev, u1, u2, h1, h2, theta):
    """:285-327 with theta_in_Wt = true: theta [nk+1, N2] on the interfaces, G = M1^-1 F(1/2 theta_k + 1/2 theta_k+1; no vert_scale) F"""
    g = hz.g
    F = hz._solve(hz.M1[lev], flux_rhs(g, lev, u1, u2, h1, h2), ("M1", lev))
    th = 0.5 * theta[lev] + 0.5 * theta[lev + 1]
    G = hz._solve(hz.M1[lev], g.mat("UHMAT", lev, 0, th) @ F, ("M1", lev))
    return F, G


def advection_rhs(hz, u1, u2, h1, h2, theta):
    """:330-375 (do_temp_visc = false) -> dF = E21 Fk, dG = E21 Gk [nk, N2] and Fk, Gk [nk, N1]"""
    g = hz.g
    dF, dG, Fk, Gk = (np.zeros((hz.nk, n)) for n in (g.N2, g.N2, g.N1, g.N1))
    for k in range(hz.nk):
        Fk[k], Gk[k] = diagnose_fluxes(hz, k, u1[k], u2[k], h1[k], h2[k], theta)
        dF[k], dG[k] = g.E21 @ Fk[k], g.E21 @ Gk[k]
    return dF, dG, Fk, Gk


def momentum_rhs(hz, lev, theta, dudz1, dudz2, velz1, velz2, Pi, velx1, velx2, rho1, rho2, Fx=None, Fz=None, dwdx1=None, dwdx2=None, Fk=None):
    """:496-635; theta [nk+1, N2] on the interfaces, Pi and the velocities / densities this level's vectors, the rest [nk-1, .] interface
    arrays.  Returns fu, or with Fk (this level's mass flux) given (fu, k2i term, sum of |Fk . dp| entries / SCALE)"""
    g = hz.g
    theta_h = 0.5 * theta[lev] + 0.5 * theta[lev + 1]                                   # :514-517
    Phi = hz.diagnose_Phi(lev, velx1, velx2, velz1, velz2)
    dPi = hz.grad(Pi, lev)
    fu = g.E12 @ Phi
    uh = 0.5 * velx1 + 0.5 * velx2
    q = hz.diagnose_q(lev, 0.5 * rho1 + 0.5 * rho2, uh)
    R = g.mat("ROTMAT", lev, 0, q)
    if Fx is None:
        Fx = hz._solve(hz.M1[lev], flux_rhs(g, lev, velx1, velx2, rho1, rho2), ("M1", lev))    # :538-548
    fu = fu + R @ Fx
    dp = g.mat("UHMAT", lev, 0, theta_h) @ dPi                                          # :556-558
    fu = fu + dp
    for il in ((lev - 1,) if lev > 0 else ()) + ((lev,) if lev < hz.nk - 1 else ()):    # :565-607
        dz = 0.5 * dudz1[il] + 0.5 * dudz2[il]
        if dwdx1 is not None:
            dz = dz - 0.5 * dwdx1[il] - 0.5 * dwdx2[il]
        Rh = g.mat("UTQWMAT", 0, 0, dz)
        v = Fz[il] if Fz is not None else 0.5 * velz1[il] + 0.5 * velz2[il]
        fu = fu + 0.5 * (Rh @ v)
    if hz.do_visc:
        fu = fu + hz.M1[lev] @ hz.laplacian(hz.laplacian(uh, lev), lev)
    if Fk is None:
        return fu
    return fu, float(Fk @ dp) / SCALE, float(np.abs(Fk * dp).sum()) / SCALE


def theta_interfaces(c, rho, rt):
    """VertSolve::diagTheta2 (= Euler::diagTheta) of horizontal rho, rt -> [nk+1, N2] horizontal"""
    rv, tv = sc.to_vert(c, rho), sc.to_vert(c, rt)
    where = [(P, e) for _, _, P in c["patches"] for e in range(P.nEl)]
    th = np.stack([P.diag_theta2(e % P.nElsX, e // P.nElsX, rv[E], tv[E]) for E, (P, e) in enumerate(where)])
    return to_horiz(c, th, c["nk"] + 1)


def to_horiz(c, av, rows):
    """strang_case.to_horiz for up to nk+1 rows (the interface fields)"""
    nk, out, e0 = c["nk"], np.zeros((rows, c["gd"].N2)), 0
    for t, g, P in c["patches"]:
        n2 = P.n2e
        a = av[e0:e0 + P.nEl].reshape(P.nEl, rows, n2)
        i2 = P.elinds("n2")
        own = sc._own(t)
        for k in range(rows):
            row = np.zeros(P.n2)
            row[i2] = a[:, k, :]
            out[k, own] = row
        e0 += P.nEl
    return out


def newton2(c, dt, velz_i, rho_i, rt_i, exner_i, zv, nits, forcing=None, hs_forcing=False):
    """`nits` iterations of VertSolve::solve_schur_2 (eul/VertSolve.cpp:1119-1207) for every column of every patch (vertical arrays
    [nEl, slots n2e], elements patch by patch).  forcing(rho_i, rho_j, theta_h) -> (dFx, dGx) in the vertical layout: HorizSolve::advection_rhs
    at the head of every iteration (:1124), added to dF_z / dG_z before the VB product (:1145-1146).  Returns (velz, rho, rt, exner) of
    the new time level and the time-centred theta_h [nEl, (nk+1) n2e], exner_h the loop leaves in VertSolve"""
    from oracle.vert_oracle import _v10
    where = [(P, e) for _, _, P in c["patches"] for e in range(P.nEl)]
    P0 = where[0][0]
    V10 = _v10(P0.nk, P0.n2e)
    velz_j, rho_j, rt_j, exner_j = velz_i.copy(), rho_i.copy(), rt_i.copy(), exner_i.copy()
    col = lambda f: np.stack([f(P, e % P.nElsX, e // P.nElsX, E) for E, (P, e) in enumerate(where)])
    theta_i = col(lambda P, ex, ey, E: P.diag_theta2(ex, ey, rho_i[E], rt_i[E]))
    theta_h = theta_i.copy()
    exner_h, velz_h, rho_h, rt_h = exner_i.copy(), velz_i.copy(), rho_i.copy(), rt_i.copy()
    for _ in range(nits):
        dFx, dGx = forcing(rho_i, rho_j, theta_h) if forcing is not None else (None, None)
        for E, (P, e) in enumerate(where):
            ex, ey = e % P.nElsX, e // P.nElsX
            F_w, F_z, G_z, _, _ = s2.assemble_residual(P, ex, ey, dt, theta_h[E], exner_h[E], velz_i[E], velz_j[E], rho_i[E], rho_j[E], zv[E], V10)
            F_exner = P.eos_residual(ex, ey, rt_j[E], exner_j[E])
            VB = P.colop_dense("CONST", ex, ey)
            dF_z = rho_j[E] + dt * (V10 @ F_z) - rho_i[E]
            dG_z = rt_j[E] + dt * (V10 @ G_z) - rt_i[E]
            if dFx is not None:
                dF_z = dF_z + dt * dFx[E]
                dG_z = dG_z + dt * dGx[E]
            F_rho, F_rt = VB @ dF_z, VB @ dG_z
            if hs_forcing:
                F_rt = F_rt + dt * P.temp_forcing_hs(ex, ey, exner_h[E], theta_h[E], rho_h[E])
            sol = P.solve_schur_column_3(ex, ey, dt, theta_h[E], velz_h[E], rho_h[E], rt_h[E], exner_h[E], F_w, F_rho, F_rt, F_exner, flags=0)
            velz_j[E] += sol["d_u"]; rho_j[E] += sol["d_rho"]; rt_j[E] += sol["d_rt"]; exner_j[E] += sol["d_pi"]
            exner_h[E] = 0.5 * exner_i[E] + 0.5 * exner_j[E]; velz_h[E] = 0.5 * velz_i[E] + 0.5 * velz_j[E]
            rho_h[E] = 0.5 * rho_i[E] + 0.5 * rho_j[E]; rt_h[E] = 0.5 * rt_i[E] + 0.5 * rt_j[E]
        theta_h = 0.5 * col(lambda P, ex, ey, E: P.diag_theta2(ex, ey, rho_j[E], rt_j[E])) + 0.5 * theta_i
    return (velz_j, rho_j, rt_j, exner_j), theta_h, exner_h


class Restatement2(sc.Restatement):
    """Euler::Strang, stage by stage, on Restatement's carried state"""

    def __init__(self, c, dt=sc.DT, nits=sc.NITS, hs_forcing=False, transport=True):
        """transport = False: stage 2 without the horizontal forcing (the sensitivity check of tests/test_strang2_cpu.py)"""
        super().__init__(c, dt, nits, hs_forcing)
        self.transport = transport

    def momentum_rhs(self, theta, dudz1, dudz2, velz1, velz2, Pi, velx1, velx2, rho1, rho2, Fz, dwdx1, dwdx2, Fk=None):
        out = [momentum_rhs(self.hz, k, theta, dudz1, dudz2, velz1, velz2, Pi[k], velx1[k], velx2[k], rho1[k], rho2[k],
                            Fz=Fz, dwdx1=dwdx1, dwdx2=dwdx2, Fk=None if Fk is None else Fk[k]) for k in range(self.c["nk"])]
        if Fk is None:
            return np.stack(out)
        self.k2i, self.k2i_abs = sum(o[1] for o in out), sum(o[2] for o in out)          # :560-563
        return np.stack([o[0] for o in out])

    def stage1(self, velx, velz_h0, rho, rt, exner):
        """:1186-1251 -> predictor velx"""
        gd = self.gd
        if not self.first_step:
            self.uz_prev = self.uz.copy()                                              # :1187-1189
        self.u_prev, self.u_curr = self.u_curr, velx.copy()                            # :1195-1196
        theta_0 = theta_interfaces(self.c, rho, rt)                                     # :1201-1202
        self.uz = vc.horiz_pot_vort(gd, velx, rho)[0]                                   # :1203
        self.dwdx1 = vc.vert_vort(gd, velz_h0, rho)[0]                                  # :1204
        if self.first_step:
            self.uz_prev = self.uz.copy()                                              # :1205
        Fz = vc.vert_mass_flux(gd, velz_h0, velz_h0, rho, rho)                          # :1206
        self.Fu_1 = self.momentum_rhs(theta_0, self.uz, self.uz, velz_h0, velz_h0, exner, velx, velx, rho, rho, Fz, self.dwdx1, self.dwdx1)
        ex = exner if self.hs_forcing else None
        if self.first_step:
            return sc.momentum_update(self.dense, self.hz.M1, self.dt, velx, self.Fu_1, 1.0, ex)         # :1214-1219
        return sc.momentum_update(self.dense, self.hz.M1, self.dt, self.u_prev, self.Fu_1, 2.0, ex)      # :1220-1226 (leapfrog)

    def stage2(self, velx_0, velx_p, velz_v, rho, rt, exner):
        """:1253-1260 -> (velz, rho, rt, exner) of the new time level in the vertical layout; leaves theta_h [nk+1, N2], exner_h (horizontal)"""
        c, nk = self.c, self.c["nk"]
        self.Fk = None

        def forcing(rho_i, rho_j, theta_h):
            dF, dG, self.Fk, _ = advection_rhs(self.hz, velx_0, velx_p, rho, sc.to_horiz(c, rho_j, nk), to_horiz(c, theta_h, nk + 1))
            return sc.to_vert(c, dF), sc.to_vert(c, dG)
        new, th, eh = newton2(c, self.dt, velz_v, sc.to_vert(c, rho), sc.to_vert(c, rt), sc.to_vert(c, exner), c["zv_v"], self.nits,
                              forcing=forcing if self.transport else None, hs_forcing=self.hs_forcing)
        self.theta_h, self.exner_h = to_horiz(c, th, nk + 1), sc.to_horiz(c, eh, nk)
        return new

    def stage3(self, velx_0, velx_p, velz_h0, velz_hn, rho_0, rho_n, exner_n):
        """:1262-1300 -> the corrected velx"""
        gd = self.gd
        self.uz = vc.horiz_pot_vort(gd, velx_p, rho_n)[0]                               # :1264
        dwdx2 = vc.vert_vort(gd, velz_hn, rho_n)[0]                                     # :1265
        Fz = vc.vert_mass_flux(gd, velz_h0, velz_hn, rho_0, rho_n)                      # :1266
        self.Fu_3 = self.momentum_rhs(self.theta_h, self.uz, self.uz_prev, velz_hn, velz_h0, self.exner_h, velx_0, velx_p, rho_0, rho_n,
                                      Fz, self.dwdx1, dwdx2, Fk=self.Fk)
        return sc.momentum_update(self.dense, self.hz.M1, self.dt, velx_0, self.Fu_3, 1.0, exner_n if self.hs_forcing else None)
