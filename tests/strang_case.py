"""The case and the numpy restatement of Euler::Strang_ec (eul/Euler_2.cpp:1366-1557) shared by tests/test_strang_cpu.py and
tests/test_gpu_strang.py, and the point-wise Bernoulli formula tests/test_gpu_bernoulli.py is written from.

Case: the p = 3, ne = 2 cubed sphere of tests/vort_diag_case.py with nk = 4 levels (the Rayleigh layer of the vertical solve needs four;
z_levels of tests/helpers.py), the EOS-consistent column at rest with 1e-4 perturbations of
tests/test_gpu_column.py::test_vertical_newton_loop_matches_oracle on every patch, the physically scaled random velx of vort_diag_case and a
vertical velocity of 0.1 m/s scale (not zero: HorizSolve::diagVertVort of a zero field is a solve with a zero right-hand side), dt = 0.5, and
a FIXED Newton count (NITS iterations, no convergence test) on both sides.

Restatement: composes what the other restatements already provide -- oracle.horiz_oracle.GlobalDense / HorizOracle for the right-hand sides
(dense LU for every KSPSolve), the functions of tests/vort_diag_case.py for HorizPotVort / diagVertVort / VertMassFlux, the dense M1 (+ M1ray) of
tests/hmomentum_case.py for the momentum update, energetics_case.theta_L2, and newton(), the Newton loop of oracle/vert_oracle.py
(VertSolve::solve_schur_eta, eul/VertSolve.cpp:1721-1973) with the horizontal transport tendencies dFx, dGx of :1799 and :1823-1825 added.

Layouts (numpy, global numbering): velx [nk, N1]; rho, rt, exner [nk, N2] horizontal; velz [nEl, (nk-1) n2e] vertical, elements patch by
patch (the device's numbering="global" order).

Not restated: the reference hands momentum_rhs_ec of stage 3 the LOCAL velocity vectors in the other order than the global ones (:1475: velx_0,
velx with ul, ul_prev); the restatement, like mimsem_amd/euler.py, pairs each global vector with its own local copy."""
import numpy as np

from tests import energetics_case as ec
from tests import hmomentum_case as hm
from tests import vort_diag_case as vc
from tests.helpers import z_levels

PN, NE, NK = 3, 2, 4
DT, NITS = 0.5, 3
SCALE = 1.0e8


def _own(t):
    return t.pi * t.n2 + np.arange(t.n2)


def to_horiz(c, av, rows):
    """[nEl, rows n2e] vertical -> [rows, N2] horizontal, patch by patch (L2Vecs::VertToHoriz)"""
    nk, out, e0 = c["nk"], np.zeros((rows, c["gd"].N2)), 0
    for t, g, P in c["patches"]:
        b = np.zeros((P.nEl, nk * P.n2e))
        b[:, :rows * P.n2e] = av[e0:e0 + P.nEl]
        out[:, _own(t)] = P.vert_to_horiz(b)[:rows]
        e0 += P.nEl
    return out


def to_vert(c, a):
    return ec.to_vert(c["patches"], a, c["nk"])


def make_case(seed=31, nk=NK):
    """mesh, dense global matrices, geopotential and the initial state; the oracle library must be built (the `oracle` fixture)"""
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from oracle import horiz_oracle as ho
    cs = CubedSphere(PN, NE, 6); coords = sphere_coords(PN, NE)
    topos = [Topo(cs, p, nk) for p in range(6)]
    geoms = [Geom(t, cs, coords, nk) for t in topos]
    levs = z_levels(nk, geoms[0].n0)
    for g in geoms:
        g.set_levels(levs)
    gd = ho.GlobalDense(cs, topos, geoms, coords, levs)
    c = dict(cs=cs, coords=coords, topos=topos, geoms=geoms, levs=levs, gd=gd, ho=ho, nk=nk, patches=list(zip(topos, geoms, gd.P)))
    r = np.random.default_rng(seed)
    area = np.mean([P.det.mean() for P in gd.P]) * 4.0 / (PN * PN); dz = np.mean([P.thick.mean() for P in gd.P]); ln = np.sqrt(area)
    # the column at rest of test_vertical_newton_loop_matches_oracle: a constant value v is the 2-form with DoF_j = v * (area of sub-cell j)
    # * det * thickness
    rho_v, th_v = np.linspace(1.2, 0.5, nk), np.linspace(290.0, 330.0, nk)
    pi_v = 1004.5 * (287.0 * rho_v * th_v / 1.0e5) ** (287.0 / 717.5)
    cols = {n: [] for n in ("rho", "rt", "exner")}
    for t, g, P in c["patches"]:
        n2 = P.n2e
        wd = np.diff(P.arr("qx", (P.mp1,))); wj = np.outer(wd, wd).ravel()
        inds0 = g.all_inds0_l()
        detm = P.det.mean(axis=1)
        thm = np.stack([[P.thick[k, inds0[e]].mean() for k in range(nk)] for e in range(P.nEl)])
        for n, v in (("rho", rho_v), ("rt", rho_v * th_v), ("exner", pi_v)):
            a = np.zeros((P.nEl, nk * n2))
            for e in range(P.nEl):
                for k in range(nk):
                    a[e, k * n2:(k + 1) * n2] = v[k] * wj * detm[e] * thm[e, k]
            cols[n].append(a * (1.0 + 1e-4 * r.standard_normal(a.shape)))
    for n in cols:
        c[n] = to_horiz(c, np.concatenate(cols[n]), nk)
    c["velx"] = r.standard_normal((nk, gd.N1)) * 20.0 * ln * dz
    c["velz_v"] = to_vert(c, 0.1 * r.standard_normal((nk - 1, gd.N2)) * area)
    c["zv_v"] = ec.init_gz(c["patches"], levs, nk)
    c["lat"] = np.concatenate([P.sq[:, 1][P.elinds("q")] for P in gd.P])           # Geom::s[.][1] at the quadrature points [nEl, mp12]
    c["state"] = (c["velx"], c["velz_v"], c["rho"], c["rt"], c["exner"])
    return c


class DenseM1(hm.Sphere):
    """hmomentum_case.Sphere's dense M1 / M1ray assembly (element matrices of the oracle, assembled by global edge id) on the patches of a case"""

    def __init__(self, c):
        self.patches = c["gd"].P
        P = self.patches[0]
        self.nElp, self.n1e, self.n2e = P.nEl, P.n1e, P.n2e
        self.n1, self.n2 = c["gd"].N1, c["gd"].N2
        self.idx = np.concatenate([np.concatenate([t.all_inds1x_g(), t.all_inds1y_g()], axis=1) for t in c["topos"]])
        self._m1 = {}
        self._own = [_own(t) for t in c["topos"]]

    def local2(self, f):
        """a global 2-form row as the list of patch-local vectors m1ray takes"""
        return [np.ascontiguousarray(f[o]) for o in self._own]


def momentum_update(dense, M1, dt, u_a, Fu, cfac, exner=None):
    """(M1 [+ M1ray(c dt, exner[k], exner[0])]) velx = M1 u_a - c dt Fu on every level (eul/Euler_2.cpp:1431-1453, :1477-1489); M1: one dense
    matrix per level; exner None: no Held-Suarez friction"""
    out = np.zeros_like(u_a)
    for k in range(u_a.shape[0]):
        A = M1[k]
        b = A @ u_a[k] - cfac * dt * Fu[k]
        if exner is not None:
            A = A + dense.m1ray(k, cfac * dt, dense.local2(exner[k]), dense.local2(exner[0]))
        out[k] = np.linalg.solve(A, b)
    return out


def newton(c, dt, velz_i, rho_i, rt_i, exner_i, zv, nits, forcing=None, hs_forcing=False):
    """`nits` iterations of VertSolve::solve_schur_eta for every column of every patch, written after oracle/vert_oracle.py::solve_schur_eta
    (vertical arrays [nEl, slots n2e], elements patch by patch).  forcing(rho_i, rho_j, theta_l2_h) -> (dFx, dGx) in the vertical layout:
    HorizSolve::advection_rhs_ec re-evaluated at the head of every iteration (:1798-1799), added as F_rho += dt dFx, F_rt += dt dGx
    (:1823-1825).  Returns (velz, rho, rt, exner) of the new time level and the time-centred theta_l2_h, exner_h the loop leaves in VertSolve"""
    from oracle.vert_oracle import _v10, assemble_residual_ec
    where = [(P, e) for _, _, P in c["patches"] for e in range(P.nEl)]
    P0 = where[0][0]
    V10 = _v10(P0.nk, P0.n2e)
    velz_j, rho_j, rt_j, exner_j = velz_i.copy(), rho_i.copy(), rt_i.copy(), exner_i.copy()
    col = lambda f: np.stack([f(P, e % P.nElsX, e // P.nElsX, E) for E, (P, e) in enumerate(where)])
    theta_l2_i = col(lambda P, ex, ey, E: P.diag_theta_L2(ex, ey, rho_i[E], rt_i[E]))
    theta_i = col(lambda P, ex, ey, E: P.diag_theta2(ex, ey, rho_i[E], rt_i[E]))
    theta_l2_h, theta_h = theta_l2_i.copy(), theta_i.copy()
    exner_h, velz_h, rho_h, rt_h = exner_i.copy(), velz_i.copy(), rho_i.copy(), rt_i.copy()
    for _ in range(nits):
        dFx, dGx = forcing(rho_i, rho_j, theta_l2_h) if forcing is not None else (None, None)
        for E, (P, e) in enumerate(where):
            ex, ey = e % P.nElsX, e // P.nElsX
            D = lambda op, **kw: P.colop_dense(op, ex, ey, **kw)
            F_w, F_z, G_z, ftc = assemble_residual_ec(P, ex, ey, dt, theta_l2_h[E], exner_h[E], velz_i[E], velz_j[E], rho_i[E], rho_j[E], zv[E], V10)
            F_exner = P.eos_residual(ex, ey, rt_j[E], exner_j[E])
            VB = D("CONST")
            dF_z = rho_j[E] + dt * (V10 @ F_z) - rho_i[E]
            dG_z = rt_j[E] + 0.5 * dt * (V10 @ G_z) - rt_i[E]
            F_rho = VB @ dF_z
            F_rt = VB @ dG_z
            if dFx is not None:
                F_rho = F_rho + dt * dFx[E]
                F_rt = F_rt + dt * dGx[E]
            F_rt = F_rt + ftc
            if hs_forcing:
                F_rt = F_rt + dt * P.temp_forcing_hs(ex, ey, exner_h[E], theta_h[E], rho_h[E])
            t1 = D("CONST_RHO_INV", f1=rt_h[E]) @ F_rt - D("CONST_RHO_INV", f1=rho_h[E]) @ F_rho
            F_eta = VB @ t1
            th_w3 = D("CONST_RHO_INV", f1=rho_h[E]) @ (VB @ rt_h[E])
            VBinv = D("CONST_INV")
            eta = VBinv @ P.const_log_theta_plus_eta(ex, ey, th_w3, None)
            sol = P.solve_schur_column_eta(ex, ey, dt, th_w3, rho_h[E], eta, exner_h[E], F_w, F_rho, F_eta, F_exner)
            th_w3 = D("CONST_RHO_INV", f1=rho_j[E]) @ (VB @ rt_j[E])
            eta = VBinv @ P.const_log_theta_plus_eta(ex, ey, th_w3, sol["d_eta"])
            velz_j[E] += sol["d_u"]; rho_j[E] += sol["d_rho"]; exner_j[E] += sol["d_pi"]
            rt_j[E] = VBinv @ P.const_rho_exp_eta(ex, ey, rho_j[E], eta)
            exner_h[E] = 0.5 * exner_i[E] + 0.5 * exner_j[E]; velz_h[E] = 0.5 * velz_i[E] + 0.5 * velz_j[E]
            rho_h[E] = 0.5 * rho_i[E] + 0.5 * rho_j[E]; rt_h[E] = 0.5 * rt_i[E] + 0.5 * rt_j[E]
        theta_h = 0.5 * col(lambda P, ex, ey, E: P.diag_theta2(ex, ey, rho_j[E], rt_j[E])) + 0.5 * theta_i
        theta_l2_h = 0.5 * col(lambda P, ex, ey, E: P.diag_theta_L2(ex, ey, rho_j[E], rt_j[E])) + 0.5 * theta_l2_i
    return (velz_j, rho_j, rt_j, exner_j), theta_l2_h, exner_h


class Restatement:
    """Euler::Strang_ec, stage by stage; carries first_step, u_prev / u_curr and uz / uz_prev between steps as the reference does"""

    def __init__(self, c, dt=DT, nits=NITS, hs_forcing=False):
        self.c, self.gd, self.dt, self.nits, self.hs_forcing = c, c["gd"], dt, nits, hs_forcing
        self.hz = c["ho"].HorizOracle(c["gd"])
        self.dense = DenseM1(c)
        self.first_step, self.u_prev, self.u_curr, self.uz, self.uz_prev = True, None, None, None, None

    def momentum_rhs(self, theta, dudz1, dudz2, velz1, velz2, Pi, velx1, velx2, rho1, rho2, Fz, dwdx1, dwdx2):
        return np.stack([self.hz.momentum_rhs_ec(k, theta[k], dudz1, dudz2, velz1, velz2, Pi[k], velx1[k], velx2[k], rho1[k], rho2[k],
                                                 Fz=Fz, dwdx1=dwdx1, dwdx2=dwdx2) for k in range(self.c["nk"])])

    def stage1(self, velx, velz_h0, rho, rt, exner):
        """:1399-1457 -> predictor velx; leaves Fu_1, dwdx1 and the carried vectors of this step"""
        gd = self.gd
        if not self.first_step:
            self.uz_prev = self.uz.copy()                                              # :1407-1409
        self.u_prev, self.u_curr = self.u_curr, velx.copy()                            # :1415-1416
        theta_0 = ec.theta_L2(self.c, rho, rt)                                          # :1421-1422
        self.uz = vc.horiz_pot_vort(gd, velx, rho)[0]                                   # :1423
        self.dwdx1 = vc.vert_vort(gd, velz_h0, rho)[0]                                  # :1424
        if self.first_step:
            self.uz_prev = self.uz.copy()                                              # :1425
        Fz = vc.vert_mass_flux(gd, velz_h0, velz_h0, rho, rho)                          # :1426
        self.Fu_1 = self.momentum_rhs(theta_0, self.uz, self.uz, velz_h0, velz_h0, exner, velx, velx, rho, rho, Fz, self.dwdx1, self.dwdx1)
        ex = exner if self.hs_forcing else None
        if self.first_step:
            return momentum_update(self.dense, self.hz.M1, self.dt, velx, self.Fu_1, 1.0, ex)          # :1433-1438
        return momentum_update(self.dense, self.hz.M1, self.dt, self.u_prev, self.Fu_1, 2.0, ex)       # :1440-1444 (leapfrog)

    def stage2(self, velx_0, velx_p, velz_v, rho, rt, exner):
        """:1461-1466 -> (velz, rho, rt, exner) of the new time level in the vertical layout; leaves theta_l2_h, exner_h (horizontal)"""
        c, nk = self.c, self.c["nk"]

        def forcing(rho_i, rho_j, theta_l2_h):
            dF, dG, self.Fk, _ = self.hz.advection_rhs_ec(velx_0, velx_p, rho, to_horiz(c, rho_j, nk), to_horiz(c, theta_l2_h, nk))
            return to_vert(c, dF), to_vert(c, dG)
        new, th, eh = newton(c, self.dt, velz_v, to_vert(c, rho), to_vert(c, rt), to_vert(c, exner), c["zv_v"], self.nits,
                             forcing=forcing, hs_forcing=self.hs_forcing)
        self.theta_l2_h, self.exner_h = to_horiz(c, th, nk), to_horiz(c, eh, nk)
        return new

    def stage3(self, velx_0, velx_p, velz_h0, velz_hn, rho_0, rho_n, exner_n):
        """:1470-1493 -> the corrected velx"""
        gd = self.gd
        self.uz = vc.horiz_pot_vort(gd, velx_p, rho_n)[0]                               # :1470
        dwdx2 = vc.vert_vort(gd, velz_hn, rho_n)[0]                                     # :1471
        Fz = vc.vert_mass_flux(gd, velz_h0, velz_hn, rho_0, rho_n)                      # :1472
        self.Fu_3 = self.momentum_rhs(self.theta_l2_h, self.uz, self.uz_prev, velz_hn, velz_h0, self.exner_h, velx_0, velx_p, rho_0, rho_n,
                                      Fz, self.dwdx1, dwdx2)
        # the horizontal kinetic-to-internal exchange of this evaluation (eul/HorizSolve.cpp:699-708) with Fk of the last transport evaluation:
        # k2i = sum_k Fk_k . dp_k / SCALE, dp_k = E12 M2h(Pi_k, vert) theta_k; beside it S_abs, the sum of the absolute entry-wise products
        self.k2i, self.k2i_abs = 0.0, 0.0
        for k in range(self.c["nk"]):
            dp = gd.E12 @ (gd.mat("WHMAT", k, 1, self.exner_h[k]) @ self.theta_l2_h[k])
            self.k2i += float(self.Fk[k] @ dp) / SCALE
            self.k2i_abs += float(np.abs(self.Fk[k] * dp).sum()) / SCALE
        return momentum_update(self.dense, self.hz.M1, self.dt, velx_0, self.Fu_3, 1.0, exner_n if self.hs_forcing else None)

    def step(self, velx, velz_v, rho, rt, exner):
        c, nk = self.c, self.c["nk"]
        velz_h0 = to_horiz(c, velz_v, nk - 1)
        self.velx_p = self.stage1(velx, velz_h0, rho, rt, exner)
        velz_n, rho_nv, rt_nv, exner_nv = self.stage2(velx, self.velx_p, velz_v, rho, rt, exner)
        rho_n, rt_n, exner_n = (to_horiz(c, a, nk) for a in (rho_nv, rt_nv, exner_nv))
        velx_n = self.stage3(velx, self.velx_p, velz_h0, to_horiz(c, velz_n, nk - 1), rho, rho_n, exner_n)
        self.first_step = False
        return velx_n, velz_n, rho_n, rt_n, exner_n


def energetics(c, state):
    """{name: (sum, S_abs)} of keh, ie, entr, mass, kev, k2p, p2k, pe of a state, by tests/energetics_case.py"""
    d = dict(c)
    d["velx"], d["velz_v"], d["rho"], d["rt"], d["exner"] = state
    d["rho_v"] = to_vert(c, d["rho"])
    out = ec.restate_horizontal(d)
    out.update(ec.restate_column(d))
    return out


def bernoulli_pointwise(P, t, lev, nk, u1, u2, velz1, velz2):
    """the point-wise form of HorizSolve::diagnose_Phi csrc/bernoulli.inc is written from, on one patch: with t = thickInv, d = det, J the
    Jacobian, Q the weight, (u_a, v_a) the local interpolants of velx_a, U_a = J (u_a, v_a) / d, s_a the local interpolant of the level's
    mean of the two neighbouring interfaces of velz_a,
        c_q = SCALE Q [t^2/6 (U1.U1 + U1.U2 + U2.U2) + t/(6 d^2) (s1^2 + s1 s2 + s2^2)],   Phi[e, j] = sum_q W[q][j] c_q.
    u1, u2: patch-local 1-form vectors of the level; velz1, velz2: [nk-1, n2] patch-local.  Returns the patch-local 2-form vector"""
    W, Q, iq, i2 = P.arr("W", (P.mp12, P.n2e)), P.arr("Q", (P.mp12,)), P.elinds("q"), P.elinds("n2")
    zb = []
    for vz in (velz1, velz2):
        z = np.zeros(P.n2)
        if lev > 0: z += 0.5 * vz[lev - 1]
        if lev < nk - 1: z += 0.5 * vz[lev]
        zb.append(z)
    out = np.zeros(P.n2)
    for e in range(P.nEl):
        ex, ey = e % P.nElsX, e // P.nElsX
        cq = np.zeros(P.mp12)
        for q in range(P.mp12):
            px, py = q % P.mp1, q // P.mp1
            J = np.array(P.J[e, q]).reshape(2, 2); d = P.det[e, q]; ti = P.thickInv[lev, iq[e, q]]
            U1 = J @ np.array(P.interp("1l", ex, ey, px, py, u1)) / d
            U2 = J @ np.array(P.interp("1l", ex, ey, px, py, u2)) / d
            s1, s2 = (P.interp("2g", ex, ey, px, py, z)[0] * d for z in zb)             # "2g" holds the 1/d: the local interpolant is s d
            cq[q] = SCALE * Q[q] * (ti * ti / 6.0 * (U1 @ U1 + U1 @ U2 + U2 @ U2) + ti / (6.0 * d * d) * (s1 * s1 + s1 * s2 + s2 * s2))
        out[i2[e]] = W.T @ cq
    return out
