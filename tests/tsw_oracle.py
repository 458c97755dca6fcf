"""CPU restatement of the reference's thermal shallow-water step, ThermalSW_EEC_2::solve_rk (src/ThermalSW_EEC_2.cpp:859-1004, DO_THERMAL
defined at :25) and everything it calls -- TEST INFRASTRUCTURE ONLY, built on the shallow-water oracle (oracle/sw_oracle.py): the same
global matrices (dense numpy, or scipy.sparse with sparse=True), every KSPSolve a direct solve.

The step keeps the reference's STATEFUL matrices: diagnose_ds (:253-268) re-assembles K with d = M1h(h)^-1 E12 M2 s and M1h with s, and
rhs_u (:1045-1093) uses those (K(d)^T, M1h(s)), not K(u) and M1h(h).  src flavour: unit thickness, signed Jacobian determinant."""
import math

import numpy as np

from oracle import pyoracle
from oracle.globalmat import GlobalMat
from oracle.sw_oracle import RAD_SPHERE, SWOracle

RK3 = ((0.0, 1.0), (0.75, 0.25), (1.0 / 3.0, 2.0 / 3.0))      # (alpha, beta) of the three stages, :894-1000


def s_init(xq):
    """src/GalewskyTSW_2.cpp:77-89 at points xq [n, 3]: the buoyancy with the localised perturbation of the Galewsky depth"""
    phi = np.arcsin(xq[:, 2] / RAD_SPHERE)
    lam = np.arctan2(xq[:, 1], xq[:, 0])
    alpha, beta, phi2 = 1.0 / 3.0, 1.0 / 15.0, math.pi / 4.0
    return 9.80616 - 0.1 * 9.80616 * np.cos(phi) * np.exp(-1.0 * (lam / alpha) ** 2) * np.exp(-1.0 * ((phi2 - phi) / beta) ** 2)


class TSWOracle(SWOracle):
    def __init__(self, sphere, topos, geoms, coords, sparse=False):
        super().__init__(sphere, topos, geoms, coords, sparse=sparse)
        n = self.P[0].n
        self.tab = pyoracle.tables(n, n)
        self.ones2 = self.project(0, np.ones(self.NQ))        # int2(h) = sum_e sum_q w_q det_q interp2_g(h) = h . (WtQ 1): det cancels
        self.steps = 0

    # ---- matrices the thermal step adds -------------------------------------------------------------------------------------
    def M2h(self, fg):
        """Whmat::assemble(f)  src/Assembly.cpp:1558-1605 (interp2_g divides by det: Qaa = f(x_q)/det w_q)"""
        M = GlobalMat((self.N2, self.N2), self.sparse)
        for t, P in zip(self.topos, self.P):
            g2 = t.all_inds2_g()
            em = P.op_elmats("WHMAT", 0, 1.0, 0, self._local2(t, fg)).reshape(P.nEl, P.n2e, P.n2e)
            M.add(g2, g2, em)
        return M.done()

    def grad(self, phi):
        return self._solve(self.M1, self.E12M2 @ phi, "M1")                          # :154-164

    def diagnose_q(self, u, h):
        return self._solve(self.M0h(h), self.E01M1 @ u + self.M0 @ self.fg)         # :227-239

    # ---- one stage -----------------------------------------------------------------------------------------------------------
    def diagnose(self, u, h, S):
        """diagnose_s, diagnose_F, diagnose_Phi, diagnose_ds, diagnose_G of one stage (:241-284, :1005-1043) and the pieces of rhs_u"""
        d = {}
        M2h_h = self.M2h(h)
        d["s"] = s = self._solve(M2h_h, self.M2 @ S)                                  # diagnose_s
        M1h_h = self.M1h(h)
        d["F"] = F = self._solve(self.M1, M1h_h @ u, "M1")                            # diagnose_F
        d["Phi"] = self.K(u) @ u + 0.5 * (self.M2 @ S) + 0.25 * (self.M2h(s) @ h)     # diagnose_Phi (the 1/2 of K(u) u inside WtQUmat)
        d["d"] = ds = self._solve(M1h_h, self.E12M2 @ s)                             # diagnose_ds: ksp1h on M1h(h) ...
        K_d, M1h_s = self.K(ds), self.M1h(s)                                         # ... then K <- K(d), M1h <- M1h(s)
        d["G"] = self._solve(self.M1, M1h_s @ F, "M1")                               # diagnose_G
        d["h2"] = h2 = self._solve(self.M2, M2h_h @ h, "M2")                          # rhs_u :1078-1080
        q = self.diagnose_q(u, h)
        d["fu"] = (self.E12 @ d["Phi"] + self.R(q) @ F + 0.25 * (M1h_s @ self.grad(h)) - 0.5 * (K_d.T @ h2))     # rhs_u :1045-1093
        d["grad_s"] = gs = self.grad(s)
        d["fS"] = (0.5 * (self.M2 @ (self.E21 @ d["G"])) + 0.5 * (self.M2h(s) @ (self.E21 @ F))                  # rhs_S :1095-1120
                   + self.K(gs) @ F)
        return d

    def update(self, d, ui, hi, Si, uj, hj, Sj, dt, alpha, beta):
        """the u, h and S updates of a stage with coefficients (alpha, beta) (:894-1000)"""
        u = self._solve(self.M1, self.M1 @ (alpha * ui + beta * uj) - (beta * dt) * d["fu"], "M1")
        h = alpha * hi + beta * (hj - dt * (self.E21 @ d["F"]))
        S = self._solve(self.M2, self.M2 @ (alpha * Si + beta * Sj) - (beta * dt) * d["fS"], "M2")
        return u, h, S

    def solve_rk(self, u, h, S, dt):
        """ThermalSW_EEC_2::solve_rk(dt) (:859-1004): three stages from (u, h, S); returns the new state"""
        uj, hj, Sj = u.copy(), h.copy(), S.copy()
        for alpha, beta in RK3:
            d = self.diagnose(uj, hj, Sj)
            uj, hj, Sj = self.update(d, u, h, S, uj, hj, Sj, dt, alpha, beta)
        self.steps += 1
        return uj, hj, Sj

    # ---- initial state and invariants ----------------------------------------------------------------------------------------
    def initial_state(self, uq, hq, sq):
        """GalewskyTSW_2 main (src/GalewskyTSW_2.cpp:118-126): u, h, s projected; S = M2^-1 M2h(h) s"""
        u, h, s = self.init1(uq), self.init2(hq), self.init2(sq)
        return u, h, self._solve(self.M2, self.M2h(h) @ s, "M2")

    def _energy(self, u, h, S):
        """intE (:726-763): sum over elements and points of det w 1/2 (S h + h |u|^2), interp1_g / interp2_g at every point"""
        W, U, V, Q = self.tab["W"], self.tab["U"], self.tab["V"], self.tab["Q"]
        tot = 0.0
        for t, P in zip(self.topos, self.P):
            ul, hl, Sl = self._local1(t, u), self._local2(t, h), self._local2(t, S)
            i1x, i1y, i2 = P.elinds("n1x"), P.elinds("n1y"), P.elinds("n2")
            det, J = P.det, P.J
            hq = (hl[i2] @ W.T) / det
            Sq = (Sl[i2] @ W.T) / det
            a, b = ul[i1x] @ U.T, ul[i1y] @ V.T
            ux = (J[..., 0] * a + J[..., 1] * b) / det
            uy = (J[..., 2] * a + J[..., 3] * b) / det
            tot += float((det * Q[None, :] * 0.5 * (Sq * hq + hq * (ux * ux + uy * uy))).sum())
        return tot

    def invariants(self, u, h, S):
        """writeConservation (:765-858): mass int2(h), buoyancy int2(S), energy intE, enstrophy q^T M0h(h) q, vorticity sum M0 w,
        entropy 1/2 (M2 M2h(h)^-1 M2 S) . S"""
        q = self.diagnose_q(u, h)
        w = self._solve(self.M0, self.E01M1 @ u, "M0")
        e = self.M2 @ self._solve(self.M2h(h), self.M2 @ S)
        return dict(mass=float(h @ self.ones2), buoyancy=float(S @ self.ones2), energy=self._energy(u, h, S),
                    enstrophy=float(q @ (self.M0h(h) @ q)), vorticity=float((self.M0 @ w).sum()), entropy=0.5 * float(e @ S))
