"""Thermal shallow water: the energy-conserving SSP-RK3 step of (u, h, S) on the device -- the host-side mirror of the reference's
ThermalSW_EEC_2 (src/ThermalSW_EEC_2.cpp, DO_THERMAL), the model the reference's src/ builds today (GalewskyTSW_2).  S is the
depth-integrated buoyancy, s = M2h(h)^-1 M2 S the buoyancy.

src flavour, one GPU, global numbering (the reference's local and global vectors coincide): an Engine with nk = 1 and unit thickness,
as SWEqn is built.  Per stage (solve_rk, :859-1004):
  k_tsw_diagnose     s, Phi = K(u) u + 1/2 M2 S + 1/4 M2h(s) h, h2 = M2^-1 M2h(h) h     (element-local, one launch)
  five M1 solves     F = M1^-1 M1h(h) u, grad h, grad s, G = M1^-1 M1h(s) F, the u update  (MassSolver: fixed-length block Chebyshev)
  one M1h(h) solve   d = M1h(h)^-1 E12 M2 s                                            (PCG on the element blocks of M1h(h))
  fu                 E12 Phi + R(q) F + 1/4 M1h(s) grad h - 1/2 K(d)^T h2               (accumulating applies)
  k_tsw_update       div F, fS, the new h and S                                        (element-local, one launch)
The reference's M1h and K are STATEFUL: diagnose_ds (:253-268) leaves K(d) and M1h(s) assembled, and rhs_u uses those.
fused=False composes the same stage from the engine's existing applies (no new kernel): the device-side cross-check of the two kernels."""
import math

import numpy as np
import torch

from .checks import CheckLog, accepted, log_true_residual
from .geom import gll_weights
from .krylov import MassSolver, edge_sharing_weights, element_block_preconditioner, pcg_engine
from .sweqn import RAD_SPHERE, galewsky

RK3 = ((0.0, 1.0), (0.75, 0.25), (1.0 / 3.0, 2.0 / 3.0))      # (alpha, beta) of the three stages, :894-1000
FLAG_ACCUM = 2


def galewsky_tsw(xq):
    """src/GalewskyTSW_2.cpp:20-89 at points xq [n, 3] (torch): (u [n, 2], h [n], s [n]) -- the Galewsky jet and depth of sweqn.galewsky and
    the buoyancy s_init with the same localised perturbation"""
    u, h = galewsky(xq)
    phi = torch.asin(xq[:, 2] / RAD_SPHERE)
    lam = torch.atan2(xq[:, 1], xq[:, 0])
    alpha, beta, phi2 = 1.0 / 3.0, 1.0 / 15.0, math.pi / 4.0
    s = 9.80616 - 0.1 * 9.80616 * torch.cos(phi) * torch.exp(-1.0 * (lam / alpha) ** 2) * torch.exp(-1.0 * ((phi2 - phi) / beta) ** 2)
    return u, h, s


class ThermalSW:
    def __init__(self, eng, quad_coords, rtol=1e-14, fused=True):
        """eng: Engine over the whole sphere (numbering="global", nk=1, unit thickness); quad_coords: [nq, 3] xyz of the quadrature-point
        grid in the engine's quad-grid numbering; fused: the stage's 2-form half in the two mimsem_tsw_* launches (False: composed from
        the existing applies)"""
        if eng.nk != 1:
            raise ValueError("ThermalSW needs an engine with nk = 1")
        self.eng, self.rtol, self.fused = eng, rtol, fused
        self.omega = 7.292e-5                                                     # :38
        self.n0, self.n1, self.n2 = eng.sizes[0], eng.sizes[1], eng.sizes[2]
        xq = torch.as_tensor(quad_coords, dtype=torch.float64, device=eng.device)
        lat = torch.asin(xq[:, 2] / RAD_SPHERE)
        self.m0 = eng.pvec(0, 1, 1.0)                                             # M0 is diagonal (collocated 0-forms)
        self.m2inv = eng.element_matrices("WMATINV")                              # M2_e^-1, [nEl, n2e^2]: M2 is element-block diagonal
        self.fg = eng.apply("PTQ", (2.0 * self.omega * torch.sin(lat)).unsqueeze(0)) / self.m0      # coriolis() :166-212
        self.m0fg = self.m0 * self.fg
        self.mass = MassSolver(eng, scale=1.0, vert_scale=False)                  # ksp (M1, PCBJACOBI): fixed-length block Chebyshev
        self.ones2 = eng.apply("WTQ", torch.ones(1, eng.sizes["q"], dtype=torch.float64, device=eng.device))   # int2(h) = h . WtQ 1
        n = eng.mesh.n
        w = gll_weights(n)
        self.Qw = torch.as_tensor(np.outer(w, w).reshape(-1), device=eng.device)      # point q = qy (n+1) + qx
        self.det = torch.as_tensor(eng.mesh.det, device=eng.device)
        self._d1 = edge_sharing_weights(eng)
        if not torch.all(torch.as_tensor(eng.mesh.thickInv) == 1.0):
            raise ValueError("ThermalSW needs unit thickness (the src flavour: levels 0 and 1)")
        self.m1h_its = 16                   # fixed length of the M1h(h) PCG (12 reach rtol 1e-14 on the Galewsky state at ne 2 ... 24)
        self._log1h = torch.zeros(1, dtype=torch.float64, device=eng.device)        # worst |b - M1h x|^2 / |b|^2 of the step's stages, read with the step's check
        self.steps = 0
        self.redone = 0                     # steps redone by the adaptive solvers after a missed check
        self.its = {}

    # ---- operators (src flavour: scale 1, flags 0); vectors are [1, n] rows ----------------------------------------------------
    def M1(self, u): return self.eng.apply("UMAT", u)
    def M2(self, h): return self.eng.apply("WMAT", h)
    def E(self, name, x): return self.eng.incidence(name, x)
    def M2inv(self, x): return self.eng.blocks_apply(2, self.m2inv.view(self.eng.nEl, self.eng.n2e, self.eng.n2e), x)

    def solve_M1(self, b):
        """KSPSolve(ksp, b, x) on M1: the fixed-length solve, its check logged on the device (MassSolver.verify after the step)"""
        x, its = self.mass.solve(b, rtol=self.rtol)
        self.its["M1"] = its
        return x

    def solve_M1h(self, h, b):
        """KSPSolve(ksp1h, b, d) on M1h(h) (diagnose_ds :253-268): PCG preconditioned by the inverted element blocks of M1h(h), weighted by
        1/(elements sharing the edge) -- h changes every stage, so the blocks are rebuilt per solve.  A FIXED number of iterations (no host
        synchronisation); the true residual is logged on the device and read with the step's single check (solve_rk).  After a missed
        check: the adaptive PCG to rtol."""
        eng = self.eng
        P = element_block_preconditioner(eng, eng.element_matrices("UHMAT", f=h[0]), self._d1)
        A = lambda v: eng.apply("UHMAT", v, f=h)
        pre = lambda r: eng.blocks_apply(1, P, r, transpose=True)
        if self.m1h_its > 0:
            x, its = pcg_engine(eng, A, b, pre, fixed_its=self.m1h_its)
            log_true_residual(eng, A, x, b, self._log1h)
        else:
            x, its = pcg_engine(eng, A, b, pre, rtol=self.rtol, maxit=1000, check_every=4)
        self.its["M1h"] = its
        return x

    def check(self):
        """the step's ONE read: MassSolver's log of the fixed-length M1 solves and the M1h residuals, in one transfer.  False: a solve
        missed its tolerance -- the mass solver has switched to PCG and the M1h solve to the adaptive PCG; the caller redoes the step"""
        ratio, ml = CheckLog.read(self._log1h, self.mass.check_log)
        self._log1h.zero_()
        ok1h = bool(accepted(ratio, 1.0, 30.0 * self.rtol)[0].all())
        okm = self.mass.verify(self.rtol, host=ml)
        if not ok1h:
            self.m1h_its = 0
        return ok1h and okm

    def grad(self, phi):
        return self.solve_M1(self.E("E12", self.M2(phi)))                       # :154-164

    def q(self, u, h):
        """diagnose_q (:227-239): M0h(h) q = E01 M1 u + M0 f; Phmat is diagonal at GLL collocation"""
        return (self.m0fg + self.E("E01", self.M1(u))) / self.eng.pvec(0, 1, 1.0, h2=h)

    # ---- the 2-form half of a stage ---------------------------------------------------------------------------------------------
    def diagnose(self, h, S, u):
        """(s, Phi, h2) of a stage: diagnose_s (:241-251), diagnose_Phi (:1019-1043), h2 of rhs_u (:1078-1080)"""
        eng = self.eng
        if self.fused:
            s, Phi, h2 = eng.tsw_diagnose(h[0], S[0], u[0], self.m2inv)
            return s.unsqueeze(0), Phi.unsqueeze(0), h2.unsqueeze(0)
        M2S = self.M2(S)
        s = eng.apply("WHMATINV", M2S, f=h)                                      # element-exact M2h(h)^-1
        Phi = eng.apply("WTQUMAT", u, f=u)                                       # K(u) u, the 1/2 inside
        Phi.add_(M2S, alpha=0.5)
        eng.apply("WHMAT", h, f=s, alpha=0.25, flags=FLAG_ACCUM, out=Phi)
        h2 = self.M2inv(eng.apply("WHMAT", h, f=h))
        return s, Phi, h2

    def update(self, F, G, gs, s, hi, Si, hj, Sj, dt, alpha, beta):
        """h_j, S_j <- the stage's h and S updates in place (:894-1000, rhs_S :1095-1120)"""
        eng = self.eng
        if self.fused:
            eng.tsw_update(F[0], G[0], gs[0], s[0], self.m2inv, hi[0], Si[0], hj[0], Sj[0], alpha, beta, dt)
            return
        divF = self.E("E21", F)
        fS = self.M2(self.E("E21", G)).mul_(0.5)
        eng.apply("WHMAT", divF, f=s, alpha=0.5, flags=FLAG_ACCUM, out=fS)
        eng.apply("WTQUMAT", F, f=gs, alpha=1.0, flags=FLAG_ACCUM, out=fS)
        hj.copy_(alpha * hi + beta * (hj - dt * divF))
        Sj.copy_(alpha * Si + beta * Sj - (beta * dt) * self.M2inv(fS))

    def stage(self, ui, hi, Si, uj, hj, Sj, dt, alpha, beta):
        """one stage from (uj, hj, Sj); returns the new uj, updates hj and Sj in place"""
        eng = self.eng
        s, Phi, h2 = self.diagnose(hj, Sj, uj)
        F = self.solve_M1(eng.apply("UHMAT", uj, f=hj))                                  # diagnose_F
        d = self.solve_M1h(hj, self.E("E12", self.M2(s)))                                # diagnose_ds: then K <- K(d), M1h <- M1h(s)
        G = self.solve_M1(eng.apply("UHMAT", F, f=s))                                    # diagnose_G
        gh, gs = self.grad(hj), self.grad(s)
        fu = self.E("E12", Phi)                                                           # rhs_u :1045-1093
        eng.apply("ROTMAT", F, f=self.q(uj, hj), flags=FLAG_ACCUM, out=fu)
        eng.apply("UHMAT", gh, f=s, alpha=0.25, flags=FLAG_ACCUM, out=fu)                 # 1/4 M1h(s) grad h
        eng.apply("UTQWMAT", h2, f=d, alpha=-0.25, flags=FLAG_ACCUM, out=fu)              # -1/2 K(d)^T h2 = -1/4 UtQWmat(d) h2
        unew = self.solve_M1(self.M1(alpha * ui + beta * uj) - (beta * dt) * fu)
        self.update(F, G, gs, s, hi, Si, hj, Sj, dt, alpha, beta)
        return unew

    def solve_rk(self, u, h, S, dt):
        """ThermalSW_EEC_2::solve_rk(dt) (:859-1004): the new (u, h, S) from [1, n] rows.  The checks of every fixed-length M1 solve of the
        step (15, within MassSolver's 16-slot log) and of its three M1h solves are read once at its end (check()); a missed check redoes
        the step with the adaptive solvers."""
        for attempt in range(2):
            uj, hj, Sj = u.clone(), h.clone(), S.clone()
            for alpha, beta in RK3:
                uj = self.stage(u, h, S, uj, hj, Sj, dt, alpha, beta)
            if self.check():
                break
            self.redone += 1                                                              # (check() switched to the adaptive solvers)
        self.steps += 1
        return uj, hj, Sj

    # ---- initial state and invariants -------------------------------------------------------------------------------------------
    def init(self, uq, hq, sq):
        """GalewskyTSW_2 main (src/GalewskyTSW_2.cpp:118-126): u = M1^-1 UtQ uq, h = M2^-1 WtQ hq, s likewise, S = M2^-1 M2h(h) s"""
        eng = self.eng
        b = eng.apply("UTQ", uq.reshape(1, -1).contiguous())
        u = self.solve_M1(b)
        if not self.mass.verify(self.rtol):
            u = self.solve_M1(b)                                                          # (verify() switched the mass solver to PCG)
        h = self.M2inv(eng.apply("WTQ", hq.reshape(1, -1).contiguous()))
        s = self.M2inv(eng.apply("WTQ", sq.reshape(1, -1).contiguous()))
        S = self.M2inv(eng.apply("WHMAT", s, f=h))
        return u, h, S

    def invariants(self, u, h, S):
        """writeConservation (:765-858): mass int2(h), buoyancy int2(S), energy intE(u, h, S), enstrophy q^T M0h q, vorticity sum M0 w,
        entropy 1/2 (M2 M2h(h)^-1 M2 S) . S"""
        eng = self.eng
        m0h = eng.pvec(0, 1, 1.0, h2=h)
        q = (self.m0fg + self.E("E01", self.M1(u))) / m0h
        hq, Sq = eng.interp_quad(2, h[0]), eng.interp_quad(2, S[0])                     # interp2_g (/ det)
        uq = eng.interp_quad(1, u[0])                                                    # interp1_g (J / det)
        wd = self.det * self.Qw[None, :]
        ener = (wd * 0.5 * (Sq * hq + hq * (uq[..., 0] ** 2 + uq[..., 1] ** 2))).sum()
        ent = (self.M2(eng.apply("WHMATINV", self.M2(S), f=h)) * S).sum() * 0.5
        vals = torch.stack([(h * self.ones2).sum(), (S * self.ones2).sum(), ener, (q * m0h * q).sum(), self.E("E01", self.M1(u)).sum(), ent])
        v = vals.cpu().numpy()
        return dict(mass=float(v[0]), buoyancy=float(v[1]), energy=float(v[2]), enstrophy=float(v[3]), vorticity=float(v[4]), entropy=float(v[5]))
