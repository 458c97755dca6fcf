"""Host-side mirror of the reference's HorizSolve (eul/HorizSolve.cpp): the weak-form differential operators (grad, curl,
laplacian :208-283) and the right-hand sides of the horizontal dynamics (diagnose_fluxes :285-327, advection_rhs :330-375,
advection_rhs_ec :380-417, diagnose_Phi :419-470, diagnose_q :472-493, momentum_rhs :496-635, momentum_rhs_ec :637-786) composed from engine applies, incidence stencils and
the device mass solves -- EVERY LEVEL IN ONE CALL of each operator (the reference loops `for(kk...)` around per-level
assemble + MatMult + KSPSolve).  SURVEY 8(f) row N2.  Single GPU, global numbering (local == global vectors).

Field layout: horizontal, one row per level: 1-forms [nk, n1], 2-forms [nk, n2], 0-forms [nk, n0]; interface quantities
(velz, dudz, dwdx, Fz) [nk-1, .]."""
import math

import torch

from .krylov import MassSolver

SCALE = 1.0e8
OMEGA = 7.29212e-5             # eul/HorizSolve.cpp:23
RAD_EARTH = 6371220.0
VERT, ACCUM = 1, 2


class HorizSolve:
    def __init__(self, eng, del2=None, quad_coords=None, do_visc=True):
        self.eng, self.nk, self.do_visc = eng, eng.nk, do_visc
        if del2 is None:                                        # viscosity() :112-120, with the GLOBAL node count nDofs0G
            n0g = float(eng.wsum(0, torch.ones(eng.sizes[0], dtype=torch.float64, device=eng.device)))
            dx = math.sqrt(4.0 * math.pi * RAD_EARTH * RAD_EARTH / n0g)
            del2 = -math.sqrt(0.072 * dx ** 3.2)
        self.del2 = del2
        self.m1 = MassSolver(eng, SCALE, True)
        self.m0 = eng.pvec(0, eng.nk, SCALE)                  # M0 is diagonal for the collocated 0-forms (Pvec)
        self.fg = None
        self.k2i_dev = None
        self.fused_phi = False                                  # diagnose_Phi: True = the one-launch kernel (Engine.bernoulli), False = the eight composed launches
        self.fused_hu = False                                   # the mass-flux right-hand side of advection_rhs / momentum_rhs: True = Engine.flux_rhs
                                                                # (two launches), False = _uvec_hu4 (four accumulated applies); the _ec methods keep _uvec_hu4
        self.fused_forcing = False                              # the element-local sum of momentum_rhs (rotational term, pressure gradient force, second
                                                                # vorticity term): True = Engine.momentum_forcing (two launches), False = the composed applies
        if quad_coords is not None:
            self.coriolis(quad_coords)

    @property
    def k2i(self):
        """horizontal kinetic-to-internal energy exchange of the last momentum_rhs_ec (:697-701)"""
        return 0.0 if self.k2i_dev is None else float(self.k2i_dev)

    def verify(self):
        """every fixed-length 1-form mass solve since the last call met its check (MassSolver.verify: one read of a small device log); False:
        the solver has switched itself to PCG -- redo the evaluation"""
        return self.m1.verify()

    # ---- operators --------------------------------------------------------------------------------------------------
    def _ap(self, op, x, f=None, flags=0, alpha=1.0, out=None):
        return self.eng.apply(op, x, f=f, lev0=0, scale=SCALE, flags=flags, alpha=alpha, out=out)

    def coriolis(self, quad_coords):
        """:124-161: fg[k] = M0(k, scale 1)^-1 PtQ (2 Omega sin(lat))"""
        xq = torch.as_tensor(quad_coords, dtype=torch.float64, device=self.eng.device)
        fq = (2.0 * OMEGA * torch.sin(torch.asin(xq[:, 2] / RAD_EARTH))).unsqueeze(0)
        b = self.eng.apply("PTQ", fq)
        self.fg = b / self.eng.pvec(0, self.nk, 1.0)

    def grad(self, phi):
        """u = M1^-1 E12 M2 phi   (:208-228), phi: [nk, n2]"""
        rhs = self.eng.incidence("E12", self._ap("WMAT", phi, flags=VERT))
        u, self.last_its = self.m1.solve(rhs)
        return u

    def curl(self, u, fg=None):
        """w = M0^-1 E01 M1 u (+ f)   (:233-254), u: [nk, n1]"""
        t = self.eng.incidence("E01", self.m1.apply(u))
        return self.eng.combine(t, 1.0, "div", self.m0, beta=0.0 if fg is None else 1.0, c=fg, out=t)

    def laplacian(self, u):
        """del2 * (grad(E21 u) + E10 curl(u))   (:256-283)"""
        ddu = self.grad(self.eng.incidence("E21", u))
        return self.eng.combine(ddu, self.del2, beta=self.del2, c=self.eng.incidence("E10", self.curl(u)), out=ddu)

    def _uvec_hu4(self, ua, ub, ha, hb):
        """the four m1->assemble_hu(level, SCALE, u, h, false, fac) calls + gtol_1 reverse-add (:300-305, :675-682)"""
        hu = self._ap("UHMAT", ua, f=ha, flags=VERT, alpha=1.0 / 3.0)
        self._ap("UHMAT", ua, f=hb, flags=VERT | ACCUM, alpha=1.0 / 6.0, out=hu)
        self._ap("UHMAT", ub, f=ha, flags=VERT | ACCUM, alpha=1.0 / 6.0, out=hu)
        self._ap("UHMAT", ub, f=hb, flags=VERT | ACCUM, alpha=1.0 / 3.0, out=hu)
        return hu

    def _hu(self, ua, ub, ha, hb):
        """_uvec_hu4 as the two non-_ec right-hand sides form it: by the fused kernel when fused_hu is set"""
        if self.fused_hu:
            return self.eng.flux_rhs(ua, ub, ha, hb, scale=SCALE)
        return self._uvec_hu4(ua, ub, ha, hb)

    def _theta_levels(self, theta):
        """1/2 theta_k + 1/2 theta_{k+1} of theta on the nk+1 interfaces (:314-316, :515-517)"""
        return self.eng.combine(theta[:-1], 0.5, beta=0.5, c=theta[1:])

    # ---- fluxes and the transport right-hand side ---------------------------------------------------------------------
    def diagnose_fluxes(self, u1, u2, h1, h2, theta, theta_in_Wt=False):
        """:285-327: F = M1^-1 (hu), G = M1^-1 F(theta) F   -- all levels.  theta_in_Wt = false (the _ec callers): theta [nk, n2] in the
        levels, F(theta_k; vert_scale).  theta_in_Wt = true (advection_rhs): theta [nk+1, n2] on the interfaces,
        F(1/2 theta_k + 1/2 theta_{k+1}; no vert_scale) (:313-317), and the mass-flux right-hand side by fused_hu"""
        if not theta_in_Wt:
            F, _ = self.m1.solve(self._uvec_hu4(u1, u2, h1, h2))
            G, _ = self.m1.solve(self._ap("UHMAT", F, f=theta, flags=VERT))
            return F, G
        F, _ = self.m1.solve(self._hu(u1, u2, h1, h2))
        G, _ = self.m1.solve(self._ap("UHMAT", F, f=self._theta_levels(theta), flags=0))
        return F, G

    def advection_rhs(self, u1, u2, h1, h2, theta):
        """:330-375, theta [nk+1, n2] on the interfaces; returns dF = E21 Fk, dG = E21 Gk [nk, n2] in the horizontal layout (no M2 factor:
        VertSolve::solve_schur_2 applies VB after adding them) and Fk, Gk, which are kept in self.Fk, self.Gk.  The do_temp_visc branch
        (:341-364) is not built: the flag is false in the reference's constructor and no driver sets it"""
        Fk, Gk = self.diagnose_fluxes(u1, u2, h1, h2, theta, theta_in_Wt=True)
        dF, dG = self.eng.incidence("E21", Fk), self.eng.incidence("E21", Gk)
        self.Fk, self.Gk = Fk, Gk
        return dF, dG, Fk, Gk

    def advection_rhs_ec(self, u1, u2, h1, h2, theta):
        """:380-417 ; returns dF, dG in the horizontal layout (the caller's HorizToVert is mimsem_l2_transpose) and Fk, Gk"""
        eng = self.eng
        Fk, Gk = self.diagnose_fluxes(u1, u2, h1, h2, theta)
        dFk = eng.incidence("E21", Fk)
        dF = self._ap("WMAT", dFk, flags=VERT)
        # (sums of operator results are accumulated by the operator kernels themselves: MIMSEM_FLAG_ACCUM + alpha, no elementwise passes)
        dG = self._ap("WMAT", eng.incidence("E21", Gk), flags=VERT, alpha=0.5)
        self._ap("WHMAT", dFk, f=theta, flags=VERT | ACCUM, alpha=0.5, out=dG)
        self.dTheta = self.grad(theta)                                           # (kept: momentum_rhs_ec of the same stage needs the same gradient)
        self._ap("WTQUMAT", Fk, f=self.dTheta, flags=ACCUM, out=dG)             # K incl. its 0.5 factor
        self.Fk, self.Gk = Fk, Gk
        return dF, dG, Fk, Gk

    # ---- momentum right-hand side ---------------------------------------------------------------------------------------
    def _to_levels(self, a):
        """0.5*(interface k-1) + 0.5*(interface k) with the missing boundary interfaces left out (:451-459)"""
        return self.eng.interface_average(a, self.nk)

    def diagnose_Phi(self, u1, u2, velz1, velz2):
        """:419-470"""
        if self.fused_phi:
            return self.eng.bernoulli(u1, u2, velz1, velz2, scale=SCALE)
        Phi = self._ap("WTQUMAT", u1, f=u1, alpha=1.0 / 3.0)
        self._ap("WTQUMAT", u2, f=u1, flags=ACCUM, alpha=1.0 / 3.0, out=Phi)
        self._ap("WTQUMAT", u2, f=u2, flags=ACCUM, alpha=1.0 / 3.0, out=Phi)
        z1, z2 = self._to_levels(velz1), self._to_levels(velz2)
        self._ap("WHMAT", z1, f=z1, flags=ACCUM, alpha=1.0 / 6.0, out=Phi)
        self._ap("WHMAT", z2, f=z1, flags=ACCUM, alpha=1.0 / 6.0, out=Phi)
        self._ap("WHMAT", z2, f=z2, flags=ACCUM, alpha=1.0 / 6.0, out=Phi)
        return Phi

    def diagnose_q(self, rho, u):
        """:472-493: (M0h(rho)) q = E01 M1 u + M0 f ; M0h is diagonal"""
        eng = self.eng
        rhs = eng.incidence("E01", self.m1.apply(u))
        eng.combine(self.m0, 1.0, "mul", self.fg.expand_as(self.m0) if self.fg.shape != self.m0.shape else self.fg, beta=1.0, c=rhs, out=rhs)
        return eng.combine(rhs, 1.0, "div", eng.pvec(0, self.nk, SCALE, h2=rho), out=rhs)

    def momentum_rhs_ec(self, theta, dudz1, dudz2, velz1, velz2, Pi, velx1, velx2, rho1, rho2, Fx=None, Fz=None,
                        dwdx1=None, dwdx2=None, Fk=None, dTheta=None):
        """:637-786 for every level at once; returns fu [nk, n1]; self.k2i = the kinetic-to-internal exchange (needs Fk).
        dTheta (optional, like Fx): grad(theta) when the caller has it already -- advection_rhs_ec of the same stage solved the same system
        for the same theta (:403 and :659 in the reference, two KSPSolves with one answer); passing self.dTheta saves one of the seven
        1-form mass solves of a right-hand-side evaluation"""
        eng = self.eng
        Phi = self.diagnose_Phi(velx1, velx2, velz1, velz2)
        dPi = self.grad(Pi)
        if dTheta is None:
            dTheta = self.grad(theta)
        fu = eng.incidence("E12", Phi)
        uh = eng.combine(velx1, 0.5, beta=0.5, c=velx2)
        q = self.diagnose_q(eng.combine(rho1, 0.5, beta=0.5, c=rho2), uh)
        if Fx is None:
            Fx, _ = self.m1.solve(self._uvec_hu4(velx1, velx2, rho1, rho2))
        self._ap("ROTMAT", Fx, f=q, flags=ACCUM, out=fu)
        self._ap("UHMAT", dPi, f=theta, flags=VERT | ACCUM, alpha=0.5, out=fu)  # pressure gradient force
        self._ap("UHMAT", dTheta, f=Pi, flags=VERT | ACCUM, alpha=-0.5, out=fu)
        dp = eng.incidence("E12", self._ap("WHMAT", theta, f=Pi, flags=VERT))
        eng.combine(dp, 0.5, beta=1.0, c=fu, out=fu)
        if Fk is not None:
            self.k2i_dev = self.eng.wsum(1, eng.combine(Fk, 1.0, "mul", dp)) / SCALE   # stays on the device (no host sync: hipGraph-capturable)
        return self._vorticity_and_viscosity(fu, uh, dudz1, dudz2, velz1, velz2, Fz, dwdx1, dwdx2)

    def _vorticity_operands(self, dudz1, dudz2, velz1, velz2, Fz, dwdx1, dwdx2):
        """coefficient and input of the second vorticity term (:565-607): Rh is linear in its coefficient, so dudz_h - dwdx_h is one field"""
        eng = self.eng
        dz = eng.combine(dudz1, 0.5, beta=0.5, c=dudz2)
        if dwdx1 is not None:
            eng.combine(dwdx1, -0.5, beta=1.0, c=dz, out=dz)
            eng.combine(dwdx2, -0.5, beta=1.0, c=dz, out=dz)
        v = Fz if Fz is not None else eng.combine(velz1, 0.5, beta=0.5, c=velz2)
        return dz, v

    def _viscosity(self, fu, uh):
        """the biharmonic viscosity (:609-623, :754-768), added to fu"""
        if self.do_visc:
            self._ap("UMAT", self.laplacian(self.laplacian(uh)), flags=VERT | ACCUM, out=fu)
        return fu

    def _vorticity_and_viscosity(self, fu, uh, dudz1, dudz2, velz1, velz2, Fz, dwdx1, dwdx2):
        """the end both momentum right-hand sides share (:565-623, :710-768): the second vorticity term and the biharmonic viscosity, added to fu"""
        eng = self.eng
        # second vorticity term: interface i feeds levels i and i+1
        dz, v = self._vorticity_operands(dudz1, dudz2, velz1, velz2, Fz, dwdx1, dwdx2)
        t = eng.apply("UTQWMAT", v, f=dz, lev0=0, scale=SCALE)                  # UtQWmat::assemble(u1, scale): no thickness
        eng.combine(t, 0.5, beta=1.0, c=fu[1:], out=fu[1:])
        eng.combine(t, 0.5, beta=1.0, c=fu[:-1], out=fu[:-1])
        return self._viscosity(fu, uh)

    def _rotational_operands(self, velx1, velx2, uh, rho1, rho2, Fx):
        """(q, a) of the rotational term R(q) a (:519-554): the potential vorticity of the mean state and the mass flux, solved for when
        the caller has none"""
        q = self.diagnose_q(self.eng.combine(rho1, 0.5, beta=0.5, c=rho2), uh)
        if Fx is None:
            Fx, _ = self.m1.solve(self._hu(velx1, velx2, rho1, rho2))
        return q, Fx

    def momentum_rhs(self, theta, dudz1, dudz2, velz1, velz2, Pi, velx1, velx2, rho1, rho2, Fx=None, Fz=None, dwdx1=None, dwdx2=None, Fk=None):
        """:496-635 for every level at once: momentum_rhs_ec with theta [nk+1, n2] on the interfaces.  There is no grad(theta); the pressure
        gradient force is the single term fu += F(theta_h; no vert_scale) dPi, theta_h = 1/2 theta_k + 1/2 theta_{k+1} (:514-517, :556-558),
        and self.k2i = sum_k Fk_k . (F(theta_h) dPi)_k / SCALE (:560-563, needs Fk).  The mass flux of the rotational term (Fx None) is
        formed by fused_hu.  With fused_forcing the rotational term, the pressure gradient force and the second vorticity term are one
        Engine.momentum_forcing call; dp for k2i then keeps its own Uhmat apply.  Returns fu [nk, n1]"""
        eng = self.eng
        Phi = self.diagnose_Phi(velx1, velx2, velz1, velz2)
        dPi = self.grad(Pi)
        fu = eng.incidence("E12", Phi)
        uh = eng.combine(velx1, 0.5, beta=0.5, c=velx2)
        q, a = self._rotational_operands(velx1, velx2, uh, rho1, rho2, Fx)
        theta_h = self._theta_levels(theta)
        if self.fused_forcing:
            eng.momentum_forcing(rot=(q, a), pgf=(theta_h, dPi), vor=self._vorticity_operands(dudz1, dudz2, velz1, velz2, Fz, dwdx1, dwdx2),
                                 scale=SCALE, flags=ACCUM, out=fu)
            if Fk is not None:
                dp = self._ap("UHMAT", dPi, f=theta_h, flags=0)
                self.k2i_dev = self.eng.wsum(1, eng.combine(Fk, 1.0, "mul", dp)) / SCALE
            return self._viscosity(fu, uh)
        self._ap("ROTMAT", a, f=q, flags=ACCUM, out=fu)
        dp = self._ap("UHMAT", dPi, f=theta_h, flags=0)                          # pressure gradient force
        eng.combine(dp, 1.0, beta=1.0, c=fu, out=fu)
        if Fk is not None:
            self.k2i_dev = self.eng.wsum(1, eng.combine(Fk, 1.0, "mul", dp)) / SCALE   # stays on the device (no host sync)
        return self._vorticity_and_viscosity(fu, uh, dudz1, dudz2, velz1, velz2, Fz, dwdx1, dwdx2)


LX = 1000.0                    # box/HorizSolve.cpp:22


def uniform_thickness(thick, rtol=1e-14):
    """the one layer thickness of a mesh whose layers all have it (thick: any array of thicknesses, e.g. DeviceMesh.thick), to rtol
    relative; ValueError otherwise"""
    import numpy as np
    thick = np.asarray(thick, dtype=np.float64)
    lo, hi = float(thick.min()), float(thick.max())
    if not (lo > 0.0 and hi - lo <= rtol * hi):
        raise ValueError("BoxHorizSolve: uniform layers only -- the thickness ranges from %.17g to %.17g" % (lo, hi))
    return hi


class BoxHorizSolve(HorizSolve):
    """HorizSolve of the doubly periodic box (box/HorizSolve.cpp).  What differs from the sphere's class:

      viscosity()      :106-114: del2 = -sqrt(2 * 0.072 dx^3.2), dx = sqrt(LX^2 / nDofs0G)
      rotational term  diagnose_wxu :382-410: R(1/2 curl u1 + 1/2 curl u2; level) (1/2 u1 + 1/2 u2), curl = M0^-1 E01 M1 u without a Coriolis
                       term -- no diagnose_q, no mass-flux solve.  curl is linear: one curl of the mean velocity
      momentum_rhs     :412-526: E12 Phi + wxu + F(theta_h; no const_vert) dPi + the Rh terms + M1 del^4, through HorizSolve.momentum_rhs with
                       the rotational operands above; the Rh coefficient is dudz_h - dwdx_h by linearity (_vorticity_operands); k2i as there
      advection_rhs    :214-324: the sphere's theta_in_Wt branch, inherited; do_temp_visc (:285-310) is not built, its only caller
                       (box/VertSolve.cpp:1333) passes false

    UNIFORM LAYERS ONLY.  The reference assembles M1->M, M2->M and m0 once, at level 0 (box/Assembly.cpp:44), and applies them at every
    level; on layers of one thickness they are the level-k operators the solvers of the base class apply.  Every box/ driver has such layers
    (z_at_level = ki ZTOP / NK); the constructor raises on any other mesh.

    A defect of the reference that is NOT mirrored: the box diagnose_Phi (:326-380) takes its kinetic-energy part from Wvec::assemble_K, whose
    Wt table is allocated zeroed and never filled (box/Assembly.cpp:2994-3005), so that part is zero in the reference as written.  Built is
    the evident intent, the commented-out K->assemble form at :336-349 -- the sphere's diagnose_Phi, inherited.  The _ec routines have no
    box twin"""

    def __init__(self, eng, lx=LX, del2=None, do_visc=True):
        self.thickness = uniform_thickness(eng.mesh.thick)
        self.lx = lx
        if del2 is None:
            n0g = float(eng.wsum(0, torch.ones(eng.sizes[0], dtype=torch.float64, device=eng.device)))
            del2 = self.viscosity(lx, n0g)
        super().__init__(eng, del2=del2, quad_coords=None, do_visc=do_visc)

    @staticmethod
    def viscosity(lx, n0g):
        """:106-114 with the GLOBAL node count nDofs0G"""
        dx = math.sqrt(lx * lx / n0g)
        return -math.sqrt(2.0 * 0.072 * dx ** 3.2)

    def _rotational_operands(self, velx1, velx2, uh, rho1, rho2, Fx):
        """diagnose_wxu :382-410: the relative vorticity of the mean velocity and the mean velocity itself"""
        return self.curl(uh), uh

    def _no_box_twin(self, *a, **kw):
        raise NotImplementedError("BoxHorizSolve: box/HorizSolve.cpp has no such routine")

    coriolis = diagnose_q = momentum_rhs_ec = advection_rhs_ec = _no_box_twin
