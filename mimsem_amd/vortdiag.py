"""The three interface-level diagnoses Euler::Strang_ec runs before each horizontal momentum solve (eul/Euler_2.cpp:1423-1426, :1470-1472)
-- the producers of HorizSolve.momentum_rhs_ec's dudz, dwdx and Fz -- for all nk - 1 interfaces at once:

  horiz_pot_vort   Euler::HorizPotVort (eul/Euler_2.cpp:1051-1101)      uz_i   = M1t_h(rho_i)^-1 (M1_{i+1} velx_{i+1} - M1_i velx_i)
  vert_vort        HorizSolve::diagVertVort (eul/HorizSolve.cpp:823-861)  dwdx_i = F(rho_i, level 0)^-1 E12 M2(level 0) velz_i
  vert_mass_flux   Euler::VertMassFlux (eul/Euler_2.cpp:1559-1572)       Fz     = VertToHoriz diagnose_F_z HorizToVert

with rho_i = 1/2 rho_i + 1/2 rho_{i+1}.  The reference assembles M2 and F of diagVertVort at level 0 for EVERY interface; that is kept
(Engine.apply_levels / elem_block_pc_levels with level step 0).  Both solves are 1-form mass solves whose matrix changes with the density
on every call: the element-block preconditioner of all interfaces is rebuilt in one launch (mimsem_elem_block_pc_build_levels) and one
batched PCG runs over the interfaces.

The solves follow ThermalSW.solve_M1h: a FIXED number of iterations without host synchronisation, the true residual of every interface
logged on the device, one check() reading the log; after a miss the solves run the adaptive PCG to rtol.  The first solve of each kind
runs adaptively to find its count.  Single GPU, global numbering; vectors as in HorizSolve ([nk, n] levels, [nk - 1, n] interfaces)."""
import torch

from .checks import CheckLog, accepted, log_true_residual
from .horizsolve import SCALE, VERT
from .krylov import pcg_engine

MARGIN = 2        # iterations added to the count the adaptive solve needed (its convergence test runs every second iteration)


class VortDiag:
    def __init__(self, eng, horiz, vert=None, rtol=1e-14):
        """eng: Engine with nk >= 2 levels; horiz: the HorizSolve whose momentum_rhs_ec takes the results; vert: the VertSolve of
        vert_mass_flux (made on first use when None)"""
        if horiz.eng is not eng:
            raise ValueError("VortDiag: horiz belongs to another engine")
        if eng.nk < 2:
            raise ValueError("VortDiag needs at least one interface (nk >= 2)")
        self.eng, self.horiz, self.vert, self.rtol = eng, horiz, vert, rtol
        self.nk, self.ni = eng.nk, eng.nk - 1
        self._its = {"uz": None, "dwdx": None}          # fixed PCG length per solve: None = find it adaptively, 0 = adaptive from now on
        # worst |b - A x|^2 / |b|^2 per interface since check(): rows uz, dwdx and the unit-thickness mass solve of vert_mom_vort
        self._log = torch.zeros(3, self.ni, dtype=torch.float64, device=eng.device)
        self.its = {}                                   # iterations of the last solve of each kind
        self.fixed_its = {}                             # the fixed_its its PCG was launched with (0: adaptive)
        self.logged = 0
        self.missed = 0
        self.unit_mass = None                           # vert_mom_vort's mass solver without thickness (made on first use)

    @property
    def m_its(self):
        """the fixed PCG length (the larger of the two solves'; None before the first solve, 0 once adaptive); setting it sets both"""
        v = list(self._its.values())
        return None if None in v else max(v)

    @m_its.setter
    def m_its(self, n):
        self._its = {k: n for k in self._its}

    def rho_bar(self, rho):
        """rho_h of the interfaces: VecAXPY(rho_h, 0.5, rho[i]); VecAXPY(rho_h, 0.5, rho[i+1]) on a zeroed vector"""
        return self.eng.combine(rho[:-1], 0.5, beta=0.5, c=rho[1:])

    def _solve(self, kind, A, b, P):
        eng = self.eng
        pre = lambda r: eng.blocks_apply(1, P, r, transpose=True)
        m = self._its[kind]
        if m:
            x, its = pcg_engine(eng, A, b, pre, fixed_its=m)
            log_true_residual(eng, A, x, b, self._log[0 if kind == "uz" else 1])      # (NaN propagates: a miss)
            self.logged += 1
        else:
            x, its = pcg_engine(eng, A, b, pre, rtol=self.rtol, maxit=1000, check_every=2)
            if m is None:
                self._its[kind] = its + MARGIN
        self.its[kind], self.fixed_its[kind] = its, m or 0
        return x

    def check(self):
        """the ONE read of the fixed-length solves since the last call.  False: some interface missed 30 rtol -- the solves have switched
        to the adaptive PCG (vert_mom_vort's mass solver leaves its fixed-length mode); the caller redoes the diagnoses"""
        v, = CheckLog.read(self._log)
        self._log.zero_()
        self.logged = 0
        ok = bool(accepted(v, 1.0, 30.0 * self.rtol)[0].all())
        if not ok:
            self.missed += 1
            self.m_its = 0
            if self.unit_mass is not None:
                self.unit_mass.chebyshev = False
        return ok

    def horiz_pot_vort(self, velx, rho):
        """uz [nk-1, n1] from velx [nk, n1], rho [nk, n2]"""
        eng = self.eng
        Mu = eng.apply("UMAT", velx, lev0=0, scale=SCALE, flags=VERT)            # M1->assemble(k, SCALE, true)
        du = eng.combine(Mu[1:], 1.0, beta=-1.0, c=Mu[:-1])
        rb = self.rho_bar(rho)
        P = eng.elem_block_pc_levels("UTMAT_H", self.ni, f=rb, lev0=0, lev_step=1, scale=SCALE)
        A = lambda v: eng.apply("UTMAT_H", v, f=rb, lev0=0, scale=SCALE)         # M1t->assemble_h(i, SCALE, rho_h)
        return self._solve("uz", A, du, P)

    def vert_vort(self, velz_h, rho):
        """dwdx [nk-1, n1] from velz_h [nk-1, n2] (horizontal layout), rho [nk, n2]"""
        eng = self.eng
        rhs = eng.incidence("E12", eng.apply_levels("WMAT", velz_h, 0, lev0=0, scale=SCALE, flags=VERT))     # M2->assemble(0, SCALE, true)
        rb = self.rho_bar(rho)
        P = eng.elem_block_pc_levels("UHMAT", self.ni, f=rb, lev0=0, lev_step=0, scale=SCALE)
        A = lambda v: eng.apply_levels("UHMAT", v, 0, f=rb, lev0=0, scale=SCALE)  # F->assemble(rho_h, 0, false, SCALE)
        return self._solve("dwdx", A, rhs, P)

    def vert_mom_vort(self, ul, velz_h):
        """VertSolve::AssembleVertMomVort of the box twin (box/VertSolve.cpp:1460-1499): uuz [nEl, (nk-1) n2e] in the VERTICAL layout from
        ul [nk, n1] and velz_h [nk-1, n2] (horizontal layout), all nk - 1 interfaces per call:
            dwdx_i = M1o^-1 E12 M2o velz_i,   uuz_i = Rz(1/2 u_i + 1/2 u_{i+1}; SCALE) dwdx_i,   HorizToVert
        M1o / M2o: level 0, SCALE, no thickness (box/Assembly.cpp:45,172); Rz = WtQdUdz_mat.  The mass solve is unit_mass, a MassSolver
        without thickness, fixed length.  Its TRUE residual is logged with the other solves of this class and read by check(): on a uniform
        box the element-block preconditioner is exact (P M1o = I), the residual the last Chebyshev sweep saw -- what MassSolver.verify()
        judges -- is then zero after the first step whatever the later steps do, and only the true residual shows a solve cut short"""
        eng = self.eng
        if self.unit_mass is None:
            from .krylov import MassSolver
            self.unit_mass = MassSolver(eng, SCALE, vert_scale=False)
        rhs = eng.incidence("E12", eng.apply_levels("WMAT", velz_h, 0, lev0=0, scale=SCALE, flags=0))        # M2->assemble(0, SCALE, false), E12
        dwdx, self.its["unit_mass"] = self.unit_mass.solve(rhs, lev0=0)                                  # KSPSolve(ksp1, tmp1, dwdx)
        log_true_residual(eng, lambda v: self.unit_mass.apply(v, 0), dwdx, rhs, self._log[2])
        self.logged += 1
        ub = eng.combine(ul[:-1], 0.5, beta=0.5, c=ul[1:])                                                # 0.5 ul[kk] + 0.5 ul[kk+1]
        return eng.l2_horiz_to_vert(eng.apply("WTQDUDZ", dwdx, f=ub, lev0=0, scale=SCALE))              # Rz->assemble(_ul, SCALE), HorizToVert

    def vert_mass_flux(self, velz1, velz2, rho1, rho2):
        """Fz [nk-1, n2] in the horizontal layout from velz [nk-1, n2] and rho [nk, n2] in the horizontal layout"""
        eng = self.eng
        if self.vert is None:
            from .vertsolve import VertSolve
            self.vert = VertSolve(eng, 0.0)                                      # (diagnose_F_z does not use the time step)
        tv = eng.l2_horiz_to_vert
        F = self.vert.diagnose_F_z(tv(velz1), tv(velz2), tv(rho1), tv(rho2))
        return eng.l2_vert_to_horiz(F.contiguous(), self.ni)
