"""Euler::Strang_ec (eul/Euler_2.cpp:1366-1557): one time step of the 3-D compressible Euler equations -- explicit horizontal momentum
predictor, implicit vertical Newton solve with the horizontal transport re-evaluated in every iteration, explicit horizontal corrector --
joined from the parts that each run on the device already:

  stage 1 (:1421-1457)  diagTheta_L2, VortDiag.horiz_pot_vort / vert_vort / vert_mass_flux, HorizSolve.momentum_rhs_ec, HorizMomentum.predictor
  stage 2 (:1461-1466)  VertSolve.solve_schur_eta with HorizSolve.advection_rhs_ec(velx_0, velx) as its horizontal forcing
  stage 3 (:1470-1493)  the three diagnoses on the new state, momentum_rhs_ec on the time-centred fields the solve left, HorizMomentum.corrector
  :1501                 Energetics.diagnostics on the new state: the line of output/energetics.dat

State carried between steps, as the reference carries it: first_step; u_prev / u_curr (:1415-1416: stage 1 of a later step is the leapfrog
M1 velx = M1 u_prev - 2 dt Fu); uz / uz_prev (:1425 on the first step uz_prev is stage 1's uz, :1407-1409 later the uz stage 3 of the step
before left).

Layouts, those of Energetics.diagnostics: velx [nk, n1]; rho, rt, exner [nk, n2] horizontal; velz [nEl, (nk-1) n2e] vertical.

The fixed-length solves are checked within the step: VortDiag.check() (the two density-weighted solves) once at its end; HorizSolve.verify()
(the 1-form mass solves) after stage 1, at the head of every Newton iteration -- where the host waits for the iteration's norms anyway -- and
at the end, because its device log keeps 16 solves and a step has more.  On a miss those solvers have switched to their adaptive forms and
the step is redone from its inputs.  The carried state is committed only after the checks pass, so a redone step sees what the missed one
saw (ThermalSW treats a missed step the same way).

One difference from the reference, kept out on purpose: at :1475 the reference pairs the global vectors (velx_0, velx) with the LOCAL copies
in the other order (ul, ul_prev).  HorizSolve.momentum_rhs_ec has one vector per argument (local == global on one context), so each velocity
is paired with itself.  Single context, global numbering; sharded engines are not supported."""
from .energetics import Energetics
from .hmomentum import HorizMomentum
from .horizsolve import HorizSolve
from .vertsolve import VertSolve
from .vortdiag import VortDiag


class Euler:
    # diagnose_Phi inside the step: the one-launch kernel (mimsem_horiz_bernoulli) or the eight composed launches -- decided by the
    # measurement of scripts/prof_strang.py (profiles/strang_ec.txt)
    FUSED_PHI = True

    def __init__(self, eng, dt, levs, quad_coords, hs_forcing=False, hs_lat=None, newton_maxit=20, newton_tol=1e-12, do_visc=True):
        """eng: Engine (one context, global numbering, nk >= 2); levs: interface heights on the quadrature grid [nk+1, nq] (VertSolve.init_gz);
        quad_coords: [nq, 3] (HorizSolve.coriolis); hs_lat: latitude of the quadrature points [nEl, mp12], needed with hs_forcing"""
        if hasattr(eng, "halo"):
            raise NotImplementedError("Euler: sharded engines are not supported")
        if hs_forcing and hs_lat is None:
            raise ValueError("Euler: Held-Suarez forcing needs hs_lat")
        self.eng, self.dt, self.nk = eng, dt, eng.nk
        self.hs_forcing, self.hs_lat = hs_forcing, hs_lat
        self.newton_maxit, self.newton_tol = newton_maxit, newton_tol
        self.horiz = HorizSolve(eng, quad_coords=quad_coords, do_visc=do_visc)
        self.horiz.fused_phi = self.FUSED_PHI
        self.vert = VertSolve(eng, dt)
        self.vort = VortDiag(eng, self.horiz, self.vert)
        self.hmom = HorizMomentum(eng, self.horiz, dt, hs_forcing)
        self.energetics = Energetics(eng, self.vert, self.horiz)
        self.zv = self.vert.init_gz(levs)
        self.energetics.set_geopotential(self.zv)
        self.first_step = True
        self.u_prev = self.u_curr = self.uz = self.uz_prev = None
        self.steps = 0
        self.redone = 0                  # steps that missed a check and were run again

    def _step(self, velx, velz, rho, rt, exner, carried):
        """one evaluation of the step from `carried` = (first_step, u_curr, uz); changes nothing of self.first_step / u_* / uz*.
        Returns the new fields, the carried vectors of the step and whether every HorizSolve.verify() along the way passed"""
        eng, nk, horiz, vert, vort = self.eng, self.nk, self.horiz, self.vert, self.vort
        first, u_curr, uz_last = carried
        to_v = eng.l2_horiz_to_vert
        to_h = lambda a, rows=nk: eng.l2_vert_to_horiz(a.contiguous(), rows)
        # 0. the initial fields in both layouts (:1390-1395); the carried vectors of this step (:1399-1417)
        velz_h0 = to_h(velz, nk - 1)
        rho_v, rt_v, exner_v = to_v(rho), to_v(rt), to_v(exner)
        uz_prev = None if first else uz_last
        u_prev, u_curr = u_curr, velx.clone()
        # 1. explicit horizontal momentum solve, the predictor (:1421-1457)
        theta_0 = to_h(eng.diag_theta(0, rho_v, rt_v))
        uz = vort.horiz_pot_vort(velx, rho)
        dwdx1 = vort.vert_vort(velz_h0, rho)
        if first:
            uz_prev = uz                                                                # :1425
        Fz = vort.vert_mass_flux(velz_h0, velz_h0, rho, rho)
        Fu = horiz.momentum_rhs_ec(theta_0, uz, uz, velz_h0, velz_h0, exner, velx, velx, rho, rho, Fz=Fz, dwdx1=dwdx1, dwdx2=dwdx1)
        velx_p = self.hmom.predictor(velx, u_prev, Fu, exner, first)
        ok = [horiz.verify()]
        # 2. implicit vertical solve (:1461-1466): advection_rhs_ec(velx_0, velx, rho_i, rho_j, theta_l2_h) at the head of every Newton iteration
        # (eul/VertSolve.cpp:1798-1799); rho_i in the horizontal layout is the rho this step was given

        def forcing(rho_i, rho_j, theta_l2_h):
            ok.append(horiz.verify())                                                   # (the solves of the iteration before)
            dF, dG, _, _ = horiz.advection_rhs_ec(velx, velx_p, rho, to_h(rho_j), to_h(theta_l2_h))
            return to_v(dF), to_v(dG)
        velz_n, rho_nv, rt_nv, exner_nv = vert.solve_schur_eta(velz, rho_v, rt_v, exner_v, self.zv, horiz_forcing=forcing, udwdx=None,
                                                               hs_lat=self.hs_lat if self.hs_forcing else None,
                                                               maxit=self.newton_maxit, tol=self.newton_tol)
        rho_n, rt_n, exner_n = to_h(rho_nv), to_h(rt_nv), to_h(exner_nv)
        velz_hn = to_h(velz_n, nk - 1)
        # 3. explicit horizontal solve, the corrector (:1470-1493): the time-centred theta_l2_h, exner_h the vertical solve left; the friction
        # takes the NEW exner (:1482: the L2Vecs the solve overwrote in place); Fk of the last advection_rhs_ec makes k2i the reference's (:704-708)
        uz = vort.horiz_pot_vort(velx_p, rho_n)
        dwdx2 = vort.vert_vort(velz_hn, rho_n)
        Fz = vort.vert_mass_flux(velz_h0, velz_hn, rho, rho_n)
        Fu = horiz.momentum_rhs_ec(to_h(vert.theta_l2_h), uz, uz_prev, velz_hn, velz_h0, to_h(vert.exner_h), velx, velx_p, rho, rho_n,
                                   Fz=Fz, dwdx1=dwdx1, dwdx2=dwdx2, Fk=horiz.Fk)
        velx_n = self.hmom.corrector(velx, Fu, exner_n)
        ok.append(horiz.verify())
        return (velx_n, velz_n, rho_n, rt_n, exner_n), (u_prev, u_curr, uz, uz_prev), all(ok)

    def strang_ec(self, velx, velz, rho, rt, exner, diagnostics=True):
        """one step; the inputs are not changed.  Returns (velx, velz, rho, rt, exner, values): the new fields and the twelve numbers of
        Energetics.diagnostics on them (None with diagnostics=False)"""
        carried = (self.first_step, self.u_curr, self.uz)
        for attempt in range(2):
            new, kept, ok_m1 = self._step(velx, velz, rho, rt, exner, carried)
            ok_vort = self.vort.check()                                                 # (the log is read and cleared)
            if ok_m1 and ok_vort:
                break
            self.redone += 1
        else:
            raise RuntimeError("Euler.strang_ec: a solve missed its check again after the switch to the adaptive solvers")
        self.u_prev, self.u_curr, self.uz, self.uz_prev = kept
        self.first_step = False
        self.steps += 1
        values = self.energetics.diagnostics(*new) if diagnostics else None            # :1501
        return (*new, values)
