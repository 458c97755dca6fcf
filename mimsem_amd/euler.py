"""Euler::Strang_ec (eul/Euler_2.cpp:1366-1557) and Euler::Strang (:1146-1364; Euler.strang says where it differs): one time step of the 3-D
compressible Euler equations -- explicit horizontal momentum
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
is paired with itself.  Single context, global numbering; sharded engines are not supported.

The baroclinic-wave driver around the step (eul/UMJS14.cpp:291-353) is host-side composition of the same device calls: init1 / init2
(eul/Euler_2.cpp:429-529) project fields given on the quadrature grid, initial_state applies them to mimsem_amd/umjs14.py, run loops
strang_ec with the reference's dump numbering, dump is the `save` branch (:1503-1534) and load the restart branch (UMJS14.cpp:334-344)."""
import os

import numpy as np
import torch

from . import bubble, io, umjs14
from .energetics import Energetics
from .geom import gll_weights
from .hmomentum import HorizMomentum
from .horizsolve import LX, SCALE, VERT, BoxHorizSolve, HorizSolve
from .vertsolve import VertSolve
from .vortdiag import VortDiag


def last_writer_table(indsq, nq):
    """for every global quadrature point the flat index e mp12 + i of the element-local point whose value Geom::write0 / write1 / write2
    leave there.  They store with INSERT_VALUES in the element loop ey, ex ascending (eul/Geom.cpp:441-452), so of the elements that share a
    point the one visited last wins; patches count in the order of their ranks (between ranks PETSc leaves the order of INSERT_VALUES open).
    indsq [nEl, mp12]: DeviceMesh.indsq, elements patch by patch in that loop order.  numpy's indexed assignment keeps the last of repeated
    indices, which is the rule"""
    iq = np.asarray(indsq).reshape(-1)
    last = np.full(nq, -1, dtype=np.int64)
    last[iq] = np.arange(iq.size)
    if (last < 0).any():
        raise ValueError("last_writer_table: a quadrature point that no element holds")
    return last


class Euler:
    # diagnose_Phi inside the step: the one-launch kernel (mimsem_horiz_bernoulli) or the eight composed launches -- decided by the
    # measurement of scripts/prof_strang.py (profiles/strang_ec.txt)
    FUSED_PHI = True
    # the mass-flux right-hand side inside strang: the two-launch kernel (mimsem_horiz_flux_rhs) or four accumulated Uhmat applies -- to be
    # decided by the measurement of scripts/prof_strang2.py (profiles/strang.txt); that file does not exist yet, so the composed route
    FUSED_HU = False

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
        self.horiz = self._make_horiz(quad_coords, do_visc)
        self.horiz.fused_phi = self.FUSED_PHI
        self.vert = self._make_vert()
        self.vort = VortDiag(eng, self.horiz, self.vert)
        self.hmom = HorizMomentum(eng, self.horiz, dt, hs_forcing)
        self.energetics = Energetics(eng, self.vert, self.horiz)
        self.zv = self.vert.init_gz(levs)
        self.energetics.set_geopotential(self.zv)
        self.first_step = True
        self.u_prev = self.u_curr = self.uz = self.uz_prev = None
        self.steps = 0
        self.redone = 0                  # steps that missed a check and were run again
        self.xq = np.asarray(quad_coords, dtype=np.float64)
        self.step = 0                    # the dump counter (Euler::step, set to startStep by the driver: eul/UMJS14.cpp:297)
        self.init1_redone = 0            # init1 solves run again after a missed check
        self._m2inv = self._last = self._thick = None

    def _make_horiz(self, quad_coords, do_visc):
        return HorizSolve(self.eng, quad_coords=quad_coords, do_visc=do_visc)

    def _make_vert(self):
        return VertSolve(self.eng, self.dt)

    def _step(self, velx, velz, rho, rt, exner, carried, ec=True):
        """one evaluation of the step from `carried` = (first_step, u_curr, uz); changes nothing of self.first_step / u_* / uz*.
        ec: Strang_ec (theta in the levels, the _ec right-hand sides, solve_schur_eta); else Strang (theta on the interfaces, momentum_rhs /
        advection_rhs, solve_schur_2) -- the comments name the lines of Strang_ec, Strang's are :1170-1300 in the same order.
        Returns the new fields, the carried vectors of the step and whether every HorizSolve.verify() along the way passed"""
        eng, nk, horiz, vert, vort = self.eng, self.nk, self.horiz, self.vert, self.vort
        first, u_curr, uz_last = carried
        rows_th = nk if ec else nk + 1                                                  # theta: L2 in the levels / on the nk+1 interfaces
        mom_rhs, adv_rhs = (horiz.momentum_rhs_ec, horiz.advection_rhs_ec) if ec else (horiz.momentum_rhs, horiz.advection_rhs)
        solve = vert.solve_schur_eta if ec else vert.solve_schur_2
        to_v = eng.l2_horiz_to_vert
        to_h = lambda a, rows=nk: eng.l2_vert_to_horiz(a.contiguous(), rows)
        # 0. the initial fields in both layouts (:1390-1395); the carried vectors of this step (:1399-1417)
        velz_h0 = to_h(velz, nk - 1)
        rho_v, rt_v, exner_v = to_v(rho), to_v(rt), to_v(exner)
        uz_prev = None if first else uz_last
        u_prev, u_curr = u_curr, velx.clone()
        # 1. explicit horizontal momentum solve, the predictor (:1421-1457)
        theta_0 = to_h(self._stage1_theta(ec, rho_v, rt_v, velz), rows_th)
        self._theta_0 = theta_0                                                         # (what the box twin's diagnostics take the entropy of)
        uz = vort.horiz_pot_vort(velx, rho)
        dwdx1 = vort.vert_vort(velz_h0, rho)
        if first:
            uz_prev = uz                                                                # :1425
        Fz = vort.vert_mass_flux(velz_h0, velz_h0, rho, rho)
        Fu = mom_rhs(theta_0, uz, uz, velz_h0, velz_h0, exner, velx, velx, rho, rho, Fz=Fz, dwdx1=dwdx1, dwdx2=dwdx1)
        velx_p = self.hmom.predictor(velx, u_prev, Fu, exner, first)
        ok = [horiz.verify()]
        # 2. implicit vertical solve (:1461-1466): advection_rhs_ec(velx_0, velx, rho_i, rho_j, theta_l2_h) at the head of every Newton iteration
        # (eul/VertSolve.cpp:1798-1799); rho_i in the horizontal layout is the rho this step was given

        def forcing(rho_i, rho_j, theta_l2_h):
            ok.append(horiz.verify())                                                   # (the solves of the iteration before)
            dF, dG, _, _ = adv_rhs(velx, velx_p, rho, to_h(rho_j), to_h(theta_l2_h, rows_th))
            return to_v(dF), to_v(dG)
        velz_n, rho_nv, rt_nv, exner_nv = solve(velz, rho_v, rt_v, exner_v, self.zv, horiz_forcing=forcing,
                                                hs_lat=self.hs_lat if self.hs_forcing else None,
                                                maxit=self.newton_maxit, tol=self.newton_tol,
                                                **self._vertical_solve_options(first, velx, velx_p, velz_h0))
        rho_n, rt_n, exner_n = to_h(rho_nv), to_h(rt_nv), to_h(exner_nv)
        velz_hn = to_h(velz_n, nk - 1)
        # 3. explicit horizontal solve, the corrector (:1470-1493): the time-centred theta_l2_h, exner_h the vertical solve left; the friction
        # takes the NEW exner (:1482: the L2Vecs the solve overwrote in place); Fk of the last advection_rhs_ec makes k2i the reference's (:704-708)
        uz = vort.horiz_pot_vort(velx_p, rho_n)
        dwdx2 = vort.vert_vort(velz_hn, rho_n)
        Fz = vort.vert_mass_flux(velz_h0, velz_hn, rho, rho_n)
        theta_h = to_h(vert.theta_l2_h if ec else vert.theta_h, rows_th)
        Fu = mom_rhs(theta_h, uz, uz_prev, velz_hn, velz_h0, to_h(vert.exner_h), velx, velx_p, rho, rho_n,
                     Fz=Fz, dwdx1=dwdx1, dwdx2=dwdx2, Fk=horiz.Fk)
        velx_n = self.hmom.corrector(velx, Fu, exner_n)
        ok.append(horiz.verify())
        return (velx_n, velz_n, rho_n, rt_n, exner_n), (u_prev, u_curr, uz, uz_prev), all(ok)

    # ---- what the box twin's step does differently (BoxEuler) ------------------------------------------------------------------------------
    def _stage1_theta(self, ec, rho_v, rt_v, velz):
        """theta_0 of stage 1 in the vertical layout: diagTheta_L2 (:1421) / diagTheta2 (:1201)"""
        return self.eng.diag_theta(0 if ec else 1, rho_v, rt_v)

    def _vertical_solve_options(self, first, velx, velx_p, velz_h0):
        """further keyword arguments of the vertical solve of stage 2"""
        return dict(udwdx=None)

    def _diagnostics(self, new):
        """the energetics line of the new state (:1501)"""
        return self.energetics.diagnostics(*new)

    def strang_ec(self, velx, velz, rho, rt, exner, diagnostics=True):
        """one step; the inputs are not changed.  Returns (velx, velz, rho, rt, exner, values): the new fields and the twelve numbers of
        Energetics.diagnostics on them (None with diagnostics=False)"""
        return self._checked_step("strang_ec", True, velx, velz, rho, rt, exner, diagnostics)

    def strang(self, velx, velz, rho, rt, exner, diagnostics=True):
        """Euler::Strang (eul/Euler_2.cpp:1146-1364), the integrator of eul/HeldSuarez.cpp: the skeleton of strang_ec -- the same carried state,
        check points, redo on a miss and energetics line -- with theta on the nk+1 interfaces:
          stage 1 (:1199-1251)  theta_0 = diagTheta (= VertSolve::diagTheta2), HorizSolve.momentum_rhs in place of momentum_rhs_ec
          stage 2 (:1253-1260)  VertSolve.solve_schur_2 with HorizSolve.advection_rhs(velx_0, velx, rho_0, rho_j, theta_h) as its forcing
          stage 3 (:1262-1300)  momentum_rhs on vert.theta_h, vert.exner_h with Fk of the last advection_rhs; the corrector takes the new exner
        The mass-flux right-hand sides of the two take the route FUSED_HU names.  Two lines of the reference are not mirrored: :1180 fills
        vert->theta_h on the first step, which solve_schur_2 overwrites before any read; :1269 hands stage 3 the local velocity copies in the
        other order than the global vectors (the :1475 quirk of Strang_ec) -- each velocity is paired with itself, as strang_ec does.
        Same arguments and result as strang_ec"""
        self.horiz.fused_hu = self.FUSED_HU
        return self._checked_step("strang", False, velx, velz, rho, rt, exner, diagnostics)

    def _checked_step(self, name, ec, velx, velz, rho, rt, exner, diagnostics):
        carried = (self.first_step, self.u_curr, self.uz)
        for attempt in range(2):
            new, kept, ok_m1 = self._step(velx, velz, rho, rt, exner, carried, ec)
            ok_vort = self.vort.check()                                                 # (the log is read and cleared)
            if ok_m1 and ok_vort:
                break
            self.redone += 1
        else:
            raise RuntimeError("Euler.%s: a solve missed its check again after the switch to the adaptive solvers" % name)
        self.u_prev, self.u_curr, self.uz, self.uz_prev = kept
        self.first_step = False
        self.steps += 1
        values = self._diagnostics(new) if diagnostics else None                       # :1501
        return (*new, values)

    # ---- the initial state (eul/Euler_2.cpp:429-529, eul/UMJS14.cpp:318-322) -----------------------------------------------------------
    def _m2_inverse(self):
        """the exact inverses of the nk x nEl element blocks of M2(k, SCALE, vert_scale = true) -- M2 is element-block diagonal, and the levels
        do not change: built once"""
        if self._m2inv is None:
            eng, n2e = self.eng, self.eng.n2e
            B = torch.stack([eng.element_matrices("WMAT", lev=k, scale=SCALE, flags=VERT).view(eng.nEl, n2e, n2e) for k in range(self.nk)])
            self._m2inv = eng.block_inverse(B.view(self.nk * eng.nEl, n2e, n2e)).view(self.nk, eng.nEl, n2e, n2e)
        return self._m2inv

    def _quad_rows(self, fq, cols, what):
        fq = torch.as_tensor(fq, dtype=torch.float64).to(self.eng.device).reshape(-1, cols).contiguous()
        if fq.shape[0] != self.nk:
            raise ValueError("Euler.%s: one row of the quadrature grid per level expected" % what)
        return fq

    def init2(self, fq):
        """:489-529: fq [nk, nq] on the quadrature grid -> the 2-form [nk, n2], h_k = M2(k, SCALE, true)^-1 SCALE WtQ f_k"""
        b = self.eng.apply("WTQ", self._quad_rows(fq, self.eng.sizes["q"], "init2"))
        return self.eng.blocks_apply(2, self._m2_inverse(), b.mul_(SCALE))

    def init1(self, uq):
        """:429-487: uq [nk, nq, 2] (func_x, func_y interleaved per quadrature point, :454-455) -> the 1-form [nk, n1],
        u_k = M1(k, SCALE, true)^-1 SCALE UtQ uq_k, every level in one batched solve of HorizSolve's mass solver.  eul/'s UtQmat
        (eul/Assembly.cpp:824-902) is src/'s (src/Assembly.cpp:1052-1139) entry for entry -- J[0][0], J[1][0] on the x edges, J[0][1], J[1][1] on
        the y edges, columns 2 q + {0, 1}, no thickness factor -- so Engine.apply("UTQ") is the operator.  The solve is checked through
        verify(); after a miss the solver has switched to its adaptive form and the solve is run again"""
        b = self.eng.apply("UTQ", self._quad_rows(uq, self.eng.sizes["q2"], "init1")).mul_(SCALE)
        for attempt in range(2):
            u, _ = self.horiz.m1.solve(b)
            if self.horiz.verify():
                return u
            self.init1_redone += 1
        raise RuntimeError("Euler.init1: the solve missed its check again after the switch to the adaptive solver")

    def initial_state(self, vp=umjs14.VP, cut=True):
        """(velx, velz, rho, rt, exner) of the baroclinic-wave case in strang_ec's layouts (eul/UMJS14.cpp:313-322): the analytic fields of
        mimsem_amd/umjs14.py at this object's quadrature points and level count, projected by init1 / init2; velz = 0.  The levels this
        object was built with are expected to be umjs14.levels(nk, quad_coords); vp = 0 gives the steady state; cut=False is the wind
        perturbation of eul/HeldSuarez.cpp, not cut beyond D0 (mimsem_amd/heldsuarez.py)"""
        uq, rho, rt, exner = umjs14.layer_fields(self.nk, self.xq, vp, cut)
        velz = self.eng.zeros(self.eng.nEl, (self.nk - 1) * self.eng.n2e)
        return self.init1(uq), velz, self.init2(rho), self.init2(rt), self.init2(exner)

    # ---- the loop, the `save` branch and the restart (eul/UMJS14.cpp:334-353, eul/Euler_2.cpp:1503-1534) -------------------------------------
    def run(self, state, nsteps, dump_every=0, outdir="output", start_step=0, on_step=None, integrator="strang_ec", on_state=None):
        """the driver's loop (eul/UMJS14.cpp:347-353): step = start_step dump_every + 1 .. nsteps, each one strang_ec (or, with
        integrator="strang", strang: eul/HeldSuarez.cpp:352) whose twelve numbers go to
        outdir/energetics.dat (Energetics.write_line); on a step with step % dump_every == 0 the dump counter self.step (which starts at
        start_step) goes up by one and dump() writes under it.  on_step(step, values), when given, is called after every step;
        on_state(step, state), when given, before it with the step's new fields (ZonalStats.sample fits as it is).  Returns the final state"""
        if integrator not in ("strang_ec", "strang"):
            raise ValueError("Euler.run: integrator is 'strang_ec' or 'strang', got %r" % (integrator,))
        one_step = getattr(self, integrator)
        self.step = start_step
        os.makedirs(outdir, exist_ok=True)
        path = os.path.join(outdir, "energetics.dat")
        state = tuple(state)
        for step in range(start_step * dump_every + 1, nsteps + 1):
            out = one_step(*state)
            state = out[:5]
            Energetics.write_line(path, out[5])
            if dump_every and step % dump_every == 0:
                self.step += 1                                                          # :1505
                self.dump(state, self.step, outdir)
            if on_state is not None:
                on_state(step, state)
            if on_step is not None:
                on_step(step, out[5])
        return state

    def last_writer(self):
        """last_writer_table of this mesh as a device tensor, made once"""
        if self._last is None:
            self._last = torch.as_tensor(last_writer_table(self.eng.mesh.indsq, self.eng.sizes["q"]), device=self.eng.device)
            self._thick = torch.as_tensor(np.ascontiguousarray(self.eng.mesh.thick), device=self.eng.device)
        return self._last

    def quad_fields(self, state):
        """the physical fields of the `save` branch on the quadrature grid, {name: [nlev, nq] device tensor} in the global quadrature numbering:
        Geom::write0 of the vorticity (HorizSolve::curl per level), write1 of velocity_h (two components), write2 with vert_scale = true of
        density, rhoTheta, exner -- each divided by the level's thickness -- and write2 with vert_scale = false of theta (nk+1 levels) and
        velocity_z (nk-1 levels).  A point shared by several elements takes the value of last_writer()'s element, by a gather.  Returns that
        dict and the two fields diagnosed on the way, theta [nk+1, n2] and velz in the horizontal layout [nk-1, n2]"""
        eng, nk = self.eng, self.nk
        velx, velz, rho, rt, exner = state
        last = self.last_writer()
        pick = lambda a, thick: (a / self._thick if thick else a).reshape(a.shape[0], -1)[:, last].contiguous()
        theta = eng.l2_vert_to_horiz(eng.diag_theta(1, eng.l2_horiz_to_vert(rho), eng.l2_horiz_to_vert(rt)), nk + 1)
        velz_h = eng.l2_vert_to_horiz(velz.contiguous(), nk - 1)
        uq = eng.interp_quad(1, velx)
        out = {"vorticity": pick(eng.interp_quad(0, self.horiz.curl(velx)), True),
               "velocity_h_x": pick(uq[..., 0], True), "velocity_h_y": pick(uq[..., 1], True)}
        for name, a in (("density", rho), ("rhoTheta", rt), ("exner", exner)):
            out[name] = pick(eng.interp_quad(2, a), True)
        out["theta"] = pick(eng.interp_quad(2, theta), False)
        out["velocity_z"] = pick(eng.interp_quad(2, velz_h), False)
        return out, theta, velz_h

    def dump(self, state, step, outdir="output"):
        """the `save` branch of Strang_ec (eul/Euler_2.cpp:1503-1534) for `state` under the dump index `step`:
          - the raw degree-of-freedom vectors, the .vec files of Geom::write1 / write2 (eul/Geom.cpp:553, :627) that LoadVecs / LoadVecsVert
            read back, in the reference's names <field>_<level %.3u>_<step %.4u>.vec: velocity_h, density, rhoTheta, exner (nk levels),
            velocity_z (nk-1 levels in the horizontal layout, Geom::writeVertToHoriz) and theta (nk+1 levels, diagTheta2 of the state);
          - quad_fields() as one [nlev, nq] array per field, <field>_<step %.4u>.npy.
        The reference writes the quadrature-grid fields through PETSc's ASCII viewer (.dat); that format is third-party and unpinned in the
        reference and is not reproduced"""
        velx, velz, rho, rt, exner = state
        quad, theta, velz_h = self.quad_fields(state)
        host = lambda a: a.detach().cpu().numpy()
        for name, a in (("velocity_h", velx), ("density", rho), ("rhoTheta", rt), ("exner", exner), ("velocity_z", velz_h), ("theta", theta)):
            io.save_levels(name, step, host(a), outdir)
        for name, a in quad.items():
            np.save(os.path.join(outdir, "%s_%.4u.npy" % (name, step)), host(a))

    def load(self, step, outdir="output"):
        """the restart branch (eul/UMJS14.cpp:334-344): (velx, velz, rho, rt, exner) from the .vec files of dump index `step`.  As in the
        reference a restarted Euler begins with first_step = True: u_prev / uz_prev are not in the dumps, the first step after a restart
        takes the forward predictor and uz_prev = uz, so a restarted run is not the continued run"""
        eng, nk = self.eng, self.nk
        rows = lambda name, n: eng.tensor(io.load_levels(name, step, n, outdir))
        rho, velx, exner, rt = rows("density", nk), rows("velocity_h", nk), rows("exner", nk), rows("rhoTheta", nk)
        velz = eng.l2_horiz_to_vert(rows("velocity_z", nk - 1))                       # LoadVecsVert :251-267
        self.first_step = True
        self.u_prev = self.u_curr = self.uz = self.uz_prev = None
        return velx, velz, rho, rt, exner


class BoxEuler(Euler):
    """Euler::Strang of the doubly periodic box (box/Euler_2.cpp:1306-1477): Euler.strang's skeleton -- the carried state, the check points,
    the redo on a miss, the commit after the checks -- on BoxHorizSolve, with what the box twin does differently:

      stage 1 (:1359-1383)  theta_0 = Euler::diagTheta (:543-565) = diag_theta_wup(0.25 dt, rho, rt, velz): the test functions upwinded by the
                            vertical velocity; plain M1 predictor and corrector solves, no friction
      uuz (:1337)           AssembleVertMomVort(velz_0) runs before ul is filled on the first step and PETSc vectors start zeroed: uuz = 0 on
                            the first step, vert_mom_vort(velx, velz_0) on later ones (ul then holds the velocity the last step left)
      stage 2 (:1392)       solve_schur_2(schur3_flags = 3, theta_up, udwdx = uuz, vert_mom_vort bound to the predictor velocity (u2l = ul,
                            box/VertSolve.cpp:1403), horiz_forcing = advection_rhs(velx_0, velx_p, ...))
      stage 3 (:1399-1413)  on vert.theta_h / vert.exner_h with Fk of the last advection_rhs; uz / uz_prev and u_prev / u_curr as on the sphere.
                            The order of the local copies at :1403 (ul, ul_prev against velx_0, velx) has no effect here: the box Phi and wxu
                            are symmetric in the pair
      diagnostics (:887-1026)  eleven numbers are Energetics' own; the entropy is the box's: CP sum_columns sum_{k=0..nk} lz_k sum_q Q_q
                            log((W theta_k)_q), lz half a layer at both ends, of STAGE 1's theta_0 -- the field the reference passes (:1421)

    Orders 1..4 (Engine.diag_theta_wup).  Uniform layers only (BoxHorizSolve).  Not built: Trapazoidal (:1065), the quadrature-grid dumps"""
    # the element-local sum of momentum_rhs: mimsem_horiz_momentum_forcing (two launches) or the composed applies -- decided by the
    # measurement of scripts/prof_box_strang.py (profiles/box_strang.txt: p = 4, 32 x 32 x 64; one evaluation 585 us against 609 us, the
    # forcing alone 63 us against 115 us)
    FUSED_FORCING = True
    # the entropy of the energetics line: mimsem_euler_log_entropy (two launches, nothing but theta read) or interp_quad, torch.log and a
    # weighted sum -- decided by the measurement of scripts/prof_box_entropy.py (profiles/box_entropy.txt: p = 4, 32 x 32 x 64; 24.9 us
    # against 43.7 us)
    FUSED_ENTROPY = True

    def __init__(self, eng, dt, levs, quad_coords, lx=LX, newton_maxit=20, newton_tol=1e-12, do_visc=True):
        """eng: Engine of a one-patch PeriodicBox (global numbering, nk >= 4, order <= 4); levs [nk+1, nq]; quad_coords [nq, 3]"""
        if eng.mesh.n > 4:
            raise NotImplementedError("BoxEuler: orders 1..4 (the upwinded theta diagnosis), got %d" % eng.mesh.n)
        self.lx = lx
        super().__init__(eng, dt, levs, quad_coords, newton_maxit=newton_maxit, newton_tol=newton_tol, do_visc=do_visc)
        self.horiz.fused_forcing = self.FUSED_FORCING
        self._theta_0 = None
        w = torch.as_tensor(gll_weights(eng.mesh.m), dtype=torch.float64, device=eng.device)
        self._Q = (w[:, None] * w[None, :]).reshape(-1)                                 # Q_q = w_qx w_qy, q = qy mp1 + qx
        lz = torch.full((self.nk + 1,), self.horiz.thickness, dtype=torch.float64, device=eng.device)
        lz[0] *= 0.5; lz[-1] *= 0.5                                                     # :988
        self._lz = lz

    def _make_horiz(self, quad_coords, do_visc):
        return BoxHorizSolve(self.eng, lx=self.lx, do_visc=do_visc)

    def _make_vert(self):
        return VertSolve(self.eng, self.dt, rayleigh=0.0)                               # box/VertSolve.cpp:30: no Rayleigh layer

    def _stage1_theta(self, ec, rho_v, rt_v, velz):
        return self.eng.diag_theta_wup(0.25 * self.dt, rho_v, rt_v, velz)              # Euler::diagTheta :543-565

    def _vertical_solve_options(self, first, velx, velx_p, velz_h0):
        eng, nk = self.eng, self.nk
        uuz = eng.zeros(eng.nEl, (nk - 1) * eng.n2e) if first else self.vort.vert_mom_vort(velx, velz_h0)             # :1337
        mom_vort = lambda velz_j: self.vort.vert_mom_vort(velx_p, eng.l2_vert_to_horiz(velz_j.contiguous(), nk - 1))   # box/VertSolve.cpp:1403
        return dict(udwdx=uuz, schur3_flags=3, theta_up=True, vert_mom_vort=mom_vort)

    def entropy(self, theta):
        """:979-997 of theta [nk+1, n2] (horizontal layout), a device scalar"""
        if self.FUSED_ENTROPY:
            return self.eng.log_entropy(theta, self._lz, bubble.CP)[0]
        tq = self.eng.interp_quad(2, theta, push_forward=False)                        # W theta_k at the points: [nk+1, nEl, mp12]
        return bubble.CP * (self._lz[:, None, None] * self._Q[None, None, :] * torch.log(tq)).sum()

    def _diagnostics(self, new):
        out = self.energetics.diagnostics(*new, read=False).clone()
        out[11] = self.entropy(self._theta_0)
        return out.tolist()

    def strang(self, velx, velz, rho, rt, exner, diagnostics=True):
        """one step; the inputs are not changed.  Returns (velx, velz, rho, rt, exner, values) as Euler.strang"""
        return self._checked_step("strang", False, velx, velz, rho, rt, exner, diagnostics)

    def strang_ec(self, *a, **kw):
        raise NotImplementedError("BoxEuler: the box twin has no Strang_ec")

    def initial_state(self, theta_0=bubble.THETA_0, ztop=bubble.ZTOP):
        """(velx, velz, rho, rt, exner) of the rising bubble (box/Bubble.cpp:179-183): the analytic fields of mimsem_amd/bubble.py at this
        object's quadrature points and level count, projected by init1 / init2 -- which are box/Euler_2.cpp:719-817 line for line: the same
        UtQ / WtQ operators, SCALE, and M1->M / M2->M, on uniform layers the level-k matrices; velz = 0"""
        uq, rho, rt, exner = bubble.layer_fields(self.nk, self.xq, ztop=ztop, lx=self.lx, theta_0=theta_0)
        velz = self.eng.zeros(self.eng.nEl, (self.nk - 1) * self.eng.n2e)
        return self.init1(uq), velz, self.init2(rho), self.init2(rt), self.init2(exner)

    def run(self, state, nsteps, dump_every=0, outdir="output", start_step=0, on_step=None):
        """the driver's loop (box/Bubble.cpp:208-215), as Euler.run with Strang"""
        return super().run(state, nsteps, dump_every, outdir, start_step, on_step, integrator="strang")

    def dump(self, state, step, outdir="output"):
        """the .vec files of the `save` branch (:1424-1454): velocity_h, density, rhoTheta, exner (nk levels), velocity_z (nk-1 levels in the
        horizontal layout) and theta (nk+1 levels, Euler::diagTheta of the state: the upwinded diagnosis).  The quadrature-grid fields are not
        written"""
        eng, nk = self.eng, self.nk
        velx, velz, rho, rt, exner = state
        theta = eng.l2_vert_to_horiz(eng.diag_theta_wup(0.25 * self.dt, eng.l2_horiz_to_vert(rho), eng.l2_horiz_to_vert(rt), velz), nk + 1)
        velz_h = eng.l2_vert_to_horiz(velz.contiguous(), nk - 1)
        for name, a in (("velocity_h", velx), ("density", rho), ("rhoTheta", rt), ("exner", exner), ("velocity_z", velz_h), ("theta", theta)):
            io.save_levels(name, step, a.detach().cpu().numpy(), outdir)
