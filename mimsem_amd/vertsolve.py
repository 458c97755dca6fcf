"""Host-side mirror of the per-column residual assembly of the reference's VertSolve (eul/VertSolve.cpp:237-286,
432-502): compositions of VertOps operators and mat-vecs, here issued for ALL columns at once through the C ABI
(mimsem_colop_apply) on "vertical" device arrays [nEl][nslots*n2e] (L2Vecs::vz concatenated)."""
import os
import types

import torch

SCALE = 1.0e8          # eul/VertOps.cpp:21
RAYLEIGH = 4.0 / 120.0  # eul/VertSolve.cpp:32
FLAG_VERT = 1


class VertSolve:
    # solve_schur_2's default route: fused where its median iteration measured lower than the composed one's (profiles/schur2_newton.txt:
    # 0.627 / 1.093 ms at order 2, 1.170 / 2.088 ms at order 3, 2.060 / 4.348 ms at order 4); order 1 is not measured and stays composed
    FUSED2_ORDERS = (2, 3, 4)

    def __init__(self, eng, dt, rayleigh=RAYLEIGH):
        self.eng, self.dt, self.rayleigh = eng, dt, rayleigh
        self.nk, self.n2e = eng.nk, eng.n2e
        self.k2i_z = 0.0
        self._blocks = {}
        # orders 1..4: residual assembly / update of the Newton loop through the fused entry points (mimsem_column_newton_*: four
        # launches per iteration instead of ~150 single-operator calls); MIMSEM_NEWTON_FUSED=0 keeps the composed form below
        self.fused = os.environ.get("MIMSEM_NEWTON_FUSED", "1") != "0"
        # solve_schur_2: the fused route (mimsem_column_newton2_*) at the orders where it measured faster than the composed one
        # (profiles/schur2_newton.txt); MIMSEM_NEWTON_FUSED=0 keeps the composed form of both loops
        self.fused2 = self.fused and eng.mesh.n in self.FUSED2_ORDERS

    # thin wrappers: vo->AssembleX(ex,ey,...,M); MatMult(M, x, y) for every column
    _GEOMETRY_ONLY = ("CONST", "CONST_INV", "LINEAR", "LINEAR_INV", "RAYLEIGH")

    def _mv(self, colop, x, f1=None, f2=None, flags=0, rows=None, transpose=False):
        if colop in self._GEOMETRY_ONLY and f1 is None and f2 is None and flags == 0:
            # assembled once per VertSolve (the reference re-assembles before every MatMult; the blocks only depend on the mesh)
            if colop not in self._blocks:
                self._blocks[colop] = self.eng.colop_blocks(colop)
            return self.eng.colop_apply_blocks(colop, self._blocks[colop], x, rows, transpose=transpose)
        return self.eng.colop_apply(colop, x, f1=f1, f2=f2, flags=flags, transpose=transpose, nout_slots=rows)

    def V10(self, x):
        """MatMult(vo->V10, x, y): (nk x (nk-1)) -I/+I vertical divergence (eul/VertOps.cpp:134-163)"""
        return self.eng.column_incidence("V10", x.contiguous())

    def V01(self, x):
        """MatMult(vo->V01, x, y): V01 = -V10^T, vertical gradient across interfaces"""
        return self.eng.column_incidence("V01", x.contiguous())

    def diagnose_F_z(self, velz1, velz2, rho1, rho2):
        """eul/VertSolve.cpp:237-260"""
        nm = self.nk - 1
        t1 = self._mv("LINEAR_RT", velz1, f1=rho1, flags=FLAG_VERT, rows=nm)
        t2 = self._mv("LINEAR_RT", velz2, f1=rho1, flags=FLAG_VERT, rows=nm)
        F = (1.0 / 3.0) * self._mv("LINEAR_INV", t1, rows=nm) + (1.0 / 6.0) * self._mv("LINEAR_INV", t2, rows=nm)
        t1 = self._mv("LINEAR_RT", velz1, f1=rho2, flags=FLAG_VERT, rows=nm)
        t2 = self._mv("LINEAR_RT", velz2, f1=rho2, flags=FLAG_VERT, rows=nm)
        F += (1.0 / 6.0) * self._mv("LINEAR_INV", t1, rows=nm) + (1.0 / 3.0) * self._mv("LINEAR_INV", t2, rows=nm)
        return F

    def diagnose_Phi_z(self, velz1, velz2, zv):
        """eul/VertSolve.cpp:262-286"""
        nk = self.nk
        Phi = (1.0 / 6.0) * self._mv("CONLIN_W", velz1, f1=velz1, rows=nk)
        Phi += (1.0 / 6.0) * self._mv("CONLIN_W", velz2, f1=velz1, rows=nk)
        Phi += (1.0 / 6.0) * self._mv("CONLIN_W", velz2, f1=velz2, rows=nk)
        return Phi + zv

    def assemble_residual_ec(self, theta, Pi, velz1, velz2, rho1, rho2, zv):
        """eul/VertSolve.cpp:432-502 -> (fw, F, G, f_theta_corr); theta/Pi/rho on levels, velz on interfaces.  Leaves F * tA1 (the
        integrand of k2i_z) in self._k2i"""
        nk, nm, dt = self.nk, self.nk - 1, self.dt
        F = self.diagnose_F_z(velz1, velz2, rho1, rho2)
        Phi = self.diagnose_Phi_z(velz1, velz2, zv)
        fw = self._mv("LINEAR", velz2, rows=nm) - self._mv("LINEAR", velz1, rows=nm)
        fw += dt * self.V01(Phi)                                            # bernoulli function term
        tB = self._mv("CONST", Pi, rows=nk)
        tA2 = self._mv("LINEAR_INV", self.V01(tB), rows=nm)                 # pressure gradient
        tA1 = self._mv("LINEAR_RT", tA2, f1=theta, flags=FLAG_VERT, rows=nm)
        fw += 0.5 * dt * tA1
        self._k2i = F * tA1                                                 # kinetic to internal energy power, entry by entry (k2i_z: _newton)
        G = self._mv("LINEAR_INV", self._mv("LINEAR_RT", F, f1=theta, flags=FLAG_VERT, rows=nm), rows=nm)
        if self.rayleigh:
            fw += 0.5 * dt * self.rayleigh * (self._mv("RAYLEIGH", velz2, rows=nm) + self._mv("RAYLEIGH", velz1, rows=nm))
        # additional terms to ensure conservation of entropy
        tA2 = self._mv("LINEAR_INV", self.V01(self._mv("CONST", theta, rows=nk)), rows=nm)   # theta gradient
        fw += 0.5 * dt * self.V01(self._mv("CONST_RHO", Pi, f1=theta, rows=nk))
        fw -= 0.5 * dt * self._mv("CONLIN_W", Pi, f1=tA2, rows=nm, transpose=True)
        f_theta_corr = 0.5 * dt * self._mv("CONST_RHO", self.V10(F), f1=theta, rows=nk)
        f_theta_corr += 0.5 * dt * self._mv("CONLIN_W", F, f1=tA2, rows=nk)
        return fw, F, G, f_theta_corr

    def init_gz(self, levs, gravity=9.80616):
        """VertSolve::initGZ (eul/VertSolve.cpp:89-175): zv_k = W^T diag(SCALE w_q / 2) (g z_k + g z_{k+1}), the weak-form geopotential
        of every level from the interface heights on the quadrature grid (Geom::levs [nk+1, nq]); returned in the vertical layout"""
        eng = self.eng
        gz = gravity * torch.as_tensor(levs, dtype=torch.float64, device=eng.device)
        zh = (0.5 * SCALE) * eng.apply("WTQ", (gz[:-1] + gz[1:]).contiguous())
        return eng.l2_horiz_to_vert(zh)

    def horiz_forcing_from(self, hs, velx1, velx2):
        """the horizontal transport tendencies the Newton loop adds (eul/VertSolve.cpp:1799): HorizSolve::advection_rhs_ec on the
        horizontal layout, transposed into the vertical one (L2Vecs::HorizToVert)"""
        eng, nk = self.eng, self.nk

        def forcing(rho_i, rho_j, theta_l2_h):
            dF, dG, _, _ = hs.advection_rhs_ec(velx1, velx2, eng.l2_vert_to_horiz(rho_i, nk), eng.l2_vert_to_horiz(rho_j, nk),
                                                eng.l2_vert_to_horiz(theta_l2_h, nk))
            return eng.l2_horiz_to_vert(dF), eng.l2_horiz_to_vert(dG)
        return forcing

    # ---- the vertical implicit solve: the caller of the column path ---------------------------------------
    def solve_schur_eta(self, velz_i, rho_i, rt_i, exner_i, zv, horiz_forcing=None, udwdx=None, hs_lat=None, maxit=20, tol=1.0e-12,
                        verbose=False):
        """VertSolve::solve_schur_eta (eul/VertSolve.cpp:1721-1973) for EVERY column at once: Newton iterations on (w, rho, eta, Pi)
        with solve_schur_column_eta as the linear solve, all state in the "vertical" layout [nEl][slots*n2e] (L2Vecs::vz).

        horiz_forcing(rho_i, rho_j, theta_l2_h) -> (dFx, dGx): the horizontal transport tendencies of advection_rhs_ec in the
        vertical layout ([nEl][nk*n2e]); None = no horizontal wind.  udwdx: optional [nEl][(nk-1)*n2e].  hs_lat: latitude of the
        quadrature points [nEl][mp12] switches the Held-Suarez temperature forcing on.
        Returns (velz, rho, rt, exner) at the new time level and leaves theta_h / theta_l2_h / exner_h (the time-centred fields
        the horizontal corrector reads) and the per-iteration max-norms in self.*"""
        eng, nk, dt = self.eng, self.nk, self.dt
        x_i = (velz_i, rho_i, rt_i, exner_i)
        mv = self._mv

        def composed(S):
            """one iteration on the single-operator entry points: every order"""
            dFx, dGx = horiz_forcing(rho_i, S.rho_j, S.theta_l2_h) if horiz_forcing is not None else (None, None)
            F_w, F_z, G_z, ftc = self.assemble_residual_ec(S.theta_l2_h, S.exner_h, velz_i, S.velz_j, rho_i, S.rho_j, zv)     # :1806
            if udwdx is not None:
                F_w = F_w + dt * udwdx
            F_exner = eng.column_eos(0, S.rt_j, S.exner_j)                # Assemble_EOS_Residual :1810
            dF_z = S.rho_j + dt * self.V10(F_z) - rho_i                   # VecAYPX / VecAXPY :1815-1819
            dG_z = S.rt_j + 0.5 * dt * self.V10(G_z) - rt_i
            F_rho = mv("CONST", dF_z, rows=nk)
            F_rt = mv("CONST", dG_z, rows=nk) + ftc
            if dFx is not None:
                F_rho = F_rho + dt * dFx
                F_rt = F_rt + dt * dGx
            if hs_lat is not None:
                F_rt = F_rt + dt * eng.temp_forcing_hs(hs_lat, S.exner_h, S.theta_h, S.rho_h)                         # :1831-1834
            # entropy residual from the (rho theta) and rho residuals :1836-1842
            t1 = mv("CONST_RHO_INV", F_rt, f1=S.rt_h, rows=nk) - mv("CONST_RHO_INV", F_rho, f1=S.rho_h, rows=nk)
            F_eta = mv("CONST", t1, rows=nk)
            # theta_h in W3 and eta_h :1844-1851
            th_w3 = mv("CONST_RHO_INV", mv("CONST", S.rt_h, rows=nk), f1=S.rho_h, rows=nk)
            eta = mv("CONST_INV", eng.column_eos(2, th_w3, None), rows=nk)
            d_w, d_rho, d_eta, d_exner = eng.solve_schur_eta(dt, th_w3, S.rho_h, eta, S.exner_h, F_w, F_rho, F_eta, F_exner)   # :1855
            # theta_j (before the update) and eta_j :1858-1865
            th_w3 = mv("CONST_RHO_INV", mv("CONST", S.rt_j, rows=nk), f1=S.rho_j, rows=nk)
            eta = mv("CONST_INV", eng.column_eos(2, th_w3, d_eta), rows=nk)
            S.velz_j = S.velz_j + d_w; S.rho_j = S.rho_j + d_rho; S.exner_j = S.exner_j + d_exner
            S.rt_j = mv("CONST_INV", eng.column_eos(3, S.rho_j, eta), rows=nk)                                        # :1871-1872
            return self._composed_norms_and_halves(S, d_exner, d_w, d_rho, d_eta, eta)

        def fused(S):
            """the same iteration on the fused entry points (orders 1..4): mimsem_column_newton_residual (2 launches),
            mimsem_column_solve_schur_eta (3), mimsem_column_newton_update (1) and the reduction of the norm partials; every statement of
            composed() has its counterpart inside those kernels"""
            add_rho = add_rt = None
            if horiz_forcing is not None:
                add_rho, add_rt = horiz_forcing(rho_i, S.rho_j, S.theta_l2_h)
            if hs_lat is not None:
                hs = eng.temp_forcing_hs(hs_lat, S.exner_h, S.theta_h, S.rho_h)                                      # :1831-1834
                add_rt = hs if add_rt is None else add_rt + hs
            F_w, F_rho, F_eta, F_exner, th_w3, eta, self._k2i = eng.newton_residual(
                dt, self.rayleigh or 0.0, S.theta_l2_h, S.exner_h, velz_i, S.velz_j, rho_i, S.rho_j, zv, rt_i, S.rt_j, S.rho_h, S.rt_h, S.exner_j,
                add_w=udwdx, add_rho=add_rho, add_rt=add_rt)
            if getattr(self, "keep_solve_args", False):     # (bench: the linear solve of this iteration again, alone, on the state it was given)
                self.last_solve_args = (dt, th_w3.clone(), S.rho_h.clone(), eta.clone(), S.exner_h.clone(), [F_w.clone(), F_rho.clone(), F_eta.clone(), F_exner.clone()])
            d_w, d_rho, d_eta, d_exner = eng.solve_schur_eta(dt, th_w3, S.rho_h, eta, S.exner_h, F_w, F_rho, F_eta, F_exner)   # :1855
            S.velz_h, S.rho_h, S.rt_h, S.exner_h, nrm = eng.newton_update(d_w, d_rho, d_eta, d_exner, velz_i, rho_i, rt_i, exner_i,
                                                                          S.velz_j, S.rho_j, S.rt_j, S.exner_j)
            if hasattr(eng, "max_norms"):
                return eng.max_norms(nrm)                                           # MaxNorm :228 for exner, w, rho, eta (two launches)
            cs = nrm.sum(dim=2)                                                     # [8, nEl]: column sums of squares
            return torch.sqrt(cs[0::2] / cs[1::2]).amax(dim=1)

        if self.fused and eng.mesh.n <= 4:
            def theta(S, blend):                                                    # diagTheta2 :1766, diagTheta_L2 :1773; blended :1896-1912
                if not blend:
                    return eng.diag_theta_blend(S.rho_j, S.rt_j)
                return eng.diag_theta_blend(S.rho_j, S.rt_j, blend2=S.theta_i, blendL=S.theta_l2_i, wa=0.5, wb=0.5)
            step = fused
        else:
            def theta(S, blend):
                th, thl = eng.diag_theta(1, S.rho_j, S.rt_j), eng.diag_theta(0, S.rho_j, S.rt_j)
                return (0.5 * th + 0.5 * S.theta_i, 0.5 * thl + 0.5 * S.theta_l2_i) if blend else (th, thl)
            step = composed
        return self._newton(x_i, maxit, tol, verbose, "eta", ("exner", "rho"), step, theta)                          # stop rule :1922

    @staticmethod
    def _composed_norms_and_halves(S, d_exner, d_w, d_rho, d_last, x_last):
        """what the update kernels of the fused routes leave, composed: the four max-norms of VertSolve::MaxNorm (:228; exner, w, rho and the
        loop's fourth variable) as a device tensor, and the half-time states of the updated iterate"""
        col = lambda dx, x: (torch.linalg.vector_norm(dx, dim=1) / torch.linalg.vector_norm(x, dim=1)).max()
        S.exner_h = 0.5 * S.exner_i + 0.5 * S.exner_j; S.velz_h = 0.5 * S.velz_i + 0.5 * S.velz_j
        S.rho_h = 0.5 * S.rho_i + 0.5 * S.rho_j; S.rt_h = 0.5 * S.rt_i + 0.5 * S.rt_j
        return torch.stack([col(d_exner, S.exner_j), col(d_w, S.velz_j), col(d_rho, S.rho_j), col(d_last, x_last)])

    def _newton(self, x_i, maxit, tol, verbose, last, stop, step, theta):
        """The loop of both solves on either route.  x_i = (velz_i, rho_i, rt_i, exner_i).  The state S holds them, the iterate x_j (clones),
        the half-time fields x_h and theta_i / theta_l2_i / theta_h / theta_l2_h (the _l2 ones None where the loop has none).  step(S) runs one
        iteration up to and including the update of x_j and x_h and returns the four max-norms (exner, w, rho, `last`) as a device tensor;
        theta(S, blend) diagnoses theta of x_j -> (theta2, theta_l2 | None), blended half and half with theta_i where blend.  stop: the norms
        that must be below tol.  Leaves history, k2i_z (of the last iteration's self._k2i), theta_h, theta_l2_h and exner_h in self.*"""
        S = types.SimpleNamespace()
        S.velz_i, S.rho_i, S.rt_i, S.exner_i = x_i
        S.velz_j, S.rho_j, S.rt_j, S.exner_j = (x.clone() for x in x_i)                                   # :1099-1102
        S.velz_h, S.rho_h, S.rt_h, S.exner_h = x_i                                                        # :1112-1117 (never written in place)
        S.theta_i, S.theta_l2_i = theta(S, False)
        S.theta_h, S.theta_l2_h = S.theta_i, S.theta_l2_i
        self.history = []
        self._k2i = None
        keys = ("exner", "w", "rho", last)
        for itt in range(1, maxit + 1):
            nv = self.eng.allreduce(step(S), op="max")                                                    # MPI_Allreduce(MAX) :1915-1918, :1195-1198
            # (the theta diagnosis does not depend on the norms: launched BEFORE the host waits for them, it runs under the read-back)
            S.theta_h, S.theta_l2_h = theta(S, True)
            norms = dict(zip(keys, nv.tolist()))
            self.history.append(norms)
            if verbose:
                print("\t%d:\t" % itt + "\t".join("|d_%s|/|%s|: %.6e" % (k, k, norms[k]) for k in keys))
            if all(norms[k] < tol for k in stop):
                break
        self.k2i_z = float(self._k2i.sum()) / SCALE if self._k2i is not None else 0.0                     # :415-416, last iteration
        self.theta_h, self.exner_h = S.theta_h, S.exner_h
        if S.theta_l2_h is not None:
            self.theta_l2_h = S.theta_l2_h
        return S.velz_j, S.rho_j, S.rt_j, S.exner_j

    # ---- the other vertical implicit solve: the caller of solve_schur_column_3, the vertical half of Euler::Strang -----------------------
    def assemble_residual(self, theta, Pi, velz1, velz2, rho1, rho2, zv):
        """eul/VertSolve.cpp:386-430 -> (fw, F, G); theta on the nk+1 INTERFACES (AssembleLinearWithTheta), Pi / rho on levels, velz on the
        nk-1 interfaces.  Leaves F * tA1 (the integrand of k2i_z, :415) in self._k2i"""
        nk, nm, dt = self.nk, self.nk - 1, self.dt
        F = self.diagnose_F_z(velz1, velz2, rho1, rho2)
        Phi = self.diagnose_Phi_z(velz1, velz2, zv)
        fw = self._mv("LINEAR", velz2, rows=nm) - self._mv("LINEAR", velz1, rows=nm)
        fw += dt * self.V01(Phi)                                            # bernoulli function term
        tA2 = self._mv("LINEAR_INV", self.V01(self._mv("CONST", Pi, rows=nk)), rows=nm)     # pressure gradient
        tA1 = self._mv("LINEAR_THETA", tA2, f1=theta, rows=nm)
        fw += dt * tA1
        self._k2i = F * tA1                                                 # kinetic to internal energy power, entry by entry
        G = self._mv("LINEAR_INV", self._mv("LINEAR_THETA", F, f1=theta, rows=nm), rows=nm)
        if self.rayleigh:
            fw += 0.5 * dt * self.rayleigh * (self._mv("RAYLEIGH", velz2, rows=nm) + self._mv("RAYLEIGH", velz1, rows=nm))
        return fw, F, G

    def solve_schur_2(self, velz_i, rho_i, rt_i, exner_i, zv, horiz_forcing=None, udwdx=None, hs_lat=None, maxit=20, tol=1.0e-12,
                      schur3_flags=0, verbose=False, fused=None, theta_up=False, vert_mom_vort=None):
        """VertSolve::solve_schur_2 (eul/VertSolve.cpp:1059-1246) for EVERY column at once: Newton iterations on (w, rho, rt, Pi) with
        solve_schur_column_3 as the linear solve, all state in the "vertical" layout [nEl][slots*n2e] (L2Vecs::vz).

        horiz_forcing(rho_i, rho_j, theta_h) -> (dFx, dGx): HorizSolve::advection_rhs (:1124) in the vertical layout ([nEl][nk*n2e]);
        theta_h is on the nk+1 interfaces; the two join dF_z / dG_z BEFORE the VB product.  udwdx: optional [nEl][(nk-1)*n2e] (:1134).
        hs_lat: latitude of the quadrature points [nEl][mp12] switches the Held-Suarez temperature forcing on (:1151-1154).
        schur3_flags: passed to solve_schur_3 (3 with rayleigh = 0: the box twin's solve).  fused: None = the default route of this order.
        theta_up / vert_mom_vort: the loop of the box twin (box/VertSolve.cpp:1264-1458; with schur3_flags = 3, rayleigh = 0, no hs_lat).
        theta_up: theta_i / theta_j come from diagTheta2 with the test functions upwinded by velz_i / velz_j over 0.25 dt (box :1312, :1394;
        Engine.diag_theta_wup, orders 1..4, needs |0.25 dt w| < 1).  vert_mom_vort(velz_j) -> uuz [nEl][(nk-1)*n2e] (VortDiag.vert_mom_vort
        bound to u2l): with udwdx it makes the term time-centred, F_w += 0.5 dt udwdx + 0.5 dt uuz_j (box :1343-1346), uuz_j = udwdx in
        the first iteration (:1326) and recomputed from velz_j at the end of each (:1403).
        Stops when the exner, rho AND rt norms are below tol (:1202).  Returns (velz, rho, rt, exner) at the new time level and leaves
        theta_h / exner_h (what Euler::Strang reads), the per-iteration max-norms (history: exner, w, rho, rt) and k2i_z in self.*"""
        eng, nk, dt = self.eng, self.nk, self.dt
        fused = self.fused2 if fused is None else (fused and eng.mesh.n <= 4)       # (above order 4 the entries are unsupported: composed)
        x_i = (velz_i, rho_i, rt_i, exner_i)
        centred = udwdx is not None and vert_mom_vort is not None
        uuz_j = udwdx                                                                                   # box :1326

        def step(S):
            dFx, dGx = horiz_forcing(rho_i, S.rho_j, S.theta_h) if horiz_forcing is not None else (None, None)      # :1124
            hs = eng.temp_forcing_hs(hs_lat, S.exner_h, S.theta_h, S.rho_h) if hs_lat is not None else None        # :1152
            if fused:
                F_w, F_rho, F_rt, F_exner, self._k2i = eng.newton2_residual(
                    dt, self.rayleigh or 0.0, S.theta_h, S.exner_h, velz_i, S.velz_j, rho_i, S.rho_j, zv, rt_i, S.rt_j, S.exner_j,
                    add_w=0.5 * udwdx + 0.5 * uuz_j if centred else udwdx, add_rho_pre=dFx, add_rt_pre=dGx, add_rt_post=hs)
            else:
                F_w, F_z, G_z = self.assemble_residual(S.theta_h, S.exner_h, velz_i, S.velz_j, rho_i, S.rho_j, zv)     # :1131
                if centred:
                    F_w = F_w + 0.5 * dt * udwdx + 0.5 * dt * uuz_j                                        # box :1343-1346
                elif udwdx is not None:
                    F_w = F_w + dt * udwdx                                                                 # :1134
                F_exner = eng.column_eos(0, S.rt_j, S.exner_j)                                             # Assemble_EOS_Residual :1135
                dF_z = S.rho_j + dt * self.V10(F_z) - rho_i                                                # :1137-1142
                dG_z = S.rt_j + dt * self.V10(G_z) - rt_i
                if dFx is not None:
                    dF_z = dF_z + dt * dFx                                                                 # :1145-1146
                    dG_z = dG_z + dt * dGx
                F_rho = self._mv("CONST", dF_z, rows=nk)                                                   # :1148-1149
                F_rt = self._mv("CONST", dG_z, rows=nk)
                if hs is not None:
                    F_rt = F_rt + dt * hs                                                                  # :1153
            d_w, d_rho, d_rt, d_exner = eng.solve_schur_3(dt, S.theta_h, S.velz_h, S.rho_h, S.rt_h, S.exner_h, F_w, F_rho, F_rt, F_exner,
                                                          flags=schur3_flags)                              # :1156
            if fused:
                S.velz_h, S.rho_h, S.rt_h, S.exner_h, nrm = eng.newton2_update(d_w, d_rho, d_rt, d_exner, velz_i, rho_i, rt_i, exner_i,
                                                                               S.velz_j, S.rho_j, S.rt_j, S.exner_j)     # :1159-1183
                return eng.max_norms(nrm)                                                                  # MaxNorm :228 (two launches)
            S.velz_j = S.velz_j + d_w; S.rho_j = S.rho_j + d_rho; S.rt_j = S.rt_j + d_rt; S.exner_j = S.exner_j + d_exner
            return self._composed_norms_and_halves(S, d_exner, d_w, d_rho, d_rt, S.rt_j)

        def theta(S, blend):
            """diagTheta2 of the iterate (:1105, box :1312), blended with theta_i (:1186-1191, box :1394-1399); this loop has no theta_l2"""
            nonlocal uuz_j
            bl = dict(blend2=S.theta_i, wa=0.5, wb=0.5) if blend and fused else {}
            if theta_up:
                th = eng.diag_theta_wup(0.25 * dt, S.rho_j, S.rt_j, S.velz_j, **bl)
            elif fused:
                th, _ = eng.diag_theta_blend(S.rho_j, S.rt_j, wantL=False, **bl)
            else:
                th = eng.diag_theta(1, S.rho_j, S.rt_j)
            if blend and not fused:
                th = 0.5 * th + 0.5 * S.theta_i
            if blend and centred:
                uuz_j = vert_mom_vort(S.velz_j)                                                            # AssembleVertMomVort, box :1403
            return th, None
        return self._newton(x_i, maxit, tol, verbose, "rt", ("exner", "rho", "rt"), step, theta)           # stop rule :1202
