"""Rotating shallow water: one Picard/Rosenbrock time step on the device -- the host-side mirror of the reference's
SWEqn (src/SWEqn_Picard.cpp), SURVEY 8(f) row N3.  Every matrix of the reference (M0, M1, M2, M1h, M0h, K, R, R_up, the
packed [u,h] operator A) is applied matrix-free through the C-ABI engine; the KSP solves are device Krylov iterations.

src/ flavour: no SCALE, no layer thickness (the engine runs with nk = 1 and unit thickness), signed Jacobian determinant.
Single GPU, global numbering: the reference's local (`*l`) and global vectors coincide, so its VecScatters are identities."""
import math
import os

import numpy as np
import torch

from ._switches import experiment

from .checks import CheckLog, accepted, rate_steps
from .geom import gll_weights
from .krylov import (ChebyshevMass, GraphedChebyshev, GraphedGMRES, GraphedRichardson, arnoldi_ritz, chebyshev_ellipse_coefs, chebyshev_ellipse_rate,
                     edge_sharing_weights, element_block_preconditioner, gmres, lanczos_bounds, pcg_engine, ritz_margins, seeded_randn)

RAD_EARTH = 6371220.0          # src/SWEqn_Picard.cpp:22-23
RAD_SPHERE = 6371220.0
H_MEAN = 1.0e+4                # :27
ROS_ALPHA = 0.5                # :29
UP_TAU = 0.5                   # :30


class SWEqn:
    def __init__(self, eng, quad_coords, krylov_rtol=1e-14, use_graphs=True):
        """eng: Engine over the whole sphere (numbering="global", nk=1, unit thickness); quad_coords: [nq, 3] xyz of the
        quadrature-point grid in the engine's quad-grid numbering (Geom::x)."""
        assert eng.nk == 1
        self.eng, self.rtol = eng, krylov_rtol
        self.grav = 9.80616 * (RAD_SPHERE / RAD_EARTH)          # :52
        self.omega = 7.292e-5                                    # :53
        self.step = 0
        self.n1, self.n2 = eng.sizes[1], eng.sizes[2]
        xq = torch.as_tensor(quad_coords, dtype=torch.float64, device=eng.device)
        self.lat = torch.asin(xq[:, 2] / RAD_SPHERE)
        self.m0 = eng.pvec(0, 1, 1.0)                            # M0 is diagonal (collocated 0-forms): Pmat as a vector
        self.m1_pre = element_block_preconditioner(eng, eng.element_matrices("UMAT"))     # of M1 (the reference: PCBJACOBI, one block per element, :88-90)
        self.m2_inv = eng.element_matrices("WMATINV").view(eng.nEl, eng.n2e, eng.n2e)            # M2 is element-block diagonal: its exact inverse, built once
        self.coriolis()
        self.A_dt = None
        self.its = {}
        self.dist = hasattr(eng, "halo")                             # a DistEngine: this rank's patches + the halo plans
        self.graphs = use_graphs and not self.dist                  # hipGraph recording is single-rank (the exchanges are not recorded)
        # ... but the FIXED-LENGTH solves are exactly what a sharded run wants (round 6): a Chebyshev step needs its operator and
        # preconditioner results completed over the halo and NOTHING else -- no inner product, hence no all-reduce inside any solve; the check
        # norms of a whole Picard iteration are ownership-weighted partial sums reduced ONCE (_PicardGraph.replay)
        self.fixed = use_graphs
        self.recalibrations = 0             # times the spectral regions were estimated again after a missed check (self-healing)
        self.fixed_iterations = 0           # Picard iterations taken in the fixed-length mode / on the adaptive (Krylov) path
        self.adaptive_iterations = 0
        self._misses = 0
        self._gA = None
        self._pcA = None
        self._gq = None
        self._rq = None
        self._rM1 = None
        self._guess = {}
        self._m0fg = None
        self.chunk = int(experiment("MIMSEM_SW_CHUNK", "10"))
        self.fused_sweeps = experiment("MIMSEM_SW_FUSED_SWEEPS", "1") == "1"
        self.warm_start = experiment("MIMSEM_SW_WARM_START", "1") == "1"
        # Initial guesses of the nested solves from the counterpart solves of the previous steps (round 5 experiment, OFF): every solve of a
        # step has a counterpart a step ago -- the same diagnostic, the same Picard iteration.  MIMSEM_SW_EXTRAPOLATE=2 starts from the linear
        # extrapolation 2 x(n-1) - x(n-2) of the last two counterparts, 1 from the last one, 0 (default) from what round 4 did (the last
        # solution of the same diagnostic; zero for the [u|h] system).  Measured (profiles/r05_sw_extrapolate_ab.txt): the Picard increments
        # of successive steps are NOT close -- |P (b - A x0)| / |P b| = 0.5 ... 1.8 for the extrapolated guess of the [u|h] solve on the
        # Galewsky run (dt = 360 s resolves the grid-scale gravity waves with 2.5 steps per period: the increments oscillate) -- GMRES needs
        # its 25-26 iterations either way and the step is 0-6 % slower.  Kept as the record of the experiment.
        self.extrapolate = int(experiment("MIMSEM_SW_EXTRAPOLATE", "0"))
        # Polynomial preconditioning of the [u|h] solve (round 5): d Richardson steps on the coupled element blocks as ONE application of the
        # preconditioner, P_d = sum_{i<d} (I - P A)^i P -- an Arnoldi step then costs d operator passes but ONE orthogonalisation (4 launches +
        # a host synchronisation, ~28 of the ~43 us of a step), and GMRES needs ~1/d of the iterations where I - P A contracts.
        # MIMSEM_SW_POLY=d (1 = round 4's plain P; default 2).  Measured (scripts/ab_sw_poly.sh, profiles/r05_sw_poly_ab.txt): GMRES iterations
        # 26 -> 16 / 13 / 11 for d = 2 / 3 / 4, config 3 211.9 -> 222.7 / 222.1 / 220.3 steps/s, config 2 16.1 -> 16.1 / 16.4 / 16.1; error norms
        # and conservation drifts unchanged to 12 digits.  The iterations fall more slowly than 1/d (I - P A is not a strong contraction on the
        # gravity-wave part of the spectrum), so the operator passes grow 26 -> 32 / 39 / 44 while the orthogonalisations shrink: d = 2 it is.
        self.poly = max(1, int(experiment("MIMSEM_SW_POLY", "2")))
        # Round 5: the [u|h] solve WITHOUT a Krylov method.  Under the coupled element blocks the spectrum of P A is a real interval to within
        # a few per cent (Ritz values on the config-3 sphere, dt = 360 s: Re in [0.347, 1.184], |Im| <= 0.047; scripts/exp/sw_spectrum.py), so
        # a Chebyshev semi-iteration with a FIXED step count applies (krylov.GraphedChebyshev): ~30 steps of {P A d: 3 launches, one fused
        # vector update} in ONE hipGraph replay with ONE scalar read, against 16-26 Arnoldi steps of 8 launches and a host synchronisation
        # each.  The interval comes from 40 Arnoldi steps once per dt (set-up); a solve whose recurrence residual misses the tolerance is
        # finished by the GMRES from the iterate reached.  MIMSEM_SW_CHEB=0 selects the GMRES alone.
        self.cheb = os.environ.get("MIMSEM_SW_CHEB", "1") == "1"
        self._cA = None
        # ... and with every nested solve of a Picard iteration of FIXED length (Chebyshev for the [u|h] system, the 1-form mass and the
        # upwinded lumped 0-form mass) the WHOLE iteration -- residual assembly, its solves, the [u|h] solve, the update, every check norm --
        # is ONE hipGraph: one replay and one read of a handful of scalars per Picard iteration, no Python between the ~450 launches
        # (MIMSEM_SW_GRAPH_ITER=0: the nested solves each in their own graph, Python in between, as before).
        self.graph_iter = os.environ.get("MIMSEM_SW_GRAPH_ITER", "1") == "1"
        self._inline = None                 # the _PicardGraph that is recording / warming up: nested solves run inline and log their check norms
        self._pg = None
        self._hist = {}
        self.richardson = experiment("MIMSEM_SW_RICHARDSON", "1") == "1"
        self.coupled_pc = experiment("MIMSEM_SW_PC", "coupled") == "coupled"

    # ---- operator applies (src flavour: scale 1, flags 0) ---------------------------------------------------
    def _guess_for(self, key, shape):
        """initial guess of the solve `key` from the solutions its counterparts had in the last two steps (None: start from P^-1 b / zero)"""
        if not self.warm_start or self.extrapolate <= 0:
            return None
        h = self._hist.get(key)
        if not h or h[-1].shape != shape:
            return None
        if self.extrapolate >= 2 and len(h) == 2 and h[0].shape == shape:
            return torch.add(h[1], h[1]).sub_(h[0])
        return h[-1]

    @staticmethod
    def _base(key):
        """"F0", "F1" -> "F" (what self.its and the round-4 guesses are keyed by); "M1" stays"""
        return key if key == "M1" else key.rstrip("0123456789")

    def _remember(self, key, x):
        if self.extrapolate > 0:
            h = self._hist.setdefault(key, [])
            h.append(x)
            del h[:-2]

    def M1(self, u): return self.eng.apply("UMAT", u)
    def M2(self, h): return self.eng.apply("WMAT", h)
    def M1h(self, h, u, out=None, alpha=1.0, accum=False):
        return self.eng.apply("UHMAT", u, f=h, alpha=alpha, flags=2 if accum else 0, out=out)
    def K(self, ul, u): return self.eng.apply("WTQUMAT", u, f=ul)
    def R(self, q, u): return self.eng.apply("ROTMAT", u, f=q)
    def R_up(self, q, ul, dt, u): return self.eng.apply_up("ROTMAT_UP", u, q, ul, fac=UP_TAU, dt=dt)
    def E(self, name, x): return self.eng.incidence(name, x)

    def precond_M1(self, r, out=None):
        return self.eng.blocks_apply(1, self.m1_pre, r, transpose=True, out=out)        # symmetric blocks: the coalesced read order

    def solve_M1(self, b, key="M1"):
        """KSPSolve(ksp, b, x) on M1 (:84-92).  Single rank: hipGraph-captured preconditioned Richardson sweeps (P^-1 M1 is within
        ~10 % of the identity); otherwise / if they do not contract: SPD => preconditioned CG reaches the same solution"""
        if self._inline is not None:
            return self._inline.m1(b)
        if self.graphs and self.cheb and self.eng.mesh.n <= 5 and self.fused_sweeps and not hasattr(self.eng, "halo") and \
                experiment("MIMSEM_SW_CHEB_M1", "1") == "1":
            # round 5: a FIXED-length Chebyshev semi-iteration on the fused block sweep (krylov.ChebyshevMass: 3 launches per step, spectrum of
            # P M1 from 25 Lanczos steps once), the whole solve with its two norms in ONE hipGraph replay -- ~15 steps where the Richardson
            # sweeps below take 20 and a host read per chunk of 10
            res = self._solve_M1_chebyshev(b)
            if res is not None:
                self.its[self._base(key)] = res[1]
                self._guess[self._base(key)] = res[0]
                return res[0]
        if self.graphs and self.richardson:
            if self._rM1 is None or self._rM1.x.shape != b.shape:
                if self.eng.mesh.n <= 5 and self.fused_sweeps:
                    cm = self.m1_pre.transpose(1, 2).contiguous()          # column-major blocks for the fused three-launch sweep
                    self._rM1 = GraphedRichardson(self.eng, tuple(b.shape), chunk=self.chunk,
                                                  sweep=lambda x, rhs, upd: self.eng.block_richardson_sweep("UMAT", cm, x, rhs, upd=upd))
                else:
                    self._rM1 = GraphedRichardson(self.eng, tuple(b.shape), lambda x, rhs: self.precond_M1(rhs - self.M1(x)), chunk=self.chunk)
            if self.extrapolate > 0:
                x0 = self._guess_for(key, b.shape)
            else:
                x0 = self._guess.get(self._base(key)) if self.warm_start else None      # (round 4) the previous solution of the same diagnostic: a nearby system
                x0 = x0 if (x0 is not None and x0.shape == b.shape) else None
            res = self._rM1.solve(b, self.precond_M1, rtol=self.rtol, x0=x0)
            if res is not None:
                self.its[self._base(key)] = res[1]
                self._guess[self._base(key)] = res[0]
                self._remember(key, res[0])
                return res[0]
        with self.eng.space(1):
            x, its = pcg_engine(self.eng, self.M1, b, self.precond_M1, rtol=self.rtol, maxit=1000, check_every=2)
        self.its[self._base(key)] = its
        return x

    def _solve_M1_chebyshev(self, b):
        st = getattr(self, "_cM1", None)
        if st is None or st["b"].shape != b.shape:
            cm = self.m1_pre.transpose(1, 2).contiguous()
            rb = seeded_randn(b.shape, 4321, self.eng.device)
            lmin, lmax = lanczos_bounds(self.M1, self.precond_M1, rb, its=25)
            ch = ChebyshevMass(self.eng, lambda x, rhs, p, al, be, upd: self.eng.block_chebyshev_sweep("UMAT", cm, x, rhs, p, al, be, upd=upd),
                               lmin, lmax, rtol=self.rtol)
            st = {"ch": ch, "b": torch.zeros_like(b), "x": torch.zeros_like(b), "nrm": torch.zeros(2, dtype=torch.float64, device=self.eng.device),
                  "graph": None, "bad": 0}

            def run():
                c = self.precond_M1(st["b"])
                self.eng.rowdot(c.reshape(1, -1), c.reshape(1, -1), out=st["nrm"][1:2])
                st["x"].copy_(ch.solve(st["b"], want_residual=True))
                self.eng.rowdot(ch.upd.reshape(1, -1), ch.upd.reshape(1, -1), out=st["nrm"][0:1])      # the last preconditioned residual P (b - M1 x)
            st["run"] = run
            self._cM1 = st
        if st["bad"] >= 2:
            return None
        st["b"].copy_(b)
        if st["graph"] is None:
            st["graph"], _ = self.eng.capture(st["run"])
        st["graph"].replay()
        z2, c2 = CheckLog.read(st["nrm"])[0].tolist()
        # (the residual the last sweep saw belongs to the iterate BEFORE its update: one more contraction lies between it and the result)
        if not accepted(z2, c2, 30.0 * self.rtol)[0]:
            st["bad"] += 1
            return None
        return st["x"].clone(), st["ch"].steps

    # ---- diagnostics ------------------------------------------------------------------------------------------
    def coriolis(self):
        """:186-233: f = 2 Omega sin(lat) at the quadrature points, projected onto the 0-forms"""
        fq = (2.0 * self.omega * torch.sin(self.lat)).unsqueeze(0)
        self.fg = self.eng.apply("PTQ", fq) / self.m0

    def curl(self, u):
        """:236-250: w = M0^-1 E01 M1 u"""
        return self.E("E01", self.M1(u)) / self.m0

    def F_rhs(self, ui, uj, hi, hj):
        """the right-hand side of diagnose_F: 1/3 M1h(hi) ui + 1/6 M1h(hi) uj + 1/6 M1h(hj) ui + 1/3 M1h(hj) uj"""
        loc = getattr(self.eng, "eng", self.eng)                   # local partial sums, one halo reduction
        # M1h is LINEAR in its thickness field: two applies on hi/3 + hj/6 and hi/6 + hj/3 (two small combines on 2-forms) instead of four applies
        # -- 6 launches instead of 8 (round 6, late; the step is launch-bound)
        hu = loc.apply("UHMAT", ui, f=loc.combine(hi, 1.0 / 3.0, beta=1.0 / 6.0, c=hj))
        loc.apply("UHMAT", uj, f=loc.combine(hi, 1.0 / 6.0, beta=1.0 / 3.0, c=hj), flags=2, out=hu)
        self.eng.complete(1, hu)
        return hu

    def diagnose_F(self, ui, uj, hi, hj, key="F"):
        """:253-284: F = M1^-1 (1/3 M1h(hi) ui + 1/6 M1h(hi) uj + 1/6 M1h(hj) ui + 1/3 M1h(hj) uj)"""
        return self.solve_M1(self.F_rhs(ui, uj, hi, hj), key)

    def q_rhs(self, u, h):
        """the right-hand side and the lumped diagonal of diagnose_q: M0 f + E01 M1 u, Phmat::assemble(h)"""
        if self._m0fg is None:
            self._m0fg = self.m0 * self.fg
        return self._m0fg + self.E("E01", self.M1(u)), self.eng.pvec(0, 1, 1.0, h2=h)

    def diagnose_Phi(self, ui, uj, hi, hj):
        """:289-320 (integral form): 1/3 K(ui) ui + 1/3 K(ui) uj + 1/3 K(uj) uj + g/2 M2 (hi + hj)"""
        # (the factors ride in the applies' alpha, the sums in their accumulate form, M2 is applied once to hi + hj: 4 launches + 1
        # instead of 5 applies and 9 framework kernels -- the step is launch-bound)
        Phi = self.eng.apply("WTQUMAT", ui, f=ui, alpha=1.0 / 3.0)
        self.eng.apply("WTQUMAT", uj, f=ui, alpha=1.0 / 3.0, flags=2, out=Phi)
        self.eng.apply("WTQUMAT", uj, f=uj, alpha=1.0 / 3.0, flags=2, out=Phi)
        self.eng.apply("WMAT", hi + hj, alpha=self.grav / 2.0, flags=2, out=Phi)
        return Phi

    def diagnose_q(self, dt, u, h, key="q"):
        """:322-341: M0h q = M0 f + E01 M1 u ; M0h upwinded (Phmat::assemble_up) when dt > 1e-6"""
        rhs, m0h = self.q_rhs(u, h)                              # (Phmat::assemble(h) is diagonal)
        if dt > 1.0e-6 and self._inline is not None:
            return self._inline.q(rhs, m0h, h, u, dt)
        if dt > 1.0e-6:
            A = lambda q: self.eng.apply_up("PHMAT_UP", q, h, u, fac=UP_TAU, dt=dt)
            if self.graphs:
                # the Arnoldi step is captured once per dt on FIXED coefficient buffers (a hipGraph records pointers, not values);
                # every later solve copies its (h, u, lumped M0h) in and replays
                if self._gq is None or self._gq[0] != dt:
                    bh, bu, bm = torch.empty_like(h), torch.empty_like(u), torch.empty_like(m0h)
                    body = lambda v: self.eng.apply_up("PHMAT_UP", v, bh, bu, fac=UP_TAU, dt=dt) / bm
                    self._gq = (dt, GraphedGMRES(self.eng, self.eng.sizes[0], body, restart=30), bh, bu, bm)
                _, g, bh, bu, bm = self._gq
                bh.copy_(h); bu.copy_(u); bm.copy_(m0h)
                if self.richardson:
                    if self._rq is None or self._rq[0] != dt:
                        if self.fused_sweeps:
                            bmi = torch.empty_like(bm)
                            tau = 1.0 / (1.0 / (UP_TAU * dt))
                            swp = lambda x, b, upd: self.eng.richardson_sweep("PHMAT_UP", x, b, bmi, f=bh, u=bu, tau=tau, upd=upd)
                            self._rq = (dt, GraphedRichardson(self.eng, tuple(rhs.shape), chunk=self.chunk, sweep=swp), bh, bmi)
                        else:
                            upd = lambda x, b: (b - self.eng.apply_up("PHMAT_UP", x, bh, bu, fac=UP_TAU, dt=dt)) / bm
                            self._rq = (dt, GraphedRichardson(self.eng, tuple(rhs.shape), upd, chunk=self.chunk), bh, None)
                    if self._rq[2] is bh:
                        if self._rq[3] is not None:
                            torch.reciprocal(m0h, out=self._rq[3])
                        x0 = self._guess_for(key, rhs.shape) if self.extrapolate > 0 else (self._guess.get("q") if self.warm_start else None)
                        res = self._rq[1].solve(rhs, lambda r: r / m0h, rtol=self.rtol, x0=x0)
                        if res is not None:
                            self.its["q"] = res[1]
                            self._guess["q"] = res[0]
                            self._remember(key, res[0])
                            return res[0]
                q, its, _ = g.solve(A, rhs, lambda r: r / m0h, rtol=self.rtol, maxit=1000)
                self.its["q"] = its
                return q
            with self.eng.space(0):
                q, its, _ = gmres(A, rhs, precond=lambda r: r / m0h, rtol=self.rtol, restart=30, maxit=1000, eng=self.eng)
            self.its["q"] = its
            return q
        return rhs / m0h

    # ---- the packed [u,h] system ---------------------------------------------------------------------------------
    def pack(self, u, h): return torch.cat([u, h], dim=1)
    def unpack(self, x): return x[:, :self.n1].contiguous(), x[:, self.n1:].contiguous()

    def assemble_residual(self, ui, hi, uj, hj, dt, q_exact=False, bot=None, qi=None, qj=None, it=0, before_q=None, F=None):
        """:402-607.  qi / qj: potential vorticities already diagnosed from (ui, hi) / (uj, hj) -- the reference re-solves for qi in
        every Picard iteration although (ui, hi) is the fixed start-of-step state; solve() passes the first result back in.
        F: the mass flux when the caller has solved for it already (_PicardGraph: together with q, in shared launches)."""
        if F is None:
            F = self.diagnose_F(ui, uj, hi, hj, key="F%d" % it)      # (keys: the counterpart of a solve is the same Picard iteration of the last step)
        Phi = self.diagnose_Phi(ui, uj, hi, hj)
        if bot is not None:
            Phi = Phi + self.grav * self.M2(bot)
        # (sharded: E12 Phi, the rotational terms and M1 (uj - ui) are all LOCAL partial sums of 1-form results until the packed residual is
        #  complete -- they are added on the rank's own engine and completed over the halo ONCE, as the C++ host does; one rank: loc is eng)
        loc = getattr(self.eng, "eng", self.eng)
        fu = loc.incidence("E12", Phi)
        if q_exact:
            um, hm = torch.add(ui, uj).mul_(0.5), torch.add(hi, hj).mul_(0.5)
            q = self.diagnose_q(0.0, um, hm, key="qm%d" % it)
            loc.apply("ROTMAT", F, f=q, flags=2, out=fu)                                          # fu += R(q) F
        else:
            if before_q is not None:
                before_q()                     # (qi / qj were diagnosed on a parallel branch of the recorded graph: join it here)
            qi = self.diagnose_q(dt, ui, hi, key="qi") if qi is None else qi
            qj = self.diagnose_q(dt, uj, hj, key="qj%d" % it) if qj is None else qj
            loc.apply_up("ROTMAT_UP", F, qi, ui, fac=UP_TAU, dt=dt, alpha=0.5, flags=2, out=fu)            # fu += 1/2 R_up(qi, ui) F
            loc.apply_up("ROTMAT_UP", F, qj, uj, fac=UP_TAU, dt=dt, alpha=0.5, flags=2, out=fu)
        # the mass terms are linear: M1 (uj - ui) and M2 (hj - hi + dt E21 F) -- two applies instead of five; both halves of the packed
        # residual are written in place (no concatenation)
        res = torch.empty(ui.shape[0], self.n1 + self.n2, dtype=ui.dtype, device=ui.device)
        ru, rh = res[:, :self.n1], res[:, self.n1:]
        loc.apply("UMAT", uj - ui, out=ru)
        ru.add_(fu, alpha=dt)
        self.eng.complete(1, ru)
        self.eng.apply("WMAT", torch.add(hj - hi, self.E("E21", F), alpha=dt), out=rh)
        return res

    def apply_A(self, x, dt):
        """:622-725 without forming A: [[M1 + a dt R(f), a dt g E12 M2], [a dt H M2 E21, M2]] -- one fused element pass
        (mimsem_sw_operator_apply) + the 1-form gather; sharded: local partial sums, then one halo reduction"""
        eng, n1 = self.eng, self.n1
        loc = getattr(eng, "eng", eng)
        y = loc.sw_operator(ROS_ALPHA * dt, self.grav, H_MEAN, self.fg, x)
        eng.complete(1, y[:, :n1])
        return y

    def apply_A_composed(self, x, dt):
        """the same operator from the individual engine operators (the parity check of the fused kernel)"""
        eng, n1 = self.eng, self.n1
        loc = getattr(eng, "eng", eng)                             # sharded: add the LOCAL partial sums first, reduce the halo once
        u, h = x[:, :n1], x[:, n1:]                                # views of the packed vector (one row => contiguous)
        a = ROS_ALPHA * dt
        y = torch.empty_like(x)
        yu, yh = y[:, :n1], y[:, n1:]
        loc.apply("UMAT", u, out=yu)
        loc.apply("ROTMAT", u, f=self.fg, alpha=a, flags=2, out=yu)                       # += a R(f) u
        yu += (a * self.grav) * loc.incidence("E12", loc.apply("WMAT", h))
        eng.complete(1, yu)
        w = eng.incidence("E21", u)
        w *= a * H_MEAN
        w += h
        eng.apply("WMAT", w, out=yh)                                                      # M2 (a H E21 u + h)
        return y

    def _coupled_element_blocks(self, dt):
        """Element blocks of A itself, inverted: A_e = [[M1_e + a R_e(f), a g E12_e M2_e], [a H M2_e E21_e, M2_e]] with the element's
        own 2 n1e edges and n2e faces (E21_e = the +-1 face-edge stencil of one element, E12_e = -E21_e^T).  The preconditioner is
        P^-1 = sum_e R_e^T D_e A_e^-1 D_e R_e (D_e = 1/multiplicity on the edges, 1 on the faces): the gravity-wave coupling INSIDE
        an element is inverted exactly, which the block-diagonal {M1, M2} preconditioner ignores -- 62 -> ~20 GMRES iterations
        on the 24x24x6 sphere at dt = 360 s.  Stored column-major per element for mimsem_sw_blocks_apply."""
        eng = self.eng
        loc = getattr(eng, "eng", eng)
        n, n1e, n2e, nEl = eng.mesh.n, eng.n1e, eng.n2e, eng.nEl
        a = ROS_ALPHA * dt
        dev = eng.device
        em = loc.element_matrices("UMAT").view(nEl, 2, 2, n1e, n1e)
        M1e = em.permute(0, 1, 3, 2, 4).reshape(nEl, 2 * n1e, 2 * n1e)
        rot = loc.element_matrices("ROTMAT", f=self.fg[0].contiguous()).view(nEl, 2, n1e, n1e)       # UtQV (x rows, y cols), VtQU
        Re = torch.zeros_like(M1e)
        Re[:, :n1e, n1e:] = rot[:, 0]; Re[:, n1e:, :n1e] = rot[:, 1]
        M2e = loc.element_matrices("WMAT").view(nEl, n2e, n2e)
        E21 = torch.zeros(n2e, 2 * n1e, dtype=torch.float64, device=dev)
        for q in range(n2e):
            jj, ii = q % n, q // n
            E21[q, ii * (n + 1) + jj] = -1.0; E21[q, ii * (n + 1) + jj + 1] = 1.0
            E21[q, n1e + ii * n + jj] = -1.0; E21[q, n1e + (ii + 1) * n + jj] = 1.0
        Ae = torch.zeros(nEl, 2 * n1e + n2e, 2 * n1e + n2e, dtype=torch.float64, device=dev)
        Ae[:, :2 * n1e, :2 * n1e] = M1e + a * Re
        Ae[:, :2 * n1e, 2 * n1e:] = (a * self.grav) * (-E21.T) @ M2e
        Ae[:, 2 * n1e:, :2 * n1e] = (a * H_MEAN) * M2e @ E21
        Ae[:, 2 * n1e:, 2 * n1e:] = M2e
        d = torch.cat([edge_sharing_weights(eng), torch.ones(nEl, n2e, dtype=torch.float64, device=dev)], dim=1)
        C = d[:, :, None] * getattr(self.eng, "eng", self.eng).block_inverse(Ae) * d[:, None, :]
        return C.transpose(1, 2).contiguous()                     # column-major per element

    def _krylov_body1(self, dt):
        """v -> P A v with the plain (degree-1) preconditioner"""
        keep, self.poly = self.poly, 1
        try:
            return self._krylov_body(dt)
        finally:
            self.poly = keep

    def _krylov_body(self, dt):
        """v -> P A v for the graph-captured Arnoldi step: one fused call (three launches) when the coupled blocks are in use"""
        if self.eng.mesh.n <= 4 and self.coupled_pc and not hasattr(self.eng, "halo"):
            if self._pcA is None or self._pcA[0] != dt:
                self._pcA = (dt, self._coupled_element_blocks(dt))
            blocks = self._pcA[1]
            body1 = lambda v: self.eng.sw_operator_precond(ROS_ALPHA * dt, self.grav, H_MEAN, self.fg, blocks, v)
        else:
            body1 = lambda v: self.precond_A(self.apply_A(v, dt), dt)
        if self.poly <= 1:
            return body1

        def body(v):                                                  # P_d A v = (I - (I - P A)^d) v: w <- v, d times w <- w - P A w; v - w
            w = v
            for _ in range(self.poly):
                w = w - body1(w)
            return v - w
        return body

    def _krylov_body_orth(self, dt):
        """(v, V, k, h, out) -> out = P A v orthogonalised once against V[:k]: the body above with its 1-form gather folded into the first
        Gram-Schmidt pass (mimsem_sw_operator_precond_orthogonalize, round 4).  OPT-IN (MIMSEM_SW_FUSED_DOTS=1): one launch less per Arnoldi step and
        SLOWER -- every one of the k row-blocks of the dot pass repeats the gather (192-196 against 205-208 steps/s, profiles/r04_sw_cgs2_ab.txt);
        None otherwise, and where the fused body does not apply"""
        if not (self.eng.mesh.n <= 4 and self.coupled_pc and not hasattr(self.eng, "halo")) or experiment("MIMSEM_SW_FUSED_DOTS", "0") != "1":
            return None
        if self.poly > 1:
            return None                                               # (the fused form is the plain preconditioner's)
        if self._pcA is None or self._pcA[0] != dt:
            self._pcA = (dt, self._coupled_element_blocks(dt))
        blocks = self._pcA[1]
        return lambda v, V, k, h, out: self.eng.sw_operator_precond_orthogonalize(ROS_ALPHA * dt, self.grav, H_MEAN, self.fg, blocks, v, V, k, h, out)

    def precond_A(self, r, dt=None):
        """dt given (and order <= 4): the coupled element blocks above; otherwise block diagonal -- the element-block preconditioner
        on M1, the exact element-wise inverse on M2 (WmatInv)"""
        n1 = self.n1
        if dt is not None and self.eng.mesh.n <= 4 and self.coupled_pc:
            if self._pcA is None or self._pcA[0] != dt:
                self._pcA = (dt, self._coupled_element_blocks(dt))
            loc = getattr(self.eng, "eng", self.eng)
            z = loc.sw_blocks_apply(self._pcA[1], r)
            self.eng.complete(1, z[:, :n1])
            return z
        y = torch.empty_like(r)
        self.precond_M1(r[:, :n1], out=y[:, :n1])
        self.eng.blocks_apply(2, self.m2_inv, r[:, n1:], out=y[:, n1:])
        return y

    def solve(self, un, hn, dt, nits=99, q_exact=False, bot=None, verbose=False, restart=60):
        """:727-791: Picard iterations x += A^-1 (-f(x)) until |dx|/|x| < 1e-14 or nits"""
        if self.fixed and self.cheb and self.graph_iter and self.eng.mesh.n <= 4 and self.coupled_pc and self.fused_sweeps:
            out = self._solve_graphed(un, hn, dt, nits, q_exact, verbose, bot)
            if out is not None:
                return out
        ui, hi = un, hn                                                    # (read only: the iterate lives in x)
        uj, hj = un, hn
        x = self.pack(uj, hj)
        it, hist = 0, []
        qi = None if q_exact else self.diagnose_q(dt, ui, hi, key="qi")   # depends on the start-of-step state only
        while True:
            f = self.assemble_residual(ui, hi, uj, hj, dt, q_exact, bot, qi=qi, qj=qi if it == 0 else None, it=it)   # iteration 0: uj = ui, hj = hi
            if self.graphs:
                if self._gA is None or self._gA[0] != (dt, restart):       # the operator is fixed for a given dt: capture once
                    self._gA = ((dt, restart), GraphedGMRES(self.eng, self.n1 + self.n2, self._krylov_body(dt), restart=restart,
                                                            body_orth=self._krylov_body_orth(dt)))
                dx0 = None
                cheb_done = False
                if self.cheb and self.eng.mesh.n <= 4 and self.coupled_pc:
                    if self._cA is None or self._cA[0] != dt:
                        body1 = self._krylov_body1(dt)
                        ev = arnoldi_ritz(body1, self.n1 + self.n2, 40, self.eng.device)
                        lmin, lmax, imax = float(ev.real.min()), float(ev.real.max()), float(abs(ev.imag).max())
                        ok = lmin > 0.02 and imax <= 0.15 * (lmax - lmin)          # a real, positive interval (else: the GMRES)
                        step = None
                        if experiment("MIMSEM_SW_CHEB_FUSED", "1") == "1" and not hasattr(self.eng, "halo"):
                            blocks = self._pcA[1]                                   # (set by _krylov_body1: the coupled element blocks of this dt)
                            step = lambda ca, cb, x, r, d: self.eng.sw_operator_precond_chebyshev(ROS_ALPHA * dt, self.grav, H_MEAN, self.fg, blocks, ca, cb, x, r, d)
                        self._cA = (dt, GraphedChebyshev(self.eng, tuple(f.shape), body1, lambda r: self.precond_A(r, dt), lmin, lmax, rtol=self.rtol, step=step)
                                    if ok else None, (lmin, lmax, imax))
                    if self._cA[1] is not None:
                        res_c = self._cA[1].solve(-f)
                        if res_c is not None and res_c[1] > 0:
                            dx, its, res = res_c[0], res_c[1], res_c[2]
                            cheb_done = True
                        elif res_c is not None:
                            dx0 = res_c[0]                                          # short of the tolerance: the GMRES finishes from here
                # the increment of Picard iteration `it` is close to the one the same iteration produced a step ago (smooth flow)
                if dx0 is None:
                    dx0 = self._guess_for("A%d" % it, f.shape) if it < 8 else None
                pc = lambda r: self.precond_A(r, dt)
                if self.poly > 1:
                    body1 = self._krylov_body1(dt)

                    def pc(r, p1=pc):                                 # P_d r = sum_{i<d} (I - P A)^i P r
                        z = p1(r); acc = z
                        for _ in range(self.poly - 1):
                            z = z - body1(z); acc = acc + z
                        return acc
                if not cheb_done:
                    dx, its, res = self._gA[1].solve(lambda v: self.apply_A(v, dt), -f, pc, x0=dx0, rtol=self.rtol, maxit=1000)
                if it < 8:
                    self._remember("A%d" % it, dx)
            else:
                with self.eng.space("uh"):
                    dx, its, res = gmres(lambda v: self.apply_A(v, dt), -f, precond=lambda r: self.precond_A(r, dt), rtol=self.rtol,
                                         restart=restart, maxit=1000, eng=self.eng)
            self.its["A"] = its
            x = x + dx
            uj, hj = self.unpack(x)
            with self.eng.space("uh"):
                norm_x, norm_dx = self.eng.norm(x), self.eng.norm(dx)
            norm = norm_dx / norm_x
            hist.append(norm)
            if verbose:
                print("iteration: %d\t|x|: %.6e\t|dx|: %.6e\t|dx|/|x|: %.6e  (gmres %d)" % (it, norm_x, norm_dx, norm, its))
            it += 1
            if not (norm > 1.0e-14 and it < nits):
                break
        self.step += 1
        self.history = hist
        self.adaptive_iterations += len(hist)
        return uj, hj

    MAX_MISSES = 3

    def _solve_graphed(self, un, hn, dt, nits, q_exact, verbose, bot=None):
        """SWEqn::solve with one hipGraph replay per Picard iteration (_PicardGraph; sharded: the same launches eagerly with the halo exchanges in
        between and one all-reduce of the check norms).  SELF-HEALING (round 6): the spectral regions the fixed step counts rest on were
        estimated on the state of some earlier step (the upwinded q system follows the flow); when a check misses, they are estimated again
        from the CURRENT start-of-step state, the iteration is recorded again and the step retried once; only the step whose retry fails too
        runs on the adaptive path (None is returned), and only after MAX_MISSES such steps in a row does the object stay adaptive."""
        key = (dt, bool(q_exact), tuple(un.shape), bot is not None)
        for attempt in (0, 1):
            pg = self._pg
            if pg is None or pg.key != key:
                try:
                    pg = self._pg = _PicardGraph(self, dt, bool(q_exact), un, hn, has_bot=bot is not None, widen=1.0 + 0.5 * min(self._misses + attempt, 4))
                except _NoGraph:
                    self._pg = _PicardGraph.__new__(_PicardGraph); self._pg.key = key; self._pg.broken = True
                    return None
            if pg.broken:
                return None
            out = self._run_fixed(pg, un, hn, nits, verbose, bot)
            if out is not None:
                self._misses = 0
                return out
            if attempt == 0:
                self.recalibrations += 1
                self._pg = None                      # (estimated again from (un, hn) at the top of the loop)
        self._misses += 1
        if self._misses >= self.MAX_MISSES:
            pg.broken = True
        return None

    def _run_fixed(self, pg, un, hn, nits, verbose, bot):
        pg.ui.copy_(un); pg.hi.copy_(hn)
        if bot is not None:
            pg.bot.copy_(bot)                        # (a recording names buffers, not values: the topography the caller passes is copied in)
        pg.x[:, :self.n1].copy_(un); pg.x[:, self.n1:].copy_(hn)
        it, hist = 0, []
        while True:
            vals = pg.replay(first=(it == 0))
            ok, norm = pg.verify(vals, first=(it == 0))
            if not ok:
                pg.fails += 1
                self.last_miss = pg.last_miss
                return None
            hist.append(norm)
            if verbose:
                print("iteration: %d\t|dx|/|x|: %.6e  (fixed length)" % (it, norm))
            it += 1
            if not (norm > 1.0e-14 and it < nits):
                break
        self.its.update(pg.its)
        self.step += 1
        self.history = hist
        self.fixed_iterations += len(hist)
        return pg.x[:, :self.n1].clone(), pg.x[:, self.n1:].clone()

    # ---- conservation diagnostics (int0 :1202-1238, int2 :1240-1274, intE :1276-1323, writeConservation :1325-1359) ------------
    def conservation(self, u, h, bot=None):
        """mass = int2(h) = sum_q w det h_q;  vorticity = int0(curl u);  energy = 1/2 sum_q w det (g (h+b)^2 + h |u|^2);
        enstrophy = q^T M0h(h) q with q = diagnose_q(0, u, h).  The quadrature sums are written as the bilinear forms they are:
        int2(h) = 1^T (W^T diag(w)) h, energy = g/2 (h+b)^T M2 (h+b) + 1/2 u^T M1h(h) u (M2 = W^T diag(w/det) W, interp2_g = W h/det)."""
        eng = self.eng
        hb = h if bot is None else h + bot
        with eng.space(2):
            mass = float(eng.wsum(2, self._int2_weights() * h))
            pot = 0.5 * self.grav * float(eng.wsum(2, hb * self.M2(hb)))
        kin = 0.5 * float(eng.wsum(1, u * self.M1h(h, u)))
        w = self.curl(u)
        vort = float(eng.wsum(0, self.m0 * w))
        q = self.diagnose_q(0.0, u, h)
        enst = float(eng.wsum(0, q * (eng.pvec(0, 1, 1.0, h2=h) * q)))
        return dict(mass=mass, vorticity=vort, energy=pot + kin, enstrophy=enst)

    # ---- analytic-solution error norms (err0 :981-1060, err1 :1062-1145, err2 :1147-1200) ----------------------------------
    def _quad_measure(self):
        """w_q det_q per (element, quadrature point) and the quadrature-grid slot of each point"""
        if getattr(self, "_wd", None) is None:
            m = self.eng.mesh
            g1 = gll_weights(m.m)
            w2 = np.outer(g1, g1).ravel()
            self._wd = torch.as_tensor(m.det.reshape(m.nEl, -1) * w2[None, :], dtype=torch.float64, device=self.eng.device)
            self._iq = torch.as_tensor(np.asarray(m.indsq).reshape(m.nEl, -1), device=self.eng.device).long()
        return self._wd, self._iq

    def _norms(self, wd, err1, ref1, err2, ref2, mask=None):
        """[L1, L2, Linf] exactly as the reference accumulates them: sums of wd*|.| and wd*(.)^2 over all points, the largest
        wd*|err| with the wd*|ref| of THAT point -- and, across ranks, MPI_MAX of both separately (:1050-1052)."""
        if mask is not None:
            wd = wd * mask
        sums = torch.stack([(wd * err1).sum(), (wd * ref1).sum(), (wd * err2).sum(), (wd * ref2).sum()])
        li = (wd * err1).reshape(-1)
        k = torch.argmax(li)
        mx = torch.stack([li[k], (wd * ref1).reshape(-1)[k].abs()])
        sums = self.eng.allreduce(sums); mx = self.eng.allreduce(mx, op="max")
        return [float(sums[0] / sums[1]), float(torch.sqrt(sums[2] / sums[3])), float(mx[0] / mx[1])]

    def err0(self, w, wq):
        """err0(ug, fw, NULL, NULL): 0-form w [1, n0] against wq [nq] at the quadrature-grid points"""
        wd, iq = self._quad_measure()
        un = self.eng.interp_quad(0, w)[0]
        ua = wq[iq]
        return self._norms(wd, (un - ua).abs(), ua.abs(), (un - ua) ** 2, ua * ua)

    def err1(self, u, uq):
        """err1(ug, fu, fv, NULL): 1-form u [1, n1] against uq [nq, 2] (zonal, meridional)"""
        wd, iq = self._quad_measure()
        un = self.eng.interp_quad(1, u)[0]
        ua = uq[iq]
        d = un - ua
        return self._norms(wd, d.abs().sum(-1), ua.abs().sum(-1), (d * d).sum(-1), (ua * ua).sum(-1))

    def err2(self, h, hq):
        """err2(ug, fu): 2-form h [1, n2] against hq [nq]; points with |latitude| > 0.45 pi are skipped (:1167)"""
        wd, iq = self._quad_measure()
        un = self.eng.interp_quad(2, h)[0]
        ua = hq[iq]
        mask = (self.lat[iq].abs() <= 0.45 * math.pi).to(torch.float64)
        return self._norms(wd, (un - ua).abs(), ua.abs(), (un - ua) ** 2, ua * ua, mask)

    def _int2_weights(self):
        """sum_q w_q W[q][j] per 2-form DoF (= 1 up to round-off: the edge functions integrate to one and GLL is exact for them)"""
        if getattr(self, "_w2", None) is None:
            ones_q = torch.ones(1, self.eng.sizes["q"], dtype=torch.float64, device=self.eng.device)
            self._w2 = self.eng.apply("WTQ", ones_q)              # WtQmat applied to 1: W^T diag(w) 1
        return self._w2

    # ---- initial conditions (init1 :880-932, init2 :934-975) ---------------------------------------------------------
    def init1(self, uq):
        """uq: [nq, 2] zonal/meridional velocity at the quadrature-grid points -> 1-form u = M1^-1 UtQ uq"""
        b = self.eng.apply("UTQ", uq.reshape(1, -1).contiguous())
        return self.solve_M1(b, "init1")

    def init2(self, hq):
        """hq: [nq] -> 2-form h = M2^-1 WtQ hq (M2 is element-block diagonal: exact inverse)"""
        return self.eng.blocks_apply(2, self.m2_inv, self.eng.apply("WTQ", hq.reshape(1, -1).contiguous()))


class _NoGraph(Exception):
    pass


class _PicardGraph:
    """One Picard iteration of SWEqn::solve (src/SWEqn_Picard.cpp:751-765 with assemble_residual :402-607) as ONE hipGraph.  Every nested solve
    has a FIXED length -- Chebyshev semi-iterations whose step counts follow from spectral regions estimated once per dt: the [u|h] system
    (real interval, GraphedChebyshev), the 1-form mass (real interval, ChebyshevMass on the fused block sweep), the upwinded lumped 0-form
    mass (a vertical segment 1 +- i sigma: ellipse with imaginary foci, mimsem_op_chebyshev_sweep) -- so nothing inside needs the host.  Each
    solve logs {|last preconditioned residual|^2, |P b|^2} into a slot of one small device vector; after the replay the host reads that
    vector ONCE, checks every solve against its tolerance and takes |dx| / |x| for the Picard loop.  Two graphs: the first iteration of a step
    (also diagnoses q of the start-of-step state; uj = ui) and the later ones."""
    NSLOT = 16
    SPACE = {"M1": 1, "q": 0, "A": "uh", "picard": "uh"}          # the vector space of each kind of check (a DistEngine weights the norms by ownership)

    def __init__(self, S, dt, q_exact, un, hn, has_bot=False, widen=1.0):
        """widen >= 1: the safety margins around the estimated spectral regions, times widen (a re-estimate after a missed check asks for more)"""
        self.S, self.dt, self.q_exact = S, dt, q_exact
        self.dist = S.dist                   # sharded: local (ownership-weighted) check norms, one all-reduce per Picard iteration (replay)
        # ... recorded as a hipGraph all the same when the exchanges are kernels only (the one-sided transport of csrc/halo.hip: pack into the
        # neighbour's buffer, sequence flags, a device-side exchange counter); with a library or host transport the same launches run eagerly
        self.record = (not S.dist) or getattr(S.eng, "transport", None) == "peer"
        self.last_miss = None
        self.key = (dt, q_exact, tuple(un.shape), has_bot)
        self.bot = torch.zeros_like(hn) if has_bot else None          # bottom topography (SWEqn::solve's `bot`): a fixed buffer of the recording
        self.broken, self.fails = False, 0
        eng = S.eng
        dev = eng.device
        n1, n2, n0 = S.n1, S.n2, eng.sizes[0]
        self.ui, self.hi = torch.zeros_like(un), torch.zeros_like(hn)
        self.x = torch.zeros(un.shape[0], n1 + n2, dtype=torch.float64, device=dev)
        self.qi = torch.zeros(un.shape[0], n0, dtype=torch.float64, device=dev)
        self.log = CheckLog(eng, self.NSLOT)          # kinds: the keys of SPACE
        self.graphs = {}
        self.its = {}
        # ---- [u|h]: real interval of P A
        if S._pcA is None or S._pcA[0] != dt:
            S._pcA = (dt, S._coupled_element_blocks(dt))
        body1 = S._krylov_body1(dt)
        ev, ev25 = arnoldi_ritz(body1, n1 + n2, 40, dev, eng=eng, space="uh", earlier=25)
        lmin, lmax, imax = float(ev.real.min()), float(ev.real.max()), float(abs(ev.imag).max())
        # margins (round 6): three times what the ends moved between 25 and 40 Arnoldi steps, at least 1 % (rounds 5: 10 % / 5 % whatever the estimate's quality)
        mgA = ritz_margins(lmin, lmax, 3.0 * abs(lmin - float(ev25.real.min())) / lmin, 3.0 * abs(lmax - float(ev25.real.max())) / lmax, widen)
        if not (lmin > 0.02 and imax <= 0.15 * (lmax - lmin)):
            raise _NoGraph()
        self.regions = {"A": (lmin, lmax, imax)}
        blocks = S._pcA[1]
        # (a DistEngine has the same call: element pass, exchange, block pass, exchange, update)
        step = lambda ca, cb, x, r, d: eng.sw_operator_precond_chebyshev(ROS_ALPHA * dt, S.grav, H_MEAN, S.fg, blocks, ca, cb, x, r, d)
        self.chA = GraphedChebyshev(eng, (un.shape[0], n1 + n2), body1, lambda r: S.precond_A(r, dt), lmin, lmax, rtol=S.rtol, step=step,
                                    margin=mgA, space="uh")
        self.its["A"] = self.chA.steps
        # ---- M1: real interval of P M1
        cm = S.m1_pre.transpose(1, 2).contiguous()
        if self.dist:
            rb = eng.randn_global(1, 4321, cpu_generator=True).expand(un.shape[0], -1).contiguous()
            w1 = eng.weights(1)
            l1, l2, e1, e2 = lanczos_bounds(S.M1, S.precond_M1, rb, its=40, errors=True, dot=lambda a, b: eng.allreduce(torch.linalg.vecdot(a * w1, b, dim=1)))
        else:
            rb = seeded_randn(un.shape, 4321, dev)
            l1, l2, e1, e2 = lanczos_bounds(S.M1, S.precond_M1, rb, its=40, errors=True)
        self.regions["M1"] = (l1, l2)
        self.margins = {"A": mgA, "M1": ritz_margins(l1, l2, 2.0 * e1 / l1, 2.0 * e2 / l2, widen)}
        self.cm = cm
        self.chM = ChebyshevMass(eng, lambda x, rhs, p, al, be, upd: eng.block_chebyshev_sweep("UMAT", cm, x, rhs, p, al, be, upd=upd), l1, l2, rtol=S.rtol,
                                 margin=self.margins["M1"])
        self.its["F"] = self.chM.steps
        # the two vectors of a check (last preconditioned residual | P b) sit side by side: ONE two-row dot per check instead of two
        self.pairM = torch.zeros(2, un.shape[1], dtype=torch.float64, device=dev) if un.shape[0] == 1 else None
        if self.pairM is not None:
            self.chM.p = torch.zeros_like(un); self.chM.upd = self.pairM[0:1]
        # ---- the upwinded lumped 0-form mass under its diagonal: 1 +- i sigma (the upwinding is a skew perturbation of the identity)
        self.qcoef = None
        if not q_exact:
            m0h = eng.pvec(0, 1, 1.0, h2=hn)
            tau = 1.0 / (1.0 / (UP_TAU * dt))
            evq = arnoldi_ritz(lambda v: eng.apply_up("PHMAT_UP", v, hn, un, fac=UP_TAU, dt=dt) / m0h, n0, 40, dev, eng=eng, space=0)
            d0 = 0.5 * float(evq.real.max() + evq.real.min())
            a_re = 0.5 * float(evq.real.max() - evq.real.min()) * 1.5 * widen + 0.01
            a_im = float(abs(evq.imag).max()) * 1.2 * widen + 0.01
            self.regions["q"] = (d0, a_re, a_im)
            rate = chebyshev_ellipse_rate(d0, a_re, a_im)
            if not (d0 > 0.2 and rate < 0.6):
                raise _NoGraph()
            nq = rate_steps(rate, S.rtol)
            self.qcoef = chebyshev_ellipse_coefs(d0, a_re * a_re - a_im * a_im, nq)
            self.qtau = tau
            self.qp = torch.zeros(un.shape[0], n0, dtype=torch.float64, device=dev)
            self.pair0 = torch.zeros(2, n0, dtype=torch.float64, device=dev) if un.shape[0] == 1 else None
            self.qupd = self.pair0[0:1] if self.pair0 is not None else torch.zeros_like(self.qp)
            self.its["q"] = nq
        # MIMSEM_SW_FORK=1: the q solve as a parallel branch of the recorded iteration (second stream + second context of the same mesh)
        self.fork = (not q_exact) and not self.dist and experiment("MIMSEM_SW_FORK", "0") == "1"
        # round 6: the mass-flux solve (15 sweeps x 3 launches) and the potential-vorticity solve (20 x 2) of an iteration read nothing of each
        # other: mimsem_sw_dual_chebyshev issues launch k of BOTH chains as one grid -- 45 launches instead of 85 of an iteration's ~210, the same
        # bits (MIMSEM_SW_DUAL=0 under MIMSEM_EXPERIMENTS=1: the two solves one after the other, as round 5)
        self.dual = ((not q_exact) and not self.dist and not self.fork and 2 <= eng.mesh.n <= 4 and self.pairM is not None
                     and getattr(self, "pair0", None) is not None and experiment("MIMSEM_SW_DUAL", "1") == "1")
        if self.fork:
            from .device import Engine
            self.eng_q = Engine(eng.mesh, device=eng.device.index or 0)
            self.sq = torch.cuda.Stream(device=eng.device)
            self.qj = torch.zeros_like(self.qi)

    # -- the inline solves (called from SWEqn.solve_M1 / diagnose_q while this object records or warms up)
    def m1(self, b):
        if self.pairM is not None and not self.dist and hasattr(self.S.eng, "block_chebyshev_solve") and self.S.eng.n1e <= 30 and len(self.chM.coef) > 1:
            # one context: the whole solve from x = 0 as ONE call (no operator pass in the first step, nothing cleared); P b, the check's reference
            # vector, is the first step's update -- 5 launches fewer than the sweeps + the extra preconditioner application (config 2: no dual solves)
            x = self.S.eng.block_chebyshev_solve("UMAT", self.cm, b, self.chM.coef, pb=self.pairM[1:2], upd=self.pairM[0:1])
            self.log.pair(self.pairM, "M1", self.SPACE["M1"])
            return x
        x = self.chM.solve(b, want_residual=True)
        if self.pairM is not None and self.chM.upd.data_ptr() == self.pairM.data_ptr():
            self.S.precond_M1(b, out=self.pairM[1:2])
            self.log.pair(self.pairM, "M1", self.SPACE["M1"])
        else:
            self.log.two(self.chM.upd, self.S.precond_M1(b), "M1", self.SPACE["M1"])
        return x

    def q(self, rhs, m0h, h, u, dt):
        eng = self.S.eng
        dinv = torch.reciprocal(m0h)
        x = torch.zeros_like(rhs)
        self.qp.zero_()
        last = len(self.qcoef) - 1
        for k, (al, be) in enumerate(self.qcoef):
            eng.chebyshev_sweep("PHMAT_UP", x, rhs, dinv, self.qp, al, be, f=h, u=u, tau=self.qtau, upd=self.qupd if k == last else None)
        if self.pair0 is not None:
            torch.mul(rhs, dinv, out=self.pair0[1:2])
            self.log.pair(self.pair0, "q", self.SPACE["q"])
        else:
            self.log.two(self.qupd, rhs * dinv, "q", self.SPACE["q"])
        return x

    def solve_F_and_q(self, hu, rhs0, m0h, h, u):
        """M1 F = hu and M0h_up(h, u) q = rhs0 by their fixed-length Chebyshev iterations in SHARED launches; both checks logged as m1() / q() do"""
        S, eng = self.S, self.S.eng
        dinv = torch.reciprocal(m0h)
        F = torch.empty_like(hu); q = torch.empty_like(rhs0)          # (outputs of solves from x = 0: written, not updated -- nothing to clear)
        eng.sw_dual_chebyshev(self.chM.coef, self.cm, hu, self.chM.p, F, self.pairM[0:1], self.qcoef, self.qtau, h, u, rhs0, dinv, self.qp, q, self.pair0[0:1],
                              pb1=self.pairM[1:2], pb0=self.pair0[1:2])      # P hu and dinv rhs0, the checks' reference vectors, are the first steps' updates
        self.log.pair(self.pairM, "M1", self.SPACE["M1"])
        self.log.pair(self.pair0, "q", self.SPACE["q"])
        return F, q

    def _q_on_a_branch(self, first, uj, hj):
        """the potential vorticity of this iteration (from (ui, hi) in the first, (uj, hj) in the later ones) on a SECOND stream and a second
        context of the same mesh (own workspaces): ~45 of an iteration's ~225 graph nodes that depend on nothing the mass flux F and the
        Bernoulli function need -- a parallel branch of the recorded graph, joined before the rotational term reads q"""
        S = self.S
        main = torch.cuda.current_stream(S.eng.device)
        self.sq.wait_stream(main)
        eng_main, S.eng = S.eng, self.eng_q
        try:
            with torch.cuda.stream(self.sq), self.eng_q.on_current_stream():
                if first:
                    self.qi.copy_(S.diagnose_q(self.dt, self.ui, self.hi, key="qi"))
                else:
                    self.qj.copy_(S.diagnose_q(self.dt, uj, hj, key="qj1"))
        finally:
            S.eng = eng_main
        return lambda: main.wait_stream(self.sq)

    def _body(self, first):
        S, n1 = self.S, self.S.n1
        self.log.rewind()                                # (a slot claimed while recording is part of the graph: every body fills the same ones)
        uj, hj = self.x[:, :n1].contiguous(), self.x[:, n1:].contiguous()
        join = None
        F = None
        if self.dual:
            # both right-hand sides first, then the two solves together: q of (ui, hi) in the first iteration of a step (uj = ui: it is qj too),
            # of (uj, hj) in the later ones
            hu = S.F_rhs(self.ui, uj, self.hi, hj)
            uq_, hq_ = (self.ui, self.hi) if first else (uj, hj)
            rhs0, m0h = S.q_rhs(uq_, hq_)
            F, qn = self.solve_F_and_q(hu, rhs0, m0h, hq_, uq_)
            if first:
                self.qi.copy_(qn)
            qj = self.qi if first else qn
        else:
            if self.fork and not self.q_exact:
                join = self._q_on_a_branch(first, uj, hj)
            elif first and not self.q_exact:
                self.qi.copy_(S.diagnose_q(self.dt, self.ui, self.hi, key="qi"))
            qj = None if self.q_exact else (self.qi if first else (self.qj if self.fork else None))
        f = S.assemble_residual(self.ui, self.hi, uj, hj, self.dt, self.q_exact, self.bot, qi=None if self.q_exact else self.qi,
                                qj=qj, it=0 if first else 1, before_q=join, F=F)
        ch = self.chA
        ch._run(neg_of=f, nrm=self.log.claim("A"))              # A dx = -f: the sign rides in the start kernel, the check norms go straight into the log
        if not self.dist and hasattr(S.eng, "axpy_dots") and self.x.is_contiguous() and ch.x.is_contiguous():
            S.eng.axpy_dots(ch.x, self.x, self.log.claim("picard"))      # x += dx, |dx|^2, |x|^2: one launch
        else:
            self.x.add_(ch.x)
            self.log.two(ch.x, self.x, "picard", self.SPACE["picard"])

    def replay(self, first):
        """one Picard iteration; returns the host copy of the log, [NSLOT, 2].  Sharded with a library or host transport: the same sequence of
        launches eagerly, with the halo exchanges where the element-local sums need completing.  Every check norm is a local (ownership-weighted)
        partial sum: CheckLog.read holds the ONE all-reduce of a Picard iteration (this rank's count of one-sided halo plans whose exchange gave up
        waiting folded in, so every rank raises HaloTimeout after the same collective); there is none inside any solve"""
        S = self.S
        eager = self.dist and not self.record
        if eager or first not in self.graphs:
            keep = None if eager else self.x.clone()
            S._inline = self
            try:
                g = self._body(first) if eager else S.eng.capture(lambda: self._body(first))[0]
            finally:
                S._inline = None
            self.graphs[first] = (g, self.log.kinds[:self.log.size], self.log.size)
            if not eager:
                self.x.copy_(keep)
        if not eager:
            self.graphs[first][0].replay()
        return CheckLog.read(self.log)[0]

    def verify(self, vals, first):
        """vals: the host copy of the log, {|r|^2, |ref|^2} per slot.  (every check passed, |dx| / |x| of the picard slot)"""
        _, kinds, nslots = self.graphs[first]
        vals = np.asarray(vals, dtype=np.float64).reshape(-1).tolist()
        ok, norm = True, float("nan")
        for k in range(nslots):
            res2, ref2 = vals[2 * k], vals[2 * k + 1]
            if kinds[k] == "picard":
                norm = (res2 / ref2) ** 0.5 if ref2 > 0.0 else 0.0
                ok = ok and norm == norm
                continue
            # M1 / q log the residual the LAST sweep saw (one more contraction lies between it and the result): a factor 30 of slack; the
            # [u|h] system logs the recurrence residual of the result itself
            tol = self.S.rtol * (30.0 if kinds[k] in ("M1", "q") else 3.0)
            good, rel = accepted(res2, ref2, tol)
            if not good:
                ok = False
                self.last_miss = (kinds[k], rel, tol)
        return ok, norm


def williamson2(xq, alpha=0.25 * math.pi):
    """src/Williamson2.cpp:20-61 evaluated at points xq [n,3]: (u, v), h.  NB the SWEqn Coriolis term is un-rotated unless
    W2_ALPHA is defined in SWEqn_Picard.cpp (it is commented out there, :24) -- callers pass alpha=0 for a steady state."""
    U0, H0 = 38.61068276698372, 2998.1154702758267
    OMEGA, GRAV = 7.292e-5, 9.80616
    theta = torch.asin(xq[:, 2] / RAD_SPHERE)
    lam = torch.atan2(xq[:, 1], xq[:, 0])
    u = U0 * (torch.cos(theta) * math.cos(alpha) + torch.cos(lam) * torch.sin(theta) * math.sin(alpha))
    v = -U0 * torch.sin(lam) * math.sin(alpha)
    b = -torch.cos(lam) * torch.cos(theta) * math.sin(alpha) + torch.sin(theta) * math.cos(alpha)
    h = H0 - (RAD_SPHERE * OMEGA * U0 + 0.5 * U0 * U0) * b * b / GRAV
    return torch.stack([u, v], dim=1), h


def galewsky(xq):
    """src/Galewsky.cpp:24-82 evaluated at points xq [n,3]: (u, v), h -- the barotropically unstable mid-latitude jet of Galewsky,
    Scott & Polvani (2004) with its balanced depth (the reference's 1000-step rectangle rule from the equator, the latitude
    advanced BEFORE each evaluation) and the localised depth perturbation."""
    eps, umax = 1.0e-8, 80.0 * (RAD_SPHERE / RAD_EARTH)
    phi0 = math.pi / 7.0
    phi1 = math.pi / 2.0 - phi0
    en = math.exp(-4.0 / ((phi1 - phi0) * (phi1 - phi0)))

    def jet(phi):
        inside = (phi > phi0 + eps) & (phi < phi1 - eps)
        arg = torch.where(inside, (phi - phi0) * (phi - phi1), torch.full_like(phi, -1.0))
        return torch.where(inside, (umax / en) * torch.exp(1.0 / arg), torch.zeros_like(phi))

    phi = torch.asin(xq[:, 2] / RAD_SPHERE)
    lam = torch.atan2(xq[:, 1], xq[:, 0])
    ni = 1000
    dphi = (phi / ni).abs()
    sgn = torch.where(phi > 0, torch.ones_like(phi), -torch.ones_like(phi))
    h = torch.full_like(phi, 10000.0 * (RAD_SPHERE / RAD_EARTH))
    grav, omega = 9.80616 * (RAD_SPHERE / RAD_EARTH), 7.292e-5
    pp = torch.zeros_like(phi)
    for _ in range(ni):
        pp = pp + sgn * dphi
        # the reference evaluates u_init at x2 = (x, y, R sin(phiPrime)): its latitude is asin(sin(phiPrime)) = phiPrime
        u = jet(pp)
        f = 2.0 * omega * torch.sin(pp)
        h = h - RAD_SPHERE * u * (f + torch.tan(pp) * u / RAD_SPHERE) * dphi / grav
    hHat, alpha, beta, phi2 = 120.0 * (RAD_SPHERE / RAD_EARTH), 1.0 / 3.0, 1.0 / 15.0, math.pi / 4.0
    h = h + hHat * torch.cos(phi) * torch.exp(-1.0 * (lam / alpha) ** 2) * torch.exp(-1.0 * ((phi2 - phi) / beta) ** 2)
    return torch.stack([jet(phi), torch.zeros_like(phi)], dim=1), h
