// mimsem_horizsolve.hpp -- the right-hand sides of the horizontal dynamics (row N2) driven from C++ over the C ABI: the counterpart of the
// reference's HorizSolve (eul/HorizSolve.cpp: grad :208-228, curl :233-254, laplacian :256-283, diagnose_fluxes :285-327, advection_rhs_ec
// :380-417, diagnose_Phi :419-470, diagnose_q :472-493, momentum_rhs_ec :637-786) for a host that holds its fields in device memory.
// The reference loops `for (kk ...)` around a per-level assemble + MatMult + KSPSolve; here EVERY LEVEL goes through each operator in one
// call (level rows `n` doubles apart), and the ksp1 solves of all levels are ONE batched CG (mimsem_ksp_*: one block per element as in
// PCBJACOBI, the thickness of a level as a per-(level, element) factor).
// Field layout: horizontal, one row per level -- 1-forms [nk][n1], 2-forms [nk][n2], 0-forms [nk][n0]; interface quantities (velz, dudz,
// dwdx, Fz) [nk-1][.].  Header-only, C++17, no HIP toolchain needed.
// SHARDED (round 6): with a Shard (mimsem_shard.hpp) every 0/1-form result is completed over the halo -- one exchange per operator result,
// accumulations (MIMSEM_FLAG_ACCUM) through a completed temporary --, the ksp1 solves are the fixed-length Chebyshev iteration with both
// element-local sums of a sweep completed (no inner product: no all-reduce inside a solve), their spectral interval comes from Shard::ritz,
// the check log is ownership-weighted and all-reduced ONCE by verify(), and k2i() is an all-reduced weighted sum.  On the one-sided transport
// (Shard::use_peer; eager here) verify()'s all-reduce also carries the rank's count of exchanges that gave up waiting: HaloTimeout on every rank.
#pragma once
#include <cmath>
#include <utility>
#include "mimsem_mass.hpp"

namespace mimsem_host {

class HorizSolve {
    Mesh* mesh; const double* fg; Shard* sh;
    int nk, n0, n1, n2; bool have_k2i = false, wanted_fixed = true, box = false;
    DeviceArrays mem;
    double* own1n;                                           // (sharded) ownership weights of all levels side by side (the rows of a batched inner product)
    KspHandle ksp1;
    FixedMassSolve m1;
    CheckLog log;
    double *gt1, *w1, *a1, *b1, *c1, *d1, *e1, *g1, *a2, *b2, *c2, *m0, *a0, *b0, *scal;
public:
    static constexpr double SCALE = 1.0e8, OMEGA = 7.29212e-5, RAD_EARTH = 6371220.0;      // eul/HorizSolve.cpp:21-25
    double del2; bool do_visc; double rtol = 1.0e-14;
    int last_its = 0;
    // The ksp1 solves as a Chebyshev semi-iteration of FIXED length (FixedMassSolve, mimsem_mass.hpp): the spectrum of P M1 belongs to the mesh
    // and its layer thicknesses, so its interval is estimated once (mimsem_ksp_ritz on the object PCSetUp built) and the step count for `rtol`
    // follows -- no inner product, no host round trip: a whole right-hand-side evaluation can be recorded in a Graph.  EVERY solve is checked
    // (the reference monitors every KSPSolve): the first sweep's update is P b, the last sweep's the preconditioned residual it saw -- both
    // norms go into a slot of a small device log (CheckLog) with ONE two-row dot (recordable in a Graph, no host round trip); verify() reads
    // the log once -- per right-hand-side evaluation or per time step, the caller's choice, at least every MAXLOG solves (later ones share the
    // last slot) -- and on a miss turns the fixed-length mode off (the CG of the reference's structure from then on; the caller redoes the
    // evaluation).  levels_changed() after mimsem_ctx_set_levels: PCSetUp and the interval again.  use_fixed_length(false) keeps the CG.
    static constexpr int MAXLOG = 32;
    double &margin_lo = m1.margin_lo, &margin_hi = m1.margin_hi;      // the safety margins in force around the Ritz interval (use_fixed_length)
    bool& whole_solve = m1.whole_solve;  // one context: a mass solve is ONE mimsem_block_chebyshev_solve call (false: cheb_steps sweep calls)
    int& cheb_steps = m1.steps; bool fixed_length = false; int solves_checked = 0, solves_missed = 0; double worst_rel = 0.0;

    // fg: the Coriolis 0-form per level (HorizSolve::coriolis :124-161), device [nk][n0]; nDofs0G: the GLOBAL node count (viscosity() :112-120)
    // shard (optional): this rank's part of the exchanges and reductions; nDofs0G must then be the GLOBAL node count
    HorizSolve(Mesh* m, const double* fg_dev, long long nDofs0G = 0, bool visc = true, Shard* shard = nullptr)
        : mesh(m), fg(fg_dev), sh(shard), nk(m->nk_), n0(m->n0), n1(m->n1), n2(m->n2), own1n(shard ? level_rows(shard->own1) : nullptr),
          ksp1(m, MIMSEM_KSP_CG), m1(m, nk, SCALE, MIMSEM_FLAG_VERT, shard, own1n), log(m, MAXLOG, true), do_visc(visc) {
        if (sh && nDofs0G <= 0) throw std::runtime_error("HorizSolve (sharded): the global node count is needed for the viscosity");
        const double dx = std::sqrt(4.0*M_PI*RAD_EARTH*RAD_EARTH/(double)(nDofs0G > 0 ? nDofs0G : n0));
        del2 = -std::sqrt(0.072*std::pow(dx, 3.2));
        for (double** p : {&a1, &b1, &c1, &d1, &e1, &g1, &gt1, &w1}) *p = mem.get((size_t)nk*n1);
        for (double** p : {&a2, &b2, &c2}) *p = mem.get((size_t)nk*n2);
        for (double** p : {&m0, &a0, &b0}) *p = mem.get((size_t)nk*n0);
        scal = mem.get(4);
        check(mimsem_pvec(mesh->ctx, 0, nk, SCALE, nullptr, 0, m0, n0), "mimsem_pvec");                   // M0 is diagonal (collocated 0-forms)
        if (sh) sh->complete0(m0, nk);
        // ksp1 (:77-96): the 1-form mass of every level, one element block each
        check(mimsem_ksp_set_operator(ksp1, MIMSEM_OP_UMAT, 0, nk, SCALE, MIMSEM_FLAG_VERT, nullptr, 0), "mimsem_ksp_set_operator");
        check(mimsem_ksp_set_pc_bjacobi(ksp1), "mimsem_ksp_set_pc_bjacobi");
        check(mimsem_ksp_set_tolerances(ksp1, rtol, 1.0e-50, 1000, 0, 2), "mimsem_ksp_set_tolerances");
        use_fixed_length(true);
    }
    // Box mode (box/HorizSolve.cpp), selected by this tag: lx the side of the doubly periodic box; thick the HOST layer thicknesses the mesh was made
    // with (mimsem_mesh_desc::thick, `count` doubles).  What differs from the sphere: del2 = -sqrt(2 * 0.072 dx^3.2), dx = sqrt(lx^2 / nDofs0G)
    // (:106-114); the rotational operands of momentum_rhs are curl(u_h) WITHOUT Coriolis and u_h itself (diagnose_wxu :382-410) -- no diagnose_q, no
    // mass-flux solve, rho1 / rho2 may be null; the _ec routines and diagnose_q have no box twin and throw.  UNIFORM LAYERS ONLY: the reference assembles
    // its matrices once, at level 0 (box/Assembly.cpp:44); the constructor throws on any other mesh.  One context (the box is one patch).
    struct Box { double lx; const double* thick; size_t count; };
    HorizSolve(Mesh* m, const Box& bx, bool visc = true) : HorizSolve(m, nullptr, 0, visc, nullptr) {
        box = true;
        if (!bx.thick || bx.count == 0) throw std::runtime_error("HorizSolve (box): the layer thicknesses are needed for the uniform-layer check");
        double lo = bx.thick[0], hi = bx.thick[0];
        for (size_t i = 1; i < bx.count; i++) { lo = std::min(lo, bx.thick[i]); hi = std::max(hi, bx.thick[i]); }
        if (!(lo > 0.0 && hi - lo <= 1.0e-14*hi)) throw std::runtime_error("HorizSolve (box): uniform layers only");
        const double dx = std::sqrt(bx.lx*bx.lx/(double)n0);
        del2 = -std::sqrt(2.0*0.072*std::pow(dx, 3.2));
    }
    bool box_mode() const { return box; }
    HorizSolve(const HorizSolve&) = delete; HorizSolve& operator=(const HorizSolve&) = delete;
    void use_fixed_length(bool on) {
        fixed_length = false; wanted_fixed = on;
        if (!on) return;
        const double *blocks = nullptr, *escale = nullptr;
        const bool have = mimsem_ksp_get_pc_blocks(ksp1, &blocks, &escale, nullptr) == MIMSEM_OK;
        if (sh && !have) throw std::runtime_error("HorizSolve (sharded): no element blocks for this order");
        m1.use_blocks(have ? blocks : nullptr, escale);
        // margins of at most 10 % / 5 %: on a smooth thickness field the Ritz values are exact to 1e-4; every solve is still checked (verify())
        const Ritz ritz = sh ? m1.shard_ritz(1234) : Ritz([&](int steps, double* lo, double* hi, double* im) { check(mimsem_ksp_ritz(ksp1, steps, lo, hi, im), "mimsem_ksp_ritz"); });
        if (!m1.calibrate(ritz, rtol, 0.10, 0.05)) {
            if (sh) throw std::runtime_error("HorizSolve (sharded): the spectral interval does not admit the fixed-length solves (no CG on a shard)");
            return;
        }
        log.rewind(); fixed_length = true;
    }
    void shorten_for_test(int steps) { m1.shorten(steps); }      // (tests: a solve that must miss its check)
    // for a host that solves with a matrix close to M1 on the same blocks and logs into the same checks (mimsem_euler.hpp: HorizMomentum's
    // M1 + M1ray under Held-Suarez forcing): the object PCSetUp built, the fixed-length solver with its blocks and pair arrays, the log
    mimsem_ksp* mass_ksp() const { return ksp1; }
    FixedMassSolve& mass_solver() { return m1; }
    CheckLog& check_log() { return log; }
    // after mimsem_ctx_set_levels (new layer thicknesses): the element blocks and the per-(level, element) factors of the preconditioner and
    // the spectral interval belong to the old ones
    void levels_changed() {
        check(mimsem_ksp_set_pc_bjacobi(ksp1), "mimsem_ksp_set_pc_bjacobi");
        use_fixed_length(fixed_length || wanted_fixed);
    }
    // the checks of every fixed-length solve since the last call, in one read: true = all met 30 rtol (the residual the LAST sweep saw: one more
    // contraction lies between it and the result).  false: fixed_length is off now -- redo the evaluation (it then runs the CG).  Synchronises.
    bool verify() {
        if (!fixed_length && log.size() == 0) return true;
        double v[2*MAXLOG + 1];
        log.read(v);
        log.clear();
        if (sh) {                                                    // ONE all-reduce for every solve since the last call, with this rank's count of
            v[2*MAXLOG] = (double)sh->peer_timeouts();               // one-sided plans that gave up waiting (every rank sees any rank's time-out)
            sh->allreduce(v, 2*MAXLOG + 1);
            if (v[2*MAXLOG] != 0.0)
                throw HaloTimeout("HorizSolve (sharded): " + std::to_string((long)v[2*MAXLOG]) + " halo plan(s) gave up waiting for an exchange of the one-sided transport: the halo is stale");
        }
        bool ok = true;
        for (int k = 0; k < MAXLOG; k++) {
            const double r2 = v[2*k], ref2 = v[2*k + 1], rel = cheb::relative(r2, ref2);
            if (r2 == 0.0 && ref2 == 0.0) continue;                  // (slot not written, or a zero right-hand side)
            solves_checked++;
            if (!(rel <= worst_rel)) worst_rel = rel == rel ? rel : HUGE_VAL;
            if (!cheb::accepted(r2, ref2, 30.0*rtol)) { ok = false; solves_missed++; }
        }
        if (!ok && sh) throw std::runtime_error("HorizSolve (sharded): a fixed-length mass solve missed its check (no CG on a shard)");
        if (!ok) fixed_length = false;                              // the interval was too optimistic for these right-hand sides: the CG from here on
        return ok;
    }

    // u = M1^-1 E12 M2 phi  (:208-228)
    void grad(const double* phi, double* u) {
        ap(MIMSEM_OP_WMAT, MIMSEM_FLAG_VERT, nullptr, 0, phi, n2, a2, n2, 1.0);
        inc(2, a2, n2, g1, n1);
        solve_M1(g1, u);
    }
    // w = M0^-1 E01 M1 u (+ f)  (:233-254)
    void curl(const double* u, double* w, bool add_f = false) {
        ap(MIMSEM_OP_UMAT, MIMSEM_FLAG_VERT, nullptr, 0, u, n1, g1, n1, 1.0);
        inc(3, g1, n1, w, n0);
        mesh->combine(n0, 1.0, w, 2, m0, add_f ? 1.0 : 0.0, add_f ? fg : nullptr, w, nk);
    }
    // del2 (grad(E21 u) + E10 curl(u))  (:256-283)
    void laplacian(const double* u, double* out) {
        inc(1, u, n1, c2, n2);
        grad(c2, out);
        curl(u, b0);
        inc(0, b0, n0, e1, n1);
        mesh->combine(n1, del2, e1, 0, nullptr, del2, out, out, nk);
    }
    // F = M1^-1 (hu),  G = M1^-1 F(theta) F  (:285-327, theta_in_Wt = false)
    void diagnose_fluxes(const double* u1, const double* u2, const double* h1, const double* h2, const double* theta, double* F, double* G) {
        uvec_hu4(u1, u2, h1, h2, d1);
        solve_M1(d1, F);
        ap(MIMSEM_OP_UHMAT, MIMSEM_FLAG_VERT, theta, n2, F, n1, d1, n1, 1.0);
        solve_M1(d1, G);
    }
    // :380-417: dF, dG [nk][n2] (horizontal layout; the caller's HorizToVert is mimsem_l2_transpose), Fk, Gk [nk][n1]
    void advection_rhs_ec(const double* u1, const double* u2, const double* h1, const double* h2, const double* theta, double* dF, double* dG,
                          double* Fk, double* Gk) {
        no_box_twin("advection_rhs_ec");
        diagnose_fluxes(u1, u2, h1, h2, theta, Fk, Gk);
        inc(1, Fk, n1, b2, n2);
        ap(MIMSEM_OP_WMAT, MIMSEM_FLAG_VERT, nullptr, 0, b2, n2, dF, n2, 1.0);
        inc(1, Gk, n1, c2, n2);
        ap(MIMSEM_OP_WMAT, MIMSEM_FLAG_VERT, nullptr, 0, c2, n2, dG, n2, 0.5);
        ap(MIMSEM_OP_WHMAT, MIMSEM_FLAG_VERT | MIMSEM_FLAG_ACCUM, theta, n2, b2, n2, dG, n2, 0.5);
        grad(theta, gt1);                                                                                   // (kept: last_grad_theta())
        ap(MIMSEM_OP_WTQUMAT, MIMSEM_FLAG_ACCUM, gt1, n1, Fk, n1, dG, n2, 1.0);                             // K incl. its 0.5 factor
    }
    // grad(theta) of the last advection_rhs_ec [nk][n1]: momentum_rhs_ec of the same stage solves the same system for the same theta
    // (:403 and :659 in the reference, two KSPSolves with one answer) -- passed as its dTheta it saves one of the seven mass solves
    const double* last_grad_theta() const { return gt1; }
    // The switches of the non-_ec right-hand sides, as HorizSolve.fused_hu / fused_forcing / fused_phi in Python: the mass-flux right-hand side by
    // mimsem_horiz_flux_rhs, the element-local forcing of momentum_rhs by mimsem_horiz_momentum_forcing, diagnose_Phi by mimsem_horiz_bernoulli.
    // All off by default: the _ec routines keep their bits.  One context only (not on a shard).
    // In box mode fused_hu acts in advection_rhs only: the box's rotational term takes u_h itself, momentum_rhs forms no mass flux there.
    bool fused_hu = false, fused_forcing = false, fused_phi = false;
    // F = M1^-1 (hu),  G = M1^-1 F(1/2 theta_k + 1/2 theta_{k+1}; no vert_scale) F  (:285-327, theta_in_Wt = true: theta [nk+1][n2] on the interfaces)
    void diagnose_fluxes_Wt(const double* u1, const double* u2, const double* h1, const double* h2, const double* theta, double* F, double* G) {
        hu(u1, u2, h1, h2, d1);
        solve_M1(d1, F);
        theta_levels(theta, b2);                                                                            // :313-317
        ap(MIMSEM_OP_UHMAT, 0, b2, n2, F, n1, d1, n1, 1.0);
        solve_M1(d1, G);
    }
    // :330-375: dF = E21 Fk, dG = E21 Gk [nk][n2] (no M2 factor: VertSolve::solve_schur_2 applies VB after adding them), Fk, Gk [nk][n1];
    // theta [nk+1][n2] on the interfaces.  The do_temp_visc branch (:341-364) is not built, as in Python
    void advection_rhs(const double* u1, const double* u2, const double* h1, const double* h2, const double* theta, double* dF, double* dG,
                       double* Fk, double* Gk) {
        diagnose_fluxes_Wt(u1, u2, h1, h2, theta, Fk, Gk);
        inc(1, Fk, n1, dF, n2);
        inc(1, Gk, n1, dG, n2);
    }
    // :419-470
    void diagnose_Phi(const double* u1, const double* u2, const double* velz1, const double* velz2, double* Phi) {
        if (fused_phi) {
            one_context("fused_phi");
            check(mimsem_horiz_bernoulli(mesh->ctx, nk, u1, u2, n1, velz1, velz2, n2, SCALE, Phi, n2), "mimsem_horiz_bernoulli");
            return;
        }
        ap(MIMSEM_OP_WTQUMAT, 0, u1, n1, u1, n1, Phi, n2, 1.0/3.0);
        ap(MIMSEM_OP_WTQUMAT, MIMSEM_FLAG_ACCUM, u1, n1, u2, n1, Phi, n2, 1.0/3.0);
        ap(MIMSEM_OP_WTQUMAT, MIMSEM_FLAG_ACCUM, u2, n1, u2, n1, Phi, n2, 1.0/3.0);
        // 0.5 (interface k-1) + 0.5 (interface k), the missing boundary interfaces left out (:451-459)
        check(mimsem_interface_average(mesh->ctx, nk, n2, velz1, n2, b2, n2), "mimsem_interface_average");
        check(mimsem_interface_average(mesh->ctx, nk, n2, velz2, n2, c2, n2), "mimsem_interface_average");
        ap(MIMSEM_OP_WHMAT, MIMSEM_FLAG_ACCUM, b2, n2, b2, n2, Phi, n2, 1.0/6.0);
        ap(MIMSEM_OP_WHMAT, MIMSEM_FLAG_ACCUM, b2, n2, c2, n2, Phi, n2, 1.0/6.0);
        ap(MIMSEM_OP_WHMAT, MIMSEM_FLAG_ACCUM, c2, n2, c2, n2, Phi, n2, 1.0/6.0);
    }
    // (M0h(rho)) q = E01 M1 u + M0 f; M0h is diagonal  (:472-493)
    void diagnose_q(const double* rho, const double* u, double* q) {
        no_box_twin("diagnose_q");
        ap(MIMSEM_OP_UMAT, MIMSEM_FLAG_VERT, nullptr, 0, u, n1, g1, n1, 1.0);
        inc(3, g1, n1, q, n0);
        mesh->combine(n0, 1.0, m0, 1, fg, 1.0, q, q, nk);
        check(mimsem_pvec(mesh->ctx, 0, nk, SCALE, rho, n2, b0, n0), "mimsem_pvec");
        if (sh) sh->complete0(b0, nk);
        mesh->combine(n0, 1.0, q, 2, b0, 0.0, nullptr, q, nk);
    }
    // :637-786 for every level at once: fu [nk][n1].  Optional: Fx (the mass flux, else diagnosed), Fz (vertical mass flux on the interfaces,
    // else the mean vertical velocity), dwdx1 / dwdx2, Fk (then k2i() is the kinetic-to-internal exchange :697-701)
    void momentum_rhs_ec(const double* theta, const double* dudz1, const double* dudz2, const double* velz1, const double* velz2, const double* Pi,
                         const double* velx1, const double* velx2, const double* rho1, const double* rho2, double* fu,
                         const double* Fx = nullptr, const double* Fz = nullptr, const double* dwdx1 = nullptr, const double* dwdx2 = nullptr,
                         const double* Fk = nullptr, const double* dTheta = nullptr) {
        no_box_twin("momentum_rhs_ec");
        diagnose_Phi(velx1, velx2, velz1, velz2, a2);
        inc(2, a2, n2, fu, n1);
        grad(Pi, a1);                                                                                         // dPi
        if (!dTheta) { grad(theta, b1); dTheta = b1; }                                                        // dTheta
        mesh->combine(n1, 0.5, velx1, 0, nullptr, 0.5, velx2, c1, nk);                                                     // uh
        mesh->combine(n2, 0.5, rho1, 0, nullptr, 0.5, rho2, b2, nk);
        diagnose_q(b2, c1, a0);
        if (!Fx) { uvec_hu4(velx1, velx2, rho1, rho2, d1); solve_M1(d1, e1); Fx = e1; }
        ap(MIMSEM_OP_ROTMAT, MIMSEM_FLAG_ACCUM, a0, n0, Fx, n1, fu, n1, 1.0);
        ap(MIMSEM_OP_UHMAT, MIMSEM_FLAG_VERT | MIMSEM_FLAG_ACCUM, theta, n2, a1, n1, fu, n1, 0.5);            // pressure gradient force
        ap(MIMSEM_OP_UHMAT, MIMSEM_FLAG_VERT | MIMSEM_FLAG_ACCUM, Pi, n2, dTheta, n1, fu, n1, -0.5);
        ap(MIMSEM_OP_WHMAT, MIMSEM_FLAG_VERT, Pi, n2, theta, n2, a2, n2, 1.0);
        inc(2, a2, n2, d1, n1);                                                                               // dp
        mesh->combine(n1, 0.5, d1, 0, nullptr, 1.0, fu, fu, nk);
        k2i_dot(Fk, d1);
        vorticity_and_viscosity(fu, dudz1, dudz2, velz1, velz2, Fz, dwdx1, dwdx2);
    }
    // :496-635 for every level at once: momentum_rhs_ec with theta [nk+1][n2] on the interfaces.  There is no grad(theta); the pressure gradient
    // force is the single term fu += F(theta_h; no vert_scale) dPi, theta_h = 1/2 theta_k + 1/2 theta_{k+1} (:514-517, :556-558), and k2i() =
    // sum_k Fk_k . (F(theta_h) dPi)_k / SCALE (:560-563, needs Fk).  The mass flux of the rotational term (Fx null) is formed by fused_hu; with
    // fused_forcing the rotational term, the pressure gradient force and the second vorticity term are one mimsem_horiz_momentum_forcing call
    // (dp for k2i then keeps its own Uhmat apply).  The second vorticity term and the viscosity are momentum_rhs_ec's
    void momentum_rhs(const double* theta, const double* dudz1, const double* dudz2, const double* velz1, const double* velz2, const double* Pi,
                      const double* velx1, const double* velx2, const double* rho1, const double* rho2, double* fu,
                      const double* Fx = nullptr, const double* Fz = nullptr, const double* dwdx1 = nullptr, const double* dwdx2 = nullptr,
                      const double* Fk = nullptr) {
        diagnose_Phi(velx1, velx2, velz1, velz2, a2);
        inc(2, a2, n2, fu, n1);
        grad(Pi, a1);                                                                                         // dPi
        mesh->combine(n1, 0.5, velx1, 0, nullptr, 0.5, velx2, c1, nk);                                        // uh
        if (box) { curl(c1, a0); Fx = c1; }                                                                   // diagnose_wxu box :382-410
        else {
            mesh->combine(n2, 0.5, rho1, 0, nullptr, 0.5, rho2, b2, nk);
            diagnose_q(b2, c1, a0);
            if (!Fx) { hu(velx1, velx2, rho1, rho2, d1); solve_M1(d1, e1); Fx = e1; }
        }
        theta_levels(theta, b2);                                                                              // theta_h (:514-517)
        if (fused_forcing) {
            one_context("fused_forcing");
            const double* v = nk > 1 ? vorticity_operands(dudz1, dudz2, velz1, velz2, Fz, dwdx1, dwdx2, b1) : nullptr;
            check(mimsem_horiz_momentum_forcing(mesh->ctx, nk, MIMSEM_FLAG_ACCUM, SCALE, a0, Fx, b2, a1, nk > 1 ? b1 : nullptr, v, fu),
                  "mimsem_horiz_momentum_forcing");
            if (Fk) ap(MIMSEM_OP_UHMAT, 0, b2, n2, a1, n1, d1, n1, 1.0);
            k2i_dot(Fk, d1);
            viscosity(fu);
            return;
        }
        ap(MIMSEM_OP_ROTMAT, MIMSEM_FLAG_ACCUM, a0, n0, Fx, n1, fu, n1, 1.0);
        ap(MIMSEM_OP_UHMAT, 0, b2, n2, a1, n1, d1, n1, 1.0);                                                   // dp: the pressure gradient force
        mesh->combine(n1, 1.0, d1, 0, nullptr, 1.0, fu, fu, nk);
        k2i_dot(Fk, d1);
        vorticity_and_viscosity(fu, dudz1, dudz2, velz1, velz2, Fz, dwdx1, dwdx2);
    }
    // horizontal kinetic-to-internal energy exchange of the last momentum_rhs_ec / momentum_rhs that was given Fk (synchronises)
    double k2i() {
        if (!have_k2i) return 0.0;
        double v = 0.0;
        mesh->to_host(&v, scal, 1);
        if (sh) sh->allreduce(&v, 1);
        return v/SCALE;
    }
    // KSPSolve(ksp1, b, x) for all levels
    void solve_M1(const double* b, double* x) {
        if (fixed_length) {
            if (m1.solve(b, x, log) == MIMSEM_OK) { last_its = cheb_steps; return; }
            fixed_length = false;                                    // (an order the fused sweep does not cover: the CG below)
        }
        if (sh) throw std::runtime_error("HorizSolve (sharded): the 1-form mass solve exists in the fixed-length mode only");
        check(mimsem_ksp_solve(ksp1, b, n1, x, n1), "mimsem_ksp_solve");
        double rn; int reason;
        check(mimsem_ksp_get_info(ksp1, &last_its, &rn, &reason), "mimsem_ksp_get_info");
        if (reason < 0) throw std::runtime_error("HorizSolve: the 1-form mass solve did not converge");
    }

private:
    void no_box_twin(const char* what) const { if (box) throw std::runtime_error(std::string("HorizSolve (box): box/HorizSolve.cpp has no ") + what); }
    void one_context(const char* what) const { if (sh) throw std::runtime_error(std::string("HorizSolve (sharded): ") + what + " is for one context"); }
    // 1/2 theta_k + 1/2 theta_{k+1} of theta on the nk+1 interfaces (:314-316, :515-517)
    void theta_levels(const double* theta, double* th) { mesh->combine(n2, 0.5, theta, 0, nullptr, 0.5, theta + n2, th, nk); }
    // the mass-flux right-hand side of the two non-_ec routines: the fused kernel when fused_hu is set
    void hu(const double* ua, const double* ub, const double* ha, const double* hb, double* out) {
        if (!fused_hu) { uvec_hu4(ua, ub, ha, hb, out); return; }
        one_context("fused_hu");
        check(mimsem_horiz_flux_rhs(mesh->ctx, nk, ua, ub, n1, ha, hb, n2, SCALE, out, n1), "mimsem_horiz_flux_rhs");
    }
    // the sum Fk . dp over every level, left on the device for k2i() (:560-563, :697-701)
    void k2i_dot(const double* Fk, const double* dp) {
        mimsem_ctx* c = mesh->ctx;
        have_k2i = Fk != nullptr;
        if (Fk && sh) { mesh->combine(n1, 1.0, Fk, 1, own1n, 0.0, nullptr, w1, nk); check(mimsem_krylov_rowdot(c, 1, (long long)nk*n1, w1, (long long)nk*n1, dp, (long long)nk*n1, scal), "mimsem_krylov_rowdot"); }
        else if (Fk) check(mimsem_krylov_rowdot(c, 1, (long long)nk*n1, Fk, (long long)nk*n1, dp, (long long)nk*n1, scal), "mimsem_krylov_rowdot");
    }
    // coefficient and input of the second vorticity term (:565-607, :704-746): dz = 1/2 dudz1 + 1/2 dudz2 - 1/2 dwdx1 - 1/2 dwdx2 into `dz` (Rh is linear
    // in its coefficient); returns v: Fz, or the mean vertical velocity in a2
    const double* vorticity_operands(const double* dudz1, const double* dudz2, const double* velz1, const double* velz2, const double* Fz,
                                     const double* dwdx1, const double* dwdx2, double* dz) {
        mesh->combine(n1, 0.5, dudz1, 0, nullptr, 0.5, dudz2, dz, nk - 1);
        if (dwdx1) { mesh->combine(n1, -0.5, dwdx1, 0, nullptr, 1.0, dz, dz, nk - 1); mesh->combine(n1, -0.5, dwdx2, 0, nullptr, 1.0, dz, dz, nk - 1); }
        if (Fz) return Fz;
        mesh->combine(n2, 0.5, velz1, 0, nullptr, 0.5, velz2, a2, nk - 1);
        return a2;
    }
    // the end both momentum right-hand sides share (:565-623, :704-768): the second vorticity term -- interface i feeds levels i and i+1 -- and the
    // biharmonic viscosity, added to fu
    void vorticity_and_viscosity(double* fu, const double* dudz1, const double* dudz2, const double* velz1, const double* velz2, const double* Fz,
                                 const double* dwdx1, const double* dwdx2) {
        if (nk > 1) {
            const double* v = vorticity_operands(dudz1, dudz2, velz1, velz2, Fz, dwdx1, dwdx2, a1);
            apn(nk - 1, MIMSEM_OP_UTQWMAT, 0, a1, n1, v, n2, b1, n1, 1.0);                                      // UtQWmat::assemble(u1, scale): no thickness
            mesh->combine(n1, 0.5, b1, 0, nullptr, 1.0, fu + n1, fu + n1, nk - 1);
            mesh->combine(n1, 0.5, b1, 0, nullptr, 1.0, fu, fu, nk - 1);
        }
        viscosity(fu);
    }
    // the biharmonic viscosity of the mean velocity c1 (:609-623, :754-768), added to fu
    void viscosity(double* fu) {
        if (!do_visc) return;
        laplacian(c1, a1);
        laplacian(a1, b1);
        ap(MIMSEM_OP_UMAT, MIMSEM_FLAG_VERT | MIMSEM_FLAG_ACCUM, nullptr, 0, b1, n1, fu, n1, 1.0);
    }
    double* level_rows(const double* own1) {
        std::vector<double> o1(n1), on((size_t)nk*n1);
        mesh->to_host(o1.data(), own1, n1);
        for (int k = 0; k < nk; k++) std::copy(o1.begin(), o1.end(), on.begin() + (size_t)k*n1);
        double* d = mem.get(on.size());
        check(mimsem_memcpy_h2d(mesh->ctx, d, on.data(), (long long)on.size()*8), "h2d");
        return d;
    }
    static bool to_1form(int op) { return op == MIMSEM_OP_UMAT || op == MIMSEM_OP_UHMAT || op == MIMSEM_OP_ROTMAT || op == MIMSEM_OP_UTQWMAT || op == MIMSEM_OP_UTMAT || op == MIMSEM_OP_UTMAT_H; }
    // one operator over `rows` levels; sharded + 1-form result: the element-local sums are completed over the halo before anybody reads them -- an
    // accumulation (MIMSEM_FLAG_ACCUM) goes through a completed temporary (y holds complete values: partial sums must not be mixed into it)
    void apn(int rows, int op, unsigned flags, const double* f, long long fs, const double* x, long long xs, double* y, long long ys, double alpha) {
        if (sh && to_1form(op)) {
            if (flags & MIMSEM_FLAG_ACCUM) {
                check(mimsem_op_apply(mesh->ctx, op, 0, rows, SCALE, flags & ~(unsigned)MIMSEM_FLAG_ACCUM, f, fs, x, xs, w1, n1, alpha), "mimsem_op_apply");
                sh->complete1(w1, rows);
                mesh->combine(n1, 1.0, w1, 0, nullptr, 1.0, y, y, rows);
            } else {
                check(mimsem_op_apply(mesh->ctx, op, 0, rows, SCALE, flags, f, fs, x, xs, y, ys, alpha), "mimsem_op_apply");
                sh->complete1(y, rows);
            }
            return;
        }
        check(mimsem_op_apply(mesh->ctx, op, 0, rows, SCALE, flags, f, fs, x, xs, y, ys, alpha), "mimsem_op_apply");
    }
    void ap(int op, unsigned flags, const double* f, long long fs, const double* x, long long xs, double* y, long long ys, double alpha) { apn(nk, op, flags, f, fs, x, xs, y, ys, alpha); }
    void inc(int which, const double* x, long long xs, double* y, long long ys) {
        check(mimsem_incidence_apply(mesh->ctx, which, nk, x, xs, y, ys), "mimsem_incidence_apply");
        if (sh && (which == 0 || which == 2)) sh->complete1(y, nk);       // E10, E12: every edge computed by the element that owns it
        if (sh && which == 3) sh->complete0(y, nk);                        // E01
    }
    // the four m1->assemble_hu(level, SCALE, u, h, false, fac) calls (:300-305, :675-682)
    void uvec_hu4(const double* ua, const double* ub, const double* ha, const double* hb, double* hu) {
        if (sh) {                                             // the four LOCAL partial sums first, ONE exchange for their sum
            mimsem_ctx* c = mesh->ctx;
            check(mimsem_op_apply(c, MIMSEM_OP_UHMAT, 0, nk, SCALE, MIMSEM_FLAG_VERT, ha, n2, ua, n1, hu, n1, 1.0/3.0), "UHMAT");
            check(mimsem_op_apply(c, MIMSEM_OP_UHMAT, 0, nk, SCALE, MIMSEM_FLAG_VERT | MIMSEM_FLAG_ACCUM, hb, n2, ua, n1, hu, n1, 1.0/6.0), "UHMAT");
            check(mimsem_op_apply(c, MIMSEM_OP_UHMAT, 0, nk, SCALE, MIMSEM_FLAG_VERT | MIMSEM_FLAG_ACCUM, ha, n2, ub, n1, hu, n1, 1.0/6.0), "UHMAT");
            check(mimsem_op_apply(c, MIMSEM_OP_UHMAT, 0, nk, SCALE, MIMSEM_FLAG_VERT | MIMSEM_FLAG_ACCUM, hb, n2, ub, n1, hu, n1, 1.0/3.0), "UHMAT");
            sh->complete1(hu, nk);
            return;
        }
        ap(MIMSEM_OP_UHMAT, MIMSEM_FLAG_VERT, ha, n2, ua, n1, hu, n1, 1.0/3.0);
        ap(MIMSEM_OP_UHMAT, MIMSEM_FLAG_VERT | MIMSEM_FLAG_ACCUM, hb, n2, ua, n1, hu, n1, 1.0/6.0);
        ap(MIMSEM_OP_UHMAT, MIMSEM_FLAG_VERT | MIMSEM_FLAG_ACCUM, ha, n2, ub, n1, hu, n1, 1.0/6.0);
        ap(MIMSEM_OP_UHMAT, MIMSEM_FLAG_VERT | MIMSEM_FLAG_ACCUM, hb, n2, ub, n1, hu, n1, 1.0/3.0);
    }
};

}  // namespace mimsem_host
