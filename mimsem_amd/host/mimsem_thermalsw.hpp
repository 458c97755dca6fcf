// mimsem_thermalsw.hpp -- the thermal shallow-water SSP-RK3 step driven from C++ over the C ABI: the counterpart of the reference's
// ThermalSW_EEC_2 (src/ThermalSW_EEC_2.cpp, DO_THERMAL; solve_rk :859-1004, writeConservation :765-858), the model src/GalewskyTSW_2.cpp
// runs, for a host that holds (u, h, S) in device memory.  Same operations in the same order as the Python host (mimsem_amd/thermalsw.py,
// ThermalSW.stage); per stage:
//   mimsem_tsw_diagnose   s, Phi, h2                                                   (one launch)
//   five M1 solves        F, G, grad h, grad s and the u update: fixed-length block Chebyshev (mimsem_block_chebyshev_solve)
//   one M1h(h) solve      d = M1h(h)^-1 E12 M2 s: PCG of FIXED length (m1h_its), preconditioned by the element blocks of M1h(h) built in ONE
//                         capturable launch per stage (mimsem_elem_block_pc_build), its true residual logged on the device
//   fu                    E12 Phi + R(q) F + 1/4 M1h(s) grad h - 1/4 UtQWmat(d) h2       (accumulating applies: the stateful K(d), M1h(s))
//   mimsem_tsw_update     the new h and S                                                (one launch)
// Every solve logs {|residual|^2, |reference|^2} into one device array (CheckLog; the M1 solves are a FixedMassSolve: mimsem_mass.hpp); the
// step reads it ONCE at its end (host_reads) and accepts it by the one rule of cheb::accepted, as ThermalSW.check / MassSolver.verify do.
// A missed check redoes the step eagerly with adaptive solvers -- CG on M1 to rtol (class KSP)
// and CG on M1h(h) with the same preconditioner -- and keeps them from then on, as the Python host does.
// Recording (use_graph, default): the whole three-stage step is ONE hipGraph (class Graph), recorded after an eager first step for each (dt,
// u, h, S) and replayed; use_graph = false issues the same launches eagerly (the same bits).
// Header-only, C++17, no HIP toolchain needed (everything goes through include/mimsem_hip.h).
#pragma once
#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "mimsem_mass.hpp"

namespace mimsem_host {
namespace src {

class ThermalSW_EEC_2 {
public:
    double omega = 7.292e-5;             // src/ThermalSW_EEC_2.cpp:38
    double rtol = 1.0e-14;               // tolerance of every nested solve
    bool use_graph = true;               // the whole step as one recorded hipGraph
    int m1h_its = 16;                    // fixed length of the M1h(h) PCG (12 reach 1e-14 on the Galewsky state at ne 2 ... 24)
    int steps = 0, redone = 0;           // steps taken; steps redone by the adaptive solvers after a missed check
    long host_reads = 0;                 // device-to-host reads solve_rk made (one per step while every check holds)
    int recordings = 0;                  // graphs recorded
    int steps_M1 = 0;                    // length of the fixed M1 solves
    bool adaptive = false;               // the adaptive solvers are in force (after a missed check)
    int graph_nodes() const { return have_graph ? gr.nodes() : 0; }      // launches of the recorded step (0: not recorded)

    struct Invariants { double mass, buoyancy, energy, enstrophy, vorticity, entropy; };

    // fg: the Coriolis 0-form (ThermalSW_EEC_2::coriolis, :166-212: PtQ 2 omega sin(lat) / M0), device, n0 entries; it must outlive the object.
    // nq: length of the quadrature-grid vectors init() takes (default: n0, the collocated grid of a global numbering)
    ThermalSW_EEC_2(Mesh* m, const double* fg_dev, int nq_ = -1) : mesh(m), fg(fg_dev), ksp1(m, KSP::CG), M1(m, nullptr, nullptr), m1(m, 1, 1.0, 0), log(m, NSLOT), gr(m) {
        if (m->nk_ != 1) throw std::invalid_argument("ThermalSW_EEC_2 needs a context with nk = 1");
        n0 = m->n0; n1 = m->n1; n2 = m->n2; nEl = m->nEl_; n2e = m->n2e;
        nq = nq_ > 0 ? nq_ : n0;
        nd1 = 2*(n1e_of(n2e));
        for (double** p : {&ui, &uj, &b1, &F, &G, &gh, &gs, &fu, &dd, &x1, &r1h, &z1h, &p1h, &Ap1h, &w1}) *p = mem.get(n1);
        for (double** p : {&hi, &Si, &hj, &Sj, &s, &Phi, &h2, &t2, &t2b, &ones2}) *p = mem.get(n2);
        for (double** p : {&m0, &m0fg, &q, &w0, &m0h, &ones0, &e0}) *p = mem.get(n0);
        sc = mem.get(8); inv = mem.get(8);
        m2inv = mem.get((size_t)nEl*n2e*n2e);
        pcb = mem.get((size_t)nEl*nd1*nd1);
        mimsem_ctx* c = mesh->ctx;
        check(mimsem_op_element_matrices(c, MIMSEM_OP_WMATINV, 0, 1.0, 0, nullptr, m2inv), "WMATINV");      // M2_e^-1: M2 is element-block diagonal
        check(mimsem_pvec(c, 0, 1, 1.0, nullptr, 0, m0, 0), "mimsem_pvec");                                // M0 is diagonal (collocated 0-forms)
        mesh->combine(n0, 1.0, m0, 1, fg, 0.0, nullptr, m0fg);
        mesh->combine(n0, 1.0, m0, 2, m0, 0.0, nullptr, ones0);
        {   // int2(h) = h . WtQ 1
            DeviceArrays tmp;
            double* oq = tmp.get(nq);
            std::vector<double> one((size_t)nq, 1.0);
            check(mimsem_memcpy_h2d(c, oq, one.data(), (long long)nq*8), "h2d");
            check(mimsem_op_apply(c, MIMSEM_OP_WTQ, 0, 1, 1.0, 0, nullptr, 0, oq, 0, ones2, 0, 1.0), "WTQ");
            check(mimsem_ctx_sync(c), "sync");
        }
        unit_thickness_or_throw();
        // ksp (M1, PCBJACOBI; src/ThermalSW_EEC_2.cpp:77-85): the element blocks, and the spectral interval of P M1 for the fixed-length solves,
        // derived as src::SWEqn::setup does.  (The check norms of a solve stay two dots here: the recorded step keeps its launches.)
        M1.assemble(0, 1.0, false); ksp1.setOperators(M1); ksp1.setPCBJacobi(); ksp1.setTolerances(rtol, 1.0e-50, 1000);
        const double *blocks1 = nullptr, *escale1 = nullptr;
        ksp1.pcBlocks(&blocks1, &escale1);
        m1.use_blocks(blocks1, escale1); m1.log_two_dots = true;
        if (!m1.calibrate([&](int mm, double* lo, double* hi, double* im) { ksp1.ritz(mm, lo, hi, im); }, rtol, 0.4, cheb::NO_CAP))
            throw std::runtime_error("ThermalSW_EEC_2: the preconditioned M1 has no usable spectral interval");
        steps_M1 = m1.steps;
    }
    ThermalSW_EEC_2(const ThermalSW_EEC_2&) = delete; ThermalSW_EEC_2& operator=(const ThermalSW_EEC_2&) = delete;

    // GalewskyTSW_2 main (src/GalewskyTSW_2.cpp:118-126) from the quadrature-grid fields (device: uq [nq][2], hq, sq [nq]):
    // u = M1^-1 UtQ uq, h = M2^-1 WtQ hq, s likewise, S = M2^-1 M2h(h) s
    void init(const double* uq, const double* hq, const double* sq, double* u, double* h, double* S) {
        mimsem_ctx* c = mesh->ctx;
        check(mimsem_op_apply(c, MIMSEM_OP_UTQ, 0, 1, 1.0, 0, nullptr, 0, uq, 0, b1, 0, 1.0), "UTQ");
        log.rewind();
        solve_M1(b1, u);
        if (!read_and_check(false)) { adaptive = true; solve_M1(b1, u); }
        check(mimsem_op_apply(c, MIMSEM_OP_WTQ, 0, 1, 1.0, 0, nullptr, 0, hq, 0, t2, 0, 1.0), "WTQ");
        M2inv(t2, h);
        check(mimsem_op_apply(c, MIMSEM_OP_WTQ, 0, 1, 1.0, 0, nullptr, 0, sq, 0, t2, 0, 1.0), "WTQ");
        M2inv(t2, s);
        check(mimsem_op_apply(c, MIMSEM_OP_WHMAT, 0, 1, 1.0, 0, h, 0, s, 0, t2, 0, 1.0), "WHMAT");
        M2inv(t2, S);
        check(mimsem_ctx_sync(c), "sync");
    }

    // ThermalSW_EEC_2::solve_rk(dt) (:859-1004): u, h, S (device) advanced by one step in place
    void solve_rk(double* u, double* h, double* S, double dt) {
        if (adaptive) { body(u, h, S, dt); steps++; return; }
        const bool key = have_graph && dt == g_dt && u == g_u && h == g_h && S == g_S;
        if (use_graph && key) gr.launch();
        else body(u, h, S, dt);                        // eagerly (the first time: the library's workspaces get their sizes)
        if (read_and_check()) {
            if (use_graph && !key) {                   // ... and recorded for every later step with these arrays (recording executes nothing)
                gr.record([&] { body(u, h, S, dt); });
                have_graph = true; recordings++; g_dt = dt; g_u = u; g_h = h; g_S = S;
            }
            steps++;
            return;
        }
        // a missed check: the step again from its start state with the adaptive solvers (kept from here on)
        redone++; adaptive = true;
        mesh->copy(n1, ui, u); mesh->copy(n2, hi, h); mesh->copy(n2, Si, S);
        body(u, h, S, dt);
        steps++;
    }

    // writeConservation (:765-858) as ThermalSW.invariants computes them: mass int2(h), buoyancy int2(S), energy intE(u, h, S),
    // enstrophy q^T M0h q, vorticity sum M0 w, entropy 1/2 (M2 M2h(h)^-1 M2 S) . S.  intE = int 1/2 (S h + h |u|^2) is formed from the
    // mass operators: the quadrature sums of S^T M2 h and u^T M1h(h) u are those of the point-wise integral (interp2_g = h_l / det,
    // interp1_g = J u_l / det), summed in another order.  One read.
    Invariants invariants(const double* u, const double* h, const double* S) {
        mimsem_ctx* c = mesh->ctx;
        check(mimsem_krylov_rowdot(c, 1, n2, h, 0, ones2, 0, inv + 0), "rowdot");
        check(mimsem_krylov_rowdot(c, 1, n2, S, 0, ones2, 0, inv + 1), "rowdot");
        check(mimsem_op_apply(c, MIMSEM_OP_WMAT, 0, 1, 1.0, 0, nullptr, 0, h, 0, t2, 0, 1.0), "WMAT");
        check(mimsem_krylov_rowdot(c, 1, n2, S, 0, t2, 0, inv + 2), "rowdot");
        check(mimsem_op_apply(c, MIMSEM_OP_UHMAT, 0, 1, 1.0, 0, h, 0, u, 0, w1, 0, 1.0), "UHMAT");
        check(mimsem_krylov_rowdot(c, 1, n1, u, 0, w1, 0, inv + 3), "rowdot");
        diagnose_q(u, h);                               // q, m0h, w0 = E01 M1 u
        mesh->combine(n0, 1.0, q, 1, m0h, 0.0, nullptr, e0);
        check(mimsem_krylov_rowdot(c, 1, n0, e0, 0, q, 0, inv + 4), "rowdot");
        check(mimsem_krylov_rowdot(c, 1, n0, w0, 0, ones0, 0, inv + 5), "rowdot");
        check(mimsem_op_apply(c, MIMSEM_OP_WMAT, 0, 1, 1.0, 0, nullptr, 0, S, 0, t2, 0, 1.0), "WMAT");
        check(mimsem_op_apply(c, MIMSEM_OP_WHMATINV, 0, 1, 1.0, 0, h, 0, t2, 0, t2b, 0, 1.0), "WHMATINV");
        check(mimsem_op_apply(c, MIMSEM_OP_WMAT, 0, 1, 1.0, 0, nullptr, 0, t2b, 0, t2, 0, 1.0), "WMAT");
        check(mimsem_krylov_rowdot(c, 1, n2, t2, 0, S, 0, inv + 6), "rowdot");
        double v[8];
        mesh->to_host(v, inv, 7);
        return Invariants{v[0], v[1], 0.5*(v[2] + v[3]), v[4], v[5], 0.5*v[6]};
    }

private:
    static constexpr int NSLOT = 18;     // 15 fixed M1 solves and 3 M1h solves per step
    static constexpr double RK3[3][2] = {{0.0, 1.0}, {0.75, 0.25}, {1.0/3.0, 2.0/3.0}};      // (alpha, beta) of the stages, :894-1000
    Mesh* mesh; const double* fg;
    KSP ksp1; mimsem_host::Umat M1;
    DeviceArrays mem; FixedMassSolve m1; CheckLog log; Graph gr;
    bool have_graph = false; double g_dt = 0.0; const double *g_u = nullptr, *g_h = nullptr, *g_S = nullptr;
    int n0 = 0, n1 = 0, n2 = 0, nEl = 0, n2e = 0, nq = 0, nd1 = 0;
    double *ui, *uj, *b1, *F, *G, *gh, *gs, *fu, *dd, *x1, *r1h, *z1h, *p1h, *Ap1h, *w1;
    double *hi, *Si, *hj, *Sj, *s, *Phi, *h2, *t2, *t2b, *ones2;
    double *m0, *m0fg, *q, *w0, *m0h, *ones0, *e0, *sc, *inv, *m2inv, *pcb;

    static int n1e_of(int n2e_) { const int n = (int)std::lround(std::sqrt((double)n2e_)); return n*(n + 1); }
    void M2inv(const double* x, double* y) { check(mimsem_elem_blocks_apply(mesh->ctx, 2, 1, 0, m2inv, 0, nullptr, 0, x, 0, y, 0, 1.0), "M2^-1"); }
    void E(int which, const double* x, double* y) { check(mimsem_incidence_apply(mesh->ctx, which, 1, x, 0, y, 0), "mimsem_incidence_apply"); }
    void apply(int op, const double* f, const double* x, double* y, double alpha = 1.0, unsigned flags = 0) {
        check(mimsem_op_apply(mesh->ctx, op, 0, 1, 1.0, flags, f, 0, x, 0, y, 0, alpha), "mimsem_op_apply");
    }
    // ThermalSW.check / MassSolver.verify: a fixed M1 solve's last preconditioned residual within 30 rtol |P b|, an M1h solve's true residual
    // within 30 rtol |b|.  ONE read of the whole log
    bool read_and_check(bool count = true) {
        double v[2*NSLOT];
        if (log.size() == 0) return true;
        log.read(v, log.size());
        if (count) host_reads++;
        bool ok = true;
        for (int k = 0; k < log.size(); k++) ok = ok && cheb::accepted(v[2*k], v[2*k + 1], 30.0*rtol);
        return ok;
    }
    void unit_thickness_or_throw() {
        // M1 with and without the thickness factor agree on a non-constant vector only where thickInv == 1 (the src flavour)
        std::vector<double> hv((size_t)n1);
        for (int i = 0; i < n1; i++) hv[(size_t)i] = 1.0 + 0.001*(i%97);
        check(mimsem_memcpy_h2d(mesh->ctx, b1, hv.data(), (long long)n1*8), "h2d");
        apply(MIMSEM_OP_UMAT, nullptr, b1, F);
        apply(MIMSEM_OP_UMAT, nullptr, b1, G, 1.0, MIMSEM_FLAG_VERT);
        mesh->combine(n1, 1.0, F, 0, nullptr, -1.0, G, G);
        check(mimsem_krylov_rowdot(mesh->ctx, 1, n1, G, 0, G, 0, sc), "rowdot");
        double d2 = -1.0;
        mesh->to_host(&d2, sc, 1);
        if (d2 != 0.0) throw std::invalid_argument("ThermalSW_EEC_2 needs unit thickness (the src flavour: levels 0 and 1)");
    }

    // KSPSolve(ksp, b, x) on M1
    void solve_M1(const double* b, double* out) {
        if (adaptive) { ksp1.solve(b, out); return; }
        check(m1.solve(b, out, log), "FixedMassSolve::solve");
    }
    // KSPSolve(ksp1h, b, d) on M1h(h) (diagnose_ds :253-268): PCG with the element blocks of M1h(h) (PCSetUp: rebuilt every stage, one launch).
    // Fixed length: the true residual logged for the step's check.  Adaptive: to rtol, the residual read every 4 iterations
    void solve_M1h(const double* h, const double* b, double* x) {
        mimsem_ctx* c = mesh->ctx;
        check(mimsem_elem_block_pc_build(c, MIMSEM_OP_UHMAT, 0, 1.0, 0, h, pcb), "mimsem_elem_block_pc_build");
        auto A = [&](const double* v, double* y) { apply(MIMSEM_OP_UHMAT, h, v, y); };
        auto P = [&](const double* r, double* z) {
            check(mimsem_elem_blocks_apply(c, 1, 1, MIMSEM_FLAG_TRANSPOSE, pcb, 0, nullptr, 0, r, 0, z, 0, 1.0), "mimsem_elem_blocks_apply");
        };
        double *rz = sc, *rzn = sc + 1, *pAp = sc + 2, *rr = sc + 3, *bb = sc + 4;
        check(mimsem_memset(c, x, 0, (long long)n1*8), "mimsem_memset");
        mesh->copy(n1, b, r1h);
        P(r1h, z1h);
        mesh->copy(n1, z1h, p1h);
        check(mimsem_krylov_rowdot(c, 1, n1, r1h, 0, z1h, 0, rz), "rowdot");
        if (!adaptive) {
            for (int it = 0; it < m1h_its; it++) {
                cg_iteration(A, P, x, rz, rzn, pAp);
                std::swap(rz, rzn);
            }
            A(x, Ap1h);
            mesh->combine(n1, 1.0, b, 0, nullptr, -1.0, Ap1h, r1h);                       // the true residual
            log.two(r1h, b, n1);
            return;
        }
        check(mimsem_krylov_rowdot(c, 1, n1, b, 0, b, 0, bb), "rowdot");
        for (int it = 1; it <= 1000; it++) {
            cg_iteration(A, P, x, rz, rzn, pAp);
            std::swap(rz, rzn);
            if (it%4 == 0) {
                check(mimsem_krylov_rowdot(c, 1, n1, r1h, 0, r1h, 0, rr), "rowdot");
                double v[5];
                mesh->to_host(v, sc, 5);
                host_reads++;
                if (v[3] < rtol*rtol*std::max(v[4], 1e-300)) return;
            }
        }
        throw std::runtime_error("ThermalSW_EEC_2: the M1h(h) CG did not reach rtol in 1000 iterations");
    }
    template <class FA, class FP> void cg_iteration(FA& A, FP& P, double* x, const double* rz, double* rzn, double* pAp) {
        mimsem_ctx* c = mesh->ctx;
        A(p1h, Ap1h);
        check(mimsem_krylov_rowdot(c, 1, n1, p1h, 0, Ap1h, 0, pAp), "rowdot");
        check(mimsem_krylov_cg_update(c, 1, n1, rz, pAp, p1h, 0, Ap1h, 0, x, 0, r1h, 0), "mimsem_krylov_cg_update");
        P(r1h, z1h);
        check(mimsem_krylov_rowdot(c, 1, n1, r1h, 0, z1h, 0, rzn), "rowdot");
        check(mimsem_krylov_cg_direction(c, 1, n1, rzn, rz, z1h, 0, p1h, 0), "mimsem_krylov_cg_direction");
    }
    // diagnose_q (:227-239): M0h(h) q = E01 M1 u + M0 f (Phmat is diagonal at GLL collocation); leaves m0h and w0 = E01 M1 u
    void diagnose_q(const double* u, const double* h) {
        apply(MIMSEM_OP_UMAT, nullptr, u, w1);
        E(3, w1, w0);
        mesh->combine(n0, 1.0, m0fg, 0, nullptr, 1.0, w0, q);
        check(mimsem_pvec(mesh->ctx, 0, 1, 1.0, h, 0, m0h, 0), "mimsem_pvec");
        mesh->combine(n0, 1.0, q, 2, m0h, 0.0, nullptr, q);
    }
    // grad (:154-164): M1^-1 E12 M2 phi
    void grad(const double* phi, double* out) {
        apply(MIMSEM_OP_WMAT, nullptr, phi, t2);
        E(2, t2, b1);
        solve_M1(b1, out);
    }
    // one stage from (uj, hj, Sj): uj <- the new u, hj and Sj updated in place (ThermalSW.stage)
    void stage(double dt, double alpha, double beta) {
        mimsem_ctx* c = mesh->ctx;
        check(mimsem_tsw_diagnose(c, hj, Sj, uj, m2inv, s, Phi, h2), "mimsem_tsw_diagnose");
        apply(MIMSEM_OP_UHMAT, hj, uj, b1);
        solve_M1(b1, F);                                                             // diagnose_F
        apply(MIMSEM_OP_WMAT, nullptr, s, t2);
        E(2, t2, b1);
        solve_M1h(hj, b1, dd);                                                       // diagnose_ds: then K <- K(d), M1h <- M1h(s)
        apply(MIMSEM_OP_UHMAT, s, F, b1);
        solve_M1(b1, G);                                                             // diagnose_G
        grad(hj, gh); grad(s, gs);
        E(2, Phi, fu);                                                               // rhs_u :1045-1093
        diagnose_q(uj, hj);
        apply(MIMSEM_OP_ROTMAT, q, F, fu, 1.0, MIMSEM_FLAG_ACCUM);
        apply(MIMSEM_OP_UHMAT, s, gh, fu, 0.25, MIMSEM_FLAG_ACCUM);                 // 1/4 M1h(s) grad h
        apply(MIMSEM_OP_UTQWMAT, dd, h2, fu, -0.25, MIMSEM_FLAG_ACCUM);             // -1/2 K(d)^T h2 = -1/4 UtQWmat(d) h2
        mesh->combine(n1, alpha, ui, 0, nullptr, beta, uj, x1);
        apply(MIMSEM_OP_UMAT, nullptr, x1, b1);
        mesh->combine(n1, -(beta*dt), fu, 0, nullptr, 1.0, b1, b1);
        solve_M1(b1, uj);
        check(mimsem_tsw_update(c, F, G, gs, s, m2inv, hi, Si, hj, Sj, alpha, beta, dt), "mimsem_tsw_update");
    }
    // the whole step: (u, h, S) -> start state and stage state, three stages, back into (u, h, S)
    void body(double* u, double* h, double* S, double dt) {
        log.rewind();
        mesh->copy(n1, u, ui); mesh->copy(n2, h, hi); mesh->copy(n2, S, Si);
        mesh->copy(n1, u, uj); mesh->copy(n2, h, hj); mesh->copy(n2, S, Sj);
        for (int k = 0; k < 3; k++) stage(dt, RK3[k][0], RK3[k][1]);
        mesh->copy(n1, uj, u); mesh->copy(n2, hj, h); mesh->copy(n2, Sj, S);
    }
};

}  // namespace src
}  // namespace mimsem_host
