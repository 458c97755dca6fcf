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
// Every solve logs {|residual|^2, |reference|^2} into one device array; the step reads it ONCE at its end (host_reads) and accepts it by the
// rules of ThermalSW.check / MassSolver.verify.  A missed check redoes the step eagerly with adaptive solvers -- CG on M1 to rtol (class KSP)
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
#include "mimsem_sweqn.hpp"

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
    ThermalSW_EEC_2(Mesh* m, const double* fg_dev, int nq_ = -1) : mesh(m), fg(fg_dev), ksp1(m, KSP::CG), M1(m), gr(m) {
        if (m->nk_ != 1) throw std::invalid_argument("ThermalSW_EEC_2 needs a context with nk = 1");
        n0 = m->n0; n1 = m->n1; n2 = m->n2; nEl = m->nEl_; n2e = m->n2e;
        nq = nq_ > 0 ? nq_ : n0;
        nd1 = 2*(n1e_of(n2e));
        try {
            for (double** p : {&ui, &uj, &b1, &F, &G, &gh, &gs, &fu, &dd, &x1, &r1h, &z1h, &p1h, &Ap1h, &w1}) *p = device(n1);
            for (double** p : {&hi, &Si, &hj, &Sj, &s, &Phi, &h2, &t2, &t2b, &ones2}) *p = device(n2);
            for (double** p : {&m0, &m0fg, &q, &w0, &m0h, &ones0, &e0}) *p = device(n0);
            pair1 = device(2*even(n1)); upd1 = pair1; t1 = pair1 + even(n1);
            chk = device(2*NSLOT); sc = device(8); inv = device(8);
            m2inv = device((size_t)nEl*n2e*n2e);
            pcb = device((size_t)nEl*nd1*nd1);
            mimsem_ctx* c = mesh->ctx;
            check(mimsem_op_element_matrices(c, MIMSEM_OP_WMATINV, 0, 1.0, 0, nullptr, m2inv), "WMATINV");      // M2_e^-1: M2 is element-block diagonal
            check(mimsem_pvec(c, 0, 1, 1.0, nullptr, 0, m0, 0), "mimsem_pvec");                                // M0 is diagonal (collocated 0-forms)
            combine(n0, 1.0, m0, 1, fg, 0.0, nullptr, m0fg);
            combine(n0, 1.0, m0, 2, m0, 0.0, nullptr, ones0);
            {   // int2(h) = h . WtQ 1
                double* oq = device(nq);
                std::vector<double> one((size_t)nq, 1.0);
                check(mimsem_memcpy_h2d(c, oq, one.data(), (long long)nq*8), "h2d");
                const int rc = mimsem_op_apply(c, MIMSEM_OP_WTQ, 0, 1, 1.0, 0, nullptr, 0, oq, 0, ones2, 0, 1.0);
                check(mimsem_ctx_sync(c), "sync");
                mimsem_free(oq);
                check(rc, "WTQ");
            }
            unit_thickness_or_throw();
            // ksp (M1, PCBJACOBI; src/ThermalSW_EEC_2.cpp:77-85): the element blocks, and the spectral interval of P M1 for the fixed-length solves,
            // derived as src::SWEqn::setup does -- Ritz values at 25 and 40 Arnoldi steps, margins from how far the ends moved, cheb::ellipse
            M1.assemble(); ksp1.setOperators(M1); ksp1.setPCBJacobi(); ksp1.setTolerances(rtol, 1.0e-50, 1000);
            ksp1.pcBlocks(&blocks1, &escale1);
            double lo = 0.0, hi_ = 0.0, im = 0.0, lo25 = 0.0, hi25 = 0.0;
            for (const int mm : {25, 40}) { lo25 = lo; hi25 = hi_; ksp1.ritz(mm, &lo, &hi_, &im); }
            if (!(lo > 0.02)) throw std::runtime_error("ThermalSW_EEC_2: the preconditioned M1 has no usable spectral interval");
            const double mlo = 1.0 - std::min(0.4, std::max(0.01, 3.0*std::fabs(lo - lo25)/lo));
            const double mhi = 1.0 + std::max(0.01, 3.0*std::fabs(hi_ - hi25)/hi_);
            const double l1 = mlo*lo, l2 = mhi*hi_;
            steps_M1 = std::max(2, (int)std::ceil(std::log(2.0/rtol)/std::log(1.0/cheb::interval_rate(l1, l2))));
            for (const auto& ab : cheb::ellipse(0.5*(l1 + l2), 0.25*(l2 - l1)*(l2 - l1), steps_M1)) { coefM.push_back(ab.first); coefM.push_back(ab.second); }
        } catch (...) { release(); throw; }              // (a constructor that throws runs no destructor)
    }
    ~ThermalSW_EEC_2() { release(); }
    ThermalSW_EEC_2(const ThermalSW_EEC_2&) = delete; ThermalSW_EEC_2& operator=(const ThermalSW_EEC_2&) = delete;

    // GalewskyTSW_2 main (src/GalewskyTSW_2.cpp:118-126) from the quadrature-grid fields (device: uq [nq][2], hq, sq [nq]):
    // u = M1^-1 UtQ uq, h = M2^-1 WtQ hq, s likewise, S = M2^-1 M2h(h) s
    void init(const double* uq, const double* hq, const double* sq, double* u, double* h, double* S) {
        mimsem_ctx* c = mesh->ctx;
        check(mimsem_op_apply(c, MIMSEM_OP_UTQ, 0, 1, 1.0, 0, nullptr, 0, uq, 0, b1, 0, 1.0), "UTQ");
        slot = 0;
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
        copy(n1, ui, u); copy(n2, hi, h); copy(n2, Si, S);
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
        combine(n0, 1.0, q, 1, m0h, 0.0, nullptr, e0);
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
    enum LogKind { K_M1 = 1, K_M1H = 2 };
    struct MassOp : OperatorBase { explicit MassOp(Mesh* m) : OperatorBase(m, MIMSEM_OP_UMAT) {} void assemble() { up = false; field = nullptr; } };
    Mesh* mesh; const double* fg;
    KSP ksp1; MassOp M1; Graph gr;
    bool have_graph = false; double g_dt = 0.0; const double *g_u = nullptr, *g_h = nullptr, *g_S = nullptr;
    int n0 = 0, n1 = 0, n2 = 0, nEl = 0, n2e = 0, nq = 0, nd1 = 0;
    const double *blocks1 = nullptr, *escale1 = nullptr;
    std::vector<double> coefM;
    int slot = 0; int kinds[NSLOT] = {0};
    double *ui = nullptr, *uj = nullptr, *b1 = nullptr, *F = nullptr, *G = nullptr, *gh = nullptr, *gs = nullptr, *fu = nullptr, *dd = nullptr,
           *x1 = nullptr, *r1h = nullptr, *z1h = nullptr, *p1h = nullptr, *Ap1h = nullptr, *w1 = nullptr;
    double *hi = nullptr, *Si = nullptr, *hj = nullptr, *Sj = nullptr, *s = nullptr, *Phi = nullptr, *h2 = nullptr, *t2 = nullptr, *t2b = nullptr, *ones2 = nullptr;
    double *m0 = nullptr, *m0fg = nullptr, *q = nullptr, *w0 = nullptr, *m0h = nullptr, *ones0 = nullptr, *e0 = nullptr;
    double *pair1 = nullptr, *upd1 = nullptr, *t1 = nullptr, *chk = nullptr, *sc = nullptr, *inv = nullptr, *m2inv = nullptr, *pcb = nullptr;

    static int n1e_of(int n2e_) { const int n = (int)std::lround(std::sqrt((double)n2e_)); return n*(n + 1); }
    static size_t even(long long n) { return (size_t)((n + 1) & ~1LL); }
    double* device(size_t n) { return mesh->device_alloc(std::max<size_t>(n, 1)); }
    void release() {
        for (double** p : {&ui, &uj, &b1, &F, &G, &gh, &gs, &fu, &dd, &x1, &r1h, &z1h, &p1h, &Ap1h, &w1, &hi, &Si, &hj, &Sj, &s, &Phi, &h2, &t2, &t2b,
                           &ones2, &m0, &m0fg, &q, &w0, &m0h, &ones0, &e0, &pair1, &chk, &sc, &inv, &m2inv, &pcb}) { if (*p) mimsem_free(*p); *p = nullptr; }
        upd1 = t1 = nullptr;
    }
    void combine(long long n, double a, const double* A, int op, const double* B, double b, const double* C, double* out) {
        check(mimsem_vec_combine(mesh->ctx, 1, n, a, A, 0, op, B, 0, b, C, 0, out, 0), "mimsem_vec_combine");
    }
    void copy(long long n, const double* a, double* out) { combine(n, 1.0, a, 0, nullptr, 0.0, nullptr, out); }
    void M2inv(const double* x, double* y) { check(mimsem_elem_blocks_apply(mesh->ctx, 2, 1, 0, m2inv, 0, nullptr, 0, x, 0, y, 0, 1.0), "M2^-1"); }
    void E(int which, const double* x, double* y) { check(mimsem_incidence_apply(mesh->ctx, which, 1, x, 0, y, 0), "mimsem_incidence_apply"); }
    void apply(int op, const double* f, const double* x, double* y, double alpha = 1.0, unsigned flags = 0) {
        check(mimsem_op_apply(mesh->ctx, op, 0, 1, 1.0, flags, f, 0, x, 0, y, 0, alpha), "mimsem_op_apply");
    }
    void log_pair(int kind, const double* r, const double* ref, long long n) {
        if (slot >= NSLOT) throw std::runtime_error("ThermalSW_EEC_2: check-norm slots exhausted");
        kinds[slot] = kind;
        check(mimsem_krylov_rowdot(mesh->ctx, 1, n, r, n, r, n, chk + 2*slot), "mimsem_krylov_rowdot");
        check(mimsem_krylov_rowdot(mesh->ctx, 1, n, ref, n, ref, n, chk + 2*slot + 1), "mimsem_krylov_rowdot");
        slot++;
    }
    // ThermalSW.check / MassSolver.verify: a fixed M1 solve's last preconditioned residual within 30 rtol |P b|, an M1h solve's true residual
    // within 30 rtol |b| (NaN compares false: a miss).  ONE read of the whole log
    bool read_and_check(bool count = true) {
        double v[2*NSLOT];
        const int n = slot;
        if (n == 0) return true;
        mesh->to_host(v, chk, 2*(size_t)n);
        if (count) host_reads++;
        bool ok = true;
        for (int k = 0; k < n; k++) {
            const double r2 = v[2*k], ref2 = v[2*k + 1];
            if (kinds[k] == K_M1H) { if (!(r2 <= (30.0*rtol)*(30.0*rtol)*ref2)) ok = false; continue; }
            if (r2 == 0.0 && ref2 == 0.0) continue;
            const double rel = ref2 > 0.0 ? std::sqrt(r2/ref2) : HUGE_VAL;
            if (!(rel <= 30.0*rtol)) ok = false;
        }
        return ok;
    }
    void unit_thickness_or_throw() {
        // M1 with and without the thickness factor agree on a non-constant vector only where thickInv == 1 (the src flavour)
        std::vector<double> hv((size_t)n1);
        for (int i = 0; i < n1; i++) hv[(size_t)i] = 1.0 + 0.001*(i%97);
        check(mimsem_memcpy_h2d(mesh->ctx, b1, hv.data(), (long long)n1*8), "h2d");
        apply(MIMSEM_OP_UMAT, nullptr, b1, F);
        apply(MIMSEM_OP_UMAT, nullptr, b1, G, 1.0, MIMSEM_FLAG_VERT);
        combine(n1, 1.0, F, 0, nullptr, -1.0, G, G);
        check(mimsem_krylov_rowdot(mesh->ctx, 1, n1, G, 0, G, 0, sc), "rowdot");
        double d2 = -1.0;
        mesh->to_host(&d2, sc, 1);
        if (d2 != 0.0) throw std::invalid_argument("ThermalSW_EEC_2 needs unit thickness (the src flavour: levels 0 and 1)");
    }

    // KSPSolve(ksp, b, x) on M1
    void solve_M1(const double* b, double* out) {
        if (adaptive) { ksp1.solve(b, out); return; }
        check(mimsem_block_chebyshev_solve(mesh->ctx, MIMSEM_OP_UMAT, 0, 1, 1.0, 0, nullptr, 0, blocks1, escale1, 0, b, 0, (int)coefM.size()/2,
                                           coefM.data(), out, 0, t1, 0, upd1, 0), "mimsem_block_chebyshev_solve");
        log_pair(K_M1, upd1, t1, n1);
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
        copy(n1, b, r1h);
        P(r1h, z1h);
        copy(n1, z1h, p1h);
        check(mimsem_krylov_rowdot(c, 1, n1, r1h, 0, z1h, 0, rz), "rowdot");
        if (!adaptive) {
            for (int it = 0; it < m1h_its; it++) {
                cg_iteration(A, P, x, rz, rzn, pAp);
                std::swap(rz, rzn);
            }
            A(x, Ap1h);
            combine(n1, 1.0, b, 0, nullptr, -1.0, Ap1h, r1h);                       // the true residual
            log_pair(K_M1H, r1h, b, n1);
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
        combine(n0, 1.0, m0fg, 0, nullptr, 1.0, w0, q);
        check(mimsem_pvec(mesh->ctx, 0, 1, 1.0, h, 0, m0h, 0), "mimsem_pvec");
        combine(n0, 1.0, q, 2, m0h, 0.0, nullptr, q);
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
        combine(n1, alpha, ui, 0, nullptr, beta, uj, x1);
        apply(MIMSEM_OP_UMAT, nullptr, x1, b1);
        combine(n1, -(beta*dt), fu, 0, nullptr, 1.0, b1, b1);
        solve_M1(b1, uj);
        check(mimsem_tsw_update(c, F, G, gs, s, m2inv, hi, Si, hj, Sj, alpha, beta, dt), "mimsem_tsw_update");
    }
    // the whole step: (u, h, S) -> start state and stage state, three stages, back into (u, h, S)
    void body(double* u, double* h, double* S, double dt) {
        slot = 0;
        copy(n1, u, ui); copy(n2, h, hi); copy(n2, S, Si);
        copy(n1, u, uj); copy(n2, h, hj); copy(n2, S, Sj);
        for (int k = 0; k < 3; k++) stage(dt, RK3[k][0], RK3[k][1]);
        copy(n1, uj, u); copy(n2, hj, h); copy(n2, Sj, S);
    }
};

}  // namespace src
}  // namespace mimsem_host
