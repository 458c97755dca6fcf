// mimsem_vertsolve.hpp -- the vertical implicit solve (the caller of rows C5-C8) driven from C++ over the C ABI: the two Newton loops of the
// reference's VertSolve for EVERY column at once, on the fused entry points of the library.
//   VertSolveEta  VertSolve::solve_schur_eta (eul/VertSolve.cpp:1721-1973): per iteration mimsem_column_newton_residual (assemble_residual_ec with
//                 diagnose_F_z / diagnose_Phi_z, the EOS and entropy residuals: :237-286, :432-502, :1806-1851), mimsem_column_solve_schur_eta
//                 (:677-823: the linear solve) and mimsem_column_newton_update (:1858-1912); stops on the exner and rho norms
//   VertSolve2    VertSolve::solve_schur_2 (:1059-1246), the loop around solve_schur_column_3 and the vertical half of Euler::Strang: per iteration
//                 mimsem_column_newton2_residual (assemble_residual :386-430 and the right-hand sides of :1134-1154), mimsem_column_solve_schur_3
//                 (:504-675) and mimsem_column_newton2_update (:1159-1183); theta lives on the nk+1 interfaces only; stops on THREE norms (:1202).
//                 With theta_up / vert_mom_vort the loop of the box twin (box/VertSolve.cpp:1264-1458): theta from mimsem_column_diag_theta_wup,
//                 the u dw/dx term time-centred between udwdx and AssembleVertMomVort of the iterate
// Both then take the max-norms of VertSolve::MaxNorm (:228: mimsem_column_max_norms) and mimsem_column_diag_theta_blend (diagTheta2 / diagTheta_L2
// :289-352 with the half-time blend): VertNewton below is that shared loop.  All state in the "vertical" layout of L2Vecs::vz: [nEl][slots*n2e], velz
// on the nk-1 interfaces, theta on nk+1, the rest on the nk levels.  Orders 1..4 (the fused entries' range).  Header-only, C++17, no HIP toolchain.
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include "mimsem_mass.hpp"

namespace mimsem_host {

// What the two loops share: the arrays both use, copy-in and copy-out, the norms, the theta diagnosis, k2i_z.  A solve hands newton() its own
// iteration (forcing, residual, linear solve, update) and its own record of the norms.
class VertNewton {
public:
    double k2i_z = 0.0;                               // VertSolve::k2i_z of the last iteration (:415-416)
    double rayleigh = 4.0/120.0;                      // RAYLEIGH, eul/VertSolve.cpp:32 (the sponge layer at the model top; 0 switches it off)
    // the horizontal transport tendencies the loop adds: forcing(rho_i, rho_j, theta, add_rho, add_rt) fills the two output arrays ([nEl][nk*n2e]);
    // empty = no horizontal wind.  theta is theta_l2_h on the levels for VertSolveEta (advection_rhs_ec, :1799, :1822-1826) and theta_h on the
    // nk+1 interfaces for VertSolve2 (advection_rhs, :1124: the two join dF_z / dG_z BEFORE the VB product, :1145-1146)
    std::function<void(const double*, const double*, const double*, double*, double*)> horiz_forcing;
    // Several ranks (round 6): the columns of an element live on ONE rank, so the solve needs no exchange at all -- what crosses
    // ranks is the reference's MPI_Allreduce(MAX) of the four update norms per iteration (eul/VertSolve.cpp:1915-1918, :1195-1198: every rank must
    // stop at the same iteration) and the sum of k2i_z.  A host with more than one rank sets the two callbacks (in place, n host doubles;
    // MPI_Allreduce with MPI_MAX / MPI_SUM on MPI_COMM_WORLD); unset = one rank.
    std::function<void(double*, int)> allreduce_max, allreduce_sum;

    VertNewton(const VertNewton&) = delete; VertNewton& operator=(const VertNewton&) = delete;
    const double* theta_half() const { return theta_h; }          // [nEl][(nk+1)*n2e]
    const double* exner_half() const { return exner_h; }

protected:
    VertNewton(Mesh* m, double dt_) : mesh(m), dt(dt_) {
        nEl = m->nEl_; n2 = m->n2e; nk = m->nk_;
        nl = (size_t)nEl*nk*n2; ni = (size_t)nEl*(nk - 1)*n2; nt = (size_t)nEl*(nk + 1)*n2;
        for (double** p : {&velz_j, &velz_h, &F_w, &d_w, &k2i, &ones_i}) *p = mem.get(ni);
        for (double** p : {&rho_j, &rt_j, &exner_j, &rho_h, &rt_h, &exner_h, &F_rho, &F_exner, &d_rho, &d_exner, &add_rho, &add_rt}) *p = mem.get(nl);
        for (double** p : {&theta_i, &theta_h}) *p = mem.get(nt);
        nrm = mem.get(8*nl); sums = mem.get((size_t)4*nEl + 4);
        // a vector of ones as long as an interface field: the sum of k2i is a row dot with it
        std::vector<double> one(ni, 1.0);
        check(mimsem_memcpy_h2d(mesh->ctx, ones_i, one.data(), (long long)ni*8), "h2d");
    }

    // The loop: velz / rho / rt / exner at the old time level in, at the new one out (in place).  step() is one iteration up to and including the
    // update, which leaves the squares in nrm; record(mx) keeps the four norms and says whether to stop.  Returns the number of iterations run.
    // theta_up: theta_i / theta_h from diagTheta2 with the test functions upwinded by velz / velz_j over 0.25 dt (box/VertSolve.cpp:1312, :1394-1399;
    // that loop has no level arrays); after(): what follows the theta diagnosis of an iteration (box :1403).
    template <class Step, class Record>
    int newton(double* velz, double* rho, double* rt, double* exner, int maxit, Step step, Record record) {
        return newton(velz, rho, rt, exner, maxit, step, record, false, [] {});
    }
    template <class Step, class Record, class After>
    int newton(double* velz, double* rho, double* rt, double* exner, int maxit, Step step, Record record, bool theta_up, After after) {
        mimsem_ctx* c = mesh->ctx;
        mesh->copy(ni, velz, velz_j); mesh->copy(nl, rho, rho_j); mesh->copy(nl, rt, rt_j); mesh->copy(nl, exner, exner_j);      // :1099-1102
        // diagTheta2 (:1766, :1105) and, for the loop that has the level arrays, diagTheta_L2 (:1773)
        if (theta_up) check(mimsem_column_diag_theta_wup(c, 0.25*dt, rho, rt, velz, theta_i, nullptr, 1.0, 0.0), "diag_theta_wup");
        else check(mimsem_column_diag_theta_blend(c, rho, rt, theta_i, nullptr, theta_l2_i, nullptr, 1.0, 0.0), "diag_theta_blend");
        mesh->copy(nt, theta_i, theta_h);
        if (theta_l2_i) mesh->copy(nl, theta_l2_i, theta_l2_h);
        mesh->copy(nl, exner, exner_h); mesh->copy(ni, velz, velz_h); mesh->copy(nl, rho, rho_h); mesh->copy(nl, rt, rt_h);       // :1112-1117
        int it = 0;
        for (it = 1; it <= maxit; it++) {
            step();
            // MaxNorm (:228): per column sqrt(sum d^2 / sum x^2), the maximum over the columns (the rank-local part of the MPI_Allreduce(MAX))
            check(mimsem_column_max_norms(c, nrm, sums, sums + 4*(size_t)nEl), "column_max_norms");
            // (the theta diagnosis does not depend on the norms: launched before the host waits for them)                   :1896-1912, :1186-1191
            if (theta_up) check(mimsem_column_diag_theta_wup(c, 0.25*dt, rho_j, rt_j, velz_j, theta_h, theta_i, 0.5, 0.5), "diag_theta_wup");
            else check(mimsem_column_diag_theta_blend(c, rho_j, rt_j, theta_h, theta_i, theta_l2_h, theta_l2_i, 0.5, 0.5), "diag_theta_blend");
            after();                     // (before the norms are read: on the LAST iteration too, as box :1403 and the Python loop have it)
            double mx[4];
            mesh->to_host(mx, sums + 4*(size_t)nEl, 4);
            if (allreduce_max) allreduce_max(mx, 4);                                                                        // :1915-1918, :1195-1198
            if (record(mx)) break;
        }
        // k2i_z = sum(F_z . VA(theta) grad Pi) / SCALE of the last iteration
        double s = 0.0;
        check(mimsem_krylov_rowdot(c, 1, (long long)ni, k2i, (long long)ni, ones_i, 0, sums), "krylov_rowdot");
        mesh->to_host(&s, sums, 1);
        if (allreduce_sum) allreduce_sum(&s, 1);
        k2i_z = s/1.0e8;
        mesh->copy(ni, velz_j, velz); mesh->copy(nl, rho_j, rho); mesh->copy(nl, rt_j, rt); mesh->copy(nl, exner_j, exner);       // :1209-1212
        return std::min(it, maxit);
    }

    Mesh* mesh; double dt; DeviceArrays mem;
    int nEl = 0, n2 = 0, nk = 0; size_t nl = 0, ni = 0, nt = 0;
    double *velz_j, *velz_h, *F_w, *d_w, *k2i, *ones_i;
    double *rho_j, *rt_j, *exner_j, *rho_h, *rt_h, *exner_h, *F_rho, *F_exner, *d_rho, *d_exner, *add_rho, *add_rt;
    double *theta_i, *theta_h, *nrm, *sums;
    double *theta_l2_i = nullptr, *theta_l2_h = nullptr;       // VertSolveEta's alone: null = no diagTheta_L2
};

class VertSolveEta : public VertNewton {
public:
    struct Norms { double exner, w, rho, eta; };
    std::vector<Norms> history;                       // |d x| / |x| (max over the columns) of the iterations of the last solve

    VertSolveEta(Mesh* m, double dt_) : VertNewton(m, dt_) {
        for (double** p : {&theta_l2_i, &theta_l2_h, &F_eta, &d_eta, &th_w3, &eta}) *p = mem.get(nl);
    }

    // VertSolve::solve_schur_eta: zv from VertSolve::initGZ.  udwdx (nullable, [nEl][(nk-1)*n2e]): the u dw/dx term (:1809); hs_lat (nullable,
    // [nEl][mp12]): the Held-Suarez temperature forcing.  theta_h / theta_l2_h / exner_h (what the horizontal corrector reads) stay in the accessors.
    int solve_schur_eta(double* velz, double* rho, double* rt, double* exner, const double* zv, int maxit = 20, double tol = 1.0e-12,
                        const double* udwdx = nullptr, const double* hs_lat = nullptr) {
        mimsem_ctx* c = mesh->ctx;
        history.clear();
        return newton(velz, rho, rt, exner, maxit, [&] {
            const double *a_rho = nullptr, *a_rt = nullptr;
            if (horiz_forcing) { horiz_forcing(rho, rho_j, theta_l2_h, add_rho, add_rt); a_rho = add_rho; a_rt = add_rt; }
            if (hs_lat) {                                                                                                                // :1831-1834
                double* dst = a_rt ? th_w3 : add_rt;                       // (th_w3 is free until the residual call below fills it)
                check(mimsem_column_temp_forcing_hs(c, hs_lat, exner_h, theta_h, rho_h, dst), "temp_forcing_hs");
                if (a_rt) check(mimsem_vec_combine(c, 1, (long long)nl, 1.0, th_w3, 0, 0, nullptr, 0, 1.0, add_rt, 0, add_rt, 0), "vec_combine");
                a_rt = add_rt;
            }
            check(mimsem_column_newton_residual(c, dt, rayleigh, theta_l2_h, exner_h, velz, velz_j, rho, rho_j, zv, rt, rt_j, rho_h, rt_h, exner_j,
                                                udwdx, a_rho, a_rt, F_w, F_rho, F_eta, F_exner, th_w3, eta, k2i), "newton_residual");
            check(mimsem_column_solve_schur_eta(c, dt, th_w3, rho_h, eta, exner_h, F_w, F_rho, F_eta, F_exner, d_w, d_rho, d_eta, d_exner), "solve_schur_eta");   // :1855
            check(mimsem_column_newton_update(c, d_w, d_rho, d_eta, d_exner, velz, rho, rt, exner, velz_j, rho_j, rt_j, exner_j,
                                              velz_h, rho_h, rt_h, exner_h, nrm), "newton_update");
        }, [&](const double* mx) { history.push_back({mx[0], mx[1], mx[2], mx[3]}); return mx[0] < tol && mx[2] < tol; });                // :1922
    }
    const double* theta_l2_half() const { return theta_l2_h; }    // [nEl][nk*n2e]

private:
    double *F_eta, *d_eta, *th_w3, *eta;
};

class VertSolve2 : public VertNewton {
public:
    struct Norms { double exner, w, rho, rt; };
    std::vector<Norms> history;                       // |d x| / |x| (max over the columns) of the iterations of the last solve
    unsigned schur3_flags = 0;                        // passed to mimsem_column_solve_schur_3 (MIMSEM_SCHUR3_BOX: box/VertSolve.cpp, with rayleigh = 0)
    // The loop of the box twin (box/VertSolve.cpp:1264-1458; with schur3_flags = 3 and rayleigh = 0).  theta_up: theta_i / theta_j from
    // mimsem_column_diag_theta_wup(0.25 dt, ..) at the start and after every iteration (:1312, :1394; orders 1..4, needs |0.25 dt w| < 1).
    // vert_mom_vort(velz_j, uuz_j): AssembleVertMomVort (:1460-1499) of the iterate into uuz_j [nEl][(nk-1)*n2e]; with udwdx it makes the term
    // time-centred, F_w += 1/2 dt udwdx + 1/2 dt uuz_j (:1343-1346), uuz_j = udwdx in the first iteration (:1326) and recomputed at the end of
    // each (:1403); without udwdx it is not called (the reference's `if(udwdx)`).  Both off: the eul loop, bit for bit.
    bool theta_up = false;
    std::function<void(const double*, double*)> vert_mom_vort;

    VertSolve2(Mesh* m, double dt_) : VertNewton(m, dt_) {
        for (double** p : {&F_rt, &d_rt, &hs}) *p = mem.get(nl);
        for (double** p : {&uuz_j, &add_w}) *p = mem.get(ni);
    }

    // VertSolve::solve_schur_2: zv from VertSolve::initGZ.  udwdx (nullable, [nEl][(nk-1)*n2e]): :1134; hs_lat (nullable, [nEl][mp12]): the Held-Suarez
    // temperature forcing (:1151-1154).  theta_h / exner_h (what Euler::Strang reads afterwards) stay in the accessors.
    int solve_schur_2(double* velz, double* rho, double* rt, double* exner, const double* zv, int maxit = 20, double tol = 1.0e-12,
                      const double* udwdx = nullptr, const double* hs_lat = nullptr) {
        mimsem_ctx* c = mesh->ctx;
        history.clear();
        const bool centred = udwdx && vert_mom_vort;
        if (centred) mesh->copy(ni, udwdx, uuz_j);                                                                              // box :1326
        return newton(velz, rho, rt, exner, maxit, [&] {
            const double *a_rho = nullptr, *a_rt = nullptr, *a_hs = nullptr, *a_w = udwdx;
            if (centred) {                                                                                                      // box :1343-1346
                check(mimsem_vec_combine(c, 1, (long long)ni, 0.5, udwdx, 0, 0, nullptr, 0, 0.5, uuz_j, 0, add_w, 0), "vec_combine");
                a_w = add_w;
            }
            if (horiz_forcing) { horiz_forcing(rho, rho_j, theta_h, add_rho, add_rt); a_rho = add_rho; a_rt = add_rt; }            // :1124
            if (hs_lat) { check(mimsem_column_temp_forcing_hs(c, hs_lat, exner_h, theta_h, rho_h, hs), "temp_forcing_hs"); a_hs = hs; }
            check(mimsem_column_newton2_residual(c, dt, rayleigh, theta_h, exner_h, velz, velz_j, rho, rho_j, zv, rt, rt_j, exner_j,
                                                 a_w, a_rho, a_rt, a_hs, F_w, F_rho, F_rt, F_exner, k2i), "newton2_residual");
            check(mimsem_column_solve_schur_3(c, dt, schur3_flags, theta_h, velz_h, rho_h, rt_h, exner_h, F_w, F_rho, F_rt, F_exner,
                                              d_w, d_rho, d_rt, d_exner, nullptr), "solve_schur_3");                              // :1156
            check(mimsem_column_newton2_update(c, d_w, d_rho, d_rt, d_exner, velz, rho, rt, exner, velz_j, rho_j, rt_j, exner_j,
                                               velz_h, rho_h, rt_h, exner_h, nrm), "newton2_update");                             // :1159-1183
        }, [&](const double* mx) { history.push_back({mx[0], mx[1], mx[2], mx[3]}); return mx[0] < tol && mx[2] < tol && mx[3] < tol; },    // :1202
        theta_up, [&] { if (centred) vert_mom_vort(velz_j, uuz_j); });                                                            // box :1403
    }

private:
    double *F_rt, *d_rt, *hs, *uuz_j, *add_w;
};

}  // namespace mimsem_host
