// mimsem_euler.hpp -- Euler::Strang_ec (eul/Euler_2.cpp:1366-1557), the integrator of eul/UMJS14.cpp, and Euler::Strang (:1146-1364), the
// integrator of eul/HeldSuarez.cpp, driven from C++ over the C ABI: the
// counterpart of mimsem_amd/euler.py and of the three modules between it and HorizSolve / VertSolve, mirrored line for line where it can be:
//   VortDiag       mimsem_amd/vortdiag.py   Euler::HorizPotVort (:1051-1101), HorizSolve::diagVertVort (eul/HorizSolve.cpp:823-861) and
//                                           Euler::VertMassFlux (:1559-1572) for all nk - 1 interfaces at once
//   HorizMomentum  mimsem_amd/hmomentum.py  the explicit horizontal momentum update of stages 1 and 3 (:1431-1456, :1477-1492)
//   Energetics     mimsem_amd/energetics.py the twelve numbers of Euler::diagnostics (:600-744) and the line of output/energetics.dat
//   Euler          mimsem_amd/euler.py      Strang_ec and Strang, one skeleton, with the state it carries between steps
// Layouts are the reference's: velx [nk][n1]; rho, rt, exner [nk][n2] (horizontal, L2Vecs::vh); velz [nEl][(nk-1) n2e] (vertical, L2Vecs::vz).
// All pointers are device pointers.  One context, global numbering.  Header-only, C++17, no HIP toolchain needed.
// Not here: the box twin's step, init1 / init2, dumps and restart (the state
// comes from the Python driver's files), recording the stages as graphs, sharded meshes.
#pragma once
#include <cstdio>
#include <map>
#include <string>
#include <vector>
#include "mimsem_horizsolve.hpp"
#include "mimsem_vertsolve.hpp"

namespace mimsem_host {

// L2Vecs::HorizToVert / VertToHoriz for `rows` levels or interfaces
struct L2Layout {
    Mesh* mesh;
    void to_vert(const double* vh, int rows, double* vz) const { check(mimsem_l2_transpose(mesh->ctx, 0, rows, const_cast<double*>(vh), mesh->n2, vz), "mimsem_l2_transpose"); }
    void to_horiz(const double* vz, int rows, double* vh) const { check(mimsem_l2_transpose(mesh->ctx, 1, rows, vh, mesh->n2, const_cast<double*>(vz)), "mimsem_l2_transpose"); }
};
// the LINEAR_INV blocks of every column (VertOps::AssembleLinearInv): they depend on the geometry only
inline double* linear_inv_blocks(Mesh* mesh, DeviceArrays& mem) {
    const int nb = mimsem_colop_nblocks(mesh->ctx, MIMSEM_V_LINEAR_INV);
    if (nb <= 0) throw std::runtime_error("mimsem_colop_nblocks(LINEAR_INV)");
    double* p = mem.get((size_t)mesh->nEl_*nb*mesh->n2e*mesh->n2e);
    check(mimsem_colop_blocks(mesh->ctx, MIMSEM_V_LINEAR_INV, 0, nullptr, nullptr, p), "mimsem_colop_blocks");
    return p;
}

// (mimsem_shim.hpp already has mimsem_host::Euler, the reference-shaped holder of the two energetics kernels: the classes of the step live in
// mimsem_host::eul)
namespace eul {

// The two density-dependent interface solves are 1-form mass solves whose matrix changes with every call: the element-block preconditioner of
// all interfaces is rebuilt in one launch (mimsem_elem_block_pc_build_levels) and one batched PCG runs over the interfaces.  The first solve of
// each kind is adaptive and finds its count (iterations + MARGIN); later solves run that many iterations without a host read
// (mimsem_ksp_set_fixed_iterations) and log the true residual of every interface on the device; check_log() (VortDiag.check of the Python host) is
// the one read of the log, and after a miss both solves are adaptive.
class VortDiag {
public:
    static constexpr double SCALE = 1.0e8;
    static constexpr int MARGIN = 2;       // iterations added to the count the adaptive solve needed (its convergence test runs every second iteration)
    enum { UZ = 0, DWDX = 1, UNIT = 2 };      // UNIT: the unit-thickness mass solve of vert_mom_vort (the box twin)
    double rtol = 1.0e-14;
    int m_its[3] = {-1, -1, -1};               // fixed PCG length per solve: -1 = find it adaptively, 0 = adaptive from now on
    int its[3] = {0, 0, 0}, fixed_its[3] = {0, 0, 0};      // iterations of the last solve of each kind; the fixed length it was launched with (0: adaptive)
    int logged = 0, missed = 0;

    explicit VortDiag(Mesh* m) : mesh(m), l2{m}, nk(m->nk_), ni(m->nk_ - 1), n1(m->n1), n2(m->n2), uz_ksp(m, MIMSEM_KSP_CG), dwdx_ksp(m, MIMSEM_KSP_CG), unit_ksp(m, MIMSEM_KSP_CG) {
        if (nk < 2) throw std::runtime_error("VortDiag needs at least one interface (nk >= 2)");
        int n = 1; while (n*n < m->n2e) n++;
        nd = 2*n*(n + 1);
        Mu = mem.get((size_t)nk*n1); rhs = mem.get((size_t)ni*n1); rb = mem.get((size_t)ni*n2); t2 = mem.get((size_t)ni*n2);
        P = mem.get((size_t)ni*m->nEl_*nd*nd); log = mem.get(3*(size_t)ni); dw = mem.get((size_t)ni*n1);
        for (double** p : {&ca, &cb, &cc, &cd}) *p = mem.get((size_t)ni*n2);
        linv = linear_inv_blocks(m, mem);
        mesh->zero(3LL*ni, log);
        check(mimsem_ksp_set_operator_shell(uz_ksp, ni, n1, &VortDiag::apply_uz, this), "mimsem_ksp_set_operator_shell");
        check(mimsem_ksp_set_operator_shell(dwdx_ksp, ni, n1, &VortDiag::apply_dwdx, this), "mimsem_ksp_set_operator_shell");
        for (mimsem_ksp* k : {(mimsem_ksp*)uz_ksp, (mimsem_ksp*)dwdx_ksp}) check(mimsem_ksp_set_pc_shell(k, &VortDiag::apply_pc, this), "mimsem_ksp_set_pc_shell");
    }
    VortDiag(const VortDiag&) = delete; VortDiag& operator=(const VortDiag&) = delete;
    void force_its(int n) { m_its[UZ] = m_its[DWDX] = m_its[UNIT] = n; }          // (tests: a count that must miss its check; 0: adaptive)

    // uz [nk-1][n1] from velx [nk][n1], rho [nk][n2]:  uz_i = M1t_h(rho_i)^-1 (M1_{i+1} velx_{i+1} - M1_i velx_i)
    void horiz_pot_vort(const double* velx, const double* rho, double* uz) {
        mimsem_ctx* c = mesh->ctx;
        check(mimsem_op_apply(c, MIMSEM_OP_UMAT, 0, nk, SCALE, MIMSEM_FLAG_VERT, nullptr, 0, velx, n1, Mu, n1, 1.0), "UMAT");            // M1->assemble(k, SCALE, true)
        mesh->combine(n1, 1.0, Mu + n1, 0, nullptr, -1.0, Mu, rhs, ni);
        rho_bar(rho);
        check(mimsem_elem_block_pc_build_levels(c, MIMSEM_OP_UTMAT_H, 0, 1, ni, SCALE, 0, rb, n2, P), "mimsem_elem_block_pc_build_levels");
        solve(UZ, rhs, uz);                                                                                                                // M1t->assemble_h(i, SCALE, rho_h)
    }
    // dwdx [nk-1][n1] from velz_h [nk-1][n2] (horizontal layout), rho [nk][n2]:  dwdx_i = F(rho_i, level 0)^-1 E12 M2(level 0) velz_i
    void vert_vort(const double* velz_h, const double* rho, double* dwdx) {
        mimsem_ctx* c = mesh->ctx;
        check(mimsem_op_apply_levels(c, MIMSEM_OP_WMAT, 0, 0, ni, SCALE, MIMSEM_FLAG_VERT, nullptr, 0, velz_h, n2, t2, n2, 1.0), "WMAT");  // M2->assemble(0, SCALE, true)
        check(mimsem_incidence_apply(c, 2, ni, t2, n2, rhs, n1), "mimsem_incidence_apply");
        rho_bar(rho);
        check(mimsem_elem_block_pc_build_levels(c, MIMSEM_OP_UHMAT, 0, 0, ni, SCALE, 0, rb, n2, P), "mimsem_elem_block_pc_build_levels");
        solve(DWDX, rhs, dwdx);                                                                                                            // F->assemble(rho_h, 0, false, SCALE)
    }
    // Fz [nk-1][n2] (horizontal layout) = VertToHoriz diagnose_F_z (eul/VertSolve.cpp:237-260) of velz [nEl][(nk-1) n2e], rho [nEl][nk n2e]
    // in the VERTICAL layout (the step holds both layouts of each: HorizToVert is not repeated here)
    void vert_mass_flux(const double* velz1_v, const double* velz2_v, const double* rho1_v, const double* rho2_v, double* Fz) {
        const long long n = (long long)ni*n2;
        flux(velz1_v, rho1_v, ca); flux(velz2_v, rho1_v, cb);
        mesh->combine(n, 1.0/3.0, ca, 0, nullptr, 1.0/6.0, cb, cc);
        flux(velz1_v, rho2_v, ca); flux(velz2_v, rho2_v, cb);
        mesh->combine(n, 1.0/6.0, ca, 0, nullptr, 1.0/3.0, cb, cd);
        mesh->combine(n, 1.0, cd, 0, nullptr, 1.0, cc, cc);
        l2.to_horiz(cc, ni, Fz);
    }
    // VertSolve::AssembleVertMomVort of the box twin (box/VertSolve.cpp:1460-1499): uuz [nEl][(nk-1) n2e] in the VERTICAL layout from ul [nk][n1]
    // and velz_h [nk-1][n2] (horizontal layout), all nk - 1 interfaces per call:
    //     dwdx_i = M1o^-1 E12 M2o velz_i,   uuz_i = Rz(1/2 u_i + 1/2 u_{i+1}; SCALE) dwdx_i,   HorizToVert
    // M1o / M2o: level 0, SCALE, no thickness (box/Assembly.cpp:45,172); Rz = WtQdUdz_mat.  The mass solve is the third of this class's batched
    // PCGs (element blocks of the thickness-free M1, made once): adaptive the first time, then of fixed length with the TRUE residual of every
    // interface in the log that check_log() reads
    void vert_mom_vort(const double* ul, const double* velz_h, double* uuz) {
        mimsem_ctx* c = mesh->ctx;
        if (!unit_ready) {
            check(mimsem_ksp_set_operator(unit_ksp, MIMSEM_OP_UMAT, 0, ni, SCALE, 0, nullptr, 0), "mimsem_ksp_set_operator");
            check(mimsem_ksp_set_pc_bjacobi(unit_ksp), "mimsem_ksp_set_pc_bjacobi");
            unit_ready = true;
        }
        check(mimsem_op_apply_levels(c, MIMSEM_OP_WMAT, 0, 0, ni, SCALE, 0, nullptr, 0, velz_h, n2, t2, n2, 1.0), "WMAT");                  // M2->assemble(0, SCALE, false)
        check(mimsem_incidence_apply(c, 2, ni, t2, n2, rhs, n1), "mimsem_incidence_apply");
        solve(UNIT, rhs, dw);                                                                                                              // KSPSolve(ksp1, tmp1, dwdx)
        mesh->combine(n1, 0.5, ul, 0, nullptr, 0.5, ul + n1, Mu, ni);                                                                      // 0.5 ul[kk] + 0.5 ul[kk+1]
        check(mimsem_op_apply(c, MIMSEM_OP_WTQDUDZ, 0, ni, SCALE, 0, Mu, n1, dw, n1, t2, n2, 1.0), "WTQDUDZ");                              // Rz->assemble(_ul, SCALE)
        l2.to_vert(t2, ni, uuz);
    }
    // the ONE read of the fixed-length solves since the last call.  false: some interface missed 30 rtol (NaN: a miss) -- both solves have
    // switched to the adaptive PCG; the caller redoes the diagnoses
    bool check_log() {
        std::vector<double> v(3*(size_t)ni);
        mesh->to_host(v.data(), log, v.size());
        mesh->zero(3LL*ni, log);
        logged = 0;
        bool ok = true;
        for (double x : v) if (!(x <= (30.0*rtol)*(30.0*rtol))) ok = false;
        if (!ok) { missed++; force_its(0); }
        return ok;
    }

private:
    static int apply_uz(void* u, int nlev, const double* x, long long xs, double* y, long long ys) {
        VortDiag* s = (VortDiag*)u;
        return mimsem_op_apply(s->mesh->ctx, MIMSEM_OP_UTMAT_H, 0, nlev, SCALE, 0, s->rb, s->n2, x, xs, y, ys, 1.0);
    }
    static int apply_dwdx(void* u, int nlev, const double* x, long long xs, double* y, long long ys) {
        VortDiag* s = (VortDiag*)u;
        return mimsem_op_apply_levels(s->mesh->ctx, MIMSEM_OP_UHMAT, 0, 0, nlev, SCALE, 0, s->rb, s->n2, x, xs, y, ys, 1.0);
    }
    static int apply_pc(void* u, int nlev, const double* x, long long xs, double* y, long long ys) {
        VortDiag* s = (VortDiag*)u;
        return mimsem_elem_blocks_apply(s->mesh->ctx, 1, nlev, MIMSEM_FLAG_TRANSPOSE, s->P, (long long)s->mesh->nEl_*s->nd*s->nd, nullptr, 0, x, xs, y, ys, 1.0);
    }
    // rho_h of the interfaces: VecAXPY(rho_h, 0.5, rho[i]); VecAXPY(rho_h, 0.5, rho[i+1])
    void rho_bar(const double* rho) { mesh->combine(n2, 0.5, rho, 0, nullptr, 0.5, rho + n2, rb, ni); }
    // LINEAR_INV LINEAR_RT(rho, vert) velz
    void flux(const double* velz_v, const double* rho_v, double* out) {
        check(mimsem_colop_apply(mesh->ctx, MIMSEM_V_LINEAR_RT, MIMSEM_FLAG_VERT, 0, rho_v, nullptr, velz_v, cd), "LINEAR_RT");
        check(mimsem_colop_apply_blocks(mesh->ctx, MIMSEM_V_LINEAR_INV, 0, linv, cd, out), "LINEAR_INV");
    }
    void solve(int kind, const double* b, double* x) {
        mimsem_ksp* k = kind == UZ ? uz_ksp : (kind == DWDX ? dwdx_ksp : unit_ksp);
        const int m = m_its[kind];
        if (m > 0) {
            check(mimsem_ksp_set_fixed_iterations(k, m, log + (size_t)kind*ni), "mimsem_ksp_set_fixed_iterations");
            check(mimsem_ksp_solve(k, b, n1, x, n1), "mimsem_ksp_solve");
            logged++; its[kind] = m;
        } else {
            check(mimsem_ksp_set_fixed_iterations(k, 0, nullptr), "mimsem_ksp_set_fixed_iterations");
            check(mimsem_ksp_set_tolerances(k, rtol, 1.0e-50, 1000, 0, 2), "mimsem_ksp_set_tolerances");
            check(mimsem_ksp_solve(k, b, n1, x, n1), "mimsem_ksp_solve");
            double rn; int reason;
            check(mimsem_ksp_get_info(k, &its[kind], &rn, &reason), "mimsem_ksp_get_info");
            if (reason < 0) throw std::runtime_error("VortDiag: an interface solve did not converge");
            if (m < 0) m_its[kind] = its[kind] + MARGIN;
        }
        fixed_its[kind] = m > 0 ? m : 0;
    }
    Mesh* mesh; L2Layout l2; int nk, ni, n1, n2, nd = 0;
    DeviceArrays mem; KspHandle uz_ksp, dwdx_ksp, unit_ksp; bool unit_ready = false;
    double *Mu, *rhs, *rb, *t2, *P, *log, *ca, *cb, *cc, *cd, *linv, *dw;
};

// M1->assemble(kk); bu = M1 u_a - c dt Fu;  if(hs_forcing) M1 += M1ray(kk, c dt, exner[kk], exner[0]);  KSPSolve(ksp1, bu, velx[kk])  -- every
// level in one call of each kernel.  Without Held-Suarez friction the solve is HorizSolve's (FixedMassSolve, its log and its CG).  With it the
// matrix M1 + M1ray(c dt) is ONE operator (MIMSEM_OP_UMAT_FRIC) and the solve mimsem_fric_chebyshev_solve on HorizSolve's blocks: the
// spectral interval of P M1 from mimsem_ksp_ritz with its upper end widened by 1 + tau K_F (krylov.friction_interval), the check norms in
// HorizSolve's log so that its verify() covers the solve; once verify() has switched the fixed-length mode off, a CG on the same operator.
class HorizMomentum {
public:
    static constexpr double SCALE = HorizSolve::SCALE, K_F = 1.1574074074074073e-05;      // 1 / day: Held-Suarez k_f (include/mimsem_hip.h)
    int last_steps = 0;
    HorizMomentum(Mesh* m, HorizSolve* h, double dt_, bool hs) : mesh(m), horiz(h), dt(dt_), hs_forcing(hs), nk(m->nk_), n1(m->n1), n2(m->n2), cg(m, MIMSEM_KSP_CG) {
        b = mem.get((size_t)nk*n1);
        if (!hs) return;
        check(mimsem_ksp_set_operator_shell(cg, nk, n1, &HorizMomentum::apply_fric, this), "mimsem_ksp_set_operator_shell");
        check(mimsem_ksp_set_pc_shell(cg, &HorizMomentum::apply_pc, this), "mimsem_ksp_set_pc_shell");
        check(mimsem_ksp_set_tolerances(cg, horiz->rtol, 1.0e-50, 1000, 0, 2), "mimsem_ksp_set_tolerances");
    }
    HorizMomentum(const HorizMomentum&) = delete; HorizMomentum& operator=(const HorizMomentum&) = delete;
    // velx of  (M1 [+ M1ray(c dt, exner[k], exner[0])]) velx = M1 u_a - c dt Fu  on all levels; u_a, Fu, out [nk][n1], exner [nk][n2]
    void update(const double* u_a, const double* Fu, double c, const double* exner, double* out) {
        const double tau = c*dt;
        mesh->combine(n1, -tau, Fu, 0, nullptr, 0.0, nullptr, b, nk);
        check(mimsem_op_apply(mesh->ctx, MIMSEM_OP_UMAT, 0, nk, SCALE, MIMSEM_FLAG_VERT | MIMSEM_FLAG_ACCUM, nullptr, 0, u_a, n1, b, n1, 1.0), "UMAT");
        if (!hs_forcing) { horiz->solve_M1(b, out); last_steps = horiz->last_its; return; }
        if (!exner) throw std::runtime_error("HorizMomentum::update: Held-Suarez forcing needs the exner field");
        solve_fric(tau, exner, out);
    }
    // stage 1 (:1433-1445): c = 1, u_a = velx on the first step, else c = 2, u_a = u_prev (leapfrog); exner = exner_0
    void predictor(const double* velx, const double* u_prev, const double* Fu, const double* exner, bool first_step, double* out) {
        if (first_step) update(velx, Fu, 1.0, exner, out); else update(u_prev, Fu, 2.0, exner, out);
    }
    // stage 3 (:1477-1489): c = 1, u_a = velx_0; exner = the field the vertical solve left
    void corrector(const double* velx_0, const double* Fu, const double* exner_h, double* out) { update(velx_0, Fu, 1.0, exner_h, out); }
    bool verify() { return horiz->verify(); }

private:
    struct Coef { int steps = 0; std::vector<double> flat; };
    static int apply_fric(void* u, int nlev, const double* x, long long xs, double* y, long long ys) {
        HorizMomentum* s = (HorizMomentum*)u;
        return mimsem_op_apply_up(s->mesh->ctx, MIMSEM_OP_UMAT_FRIC, 0, nlev, SCALE, s->tau_now, 0, s->exner_now, s->n2, s->exner_now, 0, x, xs, y, ys, 1.0);
    }
    static int apply_pc(void* u, int nlev, const double* x, long long xs, double* y, long long ys) {
        HorizMomentum* s = (HorizMomentum*)u;
        const FixedMassSolve& m1 = s->horiz->mass_solver();
        if (!m1.blocks()) return mimsem_vec_combine(s->mesh->ctx, nlev, s->n1, 1.0, x, xs, 0, nullptr, 0, 0.0, nullptr, 0, y, ys);
        return mimsem_elem_blocks_apply(s->mesh->ctx, 1, nlev, 0, m1.blocks(), 0, m1.elem_scale(), s->mesh->nEl_, x, xs, y, ys, 1.0);
    }
    const Coef& coef_for(double tau) {
        auto it = coefs.find(tau);
        if (it != coefs.end()) return it->second;
        const Ritz ritz = [&](int steps, double* lo, double* hi, double* im) { check(mimsem_ksp_ritz(horiz->mass_ksp(), steps, lo, hi, im), "mimsem_ksp_ritz"); };
        const RitzInterval r = ritz_interval(ritz, 0.10, 0.05, 1.0);
        const double l1 = r.lmin(), l2 = r.lmax()*(1.0 + tau*K_F);                  // friction_interval: the lower end stays, the upper widens
        Coef c;
        c.steps = cheb::interval_steps(l1, l2, horiz->rtol);
        for (const auto& ab : cheb::ellipse(0.5*(l1 + l2), 0.25*(l2 - l1)*(l2 - l1), c.steps)) { c.flat.push_back(ab.first); c.flat.push_back(ab.second); }
        return coefs.emplace(tau, std::move(c)).first->second;
    }
    void solve_fric(double tau, const double* exner, double* out) {
        FixedMassSolve& m1 = horiz->mass_solver();
        if (horiz->fixed_length) {
            const Coef& c = coef_for(tau);
            const int rc = mimsem_fric_chebyshev_solve(mesh->ctx, MIMSEM_OP_UMAT, 0, nk, SCALE, MIMSEM_FLAG_VERT, nullptr, 0, m1.blocks(), m1.elem_scale(), mesh->nEl_,
                                                       b, n1, c.steps, c.flat.data(), out, n1, m1.ref(), n1, m1.upd(), n1, tau, exner, n2, exner);
            if (rc != MIMSEM_ERR_UNSUPPORTED) {
                check(rc, "mimsem_fric_chebyshev_solve");
                m1.log_last(horiz->check_log());
                last_steps = c.steps;
                return;
            }
        }
        tau_now = tau; exner_now = exner;
        check(mimsem_ksp_solve(cg, b, n1, out, n1), "mimsem_ksp_solve");
        double rn; int reason;
        check(mimsem_ksp_get_info(cg, &last_steps, &rn, &reason), "mimsem_ksp_get_info");
        if (reason < 0) throw std::runtime_error("HorizMomentum: the solve with M1 + M1ray did not converge");
    }
    Mesh* mesh; HorizSolve* horiz; double dt; bool hs_forcing; int nk, n1, n2;
    DeviceArrays mem; KspHandle cg; double* b = nullptr;
    std::map<double, Coef> coefs; double tau_now = 0.0; const double* exner_now = nullptr;
};

// Euler::diagnostics: keh kev pe ie k2p p2k k2i i2k k2i_z i2k_z mass entr, the line the reference appends to output/energetics.dat
class Energetics {
public:
    static constexpr int NFIELDS = 12;
    Energetics(Mesh* m, HorizSolve* h, VertNewton* v, const double* zv_) : mesh(m), l2{m}, horiz(h), vert(v), zv(zv_), nk(m->nk_), n1(m->n1), n2(m->n2) {
        if (nk < 2) throw std::runtime_error("Energetics needs at least one interface (nk >= 2)");
        rho_v = mem.get((size_t)nk*n2); rt_v = mem.get((size_t)nk*n2); th_v = mem.get((size_t)nk*n2); theta = mem.get((size_t)nk*n2);
        out8 = mem.get(8);
        linv = linear_inv_blocks(m, mem);
    }
    Energetics(const Energetics&) = delete; Energetics& operator=(const Energetics&) = delete;
    void use_vert(VertNewton* v) { vert = v; }       // the loop whose k2i_z the line takes: the one the last step ran
    // velx [nk][n1]; rho, rt, exner [nk][n2] horizontal; velz [nEl][(nk-1) n2e] vertical.  k2i is what the last momentum_rhs_ec that was given
    // Fk left in HorizSolve, k2i_z what the last vertical solve left; i2k = i2k_z = 0 as in the reference (:695)
    std::vector<double> diagnostics(const double* velx, const double* velz, const double* rho, const double* rt, const double* exner) {
        mimsem_ctx* c = mesh->ctx;
        l2.to_vert(rho, nk, rho_v); l2.to_vert(rt, nk, rt_v);                                          // :626-627, :701-702
        check(mimsem_column_diag_theta(c, 0, rho_v, rt_v, th_v), "mimsem_column_diag_theta");         // diagTheta_L2
        l2.to_horiz(th_v, nk, theta);                                                                  // :703-704
        check(mimsem_euler_energetics_horiz(c, nk, velx, n1, rho, n2, rt, n2, exner, n2, theta, n2, out8), "mimsem_euler_energetics_horiz");     // keh ie entr mass
        check(mimsem_euler_energetics_column(c, velz, rho_v, zv, linv, out8 + 4), "mimsem_euler_energetics_column");                            // kev k2p p2k pe
        double v[8];
        mesh->to_host(v, out8, 8);
        const double k2i = horiz ? horiz->k2i() : 0.0;
        return {v[0], v[4], v[7], v[1], v[5], v[6], k2i, 0.0, vert ? vert->k2i_z : 0.0, 0.0, v[3], v[2]};
    }
    // append one line in the reference's format (file.precision(16); value, tab, ..., endl :716-734)
    static void write_line(const char* path, const std::vector<double>& values) {
        if ((int)values.size() != NFIELDS) throw std::runtime_error("Energetics::write_line: 12 values expected");
        FILE* f = std::fopen(path, "a");
        if (!f) throw std::runtime_error(std::string("cannot write ") + path);
        for (double v : values) std::fprintf(f, "%.16g\t", v);
        std::fprintf(f, "\n");
        std::fclose(f);
    }
private:
    Mesh* mesh; L2Layout l2; HorizSolve* horiz; VertNewton* vert; const double* zv; int nk, n1, n2;
    DeviceArrays mem; double *rho_v, *rt_v, *th_v, *theta, *out8, *linv;
};

// One time step: explicit horizontal momentum predictor, implicit vertical Newton solve with the horizontal transport re-evaluated in every
// iteration, explicit horizontal corrector.
//   stage 1 (:1421-1457)  diagTheta_L2, the three diagnoses of VortDiag, HorizSolve::momentum_rhs_ec, HorizMomentum::predictor
//   stage 2 (:1461-1466)  VertSolveEta::solve_schur_eta with HorizSolve::advection_rhs_ec(velx_0, velx) as its horizontal forcing
//   stage 3 (:1470-1493)  the diagnoses on the new state, momentum_rhs_ec on the time-centred fields the solve left, HorizMomentum::corrector
//   :1501                 Energetics::diagnostics on the new state
// Carried between steps, as the reference carries it: first_step; u_prev / u_curr (:1415-1416: stage 1 of a later step is the leapfrog
// M1 velx = M1 u_prev - 2 dt Fu); uz / uz_prev (:1425 on the first step uz_prev is stage 1's uz, :1407-1409 later the uz stage 3 of the step
// before left).  The fixed-length solves are checked within the step -- VortDiag::check_log() once at its end, HorizSolve::verify() after
// stage 1, at the head of every Newton iteration and at the end --; on a miss those solvers have switched to their adaptive forms and the step
// is run once more from its inputs; the carried state is committed only after the checks passed, and a second miss throws.
// As mimsem_amd/euler.py, each velocity of stage 3 is paired with itself (the reference hands momentum_rhs_ec the local copies in the other
// order than the global vectors at :1475).
// fused_hu / fused_phi / fused_forcing: HorizSolve's switches during Strang (Euler.FUSED_HU / FUSED_PHI of the Python host); Strang_ec runs with
// the switches the HorizSolve has, all off unless the caller sets them
struct EulerOptions { bool hs_forcing = false; const double* hs_lat = nullptr; bool do_visc = true; int newton_maxit = 20; double newton_tol = 1.0e-12;
                      bool fused_hu = false, fused_phi = false, fused_forcing = false; };
class Euler {
public:
    using Options = EulerOptions;
    HorizSolve horiz; VertSolveEta vert; VertSolve2 vert2; VortDiag vort; HorizMomentum hmom; Energetics energetics;
    bool first_step = true;
    int steps = 0, redone = 0;           // steps taken; steps that missed a check and were run again
    std::vector<VertSolveEta::Norms> newton_history;      // of the last step's vertical solve (Strang: the fourth norm is rt's)
    int newton_its = 0;
    std::vector<double> values;          // the twelve numbers of the last step

    // fg: the Coriolis 0-form per level [nk][n0] (HorizSolve::coriolis); zv: the geopotential of VertSolve::initGZ [nEl][nk n2e]; hs_lat
    // [nEl][mp12] with hs_forcing.  All device pointers that stay valid for the life of the object
    Euler(Mesh* m, double dt_, const double* fg, const double* zv_, const Options& o = Options())
        : horiz(m, fg, 0, o.do_visc), vert(m, dt_), vert2(m, dt_), vort(m), hmom(m, &horiz, dt_, o.hs_forcing), energetics(m, &horiz, &vert, zv_),
          dt(dt_), mesh(m), l2{m}, opt(o), zv(zv_), nk(m->nk_), ni(m->nk_ - 1), n1(m->n1), n2(m->n2) {
        if (o.hs_forcing && !o.hs_lat) throw std::runtime_error("Euler: Held-Suarez forcing needs hs_lat");
        alloc();
    }
    Euler(const Euler&) = delete; Euler& operator=(const Euler&) = delete;
    virtual ~Euler() = default;

    // one step, in place: velx [nk][n1]; rho, rt, exner [nk][n2]; velz [nEl][(nk-1) n2e]
    void Strang_ec(double* velx, double* velz, double* rho, double* rt, double* exner, bool diagnostics = true) {
        checked_step("Strang_ec", true, velx, velz, rho, rt, exner, diagnostics);
    }
    // Euler::Strang (:1146-1364): the skeleton of Strang_ec -- the same carried state, check points, redo on a miss and energetics line -- with
    // theta on the nk + 1 interfaces:
    //   stage 1 (:1199-1251)  theta_0 = diagTheta (= VertSolve::diagTheta2), HorizSolve::momentum_rhs in place of momentum_rhs_ec
    //   stage 2 (:1253-1260)  VertSolve2::solve_schur_2 with HorizSolve::advection_rhs(velx_0, velx, rho_0, rho_j, theta_h) as its forcing
    //   stage 3 (:1262-1300)  momentum_rhs on the theta_h, exner_h the solve left, with Fk of the last advection_rhs; the corrector takes the new exner
    // As mimsem_amd/euler.py, :1180 (theta_h filled on the first step, overwritten before any read) and the order of the local copies at :1269 are
    // not mirrored.  HorizSolve's switches are the options' for the length of the call
    void Strang(double* velx, double* velz, double* rho, double* rt, double* exner, bool diagnostics = true) {
        const bool hu = horiz.fused_hu, phi = horiz.fused_phi, forcing = horiz.fused_forcing;
        horiz.fused_hu = opt.fused_hu; horiz.fused_phi = opt.fused_phi; horiz.fused_forcing = opt.fused_forcing;
        try { checked_step("Strang", false, velx, velz, rho, rt, exner, diagnostics); }
        catch (...) { horiz.fused_hu = hu; horiz.fused_phi = phi; horiz.fused_forcing = forcing; throw; }
        horiz.fused_hu = hu; horiz.fused_phi = phi; horiz.fused_forcing = forcing;
    }
    const double* u_prev() const { return have_u_prev ? u_prev_ : nullptr; }            // null before the second step, as the reference's
    const double* u_curr() const { return first_step ? nullptr : u_curr_; }
    const double* uz() const { return first_step ? nullptr : uz_; }
    const double* uz_prev() const { return first_step ? nullptr : uz_prev_; }

protected:
    // the box twin (box::Euler below): HorizSolve in box mode, VertSolve2 as box/VertSolve.cpp has it (theta_up, schur3_flags = 3, no Rayleigh layer)
    Euler(Mesh* m, double dt_, const HorizSolve::Box& bx, const double* zv_, const Options& o)
        : horiz(box_order(m), bx, o.do_visc), vert(m, dt_), vert2(m, dt_), vort(m), hmom(m, &horiz, dt_, false), energetics(m, &horiz, &vert2, zv_),
          box(true), dt(dt_), mesh(m), l2{m}, opt(o), zv(zv_), nk(m->nk_), ni(m->nk_ - 1), n1(m->n1), n2(m->n2) {
        if (o.hs_forcing) throw std::runtime_error("box::Euler: no Held-Suarez forcing");
        alloc();
        vert2.theta_up = true; vert2.schur3_flags = 3; vert2.rayleigh = 0.0;
        uuz = mem.get((size_t)ni*n2); velz_hj = mem.get((size_t)ni*n2);
    }
    // (the order is read before anything is built: the column entries of the other members refuse order 5 with messages of their own)
    static Mesh* box_order(Mesh* m) { if (m->n2e > 16) throw std::runtime_error("box::Euler: orders 1..4 (the upwinded theta diagnosis)"); return m; }
    bool box = false; double dt = 0.0;
    double *uuz = nullptr, *velz_hj = nullptr;
    const double* theta_0_interfaces() const { return theta_0i; }      // stage 1's theta_0 [nk+1][n2] of the last step (Strang)
    Mesh* mesh_() const { return mesh; }

private:
    void alloc() {
        const size_t s1 = (size_t)nk*n1, s2 = (size_t)nk*n2, i1 = (size_t)ni*n1, i2 = (size_t)ni*n2;
        for (double** p : {&u_prev_, &u_curr_, &k_u_curr, &Fu, &velx_p, &velx_n, &Fk, &Gk}) *p = mem.get(s1);
        for (double** p : {&uz_, &uz_prev_, &uz1, &uz3, &dwdx1, &dwdx2}) *p = mem.get(i1);
        for (double** p : {&rho_v, &rt_v, &exner_v, &th_v, &theta_0, &rho_nv, &rt_nv, &exner_nv, &rho_n, &rt_n, &exner_n, &hA, &hB, &dF, &dG, &theta_h, &exner_hh}) *p = mem.get(s2);
        for (double** p : {&velz_h0, &velz_hn, &velz_n, &Fz}) *p = mem.get(i2);
        for (double** p : {&th_vi, &theta_0i, &theta_hi, &hBi}) *p = mem.get(s2 + (size_t)n2);        // theta on the nk + 1 interfaces (Strang)
    }
    void checked_step(const char* name, bool ec, double* velx, double* velz, double* rho, double* rt, double* exner, bool diagnostics) {
        const double *k_u_prev = nullptr, *k_uz_prev = nullptr;
        bool ok = false;
        for (int attempt = 0; attempt < 2 && !ok; attempt++) {
            const bool ok_m1 = step(ec, velx, velz, rho, rt, exner, &k_u_prev, &k_uz_prev);
            const bool ok_vort = vort.check_log();                                      // (the log is read and cleared)
            ok = ok_m1 && ok_vort;
            if (!ok) redone++;
        }
        if (!ok) throw std::runtime_error(std::string("Euler::") + name + ": a solve missed its check again after the switch to the adaptive solvers");
        // commit: (u_prev, u_curr, uz, uz_prev) of the step; k_u_prev is the old u_curr, k_uz_prev stage 1's uz or the old uz
        if (k_u_prev) mesh->copy((long long)nk*n1, k_u_prev, u_prev_);
        have_u_prev = k_u_prev != nullptr;
        mesh->copy((long long)nk*n1, k_u_curr, u_curr_);
        mesh->copy((long long)ni*n1, k_uz_prev, uz_prev_);
        mesh->copy((long long)ni*n1, uz3, uz_);
        first_step = false;
        steps++;
        mesh->copy((long long)nk*n1, velx_n, velx); mesh->copy((long long)ni*n2, velz_n, velz);
        mesh->copy((long long)nk*n2, rho_n, rho); mesh->copy((long long)nk*n2, rt_n, rt); mesh->copy((long long)nk*n2, exner_n, exner);
        energetics.use_vert(ec ? static_cast<VertNewton*>(&vert) : static_cast<VertNewton*>(&vert2));
        if (diagnostics) values = energetics.diagnostics(velx, velz, rho, rt, exner);     // :1501
    }
    // one evaluation of the step from the carried state; changes nothing of first_step / u_* / uz*.  The new fields go to velx_n, velz_n,
    // rho_n, rt_n, exner_n, the carried vectors of the step to k_u_curr, uz3 and the two pointers.  Returns whether every verify() passed.
    // ec: Strang_ec (theta in the levels, the _ec right-hand sides, solve_schur_eta); else Strang (theta on the interfaces, momentum_rhs /
    // advection_rhs, solve_schur_2) -- the comments name the lines of Strang_ec, Strang's are :1170-1300 in the same order
    bool step(bool ec, const double* velx, const double* velz, const double* rho, const double* rt, const double* exner, const double** k_u_prev, const double** k_uz_prev) {
        mimsem_ctx* c = mesh->ctx;
        const bool first = first_step;
        // 0. the initial fields in both layouts (:1390-1395); the carried vectors of this step (:1399-1417)
        l2.to_horiz(velz, ni, velz_h0);
        l2.to_vert(rho, nk, rho_v); l2.to_vert(rt, nk, rt_v); l2.to_vert(exner, nk, exner_v);
        const double* uz_prev = first ? nullptr : uz_;
        const double* u_prev = first ? nullptr : u_curr_;
        mesh->copy((long long)nk*n1, velx, k_u_curr);
        // 1. explicit horizontal momentum solve, the predictor (:1421-1457)
        if (ec) { check(mimsem_column_diag_theta(c, 0, rho_v, rt_v, th_v), "mimsem_column_diag_theta"); l2.to_horiz(th_v, nk, theta_0); }
        else {
            if (box) check(mimsem_column_diag_theta_wup(c, 0.25*dt, rho_v, rt_v, velz, th_vi, nullptr, 1.0, 0.0), "mimsem_column_diag_theta_wup");      // box Euler::diagTheta :543-565
            else check(mimsem_column_diag_theta(c, 1, rho_v, rt_v, th_vi), "mimsem_column_diag_theta");                                       // diagTheta2 :1201
            l2.to_horiz(th_vi, nk + 1, theta_0i);
        }
        vort.horiz_pot_vort(velx, rho, uz1);
        vort.vert_vort(velz_h0, rho, dwdx1);
        if (first) uz_prev = uz1;                                                       // :1425
        vort.vert_mass_flux(velz, velz, rho_v, rho_v, Fz);
        if (ec) horiz.momentum_rhs_ec(theta_0, uz1, uz1, velz_h0, velz_h0, exner, velx, velx, rho, rho, Fu, nullptr, Fz, dwdx1, dwdx1);
        else horiz.momentum_rhs(theta_0i, uz1, uz1, velz_h0, velz_h0, exner, velx, velx, rho, rho, Fu, nullptr, Fz, dwdx1, dwdx1);
        hmom.predictor(velx, u_prev, Fu, exner, first, velx_p);
        bool ok = horiz.verify();
        // 2. implicit vertical solve (:1461-1466): advection_rhs_ec(velx_0, velx, rho_i, rho_j, theta_l2_h) at the head of every Newton iteration
        // (eul/VertSolve.cpp:1798-1799); rho_i in the horizontal layout is the rho this step was given
        auto forcing = [&](const double*, const double* rho_j, const double* theta_half, double* add_rho, double* add_rt) {
            if (!horiz.verify()) ok = false;                                            // (the solves of the iteration before)
            l2.to_horiz(rho_j, nk, hA);
            if (ec) { l2.to_horiz(theta_half, nk, hB); horiz.advection_rhs_ec(velx, velx_p, rho, hA, hB, dF, dG, Fk, Gk); }
            else { l2.to_horiz(theta_half, nk + 1, hBi); horiz.advection_rhs(velx, velx_p, rho, hA, hBi, dF, dG, Fk, Gk); }
            l2.to_vert(dF, nk, add_rho); l2.to_vert(dG, nk, add_rt);
        };
        mesh->copy((long long)ni*n2, velz, velz_n); mesh->copy((long long)nk*n2, rho_v, rho_nv);
        mesh->copy((long long)nk*n2, rt_v, rt_nv); mesh->copy((long long)nk*n2, exner_v, exner_nv);
        const double* lat = opt.hs_forcing ? opt.hs_lat : nullptr;
        if (ec) {
            vert.horiz_forcing = forcing;
            newton_its = vert.solve_schur_eta(velz_n, rho_nv, rt_nv, exner_nv, zv, opt.newton_maxit, opt.newton_tol, nullptr, lat);
            vert.horiz_forcing = nullptr;
            newton_history = vert.history;
        } else {
            const double* udwdx = nullptr;
            if (box) {
                // box :1337: AssembleVertMomVort(velz_0) runs before ul is filled on the first step and PETSc vectors start zeroed: uuz = 0 on the
                // first step, vert_mom_vort(velx, velz_0) on later ones; in the loop it is bound to the predictor velocity (box/VertSolve.cpp:1403)
                if (first) mesh->zero((long long)ni*n2, uuz); else vort.vert_mom_vort(velx, velz_h0, uuz);
                udwdx = uuz;
                vert2.vert_mom_vort = [&](const double* velz_j, double* uuz_j) { l2.to_horiz(velz_j, ni, velz_hj); vort.vert_mom_vort(velx_p, velz_hj, uuz_j); };
            }
            vert2.horiz_forcing = forcing;
            newton_its = vert2.solve_schur_2(velz_n, rho_nv, rt_nv, exner_nv, zv, opt.newton_maxit, opt.newton_tol, udwdx, lat);
            vert2.horiz_forcing = nullptr; vert2.vert_mom_vort = nullptr;
            newton_history.clear();
            for (const auto& h : vert2.history) newton_history.push_back({h.exner, h.w, h.rho, h.rt});
        }
        l2.to_horiz(rho_nv, nk, rho_n); l2.to_horiz(rt_nv, nk, rt_n); l2.to_horiz(exner_nv, nk, exner_n);
        l2.to_horiz(velz_n, ni, velz_hn);
        // 3. explicit horizontal solve, the corrector (:1470-1493): the time-centred theta_l2_h, exner_h the vertical solve left; the friction
        // takes the NEW exner (:1482); Fk of the last advection_rhs_ec makes k2i the reference's (:704-708)
        vort.horiz_pot_vort(velx_p, rho_n, uz3);
        vort.vert_vort(velz_hn, rho_n, dwdx2);
        vort.vert_mass_flux(velz, velz_n, rho_v, rho_nv, Fz);
        if (ec) {
            l2.to_horiz(vert.theta_l2_half(), nk, theta_h); l2.to_horiz(vert.exner_half(), nk, exner_hh);
            horiz.momentum_rhs_ec(theta_h, uz3, uz_prev, velz_hn, velz_h0, exner_hh, velx, velx_p, rho, rho_n, Fu, nullptr, Fz, dwdx1, dwdx2, Fk);
        } else {
            l2.to_horiz(vert2.theta_half(), nk + 1, theta_hi); l2.to_horiz(vert2.exner_half(), nk, exner_hh);
            horiz.momentum_rhs(theta_hi, uz3, uz_prev, velz_hn, velz_h0, exner_hh, velx, velx_p, rho, rho_n, Fu, nullptr, Fz, dwdx1, dwdx2, Fk);
        }
        hmom.corrector(velx, Fu, exner_n, velx_n);
        if (!horiz.verify()) ok = false;
        *k_u_prev = u_prev; *k_uz_prev = uz_prev;
        return ok;
    }
    Mesh* mesh; L2Layout l2; Options opt; const double* zv; int nk, ni, n1, n2; bool have_u_prev = false;
    DeviceArrays mem;
    double *u_prev_, *u_curr_, *k_u_curr, *Fu, *velx_p, *velx_n, *Fk, *Gk;
    double *uz_, *uz_prev_, *uz1, *uz3, *dwdx1, *dwdx2;
    double *rho_v, *rt_v, *exner_v, *th_v, *theta_0, *rho_nv, *rt_nv, *exner_nv, *rho_n, *rt_n, *exner_n, *hA, *hB, *dF, *dG, *theta_h, *exner_hh;
    double *velz_h0, *velz_hn, *velz_n, *Fz;
    double *th_vi, *theta_0i, *theta_hi, *hBi;
};

}  // namespace eul

// Euler::Strang of the doubly periodic box (box/Euler_2.cpp:1306-1477): eul::Euler::Strang's skeleton -- the carried state, the check points, the redo
// on a miss, the commit after the checks -- on the box-mode HorizSolve, with what the box twin does differently:
//   stage 1 (:1359-1383)  theta_0 = Euler::diagTheta (:543-565) = diag_theta_wup(0.25 dt, rho, rt, velz); plain M1 predictor and corrector, no friction
//   uuz (:1337)           0 on the first step, vert_mom_vort(velx, velz_0) afterwards
//   stage 2 (:1392)       solve_schur_2(schur3_flags = 3, theta_up, udwdx = uuz, vert_mom_vort bound to the predictor velocity, advection_rhs as forcing)
//   diagnostics (:887-1026)  eleven numbers are Energetics' own; slot 11 is the box entropy CP sum_k lz_k sum_q Q_q log((W theta_k)_q) of STAGE 1's theta_0
//                            (:979-997, :1421), lz half a layer at both ends: mimsem_euler_log_entropy
// Orders 1..4, uniform layers only (both refused by the constructors).  The element-local forcing is fused by default, as BoxEuler.FUSED_FORCING.
namespace box {

inline eul::EulerOptions default_options() { eul::EulerOptions o; o.fused_forcing = true; o.fused_phi = true; return o; }

class Euler : public eul::Euler {
public:
    static constexpr double CP = 1004.5;                      // box/Euler_2.cpp:27
    Euler(Mesh* m, double dt_, const HorizSolve::Box& bx, const double* zv_, const Options& o = default_options()) : eul::Euler(m, dt_, bx, zv_, o) {
        std::vector<double> lz((size_t)m->nk_ + 1, bx.thick[0]);
        lz.front() *= 0.5; lz.back() *= 0.5;                  // :988
        lz_dev = mem_.get(lz.size()); ent = mem_.get(1);
        check(mimsem_memcpy_h2d(m->ctx, lz_dev, lz.data(), (long long)lz.size()*8), "h2d");
    }
    void Strang(double* velx, double* velz, double* rho, double* rt, double* exner, bool diagnostics = true) {
        eul::Euler::Strang(velx, velz, rho, rt, exner, diagnostics);
        if (!diagnostics) return;
        Mesh* m = mesh_();
        check(mimsem_euler_log_entropy(m->ctx, m->nk_ + 1, theta_0_interfaces(), m->n2, lz_dev, CP, ent), "mimsem_euler_log_entropy");
        m->to_host(&values[11], ent, 1);
    }
    void Strang_ec(double*, double*, double*, double*, double*, bool = true) { throw std::runtime_error("box::Euler: the box twin has no Strang_ec"); }
private:
    DeviceArrays mem_; double *lz_dev = nullptr, *ent = nullptr;
};

}  // namespace box
}  // namespace mimsem_host
