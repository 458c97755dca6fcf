// column_newton2.inc -- included by column_kernels.hip after column_newton.inc (same translation unit: ColTask, NewtonGeo, newton_grid).
//
// The residual assembly and the update of the OTHER vertical Newton loop, VertSolve::solve_schur_2 (eul/VertSolve.cpp:1059-1246), the
// caller of solve_schur_column_3: assemble_residual (:386-430) with diagnose_F_z / diagnose_Phi_z (:237-286), the right-hand sides of
// :1134-1154 and the update, half-time states and norms of :1159-1183, for ALL columns in three launches:
//   k_newton2_ifc   one task per (column, interface): F_z, G_z, the interface part of F_w, k2i
//   k_newton2_lev   one task per (column, level):     F_w completed, F_rho, F_rt, F_exner
//   k_newton2_upd   one thread per level entry:       x_j += d_x, x_h = 0.5 x_i + 0.5 x_j, the squares MaxNorm sums
// Against k_newton_ifc / k_newton_lev: theta lives on the nk+1 INTERFACES (AssembleLinearWithTheta, VertOps.cpp:669-730, not
// AssembleLinearWithRT), the pressure gradient and V10 G_z enter with dt (not dt/2), there are no entropy-conservation terms, no
// f_theta_corr and no entropy variables, and the horizontal forcing is added BEFORE the VB product (:1145-1149), the Held-Suarez term
// after it (:1151-1154).  Same 16-lane tasks on the LDS-free row algebra; the only block formed is VA^-1 (in registers, as k_newton_ifc).

namespace {

// ---- launch 1: interfaces ------------------------------------------------------------------------------------------------------
struct Newton2IfcArgs {
    NewtonGeo g;
    double dt, rayleigh;
    const double *theta, *Pi, *velz1, *velz2, *rho1, *rho2, *add_w;     // theta [nEl][nk+1][n2]; add_w optional
    double *F, *G, *u, *fwA, *k2;                                        // [nEl][nk-1][n2] each
};
template <int N>
__global__ __launch_bounds__(64) void k_newton2_ifc(Newton2IfcArgs a) {
    using T = ColTask<N>; using R = dpp::Rows<N>;
    constexpr int N2 = T::N2, NP = T::NP;
    const int lane = threadIdx.x, r = lane%16;
    const int nk = a.g.nk, nm = nk - 1;
    const long long task0 = (long long)blockIdx.x*4 + lane/16, ntask = (long long)a.g.nEl*nm;
    const bool live = task0 < ntask;
    const long long task = live ? task0 : ntask - 1;
    const int e = (int)(task/nm), i = (int)(task%nm);
    T t; t.init(a.g, e, r);
    const bool act = live && r < N2;
    const double hdt = 0.5*a.dt;
    const size_t v0 = ((size_t)e*nk + i)*N2 + t.rr, v1 = v0 + N2, io = ((size_t)e*nm + i)*N2 + t.rr;
    const size_t to = ((size_t)e*(nk + 1) + i + 1)*N2 + t.rr;           // interface i of the nk-1 inner ones is slot i+1 of the nk+1

    double tI0[NP], th0[NP], tI1[NP], th1[NP];
    t.geo(tI0, th0, i); t.geo(tI1, th1, i + 1);
    double thq[NP], piq0[NP], piq1[NP], c[NP], x[NP];
    t.interp(thq, a.theta[to]);
    t.interp(piq0, a.Pi[v0]); t.interp(piq1, a.Pi[v1]);
    // A^-1                                               AssembleLinearInv, VertOps.cpp:422-430
    double Ai[N2];
#pragma unroll
    for (int p = 0; p < NP; p++) c[p] = t.q0[p]*(0.5*(th0[p] + th1[p]));
    t.inv_block(Ai, c);
    double v1q[NP], v2q[NP];
    t.interp(v1q, a.velz1[io]); t.interp(v2q, a.velz2[io]);
    // F_z = A^-1 (1/3 VA(rho1) w1 + 1/6 VA(rho1) w2 + 1/6 VA(rho2) w1 + 1/3 VA(rho2) w2)      diagnose_F_z, VertSolve.cpp:237-260
    {
        double r1a[NP], r1b[NP], r2a[NP], r2b[NP];
        t.interp(r1a, a.rho1[v0]); t.interp(r1b, a.rho1[v1]); t.interp(r2a, a.rho2[v0]); t.interp(r2b, a.rho2[v1]);
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const double c1 = t.q0[p]*(0.5*r1a[p]/t.det[p]) + t.q0[p]*(0.5*r1b[p]/t.det[p]);       // AssembleLinearWithRT(rho, internal) :621-662
            const double c2 = t.q0[p]*(0.5*r2a[p]/t.det[p]) + t.q0[p]*(0.5*r2b[p]/t.det[p]);
            x[p] = c1*((1.0/3.0)*v1q[p] + (1.0/6.0)*v2q[p]) + c2*((1.0/6.0)*v1q[p] + (1.0/3.0)*v2q[p]);
        }
    }
    const double F = R::matvec(Ai, t.proj(x));
    // interface part of Phi_z: u = 1/6 (C(w1) w1 + C(w1) w2 + C(w2) w2), C(f) = W^T diag(w S/det 0.5 f_q/det) W    diagnose_Phi_z :262-286
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const double cw1 = t.q0[p]*(0.5*v1q[p]/t.det[p]), cw2 = t.q0[p]*(0.5*v2q[p]/t.det[p]);       // AssembleConLinWithW :551-600
        x[p] = (1.0/6.0)*(cw1*v1q[p]) + (1.0/6.0)*(cw1*v2q[p]) + (1.0/6.0)*(cw2*v2q[p]);
    }
    const double u = t.proj(x);
    // F_w, the terms that live on this interface alone         assemble_residual :396-412
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = (t.q0[p]*(0.5*th0[p]) + t.q0[p]*(0.5*th1[p]))*(v2q[p] - v1q[p]);     // VA w2 - VA w1 (AssembleLinear :242-267)
    double fw = t.proj(x);
    // pressure gradient tA2 = A^-1 V01 (VB Pi); tA1 = VA(theta) tA2, theta of THIS interface (AssembleLinearWithTheta :685-725)
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = (t.q0[p]*tI1[p])*piq1[p];                                            // AssembleConst :201-209
    double bp = t.proj(x);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = (t.q0[p]*tI0[p])*piq0[p];
    bp -= t.proj(x);
    const double gPi = R::matvec(Ai, bp);
    double cT[NP], gq[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) cT[p] = t.q0[p]*(0.5*th0[p])*(thq[p]/t.det[p]) + t.q0[p]*(0.5*th1[p])*(thq[p]/t.det[p]);
    t.interp(gq, gPi);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = cT[p]*gq[p];
    const double tA1 = t.proj(x);
    fw += a.dt*tA1;                                                                                           // :412
    // G_z = A^-1 VA(theta) F                                                                                  :419-420
    t.interp(gq, F);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = cT[p]*gq[p];
    const double G = R::matvec(Ai, t.proj(x));
    // Rayleigh friction on the three interfaces below the lid (AssembleRayleigh :826-888)                     :424-428
    {
        const int s = nk - 2 - i;
        const double wgt = (s == 0) ? 0.5 : (s == 1 ? 0.25 : (s == 2 ? 0.125 : 0.0));
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = (t.q0[p]*(wgt*(th1[p] + th0[p])))*(v2q[p] + v1q[p]);
        fw += hdt*a.rayleigh*t.proj(x);
    }
    if (a.add_w) fw += a.dt*a.add_w[io];                                                                      // :1134
    if (act) { a.F[io] = F; a.G[io] = G; a.u[io] = u; a.fwA[io] = fw; a.k2[io] = F*tA1; }
}

// ---- launch 2: levels ----------------------------------------------------------------------------------------------------------
struct Newton2LevArgs {
    NewtonGeo g;
    double dt;
    const double *zv, *rho_i, *rho_j, *rt_i, *rt_j, *exner_j, *add_rho_pre, *add_rt_pre, *add_rt_post;
    const double *F, *G, *u, *fwA;
    double *F_w, *F_rho, *F_rt, *F_exner;
};
template <int N>
__global__ __launch_bounds__(64) void k_newton2_lev(Newton2LevArgs a) {
    using T = ColTask<N>;
    constexpr int N2 = T::N2, NP = T::NP;
    const int lane = threadIdx.x, r = lane%16;
    const int nk = a.g.nk, nm = nk - 1;
    const long long task0 = (long long)blockIdx.x*4 + lane/16, ntask = (long long)a.g.nEl*nk;
    const bool live = task0 < ntask;
    const long long task = live ? task0 : ntask - 1;
    const int e = (int)(task/nk), k = (int)(task%nk);
    T t; t.init(a.g, e, r);
    const bool act = live && r < N2;
    const double dt = a.dt;
    const size_t vo = ((size_t)e*nk + k)*N2 + t.rr;
    const bool lo = k > 0, hi = k < nk - 1;
    const size_t im = ((size_t)e*nm + (lo ? k - 1 : 0))*N2 + t.rr, ik = ((size_t)e*nm + (hi ? k : 0))*N2 + t.rr;
    // F_w of interface k: + dt V01 Phi, Phi_m = u_{m-1} + u_m + zv_m                                  :402-403
    if (hi) {
        const double up = (k + 1 < nm) ? a.u[ik + N2] : 0.0, um = lo ? a.u[im] : 0.0;
        double phi_hi = a.u[ik] + up; phi_hi += a.zv[vo + N2];
        double phi_lo = um + a.u[ik]; phi_lo += a.zv[vo];
        if (act) a.F_w[ik] = a.fwA[ik] + dt*(phi_hi - phi_lo);
    }
    const double Fm = lo ? a.F[im] : 0.0, Fk = hi ? a.F[ik] : 0.0, Gm = lo ? a.G[im] : 0.0, Gk = hi ? a.G[ik] : 0.0;
    const double V10F = Fk - Fm, V10G = Gk - Gm;                          // V10 = [-I | +I], VertOps.cpp:134-163
    double tI[NP], th[NP], cB[NP], x[NP], q[NP];
    t.geo(tI, th, k);
#pragma unroll
    for (int p = 0; p < NP; p++) cB[p] = t.q0[p]*tI[p];                    // AssembleConst :201-209
    // F_rho = VB (rho_j + dt V10 F - rho_i + dt dFx),  F_rt = VB (rt_j + dt V10 G - rt_i + dt dGx) + dt HS      (:1137-1154)
    double dF = (a.rho_j[vo] + dt*V10F) - a.rho_i[vo];
    if (a.add_rho_pre) dF += dt*a.add_rho_pre[vo];
    t.interp(q, dF);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = cB[p]*q[p];
    const double F_rho = t.proj(x);
    double dG = (a.rt_j[vo] + dt*V10G) - a.rt_i[vo];
    if (a.add_rt_pre) dG += dt*a.add_rt_pre[vo];
    t.interp(q, dG);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = cB[p]*q[p];
    double F_rt = t.proj(x);
    if (a.add_rt_post) F_rt += dt*a.add_rt_post[vo];
    // EOS residual                                                                                     Assemble_EOS_Residual :987-1047
    double ek[NP];
    t.interp(q, a.rt_j[vo]); t.interp(ek, a.exner_j[vo]);
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const double rk = q[p]*(1.0/(t.det[p]*th[p])), ekk = ek[p]*(1.0/(t.det[p]*th[p]));
        double v = log(ekk) - (RD/CV)*log(rk) - log(CP) - (RD/CV)*log(RD/P0);
        x[p] = v*(0.5*t.Q[p]*VSCALE);
    }
    const double F_ex = 2.0*t.proj(x);
    if (act) { a.F_rho[vo] = F_rho; a.F_rt[vo] = F_rt; a.F_exner[vo] = F_ex; }
}

// ---- launch 3 (after the Schur solve): the update, the half-time states, the norm partials (:1159-1183) -------------------------
struct Newton2UpdArgs {
    long long per; int nkn2, nmn2;                            // nEl nk n2; nk n2; (nk-1) n2
    const double *d_w, *d_rho, *d_rt, *d_exner;
    const double *velz_i, *rho_i, *rt_i, *exner_i;
    double *velz_j, *rho_j, *rt_j, *exner_j;                  // in: iterate before the update, out: after
    double *velz_h, *rho_h, *rt_h, *exner_h;                  // 0.5 x_i + 0.5 x_j
    double *nrm;                                              // [8][nEl][nk*n2]: squares of d_exner, exner, d_w, w, d_rho, rho, d_rt, rt
};
__global__ __launch_bounds__(256) void k_newton2_upd(Newton2UpdArgs a) {
    const long long vo = (long long)blockIdx.x*256 + threadIdx.x;
    if (vo >= a.per) return;
    const long long e = vo/a.nkn2; const int s = (int)(vo%a.nkn2);
    const double d_ex = a.d_exner[vo], d_rho = a.d_rho[vo], d_rt = a.d_rt[vo];
    const double ex = a.exner_j[vo] + d_ex, rho = a.rho_j[vo] + d_rho, rt = a.rt_j[vo] + d_rt;
    a.exner_j[vo] = ex; a.rho_j[vo] = rho; a.rt_j[vo] = rt;
    a.exner_h[vo] = 0.5*a.exner_i[vo] + 0.5*ex; a.rho_h[vo] = 0.5*a.rho_i[vo] + 0.5*rho; a.rt_h[vo] = 0.5*a.rt_i[vo] + 0.5*rt;
    a.nrm[0*a.per + vo] = d_ex*d_ex;   a.nrm[1*a.per + vo] = ex*ex;
    a.nrm[4*a.per + vo] = d_rho*d_rho; a.nrm[5*a.per + vo] = rho*rho;
    a.nrm[6*a.per + vo] = d_rt*d_rt;   a.nrm[7*a.per + vo] = rt*rt;
    double dw = 0.0, wn = 0.0;
    if (s < a.nmn2) {                                         // the nk-1 interfaces of the column; the row's last n2 entries stay zero
        const long long io = e*a.nmn2 + s;
        dw = a.d_w[io]; wn = a.velz_j[io] + dw;
        a.velz_j[io] = wn; a.velz_h[io] = 0.5*a.velz_i[io] + 0.5*wn;
    }
    a.nrm[2*a.per + vo] = dw*dw; a.nrm[3*a.per + vo] = wn*wn;
}

// the level counts mimsem_column_solve_schur_3 takes (column_hs.inc: nk < 4 is an argument error there too)
int newton2_check(const mimsem_ctx* c) {
    if (c->nk < 4) return MIMSEM_ERR_ARG;
    if (c->es.n < 1 || c->es.n > 4) return MIMSEM_ERR_UNSUPPORTED;
    return MIMSEM_OK;
}

}  // namespace

extern "C" {

int mimsem_column_newton2_residual(mimsem_ctx* c, double dt, double rayleigh,
        const double* theta_h, const double* Pi, const double* velz_i, const double* velz_j, const double* rho_i, const double* rho_j,
        const double* zv, const double* rt_i, const double* rt_j, const double* exner_j,
        const double* add_w, const double* add_rho_pre, const double* add_rt_pre, const double* add_rt_post,
        double* F_w, double* F_rho, double* F_rt, double* F_exner, double* k2i) {
    if (!c || !theta_h || !Pi || !velz_i || !velz_j || !rho_i || !rho_j || !zv || !rt_i || !rt_j || !exner_j ||
        !F_w || !F_rho || !F_rt || !F_exner || !k2i) return MIMSEM_ERR_ARG;
    int rc = newton2_check(c);
    if (rc) return rc;
    const long long nEl = c->nEl, nk = c->nk;
    if (nEl == 0) return MIMSEM_OK;
    mimsem::NewtonWS w;
    if ((rc = plan_col(c, w, false))) return rc;
    Newton2IfcArgs ia{};
    fill_newton_geo(c, ia.g);
    ia.dt = dt; ia.rayleigh = rayleigh; ia.theta = theta_h; ia.Pi = Pi; ia.velz1 = velz_i; ia.velz2 = velz_j; ia.rho1 = rho_i; ia.rho2 = rho_j;
    ia.add_w = add_w;
    ia.F = w.F; ia.G = w.G; ia.u = w.u; ia.fwA = w.fwA; ia.k2 = k2i;
    if ((rc = for_order<1, 2, 3, 4>(c->es.n, [&](auto N) { hipLaunchKernelGGL((k_newton2_ifc<N()>), dim3(newton_grid(nEl*(nk - 1))), dim3(64), 0, c->stream, ia); }))) return rc;
    MIMSEM_HIP_TRY(hipGetLastError());
    Newton2LevArgs la{};
    la.g = ia.g; la.dt = dt; la.zv = zv; la.rho_i = rho_i; la.rho_j = rho_j; la.rt_i = rt_i; la.rt_j = rt_j; la.exner_j = exner_j;
    la.add_rho_pre = add_rho_pre; la.add_rt_pre = add_rt_pre; la.add_rt_post = add_rt_post;
    la.F = ia.F; la.G = ia.G; la.u = ia.u; la.fwA = ia.fwA;
    la.F_w = F_w; la.F_rho = F_rho; la.F_rt = F_rt; la.F_exner = F_exner;
    if ((rc = for_order<1, 2, 3, 4>(c->es.n, [&](auto N) { hipLaunchKernelGGL((k_newton2_lev<N()>), dim3(newton_grid(nEl*nk)), dim3(64), 0, c->stream, la); }))) return rc;
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

int mimsem_column_newton2_update(mimsem_ctx* c, const double* d_w, const double* d_rho, const double* d_rt, const double* d_exner,
        const double* velz_i, const double* rho_i, const double* rt_i, const double* exner_i,
        double* velz_j, double* rho_j, double* rt_j, double* exner_j,
        double* velz_h, double* rho_h, double* rt_h, double* exner_h, double* norm_squares) {
    if (!c || !d_w || !d_rho || !d_rt || !d_exner || !velz_i || !rho_i || !rt_i || !exner_i || !velz_j || !rho_j || !rt_j || !exner_j ||
        !velz_h || !rho_h || !rt_h || !exner_h || !norm_squares) return MIMSEM_ERR_ARG;
    int rc = newton2_check(c);
    if (rc) return rc;
    Newton2UpdArgs a{};
    a.nkn2 = c->nk*c->es.n2e; a.nmn2 = (c->nk - 1)*c->es.n2e; a.per = (long long)c->nEl*a.nkn2;
    if (a.per == 0) return MIMSEM_OK;
    a.d_w = d_w; a.d_rho = d_rho; a.d_rt = d_rt; a.d_exner = d_exner;
    a.velz_i = velz_i; a.rho_i = rho_i; a.rt_i = rt_i; a.exner_i = exner_i;
    a.velz_j = velz_j; a.rho_j = rho_j; a.rt_j = rt_j; a.exner_j = exner_j;
    a.velz_h = velz_h; a.rho_h = rho_h; a.rt_h = rt_h; a.exner_h = exner_h; a.nrm = norm_squares;
    hipLaunchKernelGGL(k_newton2_upd, dim3((unsigned)((a.per + 255)/256)), dim3(256), 0, c->stream, a);
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

}  // extern "C"
