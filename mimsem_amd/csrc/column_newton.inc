// column_newton.inc -- included by column_kernels.hip after column_dpp.inc (same translation unit).
//
// Row C8 fused: the per-column residual assembly of the vertical Newton loop, VertSolve::assemble_residual_ec with
// diagnose_F_z / diagnose_Phi_z (eul/VertSolve.cpp:237-286, 432-502) and the right-hand sides, entropy variables and updates
// around the column Schur solve (VertSolve::solve_schur_eta, :1799-1912), for ALL columns in four launches instead of ~150
// single-operator calls:
//   k_newton_ifc   one task per (column, interface): F_z, G_z, the interface parts of F_w and of the corrections
//   k_newton_lev   one task per (column, level):     F_w completed, F_rho, F_rt -> F_eta, F_exner, theta in W3, eta
//   k_newton_upd   one task per (column, level):     eta_j, the state update, rho theta from the EOS, the half-time states, norms
//   k_diag_theta   one task per (column, interface / level): diagTheta2 and diagTheta_L2 (:289-352)
// The OTHER vertical Newton loop, VertSolve::solve_schur_2 (:1059-1246, the caller of solve_schur_column_3: assemble_residual :386-430, the
// right-hand sides of :1134-1154, the update of :1159-1183) runs on the same two residual kernels with EC = false and an update of its own:
//   k_newton_ifc / k_newton_lev <N, EC>   EC = true is the list above.  EC = false: theta lives on the nk+1 INTERFACES
//                  (AssembleLinearWithTheta, VertOps.cpp:669-730, not AssembleLinearWithRT), the pressure gradient and V10 G_z enter with dt
//                  (not dt/2), there are no entropy-conservation terms, no f_theta_corr and no entropy variables (F_rt is the output), and
//                  the horizontal forcing is added BEFORE the VB product (:1145-1149), the Held-Suarez term after it (:1151-1154)
//   k_newton2_upd  one thread per level entry:       x_j += d_x, x_h = 0.5 x_i + 0.5 x_j, the squares MaxNorm sums
// Every operator of the chain is W^T diag(c) W (or the inverse of one) with c a pointwise function of interpolated fields, so
// an APPLY never needs the block: interpolate the vector to the quadrature points (9 DPP FMAs), scale, project back (16 DPP
// FMAs).  Blocks are only formed where an inverse is needed (A^-1, B^-1, B(rho)^-1, B(rho theta)^-1).  Tasks are 16 lanes
// (four per wavefront) on the LDS-free row algebra of column_dpp.inc; only vectors travel between the launches.

namespace {

struct NewtonGeo {
    int nEl, nk;
    const double *det, *tI, *th, *w, *W, *Eg;
    double E[20];
};
template <class A> void fill_newton_geo(const mimsem_ctx* c, A& a) {
    a.nEl = c->nEl; a.nk = c->nk;
    a.det = c->d_det; a.tI = c->d_tI; a.th = c->d_th; a.w = c->d_w; a.W = c->d_W; a.Eg = c->d_E;
    for (int i = 0; i < 20; i++) a.E[i] = i < (int)c->tab.E.size() ? c->tab.E[i] : 0.0;
}

// what every task knows about itself: basis constants of my block row / quadrature point(s), metric of my column
template <int N>
struct ColTask {
    using R = dpp::Rows<N>;
    static constexpr int N2 = R::N2, NP = R::NP, MP12 = R::MP12, MP1 = R::MP1;
    typename R::Lane Ln;
    double Wt[MP12];                 // W[q][r]: my column of W (projection)
    double q0[NP], det[NP], Q[NP];   // w_q SCALE / det, det, w_q at my quadrature point(s)
    int e, r, rr;
    const NewtonGeo* g;

    __device__ void init(const NewtonGeo& G, int e_, int r_) {
        g = &G; e = e_; r = r_; rr = r < N2 ? r : N2 - 1;
        R::init_lane(Ln, G.Eg, G.W, r);
#pragma unroll
        for (int q = 0; q < MP12; q++) Wt[q] = G.W[q*N2 + rr];
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int q = min(r + 16*p, MP12 - 1);
            det[p] = G.det[(size_t)e*MP12 + q];
            Q[p] = G.w[q%MP1]*G.w[q/MP1];
            q0[p] = Q[p]*(VSCALE/det[p]);
        }
    }
    // the opening of a task kernel: four 16-lane tasks per wavefront, `per` of them in a column.  Sets me up for my task's column, hands
    // back its index within the column (a level or an interface) and says whether this lane stores: the rows past the last task of the
    // grid redo that task and store nothing, and so do the lanes past the block row (r >= N2)
    __device__ bool start(const NewtonGeo& G, int per, int& idx) {
        const int lane = threadIdx.x, r_ = lane%16;
        const long long task0 = (long long)blockIdx.x*4 + lane/16, ntask = (long long)G.nEl*per;
        const bool live = task0 < ntask;
        const long long task = live ? task0 : ntask - 1;
        const int e_ = (int)(task/per);
        idx = (int)(task%per);
        init(G, e_, r_);
        return live && r_ < N2;
    }
    __device__ void geo(double (&tI)[NP], double (&th)[NP], int k) const {
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int q = min(r + 16*p, MP12 - 1);
            const size_t go = ((size_t)k*g->nEl + e)*MP12 + q;
            tI[p] = g->tI[go]; th[p] = g->th[go];
        }
    }
    __device__ void interp(double (&out)[NP], double f) const { R::interp(out, Ln, f); }
    // (W^T v)[r] = sum_q W[q][r] v[q]
    __device__ double proj(const double (&v)[NP]) const {
        double s = 0.0;
        dpp::ProjAcc<N>::run(s, Wt, v);
        return s;
    }
    __device__ void block(double (&M)[N2], double (&c)[NP]) const { R::assemble(M, Ln, g->E, c); }
    __device__ void inv_block(double (&M)[N2], double (&c)[NP]) const { R::assemble(M, Ln, g->E, c); R::inverse(M, r); }
};

// ---- launch 1: interfaces ------------------------------------------------------------------------------------------------------
struct NewtonIfcArgs {
    NewtonGeo g;
    double dt, rayleigh;
    const double *theta, *Pi, *velz1, *velz2, *rho1, *rho2, *add_w;     // theta: EC [nEl][nk][n2], else [nEl][nk+1][n2]; add_w optional
    double *F, *G, *u, *wF, *fwA, *k2;                                    // [nEl][nk-1][n2] each; wF: EC only
};
template <int N, bool EC>
__global__ __launch_bounds__(64) void k_newton_ifc(NewtonIfcArgs a) {
    using T = ColTask<N>; using R = dpp::Rows<N>;
    constexpr int N2 = T::N2, NP = T::NP;
    const int nk = a.g.nk, nm = nk - 1;
    T t; int i;
    const bool act = t.start(a.g, nm, i);
    const int e = t.e;
    const double hdt = 0.5*a.dt;
    const size_t v0 = ((size_t)e*nk + i)*N2 + t.rr, v1 = v0 + N2, io = ((size_t)e*nm + i)*N2 + t.rr;

    double tI0[NP], th0[NP], tI1[NP], th1[NP];
    t.geo(tI0, th0, i); t.geo(tI1, th1, i + 1);
    // theta at the quadrature points: EC from the levels below and above, else of THIS interface, slot i+1 of the nk+1 (AssembleLinearWithTheta)
    double thq0[NP], thq1[NP], piq0[NP], piq1[NP], c[NP], x[NP];
    if constexpr (EC) { t.interp(thq0, a.theta[v0]); t.interp(thq1, a.theta[v1]); }
    else t.interp(thq0, a.theta[((size_t)e*(nk + 1) + i + 1)*N2 + t.rr]);
    t.interp(piq0, a.Pi[v0]);    t.interp(piq1, a.Pi[v1]);
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
    // F_w, the terms that live on this interface alone         assemble_residual_ec :432-502
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = (t.q0[p]*(0.5*th0[p]) + t.q0[p]*(0.5*th1[p]))*(v2q[p] - v1q[p]);     // VA w2 - VA w1 (AssembleLinear :242-267)
    double fw = t.proj(x);
    double cB0[NP], cB1[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) { cB0[p] = t.q0[p]*tI0[p]; cB1[p] = t.q0[p]*tI1[p]; }                 // AssembleConst :201-209
    // pressure gradient tA2 = A^-1 V01 (VB Pi); tA1 = VA(theta) tA2
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = cB1[p]*piq1[p];
    double bp = t.proj(x);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = cB0[p]*piq0[p];
    bp -= t.proj(x);
    const double gPi = R::matvec(Ai, bp);
    double cT[NP], gq[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        if constexpr (EC) cT[p] = t.q0[p]*(0.5*thq0[p]/t.det[p]) + t.q0[p]*(0.5*thq1[p]/t.det[p]);          // AssembleLinearWithRT :621-662
        else cT[p] = t.q0[p]*(0.5*th0[p])*(thq0[p]/t.det[p]) + t.q0[p]*(0.5*th1[p])*(thq0[p]/t.det[p]);      // AssembleLinearWithTheta :685-725
    }
    t.interp(gq, gPi);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = cT[p]*gq[p];
    const double tA1 = t.proj(x);
    fw += (EC ? hdt : a.dt)*tA1;                                                                              // assemble_residual_ec: dt/2; assemble_residual: dt (:412)
    // G_z = A^-1 VA(theta) F
    t.interp(gq, F);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = cT[p]*gq[p];
    const double G = R::matvec(Ai, t.proj(x));
    // Rayleigh friction on the three interfaces below the lid (AssembleRayleigh :826-888)
    {
        const int s = nk - 2 - i;
        const double wgt = (s == 0) ? 0.5 : (s == 1 ? 0.25 : (s == 2 ? 0.125 : 0.0));
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = (t.q0[p]*(wgt*(th1[p] + th0[p])))*(v2q[p] + v1q[p]);
        fw += hdt*a.rayleigh*t.proj(x);
    }
    double wF = 0.0;
    if constexpr (EC) {
        // entropy-conservation terms: + 0.5dt V01 (VB(theta) Pi) - 0.5dt C(grad theta)^T Pi;  grad theta = A^-1 V01 (VB theta)
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = (cB1[p]*(thq1[p]/(th1[p]*t.det[p])))*piq1[p];                    // AssembleConstWithRho(theta) :508-521
        double btp = t.proj(x);
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = (cB0[p]*(thq0[p]/(th0[p]*t.det[p])))*piq0[p];
        btp -= t.proj(x);
        fw += hdt*btp;
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = cB1[p]*thq1[p];
        double bt = t.proj(x);
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = cB0[p]*thq0[p];
        bt -= t.proj(x);
        const double gTh = R::matvec(Ai, bt);
        double cg[NP];
        t.interp(gq, gTh);
#pragma unroll
        for (int p = 0; p < NP; p++) cg[p] = t.q0[p]*(0.5*gq[p]/t.det[p]);
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = cg[p]*(piq0[p] + piq1[p]);
        fw -= hdt*t.proj(x);
        t.interp(gq, F);
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = cg[p]*gq[p];
        wF = t.proj(x);
    }
    if (a.add_w) fw += a.dt*a.add_w[io];
    if (act) {
        a.F[io] = F; a.G[io] = G; a.u[io] = u;
        if constexpr (EC) a.wF[io] = wF;
        a.fwA[io] = fw; a.k2[io] = F*tA1;
    }
}

// ---- launch 2: levels ----------------------------------------------------------------------------------------------------------
struct NewtonLevArgs {
    NewtonGeo g;
    double dt;
    // theta, rho_h, rt_h: EC only.  add_rho / add_rt (optional, times dt): EC adds them to F_rho / F_rt AFTER the VB product, else they
    // join dF_z / dG_z BEFORE it (:1145-1149)
    const double *theta, *zv, *rho_i, *rho_j, *rt_i, *rt_j, *rho_h, *rt_h, *exner_j, *add_rho, *add_rt;
    const double *F, *G, *u, *wF, *fwA;                       // what k_newton_ifc left (wF: EC only)
    double *F_w, *F_rho, *F_eta, *F_exner, *th_w3, *eta;      // F_eta, th_w3, eta: EC only
    const double* add_rt_post;                                // not EC only (optional, times dt): joins F_rt after the VB product (:1151-1154)
    double* F_rt;                                             // not EC only
};
template <int N, bool EC>
__global__ __launch_bounds__(64) void k_newton_lev(NewtonLevArgs a) {
    using T = ColTask<N>; using R = dpp::Rows<N>;
    constexpr int N2 = T::N2, NP = T::NP;
    const int nk = a.g.nk, nm = nk - 1;
    T t; int k;
    const bool act = t.start(a.g, nk, k);
    const int e = t.e;
    const double dt = a.dt, hdt = 0.5*a.dt;
    const size_t vo = ((size_t)e*nk + k)*N2 + t.rr;
    const bool lo = k > 0, hi = k < nk - 1;
    const size_t im = ((size_t)e*nm + (lo ? k - 1 : 0))*N2 + t.rr, ik = ((size_t)e*nm + (hi ? k : 0))*N2 + t.rr;
    // F_w of interface k: + dt V01 Phi, Phi_m = u_{m-1} + u_m + zv_m
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
    for (int p = 0; p < NP; p++) cB[p] = t.q0[p]*tI[p];
    // f_theta_corr = 0.5dt VB(theta) V10 F + 0.5dt C(grad theta) F       (:497-500)
    double ftc = 0.0;
    if constexpr (EC) {
        double thq[NP];
        t.interp(thq, a.theta[vo]); t.interp(q, V10F);
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = (cB[p]*(thq[p]/(th[p]*t.det[p])))*q[p];
        ftc = hdt*t.proj(x) + hdt*((lo ? a.wF[im] : 0.0) + (hi ? a.wF[ik] : 0.0));
    }
    // EC:   F_rho = VB (rho_j + dt V10 F - rho_i) + dt dFx,   F_rt = VB (rt_j + 0.5dt V10 G - rt_i) + f_theta_corr + dt dGx    (:1815-1826)
    // else: F_rho = VB (rho_j + dt V10 F - rho_i + dt dFx),   F_rt = VB (rt_j + dt V10 G - rt_i + dt dGx) + dt HS               (:1137-1154)
    double dF = (a.rho_j[vo] + dt*V10F) - a.rho_i[vo];
    if constexpr (!EC) { if (a.add_rho) dF += dt*a.add_rho[vo]; }
    t.interp(q, dF);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = cB[p]*q[p];
    double F_rho = t.proj(x);
    double dG = (a.rt_j[vo] + (EC ? hdt : dt)*V10G) - a.rt_i[vo];
    if constexpr (!EC) { if (a.add_rt) dG += dt*a.add_rt[vo]; }
    t.interp(q, dG);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = cB[p]*q[p];
    double F_rt = t.proj(x);
    double F_eta = 0.0, th_w3 = 0.0, eta = 0.0;
    if constexpr (EC) {
        F_rt += ftc;
        if (a.add_rho) F_rho += dt*a.add_rho[vo];
        if (a.add_rt) F_rt += dt*a.add_rt[vo];
        // entropy residual  F_eta = VB (VB(rt_h)^-1 F_rt - VB(rho_h)^-1 F_rho)                            (:1836-1842)
        double M[N2], rtq[NP];
        t.interp(rtq, a.rt_h[vo]);
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = cB[p]*(rtq[p]/(th[p]*t.det[p]));                                 // AssembleConstWithRhoInv :461-474
        t.inv_block(M, x);
        double t1 = R::matvec(M, F_rt);
        t.interp(q, a.rho_h[vo]);
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = cB[p]*(q[p]/(th[p]*t.det[p]));
        t.inv_block(M, x);
        t1 -= R::matvec(M, F_rho);
        t.interp(q, t1);
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = cB[p]*q[p];
        F_eta = t.proj(x);
        // theta_h in W3 and eta_h = VB^-1 (W^T Q log theta)                                               (:1844-1851)
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = cB[p]*rtq[p];
        th_w3 = R::matvec(M, t.proj(x));                                      // M = VB(rho_h)^-1
        t.interp(q, th_w3);
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = t.Q[p]*(VSCALE*log(q[p]/(th[p]*t.det[p])));                      // AssembleConstWithLogThetaPlusEta :1204-1255
        const double lg = t.proj(x);
#pragma unroll
        for (int p = 0; p < NP; p++) x[p] = cB[p];
        t.inv_block(M, x);
        eta = R::matvec(M, lg);
    } else {
        if (a.add_rt_post) F_rt += dt*a.add_rt_post[vo];
    }
    // EOS residual                                                                                    Assemble_EOS_Residual :987-1047
    double ek[NP];
    t.interp(q, a.rt_j[vo]); t.interp(ek, a.exner_j[vo]);
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const double rk = q[p]*(1.0/(t.det[p]*th[p])), ekk = ek[p]*(1.0/(t.det[p]*th[p]));
        double v = log(ekk) - (RD/CV)*log(rk) - log(CP) - (RD/CV)*log(RD/P0);
        x[p] = v*(0.5*t.Q[p]*VSCALE);
    }
    const double F_ex = 2.0*t.proj(x);
    if (act) {
        if constexpr (EC) { a.F_rho[vo] = F_rho; a.F_eta[vo] = F_eta; a.F_exner[vo] = F_ex; a.th_w3[vo] = th_w3; a.eta[vo] = eta; }
        else { a.F_rho[vo] = F_rho; a.F_rt[vo] = F_rt; a.F_exner[vo] = F_ex; }
    }
}

// ---- launch 3 (after the Schur solve): eta_j, update, EOS, half states, norm partials --------------------------------------------
struct NewtonUpdArgs {
    NewtonGeo g;
    const double *d_w, *d_rho, *d_eta, *d_exner;
    const double *velz_i, *rho_i, *rt_i, *exner_i;
    double *velz_j, *rho_j, *rt_j, *exner_j;                  // in: iterate before the update, out: after
    double *velz_h, *rho_h, *rt_h, *exner_h;                  // 0.5 (x_i + x_j)
    double *nrm;                                              // [8][nEl][nk*n2]: squares of d_exner, exner, d_w, w, d_rho, rho, d_eta, eta
};
template <int N>
__global__ __launch_bounds__(64) void k_newton_upd(NewtonUpdArgs a) {
    using T = ColTask<N>; using R = dpp::Rows<N>;
    constexpr int N2 = T::N2, NP = T::NP;
    const int nk = a.g.nk, nm = nk - 1;
    T t; int k;
    const bool act = t.start(a.g, nk, k);
    const int e = t.e;
    const size_t vo = ((size_t)e*nk + k)*N2 + t.rr;
    const bool hi = k < nk - 1;
    const size_t ik = ((size_t)e*nm + (hi ? k : 0))*N2 + t.rr;
    double tI[NP], th[NP], cB[NP], x[NP], q[NP], M[N2], Bi[N2];
    t.geo(tI, th, k);
#pragma unroll
    for (int p = 0; p < NP; p++) cB[p] = t.q0[p]*tI[p];
    // theta_j in W3 (before the update) and eta_j = VB^-1 W^T Q (log theta + d_eta)                   (:1858-1865)
    const double rho_old = a.rho_j[vo], rt_old = a.rt_j[vo];
    t.interp(q, rho_old);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = cB[p]*(q[p]/(th[p]*t.det[p]));
    t.inv_block(M, x);
    t.interp(q, rt_old);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = cB[p]*q[p];
    const double thw = R::matvec(M, t.proj(x));
    double dq[NP];
    const double d_eta = a.d_eta[vo];
    t.interp(q, thw); t.interp(dq, d_eta);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = t.Q[p]*(VSCALE*(log(q[p]/(th[p]*t.det[p])) + dq[p]/(th[p]*t.det[p])));
    const double lg = t.proj(x);
#pragma unroll
    for (int p = 0; p < NP; p++) x[p] = cB[p];
    t.inv_block(Bi, x);
    const double eta = R::matvec(Bi, lg);
    // the update                                                                                       (:1867-1872)
    const double d_rho = a.d_rho[vo], d_ex = a.d_exner[vo];
    const double rho_new = rho_old + d_rho, ex_new = a.exner_j[vo] + d_ex;
    double eq[NP];
    t.interp(q, rho_new); t.interp(eq, eta);
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const double rk = q[p]*(1.0/(th[p]*t.det[p])), ekk = eq[p]*(1.0/(th[p]*t.det[p]));
        x[p] = t.Q[p]*(VSCALE*rk*exp(ekk));                                                               // AssembleConstWithRhoExpEta :1257-1305
    }
    const double rt_new = R::matvec(Bi, t.proj(x));
    const size_t per = (size_t)a.g.nEl*nk*N2;
    if (act) {
        a.rho_j[vo] = rho_new; a.exner_j[vo] = ex_new; a.rt_j[vo] = rt_new;
        a.rho_h[vo] = 0.5*a.rho_i[vo] + 0.5*rho_new; a.exner_h[vo] = 0.5*a.exner_i[vo] + 0.5*ex_new; a.rt_h[vo] = 0.5*a.rt_i[vo] + 0.5*rt_new;
        a.nrm[0*per + vo] = d_ex*d_ex; a.nrm[1*per + vo] = ex_new*ex_new;
        a.nrm[4*per + vo] = d_rho*d_rho; a.nrm[5*per + vo] = rho_new*rho_new;
        a.nrm[6*per + vo] = d_eta*d_eta; a.nrm[7*per + vo] = eta*eta;
        double dw = 0.0, wn = 0.0;
        if (hi) {
            dw = a.d_w[ik]; wn = a.velz_j[ik] + dw;
            a.velz_j[ik] = wn; a.velz_h[ik] = 0.5*a.velz_i[ik] + 0.5*wn;
        }
        a.nrm[2*per + vo] = dw*dw; a.nrm[3*per + vo] = wn*wn;
    }
}

// ---- launch 3 of the solve_schur_2 loop: the update, the half-time states, the norm partials (:1159-1183) -- elementwise, no EOS ---
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

// ---- diagTheta2 / diagTheta_L2 (VertSolve.cpp:289-352) -----------------------------------------------------------------------
//   interface I in 0..nk:  theta_I = VA2(rho)_I^-1 (VAB2 rt)_I,  VA2 lumped (block diagonal): AssembleLinearWithRho2 :361-409, AssembleLinCon2 :319-359
//   level k:               theta_k = VB(rho)_k^-1 (VB rt)_k                                  : AssembleConstWithRhoInv, AssembleConst
// out = wa * diagnosed + wb * blend   (blend optional: the half-time averages of the Newton loop)
struct DiagThetaArgs {
    NewtonGeo g;
    const double *rho, *rt;
    double *theta2; const double* blend2;          // [nEl][(nk+1)*n2] or null
    double *thetaL; const double* blendL;          // [nEl][nk*n2] or null
    double wa, wb;
};
template <int N>
__global__ __launch_bounds__(64) void k_diag_theta(DiagThetaArgs a) {
    using T = ColTask<N>; using R = dpp::Rows<N>;
    constexpr int N2 = T::N2, NP = T::NP;
    const int nk = a.g.nk, np1 = nk + 1;
    T t; int I;
    const bool act = t.start(a.g, np1, I);
    const int e = t.e;
    const bool lo = I > 0, hi = I < nk;
    const size_t vm = ((size_t)e*nk + (lo ? I - 1 : 0))*N2 + t.rr, vk = ((size_t)e*nk + (hi ? I : 0))*N2 + t.rr;
    double x[NP], c[NP], q[NP], M[N2];
    double rqm[NP], rqk[NP], tqm[NP], tqk[NP];
    t.interp(rqm, a.rho[vm]); t.interp(rqk, a.rho[vk]); t.interp(tqm, a.rt[vm]); t.interp(tqk, a.rt[vk]);
    if (a.theta2) {
#pragma unroll
        for (int p = 0; p < NP; p++) {
            c[p] = (lo ? t.q0[p]*(0.5*rqm[p]/t.det[p]) : 0.0) + (hi ? t.q0[p]*(0.5*rqk[p]/t.det[p]) : 0.0);
            x[p] = (lo ? (t.q0[p]*0.5)*tqm[p] : 0.0) + (hi ? (t.q0[p]*0.5)*tqk[p] : 0.0);
        }
        const double rhs = t.proj(x);
        t.inv_block(M, c);
        double th2 = R::matvec(M, rhs);
        const size_t to = ((size_t)e*np1 + I)*N2 + t.rr;
        if (a.blend2) th2 = a.wa*th2 + a.wb*a.blend2[to];
        if (act) a.theta2[to] = th2;
    }
    if (a.thetaL && hi) {                 // (uniform over the 16-lane row: I is a task property)
        double tI[NP], th[NP];
        t.geo(tI, th, I);
#pragma unroll
        for (int p = 0; p < NP; p++) { const double cB = t.q0[p]*tI[p]; c[p] = cB*(rqk[p]/(th[p]*t.det[p])); x[p] = cB*tqk[p]; }
        const double rhs = t.proj(x);
        t.inv_block(M, c);
        double thl = R::matvec(M, rhs);
        if (a.blendL) thl = a.wa*thl + a.wb*a.blendL[vk];
        if (act) a.thetaL[vk] = thl;
    }
}

// grid of the Newton kernels: four tasks per wavefront
unsigned newton_grid(long long tasks) { return (unsigned)((tasks + 3)/4); }

int diag_theta_fused(mimsem_ctx* c, const double* rho, const double* rt, double* theta2, const double* blend2,
                     double* thetaL, const double* blendL, double wa, double wb) {
    DiagThetaArgs a{};
    fill_newton_geo(c, a.g);
    a.rho = rho; a.rt = rt; a.theta2 = theta2; a.blend2 = blend2; a.thetaL = thetaL; a.blendL = blendL; a.wa = wa; a.wb = wb;
    const unsigned grid = newton_grid((long long)c->nEl*(c->nk + 1));
    if (int rc = for_order<1, 2, 3, 4>(c->es.n, [&](auto N) { hipLaunchKernelGGL((k_diag_theta<N()>), dim3(grid), dim3(64), 0, c->stream, a); })) return rc;
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

// ---- diagTheta2 of the box twin (box/VertSolve.cpp:499-531): test functions upwinded by the VERTICAL velocity ------------------------
//   theta = VA2_up^-1 VAB2_up rt,   AssembleLinCon_up / AssembleLinearWithRho_up (box/VertOps.cpp:2601-2741), dtw = 0.25 dt.
// At quadrature point q of level k, with wb / wt the interpolants of velz at the interfaces below / above the level (0 at the two
// ends of the column, not divided by det):  N0b = (2 - dtw wb)/2, N1b = dtw wb/2, N0t = -dtw wt/2, N1t = (2 + dtw wt)/2, and
//   VAB2_up rows k / k+1, column k:   W^T diag((N0b + N0t)/2 q0) W,  W^T diag((N1b + N1t)/2 q0) W            (q0 = w_q SCALE / det)
//   VA2_up  (k,k) += rk N0b q0,  (k,k+1) = rk N0t q0,  (k+1,k) = rk N1b q0,  (k+1,k+1) += rk N1t q0          (rk = rho_k(q) / (2 det))
// so VA2_up is block TRIDIAGONAL over the nk + 1 interfaces and not symmetric (the lumped VA2 of k_diag_theta is block diagonal).
// One task per COLUMN: a block-Thomas sweep upwards,  D'_I = D_I - L_I G_{I-1},  G_I = D'_I^-1 U_I,  y_I = D'_I^-1 (f_I - L_I y_{I-1}),
// then theta_I = y_I - G_I theta_{I+1} downwards; G and y of every interface wait in the column workspace (mimsem::ThetaWupWS).
// The sweep does not pivot across blocks and the block inverse takes the diagonal pivots: with |dtw w| < 1 the off-diagonal blocks are
// O(dtw w) of the diagonal ones (N0t, N1b against N0b, N1t), so D'_I stays a small perturbation of a mass block.  Fixed order, no atomics.
struct DiagThetaWupArgs {
    NewtonGeo g;
    double dtw;
    const double *rho, *rt, *velz;                 // [nEl][nk n2], [nEl][nk n2], [nEl][(nk-1) n2]
    double* theta2; const double* blend2;          // [nEl][(nk+1) n2]; blend2 or null
    double *G, *y;                                 // ThetaWupWS
    double wa, wb;
};
template <int N>
__global__ __launch_bounds__(64) void k_diag_theta_wup(DiagThetaWupArgs a) {
    using T = ColTask<N>; using R = dpp::Rows<N>;
    constexpr int N2 = T::N2, NP = T::NP, nn = N2*N2;
    const int lane = threadIdx.x, r = lane%16;
    const int nk = a.g.nk, np1 = nk + 1, nm = nk - 1;
    const int e0 = blockIdx.x*4 + lane/16;
    const bool live = e0 < a.g.nEl;
    const int e = live ? e0 : a.g.nEl - 1;
    T t; t.init(a.g, e, r);
    const bool act = live && r < N2;
    const double* rho = a.rho + (size_t)e*nk*N2 + t.rr;
    const double* rt = a.rt + (size_t)e*nk*N2 + t.rr;
    const double* vz = a.velz + (size_t)e*nm*N2 + t.rr;
    double* Ge = a.G + (size_t)e*nk*nn + t.rr;          // blocks lane-major ([j][r]), as k_thomas_dpp keeps its factors
    double* ye = a.y + (size_t)e*np1*N2 + t.rr;
    double* tho = a.theta2 + (size_t)e*np1*N2 + t.rr;
    const double* blo = a.blend2 ? a.blend2 + (size_t)e*np1*N2 + t.rr : nullptr;
    const double wa = a.wa, wb = a.wb, dtw = a.dtw;
    // what level I - 1 leaves for interface I: its parts of D_I and f_I, the coefficient of L_I, and w at its top (= the bottom of level I)
    double cbb[NP], cba[NP], xm[NP], wq[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) cbb[p] = cba[p] = xm[p] = wq[p] = 0.0;
    double Gp[N2], yp = 0.0;
#pragma unroll
    for (int j = 0; j < N2; j++) Gp[j] = 0.0;
#pragma unroll 1
    for (int I = 0; I <= nk; I++) {                      // (I and nk are uniform: every lane of a row takes the same branches)
        const bool lo = I > 0, hi = I < nk;
        double cD[NP], cL[NP], cU[NP], x[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) { cD[p] = cbb[p]; cL[p] = cba[p]; x[p] = xm[p]; cU[p] = 0.0; }
        if (hi) {
            // (the rows of W of my quadrature points are fetched per level too, for the three interpolations: see the projection below)
            double Wr[NP][N2], rq[NP], tq[NP], wt[NP];
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const int q = min(r + 16*p, T::MP12 - 1);
#pragma unroll
                for (int j = 0; j < N2; j++) Wr[p][j] = a.g.W[q*N2 + j];
            }
            auto interp = [&](double (&out)[NP], double v) {
#pragma unroll
                for (int p = 0; p < NP; p++) { double s = 0.0; dpp::MatvecAcc<N2>::run(s, Wr[p], v); out[p] = s; }
            };
            interp(rq, rho[(size_t)I*N2]); interp(tq, rt[(size_t)I*N2]);
            if (I < nm) interp(wt, vz[(size_t)I*N2]);
            else {
#pragma unroll
                for (int p = 0; p < NP; p++) wt[p] = 0.0;
            }
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const double sb = dtw*wq[p], st = dtw*wt[p];
                const double N0b = 0.5*(2.0 - sb), N1b = 0.5*sb, N0t = 0.5*(-st), N1t = 0.5*(2.0 + st);
                const double rk = rq[p]*(0.5/t.det[p]);
                cD[p] += (rk*N0b)*t.q0[p]; cU[p] = (rk*N0t)*t.q0[p];
                cba[p] = (rk*N1b)*t.q0[p]; cbb[p] = (rk*N1t)*t.q0[p];
                x[p] += ((0.5*(N0b + N0t))*t.q0[p])*tq[p];
                xm[p] = ((0.5*(N1b + N1t))*t.q0[p])*tq[p];
                wq[p] = wt[p];
            }
        }
        // (W^T x)[r] with my column of W fetched here, once per interface, instead of ColTask's resident copy: at order 4 the 25 doubles
        // are what the sweep's three live blocks leave no registers for
        double f = 0.0;
        {
            double Wc[T::MP12];
#pragma unroll
            for (int q = 0; q < T::MP12; q++) Wc[q] = a.g.W[q*N2 + t.rr];
            dpp::ProjAcc<N>::run(f, Wc, x);
        }
        double D[N2];
        t.block(D, cD);
        if (lo) {
            double L[N2];
            t.block(L, cL);
            dpp::MulSub<N2>::run(D, L, Gp);
            f -= R::matvec(L, yp);
        }
        R::inverse(D, r);
        yp = R::matvec(D, f);
        if (act) ye[(size_t)I*N2] = yp;
        if (hi) {
            double U[N2];
            t.block(U, cU);
            R::mul(Gp, D, U);
            if (act) {
#pragma unroll
                for (int j = 0; j < N2; j++) Ge[(size_t)I*nn + j*N2] = Gp[j];
            }
        }
    }
    // back substitution: every lane re-reads its own row of G and its own entry of y (program order)
    double th = yp;
#pragma unroll 1
    for (int I = nk; I >= 0; I--) {
        if (I < nk) {
#pragma unroll
            for (int j = 0; j < N2; j++) Gp[j] = Ge[(size_t)I*nn + j*N2];
            th = ye[(size_t)I*N2] - R::matvec(Gp, th);
        }
        const double v = blo ? wa*th + wb*blo[(size_t)I*N2] : th;
        if (act) tho[(size_t)I*N2] = v;
    }
}

int diag_theta_wup(mimsem_ctx* c, double dtw, const double* rho, const double* rt, const double* velz, double* theta2,
                   const double* blend2, double wa, double wb) {
    mimsem::ThetaWupWS w;
    if (int rc = plan_col(c, w)) return rc;
    DiagThetaWupArgs a{};
    fill_newton_geo(c, a.g);
    a.dtw = dtw; a.rho = rho; a.rt = rt; a.velz = velz; a.theta2 = theta2; a.blend2 = blend2; a.G = w.G; a.y = w.y; a.wa = wa; a.wb = wb;
    const unsigned grid = newton_grid(c->nEl);
    if (int rc = for_order<1, 2, 3, 4>(c->es.n, [&](auto N) { hipLaunchKernelGGL((k_diag_theta_wup<N()>), dim3(grid), dim3(64), 0, c->stream, a); })) return rc;
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

// VertSolve::MaxNorm (eul/VertSolve.cpp:228) on the squares mimsem_column_newton_update leaves: one workgroup per column forms the eight sums
// (fixed order: a 256-thread tree over a strided partition -- reproducible) and writes the four ratios; a second launch takes their maxima
// over the columns (NaN wins, as a comparison on the host would see it)
__global__ __launch_bounds__(256) void k_max_norms_col(int nEl, long long rowlen, const double* __restrict__ nrm, double* __restrict__ ratio) {
    __shared__ double red[8][4];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const double* row = nrm + ((size_t)q*nEl + e)*rowlen;
        double acc = 0.0;
        for (long long t = tid; t < rowlen; t += 256) acc += row[t];
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        s[q] = acc;
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 8; q++) red[q][wave] = s[q];
    }
    __syncthreads();
    if (tid < 4) {
        const double num = (red[2*tid][0] + red[2*tid][1]) + (red[2*tid][2] + red[2*tid][3]);
        const double den = (red[2*tid + 1][0] + red[2*tid + 1][1]) + (red[2*tid + 1][2] + red[2*tid + 1][3]);
        ratio[(size_t)tid*nEl + e] = sqrt(num/den);
    }
}
__global__ __launch_bounds__(256) void k_max_norms_all(int nEl, const double* __restrict__ ratio, double* __restrict__ out) {
    __shared__ double red[4];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double m = 0.0;
    for (int e = tid; e < nEl; e += 256) { const double v = ratio[(size_t)q*nEl + e]; m = (v > m || v != v) ? v : m; }
    for (int off = 32; off > 0; off >>= 1) { const double v = __shfl_down(m, off, 64); m = (v > m || v != v) ? v : m; }
    if (lane == 0) red[wave] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; w++) { const double v = red[w]; m = (v > m || v != v) ? v : m; }
        out[q] = m;
    }
}

// the level counts mimsem_column_solve_schur_3 takes (column_hs.inc: nk < 4 is an argument error there too)
int newton2_check(const mimsem_ctx* c) {
    if (c->nk < 4) return MIMSEM_ERR_ARG;
    if (c->es.n < 1 || c->es.n > 4) return MIMSEM_ERR_UNSUPPORTED;
    return MIMSEM_OK;
}

// The two launches of a residual, for the entry of either loop (which has checked its arguments and its shape): ec = the solve_schur_eta
// loop.  The pointers of the other mode are null and its kernels never read them.
int newton_residual(mimsem_ctx* c, bool ec, double dt, double rayleigh,
        const double* theta, const double* Pi, const double* velz_i, const double* velz_j, const double* rho_i, const double* rho_j,
        const double* zv, const double* rt_i, const double* rt_j, const double* rho_h, const double* rt_h, const double* exner_j,
        const double* add_w, const double* add_rho, const double* add_rt, const double* add_rt_post,
        double* F_w, double* F_rho, double* F_eta, double* F_rt, double* F_exner, double* th_w3, double* eta, double* k2i) {
    const long long nEl = c->nEl, nk = c->nk;
    mimsem::NewtonWS w;
    int rc = plan_col(c, w, ec);                       // (wF is the entropy-conservation loop's alone)
    if (rc) return rc;
    NewtonIfcArgs ia{};
    fill_newton_geo(c, ia.g);
    ia.dt = dt; ia.rayleigh = rayleigh; ia.theta = theta; ia.Pi = Pi; ia.velz1 = velz_i; ia.velz2 = velz_j; ia.rho1 = rho_i; ia.rho2 = rho_j;
    ia.add_w = add_w;
    ia.F = w.F; ia.G = w.G; ia.u = w.u; ia.wF = w.wF; ia.fwA = w.fwA; ia.k2 = k2i;
    if ((rc = for_order<1, 2, 3, 4>(c->es.n, [&](auto N) {
            const dim3 grid(newton_grid(nEl*(nk - 1)));
            if (ec) hipLaunchKernelGGL((k_newton_ifc<N(), true>), grid, dim3(64), 0, c->stream, ia);
            else hipLaunchKernelGGL((k_newton_ifc<N(), false>), grid, dim3(64), 0, c->stream, ia);
        }))) return rc;
    MIMSEM_HIP_TRY(hipGetLastError());
    NewtonLevArgs la{};
    la.g = ia.g; la.dt = dt; la.theta = ec ? theta : nullptr; la.zv = zv; la.rho_i = rho_i; la.rho_j = rho_j; la.rt_i = rt_i; la.rt_j = rt_j;
    la.rho_h = rho_h; la.rt_h = rt_h; la.exner_j = exner_j; la.add_rho = add_rho; la.add_rt = add_rt; la.add_rt_post = add_rt_post;
    la.F = ia.F; la.G = ia.G; la.u = ia.u; la.wF = ia.wF; la.fwA = ia.fwA;
    la.F_w = F_w; la.F_rho = F_rho; la.F_eta = F_eta; la.F_rt = F_rt; la.F_exner = F_exner; la.th_w3 = th_w3; la.eta = eta;
    if ((rc = for_order<1, 2, 3, 4>(c->es.n, [&](auto N) {
            const dim3 grid(newton_grid(nEl*nk));
            if (ec) hipLaunchKernelGGL((k_newton_lev<N(), true>), grid, dim3(64), 0, c->stream, la);
            else hipLaunchKernelGGL((k_newton_lev<N(), false>), grid, dim3(64), 0, c->stream, la);
        }))) return rc;
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

}  // namespace

extern "C" {

int mimsem_column_newton_residual(mimsem_ctx* c, double dt, double rayleigh,
        const double* theta, const double* Pi, const double* velz_i, const double* velz_j, const double* rho_i, const double* rho_j,
        const double* zv, const double* rt_i, const double* rt_j, const double* rho_h, const double* rt_h, const double* exner_j,
        const double* add_w, const double* add_rho, const double* add_rt,
        double* F_w, double* F_rho, double* F_eta, double* F_exner, double* th_w3, double* eta, double* k2i) {
    if (!c || !theta || !Pi || !velz_i || !velz_j || !rho_i || !rho_j || !zv || !rt_i || !rt_j || !rho_h || !rt_h || !exner_j ||
        !F_w || !F_rho || !F_eta || !F_exner || !th_w3 || !eta || !k2i) return MIMSEM_ERR_ARG;
    if (c->nk < 2) return MIMSEM_ERR_ARG;
    if (!sweep_supported(c)) return MIMSEM_ERR_UNSUPPORTED;
    return newton_residual(c, true, dt, rayleigh, theta, Pi, velz_i, velz_j, rho_i, rho_j, zv, rt_i, rt_j, rho_h, rt_h, exner_j,
                           add_w, add_rho, add_rt, nullptr, F_w, F_rho, F_eta, nullptr, F_exner, th_w3, eta, k2i);
}

// The residual of the OTHER loop, VertSolve::solve_schur_2 (eul/VertSolve.cpp:1059-1246): assemble_residual (:386-430) and the right-hand
// sides of :1134-1154.  theta_h on the nk+1 interfaces; add_rho_pre / add_rt_pre join dF_z / dG_z before the VB product, add_rt_post after it
int mimsem_column_newton2_residual(mimsem_ctx* c, double dt, double rayleigh,
        const double* theta_h, const double* Pi, const double* velz_i, const double* velz_j, const double* rho_i, const double* rho_j,
        const double* zv, const double* rt_i, const double* rt_j, const double* exner_j,
        const double* add_w, const double* add_rho_pre, const double* add_rt_pre, const double* add_rt_post,
        double* F_w, double* F_rho, double* F_rt, double* F_exner, double* k2i) {
    if (!c || !theta_h || !Pi || !velz_i || !velz_j || !rho_i || !rho_j || !zv || !rt_i || !rt_j || !exner_j ||
        !F_w || !F_rho || !F_rt || !F_exner || !k2i) return MIMSEM_ERR_ARG;
    if (int rc = newton2_check(c)) return rc;
    if (c->nEl == 0) return MIMSEM_OK;
    return newton_residual(c, false, dt, rayleigh, theta_h, Pi, velz_i, velz_j, rho_i, rho_j, zv, rt_i, rt_j, nullptr, nullptr, exner_j,
                           add_w, add_rho_pre, add_rt_pre, add_rt_post, F_w, F_rho, nullptr, F_rt, F_exner, nullptr, nullptr, k2i);
}

int mimsem_column_newton_update(mimsem_ctx* c, const double* d_w, const double* d_rho, const double* d_eta, const double* d_exner,
        const double* velz_i, const double* rho_i, const double* rt_i, const double* exner_i,
        double* velz_j, double* rho_j, double* rt_j, double* exner_j,
        double* velz_h, double* rho_h, double* rt_h, double* exner_h, double* norm_squares) {
    if (!c || !d_w || !d_rho || !d_eta || !d_exner || !velz_i || !rho_i || !rt_i || !exner_i || !velz_j || !rho_j || !rt_j || !exner_j ||
        !velz_h || !rho_h || !rt_h || !exner_h || !norm_squares) return MIMSEM_ERR_ARG;
    if (c->nk < 2) return MIMSEM_ERR_ARG;
    if (!sweep_supported(c)) return MIMSEM_ERR_UNSUPPORTED;
    NewtonUpdArgs a{};
    fill_newton_geo(c, a.g);
    a.d_w = d_w; a.d_rho = d_rho; a.d_eta = d_eta; a.d_exner = d_exner;
    a.velz_i = velz_i; a.rho_i = rho_i; a.rt_i = rt_i; a.exner_i = exner_i;
    a.velz_j = velz_j; a.rho_j = rho_j; a.rt_j = rt_j; a.exner_j = exner_j;
    a.velz_h = velz_h; a.rho_h = rho_h; a.rt_h = rt_h; a.exner_h = exner_h; a.nrm = norm_squares;
    const unsigned grid = newton_grid((long long)c->nEl*c->nk);
    if (int rc = for_order<1, 2, 3, 4>(c->es.n, [&](auto N) { hipLaunchKernelGGL((k_newton_upd<N()>), dim3(grid), dim3(64), 0, c->stream, a); })) return rc;
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

int mimsem_column_max_norms(mimsem_ctx* c, const double* norm_squares, double* ratio_ws, double* out4) {
    if (!c || !norm_squares || !ratio_ws || !out4) return MIMSEM_ERR_ARG;
    if (c->nEl == 0) return MIMSEM_OK;
    const long long rowlen = (long long)c->nk*c->es.n2e;
    hipLaunchKernelGGL(k_max_norms_col, dim3((unsigned)c->nEl), dim3(256), 0, c->stream, c->nEl, rowlen, norm_squares, ratio_ws);
    hipLaunchKernelGGL(k_max_norms_all, dim3(4), dim3(256), 0, c->stream, c->nEl, ratio_ws, out4);
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

int mimsem_column_diag_theta_blend(mimsem_ctx* c, const double* rho, const double* rt, double* theta2, const double* blend2,
                                   double* thetaL, const double* blendL, double wa, double wb) {
    if (!c || !rho || !rt || (!theta2 && !thetaL)) return MIMSEM_ERR_ARG;
    if (!sweep_supported(c)) return MIMSEM_ERR_UNSUPPORTED;
    return diag_theta_fused(c, rho, rt, theta2, blend2, thetaL, blendL, wa, wb);
}

int mimsem_column_diag_theta_wup(mimsem_ctx* c, double dtw, const double* rho, const double* rt, const double* velz,
                                 double* theta2, const double* blend2, double wa, double wb) {
    if (!c || !rho || !rt || !velz || !theta2) return MIMSEM_ERR_ARG;
    if (c->nk < 2) return MIMSEM_ERR_ARG;
    if (!sweep_supported(c)) return MIMSEM_ERR_UNSUPPORTED;
    if (c->nEl == 0) return MIMSEM_OK;
    return diag_theta_wup(c, dtw, rho, rt, velz, theta2, blend2, wa, wb);
}

}  // extern "C"
