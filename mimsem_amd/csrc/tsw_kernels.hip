// tsw_kernels.hip -- the element-local 2-form half of a thermal shallow-water SSP-RK3 stage (mimsem_tsw_* of include/mimsem_hip.h).
//
// Reference: ThermalSW_EEC_2::solve_rk (src/ThermalSW_EEC_2.cpp:859-1004) with DO_THERMAL.  Every 2-form mass matrix is block-diagonal over the
// elements (Wmat, Whmat: one n^2 x n^2 block per element, src/Assembly.cpp:1558-1605), so everything of a stage that produces a 2-form is
// element-local: each output DoF is owned by one element, no atomics and no gather-sum.  1-form inputs are read through the element's edge
// slots, as the WtQUmat apply reads them.
//   k_tsw_diagnose  diagnose_s (:241), diagnose_Phi (:1019) and the h2 = M2^-1 M2h(h) h of rhs_u (:1045):
//                   Whmat(h) of the element assembled at the quadrature points, factored (unpivoted LU), s = M2h(h)^-1 M2 S,
//                   Phi = K(u) u + 1/2 M2 S + 1/4 M2h(s) h,  h2 = M2^-1 M2h(h) h  (M2^-1: the WMATINV element inverses).
//   k_tsw_update    the h and S updates of a stage (:894-1000 and rhs_S :1095):  div F = E21 F,
//                   fS = 1/2 M2 E21 G + 1/2 M2h(s) E21 F + K(grad s) F,
//                   h_j <- alpha h_i + beta (h_j - dt div F),  S_j <- alpha S_i + beta S_j - beta dt M2^-1 fS.
// Thickness: every integrand carries the level-0 inverse thickness exactly as the engine's own operators with flags 0 do -- none in
// Wmat, once in Whmat, twice in WtQUmat (qpoint_op, elem_kernels.hip) -- so the kernels equal those applies on any context; the shallow-water
// stack runs them at unit thickness (ThermalSW checks it).
// The src flavour keeps the SIGNED Jacobian determinant: where det < 0 the 2-form blocks are negative definite, so the factorisation takes
// no square roots and no positivity (LU without pivoting exists for every definite block, of either sign).
//
// Work mapping: one wavefront per workgroup, LPE lanes per element (16 at p <= 3, 32 at p = 4, 64 at p = 5): lane l is quadrature point l in
// the point phases and 2-form row l in the row phases; the element's block, its right-hand sides and the per-point integrands live in LDS.
// At config 3 (3 456 elements, p = 3) that is 864 one-wave workgroups, a few per CU.
#include <hip/hip_runtime.h>
#include "ctx.hpp"
#include "../../include/mimsem_hip.h"

namespace {

template <int N> struct TswDims {
    static constexpr int np1 = N + 1, mp1 = N + 1, mp12 = mp1*mp1, n1e = np1*N, n2e = N*N;
    static constexpr int LPE = mp12 <= 16 ? 16 : (mp12 <= 32 ? 32 : 64);
    static constexpr int EPB = 64/LPE;
    static_assert(n1e <= LPE && n2e <= LPE && mp12 <= LPE, "one lane per point, per row and per edge pair");
};

struct TswArgs {
    int nEl;
    const double *J, *det, *tI, *E;           // metric [nEl][4][mp12], [nEl][mp12]; inverse thickness of level 0; edge table [mp1][n]
    const double* w;                          // GLL weights [mp1]
    const int *i1x, *i1y, *i2;                // element slot tables (i2 null: element-contiguous 2-forms)
    const double* minv;                       // [nEl][n2e][n2e] row-major M2_e^-1 (mimsem_op_element_matrices(WMATINV))
    // diagnose
    const double *h, *S, *u;
    double *s, *Phi, *h2;
    // update
    const double *F, *G, *gs, *sv, *hi, *Si;
    double *hj, *Sj;
    double alpha, beta, dt;
};

// the element's metric at this lane's point (lane l < mp12)
struct TswPoint { double J00, J01, J10, J11, det, Q, tI; };

template <int N>
__device__ __forceinline__ TswPoint tsw_point(const TswArgs& a, int e, int l, bool on) {
    using D = TswDims<N>;
    TswPoint g{0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0};
    if (on && l < D::mp12) {
        const double* Je = a.J + (size_t)e*4*D::mp12;
        g.J00 = Je[l]; g.J01 = Je[D::mp12 + l]; g.J10 = Je[2*D::mp12 + l]; g.J11 = Je[3*D::mp12 + l];
        g.det = a.det[(size_t)e*D::mp12 + l];
        g.Q = a.w[l%D::mp1]*a.w[l/D::mp1];
        g.tI = a.tI[(size_t)e*D::mp12 + l];
    }
    return g;
}

// edge table and the 2-form basis at the points, W(q, j) = E(qx, jx) E(qy, jy), for the whole workgroup
template <int N>
__device__ __forceinline__ void tsw_tables(const TswArgs& a, double* sE, double* sW) {
    using D = TswDims<N>;
    for (int t = threadIdx.x; t < D::mp1*N; t += 64) sE[t] = a.E[t];
    __syncthreads();
    for (int t = threadIdx.x; t < D::mp12*D::n2e; t += 64) {
        const int q = t/D::n2e, j = t%D::n2e;
        sW[t] = sE[(q%D::mp1)*N + j%N]*sE[(q/D::mp1)*N + j/N];
    }
}

// local components of a staged 1-form at point (qx, qy) (Geom::interp1_l with the collocated nodal table)
template <int N>
__device__ __forceinline__ void tsw_interp1(const double* x, const double* sE, int qx, int qy, double& u, double& v) {
    using D = TswDims<N>;
    u = 0.0; v = 0.0;
#pragma unroll
    for (int j = 0; j < N; j++) {
        u += x[j*D::np1 + qx]*sE[qy*N + j];
        v += x[D::n1e + qy*N + j]*sE[qx*N + j];
    }
}

// WtQUmat(f) applied to x at one point, the 1/2 included (src/Assembly.cpp:1185-1196): f, x local components
__device__ __forceinline__ double tsw_wtqu(const TswPoint& g, double fu, double fv, double xu, double xv) {
    const double sd = 1.0/g.det;
    double ux0 = (g.J00*fu + g.J01*fv)/g.det, ux1 = (g.J10*fu + g.J11*fv)/g.det;      // interp1_g
    ux0 *= g.tI; ux1 *= g.tI;
    double caa = 0.5*(ux0*g.J00 + ux1*g.J10)*g.Q*sd, cab = 0.5*(ux0*g.J01 + ux1*g.J11)*g.Q*sd;
    caa *= g.tI; cab *= g.tI;
    return caa*xu + cab*xv;
}

// Whmat(f) point coefficient, src/Assembly.cpp:1580-1584 (interp2_g divides by det): fq = sum_j f_j W(q, j)
__device__ __forceinline__ double tsw_whc(const TswPoint& g, double fq) {
    const double sd = 1.0/g.det;
    double c = (fq/g.det)*g.Q*sd;
    c *= g.tI;
    return c;
}

template <int N>
__global__ __launch_bounds__(64) void k_tsw_diagnose(TswArgs a) {
    using D = TswDims<N>;
    constexpr int LPE = D::LPE, EPB = D::EPB, M = D::mp12, R = D::n2e, NE = D::n1e;
    __shared__ double sE[D::mp1*N], sW[M*R];
    __shared__ double sA[EPB][R*R];
    __shared__ double sh[EPB][R], sS[EPB][R], sb[EPB][R], sr[EPB][R], sx[EPB][R];
    __shared__ double su[EPB][2*NE];
    __shared__ double sc[EPB][M], sp[EPB][M], sq[EPB][M], sk[EPB][M];
    const int el = threadIdx.x/LPE, l = threadIdx.x%LPE;
    const int eg = blockIdx.x*EPB + el;
    const bool act = eg < a.nEl;
    const int e = act ? eg : 0;
    tsw_tables<N>(a, sE, sW);
    const int slot = (act && l < R) ? (a.i2 ? a.i2[e*R + l] : e*R + l) : -1;
    if (l < R) { sh[el][l] = slot >= 0 ? a.h[slot] : 0.0; sS[el][l] = slot >= 0 ? a.S[slot] : 0.0; }
    if (l < NE) { su[el][l] = act ? a.u[a.i1x[e*NE + l]] : 0.0; su[el][NE + l] = act ? a.u[a.i1y[e*NE + l]] : 0.0; }
    const TswPoint g = tsw_point<N>(a, e, l, act);
    __syncthreads();

    // points: the integrands of M2 S, M2h(h) h, K(u) u and the Whmat(h) coefficient
    double hq = 0.0;
    if (l < M) {
        double Sq = 0.0;
#pragma unroll
        for (int j = 0; j < R; j++) { hq += sh[el][j]*sW[l*R + j]; Sq += sS[el][j]*sW[l*R + j]; }
        double uu, uv;
        tsw_interp1<N>(su[el], sE, l%D::mp1, l/D::mp1, uu, uv);
        const double ch = tsw_whc(g, hq);
        sc[el][l] = ch;
        sp[el][l] = (g.Q*(1.0/g.det))*Sq;                   // Wmat
        sq[el][l] = ch*hq;
        sk[el][l] = tsw_wtqu(g, uu, uv, uu, uv);
    }
    __syncthreads();

    // rows: the Whmat(h) block, M2 S, M2h(h) h and the first two terms of Phi
    double phi = 0.0;
    if (l < R) {
        double b = 0.0, r = 0.0, k = 0.0;
#pragma unroll 4
        for (int q = 0; q < M; q++) {
            const double wq = sW[q*R + l];
            b += wq*sp[el][q]; r += wq*sq[el][q]; k += wq*sk[el][q];
        }
#pragma unroll 1
        for (int j = 0; j < R; j++) {
            double m = 0.0;
#pragma unroll 4
            for (int q = 0; q < M; q++) m += (sW[q*R + l]*sc[el][q])*sW[q*R + j];
            sA[el][l*R + j] = m;
        }
        sb[el][l] = b; sr[el][l] = r;
        phi = k + 0.5*b;
    }
    __syncthreads();

    // s = M2h(h)^-1 M2 S: LU without pivoting (a definite block of either sign), lane l keeps row l
#pragma unroll 1
    for (int k = 0; k < R - 1; k++) {
        if (l > k && l < R) {
            const double f = sA[el][l*R + k]/sA[el][k*R + k];
            for (int j = k + 1; j < R; j++) sA[el][l*R + j] -= f*sA[el][k*R + j];
            sb[el][l] -= f*sb[el][k];
        }
        __syncthreads();
    }
#pragma unroll 1
    for (int k = R - 1; k >= 0; k--) {
        const double xk = sb[el][k]/sA[el][k*R + k];
        if (l < k) sb[el][l] -= sA[el][l*R + k]*xk;
        if (l == k) sx[el][k] = xk;
        __syncthreads();
    }

    // points: the M2h(s) h integrand
    if (l < M) {
        double s_q = 0.0;
#pragma unroll
        for (int j = 0; j < R; j++) s_q += sx[el][j]*sW[l*R + j];
        sp[el][l] = tsw_whc(g, s_q)*hq;
    }
    __syncthreads();
    if (l < R) {
        double t = 0.0, h2v = 0.0;
#pragma unroll 4
        for (int q = 0; q < M; q++) t += sW[q*R + l]*sp[el][q];
        const double* Bi = a.minv + ((size_t)e*R + l)*R;
#pragma unroll 4
        for (int k = 0; k < R; k++) h2v += Bi[k]*sr[el][k];
        phi += 0.25*t;
        if (slot >= 0) { a.s[slot] = sx[el][l]; a.Phi[slot] = phi; a.h2[slot] = h2v; }
    }
}

template <int N>
__global__ __launch_bounds__(64) void k_tsw_update(TswArgs a) {
    using D = TswDims<N>;
    constexpr int LPE = D::LPE, EPB = D::EPB, M = D::mp12, R = D::n2e, NE = D::n1e;
    __shared__ double sE[D::mp1*N], sW[M*R];
    __shared__ double sF[EPB][2*NE], sG[EPB][2*NE], sg[EPB][2*NE];
    __shared__ double ss[EPB][R], sdF[EPB][R], sdG[EPB][R], sf[EPB][R];
    __shared__ double sp[EPB][M];
    const int el = threadIdx.x/LPE, l = threadIdx.x%LPE;
    const int eg = blockIdx.x*EPB + el;
    const bool act = eg < a.nEl;
    const int e = act ? eg : 0;
    tsw_tables<N>(a, sE, sW);
    const int slot = (act && l < R) ? (a.i2 ? a.i2[e*R + l] : e*R + l) : -1;
    double hi = 0.0, hj = 0.0, Si = 0.0, Sj = 0.0;
    if (slot >= 0) { hi = a.hi[slot]; hj = a.hj[slot]; Si = a.Si[slot]; Sj = a.Sj[slot]; }
    if (l < R) ss[el][l] = slot >= 0 ? a.sv[slot] : 0.0;
    if (l < NE) {
        const int sx = act ? a.i1x[e*NE + l] : -1, sy = act ? a.i1y[e*NE + l] : -1;
        sF[el][l] = sx >= 0 ? a.F[sx] : 0.0; sF[el][NE + l] = sy >= 0 ? a.F[sy] : 0.0;
        sG[el][l] = sx >= 0 ? a.G[sx] : 0.0; sG[el][NE + l] = sy >= 0 ? a.G[sy] : 0.0;
        sg[el][l] = sx >= 0 ? a.gs[sx] : 0.0; sg[el][NE + l] = sy >= 0 ? a.gs[sy] : 0.0;
    }
    const TswPoint g = tsw_point<N>(a, e, l, act);
    __syncthreads();

    // rows: E21 (src/Assembly.cpp E21mat; face (ii, jj) <- its four edges)
    double divF = 0.0;
    if (l < R) {
        const int jj = l%N, ii = l/N;
        const double* x = sF[el]; const double* y = sF[el] + NE;
        divF = -x[ii*D::np1 + jj] + x[ii*D::np1 + jj + 1] - y[ii*N + jj] + y[(ii + 1)*N + jj];
        x = sG[el]; y = sG[el] + NE;
        sdG[el][l] = -x[ii*D::np1 + jj] + x[ii*D::np1 + jj + 1] - y[ii*N + jj] + y[(ii + 1)*N + jj];
        sdF[el][l] = divF;
    }
    __syncthreads();

    // points: the fS integrand  1/2 Wmat (E21 G) + 1/2 Whmat(s) (E21 F) + WtQUmat(grad s) F
    if (l < M) {
        double s_q = 0.0, dF = 0.0, dG = 0.0;
#pragma unroll
        for (int j = 0; j < R; j++) {
            const double wj = sW[l*R + j];
            s_q += ss[el][j]*wj; dF += sdF[el][j]*wj; dG += sdG[el][j]*wj;
        }
        double Fu, Fv, gu, gv;
        tsw_interp1<N>(sF[el], sE, l%D::mp1, l/D::mp1, Fu, Fv);
        tsw_interp1<N>(sg[el], sE, l%D::mp1, l/D::mp1, gu, gv);
        sp[el][l] = 0.5*((g.Q*(1.0/g.det))*dG) + 0.5*(tsw_whc(g, s_q)*dF) + tsw_wtqu(g, gu, gv, Fu, Fv);
    }
    __syncthreads();
    if (l < R) {
        double f = 0.0;
        for (int q = 0; q < M; q++) f += sW[q*R + l]*sp[el][q];
        sf[el][l] = f;
    }
    __syncthreads();
    if (l < R) {
        const double* Bi = a.minv + ((size_t)e*R + l)*R;
        double m = 0.0;
#pragma unroll
        for (int k = 0; k < R; k++) m += Bi[k]*sf[el][k];
        if (slot >= 0) {
            a.hj[slot] = a.alpha*hi + a.beta*(hj - a.dt*divF);
            a.Sj[slot] = a.alpha*Si + a.beta*Sj - (a.beta*a.dt)*m;
        }
    }
}

TswArgs tsw_args(const mimsem_ctx* c, const double* minv) {
    TswArgs a{};
    a.nEl = c->nEl; a.J = c->d_J; a.det = c->d_det; a.tI = c->d_tI; a.E = c->d_E; a.w = c->d_w;
    a.i1x = c->d_i1x; a.i1y = c->d_i1y; a.i2 = c->d_i2; a.minv = minv;
    return a;
}

template <int N>
int tsw_launch(mimsem_ctx* c, bool update, const TswArgs& a) {
    using D = TswDims<N>;
    const unsigned grid = (unsigned)((a.nEl + D::EPB - 1)/D::EPB);
    if (update) hipLaunchKernelGGL(k_tsw_update<N>, dim3(grid), dim3(64), 0, c->stream, a);
    else hipLaunchKernelGGL(k_tsw_diagnose<N>, dim3(grid), dim3(64), 0, c->stream, a);
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

int tsw_dispatch(mimsem_ctx* c, bool update, const TswArgs& a) {
    switch (c->es.n) {
    case 2: return tsw_launch<2>(c, update, a);
    case 3: return tsw_launch<3>(c, update, a);
    case 4: return tsw_launch<4>(c, update, a);
    case 5: return tsw_launch<5>(c, update, a);
    default: return MIMSEM_ERR_UNSUPPORTED;
    }
}

// what both entries need of the context: one level (the shallow-water stack), an order with a built kernel, the metric tables
int tsw_check_ctx(const mimsem_ctx* c) {
    if (!c || c->nk != 1) return MIMSEM_ERR_ARG;
    if (c->es.n < 2 || c->es.n > 5) return MIMSEM_ERR_UNSUPPORTED;
    if (c->nEl > 0 && (!c->d_J || !c->d_det || !c->d_tI || !c->d_E || !c->d_w || !c->d_i1x || !c->d_i1y)) return MIMSEM_ERR_STATE;
    return MIMSEM_OK;
}

}  // namespace

extern "C" {

int mimsem_tsw_diagnose(mimsem_ctx* c, const double* h, const double* S, const double* u, const double* m2inv,
                        double* s, double* Phi, double* h2) {
    int rc = tsw_check_ctx(c);
    if (rc) return rc;
    if (!h || !S || !u || !m2inv || !s || !Phi || !h2) return MIMSEM_ERR_ARG;
    if (c->nEl == 0) return MIMSEM_OK;
    TswArgs a = tsw_args(c, m2inv);
    a.h = h; a.S = S; a.u = u; a.s = s; a.Phi = Phi; a.h2 = h2;
    return tsw_dispatch(c, false, a);
}

int mimsem_tsw_update(mimsem_ctx* c, const double* F, const double* G, const double* grad_s, const double* s, const double* m2inv,
                      const double* h_i, const double* S_i, double* h_j, double* S_j, double alpha, double beta, double dt) {
    int rc = tsw_check_ctx(c);
    if (rc) return rc;
    if (!F || !G || !grad_s || !s || !m2inv || !h_i || !S_i || !h_j || !S_j) return MIMSEM_ERR_ARG;
    if (c->nEl == 0) return MIMSEM_OK;
    TswArgs a = tsw_args(c, m2inv);
    a.F = F; a.G = G; a.gs = grad_s; a.sv = s; a.hi = h_i; a.Si = S_i; a.hj = h_j; a.Sj = S_j;
    a.alpha = alpha; a.beta = beta; a.dt = dt;
    return tsw_dispatch(c, true, a);
}

}  // extern "C"
