// column_hs.inc -- included at the end of column_kernels.hip (same translation unit: shares CG, BA, Band, plan_col, for_order, bmm, ...).
//
// The column rows of the Strang / Held-Suarez path (SURVEY 8(a) C2-C6 remainder):
//   * AssembleLinearWithRho2_up / AssembleLinCon2_up   eul/VertOps.cpp:1415-1561  (test functions at departure points)
//   * diagTheta_up                                      eul/VertSolve.cpp:354-384
//   * AssembleTempForcing_HS                            eul/VertOps.cpp:1563-1633
//   * solve_schur_column_3                              eul/VertSolve.cpp:504-675   (block-PENTAdiagonal Schur complement)
// The Schur chain is written on a small block-banded matrix algebra (Band): every factor of the reference's
// MatMatMult chain is block diagonal / bidiagonal / tridiagonal, so the products are formed band by band.

namespace {

// ---- LagrangeNode::evalDeriv / LagrangeEdge::eval at an arbitrary point (eul/Basis.cpp:189-210, :274-283) ----
__device__ double d_node_deriv(int n, const double* xn, double x, int i) {
    double b = 0.0;
    for (int j = 0; j <= n; j++) {
        if (j == i) continue;
        double a = 1.0;
        for (int k = 0; k <= n; k++) {
            if (k == i || k == j) continue;
            a *= (x - xn[k])/(xn[i] - xn[k]);
        }
        b += a/(xn[i] - xn[j]);
    }
    return b;
}
__device__ double d_edge_eval(int n, const double* xn, double x, int i) {
    double c = 0.0;
    for (int j = 0; j <= i; j++) c -= d_node_deriv(n, xn, x, j);
    return c;
}

// per-level blocks with upwinded test functions: L[e][k] = Wt_up(k) diag(c_k) W
//   c_k = w S/det * 0.5 * rho_k/det (RHO2_UP)  or  w S/det * 0.5 (LINCON2_UP);  Wt_up[j][q] = e_jx(x_q + dt ul0) e_jy(y_q + dt ul1)
struct UpArgs {
    CG g; const double *J, *xn, *uh, *rho; long long uhs; const int *i1x, *i1y; double dt; int with_rho;
};
__global__ __launch_bounds__(256) void k_up_level_blocks(UpArgs a, double* __restrict__ L) {
    extern __shared__ double sm[];
    const CG& g = a.g;
    const int n = g.n, np1 = n + 1, mp1 = g.mp1, mp12 = g.mp12, n2 = g.n2, nn = n2*n2, n1e = np1*n, tid = threadIdx.x;
    const int k = blockIdx.x%g.nk, e = blockIdx.x/g.nk;
    double* sW = sm;                 // [mp12][n2]
    double* sT = sW + mp12*n2;       // [mp12][n2]  upwinded test functions
    double* sc = sT + mp12*n2;       // [mp12]
    double* su = sc + mp12;          // [2*n1e] velocity DoFs of the element at level k
    for (int t = tid; t < mp12*n2; t += 256) sW[t] = g_W(g, t/n2, t%n2);
    const double* uv = a.uh + (size_t)k*a.uhs;
    for (int t = tid; t < n1e; t += 256) { su[t] = uv[a.i1x[e*n1e + t]]; su[n1e + t] = uv[a.i1y[e*n1e + t]]; }
    __syncthreads();
    if (tid < mp12) {
        const int q = tid, qx = q%mp1, qy = q/mp1;
        const double det = g.det[(size_t)e*mp12 + q];
        double c = g_Q(g, q)*(VSCALE/det);
        if (a.with_rho) { const double rk = wint(g, a.rho, g.nk, e, k, q); c *= 0.5*rk/det; }
        else c *= 0.5;
        sc[q] = c;
        double u = 0.0, v = 0.0;                                  // Geom::interp1_l with collocated nodes
        for (int j = 0; j < n; j++) { u += su[j*np1 + qx]*g.E[qy*n + j]; v += su[n1e + qy*n + j]*g.E[qx*n + j]; }
        const double* Je = a.J + (size_t)e*4*mp12;
        const double J00 = Je[q], J01 = Je[mp12 + q], J10 = Je[2*mp12 + q], J11 = Je[3*mp12 + q];
        const double ug0 = (J00*u + J01*v)/det, ug1 = (J10*u + J11*v)/det;      // interp1_g
        double ul0 = (+J11*ug0 - J01*ug1)/det, ul1 = (-J10*ug0 + J00*ug1)/det;
        const double tI = g_tI(g, e, k, q);
        ul0 *= tI; ul1 *= tI;
        const double px = a.xn[qx] + a.dt*ul0, py = a.xn[qy] + a.dt*ul1;          // quadrature points == nodes
        double ex_[8], ey_[8];
        for (int j = 0; j < n; j++) { ex_[j] = d_edge_eval(n, a.xn, px, j); ey_[j] = d_edge_eval(n, a.xn, py, j); }
        for (int j = 0; j < n2; j++) sT[q*n2 + j] = ex_[j%n]*ey_[j/n];
    }
    __syncthreads();
    double* out = L + ((size_t)e*g.nk + k)*nn;
    for (int t = tid; t < nn; t += 256) {
        const int ii = t/n2, jj = t%n2;
        double s = 0.0;
        for (int q = 0; q < mp12; q++) s += (sT[q*n2 + ii]*sc[q])*sW[q*n2 + jj];
        out[t] = s;
    }
}

}  // namespace

int up_blocks_into_impl(mimsem_ctx* c, int colop, const double* rho, double* M, double* tmpM) {
    if (!c->col_uh) return MIMSEM_ERR_ARG;
    if (colop == MIMSEM_V_LINEAR_RHO2_UP && !rho) return MIMSEM_ERR_ARG;
    UpArgs a;
    a.g = make_cg(c); a.J = c->d_J; a.xn = c->d_xn; a.uh = c->col_uh; a.uhs = c->col_uhs; a.rho = rho;
    a.i1x = c->d_i1x; a.i1y = c->d_i1y; a.dt = c->col_param; a.with_rho = (colop == MIMSEM_V_LINEAR_RHO2_UP);
    const int nk = c->nk, n2 = c->es.n2e, nn = n2*n2, nEl = c->nEl, mp12 = c->es.mp12;
    double* L = tmpM;
    const size_t lds = (size_t)(2*mp12*n2 + mp12 + 2*c->es.n1e)*sizeof(double);
    if (lds > 64*1024)
        MIMSEM_HIP_TRY(hipFuncSetAttribute((const void*)k_up_level_blocks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_up_level_blocks, dim3((unsigned)(nEl*nk)), dim3(256), lds, c->stream, a, L);
    MIMSEM_HIP_TRY(hipGetLastError());
    if (colop == MIMSEM_V_LINEAR_RHO2_UP)      // rows kk and kk+1 both receive level kk's block (:1468-1478)
        return each(c, (long long)nEl*(nk + 1)*nn, [=] __device__(long long i) {
            const int ij = (int)(i%nn); long long t = i/nn; const int r = (int)(t%(nk + 1)), e = (int)(t/(nk + 1));
            double s = 0.0;
            if (r > 0)  s += L[((size_t)e*nk + r - 1)*nn + ij];
            if (r < nk) s += L[((size_t)e*nk + r)*nn + ij];
            M[i] = s;
        });
    // LINCON2_UP: stored (r,0) = (r, r-1) = level r-1's block, (r,1) = (r, r) = level r's block  (:1538-1550)
    return each(c, (long long)nEl*(nk + 1)*2*nn, [=] __device__(long long i) {
        const int ij = (int)(i%nn); long long t = i/nn; const int w = (int)(t%2); t /= 2;
        const int r = (int)(t%(nk + 1)), e = (int)(t/(nk + 1));
        const int lev = r - 1 + w;
        M[i] = (lev >= 0 && lev < nk) ? L[((size_t)e*nk + lev)*nn + ij] : 0.0;
    });
}

namespace {
int up_blocks_into(mimsem_ctx* c, int colop, const double* rho, double* M, double* tmpM) {
    return up_blocks_into_impl(c, colop, rho, M, tmpM);
}

// ---- block-banded matrices: blocks [e][r][b] (n2 x n2 each), block column = r + lo + b, b in [0, nb) ----

// one workgroup per block row (e, r) of C: the A.nb blocks of A's row and the A.nb x B.nb blocks of B they meet are staged in LDS
// (coalesced 648-B reads at p = 3), every output entry is formed from LDS in the same order as the entry-per-thread version below
// (which read both operands through L1 for every entry: 324 us per call against ~150 us)
__global__ __launch_bounds__(256) void k_band_mul(int n2, Band C, Band A, Band B, double alpha) {
    extern __shared__ double sm[];
    const int nn = n2*n2, tid = threadIdx.x;
    const int r = blockIdx.x%C.nr, e = blockIdx.x/C.nr;
    double* sA = sm; double* sB = sm + (size_t)A.nb*nn;
    for (int x = tid; x < A.nb*nn; x += 256) {
        const int a = x/nn, ij = x%nn, m = r + A.lo + a;
        sA[x] = (m >= 0 && m < A.nc) ? A.p[(((size_t)e*A.nr + r)*A.nb + a)*nn + ij] : 0.0;
    }
    for (int x = tid; x < A.nb*B.nb*nn; x += 256) {
        const int ab = x/nn, ij = x%nn, a = ab/B.nb, b = ab%B.nb, m = r + A.lo + a;
        sB[x] = (m >= 0 && m < A.nc) ? B.p[(((size_t)e*B.nr + m)*B.nb + b)*nn + ij] : 0.0;
    }
    __syncthreads();
    for (int x = tid; x < C.nb*nn; x += 256) {
        const int cb = x/nn, ij = x%nn, ii = ij/n2, jj = ij%n2;
        const int col = r + C.lo + cb;
        double s = 0.0;
        if (col >= 0 && col < C.nc) {
            for (int a = 0; a < A.nb; a++) {
                const int m = r + A.lo + a, b = col - m - B.lo;
                if (m < 0 || m >= A.nc || b < 0 || b >= B.nb) continue;
                const double* pa = sA + (size_t)a*nn; const double* pb = sB + ((size_t)a*B.nb + b)*nn;
                for (int k = 0; k < n2; k++) s += pa[ii*n2 + k]*pb[k*n2 + jj];
            }
        }
        C.p[(((size_t)e*C.nr + r)*C.nb + cb)*nn + ij] = alpha*s;
    }
}

// C = alpha * A . B   (band of C: lo = A.lo + B.lo, nb = A.nb + B.nb - 1)
int band_mul(mimsem_ctx* c, Band C, Band A, Band B, double alpha) {
    const int n2 = c->es.n2e, nn = n2*n2, nEl = c->nEl;
    if (C.nr != A.nr || C.nc != B.nc || A.nc != B.nr || C.lo != A.lo + B.lo || C.nb != A.nb + B.nb - 1) return MIMSEM_ERR_STATE;
    const size_t lds = (size_t)(A.nb + A.nb*B.nb)*nn*sizeof(double);
    if (lds <= 64*1024 && !exp_env("MIMSEM_BAND_NAIVE")) {
        if ((long long)nEl*C.nr == 0) return MIMSEM_OK;
        hipLaunchKernelGGL(k_band_mul, dim3((unsigned)(nEl*C.nr)), dim3(256), lds, c->stream, n2, C, A, B, alpha);
        MIMSEM_HIP_TRY(hipGetLastError());
        return MIMSEM_OK;
    }
    return each(c, (long long)nEl*C.nr*C.nb*nn, [=] __device__(long long x) {
        const int ij = (int)(x%nn), ii = ij/n2, jj = ij%n2; long long t = x/nn;
        const int cb = (int)(t%C.nb); t /= C.nb; const int r = (int)(t%C.nr), e = (int)(t/C.nr);
        const int col = r + C.lo + cb;
        double s = 0.0;
        if (col >= 0 && col < C.nc) {
            for (int a = 0; a < A.nb; a++) {
                const int m = r + A.lo + a, b = col - m - B.lo;
                if (m < 0 || m >= A.nc || b < 0 || b >= B.nb) continue;
                const double* pa = A.p + (((size_t)e*A.nr + r)*A.nb + a)*nn;
                const double* pb = B.p + (((size_t)e*B.nr + m)*B.nb + b)*nn;
                for (int k = 0; k < n2; k++) s += pa[ii*n2 + k]*pb[k*n2 + jj];
            }
        }
        C.p[x] = alpha*s;
    });
}
// C = alpha*A + beta*B ; C's band must cover both
int band_lincomb(mimsem_ctx* c, Band C, double alpha, Band A, double beta, Band B) {
    const int n2 = c->es.n2e, nn = n2*n2, nEl = c->nEl;
    if (C.nr != A.nr || C.nr != B.nr || C.nc != A.nc || C.nc != B.nc) return MIMSEM_ERR_STATE;
    if (C.lo > A.lo || C.lo > B.lo || C.lo + C.nb < A.lo + A.nb || C.lo + C.nb < B.lo + B.nb) return MIMSEM_ERR_STATE;
    return each(c, (long long)nEl*C.nr*C.nb*nn, [=] __device__(long long x) {
        const int ij = (int)(x%nn); long long t = x/nn;
        const int cb = (int)(t%C.nb); t /= C.nb; const int r = (int)(t%C.nr), e = (int)(t/C.nr);
        const int d = C.lo + cb, col = r + d;
        double s = 0.0;
        if (col >= 0 && col < C.nc) {
            const int a = d - A.lo, b = d - B.lo;
            if (a >= 0 && a < A.nb) s += alpha*A.p[(((size_t)e*A.nr + r)*A.nb + a)*nn + ij];
            if (b >= 0 && b < B.nb) s += beta*B.p[(((size_t)e*B.nr + r)*B.nb + b)*nn + ij];
        }
        C.p[x] = s;
    });
}
// T = A^T
int band_transpose(mimsem_ctx* c, Band T, Band A) {
    const int n2 = c->es.n2e, nn = n2*n2, nEl = c->nEl;
    if (T.nr != A.nc || T.nc != A.nr || T.nb != A.nb || T.lo != -(A.lo + A.nb - 1)) return MIMSEM_ERR_STATE;
    return each(c, (long long)nEl*T.nr*T.nb*nn, [=] __device__(long long x) {
        const int ij = (int)(x%nn), ii = ij/n2, jj = ij%n2; long long t = x/nn;
        const int tb = (int)(t%T.nb); t /= T.nb; const int j = (int)(t%T.nr), e = (int)(t/T.nr);
        const int k = j + T.lo + tb;            // row of A
        double s = 0.0;
        if (k >= 0 && k < A.nr) {
            const int a = j - k - A.lo;
            if (a >= 0 && a < A.nb) s = A.p[(((size_t)e*A.nr + k)*A.nb + a)*nn + jj*n2 + ii];
        }
        T.p[x] = s;
    });
}
// y = beta*y + alpha * A x on the DPP row algebra: one task = block row (e, r), 16 lanes; lane a holds row a of each block of the row
// and element a of each input slice -- the product is N2 v_fmac_f64_dpp per block (the entry-per-thread version below re-read every
// block row through L1 for each output entry: 75 us per call, 13 calls per solve)
template <int N2>
__global__ __launch_bounds__(64) void k_band_mv_dpp(int nEl, Band A, const double* __restrict__ x, double* __restrict__ y, double alpha, double beta) {
    constexpr int nn = N2*N2;
    const int lane = threadIdx.x, a = lane%16;
    const long long task0 = (long long)blockIdx.x*4 + lane/16, ntask = (long long)nEl*A.nr;
    const bool live = task0 < ntask, act = live && a < N2;
    const long long task = live ? task0 : ntask - 1;
    const int e = (int)(task/A.nr), r = (int)(task%A.nr), aa = a < N2 ? a : N2 - 1;
    double s = 0.0;
    for (int b = 0; b < A.nb; b++) {
        const int col = r + A.lo + b;
        if (col < 0 || col >= A.nc) continue;                       // (uniform over the task's lanes)
        const double* m = A.p + (((size_t)e*A.nr + r)*A.nb + b)*nn + aa*N2;
        double row[N2];
#pragma unroll
        for (int j = 0; j < N2; j++) row[j] = m[j];
        const double xv = x[((size_t)e*A.nc + col)*N2 + aa];
        dpp::MatvecAcc<N2>::run(s, row, xv);
    }
    if (act) {
        const size_t o = ((size_t)e*A.nr + r)*N2 + a;
        y[o] = (beta == 0.0 ? 0.0 : beta*y[o]) + alpha*s;
    }
}
// y = beta*y + alpha * A x
int band_mv(mimsem_ctx* c, Band A, const double* x, double* y, double alpha, double beta) {
    const int n2 = c->es.n2e, nn = n2*n2, nEl = c->nEl;
    if ((n2 == 1 || n2 == 4 || n2 == 9 || n2 == 16) && !exp_env("MIMSEM_SCHUR3_BANDS") && (long long)nEl*A.nr > 0) {
        const unsigned grid = (unsigned)(((long long)nEl*A.nr + 3)/4);
        if (n2 == 1) hipLaunchKernelGGL((k_band_mv_dpp<1>), dim3(grid), dim3(64), 0, c->stream, nEl, A, x, y, alpha, beta);
        else if (n2 == 4) hipLaunchKernelGGL((k_band_mv_dpp<4>), dim3(grid), dim3(64), 0, c->stream, nEl, A, x, y, alpha, beta);
        else if (n2 == 9) hipLaunchKernelGGL((k_band_mv_dpp<9>), dim3(grid), dim3(64), 0, c->stream, nEl, A, x, y, alpha, beta);
        else hipLaunchKernelGGL((k_band_mv_dpp<16>), dim3(grid), dim3(64), 0, c->stream, nEl, A, x, y, alpha, beta);
        MIMSEM_HIP_TRY(hipGetLastError());
        return MIMSEM_OK;
    }
    return each(c, (long long)nEl*A.nr*n2, [=] __device__(long long i) {
        const int a = (int)(i%n2); long long t = i/n2; const int r = (int)(t%A.nr), e = (int)(t/A.nr);
        double s = 0.0;
        for (int b = 0; b < A.nb; b++) {
            const int col = r + A.lo + b;
            if (col < 0 || col >= A.nc) continue;
            const double* m = A.p + (((size_t)e*A.nr + r)*A.nb + b)*nn;
            const double* xv = x + ((size_t)e*A.nc + col)*n2;
            for (int k = 0; k < n2; k++) s += m[a*n2 + k]*xv[k];
        }
        y[i] = (beta == 0.0 ? 0.0 : beta*y[i]) + alpha*s;
    });
}
// V10 (nk x nm: -I at (k,k-1), +I at (k,k)) and V01 = -V10^T (nm x nk: -I at (i,i), +I at (i,i+1))  VertOps.cpp:134-163
int band_fill_incidence(mimsem_ctx* c, Band V, int is_v01) {
    const int n2 = c->es.n2e, nn = n2*n2, nEl = c->nEl;
    return each(c, (long long)nEl*V.nr*2*nn, [=] __device__(long long x) {
        const int ij = (int)(x%nn), ii = ij/n2, jj = ij%n2; long long t = x/nn;
        const int b = (int)(t%2); t /= 2; const int r = (int)(t%V.nr);
        const int col = r + V.lo + b;
        double v = 0.0;
        if (ii == jj && col >= 0 && col < V.nc) v = (b == 0) ? -1.0 : +1.0;
        (void)is_v01;
        V.p[x] = v;
    });
}

// block-pentadiagonal L (nk rows, lo = -2, nb = 5) -> block-tridiagonal with 2x2 super-blocks (size m = 2 n2),
// K = ceil(nk/2) super rows; a padding row (nk odd) carries the identity.
__global__ __launch_bounds__(256) void k_penta_to_tri(int nEl, int nk, int n2, int K, const double* __restrict__ L, double* __restrict__ T) {
    const int m = 2*n2, mm = m*m, nn = n2*n2;
    const long long x = (long long)blockIdx.x*256 + threadIdx.x;
    const long long per = (long long)K*3*mm;
    if (x >= (long long)nEl*per) return;
    const int e = (int)(x/per);
    long long t = x%per;
    const int ij = (int)(t%mm); t /= mm; const int w = (int)(t%3), Kr = (int)(t/3);
    const int I = ij/m, Jc = ij%m;
    const int r = 2*Kr + I/n2, cc = 2*(Kr + w - 1) + Jc/n2;     // block row / column in the pentadiagonal matrix
    const int ii = I%n2, jj = Jc%n2;
    double v = 0.0;
    if (r < nk) {
        const int b = cc - r + 2;
        if (cc >= 0 && cc < nk && b >= 0 && b < 5) v = L[(((size_t)e*nk + r)*5 + b)*nn + ii*n2 + jj];
    } else if (cc == r && ii == jj) v = 1.0;
    T[x] = v;
}

// the plan of the chain (col_workspace.hpp) and what its launches have done; `dpp`: the path the plan was carved for
struct Schur3 : mimsem::Schur3WS { bool dpp = false; bool Tm_done = false; };

// the launch of the three product kernels on the DPP row algebra (column_schur3_dpp.inc)
int launch_s3_chain(mimsem_ctx* c, Schur3& S, double hdt) {
    S3Args a{};
    a.nEl = c->nEl; a.nk = c->nk; a.hdt = hdt; a.gam = RD/CV;
    a.B = S.B.p; a.Binv = S.Mrhoinv.p; a.Npiinv = S.Npiinv.p; a.Ainv = S.Ainv.p; a.Muinv = S.Muinv.p; a.Cg = S.VBA.p; a.Cv = S.Cv.p;
    a.Brinv = S.Brinv.p; a.T = S.T.p; a.Rr = S.Rr.p; a.Brt = S.Brt.p; a.Brtinv = S.Brtinv.p; a.Bth = S.Bth.p;
    a.X = S.X.p; a.Nrt = S.Nrt.p; a.GN = S.GN.p; a.GG = S.GG.p; a.QM = S.QM.p; a.Drho = S.Drho.p; a.DDM = S.DDM.p; a.L = S.L.p;
    a.Tm = S.Tm; a.K = (c->nk + 1)/2; S.Tm_done = S.Tm != nullptr;
    return for_order<1, 4, 9, 16>(c->es.n2e, [&](auto N) { return launch_s3<N()>(c, a); });
}

int schur3_operator(mimsem_ctx* c, double dt, unsigned flags, const double* theta, const double* velz, const double* rho,
                    const double* rt, const double* pi, Schur3& S) {
    const double hdt = 0.5*dt;
    int rc;
    double *cq = S.cq, *tmpM = S.tmpM;
    const Band &B = S.B, &Ainv = S.Ainv, &V01 = S.V01, &V10 = S.V10, &VBA = S.VBA;
    const bool s3_dpp = S.dpp;
    if (s3_dpp && c->es.n <= 4 && !exp_env("MIMSEM_SCHUR3_WIDE_FACTORS")) {
        // orders 1..3: every diagonal factor block assembled / inverted on the row algebra (two launches), then the three product launches
        S3FactorArgs fa{};
        fill_newton_geo(c, fa.g);
        fa.rayleigh = (flags & MIMSEM_SCHUR3_NO_RAYLEIGH) ? 0 : 1; fa.ray_param = 0.5*dt*(4.0/120.0);     // RAYLEIGH, eul/VertSolve.cpp:32, :520
        fa.cv_from_velz = (flags & MIMSEM_SCHUR3_BOX_Q) ? 0 : 1;
        fa.theta = theta; fa.velz = velz; fa.rho = rho; fa.rt = rt; fa.pi = pi;
        fa.B = B.p; fa.Binv = S.Mrhoinv.p; fa.Npiinv = S.Npiinv.p; fa.Brinv = S.Brinv.p; fa.Brt = S.Brt.p; fa.Brtinv = S.Brtinv.p; fa.Bth = S.Bth.p;
        fa.Ainv = Ainv.p; fa.Muinv = S.Muinv.p; fa.T = S.T.p; fa.Rr = S.Rr.p; fa.Cg = VBA.p; fa.Cv = S.Cv.p;
        if ((rc = launch_s3_factors(c, fa))) return rc;
        return launch_s3_chain(c, S, hdt);
    }
    if ((rc = band_fill_incidence(c, V01, 1))) return rc;              // (V01 also carries the pressure gradient below)
    if (!s3_dpp && (rc = band_fill_incidence(c, V10, 0))) return rc;

    if (flags & MIMSEM_SCHUR3_NO_RAYLEIGH) {                                        // box flavour: RAYLEIGH undefined (box/VertSolve.cpp:30)
        if ((rc = colop_blocks_into(c, MIMSEM_V_LINEAR_INV, 0, nullptr, nullptr, S.Muinv.p, cq, tmpM))) return rc;
    } else {
        const double save = c->col_param;
        c->col_param = 0.5*dt*(4.0/120.0);                                          // RAYLEIGH, eul/VertSolve.cpp:32, :520
        rc = colop_blocks_into(c, MIMSEM_V_LINEAR_RAYLEIGH_INV, 0, nullptr, nullptr, S.Muinv.p, cq, tmpM);
        c->col_param = save;
        if (rc) return rc;
    }
    if ((rc = colop_blocks_into(c, MIMSEM_V_CONST, 0, nullptr, nullptr, B.p, cq, tmpM))) return rc;              // M_rt = VB  (:524, :527)
    if ((rc = colop_blocks_into(c, MIMSEM_V_CONST_INV, 0, nullptr, nullptr, S.Mrhoinv.p, cq, tmpM))) return rc;  // :525
    if ((rc = colop_blocks_into(c, MIMSEM_V_EOS_BLOCK_INV, 0, pi, nullptr, S.Npiinv.p, cq, tmpM))) return rc;     // :526
    if ((rc = colop_blocks_into(c, MIMSEM_V_LINEAR_INV, 0, nullptr, nullptr, Ainv.p, cq, tmpM))) return rc;       // :530
    // pressure gradient  tA2 = VA_inv V01 VB pi   (:528-531)
    if ((rc = band_mv(c, B, pi, S.tA, 1.0, 0.0))) return rc;
    if ((rc = band_mv(c, V01, S.tA, S.tB, 1.0, 0.0))) return rc;
    if ((rc = band_mv(c, Ainv, S.tB, S.tC, 1.0, 0.0))) return rc;
    // G_rt = 0.5dt VBA(grad)^T VB_inv(rho) VB   (:532-541)
    if ((rc = colop_blocks_into(c, MIMSEM_V_CONLIN_W, 0, S.tC, nullptr, VBA.p, cq, tmpM))) return rc;
    if (s3_dpp) {
        // round 2: the whole MatMatMult chain (:532-627) in three launches on the DPP row algebra (column_schur3_dpp.inc); the
        // banded products below (20 launches, each reading and writing whole bands) stay selectable with MIMSEM_SCHUR3_BANDS=1
        if ((rc = colop_blocks_into(c, MIMSEM_V_CONST_RHO_INV, 0, rho, nullptr, S.Brinv.p, cq, tmpM))) return rc;
        if ((rc = colop_blocks_into(c, MIMSEM_V_LINEAR_THETA, 0, theta, nullptr, S.T.p, cq, tmpM))) return rc;
        if ((rc = colop_blocks_into(c, MIMSEM_V_LINEAR_RT, MIMSEM_FLAG_VERT, rho, nullptr, S.Rr.p, cq, tmpM))) return rc;
        if ((rc = colop_blocks_into(c, MIMSEM_V_CONST_RHO, 0, rt, nullptr, S.Brt.p, cq, tmpM))) return rc;
        if ((rc = colop_blocks_into(c, MIMSEM_V_CONST_RHO_INV, 0, rt, nullptr, S.Brtinv.p, cq, tmpM))) return rc;
        if ((rc = colop_blocks_into(c, MIMSEM_V_CONST_THETA, 0, theta, nullptr, S.Bth.p, cq, tmpM))) return rc;
        if (!(flags & MIMSEM_SCHUR3_BOX_Q))
            if ((rc = colop_blocks_into(c, MIMSEM_V_CONLIN_W, 0, velz, nullptr, S.Cv.p, cq, tmpM))) return rc;
        return launch_s3_chain(c, S, hdt);
    }
    // the banded products: their intermediates are the plan's wide-path members
    const Band &VAB = S.VAB, &Brinv = S.Brinv, &t_a = S.t_a, &G_rt = S.G_rt, &DTV1 = S.DTV1, &AinvDTV1 = S.AinvDTV1, &T = S.T, &G_pi = S.G_pi,
               &Rr = S.Rr, &X = S.X, &DX = S.DX, &Brt = S.Brt, &D_rt = S.D_rt, &t_d = S.t_d, &Bth = S.Bth, &Q = S.Q, &GNN = S.GNN, &QMD = S.QMD,
               &DD = S.DD, &DGG = S.DGG;
    if ((rc = band_transpose(c, VAB, VBA))) return rc;
    if ((rc = colop_blocks_into(c, MIMSEM_V_CONST_RHO_INV, 0, rho, nullptr, Brinv.p, cq, tmpM))) return rc;
    if ((rc = band_mul(c, t_a, VAB, Brinv, 1.0))) return rc;
    if ((rc = band_mul(c, G_rt, t_a, B, hdt))) return rc;
    // G_pi = 0.5dt VA(theta) VA_inv V01 VB      (:543-555)
    if ((rc = band_mul(c, DTV1, V01, B, 1.0))) return rc;
    if ((rc = band_mul(c, AinvDTV1, Ainv, DTV1, 1.0))) return rc;
    if ((rc = colop_blocks_into(c, MIMSEM_V_LINEAR_THETA, 0, theta, nullptr, T.p, cq, tmpM))) return rc;
    if ((rc = band_mul(c, G_pi, T, AinvDTV1, hdt))) return rc;
    // D_rho = 0.5dt VB V10 VA_inv VA(rho)       (:557-569)
    if ((rc = colop_blocks_into(c, MIMSEM_V_LINEAR_RT, MIMSEM_FLAG_VERT, rho, nullptr, Rr.p, cq, tmpM))) return rc;
    if ((rc = band_mul(c, X, Ainv, Rr, 1.0))) return rc;
    if ((rc = band_mul(c, DX, V10, X, 1.0))) return rc;
    if ((rc = band_mul(c, S.Drho, B, DX, hdt))) return rc;
    // D_rt = 0.5dt VB(rt) V10                   (:571-575)
    if ((rc = colop_blocks_into(c, MIMSEM_V_CONST_RHO, 0, rt, nullptr, Brt.p, cq, tmpM))) return rc;
    if ((rc = band_mul(c, D_rt, Brt, V10, hdt))) return rc;
    // N_rt = -R/cv VB VB_inv(rt) VB             (:577-585)
    if ((rc = colop_blocks_into(c, MIMSEM_V_CONST_RHO_INV, 0, rt, nullptr, Brt.p, cq, tmpM))) return rc;   // Brt now holds the inverse
    if ((rc = band_mul(c, t_d, Brt, B, 1.0))) return rc;
    if ((rc = band_mul(c, S.Nrt, B, t_d, -1.0*RD/CV))) return rc;
    // Q_rt_rho = 0.5dt VBA(velz) VA_inv V01 VB(theta)   (:587-599)
    if ((rc = colop_blocks_into(c, MIMSEM_V_CONST_THETA, 0, theta, nullptr, Bth.p, cq, tmpM))) return rc;
    if ((rc = band_mul(c, DTV1, V01, Bth, 1.0))) return rc;
    if ((rc = band_mul(c, AinvDTV1, Ainv, DTV1, 1.0))) return rc;
    // eul re-assembles VBA with velz (:597); the box twin does not and multiplies by VBA(pressure gradient) (box/VertSolve.cpp:978-981)
    if (!(flags & MIMSEM_SCHUR3_BOX_Q))
        if ((rc = colop_blocks_into(c, MIMSEM_V_CONLIN_W, 0, velz, nullptr, VBA.p, cq, tmpM))) return rc;
    if ((rc = band_mul(c, Q, VBA, AinvDTV1, hdt))) return rc;
    // products of the Schur complement           (:601-627)
    if ((rc = band_mul(c, S.QM, Q, S.Mrhoinv, 1.0))) return rc;
    if ((rc = band_mul(c, S.GN, G_pi, S.Npiinv, 1.0))) return rc;
    if ((rc = band_mul(c, GNN, S.GN, S.Nrt, 1.0))) return rc;
    if ((rc = band_lincomb(c, S.GG, -1.0, GNN, 1.0, G_rt))) return rc;                       // MatAYPX(Y, -1, G_rt)
    if ((rc = band_mul(c, QMD, S.QM, S.Drho, 1.0))) return rc;
    if ((rc = band_lincomb(c, DD, -1.0, QMD, 1.0, D_rt))) return rc;
    if ((rc = band_mul(c, S.DDM, DD, S.Muinv, 1.0))) return rc;
    if ((rc = band_mul(c, DGG, S.DDM, S.GG, 1.0))) return rc;
    if ((rc = band_lincomb(c, S.L, -1.0, DGG, 1.0, S.Mrt))) return rc;
    return MIMSEM_OK;
}

}  // namespace

extern "C" {

int mimsem_colop_blocks_ex(mimsem_ctx* c, int colop, unsigned flags, double param, const double* f1, const double* f2,
                           const double* uh, long long uhs, double* out) {
    if (!c) return MIMSEM_ERR_ARG;
    c->col_param = param; c->col_uh = uh; c->col_uhs = uhs;
    const int rc = mimsem_colop_blocks(c, colop, flags, f1, f2, out);
    c->col_param = 0.0; c->col_uh = nullptr; c->col_uhs = 0;
    return rc;
}

int mimsem_colop_apply_ex(mimsem_ctx* c, int colop, unsigned flags, int transpose, double param,
                          const double* f1, const double* f2, const double* uh, long long uhs,
                          const double* x, double* y) {
    if (!c) return MIMSEM_ERR_ARG;
    c->col_param = param; c->col_uh = uh; c->col_uhs = uhs;
    const int rc = mimsem_colop_apply(c, colop, flags, transpose, f1, f2, x, y);
    c->col_param = 0.0; c->col_uh = nullptr; c->col_uhs = 0;
    return rc;
}

// C1: the vertical incidence matrices of VertOps::vertOps (eul/VertOps.cpp:134-182) applied to every column:
// which 0 = V10 ((nk-1) interfaces -> nk levels), 1 = V01 = -V10^T (nk -> nk-1), 2 = V10_full (nk+1 -> nk).  Signs only: bit-exact.
int mimsem_column_incidence(mimsem_ctx* c, int which, const double* x, double* y) {
    if (!c || !x || !y || which < 0 || which > 2) return MIMSEM_ERR_ARG;
    const int nk = c->nk, n2 = c->es.n2e, nEl = c->nEl;
    const int nx = which == 0 ? nk - 1 : (which == 1 ? nk : nk + 1), ny = which == 1 ? nk - 1 : nk;
    return each(c, (long long)nEl*ny*n2, [=] __device__(long long i) {
        const int a = (int)(i%n2); long long t = i/n2; const int r = (int)(t%ny), e = (int)(t/ny);
        const double* xe = x + (size_t)e*nx*n2 + a;
        double s = 0.0;
        if (which == 0) { if (r > 0) s -= xe[(size_t)(r - 1)*n2]; if (r < nk - 1) s += xe[(size_t)r*n2]; }
        else s = -xe[(size_t)r*n2] + xe[(size_t)(r + 1)*n2];      // V01 row i: -x_i + x_{i+1} ; V10_full row k: -x_k + x_{k+1}
        y[i] = s;
    });
}

// diagTheta_up eul/VertSolve.cpp:354-384: VA2_up(rho, u) theta = VAB2_up(u) rt on the nk+1 interfaces (VA2 block diagonal)
int mimsem_column_diag_theta_up(mimsem_ctx* c, double dt, const double* rho, const double* rt,
                                const double* uh, long long uhs, double* theta) {
    if (!c || !rho || !rt || !uh || !theta) return MIMSEM_ERR_ARG;
    const int nk = c->nk, n2 = c->es.n2e, nn = n2*n2, nEl = c->nEl;
    mimsem::ColopWS w;
    int rc = plan_col(c, w, true);
    if (rc) return rc;
    double *cq = w.cq, *tmpM = w.tmpM, *M = w.M, *frt = w.frt;
    c->col_param = dt; c->col_uh = uh; c->col_uhs = uhs;
    rc = colop_blocks_into(c, MIMSEM_V_LINCON2_UP, 0, nullptr, nullptr, M, cq, tmpM);
    if (!rc) rc = stored_apply(c, MIMSEM_V_LINCON2_UP, 0, M, rt, frt);
    if (!rc) rc = colop_blocks_into(c, MIMSEM_V_LINEAR_RHO2_UP, 0, rho, nullptr, M, cq, tmpM);
    c->col_param = 0.0; c->col_uh = nullptr; c->col_uhs = 0;
    if (rc) return rc;
    if ((rc = mimsem_block_inverse_inplace(c, (long long)nEl*(nk + 1), n2, M))) return rc;
    return stored_apply(c, MIMSEM_V_LINEAR_RHO2_UP, 0, M, frt, theta);
}

// AssembleTempForcing_HS eul/VertOps.cpp:1563-1633.  lat: latitude at the quadrature points [nEl][mp12] (Geom::s[..][1])
int mimsem_column_temp_forcing_hs(mimsem_ctx* c, const double* lat, const double* exner, const double* theta,
                                  const double* rho, double* out) {
    if (!c || !lat || !exner || !theta || !rho || !out) return MIMSEM_ERR_ARG;
    const CG g = make_cg(c);
    const int nk = c->nk;
    mimsem::QuadWS w;
    int rc = plan_col(c, w);
    if (rc) return rc;
    double* rq = w.q;
    if ((rc = each(c, (long long)c->nEl*nk*g.mp12, [=] __device__(long long i) {
        const int q = (int)(i%g.mp12); long long t = i/g.mp12;
        const int k = (int)(t%nk), e = (int)(t/nk);
        const double det = g.det[(size_t)e*g.mp12 + q];
        double _e = wint(g, exner, nk, e, k, q), _tb = wint(g, theta, nk + 1, e, k, q), _tt = wint(g, theta, nk + 1, e, k + 1, q);
        double _r = wint(g, rho, nk, e, k, q), _es = wint(g, exner, nk, e, 0, q);
        _e /= (det*g_th(g, e, k, q)); _tb /= det; _tt /= det; _r /= (det*g_th(g, e, k, q)); _es /= (det*g_th(g, e, 0, q));
        // compute_k_T :1563-1587
        const double phi = lat[(size_t)e*g.mp12 + q], th = 0.5*(_tb + _tt);
        const double p = pow(_e/CP, CP/RD), ps = pow(_es/CP, CP/RD), sigma = p/ps, sigma_b = 0.7;
        const double k_a = 2.8935185185185185e-07, k_s = 2.8935185185185184e-06;
        double k_t = 0.0;
        double t_eq = 315.0 - 60.0*sin(phi)*sin(phi) - 10.0*log(p)*cos(phi)*cos(phi);
        t_eq *= pow(p, RD/CP);
        if (t_eq < 200.0) t_eq = 200.0;
        const double theta_eq = t_eq*pow(1.0/p, RD/CP);
        if (sigma > sigma_b) { k_t = (k_s - k_a)*(sigma - sigma_b)/(1.0 - sigma_b); k_t *= pow(cos(phi), 4.0); }
        k_t += k_a;
        rq[i] = g_Q(g, q)*VSCALE*_r*(k_t*(th - theta_eq));
    }))) return rc;
    return each(c, (long long)c->nEl*nk*g.n2, [=] __device__(long long i) {
        const int j = (int)(i%g.n2); const long long ek = i/g.n2;
        const double* r = rq + ek*g.mp12;
        double s = 0.0;
        for (int q = 0; q < g.mp12; q++) s += g_W(g, q, j)*r[q];
        out[i] = s;
    });
}

// solve_schur_column_3 eul/VertSolve.cpp:504-675 for every column at once; F_* are updated in place as the reference does.
// L_out (optional): the block-pentadiagonal Schur complement [nEl][nk][5][n2][n2] (block column = row - 2 + b).
int mimsem_column_solve_schur_3(mimsem_ctx* c, double dt, unsigned flags,
        const double* theta, const double* velz, const double* rho, const double* rt, const double* pi,
        double* F_u, double* F_rho, double* F_rt, double* F_pi,
        double* d_u, double* d_rho, double* d_rt, double* d_pi, double* L_out) {
    if (!c || !theta || !velz || !rho || !rt || !pi || !F_u || !F_rho || !F_rt || !F_pi || !d_u || !d_rho || !d_rt || !d_pi)
        return MIMSEM_ERR_ARG;
    if (c->nk < 4) return MIMSEM_ERR_ARG;
    c->colstat_valid = false;
    if (s3_fused_supported(c))        // orders 1..4: three launches (column_schur3_sweep.inc); MIMSEM_SCHUR3_CHAIN=1 keeps round 2's chain below
        return s3_fused_solve(c, dt, flags, theta, velz, rho, rt, pi, F_u, F_rho, F_rt, F_pi, d_u, d_rho, d_rt, d_pi, L_out);
    const int nk = c->nk, n2 = c->es.n2e, nn = n2*n2, nEl = c->nEl;
    const int m = 2*n2, K = (nk + 1)/2;
    if ((size_t)(3*m*m + 2*m)*sizeof(double) > 160*1024) return MIMSEM_ERR_UNSUPPORTED;     // p = 7
    // the path of the call, known on entry: the bands on the DPP row algebra or by banded products; the five bands eliminated directly or
    // through the 2x2 super-blocks, whose row-per-lane sweep (2x2 / 3x3 faces, m = 8 / 18) keeps its factors
    const bool dpp_sizes = n2 == 1 || n2 == 4 || n2 == 9 || n2 == 16;
    const bool penta = dpp_sizes && !getenv("MIMSEM_SCHUR3_SUPERBLOCKS");
    const bool rows = (m == 8 || m == 18) && !exp_env("MIMSEM_THOMAS_WG");
    Schur3 S;
    S.dpp = dpp_sizes && !exp_env("MIMSEM_SCHUR3_BANDS");
    int rc = plan_col(c, S, S.dpp, !(flags & MIMSEM_SCHUR3_BOX_Q), penta, rows);
    if (rc) return rc;
    if ((rc = schur3_operator(c, dt, flags, theta, velz, rho, rt, pi, S))) return rc;
    if (L_out) MIMSEM_HIP_TRY(hipMemcpyAsync(L_out, S.L.p, (size_t)nEl*nk*5*nn*sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    // residual updates (:632-639)
    if ((rc = band_mv(c, S.QM, F_rho, F_rt, -1.0, 1.0))) return rc;
    if ((rc = band_mv(c, S.GN, F_pi, F_u, -1.0, 1.0))) return rc;
    if ((rc = band_mv(c, S.DDM, F_u, F_rt, -1.0, 1.0))) return rc;
    // F_rt = -F_rt ; L d_rt = F_rt   (:652-653)
    if (penta) {
        // round 4: the five bands eliminated directly on the DPP rows (column_penta.inc), refinement and status in the same launch
        if ((rc = each(c, (long long)nEl*nk*n2, [=] __device__(long long i) { F_rt[i] *= -1.0; }))) return rc;
        if ((rc = launch_penta_dpp(c, refine_steps(), S.L.p, true, F_rt, d_rt, S.Fac, S.yws))) return rc;
        if ((rc = launch_band_lu_flagged(c, 2, S.L.p, true, F_rt, d_rt))) return rc;
        c->colstat_valid = true;
        if ((rc = band_mv(c, S.GG, d_rt, F_u, -1.0, -1.0))) return rc;
        if ((rc = band_mv(c, S.Muinv, F_u, d_u, 1.0, 0.0))) return rc;
        if ((rc = band_mv(c, S.Nrt, d_rt, F_pi, -1.0, -1.0))) return rc;
        if ((rc = band_mv(c, S.Npiinv, F_pi, d_pi, 1.0, 0.0))) return rc;
        if ((rc = band_mv(c, S.Drho, d_u, F_rho, -1.0, -1.0))) return rc;
        return band_mv(c, S.Mrhoinv, F_rho, d_rho, 1.0, 0.0);
    }
    // (rounds 1-3, kept for orders >= 5 and as the A/B: MIMSEM_SCHUR3_SUPERBLOCKS=1) through the 2x2 super-block tridiagonal form
    // 2x2 / 3x3 faces (m = 8 / 18): the row-per-lane sweep of k_block_thomas_rows (16 / 32 lanes per column) keeps its factors, and the
    // refinement step is substitution only; other orders use the workgroup-per-column kernel twice
    double *Tm = S.Tm, *fpad = S.fpad, *dpad = S.dpad, *Gws = S.Gws, *yws = S.yws, *Dinv = S.Dinv;
    auto sweep = [&](bool first) -> int {
        if (rows && first) {
            if (m == 8) hipLaunchKernelGGL((k_block_thomas_rows<8, 16>), dim3((unsigned)((nEl + 3)/4)), dim3(64), 0, c->stream, nEl, K, Tm, fpad, dpad, Gws, yws, Dinv);
            else hipLaunchKernelGGL((k_block_thomas_rows<18, 32>), dim3((unsigned)((nEl + 1)/2)), dim3(64), 0, c->stream, nEl, K, Tm, fpad, dpad, Gws, yws, Dinv);
        } else if (rows) {
            const int cpw = 64/m;
            const size_t lds = (size_t)cpw*K*m*sizeof(double);
            const unsigned grid = (unsigned)((nEl + cpw - 1)/cpw);
            if (m == 8) hipLaunchKernelGGL((k_block_thomas_resolve<8>), dim3(grid), dim3(64), lds, c->stream, nEl, K, Tm, Dinv, Gws, fpad, dpad);
            else hipLaunchKernelGGL((k_block_thomas_resolve<18>), dim3(grid), dim3(64), lds, c->stream, nEl, K, Tm, Dinv, Gws, fpad, dpad);
        } else {
            const int mm = m*m, nt = std::min(256, ((mm + 63)/64)*64);
            const size_t lds = (size_t)(3*mm + 2*m)*sizeof(double);
            if (lds > 64*1024)
                MIMSEM_HIP_TRY(hipFuncSetAttribute((const void*)k_block_thomas, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_block_thomas, dim3(nEl), dim3(nt), lds, c->stream, K, m, Tm, fpad, dpad, Gws, yws);
        }
        MIMSEM_HIP_TRY(hipGetLastError());
        return MIMSEM_OK;
    };
    if (!S.Tm_done) {
        const long long tot = (long long)nEl*K*3*m*m;
        hipLaunchKernelGGL(k_penta_to_tri, dim3((unsigned)((tot + 255)/256)), dim3(256), 0, c->stream, nEl, nk, n2, K, S.L.p, Tm);
        MIMSEM_HIP_TRY(hipGetLastError());
    }
    if ((rc = each(c, (long long)nEl*K*m, [=] __device__(long long i) {
        const int a = (int)(i%(K*m)), e = (int)(i/(K*m));
        double v = 0.0;
        if (a < nk*n2) { double* f = F_rt + (size_t)e*nk*n2 + a; *f *= -1.0; v = *f; }
        fpad[i] = v;
    }))) return rc;
    if ((rc = sweep(true))) return rc;
    if ((rc = each(c, (long long)nEl*nk*n2, [=] __device__(long long i) {
        const int a = (int)(i%(nk*n2)), e = (int)(i/(nk*n2));
        d_rt[i] = dpad[(size_t)e*K*m + a];
    }))) return rc;
    if (refine_wide()) {
        // one step of iterative refinement (see block_thomas_refined): r = F_rt - L d_rt, d_rt += solve(r)
        double* rr = S.rr;
        MIMSEM_HIP_TRY(hipMemcpyAsync(rr, F_rt, (size_t)nEl*nk*n2*sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        if ((rc = band_mv(c, S.L, d_rt, rr, -1.0, 1.0))) return rc;
        if ((rc = each(c, (long long)nEl*K*m, [=] __device__(long long i) {
            const int a = (int)(i%(K*m)), e = (int)(i/(K*m));
            fpad[i] = (a < nk*n2) ? rr[(size_t)e*nk*n2 + a] : 0.0;
        }))) return rc;
        if ((rc = sweep(false))) return rc;
        if ((rc = each(c, (long long)nEl*nk*n2, [=] __device__(long long i) {
            const int a = (int)(i%(nk*n2)), e = (int)(i/(nk*n2));
            d_rt[i] += dpad[(size_t)e*K*m + a];
        }))) return rc;
    }
    // back substitution (:656-669)
    // (F <- -(F + B d) as ONE product with alpha = beta = -1: the same bits as the sum followed by a negation, three launches fewer)
    if ((rc = band_mv(c, S.GG, d_rt, F_u, -1.0, -1.0))) return rc;
    if ((rc = band_mv(c, S.Muinv, F_u, d_u, 1.0, 0.0))) return rc;
    if ((rc = band_mv(c, S.Nrt, d_rt, F_pi, -1.0, -1.0))) return rc;
    if ((rc = band_mv(c, S.Npiinv, F_pi, d_pi, 1.0, 0.0))) return rc;
    if ((rc = band_mv(c, S.Drho, d_u, F_rho, -1.0, -1.0))) return rc;
    return band_mv(c, S.Mrhoinv, F_rho, d_rho, 1.0, 0.0);
}

}  // extern "C"
