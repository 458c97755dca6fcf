// column_schur3_dpp.inc -- included by column_hs.inc (same translation unit).
//
// The MatMatMult chain of VertSolve::solve_schur_column_3 (eul/VertSolve.cpp:528-627; box twin box/VertSolve.cpp:879-1058) in three
// launches on the DPP row algebra of column_dpp.inc.  Round 1 formed it as 20 banded products, each reading and writing whole bands
// (k_band_mul: 191 us per product, memory-bound: 3.8 of the 7.2 ms of a solve); here a task holds one block row (16 lanes, row-per-
// lane) and forms its products in registers:
//   k_s3_ifc  (column, interface i): G_rt(i,.), G_pi(i,.) N_pi^-1 = GN(i,.), GG(i,.) = G_rt - GN N_rt, X_i = A^-1 VA(rho), N_rt
//   k_s3_lev  (column, level k):     Q(k,.) -> QM = Q M_rho^-1, D_rho(k,.), DD = D_rt - QM D_rho, DDM = DD M_u^-1
//   k_s3_row  (column, level k):     L(k,.) = M_rt - DDM GG   (block-pentadiagonal)
// The diagonal factor blocks (VB, VB^-1, VA^-1, ...) still come from the coefficient + inverse passes (colop_blocks_into).

namespace {

struct S3Args {
    int nEl, nk; double hdt, gam;
    // inputs: block diagonals [nEl][ns][nn]; Cg / Cv are CONLIN_W bands stored [nEl][nk][2][nn]
    const double *B, *Binv, *Npiinv, *Ainv, *Muinv, *Cg, *Cv, *Brinv, *T, *Rr, *Brt, *Brtinv, *Bth;
    // outputs
    double *X, *Nrt, *GN, *GG, *QM, *Drho, *DDM, *L;
    // optional: L again as the block-tridiagonal matrix of 2x2 super-blocks the Thomas sweep works on, [nEl][K][3][(2 n2)^2], K = ceil(nk/2)
    double* Tm; int K;
};

template <int N2>
struct S3 {
    static constexpr int nn = N2*N2;
    __device__ static void load(double (&M)[N2], const double* p, int rr) {
#pragma unroll
        for (int j = 0; j < N2; j++) M[j] = p[rr*N2 + j];
    }
    __device__ static void store(double* p, const double (&M)[N2], int r, bool act) {
        if (!act) return;
#pragma unroll
        for (int j = 0; j < N2; j++) p[r*N2 + j] = M[j];
    }
    __device__ static void zero(double* p, int r, bool act) {
        if (!act) return;
#pragma unroll
        for (int j = 0; j < N2; j++) p[r*N2 + j] = 0.0;
    }
    __device__ static void mul(double (&C)[N2], const double (&A)[N2], const double (&Bm)[N2]) {
#pragma unroll
        for (int j = 0; j < N2; j++) C[j] = 0.0;
        dpp::MulAcc<N2>::run(C, A, Bm);
    }
    __device__ static void mul_add(double (&C)[N2], const double (&A)[N2], const double (&Bm)[N2]) { dpp::MulAcc<N2>::run(C, A, Bm); }
};

template <int N2>
__global__ __launch_bounds__(64) void k_s3_ifc(S3Args a) {
    using S = S3<N2>; constexpr int nn = S::nn;
    const int lane = threadIdx.x, r = lane%16, nk = a.nk, nm = nk - 1;
    const long long task0 = (long long)blockIdx.x*4 + lane/16, ntask = (long long)a.nEl*nm;
    const bool live = task0 < ntask, act = live && r < N2;
    const long long task = live ? task0 : ntask - 1;
    const int e = (int)(task/nm), i = (int)(task%nm), rr = r < N2 ? r : N2 - 1;
    double C[N2], Ai[N2], T[N2], t1[N2], t2[N2], M[N2];
    S::load(C, a.Cg + (((size_t)e*nk + i)*2 + 1)*nn, rr);          // VBA(grad pi) block of interface i (stored (k=i, w=1)); VAB(i,.) = its transpose = itself
    S::load(Ai, a.Ainv + ((size_t)e*nm + i)*nn, rr);
    S::load(T, a.T + ((size_t)e*nm + i)*nn, rr);
    {   // X_i = VA_inv VA(rho)   (:563-565)
        S::load(M, a.Rr + ((size_t)e*nm + i)*nn, rr);
        S::mul(t1, Ai, M);
        S::store(a.X + ((size_t)e*nm + i)*nn, t1, r, act);
    }
    double TA[N2];
    S::mul(TA, T, Ai);                                                // VA(theta) VA_inv
#pragma unroll 1
    for (int w = 0; w < 2; w++) {
        const int k = i + w;
        const size_t lo = ((size_t)e*nk + k)*nn, bo = (((size_t)e*nm + i)*2 + w)*nn;
        double Bk[N2], Grt[N2], GNw[N2], Nrt[N2];
        S::load(Bk, a.B + lo, rr);
        // G_rt(i,k) = h C_i VB_inv(rho)_k VB_k     (:532-541)
        S::load(M, a.Brinv + lo, rr);
        S::mul(t1, C, M);
        S::mul(Grt, t1, Bk);
        // G_pi(i,k) = h VA(theta) VA_inv (V01 VB)(i,k),  (V01 VB)(i,i) = -VB_i, (i,i+1) = +VB_{i+1}   (:543-555);  GN = G_pi N_pi^-1  (:603)
        S::mul(t1, TA, Bk);
        S::load(M, a.Npiinv + lo, rr);
        S::mul(GNw, t1, M);
        const double sg = (w == 0 ? -1.0 : 1.0)*a.hdt;
#pragma unroll
        for (int j = 0; j < N2; j++) GNw[j] *= sg;
        // N_rt,k = -R/cv VB VB_inv(rt) VB   (:577-585)
        S::load(M, a.Brtinv + lo, rr);
        S::mul(t1, M, Bk);
        S::mul(Nrt, Bk, t1);
#pragma unroll
        for (int j = 0; j < N2; j++) Nrt[j] *= -1.0*a.gam;
        if (w == 0 || i == nm - 1) S::store(a.Nrt + lo, Nrt, r, act);
        // GG(i,k) = G_rt - GN N_rt   (:604-606)
        S::mul(t2, GNw, Nrt);
#pragma unroll
        for (int j = 0; j < N2; j++) t2[j] = -1.0*t2[j] + a.hdt*Grt[j];
        S::store(a.GN + bo, GNw, r, act);
        S::store(a.GG + bo, t2, r, act);
    }
}

template <int N2>
__global__ __launch_bounds__(64) void k_s3_lev(S3Args a) {
    using S = S3<N2>; constexpr int nn = S::nn;
    const int lane = threadIdx.x, r = lane%16, nk = a.nk, nm = nk - 1;
    const long long task0 = (long long)blockIdx.x*4 + lane/16, ntask = (long long)a.nEl*nk;
    const bool live = task0 < ntask, act = live && r < N2;
    const long long task = live ? task0 : ntask - 1;
    const int e = (int)(task/nk), k = (int)(task%nk), rr = r < N2 ? r : N2 - 1;
    const bool lo = k > 0, hi = k < nk - 1;
    const double h = a.hdt;
    double Q[3][N2], A1[N2], A2[N2], M[N2], t1[N2];
    // Q(k,.) = h VBA(v) VA_inv V01 VB(theta):  Q(k,k') = h sum_{i in {k-1,k}} C^v_i VA_inv_i (V01 Bth)(i,k')      (:587-599)
#pragma unroll
    for (int b = 0; b < 3; b++)
#pragma unroll
        for (int j = 0; j < N2; j++) Q[b][j] = 0.0;
    if (lo) {
        double Cm[N2];
        S::load(Cm, a.Cv + (((size_t)e*nk + k)*2 + 0)*nn, rr);       // VBA(k,k-1)
        S::load(M, a.Ainv + ((size_t)e*nm + k - 1)*nn, rr);
        S::mul(A1, Cm, M);
        S::load(M, a.Bth + ((size_t)e*nk + k - 1)*nn, rr);
        S::mul(t1, A1, M);
#pragma unroll
        for (int j = 0; j < N2; j++) Q[0][j] = -h*t1[j];
        S::load(M, a.Bth + ((size_t)e*nk + k)*nn, rr);
        S::mul(t1, A1, M);
#pragma unroll
        for (int j = 0; j < N2; j++) Q[1][j] = h*t1[j];
    }
    if (hi) {
        double Cm[N2];
        S::load(Cm, a.Cv + (((size_t)e*nk + k)*2 + 1)*nn, rr);       // VBA(k,k)
        S::load(M, a.Ainv + ((size_t)e*nm + k)*nn, rr);
        S::mul(A2, Cm, M);
        S::load(M, a.Bth + ((size_t)e*nk + k)*nn, rr);
        S::mul(t1, A2, M);
#pragma unroll
        for (int j = 0; j < N2; j++) Q[1][j] -= h*t1[j];
        S::load(M, a.Bth + ((size_t)e*nk + k + 1)*nn, rr);
        S::mul(t1, A2, M);
#pragma unroll
        for (int j = 0; j < N2; j++) Q[2][j] = h*t1[j];
    }
    // QM = Q M_rho^-1 (:602); QB = QM VB (the left factor of QM D_rho, D_rho = h VB V10 X)
    double QB[3][N2];
#pragma unroll
    for (int b = 0; b < 3; b++) {
        const int kp = k - 1 + b;
        double* out = a.QM + (((size_t)e*nk + k)*3 + b)*nn;
        if (kp < 0 || kp >= nk) {
            S::zero(out, r, act);
#pragma unroll
            for (int j = 0; j < N2; j++) QB[b][j] = 0.0;
            continue;
        }
        S::load(M, a.Binv + ((size_t)e*nk + kp)*nn, rr);
        S::mul(t1, Q[b], M);
        S::store(out, t1, r, act);
        S::load(M, a.B + ((size_t)e*nk + kp)*nn, rr);
        S::mul(QB[b], t1, M);
    }
    // D_rho(k,k-1) = -h VB_k X_{k-1},  D_rho(k,k) = +h VB_k X_k        (:557-569)
    double Bk[N2];
    S::load(Bk, a.B + ((size_t)e*nk + k)*nn, rr);
#pragma unroll 1
    for (int b = 0; b < 2; b++) {
        const int i = k - 1 + b;
        double* out = a.Drho + (((size_t)e*nk + k)*2 + b)*nn;
        if (i < 0 || i >= nm) { S::zero(out, r, act); continue; }
        S::load(M, a.X + ((size_t)e*nm + i)*nn, rr);
        S::mul(t1, Bk, M);
        const double sg = (b == 0 ? -h : h);
#pragma unroll
        for (int j = 0; j < N2; j++) t1[j] *= sg;
        S::store(out, t1, r, act);
    }
    // DDM(k,i) = (D_rt(k,i) - (QM D_rho)(k,i)) M_u^-1_i,  i = k-2 .. k+1;   (QM D_rho)(k,i) = h (QB(k,i) - QB(k,i+1)) X_i    (:571-575, :607-613)
    double Brt[N2];
    S::load(Brt, a.Brt + ((size_t)e*nk + k)*nn, rr);
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int i = k - 2 + b;
        double* out = a.DDM + (((size_t)e*nk + k)*4 + b)*nn;
        if (i < 0 || i >= nm) { S::zero(out, r, act); continue; }
        // QB(k,i) sits at band slot i-(k-1) = b-1, QB(k,i+1) at b
        double d[N2];
#pragma unroll
        for (int j = 0; j < N2; j++) d[j] = (b >= 1 ? QB[b >= 1 ? b - 1 : 0][j] : 0.0) - (b <= 2 ? QB[b <= 2 ? b : 2][j] : 0.0);
        S::load(M, a.X + ((size_t)e*nm + i)*nn, rr);
        S::mul(t1, d, M);
#pragma unroll
        for (int j = 0; j < N2; j++) t1[j] = -h*t1[j] + (b == 1 ? -h*Brt[j] : (b == 2 ? h*Brt[j] : 0.0));
        S::load(M, a.Muinv + ((size_t)e*nm + i)*nn, rr);
        double o[N2];
        S::mul(o, t1, M);
        S::store(out, o, r, act);
    }
}

template <int N2>
__global__ __launch_bounds__(64) void k_s3_row(S3Args a) {
    using S = S3<N2>; constexpr int nn = S::nn;
    const int lane = threadIdx.x, r = lane%16, nk = a.nk, nm = nk - 1;
    const long long task0 = (long long)blockIdx.x*4 + lane/16, ntask = (long long)a.nEl*nk;
    const bool live = task0 < ntask, act = live && r < N2;
    const long long task = live ? task0 : ntask - 1;
    const int e = (int)(task/nk), k = (int)(task%nk), rr = r < N2 ? r : N2 - 1;
    // L(k,k'') = M_rt delta - sum_i DDM(k,i) GG(i,k''),  i = k-2..k+1, k'' in {i, i+1}      (:614-627); band slot of k'' is k''-(k-2)
    double Lb[5][N2], D[N2], G[N2];
#pragma unroll
    for (int b = 0; b < 5; b++)
#pragma unroll
        for (int j = 0; j < N2; j++) Lb[b][j] = 0.0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int i = k - 2 + b;
        if (i < 0 || i >= nm) continue;                                  // (uniform over the task's 16 lanes)
        S::load(D, a.DDM + (((size_t)e*nk + k)*4 + b)*nn, rr);
        S::load(G, a.GG + (((size_t)e*nm + i)*2 + 0)*nn, rr);
        S::mul_add(Lb[b], D, G);                                         // column k'' = i     -> slot b
        S::load(G, a.GG + (((size_t)e*nm + i)*2 + 1)*nn, rr);
        S::mul_add(Lb[b + 1], D, G);                                     // column k'' = i + 1 -> slot b + 1
    }
    double Bk[N2];
    S::load(Bk, a.B + ((size_t)e*nk + k)*nn, rr);
    constexpr int m2 = 2*N2, mm = m2*m2;
    const int Kr = k/2, Ih = k%2;
    double* Trow = a.Tm ? a.Tm + ((size_t)e*a.K + Kr)*3*mm + (size_t)(Ih*N2 + rr)*m2 : nullptr;     // my row of the super-row's three super-blocks
#pragma unroll
    for (int b = 0; b < 5; b++) {
        const int col = k - 2 + b;
        double o[N2];
#pragma unroll
        for (int j = 0; j < N2; j++) o[j] = (col >= 0 && col < nk) ? (-1.0*Lb[b][j] + (b == 2 ? Bk[j] : 0.0)) : 0.0;
        S::store(a.L + (((size_t)e*nk + k)*5 + b)*nn, o, r, act);
        if (Trow && act) {
            const int cc = col + 2*a.K;                                  // (shifted positive for the division)
            const int w = cc/2 - a.K - Kr + 1, Jh = cc%2;
            double* t = Trow + (size_t)w*mm + Jh*N2;
#pragma unroll
            for (int j = 0; j < N2; j++) t[j] = o[j];
        }
    }
    if (Trow && act) {
        // the one sub-block of my row outside the five bands: (w = 2, right half) for even k, (w = 0, left half) for odd k
        double* t = Trow + (size_t)(Ih ? 0 : 2)*mm + (Ih ? 0 : N2);
#pragma unroll
        for (int j = 0; j < N2; j++) t[j] = 0.0;
        if ((nk & 1) && k == nk - 1) {                                   // odd nk: the padding row below me carries the identity
            double* pr = a.Tm + ((size_t)e*a.K + Kr)*3*mm + (size_t)(N2 + rr)*m2;
#pragma unroll
            for (int w = 0; w < 3; w++)
#pragma unroll
                for (int j = 0; j < m2; j++) pr[(size_t)w*mm + j] = (w == 1 && j == N2 + rr) ? 1.0 : 0.0;
        }
    }
}

template <int N2>
int launch_s3(mimsem_ctx* c, const S3Args& a) {
    const long long ti = (long long)a.nEl*(a.nk - 1), tl = (long long)a.nEl*a.nk;
    hipLaunchKernelGGL((k_s3_ifc<N2>), dim3((unsigned)((ti + 3)/4)), dim3(64), 0, c->stream, a);
    hipLaunchKernelGGL((k_s3_lev<N2>), dim3((unsigned)((tl + 3)/4)), dim3(64), 0, c->stream, a);
    hipLaunchKernelGGL((k_s3_row<N2>), dim3((unsigned)((tl + 3)/4)), dim3(64), 0, c->stream, a);
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}


// ---- the diagonal factor blocks of the chain, assembled and inverted on the row algebra (orders 1..3): two launches for what the
// coefficient / block / inverse passes do in ~23 (colop_blocks_into x 14)
struct S3FactorArgs {
    NewtonGeo g;
    double ray_param; int rayleigh;                 // M_u^-1 = AssembleLinearWithRayleighInv(dt_fric) (eul) or AssembleLinearInv (box)
    int cv_from_velz;                               // VBA of Q_rt_rho: velz (eul :597) or the pressure gradient (box twin)
    const double *theta, *velz, *rho, *rt, *pi;     // theta on the nk+1 interfaces, velz on nk-1, the rest on nk levels
    double *B, *Binv, *Npiinv, *Brinv, *Brt, *Brtinv, *Bth;       // [nEl][nk][nn]
    double *Ainv, *Muinv, *T, *Rr, *Cg, *Cv;                      // [nEl][nk-1][nn]; Cg / Cv as CONLIN_W bands [nEl][nk][2][nn]
};

template <int N>
__global__ __launch_bounds__(64) void k_s3_factors_lev(S3FactorArgs a) {
    using T = ColTask<N>; using R = dpp::Rows<N>; using S = S3<N*N>;
    constexpr int N2 = T::N2, NP = T::NP, nn = N2*N2;
    const int lane = threadIdx.x, r = lane%16, nk = a.g.nk;
    const long long task0 = (long long)blockIdx.x*4 + lane/16, ntask = (long long)a.g.nEl*nk;
    const bool live = task0 < ntask;
    const long long task = live ? task0 : ntask - 1;
    const int e = (int)(task/nk), k = (int)(task%nk);
    T t; t.init(a.g, e, r);
    const bool act = live && r < N2;
    const size_t vo = ((size_t)e*nk + k)*N2 + t.rr, bo = ((size_t)e*nk + k)*nn;
    const size_t ti = ((size_t)e*(nk + 1) + k)*N2 + t.rr;
    double tI[NP], th[NP], cB[NP], c[NP], q[NP], q2[NP], B[N2], M[N2], t1[N2], t2[N2];
    t.geo(tI, th, k);
#pragma unroll
    for (int p = 0; p < NP; p++) cB[p] = t.q0[p]*tI[p];
#pragma unroll
    for (int p = 0; p < NP; p++) c[p] = cB[p];
    t.block(B, c);                                                       // VB = M_rt            AssembleConst :201-209
    S::store(a.B + bo, B, r, act);
#pragma unroll
    for (int j = 0; j < N2; j++) M[j] = B[j];
    R::inverse(M, r);                                                    // M_rho^-1 = VB^-1     AssembleConstInv :803-807
    S::store(a.Binv + bo, M, r, act);
    // N_pi^-1 = (VB VB(pi)^-1 VB)^-1                                    Assemble_EOS_BlockInv :1049-1142 (theta = NULL)
    t.interp(q, a.pi[vo]);
#pragma unroll
    for (int p = 0; p < NP; p++) c[p] = cB[p]*(q[p]/(th[p]*t.det[p]));
    t.inv_block(M, c);
    R::mul(t1, M, B);
    R::mul(t2, B, t1);
    R::inverse(t2, r);
    S::store(a.Npiinv + bo, t2, r, act);
    // VB(rho)^-1                                                        AssembleConstWithRhoInv :461-474
    t.interp(q, a.rho[vo]);
#pragma unroll
    for (int p = 0; p < NP; p++) c[p] = cB[p]*(q[p]/(th[p]*t.det[p]));
    t.inv_block(M, c);
    S::store(a.Brinv + bo, M, r, act);
    // VB(rt), VB(rt)^-1                                                 AssembleConstWithRho / ...Inv
    t.interp(q, a.rt[vo]);
#pragma unroll
    for (int p = 0; p < NP; p++) c[p] = cB[p]*(q[p]/(th[p]*t.det[p]));
    t.block(M, c);
    S::store(a.Brt + bo, M, r, act);
    R::inverse(M, r);
    S::store(a.Brtinv + bo, M, r, act);
    // VB(theta), theta on the interfaces below and above the level     AssembleConstWithTheta :946-962
    t.interp(q, a.theta[ti]); t.interp(q2, a.theta[ti + N2]);
#pragma unroll
    for (int p = 0; p < NP; p++) c[p] = cB[p]*(0.5*(q[p] + q2[p])/t.det[p]);
    t.block(M, c);
    S::store(a.Bth + bo, M, r, act);
}

template <int N>
__global__ __launch_bounds__(64) void k_s3_factors_ifc(S3FactorArgs a) {
    using T = ColTask<N>; using R = dpp::Rows<N>; using S = S3<N*N>;
    constexpr int N2 = T::N2, NP = T::NP, nn = N2*N2;
    const int lane = threadIdx.x, r = lane%16, nk = a.g.nk, nm = nk - 1;
    const long long task0 = (long long)blockIdx.x*4 + lane/16, ntask = (long long)a.g.nEl*nm;
    const bool live = task0 < ntask;
    const long long task = live ? task0 : ntask - 1;
    const int e = (int)(task/nm), i = (int)(task%nm);
    T t; t.init(a.g, e, r);
    const bool act = live && r < N2;
    const size_t v0 = ((size_t)e*nk + i)*N2 + t.rr, v1 = v0 + N2, io = ((size_t)e*nm + i)*N2 + t.rr, bo = ((size_t)e*nm + i)*nn;
    double tI0[NP], th0[NP], tI1[NP], th1[NP], c[NP], q[NP], q2[NP], Ai[N2], M[N2];
    t.geo(tI0, th0, i); t.geo(tI1, th1, i + 1);
#pragma unroll
    for (int p = 0; p < NP; p++) c[p] = t.q0[p]*(0.5*(th0[p] + th1[p]));
    t.inv_block(Ai, c);                                                  // VA^-1                AssembleLinearInv :422-430
    S::store(a.Ainv + bo, Ai, r, act);
    if (a.rayleigh) {                                                    // M_u^-1               AssembleLinearWithRayleighInv :1380-1413
        const double f = (i == nk - 2) ? (1.0 + 0.50*a.ray_param) : ((i == nk - 3) ? (1.0 + 0.25*a.ray_param) : 1.0);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = (t.q0[p]*(0.5*(th0[p] + th1[p])))*f;
        t.inv_block(M, c);
        S::store(a.Muinv + bo, M, r, act);
    } else S::store(a.Muinv + bo, Ai, r, act);
    // VA(theta), theta of interface i+1 of the nk+1                      AssembleLinearWithTheta :669-730
    t.interp(q, a.theta[((size_t)e*(nk + 1) + i + 1)*N2 + t.rr]);
#pragma unroll
    for (int p = 0; p < NP; p++) c[p] = t.q0[p]*(0.5*th0[p])*(q[p]/t.det[p]) + t.q0[p]*(0.5*th1[p])*(q[p]/t.det[p]);
    t.block(M, c);
    S::store(a.T + bo, M, r, act);
    // VA(rho), do_internal                                               AssembleLinearWithRT :607-667
    t.interp(q, a.rho[v0]); t.interp(q2, a.rho[v1]);
#pragma unroll
    for (int p = 0; p < NP; p++) c[p] = t.q0[p]*(0.5*q[p]/t.det[p]) + t.q0[p]*(0.5*q2[p]/t.det[p]);
    t.block(M, c);
    S::store(a.Rr + bo, M, r, act);
    // pressure gradient VA^-1 V01 VB pi (:528-531) and VBA(grad pi), VBA(velz)   AssembleConLinWithW :538-605: the block of interface i
    // sits at (k = i, w = 1) and (k = i+1, w = 0) of the band [nk][2]; (0, 0) and (nk-1, 1) do not exist (zero)
    t.interp(q, a.pi[v1]);
#pragma unroll
    for (int p = 0; p < NP; p++) c[p] = (t.q0[p]*tI1[p])*q[p];
    double bp = t.proj(c);
    t.interp(q, a.pi[v0]);
#pragma unroll
    for (int p = 0; p < NP; p++) c[p] = (t.q0[p]*tI0[p])*q[p];
    bp -= t.proj(c);
    const double gPi = R::matvec(Ai, bp);
    t.interp(q, gPi);
#pragma unroll
    for (int p = 0; p < NP; p++) c[p] = t.q0[p]*(0.5*q[p]/t.det[p]);
    t.block(M, c);
    S::store(a.Cg + (((size_t)e*nk + i)*2 + 1)*nn, M, r, act);
    S::store(a.Cg + (((size_t)e*nk + i + 1)*2 + 0)*nn, M, r, act);
    if (i == 0) S::zero(a.Cg + (((size_t)e*nk + 0)*2 + 0)*nn, r, act);
    if (i == nm - 1) S::zero(a.Cg + (((size_t)e*nk + nk - 1)*2 + 1)*nn, r, act);
    if (a.cv_from_velz) {
        t.interp(q, a.velz[io]);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = t.q0[p]*(0.5*q[p]/t.det[p]);
        t.block(M, c);
        S::store(a.Cv + (((size_t)e*nk + i)*2 + 1)*nn, M, r, act);
        S::store(a.Cv + (((size_t)e*nk + i + 1)*2 + 0)*nn, M, r, act);
        if (i == 0) S::zero(a.Cv + (((size_t)e*nk + 0)*2 + 0)*nn, r, act);
        if (i == nm - 1) S::zero(a.Cv + (((size_t)e*nk + nk - 1)*2 + 1)*nn, r, act);
    }
}

int launch_s3_factors(mimsem_ctx* c, const S3FactorArgs& a) {
    const long long tl = (long long)a.g.nEl*a.g.nk, ti = (long long)a.g.nEl*(a.g.nk - 1);
    if (int rc = for_order<1, 2, 3, 4>(c->es.n, [&](auto N) {
            hipLaunchKernelGGL((k_s3_factors_lev<N()>), dim3((unsigned)((tl + 3)/4)), dim3(64), 0, c->stream, a);
            hipLaunchKernelGGL((k_s3_factors_ifc<N()>), dim3((unsigned)((ti + 3)/4)), dim3(64), 0, c->stream, a); })) return rc;
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

}  // namespace
