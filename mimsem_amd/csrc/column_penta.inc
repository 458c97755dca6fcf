// column_penta.inc -- included by column_kernels.hip after column_dpp.inc (same translation unit: dpp::, ThomasCol).
//
// Round 4: the block-PENTAdiagonal solve of solve_schur_column_3 (eul/VertSolve.cpp:641-653: KSPSolve with PCLU on L_rt_rt; box twin
// box/VertSolve.cpp:1033-1041) on the DPP row algebra, without the 2 x 2 super-blocks of rounds 1-3.
//
// Rounds 1-3 regrouped the five bands into a block-TRIdiagonal matrix of (2 n2)-wide super-blocks and ran the block-Thomas sweep on
// those: 18 x 18 blocks do not fit a 16-lane DPP row (k_block_thomas_rows<18,32>: 32 lanes per column, pivot rows through
// ds_bpermute), and a super-row costs two 18^3 products and an 18 x 18 inverse = ~12 n2^3-products per level.  Eliminating the two
// sub-diagonals directly keeps every block n2 x n2 -- one row per lane, v_fmac_f64_dpp row_newbcast products, the Gauss-Jordan of
// column_dpp.inc -- and costs 6 products + 1 inverse per level:
//   row k = [a b c d e] at block columns k-2 .. k+2, normalised rows above it:  x_j + G1_j x_{j+1} + G2_j x_{j+2} = y_j
//     b' = b - a G1_{k-2}      c' = c - a G2_{k-2} - b' G1_{k-1}      d' = d - b' G2_{k-1}      f' = f - a y_{k-2} - b' y_{k-1}
//     D_k^-1 = c'^-1,   G1_k = D^-1 d',   G2_k = D^-1 e,   y_k = D^-1 f';           back:  x_k = y_k - G1_k x_{k+1} - G2_k x_{k+2}
// TWO-SIDED (twisted) like k_thomas_dpp2: DPP rows 2c / 2c+1 of a wavefront eliminate the top half of column c downwards and the
// bottom half upwards in SWEEP ORDER (step i = level i or nk-1-i; "previous" = towards the own end, "next" = towards the middle), so both
// halves execute the same instructions.  At the middle four unknowns meet: mine u1 (nearest the middle), u2 and the other half's o1, o2:
//     u2 + G1(2) u1 + G2(2) o1 = y(2)          u1 + G1(1) o1 + G2(1) o2 = y(1)          (and the same with the roles exchanged)
//   eliminate u2, o2:    P_me u1 + Q_me o1 = r_me,    P_me = I - G2(1) H2(2),  Q_me = G1(1) - G2(1) H1(2),  r_me = y(1) - G2(1) z(2)
//                        Q_o  u1 + P_o  o1 = r_o      (H, z: the other half's second row; P_o, Q_o, r_o: its P_me, Q_me, r_me)
//   =>  (P_me - W Q_o) u1 = r_me - W r_o,   W = Q_me P_o^-1:   two n2 x n2 inverses and four products per half, after two cross-row exchanges.
// Iterative refinement, per-column status and the achieved ratio exactly as in k_thomas_dpp2 (the elimination does not pivot across
// blocks; the reference's PCLU does): r = f - L x with the five bands, the kept factors {D^-1, G1, G2, b'} make the second solve
// substitution only.  One-sided form (TWO = false, four columns per wavefront) for odd nk.
//
// Band storage: L[e][k][b][.] with block column k-2+b, blocks outside the matrix stored as ZEROS (the sweep multiplies by them instead of
// branching); inside a block element (r, j) sits at r*rs + j*js -- (rs, js) = (1, n2): lane-major, the layout k_s3_sweep writes (one
// instruction stores 16 contiguous values); (n2, 1): the row-major layout of the ABI.

#ifndef MIMSEM_PENTA_PF
#define MIMSEM_PENTA_PF 9            // largest block size whose forward elimination requests the next row under the current one (A/B knob)
#endif
namespace {

template <int N2>
struct PentaOps {
    static constexpr int nn = N2*N2;
    __device__ static void ld(double (&M)[N2], const double* p, int js) {
#pragma unroll
        for (int j = 0; j < N2; j++) M[j] = p[(long long)j*js];
    }
    __device__ static void st(double* p, const double (&M)[N2], bool act) {          // lane-major
        if (!act) return;
#pragma unroll
        for (int j = 0; j < N2; j++) p[j*N2] = M[j];
    }
    // C -= A . B
    __device__ static void mulsub(double (&C)[N2], const double (&A)[N2], const double (&B)[N2]) { dpp::MulSub<N2>::run(C, A, B); }
    // C = A . B
    __device__ static void mul(double (&C)[N2], const double (&A)[N2], const double (&B)[N2]) {
#pragma unroll
        for (int j = 0; j < N2; j++) C[j] = 0.0;
        dpp::MulAcc<N2>::run(C, A, B);
    }
    __device__ static double matvec(const double (&A)[N2], double x) {
        double y = 0.0;
        dpp::MatvecAcc<N2>::run(y, A, x);
        return y;
    }
};

// LM: the bands are lane-major (the layout k_s3_sweep writes) -- the strides are then compile-time constants and every block load addresses
// its 16 elements as immediate offsets from ONE base; with run-time strides (the ABI's row-major bands) each element carries its own 64-bit
// address, and at order 4 those address registers were what pushed the two-sided kernel to 577 spilled dwords per lane (round 5).
template <int N2, bool TWO, bool LM>
__global__ __launch_bounds__(64) void k_penta_dpp(int nEl, int nk, int refine_and_flags, const double* __restrict__ L, int rs_, int js_,
                                                   const double* __restrict__ f, double* __restrict__ d, double* __restrict__ Fac,
                                                   double* __restrict__ yws, int* __restrict__ stat, double* __restrict__ ratio) {
    using P = PentaOps<N2>; constexpr int nn = N2*N2;
    const bool triage = (refine_and_flags & 0x100) != 0;               // bit 8: triage flagged columns here (the pivoted fallback is on)
    const int refine = refine_and_flags & 0xff;
    const int rs = LM ? 1 : rs_, js = LM ? N2 : js_;
    const int lane = threadIdx.x, r = lane%16, row = lane/16, h = TWO ? (row & 1) : 0;
    const int e0 = TWO ? blockIdx.x*2 + row/2 : blockIdx.x*4 + row;
    const int e = e0 < nEl ? e0 : nEl - 1, rr = r < N2 ? r : N2 - 1;
    const bool act = e0 < nEl && r < N2;
    const int m = TWO ? nk/2 : nk;
    const int kb = h ? nk - 1 : 0, ks = h ? -1 : 1;                     // level of sweep step i: kb + i ks
    // band slots in sweep order: previous-2, previous-1, diagonal, next-1, next-2
    const int o2p = (2 - 2*ks)*nn, o1p = (2 - ks)*nn, o0 = 2*nn, o1n = (2 + ks)*nn, o2n = (2 + 2*ks)*nn;
    const double* Le = L + ((size_t)e*nk + kb)*5*nn + (size_t)rr*rs;
    double* Fe = Fac + ((size_t)e*nk + kb)*4*nn + rr;                    // {D^-1, G1, G2, b'} lane-major
    double* ye = yws + ((size_t)e*nk + kb)*N2 + rr;
    const double* fe = f + ((size_t)e*nk + kb)*N2 + rr;
    double* de = d + ((size_t)e*nk + kb)*N2 + rr;
    const long long sL = (long long)ks*5*nn, sF = (long long)ks*4*nn, sV = (long long)ks*N2;
    auto other = [&](double v) { return TWO ? __shfl_xor(v, 16) : 0.0; };

    // ---- forward elimination, factors kept ----
    double G1a[N2], G2a[N2], G1b[N2], G2b[N2], ya = 0.0, yb = 0.0;       // normalised rows i-2 (a) and i-1 (b)
#pragma unroll
    for (int j = 0; j < N2; j++) { G1a[j] = 0.0; G2a[j] = 0.0; G1b[j] = 0.0; G2b[j] = 0.0; }
    {
        double nP2[N2], nP1[N2], nT[N2], nQ1[N2], nQ2[N2], nf;
        auto fetch = [&](int i) {
            const double* rw = Le + (long long)i*sL;
            P::ld(nP2, rw + o2p, js); P::ld(nP1, rw + o1p, js); P::ld(nT, rw + o0, js); P::ld(nQ1, rw + o1n, js); P::ld(nQ2, rw + o2n, js);
            nf = fe[(long long)i*sV];
        };
        constexpr bool PF = N2 <= MIMSEM_PENTA_PF;           // next row's five blocks requested under this row's arithmetic (16 x 16 blocks: no registers left for that)
        if (PF) fetch(0);
#pragma unroll 1
        for (int i = 0; i < m; i++) {
            double P2[N2], P1[N2], T[N2], Q1[N2], Q2[N2];
            if (!PF) fetch(i);
#pragma unroll
            for (int j = 0; j < N2; j++) { P2[j] = nP2[j]; P1[j] = nP1[j]; T[j] = nT[j]; Q1[j] = nQ1[j]; Q2[j] = nQ2[j]; }
            double fk = nf;
            if (PF && i + 1 < m) fetch(i + 1);
            P::mulsub(P1, P2, G1a);                                       // b' = b - a G1_{i-2}
            P::mulsub(T, P2, G2a);                                        // c' = c - a G2_{i-2} - b' G1_{i-1}
            fk -= P::matvec(P2, ya);
            P::mulsub(T, P1, G1b);
            P::mulsub(Q1, P1, G2b);                                       // d' = d - b' G2_{i-1}
            fk -= P::matvec(P1, yb);
            ThomasCol<N2>::inverse_nopivot(T, r);
#pragma unroll
            for (int j = 0; j < N2; j++) { G1a[j] = G1b[j]; G2a[j] = G2b[j]; }
            ya = yb;
            P::mul(G1b, T, Q1);
            P::mul(G2b, T, Q2);
            yb = P::matvec(T, fk);
            double* F = Fe + (long long)i*sF;
            P::st(F, T, act); P::st(F + nn, G1b, act); P::st(F + 2*nn, G2b, act); P::st(F + 3*nn, P1, act);
            if (act) ye[(long long)i*sV] = yb;
        }
    }
    // ---- the middle (two-sided): Sinv, W kept for the refinement ----
    double Sinv[N2], W[N2];
    if (TWO) {
        double t[N2], Pm[N2], Qm[N2], Po[N2], Qo[N2];
#pragma unroll
        for (int j = 0; j < N2; j++) t[j] = other(G2a[j]);                // H2(2)
        P::mul(Pm, G2b, t);
#pragma unroll
        for (int j = 0; j < N2; j++) { Pm[j] = (j == rr ? 1.0 : 0.0) - Pm[j]; t[j] = other(G1a[j]); }      // P_me = I - G2(1) H2(2);  H1(2)
#pragma unroll
        for (int j = 0; j < N2; j++) Qm[j] = G1b[j];
        P::mulsub(Qm, G2b, t);                                            // Q_me = G1(1) - G2(1) H1(2)
#pragma unroll
        for (int j = 0; j < N2; j++) { Po[j] = other(Pm[j]); Qo[j] = other(Qm[j]); }
        ThomasCol<N2>::inverse_nopivot(Po, r);
        P::mul(W, Qm, Po);                                                // W = Q_me P_o^-1
#pragma unroll
        for (int j = 0; j < N2; j++) Sinv[j] = Pm[j];
        P::mulsub(Sinv, W, Qo);
        ThomasCol<N2>::inverse_nopivot(Sinv, r);
    }
    // my two unknowns nearest the middle from my two last normalised right-hand sides y1 (step m-1), y2 (step m-2).  The G blocks of
    // those two rows are re-read from the kept factors (three block loads per call, 1 + refinement steps calls) rather than held in
    // registers across the refinement loops
    double u1, u2;
    auto middle = [&](double y1, double y2) {
        double G[N2];
        const double* F1 = Fe + (long long)(m - 1)*sF; const double* F2 = Fe + (long long)(m >= 2 ? m - 2 : 0)*sF;
        if (TWO) {
            P::ld(G, F1 + 2*nn, N2);                                      // G2(1)
            const double rme = y1 - P::matvec(G, other(y2));
            u1 = P::matvec(Sinv, rme - P::matvec(W, other(rme)));
            P::ld(G, F2 + nn, N2);                                        // G1(2)
            u2 = y2 - P::matvec(G, u1);
            P::ld(G, F2 + 2*nn, N2);                                      // G2(2)
            u2 -= P::matvec(G, other(u1));
        } else {
            u1 = y1;                                                      // G1, G2 of the last row and G2 of the one before are zero blocks
            P::ld(G, F2 + nn, N2);
            u2 = y2 - P::matvec(G, u1);
        }
    };
    // back substitution x_i = y_i - G1_i x_{i+1} - G2_i x_{i+2}, i = m-3 .. 0; update: the result is a correction (x += it), norms collected
    double s_dd = 0.0, s_d = 0.0;
    auto backsub = [&](double x1, double x2, bool update) {               // x1 = x_{i+1}, x2 = x_{i+2} of the first step
        double Ga[N2], Gb[N2], yi = 0.0, oi = 0.0;
        auto fetchb = [&](int i) {
            const double* F = Fe + (long long)i*sF;
            P::ld(Ga, F + nn, N2); P::ld(Gb, F + 2*nn, N2);
            yi = ye[(long long)i*sV];
            oi = update ? de[(long long)i*sV] : 0.0;
        };
        if (m >= 3) fetchb(m - 3);
#pragma unroll 1
        for (int i = m - 3; i >= 0; i--) {
            double A1[N2], A2[N2];
#pragma unroll
            for (int j = 0; j < N2; j++) { A1[j] = Ga[j]; A2[j] = Gb[j]; }
            const double yk = yi, ok = oi;
            if (i > 0) fetchb(i - 1);
            const double xi = yk - P::matvec(A1, x1) - P::matvec(A2, x2);
            const double xn = ok + xi;
            if (act) de[(long long)i*sV] = xn;
            s_dd += xi*xi; s_d += xn*xn;
            x2 = x1; x1 = xi;
        }
    };
    middle(yb, ya);
    double xb1 = u1, xb2 = u2;                                            // the solution at steps m-1, m-2 (kept: the residual across the middle needs them)
    if (act) { de[(long long)(m - 1)*sV] = xb1; if (m >= 2) de[(long long)(m - 2)*sV] = xb2; }
    backsub(m >= 2 ? xb2 : xb1, xb1, false);                             // first step i = m-3: x_{i+1} = x_{m-2}, x_{i+2} = x_{m-1}
    // ---- iterative refinement ----
    bool conv = false; double last = -1.0;
#pragma unroll 1
    for (int it = 0; it < refine; it++) {
        const double xo1 = other(xb1), xo2 = other(xb2);                 // the other half's unknowns nearest the middle
        // sliding window of x in sweep order around step i (own values re-read from memory: each lane reads what it stored itself)
        double xm2 = 0.0, xm1 = 0.0, x0 = de[0];
        auto xat = [&](int i) { return i < m ? de[(long long)i*sV] : (i == m ? xo1 : (i == m + 1 ? xo2 : 0.0)); };
        double xp1 = xat(1), xp2 = xat(2);
        double y1 = 0.0, y2 = 0.0;                                        // y' of steps i-1, i-2
        double nP2[N2], nP1[N2], nT[N2], nQ1[N2], nQ2[N2], nD[N2], nB[N2], nf, nx3;
        auto fetchr = [&](int i) {
            const double* rw = Le + (long long)i*sL;
            P::ld(nP2, rw + o2p, js); P::ld(nP1, rw + o1p, js); P::ld(nT, rw + o0, js); P::ld(nQ1, rw + o1n, js); P::ld(nQ2, rw + o2n, js);
            const double* F = Fe + (long long)i*sF;
            P::ld(nD, F, N2); P::ld(nB, F + 3*nn, N2);
            nf = fe[(long long)i*sV];
            nx3 = i + 3 < m ? de[(long long)(i + 3)*sV] : (i + 3 == m ? xo1 : (i + 3 == m + 1 ? xo2 : 0.0));
        };
        fetchr(0);
#pragma unroll 1
        for (int i = 0; i < m; i++) {
            double rk = nf;
            rk -= P::matvec(nP2, xm2); rk -= P::matvec(nP1, xm1); rk -= P::matvec(nT, x0); rk -= P::matvec(nQ1, xp1); rk -= P::matvec(nQ2, xp2);
            rk -= P::matvec(nP2, y2);                                     // forward solve with the kept factors: a y'_{i-2} + b' y'_{i-1}
            rk -= P::matvec(nB, y1);
            const double yn = P::matvec(nD, rk);
            const double x3 = nx3;
            if (i + 1 < m) fetchr(i + 1);
            if (act) ye[(long long)i*sV] = yn;
            y2 = y1; y1 = yn;
            xm2 = xm1; xm1 = x0; x0 = xp1; xp1 = xp2; xp2 = x3;
        }
        middle(y1, y2);
        xb1 += u1; xb2 += (m >= 2 ? u2 : 0.0);
        if (act) { de[(long long)(m - 1)*sV] = xb1; if (m >= 2) de[(long long)(m - 2)*sV] = xb2; }
        s_dd = u1*u1 + (m >= 2 ? u2*u2 : 0.0); s_d = xb1*xb1 + (m >= 2 ? xb2*xb2 : 0.0);
        backsub(m >= 2 ? u2 : u1, u1, true);
        // stop as soon as the correction of this column is below 1e-10 of the solution (uniform over the column's rows)
        double t_dd = 0.0, t_d = 0.0;
        dpp::static_for<0, N2>([&](auto mm) { t_dd += dpp::get<mm.value>(s_dd); t_d += dpp::get<mm.value>(s_d); });
        if (TWO) { t_dd += other(t_dd); t_d += other(t_d); }
        conv = t_dd <= 1.0e-20*t_d;
        const double prev = last;
        last = t_d > 0.0 ? sqrt(t_dd/t_d) : 0.0;
        if (conv) break;
        if (it > 0 && last > 0.5*prev) break;                         // stagnated at the column's conditioning floor (as k_thomas_dpp2)
    }
    int st = refine <= 0 ? 2 : (conv ? 0 : 1);
    // triage of a column the refinement left above 1e-10, as in k_thomas_dpp2 (column_dpp.inc): normwise backward error of the solution it
    // has; at round-off level the column is limited by its conditioning (status 4, not counted), otherwise it stays 1 for the pivoted LU
    if (triage && __ballot(st == 1) != 0ull) {
        const double xo1 = other(xb1), xo2 = other(xb2);
        auto xat = [&](int i) { return i < m ? de[(long long)i*sV] : (i == m ? xo1 : (i == m + 1 ? xo2 : 0.0)); };
        double xm2 = 0.0, xm1 = 0.0, x0 = de[0], xp1 = xat(1), xp2 = xat(2);
        double r2 = 0.0, a2 = 0.0, x2 = 0.0, f2 = 0.0;
        const double w = r < N2 ? 1.0 : 0.0;
#pragma unroll 1
        for (int i = 0; i < m; i++) {
            const double* rw = Le + (long long)i*sL;
            double B2[N2], B1[N2], T[N2], Q1[N2], Q2[N2];
            P::ld(B2, rw + o2p, js); P::ld(B1, rw + o1p, js); P::ld(T, rw + o0, js); P::ld(Q1, rw + o1n, js); P::ld(Q2, rw + o2n, js);
            const double fi = fe[(long long)i*sV], x3 = xat(i + 3);
            const double rk = fi - P::matvec(B2, xm2) - P::matvec(B1, xm1) - P::matvec(T, x0) - P::matvec(Q1, xp1) - P::matvec(Q2, xp2);
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < N2; j++) s += B2[j]*B2[j] + B1[j]*B1[j] + T[j]*T[j] + Q1[j]*Q1[j] + Q2[j]*Q2[j];      // (blocks outside the matrix are stored as zeros)
            r2 += w*rk*rk; a2 += w*s; x2 += w*x0*x0; f2 += w*fi*fi;
            xm2 = xm1; xm1 = x0; x0 = xp1; xp1 = xp2; xp2 = x3;
        }
        double t_r = 0.0, t_a = 0.0, t_x = 0.0, t_f = 0.0;
        dpp::static_for<0, N2>([&](auto mm) { t_r += dpp::get<mm.value>(r2); t_a += dpp::get<mm.value>(a2); t_x += dpp::get<mm.value>(x2); t_f += dpp::get<mm.value>(f2); });
        if (TWO) { t_r += other(t_r); t_a += other(t_a); t_x += other(t_x); t_f += other(t_f); }
        const double eta0 = sqrt(t_r)/(sqrt(t_a)*sqrt(t_x) + sqrt(t_f));
        if (st == 1 && eta0 <= BANDLU_ACCEPT) st = 4;                   // (NaN fails)
    }
    if (stat && r == 0 && h == 0 && e0 < nEl) { stat[1 + e] = st; ratio[e] = last; if (st == 1) { const int pos = atomicAdd(stat + nEl + 1, 1); stat[nEl + 2 + pos] = e; atomicAdd(stat, 1); } }
}

// L x = f for every column; L block-pentadiagonal [nEl][nk][5][nn]; Fac: 4 nn doubles and yws: n2 doubles per (column, level)
int launch_penta_dpp(mimsem_ctx* c, int refine, const double* L, bool rowmajor, const double* f, double* d, double* Fac, double* yws, bool counter_zeroed = false) {
    const int n2 = c->es.n2e, nk = c->nk;
    if (int rc = ensure_colstat(c)) return rc;
    if (!counter_zeroed) { MIMSEM_HIP_TRY(hipMemsetAsync(c->d_colstat, 0, sizeof(int), c->stream)); MIMSEM_HIP_TRY(hipMemsetAsync(c->d_colstat + c->nEl + 1, 0, sizeof(int), c->stream)); }
    const int rs = rowmajor ? n2 : 1, js = rowmajor ? 1 : n2;
    const bool two = nk >= 4 && nk%2 == 0 && !(exp_env("MIMSEM_PENTA2") && atoi(exp_env("MIMSEM_PENTA2")) == 0);
    if (refine > 0xff) refine = 0xff;
    if (c->pivot_fallback == 1 && !(exp_env("MIMSEM_THOMAS_TRIAGE") && atoi(exp_env("MIMSEM_THOMAS_TRIAGE")) == 0)) refine |= 0x100;      // (as launch_thomas_dpp)
    if (int rc = for_order<1, 4, 9, 16>(n2, [&](auto N) {
        if (two && !rowmajor) hipLaunchKernelGGL((k_penta_dpp<N(), true, true>), dim3((unsigned)((c->nEl + 1)/2)), dim3(64), 0, c->stream, c->nEl, nk, refine, L, rs, js, f, d, Fac, yws, c->d_colstat, c->d_colratio);
        else if (two) hipLaunchKernelGGL((k_penta_dpp<N(), true, false>), dim3((unsigned)((c->nEl + 1)/2)), dim3(64), 0, c->stream, c->nEl, nk, refine, L, rs, js, f, d, Fac, yws, c->d_colstat, c->d_colratio);
        else hipLaunchKernelGGL((k_penta_dpp<N(), false, false>), dim3((unsigned)((c->nEl + 3)/4)), dim3(64), 0, c->stream, c->nEl, nk, refine, L, rs, js, f, d, Fac, yws, c->d_colstat, c->d_colratio);
    })) return rc;
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

}  // namespace
