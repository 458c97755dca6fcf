// column_schur3_sweep.inc -- included by column_kernels.hip after column_penta.inc (same translation unit).
//
// Round 4: VertSolve::solve_schur_column_3 (eul/VertSolve.cpp:504-675; box twin box/VertSolve.cpp:879-1058) in THREE launches:
//   k_s3_sweep<N>    one task walks a column (or a run of its levels): every factor of the MatMatMult chain (:517-627) is formed in
//                    registers on the DPP row algebra and only the five bands of L_rt_rt, the updated right-hand sides (:632-639) and
//                    the six blocks per level the back substitution re-uses leave the task;
//   k_penta_dpp<N2>  the block-pentadiagonal solve with refinement and per-column status (column_penta.inc);
//   k_s3_backsub<N>  the back substitution (:656-669).
// Rounds 2-3 ran the same algebra as 2 factor + 3 chain launches that wrote and re-read ~45 blocks per (column, level) (k_s3_row alone:
// 10 written, 13 read: 1.5 GB per launch), 13 banded mat-vec launches and the 18 x 18 super-block Thomas sweep: 30 launches, 2.6 ms for
// 3 456 columns x 30 levels.
//
// The algebra, regrouped so that a block is formed once and dies early (h = dt/2, g = R_d/c_v; level k, interface i between levels i, i+1):
//   level      B = VB, B^-1, Bpi = VB(pi), Br^-1 = VB(rho)^-1, Brt = VB(rt), Brt^-1, Bth = VB(theta);   P = Br^-1 B,  R = Bpi (Brt^-1 B)
//   interface  A^-1 = VA^-1, Mu^-1 (= A^-1 below the Rayleigh layer), T = VA(theta), Rr = VA(rho), C = VBA(grad pi), Cv = VBA(velz | grad pi);
//              X = A^-1 Rr,  TA = T A^-1,  CA = Cv A^-1,  elo_i = CA Bth_i,  ehi_i = CA Bth_{i+1},
//              GG(i,i) = h (C P_i - g TA R_i),  GG(i,i+1) = h (C P_{i+1} + g TA R_{i+1})      (= G_rt - G_pi N_pi^-1 N_rt, :532-555, :577-606),
//              MG = Mu^-1 GG
//   row k      DD(k,i) = -h d(k,i) X_i  (+ h Brt_k for i = k, - h Brt_k for i = k-1),   i = k-2 .. k+1               (:557-575, :587-613)
//              d(k,k-2) = h elo_{k-1};  d(k,k-1) = h (elo_k - elo_{k-1} - ehi_{k-1});  d(k,k) = h (ehi_{k-1} - elo_k - ehi_k);  d(k,k+1) = h ehi_k
//              L(k,.) = B_k delta - sum_i DD(k,i) MG(i,.)                                                                (:614-627)
// with N_pi^-1 = (B Bpi^-1 B)^-1 = B^-1 Bpi B^-1 (so G_pi N_pi^-1 N_rt needs neither N_pi^-1 nor N_rt: B N_pi^-1 B = Bpi) and
// (Q M_rho^-1) VB = Q: both exact up to cond(VB) eps ~ 1e-15 (VB is a mass block), against the reference's chain through two more
// inverses; the parity tests hold L to the oracle's at 1e-9 relative (observed ~1e-14) and the solution at 1e-10.
// The task visits the interfaces in order; interface i contributes to rows i-1 .. i+2 ONE STEP LATER (step s: level s+1 and interface s
// are built, then the rows of interface s-1 are updated -- they need elo of interface s), so that only three partial band blocks, three
// partial right-hand sides and the five products of one interface travel from step to step.

namespace {

struct S3SweepArgs {
    int nEl, nk, chunk, nchunk;
    const double *det, *tI, *th, *w, *W, *Eg;
    double E[20];
    double hdt, gam, ray_param; int rayleigh, cv_from_velz;
    const double *theta, *velz, *rho, *rt, *pi;         // theta on the nk+1 interfaces, velz on nk-1, the rest on nk levels
    const double *F_u, *F_rho, *F_pi; double* F_rt;      // F_rt updated in place (:632-639, negated :652); F_u' goes to fu2 (a neighbouring task
    double* fu2;                                         //   still reads the original F_u of the interfaces it recomputes)
    double* L; int rowmajor;                             // [nEl][nk][5][nn]
    int* statz;                                          // the unconverged-column counter of the solve that follows, zeroed here (a memset launch less)
    double *GGl, *GGu, *Mui, *X, *Binv, *Brti;           // kept for the back substitution, lane-major blocks: [nEl][nk-1][nn] x 4, [nEl][nk][nn] x 2
    double* dump;                                        // nn doubles per task: where the stores of rows a task does not own go
};

template <class R>
struct S3Col {
    static constexpr int N2 = R::N2, NC = R::NC, nn = N2*N2, NP = R::NP, MP12 = R::MP12, MP1 = R::MP1;
    struct Lev {
        double B[NC], P[NC], Rm[NC], Bth[NC], Brt[NC];
        double th[NP], rhI[NP];
        double bpi, sv, nv;                              // B pi, Bth B^-1 F_rho, Bpi B^-1 F_pi  (distributed vectors)
    };
    struct Raw { double tI[NP], th[NP], pi, rho, rt, th0, th1, frho, fpi, frt, velz, fu; };     // level k and the vectors of interface k-1
    __device__ static void load(Raw& Wr, const S3SweepArgs& a, int e, int k, int lane_r, int rr) {
        const int nk = a.nk;
        const size_t vo = ((size_t)e*nk + k)*N2 + rr, to = ((size_t)e*(nk + 1) + k)*N2 + rr;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int q = min(lane_r + 16*p, MP12 - 1);
            const size_t go = ((size_t)k*a.nEl + e)*MP12 + q;
            Wr.tI[p] = a.tI[go]; Wr.th[p] = a.th[go];
        }
        Wr.pi = a.pi[vo]; Wr.rho = a.rho[vo]; Wr.rt = a.rt[vo];
        Wr.th0 = a.theta[to]; Wr.th1 = a.theta[to + N2];
        Wr.frho = a.F_rho[vo]; Wr.fpi = a.F_pi[vo]; Wr.frt = a.F_rt[vo];
        const size_t io = ((size_t)e*(nk - 1) + max(k - 1, 0))*N2 + rr;
        Wr.velz = a.velz ? a.velz[io] : 0.0; Wr.fu = a.F_u[io];
    }
};

// HALF (order 4 only): the half-row block layout dpp::RowsH -- 8 columns of a block row per lane, two tasks per wavefront -- in which the
// walk's ~20 live blocks fit the register file (column_dpp.inc; MIMSEM_S3_HALF=0 selects the 16-lane layout with its ~700 spilled dwords)
template <int N, bool BOX, bool HALF = false>
__global__ __launch_bounds__(64) void k_s3_sweep(S3SweepArgs a) {
    using R = std::conditional_t<HALF, dpp::RowsH, dpp::Rows<N>>;
    using SC = S3Col<R>;
    static_assert(!HALF || N == 4, "the half-row layout is the 16 x 16 block's");
    constexpr int N2 = R::N2, NC = R::NC, nn = SC::nn, NP = R::NP, MP12 = R::MP12, MP1 = R::MP1;
    const int lane = threadIdx.x, r = lane%16, c0 = R::c0(lane);
    // the four tasks of a wavefront are four COLUMNS of the same chunk of levels: chunk, owned rows and the trip count of the walk are
    // wave-uniform (scalar registers, a scalar loop).  Round 4 first dealt (column, chunk) pairs out in task order: owned() and the loop
    // bounds were lane-varying, hipcc turned the address selections below into divergent if / else regions, and at order 4 (~690 spilled
    // VGPRs) it put spill stores into a structuriser "Flow" block AHEAD of the s_or_saveexec that re-enables the else-lanes -- those lanes
    // lose the value and reload stale scratch later: wrong, run-to-run different bands in the box flavour (found by reading the ISA;
    // scripts/check_spill_slots.py looks for the pattern).  With everything the branches depend on in SGPRs there is no exec-mask
    // region left in the loop body for a spill to land in.
    if (a.statz && blockIdx.x == 0 && lane == 0) { a.statz[0] = 0; a.statz[a.nEl + 1] = 0; }      // (the pentadiagonal launch behind this one counts into them)
    const WalkTask tk = walk_task<false, R::TPW>(a.nEl, a.nchunk, lane);   // (column_dpp.inc; a task beyond the last column repeats it)
    const int e = tk.e, ch = tk.ch;
    const int nk = a.nk, nm = nk - 1;
    const int k0 = ch*a.chunk, k1 = min(nk, k0 + a.chunk);              // rows (levels, and the interfaces of the same index) this task owns
    // lanes >= N2 of a 16-lane row MIRROR lane N2-1 in everything row-indexed (same tables, same loads, the Gauss-Jordan sweep takes rr as the
    // row id), so their stores repeat lane N2-1's -- the loop body below has NO exec-mask branch: with branches around its ~130 stores per
    // step the wait-count pass drains vmcnt to 0 (which on gfx9 also waits for every store in flight) at 15 places per step.  What a task
    // does not own goes to a per-task dump block by ADDRESS SELECTION instead.
    const int rr = r < N2 ? r : N2 - 1;
    const double h = a.hdt, gam = a.gam;
    const int rs = a.rowmajor ? N2 : 1, js = a.rowmajor ? 1 : N2;

    typename R::Lane Ln;
    R::init_lane(Ln, a.Eg, a.W, HALF ? lane : r);
    double q0[NP], det[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const int q = min(r + 16*p, MP12 - 1);
        det[p] = a.det[(size_t)e*MP12 + q];
        q0[p] = (a.w[q%MP1]*a.w[q/MP1])*(VSCALE/det[p]);
    }
    auto owned = [&](int k) __attribute__((always_inline)) { return k >= k0 && k < k1; };
    auto zero = [&](double (&M)[NC]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NC; j++) M[j] = 0.0;
    };
    // the accumulators collect  sum_i DD MG - B delta  = -L:  band block (row k, slot b) <- -acc
    // (a row the task does not own goes to its dump block: the INDEX is selected before the base is added -- no pointer outside an array is
    //  ever formed.  owned() is wave-uniform: scalar selects or scalar branches, hipcc's choice -- pinning the owned index in front of the
    //  select to keep the body branch-free made no difference on one box: 509-520 against 521-522 us at order 3, scripts/ab_taskmap.sh)
    const size_t dofs = (size_t)(blockIdx.x*R::TPW + R::task(lane))*nn;
    auto put = [&](int k, int b, const double (&acc)[NC]) __attribute__((always_inline)) {
        const bool o = owned(k);
        double* base = o ? a.L : a.dump;
        const size_t io = (((size_t)e*nk + k)*5 + b)*nn, i0 = (o ? io : dofs) + (size_t)rr*rs + (size_t)c0*js;
#pragma unroll
        for (int j = 0; j < NC; j++) base[i0 + (size_t)j*js] = -acc[j];
    };
    auto put0 = [&](int k, int b, bool also) __attribute__((always_inline)) {
        const bool o = owned(k) && also;
        double* base = o ? a.L : a.dump;
        const size_t io = (((size_t)e*nk + k)*5 + b)*nn, i0 = (o ? io : dofs) + (size_t)rr*rs + (size_t)c0*js;
#pragma unroll
        for (int j = 0; j < NC; j++) base[i0 + (size_t)j*js] = 0.0;
    };
    auto stb = [&](double* basep, size_t blk, bool own, const double (&M)[NC]) __attribute__((always_inline)) {       // lane-major block kept for the back substitution
        double* base = own ? basep : a.dump;
        const size_t io = blk*nn, i0 = (own ? io : dofs) + rr + (size_t)c0*N2;
#pragma unroll
        for (int j = 0; j < NC; j++) base[i0 + (size_t)j*N2] = M[j];
    };
    auto stv = [&](double* basep, size_t idx, bool own, double v) __attribute__((always_inline)) {
        (own ? basep : a.dump)[own ? idx : dofs + rr] = v;
    };

    // level k: its five blocks and three vectors; B^-1 and Brt^-1 are kept for the back substitution
    auto build_level = [&](typename SC::Lev& V, const typename SC::Raw& Wr, int k) __attribute__((always_inline)) {
        double c[NP], cB[NP], q[NP], q2[NP], M[NC], t1[NC];
#pragma unroll
        for (int p = 0; p < NP; p++) { V.th[p] = Wr.th[p]; cB[p] = q0[p]*Wr.tI[p]; c[p] = cB[p]; }
        R::assemble(V.B, Ln, a.E, c);                                    // VB = M_rt               AssembleConst :201-209
#pragma unroll
        for (int j = 0; j < NC; j++) M[j] = V.B[j];
        R::inverse(M, HALF ? lane : rr);                                               // M_rho^-1 = VB^-1        AssembleConstInv :803-807
        stb(a.Binv, (size_t)e*nk + k, owned(k), M);
        const double gr = R::matvec(M, Wr.frho, lane), gp = R::matvec(M, Wr.fpi, lane);
        V.bpi = R::matvec(V.B, Wr.pi, lane);
        // VB(theta), theta on the interfaces below and above the level  AssembleConstWithTheta :946-962
        R::interp(q, Ln, Wr.th0); R::interp(q2, Ln, Wr.th1);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = cB[p]*(0.5*(q[p] + q2[p])/det[p]);
        R::assemble(V.Bth, Ln, a.E, c);
        V.sv = R::matvec(V.Bth, gr, lane);
        // VB(rho)^-1 -> P = VB(rho)^-1 VB                               AssembleConstWithRhoInv :461-474
        R::interp(V.rhI, Ln, Wr.rho);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = cB[p]*(V.rhI[p]/(Wr.th[p]*det[p]));
        R::assemble(M, Ln, a.E, c);
        R::inverse(M, HALF ? lane : rr);
        R::mul(V.P, M, V.B);
        // VB(rt), VB(rt)^-1                                             AssembleConstWithRho :508-521 / ...Inv
        R::interp(q, Ln, Wr.rt);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = cB[p]*(q[p]/(Wr.th[p]*det[p]));
        R::assemble(V.Brt, Ln, a.E, c);
#pragma unroll
        for (int j = 0; j < NC; j++) M[j] = V.Brt[j];
        R::inverse(M, HALF ? lane : rr);
        stb(a.Brti, (size_t)e*nk + k, owned(k), M);
        R::mul(t1, M, V.B);                                              // Brt^-1 B
        // VB(pi) -> R = Bpi (Brt^-1 B)                                  Assemble_EOS_BlockInv :1049-1142 (theta = NULL), N_rt :577-585
        R::interp(q, Ln, Wr.pi);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = cB[p]*(q[p]/(Wr.th[p]*det[p]));
        R::assemble(M, Ln, a.E, c);
        V.nv = R::matvec(M, gp, lane);
        R::mul(V.Rm, M, t1);
    };

    const int s0 = max(0, k0 - 3), s1 = min(nm, k1 + 1);
    typename SC::Lev lo;
    typename SC::Raw Wr;                                                 // level s+1 and the vectors of interface s, requested one step ahead
    SC::load(Wr, a, e, s0, r, rr);
    double frC = Wr.frt;                                                 // running F_rt of row s (frA, frB: rows s-2, s-1)
    build_level(lo, Wr, s0);
    SC::load(Wr, a, e, min(s0 + 1, nk - 1), r, rr);

    // what travels from step to step.  Four of the blocks are COLD -- written at the end of a step, read once by rows() of the next --
    // and wait in LDS (one workgroup = one wavefront: 4 x N2 x 64 doubles, conflict-free columns; lgkmcnt, not the vmcnt the stores
    // share): with them in registers the kernel spilled to scratch, and every scratch reload is a vmcnt(0) that drains the stores in flight
    __shared__ double park[(HALF ? 7 : 4)*NC*64];
    auto park_st = [&](int slot, const double (&M)[NC]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NC; j++) park[(slot*NC + j)*64 + lane] = M[j];
    };
    auto park_ld = [&](int slot, double (&M)[NC]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NC; j++) M[j] = park[(slot*NC + j)*64 + lane];
    };
    enum { P_EHI0 = 0, P_ELO1 = 1, P_EHI1 = 2, P_BRT0 = 3, P_ACCA = 4, P_ACCB = 5, P_ACCC = 6 };      // ehi of interface s-2; elo, ehi of interface s-1; Brt of level s-1;
    // half-row layout: the three running band accumulators wait in LDS too while a level and an interface are built (they are only touched by rows())
    double X1[NC], MGl1[NC], MGu1[NC];                                   // interface s-1
    double accA[NC], accB[NC], accC[NC];                                               // (row s-2, slot 3), (row s-1, slot 2), (row s, slot 1)
    double v1 = 0.0;                                                                   // Mu^-1 F_u' of interface s-1
    double frA = 0.0, frB = 0.0;
    zero(X1); zero(MGl1); zero(MGu1); zero(accA); zero(accB); zero(accC);
    park_st(P_EHI0, accA); park_st(P_ELO1, accA); park_st(P_EHI1, accA); park_st(P_BRT0, accA);
    auto acc_st = [&]() __attribute__((always_inline)) { if constexpr (HALF) { park_st(P_ACCA, accA); park_st(P_ACCB, accB); park_st(P_ACCC, accC); } };
    auto acc_ld = [&]() __attribute__((always_inline)) { if constexpr (HALF) { park_ld(P_ACCA, accA); park_ld(P_ACCB, accB); park_ld(P_ACCC, accC); } };
    acc_st();

    // the rows i-1 .. i+2 of interface i = s-1:  DD = -h d X_i (+- h Brt),  acc += DD MG,  F_rt -= DD v  (d: see the header)
    auto rows = [&](int s, const double (&elo)[NC], double frt_new) __attribute__((always_inline)) {
        double dd[NC], DD[NC], accN[NC], ehi0[NC], e1[NC];
        acc_ld();
        park_ld(P_EHI0, ehi0);
        // row s-2: d = h ehi_{i-1};  slots 3 (col i) and 4 (col i+1): the row is complete
#pragma unroll
        for (int j = 0; j < NC; j++) dd[j] = (-h*h)*ehi0[j];
        R::mul(DD, dd, X1);
        R::mul_add(accA, DD, MGl1);
        put(s - 2, 3, accA);
        R::mul(accA, DD, MGu1);
        put(s - 2, 4, accA);
        frA -= R::matvec(DD, v1, lane);
        stv(a.F_rt, ((size_t)e*nk + (s - 2))*N2 + rr, owned(s - 2), -1.0*frA);      // :652
        // row s-1: d = h (ehi_{i-1} - elo_i - ehi_i), + h Brt_i;  slots 2 (col i, complete) and 3 (col i+1, carried as accA)
        park_ld(P_ELO1, e1); park_ld(P_EHI1, accN);
#pragma unroll
        for (int j = 0; j < NC; j++) { e1[j] += accN[j]; dd[j] = (-h*h)*(ehi0[j] - e1[j]); }     // e1 = elo_i + ehi_i
        R::mul(DD, dd, X1);
        park_ld(P_BRT0, accN);
#pragma unroll
        for (int j = 0; j < NC; j++) DD[j] += h*accN[j];
        R::mul_add(accB, DD, MGl1);
        put(s - 1, 2, accB);
        R::mul(accA, DD, MGu1);
        frB -= R::matvec(DD, v1, lane);
        // row s: d = h (elo_{i+1} - elo_i - ehi_i), - h Brt_{i+1};  slots 1 (col i, complete) and 2 (col i+1 = s: starts from -B_s, carried as accB)
#pragma unroll
        for (int j = 0; j < NC; j++) dd[j] = (-h*h)*(elo[j] - e1[j]);
        R::mul(DD, dd, X1);
#pragma unroll
        for (int j = 0; j < NC; j++) DD[j] -= h*lo.Brt[j];
        R::mul_add(accC, DD, MGl1);
        put(s, 1, accC);
#pragma unroll
        for (int j = 0; j < NC; j++) accB[j] = -lo.B[j];
        R::mul_add(accB, DD, MGu1);
        frC -= R::matvec(DD, v1, lane);
        // row s+1: d = h elo_{i+1};  slots 0 (col i, complete) and 1 (col i+1, carried as accC)
#pragma unroll
        for (int j = 0; j < NC; j++) dd[j] = (-h*h)*elo[j];
        R::mul(DD, dd, X1);
        R::mul(accN, DD, MGl1);
        put(s + 1, 0, accN);
        R::mul(accC, DD, MGu1);
        const double frD = frt_new - R::matvec(DD, v1, lane);
        put0(0, 0, s == 0);                                              // (row 0, col -2): the one block no step visits
        frA = frB; frB = frC; frC = frD;                                 // rows s-1, s, s+1: next step's s-2, s-1, s
        acc_st();
    };

    const int sl = min(s1, nm - 1);                                      // steps that build an interface (s < nm)
#pragma unroll 1
    for (int s = s0; s <= sl; s++) {
        // ---- (b) A^-1, CA = Cv A^-1 and elo of interface s: the rows of interface s-1 need elo_s ----
        double Ai[NC], CA[NC], elo[NC], c[NP], wI[NP], gpi = 0.0;
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = q0[p]*(0.5*(lo.th[p] + Wr.th[p]));
        R::assemble(Ai, Ln, a.E, c);
        R::inverse(Ai, HALF ? lane : rr);                                              // VA^-1                   AssembleLinearInv :422-430
        {
            double wv = Wr.velz;                                         // eul: VBA(velz) (:597)
            if (BOX) {                                                   // box twin: Q is built from VBA(grad pi) (box/VertSolve.cpp:978-981):
#pragma unroll                                                           //   the pressure gradient of interface s is needed before level s+1 is built
                for (int p = 0; p < NP; p++) c[p] = q0[p]*Wr.tI[p];
                double Bh[NC];
                R::assemble(Bh, Ln, a.E, c);
                gpi = R::matvec(Ai, R::matvec(Bh, Wr.pi, lane) - lo.bpi, lane);
                wv = gpi;
            }
            R::interp(wI, Ln, wv);
#pragma unroll
            for (int p = 0; p < NP; p++) c[p] = q0[p]*(0.5*wI[p]/det[p]);
            double Cv[NC];
            R::assemble(Cv, Ln, a.E, c);                                 // AssembleConLinWithW :551-600
            R::mul(CA, Cv, Ai);
            R::mul(elo, CA, lo.Bth);
        }
        // ---- (c) the rows of interface s-1 ----
        rows(s, elo, Wr.frt);
        // what rows() read from the park is spent: shift the interface products now (interface s-1 becomes s-2) and park elo and Brt of
        // this step, so that neither stays in registers while level s+1 and interface s are built
        { double t[NC]; park_ld(P_EHI1, t); park_st(P_EHI0, t); }
        park_st(P_ELO1, elo); park_st(P_BRT0, lo.Brt);
        // ---- (d) level s+1 ----
        typename SC::Lev hi;
        build_level(hi, Wr, s + 1);
        const double fu_s = Wr.fu, th_if = Wr.th0;                        // F_u of interface s; theta of interface s+1 of the nk+1 (= below level s+1)
        SC::load(Wr, a, e, min(s + 2, nk - 1), r, rr);                    // level s+2 travels under (e) and the next step's (b)
        // ---- (e) interface s ----
        double T[NC], TA[NC], C[NC], GGl[NC], GGu[NC], t1[NC];
        // pressure gradient VA^-1 V01 VB pi (:528-531), C = VBA(grad pi)   AssembleConLinWithW :551-600
        if (!BOX) gpi = R::matvec(Ai, hi.bpi - lo.bpi, lane);
        R::interp(wI, Ln, gpi);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = q0[p]*(0.5*wI[p]/det[p]);
        R::assemble(C, Ln, a.E, c);
        // ehi_s = CA Bth_{s+1};  c_s = CA (s_{s+1} - s_s): F_rt -= Q M_rho^-1 F_rho (:632-633) reaches rows s and s+1
        double ehi[NC];
        R::mul(ehi, CA, hi.Bth);
        park_st(P_EHI1, ehi);                                            // (read by the rows() of the next two steps only)
        const double cs = h*R::matvec(CA, hi.sv - lo.sv, lane);
        frB -= cs; frC -= cs;                                            // (rows s and s+1 after the shift in rows())
        // T = VA(theta of interface s+1 of the nk+1)                    AssembleLinearWithTheta :669-730
        R::interp(wI, Ln, th_if);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = q0[p]*(0.5*lo.th[p])*(wI[p]/det[p]) + q0[p]*(0.5*hi.th[p])*(wI[p]/det[p]);
        R::assemble(T, Ln, a.E, c);
        R::mul(TA, T, Ai);
        // F_u' = F_u - G_pi N_pi^-1 F_pi (:635-636) = F_u - h TA (n_{s+1} - n_s)
        const double fu2 = fu_s - h*R::matvec(TA, hi.nv - lo.nv, lane);
        const size_t io = ((size_t)e*nm + s)*N2 + rr;
        stv(a.fu2, io, owned(s), fu2);
        // GG(s,s) = h (C P_s - g TA R_s),  GG(s,s+1) = h (C P_{s+1} + g TA R_{s+1})
        R::mul(GGl, C, lo.P);
        R::mul(t1, TA, lo.Rm);
#pragma unroll
        for (int j = 0; j < NC; j++) GGl[j] = h*GGl[j] - (h*gam)*t1[j];
        R::mul(GGu, C, hi.P);
        R::mul(t1, TA, hi.Rm);
#pragma unroll
        for (int j = 0; j < NC; j++) GGu[j] = h*GGu[j] + (h*gam)*t1[j];
        const size_t bo = (size_t)e*nm + s;
        stb(a.GGl, bo, owned(s), GGl); stb(a.GGu, bo, owned(s), GGu);
        // Rr = VA(rho), X = A^-1 Rr                                     AssembleLinearWithRT :607-667 (do_internal), :563-565
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = q0[p]*(0.5*lo.rhI[p]/det[p]) + q0[p]*(0.5*hi.rhI[p]/det[p]);
        R::assemble(T, Ln, a.E, c);
        R::mul(X1, Ai, T);
        stb(a.X, bo, owned(s), X1);
        // M_u^-1 = VA^-1 / f: the Rayleigh layer scales VA of the two top interfaces by f = 1 + {0.25, 0.5} dt_fric
        // (AssembleLinearWithRayleighInv :1380-1413, eul); f = 1 elsewhere and in the box twin (AssembleLinearInv)
        const double fr = a.rayleigh ? ((s == nk - 2) ? (1.0 + 0.50*a.ray_param) : ((s == nk - 3) ? (1.0 + 0.25*a.ray_param) : 1.0)) : 1.0;
        const double fri = 1.0/fr;
#pragma unroll
        for (int j = 0; j < NC; j++) Ai[j] *= fri;
        stb(a.Mui, bo, owned(s), Ai);
        R::mul(MGl1, Ai, GGl);
        R::mul(MGu1, Ai, GGu);
        v1 = R::matvec(Ai, fu2, lane);
        lo = hi;
    }
    // the walk ended at the top of the column: the rows of the last interface (no interface nm: elo = 0), then the two rows that have no
    // interface left above them
    if (s1 == nm) {
        double elo[NC];
        zero(elo);
        rows(nm, elo, 0.0);
        acc_ld();
        // shifted: accA = (row nm-1, slot 3), accB = (row nm, slot 2), frA / frB = rows nm-1 / nm
        put(nm - 1, 3, accA); put0(nm - 1, 4, true);
        put(nm, 2, accB); put0(nm, 3, true); put0(nm, 4, true);
        stv(a.F_rt, ((size_t)e*nk + nm - 1)*N2 + rr, owned(nm - 1), -1.0*frA);
        stv(a.F_rt, ((size_t)e*nk + nm)*N2 + rr, owned(nm), -1.0*frB);
    }
}

// ---- back substitution (eul/VertSolve.cpp:656-669) from the blocks the sweep kept ------------------------------------------------------
//   F_u <- -(F_u' + GG d_rt),  d_u = M_u^-1 F_u;      F_pi <- -(F_pi + N_rt d_rt),  d_pi = N_pi^-1 F_pi;      F_rho <- -(F_rho + D_rho d_u),  d_rho = M_rho^-1 F_rho
// with N_rt d = -g B (Brt^-1 (B d)),  N_pi^-1 f = B^-1 (Bpi (B^-1 f)),  (D_rho d_u)_k = h B_k (X_k du_k - X_{k-1} du_{k-1}): chains of mat-vecs.
// One task = column e, levels [k0, k1); the interface below the first level is recomputed rather than communicated.
struct S3BackArgs {
    int nEl, nk, chunk, nchunk;
    const double *det, *tI, *th, *w, *W, *Eg;
    double E[20];
    double hdt, gam;
    const double *pi, *d_rt, *fu2;
    const double *GGl, *GGu, *Mui, *X, *Binv, *Brti;
    double *F_u, *F_pi, *F_rho, *d_u, *d_pi, *d_rho;
};
template <int N>
__global__ __launch_bounds__(64) void k_s3_backsub(S3BackArgs a) {
    using R = dpp::Rows<N>; using PO = PentaOps<N*N>;
    constexpr int N2 = R::N2, nn = N2*N2, NP = R::NP, MP12 = R::MP12, MP1 = R::MP1;
    const int lane = threadIdx.x, r = lane%16;
    const WalkTask tk = walk_task<N == 4>(a.nEl, a.nchunk, lane);
    const bool live = tk.live;
    const int e = tk.e, ch = tk.ch;
    const int nk = a.nk, nm = nk - 1;
    const int k0 = ch*a.chunk, k1 = min(nk, k0 + a.chunk);
    const int rr = r < N2 ? r : N2 - 1;
    const bool act = live && r < N2;
    const double h = a.hdt, gam = a.gam;
    typename R::Lane Ln;
    R::init_lane(Ln, a.Eg, a.W, r);
    double q0[NP], det[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const int q = min(r + 16*p, MP12 - 1);
        det[p] = a.det[(size_t)e*MP12 + q];
        q0[p] = (a.w[q%MP1]*a.w[q/MP1])*(VSCALE/det[p]);
    }
    const double* dre = a.d_rt + (size_t)e*nk*N2 + rr;
    // X_i d_u,i of interface i (and the stores of F_u, d_u when the task owns it)
    auto iface = [&](int i, bool own) {
        const size_t bo = ((size_t)e*nm + i)*nn + rr, io = ((size_t)e*nm + i)*N2 + rr;
        double M[N2];
        const double d0 = dre[(size_t)i*N2], d1 = dre[(size_t)(i + 1)*N2];
        PO::ld(M, a.GGl + bo, N2);
        double fu = a.fu2[io] + PO::matvec(M, d0);
        PO::ld(M, a.GGu + bo, N2);
        fu += PO::matvec(M, d1);
        fu *= -1.0;                                                      // :656-658
        PO::ld(M, a.Mui + bo, N2);
        const double du = PO::matvec(M, fu);                             // :659
        if (act && own) { a.F_u[io] = fu; a.d_u[io] = du; }
        PO::ld(M, a.X + bo, N2);
        return PO::matvec(M, du);
    };
    double xd_below = k0 > 0 ? iface(k0 - 1, false) : 0.0;
#pragma unroll 1
    for (int k = k0; k < k1; k++) {
        const size_t vo = ((size_t)e*nk + k)*N2 + rr, lo = ((size_t)e*nk + k)*nn + rr;
        double tI[NP], th[NP], c[NP], q[NP], B[N2], M[N2];
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int qq = min(r + 16*p, MP12 - 1);
            const size_t go = ((size_t)k*a.nEl + e)*MP12 + qq;
            tI[p] = a.tI[go]; th[p] = a.th[go];
        }
        const double piv = a.pi[vo], fpi_in = a.F_pi[vo], frho_in = a.F_rho[vo], dk = dre[(size_t)k*N2];
        const double xd = k < nm ? iface(k, true) : 0.0;
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = q0[p]*tI[p];
        R::assemble(B, Ln, a.E, c);
        // F_pi <- -(F_pi + N_rt d_rt)   (:661-663),  N_rt = -g VB VB(rt)^-1 VB
        PO::ld(M, a.Brti + lo, N2);
        double fpi = fpi_in + (-1.0*gam)*R::matvec(B, PO::matvec(M, R::matvec(B, dk)));
        fpi *= -1.0;
        // d_pi = N_pi^-1 F_pi = B^-1 (Bpi (B^-1 F_pi))   (:664)
        PO::ld(M, a.Binv + lo, N2);
        R::interp(q, Ln, piv);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = (q0[p]*tI[p])*(q[p]/(th[p]*det[p]));
        double Bp[N2];
        R::assemble(Bp, Ln, a.E, c);
        const double dpi = PO::matvec(M, R::matvec(Bp, PO::matvec(M, fpi)));
        // F_rho <- -(F_rho + D_rho d_u)   (:666-668),  d_rho = M_rho^-1 F_rho   (:669)
        double frho = frho_in + h*R::matvec(B, xd - xd_below);
        frho *= -1.0;
        const double drho = PO::matvec(M, frho);
        if (act) { a.F_pi[vo] = fpi; a.d_pi[vo] = dpi; a.F_rho[vo] = frho; a.d_rho[vo] = drho; }
        xd_below = xd;
    }
}

// orders 1..4.  At order 4 a block is 32 VGPRs per lane and the walk's ~20 live blocks do not fit 512 registers: k_s3_sweep<4> compiles
// with ~390 spilled dwords per lane -- correct only while no spill lands in a divergent region (see the note on the task mapping in the
// kernel; scripts/check_spill_slots.py checks the ISA for it, tests/test_dpp_hazards.py runs it).  MIMSEM_SCHUR3_FUSED4=0 sends order 4
// back to round 2's chain kernels for the bands (+ the pentadiagonal solve of column_penta.inc).
bool s3_fused_supported(const mimsem_ctx* c) {
    const char* f4 = exp_env("MIMSEM_SCHUR3_FUSED4");
    const int nmax = (f4 && atoi(f4) == 0) ? 3 : 4;
    return c->es.n >= 1 && c->es.n <= nmax && c->nk >= 4 && !getenv("MIMSEM_SCHUR3_CHAIN");
}

// solve_schur_column_3 in three launches; L_out (optional): the bands in the ABI's row-major layout (the solve then reads them from there)
int s3_fused_solve(mimsem_ctx* c, double dt, unsigned flags, const double* theta, const double* velz, const double* rho, const double* rt,
                   const double* pi, double* F_u, double* F_rho, double* F_rt, double* F_pi, double* d_u, double* d_rho, double* d_rt,
                   double* d_pi, double* L_out) {
    mimsem::S3FusedWS w;
    int rc = plan_col(c, w);
    if (rc) return rc;
    S3SweepArgs a{};
    a.dump = w.dump;
    // order 4: the half-row block layout (two tasks per wavefront, no spill); MIMSEM_S3_HALF=0 keeps the 16-lane layout for A/B runs
    const bool half = c->es.n == 4 && !(exp_env("MIMSEM_S3_HALF") && atoi(exp_env("MIMSEM_S3_HALF")) == 0);
    fill_geo(c, a, 1, 1024, half ? 2 : 4);
    if ((rc = ensure_colstat(c))) return rc;
    a.statz = c->d_colstat;
    a.hdt = 0.5*dt; a.gam = RD/CV;
    a.rayleigh = (flags & MIMSEM_SCHUR3_NO_RAYLEIGH) ? 0 : 1; a.ray_param = 0.5*dt*(4.0/120.0);     // RAYLEIGH, eul/VertSolve.cpp:32, :520
    a.cv_from_velz = (flags & MIMSEM_SCHUR3_BOX_Q) ? 0 : 1;
    a.theta = theta; a.velz = a.cv_from_velz ? velz : nullptr; a.rho = rho; a.rt = rt; a.pi = pi;
    a.F_u = F_u; a.F_rho = F_rho; a.F_pi = F_pi; a.F_rt = F_rt; a.fu2 = w.fu2;
    a.L = L_out ? L_out : w.L; a.rowmajor = L_out ? 1 : 0;
    a.GGl = w.GGl; a.GGu = w.GGu; a.Mui = w.Mui; a.X = w.X; a.Binv = w.Binv; a.Brti = w.Brti;
    {
        const unsigned grid = walk_task_grid(a.nEl, a.nchunk, false, half ? 2 : 4);          // (four -- half-row layout: two -- columns of one chunk per wavefront)
        const auto sweep = [&](auto N) {
            if (a.cv_from_velz) hipLaunchKernelGGL((k_s3_sweep<N(), false>), dim3(grid), dim3(64), 0, c->stream, a);
            else hipLaunchKernelGGL((k_s3_sweep<N(), true>), dim3(grid), dim3(64), 0, c->stream, a);
        };
        if (half) {
            if (a.cv_from_velz) hipLaunchKernelGGL((k_s3_sweep<4, false, true>), dim3(grid), dim3(64), 0, c->stream, a);
            else hipLaunchKernelGGL((k_s3_sweep<4, true, true>), dim3(grid), dim3(64), 0, c->stream, a);
        } else
#ifdef MIMSEM_WITH_EXPERIMENTS
        if ((rc = for_order<1, 2, 3, 4>(c->es.n, sweep))) return rc;      // (order 4 on the 16-lane layout, ~700 spilled dwords per lane: MIMSEM_S3_HALF=0, DESIGN 6.5; the default is the half-row walk above)
#else
        if ((rc = for_order<1, 2, 3>(c->es.n, sweep))) return rc;
#endif
        MIMSEM_HIP_TRY(hipGetLastError());
    }
    if ((rc = launch_penta_dpp(c, refine_steps(), a.L, a.rowmajor != 0, F_rt, d_rt, w.Fac, w.yws, true))) return rc;
    if ((rc = launch_band_lu_flagged(c, 2, a.L, a.rowmajor != 0, F_rt, d_rt))) return rc;       // (opt-in: flagged columns by a pivoted band LU)
    c->colstat_valid = true;
    S3BackArgs b{};
    fill_geo(c, b, exp_env("MIMSEM_S3B_WPS") ? atoi(exp_env("MIMSEM_S3B_WPS")) : 2);      // wavefronts per SIMD the level chunking aims at (A/B knob)
    b.hdt = a.hdt; b.gam = a.gam; b.pi = pi; b.d_rt = d_rt; b.fu2 = w.fu2;
    b.GGl = w.GGl; b.GGu = w.GGu; b.Mui = w.Mui; b.X = w.X; b.Binv = w.Binv; b.Brti = w.Brti;
    b.F_u = F_u; b.F_pi = F_pi; b.F_rho = F_rho; b.d_u = d_u; b.d_pi = d_pi; b.d_rho = d_rho;
    {
        const unsigned grid = walk_task_grid(b.nEl, b.nchunk, c->es.n == 4);
        if ((rc = for_order<1, 2, 3, 4>(c->es.n, [&](auto N) { hipLaunchKernelGGL((k_s3_backsub<N()>), dim3(grid), dim3(64), 0, c->stream, b); }))) return rc;
        MIMSEM_HIP_TRY(hipGetLastError());
    }
    return MIMSEM_OK;
}

}  // namespace
