// column_pivot.inc -- included by column_kernels.hip before column_dpp.inc.
//
// The remedy behind mimsem_column_solve_status.  The reference solves every column system with KSPSolve + PCLU
// (eul/VertSolve.cpp:645-653, :783-789, :806-812; box/VertSolve.cpp:1031-1041): a banded LU that pivots over the WHOLE band.  The default
// path here eliminates block by block on the DPP row algebra (k_thomas_dpp2 / k_penta_dpp: Gauss-Jordan inside a block, no pivoting
// across blocks) and refines; on the rare column whose conditioning that cannot resolve (about 0.2 % of rough random columns with
// cond(L) ~ 1e10, and the pathological cond ~ 1e13 one of DESIGN 2) it reports status 1 instead of a silent MIMSEM_OK.  Those columns are
// re-solved INSIDE the same call, before the back substitution reads d -- ON BY DEFAULT since round 5 (mimsem_column_set_pivot_fallback(ctx, 0)
// / MIMSEM_COLUMN_PIVOT_FALLBACK=0 switch it off).
//
// Round 5: ONE WAVEFRONT per flagged column, LU with partial pivoting on the block structure (round 4: a workgroup running LAPACK's unblocked
// dgbtf2 with a __syncthreads per scalar column: ~0.9 ms for any non-empty set of flagged columns, and an extra launch of nEl workgroups when
// nothing was flagged).  A block-banded matrix with nb sub- and super-diagonal blocks (nb = 1: L_pi, nb = 2: L_rt_rt) has, in block column k,
// entries in block rows k .. k + nb only; partial pivoting over those (nb + 1) n2 rows IS partial pivoting over the scalar band (dgbtf2's
// kl + 1 candidates are these rows plus structural zeros).  The wavefront keeps the ACTIVE WINDOW in registers, one row per lane: the
// <= (nb + 1) n2 <= 48 rows that still have entries in block column k, each with its (2 nb + 1) n2 window columns (block columns
// k .. k + 2 nb: the fill of the pivoting lands there) and its right-hand side.  One pivot step = a 32-bit max over the lanes (the high word
// of |a|, lane id in the low bits: DPP row shifts + four readlanes), the pivot row through v_readlane into SGPRs, one FMA per window column
// and lane.  Rows are never swapped: a lane that supplied a pivot retires (its row is a finished row of U and goes to the workspace when the
// block column is done), the window slides by one block, and the n2 retired lanes take the rows of the next block row (staged through LDS
// while the block column was eliminated, so the global latency hides behind the pivot steps).  nb virtual identity block columns in front of
// the matrix make the first window like every other.  Multipliers and pivot lanes are kept, so the one refinement step replays the
// elimination on the residual alone.  Back substitution block by block (a block's rows in n2 lanes, x of the blocks above from LDS).
//   status 3 ("solved by the pivoted fallback") and the counter decrement ONLY for a verified solve: every norm finite and the normwise
//   backward error of the LU solve |f - A x| / (|A|_F |x| + |f|) <= 1e-12 -- what a pivoted LU delivers whatever the conditioning -- and a
//   refinement correction below half the solution
//   (round 4 marked every processed column 3, NaN included: advisor).  ratio = |correction| / |solution| of the refinement step: the
//   conditioning-limited forward indicator, same meaning as for status 0 / 1.  A column that fails the check keeps status 1 and its d.
// No slot limit (a grid of 64 wavefronts strides over the flagged columns) and no extra cost worth naming when nothing is flagged: every
// wavefront reads the unconverged counter and leaves.
// Mode 2 sends EVERY column through the pivoted LU (a validation mode: the reference's algorithm for all columns, at its price).
//
// Band storage of the input: L[e][k][b][.] with block column k - nb + b (nb = 1: tridiagonal, 3 bands; nb = 2: pentadiagonal, 5 bands),
// element (r, j) of a block at r*rs + j*js.

namespace {

struct BandLUArgs {
    int nEl, nk, rs, js, all, stop;     // stop (profiling knob MIMSEM_BLU_STOP): leave a column after phase 1..4 -- timing runs only, no result
    const double* L; const double* f; double* d;
    int* stat; double* ratio;
    double* W; long long per;           // workspace: `per` doubles per wavefront of the grid
};

constexpr int BANDLU_NMAX = 1024;       // unknowns per column the LDS vectors hold (64 levels x 16)
constexpr double BANDLU_ACCEPT = 1.0e-14;   // normwise backward error at which a flagged column's block-sweep solution stands (status 4): a pivoted LU's own level

// compile-time loop (the window columns and the pivot steps of a block column index registers)
template <int M, int END, class F> __device__ __forceinline__ void blu_static_for(F&& f) {
    if constexpr (M < END) { f(std::integral_constant<int, M>{}); blu_static_for<M + 1, END>(f); }
}
__device__ __forceinline__ double readlane_f64(double v, int l) {        // l wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
// max over the 64 lanes of an unsigned key, result wave-uniform: four DPP row shifts (lane 15 of every 16-lane row ends with the row's
// maximum; bound_ctrl: lanes shifted in from outside read 0) and one readlane per row
__device__ __forceinline__ unsigned wave_umax(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));     // row_shr:1
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));     // row_shr:2
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));     // row_shr:4
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));     // row_shr:8
    const unsigned a = __builtin_amdgcn_readlane((int)v, 15), b = __builtin_amdgcn_readlane((int)v, 31),
                   c = __builtin_amdgcn_readlane((int)v, 47), d = __builtin_amdgcn_readlane((int)v, 63);
    return max(max(a, b), max(c, d));
}
// 1 / pivot: v_rcp_f64 + three Newton steps (the IEEE division is a ~25-instruction dependent chain, and the wavefront has nothing to
// hide it behind); within an ulp or two of the quotient -- a multiplier that is off by an ulp leaves an O(eps |a|) entry behind, the size
// of the rounding of the elimination itself.  A zero or non-finite pivot gives Inf / NaN: the column then fails its verification.
__device__ __forceinline__ double blu_rcp(double x) {
    double y = __builtin_amdgcn_rcp(x);
    y = fma(fma(-x, y, 1.0), y, y);
    y = fma(fma(-x, y, 1.0), y, y);
    y = fma(fma(-x, y, 1.0), y, y);
    return y;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <int N2, int NB>
__global__ __launch_bounds__(64) void k_band_lu_wave(BandLUArgs a) {
    constexpr int NR = (NB + 1)*N2, WB = 2*NB + 1, WC = WB*N2, nn = N2*N2, RS = WC + 1;
    constexpr int NST = (N2*WC + 63)/64;                                 // staging loads per lane and block row
    static_assert(NR <= 64, "the active rows of a block column must fit one wavefront");
    const int lane = threadIdx.x;
    if (!a.all && a.stat[0] == 0) return;                                // (uniform) nothing was flagged: the whole launch is this load
    const int nk = a.nk, n = nk*N2, nbc = nk + NB, nsteps = nbc*N2;      // block columns incl. the NB virtual ones in front
    __shared__ double s_x[BANDLU_NMAX], s_r[BANDLU_NMAX], s_dx[BANDLU_NMAX], s_row[N2*RS];
    __shared__ unsigned char s_piv[(64 + 2)*16];
    double* U = a.W + (size_t)blockIdx.x*a.per;                          // [nsteps][WC + 1]: the rows of U in pivot order, and y
    double* M = U + (size_t)nsteps*RS;                                   // [nsteps][64]: the multipliers of every step, per lane

    // OWNERSHIP through the FLAGGED LIST (round 6, advisor): the solve kernels append every column they flag to a list (stat[nEl + 2 ...], its
    // length in stat[nEl + 1]); nothing writes to it while this kernel runs, so wavefront b takes entries b, b + grid, b + 2 grid, ... -- every
    // flagged column exactly once, spread evenly however they are numbered.  Round 5 dealt the columns by a running ordinal over the LIVE
    // statuses, which other wavefronts rewrite (1 -> 3 / 4) during the same launch: a column could be skipped or solved twice.  (The first
    // fix, ownership by column index e % grid, was race-free but let two of ten flagged columns meet in one wavefront: +2.5 % on the bench.)
    // Mode 2 (every column): ownership by column index.  The early exit above stays right: a zero counter means every flagged column is resolved.
    const int nlist = a.all ? a.nEl : a.stat[a.nEl + 1];
#pragma unroll 1
    for (int it = blockIdx.x; it < nlist; it += gridDim.x) {
        {
            const int e = __builtin_amdgcn_readfirstlane(a.all ? it : a.stat[a.nEl + 2 + it]);          // (wave-uniform: SGPRs for everything addressed through it)
            const int st0 = __builtin_amdgcn_readfirstlane(a.stat[1 + e]);
            if (!a.all && st0 != 1) continue;                            // (cannot happen: only flagged columns are listed; kept as the guard it is)
            const double* Le = a.L + (size_t)e*nk*WB*nn;
            const double* fe = a.f + (size_t)e*n;
            double* de = a.d + (size_t)e*n;

            // ================= residual r = f - A x with its norms (used three times: triage, verification, refinement) =================
            auto residual = [&](const double* xs, double* rs_out, double& nr2, double& na2, double& nf2) __attribute__((always_inline)) {
                double r2 = 0.0, a2 = 0.0, f2 = 0.0;
#pragma unroll 1
                for (int i = lane; i < n; i += 64) {
                    const int kr = i/N2, r = i%N2;
                    const double fi = fe[i];
                    double acc = fi;
                    double v[WC];
#pragma unroll
                    for (int bnd = 0; bnd < WB; bnd++) {                 // every load of the row in flight before the first use
                        const int cb = kr - NB + bnd;
                        const bool in = cb >= 0 && cb < nk;
                        const double* blk = Le + ((size_t)kr*WB + (in ? bnd : NB))*nn + (size_t)r*a.rs;
#pragma unroll
                        for (int j = 0; j < N2; j++) { const double t = blk[(size_t)j*a.js]; v[bnd*N2 + j] = in ? t : 0.0; }
                    }
#pragma unroll
                    for (int bnd = 0; bnd < WB; bnd++) {
                        const int cb = min(max(kr - NB + bnd, 0), nk - 1);
#pragma unroll
                        for (int j = 0; j < N2; j++) { acc = fma(-v[bnd*N2 + j], xs[cb*N2 + j], acc); a2 = fma(v[bnd*N2 + j], v[bnd*N2 + j], a2); }
                    }
                    if (rs_out) rs_out[i] = acc;
                    r2 = fma(acc, acc, r2); f2 = fma(fi, fi, f2);
                }
                nr2 = wave_sum(r2); na2 = wave_sum(a2); nf2 = wave_sum(f2);
            };
            // ---- triage: is the flagged column's block-sweep solution already as good as a pivoted LU's?  Most flagged columns are flagged
            // because their CONDITIONING keeps the refinement's correction above 1e-10 of the solution (cond ~ 1e10: ratio ~ 1e-9 from any
            // solver in double precision), not because the unpivoted elimination lost accuracy: their normwise backward error is at round-off
            // level.  Such a column keeps its solution and becomes status 4; only a column whose backward error says the elimination itself
            // went wrong (the cond ~ 1e13 column of DESIGN 2: 1e-9) pays for the factorisation below.
            if (!a.all) {
                double t2 = 0.0;
#pragma unroll 1
                for (int i = lane; i < n; i += 64) { const double v = de[i]; s_x[i] = v; t2 = fma(v, v, t2); }
                t2 = wave_sum(t2);
                __syncthreads();
                double r2, a2, f2;
                residual(s_x, nullptr, r2, a2, f2);
                const double eta0 = sqrt(r2)/(sqrt(a2)*sqrt(t2) + sqrt(f2));
                __syncthreads();
                if (eta0 <= BANDLU_ACCEPT) {                             // (NaN fails)
                    if (lane == 0) { a.stat[1 + e] = 4; if (st0 == 1) atomicSub(a.stat, 1); }
                    continue;
                }
            }
            // block row i staged into registers (issued early) and later published in LDS: s_row[r][c], c = band*N2 + j, [WC] = rhs
            double stg[NST];
            auto stage_issue = [&](int i, const double* rhs_g, const double* rhs_s) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < NST; u++) {
                    const int q = lane + 64*u, r = q/WC, cpos = q%WC, bnd = cpos/N2, j = cpos%N2, cb = i - NB + bnd;
                    stg[u] = (q < N2*WC && i < nk && cb >= 0 && cb < nk) ? Le[((size_t)i*WB + bnd)*nn + (size_t)r*a.rs + (size_t)j*a.js] : 0.0;
                }
            };
            auto stage_publish = [&](int i, const double* rhs_g, const double* rhs_s) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < NST; u++) {
                    const int q = lane + 64*u;
                    if (q < N2*WC) s_row[(q/WC)*RS + q%WC] = stg[u];
                }
                if (lane < N2) s_row[lane*RS + WC] = i < nk ? (rhs_g ? rhs_g[i*N2 + lane] : rhs_s[i*N2 + lane]) : 0.0;
            };

            // ================= factorisation, with the forward substitution of f riding along =================
            double w[WC], b;
            bool alive;
            int myt = -1;
            // lanes 0 .. NB N2 - 1: the virtual identity rows (window column = lane); lanes NB N2 .. NR - 1: block row 0 (its bands sit at
            // the window's block positions 0 .. 2 NB because the window starts NB block columns before the matrix)
            stage_issue(0, fe, nullptr);
            stage_publish(0, fe, nullptr);
            __syncthreads();
            {
                const int r0 = lane - NB*N2;
#pragma unroll
                for (int cpos = 0; cpos < WC; cpos++) w[cpos] = lane < NB*N2 ? (cpos == lane ? 1.0 : 0.0) : ((r0 >= 0 && r0 < N2) ? s_row[r0*RS + cpos] : 0.0);
                b = (r0 >= 0 && r0 < N2) ? s_row[r0*RS + WC] : 0.0;
                alive = lane < NR;
            }
            __syncthreads();
#pragma unroll 1
            for (int kb = 0; kb < nbc; kb++) {
                stage_issue(kb + 1, fe, nullptr);                        // the block row that enters when this block column is done
                blu_static_for<0, N2>([&](auto jjc) {
                    constexpr int jj = jjc.value;
                    const int t = kb*N2 + jj;
                    const unsigned hi = (unsigned)__double2hiint(w[jj]) & 0x7fffffffu;
                    const unsigned key = alive ? ((hi & ~63u) | (unsigned)lane) + 64u : 0u;       // (an alive zero still beats every retired lane)
                    const int p = (int)((wave_umax(key) - 64u) & 63u);
                    const double piv = readlane_f64(w[jj], p);
                    const double rp = blu_rcp(piv);
                    const double m = (alive && lane != p) ? w[jj]*rp : 0.0;
                    M[(size_t)t*64 + lane] = m;
                    if (lane == 0) s_piv[t] = (unsigned char)p;
#pragma unroll
                    for (int cpos = jj + 1; cpos < WC; cpos++) w[cpos] = fma(-m, readlane_f64(w[cpos], p), w[cpos]);
                    b = fma(-m, readlane_f64(b, p), b);
                    if (lane == p) { alive = false; myt = t; }
                });
                // the N2 rows that supplied the pivots are rows of U now
                const bool ret = myt >= 0;
                if (ret) {
#pragma unroll
                    for (int cpos = 0; cpos < WC; cpos++) U[(size_t)myt*RS + cpos] = w[cpos];
                    U[(size_t)myt*RS + WC] = b;
                }
                stage_publish(kb + 1, fe, nullptr);
                __syncthreads();
                const unsigned long long rm = __ballot(ret);
                const int rank = __popcll(rm & ((1ull << lane) - 1ull));
                const bool enter = ret && kb + 1 < nk;
#pragma unroll
                for (int cpos = 0; cpos < WC; cpos++) {
                    const double sh = cpos + N2 < WC ? w[cpos + N2 < WC ? cpos + N2 : 0] : 0.0;        // the window slides by one block
                    w[cpos] = ret ? (enter ? s_row[rank*RS + cpos] : 0.0) : sh;
                }
                if (ret) b = enter ? s_row[rank*RS + WC] : 0.0;
                alive = ret ? enter : alive;
                myt = -1;
                __syncthreads();
            }

            if (a.stop == 1) continue;
            // ================= back substitution: block k from the rows of U of its N2 pivot steps =================
            auto backsub = [&](double* xs) __attribute__((always_inline)) {
                constexpr bool PF = WC <= 48;                            // (order 4, pentadiagonal: two row sets would not fit the register file)
                double u[WC], y = 0.0, un[PF ? WC : 1], yn = 0.0;
                auto ldrows = [&](int kb, auto& uu, double& yy) __attribute__((always_inline)) {
                    const size_t t = (size_t)kb*N2 + (lane < N2 ? lane : N2 - 1);
#pragma unroll
                    for (int cpos = 0; cpos < WC; cpos++) uu[cpos] = U[t*RS + cpos];
                    yy = U[t*RS + WC];
                };
                if constexpr (PF) ldrows(nbc - 1, un, yn);
#pragma unroll 1
                for (int kb = nbc - 1; kb >= NB; kb--) {
                    const int k = kb - NB;
                    if constexpr (PF) {
#pragma unroll
                        for (int cpos = 0; cpos < WC; cpos++) u[cpos] = un[cpos];
                        y = yn;
                        if (kb > NB) ldrows(kb - 1, un, yn);             // the next block's rows travel under this block's arithmetic
                    } else ldrows(kb, u, y);
                    double s = y;
#pragma unroll
                    for (int cpos = N2; cpos < WC; cpos++) {
                        const int gc = k*N2 + cpos;
                        s = fma(-u[cpos], gc < n ? xs[gc] : 0.0, s);
                    }
                    double dg = 1.0;                                     // my row's diagonal entry: window column = my pivot step in the block
#pragma unroll
                    for (int jj = 0; jj < N2; jj++) dg = lane == jj ? u[jj] : dg;
                    const double rd = blu_rcp(dg);                       // (all rows at once; the chain below only multiplies)
                    double xv = 0.0;
                    blu_static_for<0, N2>([&](auto jr) {
                        constexpr int jj = N2 - 1 - jr.value;
                        const double xj = readlane_f64(s*rd, jj);
                        xv = lane == jj ? xj : xv;
                        s = fma(-u[jj], xj, s);                          // (lanes >= jj: no longer read)
                    });
                    __syncthreads();
                    if (lane < N2) xs[k*N2 + lane] = xv;
                    __syncthreads();
                }
            };
            __syncthreads();
            backsub(s_x);
            if (a.stop == 2) continue;

            double nr2, na2, nf2;
            residual(s_x, s_r, nr2, na2, nf2);
            __syncthreads();
            if (a.stop == 3) continue;

            // ================= one refinement step: the elimination replayed on r alone =================
            {
                double bb; bool al; int mt = -1;
                {
                    const int r0 = lane - NB*N2;
                    bb = (r0 >= 0 && r0 < N2) ? s_r[r0] : 0.0;
                    al = lane < NR;
                }
                double mm[N2], mn[N2];
#pragma unroll
                for (int jj = 0; jj < N2; jj++) mn[jj] = M[(size_t)jj*64 + lane];
#pragma unroll 1
                for (int kb = 0; kb < nbc; kb++) {
#pragma unroll
                    for (int jj = 0; jj < N2; jj++) mm[jj] = mn[jj];
                    if (kb + 1 < nbc) {
#pragma unroll
                        for (int jj = 0; jj < N2; jj++) mn[jj] = M[((size_t)(kb + 1)*N2 + jj)*64 + lane];
                    }
                    int pv[N2];
#pragma unroll
                    for (int jj = 0; jj < N2; jj++) pv[jj] = (int)s_piv[kb*N2 + jj];      // (one LDS round trip per block, not per step)
                    blu_static_for<0, N2>([&](auto jjc) {
                        constexpr int jj = jjc.value;
                        const int t = kb*N2 + jj;
                        const int p = __builtin_amdgcn_readfirstlane(pv[jj]);
                        bb = fma(-mm[jj], readlane_f64(bb, p), bb);
                        if (lane == p) { al = false; mt = t; }
                    });
                    const bool ret = mt >= 0;
                    if (ret) U[(size_t)mt*RS + WC] = bb;
                    const unsigned long long rm = __ballot(ret);
                    const int rank = __popcll(rm & ((1ull << lane) - 1ull));
                    const bool enter = ret && kb + 1 < nk;
                    if (ret) bb = enter ? s_r[(kb + 1)*N2 + rank] : 0.0;
                    al = ret ? enter : al;
                    mt = -1;
                }
                (void)al;
                __syncthreads();
                if (a.stop == 4) continue;
                backsub(s_dx);
            }
            double d2 = 0.0, x2 = 0.0;
#pragma unroll 1
            for (int i = lane; i < n; i += 64) {
                const double dx = s_dx[i], xv = s_x[i] + dx;
                s_x[i] = xv;
                d2 = fma(dx, dx, d2); x2 = fma(xv, xv, x2);
            }
            d2 = wave_sum(d2); x2 = wave_sum(x2);
            __syncthreads();
            // verification: the normwise backward error of the LU solve itself (the residual above, taken BEFORE the refinement step, which can
            // only lower it -- a second residual pass would cost as much as the back substitution) and a sane, finite correction
            const double eta = sqrt(nr2)/(sqrt(na2)*sqrt(x2) + sqrt(nf2));
            const double rat = x2 > 0.0 ? sqrt(d2/x2) : (d2 == 0.0 ? 0.0 : 1.0/0.0);
            const bool ok = eta <= 1.0e-12 && rat < 0.5 && x2 < 1.0/0.0;       // (NaN fails every comparison)
            if (ok) {
#pragma unroll 1
                for (int i = lane; i < n; i += 64) de[i] = s_x[i];
            }
            if (lane == 0) {
                if (ok) {
                    a.ratio[e] = rat; a.stat[1 + e] = 3;
                    if (st0 == 1) atomicSub(a.stat, 1);
                } else if (st0 != 1) {                                   // (mode 2 on a column the block sweep had resolved: it keeps d and status)
                } else {
                    a.ratio[e] = rat == rat ? fmax(rat, a.ratio[e]) : rat;      // stays flagged; a NaN ratio says why
                }
            }
            __syncthreads();
        }
    }
}

// mimsem_column_flag_for_test: the listed columns join the flagged ones (status 0 -> 1, counted)
__global__ void k_force_flags(int* stat, const int* cols, int n, int nEl) {
    const int i = blockIdx.x*blockDim.x + threadIdx.x;
    if (i < n && stat[1 + cols[i]] == 0) { stat[1 + cols[i]] = 1; const int pos = atomicAdd(stat + nEl + 1, 1); stat[nEl + 2 + pos] = cols[i]; atomicAdd(stat, 1); }
}

// re-solve the flagged columns of the solve that just ran (L, f, d: what that solve was given; the status is the context's)
int launch_band_lu_flagged(mimsem_ctx* c, int nb, const double* L, bool rowmajor, const double* f, double* d) {
    if (c->n_forceflag > 0 && c->d_forceflag && c->d_colstat) {
        hipLaunchKernelGGL(k_force_flags, dim3((unsigned)((c->n_forceflag + 255)/256)), dim3(256), 0, c->stream, c->d_colstat, c->d_forceflag, c->n_forceflag, c->nEl);
        c->n_forceflag = 0;
    }
    if (!c->pivot_fallback || c->nEl == 0) return MIMSEM_OK;
    const int n2 = c->es.n2e, nk = c->nk;
    const long long n = (long long)nk*n2;
    if (n > BANDLU_NMAX || n2 > 16 || c->es.n > 4 || nk < 1) return MIMSEM_OK;      // beyond what the kernel holds: the columns stay flagged
    const long long nsteps = (long long)(nk + nb)*n2, per = nsteps*((2*nb + 1)*n2 + 1) + nsteps*64;
    // mode 1: 64 wavefronts stride over whatever is flagged (the usual handful finds a wavefront each); mode 2: every column -- as many
    // wavefronts as 256 MB of workspace allow
    int grid = c->pivot_fallback == 2 ? (int)std::max(64LL, std::min<long long>(1024, (256LL << 20)/(per*8))) : 64;
    grid = std::max(1, std::min(grid, c->nEl));
    const long long need = per*grid;
    if (int rc = c->grow(c->d_lu, c->lu_doubles, need)) return rc;      // (MIMSEM_ERR_STATE in a capture: warm the solve up outside it)
    BandLUArgs a{};
    a.nEl = c->nEl; a.nk = nk; a.rs = rowmajor ? n2 : 1; a.js = rowmajor ? 1 : n2; a.all = c->pivot_fallback == 2;
    a.L = L; a.f = f; a.d = d; a.stat = c->d_colstat; a.ratio = c->d_colratio;
    a.W = c->d_lu; a.per = per;
    a.stop = c->blu_stop;
    if (for_order<1, 4, 9, 16>(n2, [&](auto N2) { return for_order<1, 2>(nb, [&](auto NB) {      // block size x half bandwidth in blocks
            hipLaunchKernelGGL((k_band_lu_wave<N2(), NB()>), dim3((unsigned)grid), dim3(64), 0, c->stream, a); }); })) return MIMSEM_OK;
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

}  // namespace
