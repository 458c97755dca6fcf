// column_dpp.inc -- included by column_kernels.hip (same translation unit: shares CG, plan_col, for_order, VSCALE, RD, CV, ...).
//
// Round 2: the column Schur path on an LDS-FREE block algebra.
//
// A block lives in registers with ONE ROW PER LANE of a 16-lane DPP row (four independent tasks per wavefront).  A product
// C = A . B needs, in lane r, row m of B for every m -- and gfx90a+ has exactly one DPP control that works on 64-bit VALU
// operations:  v_fmac_f64_dpp  vdst, vsrc0, vsrc1  row_newbcast:m   reads src0 from lane m of the caller's 16-lane row.  So
//       C[r][j] += A[r][m] * B[m][j]      is ONE instruction:    v_fmac_f64_dpp C_j, B_j, A_m row_newbcast:m
// with both operands in registers: no LDS publish, no LDS read per FMA, no wave-level sync.  Measured against round 1's
// "right-hand operand in LDS" form and against v_mfma_f64_16x16x4 on zero-padded blocks: 3.2x / 2.0x faster at 9x9, 4.2x / a
// tie at 16x16 (profiles/r02_block_product_ab.txt; the matrix core runs FP64 at the vector rate on gfx950, so padding 9 -> 16
// only costs).  The same control turns the Gauss-Jordan sweep of a symmetric positive definite block (every mass block
// W^T diag(c) W, c > 0, is one) into broadcasts of lane c at step c -- no pivot search, no bpermute, no un-permute through LDS --
// and makes "interpolate a distributed vector to my quadrature point" / "assemble my row of W^T diag(c) W from coefficients held one
// per lane" pure register code.
//
// Rules the code below keeps (checked on the generated ISA by scripts/check_dpp_hazards.py, tests/test_dpp_hazards.py):
//   * a DPP read of a VGPR needs two wait states after a VALU write of it, and hipcc pads nothing around inline asm: every DPP
//     source operand goes through launder() (an asm that owns the registers and issues s_nop 1) right before its first DPP use;
//   * all 16 lanes of a row stay active (EXEC all ones): predication is by data (rows >= N2 mirror row N2-1 and are never stored).
//
// On top of it:  k_schur_sweep<N>  (one task = one column x a run of levels: every factor of solve_schur_column_eta,
// eul/VertSolve.cpp:677-823, and the three Helmholtz blocks of each level without a single intermediate block in memory),
// k_thomas_dpp<N2> (block-Thomas + one refinement step in one launch) and k_schur_backsub<N> (the back substitution from
// recomputed factors).  Three launches for what took 17.

namespace dpp {

template <int M>
__device__ __forceinline__ void fmac(double& acc, double mine, double theirs) {       // acc += mine * (theirs of lane M of my row)
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(theirs), "v"(mine), "n"(M));
}
// the compiler-visible form (v_mov_b64_dpp through the LLVM intrinsic: hazards handled by hipcc) for single values
extern "C" __device__ long mimsem_llvm_update_dpp_i64(long, long, int, int, int, bool) __asm("llvm.amdgcn.update.dpp.i64");
template <int M>
__device__ __forceinline__ double get(double v) {
    return __builtin_bit_cast(double, mimsem_llvm_update_dpp_i64(0L, __builtin_bit_cast(long, v), 0x150 + M, 0xf, 0xf, true));
}

// take ownership of the registers of v[0..K) and spend two wait states: the next DPP read of them is hazard-free
template <int K> struct Launder;
#define MIMSEM_LAUNDER(K, ...) template <> struct Launder<K> { static __device__ __forceinline__ void run(double* v) { asm volatile("s_nop 1" : __VA_ARGS__); } };
#define O_(i) "+v"(v[i])
MIMSEM_LAUNDER(1, O_(0))
MIMSEM_LAUNDER(2, O_(0), O_(1))
MIMSEM_LAUNDER(4, O_(0), O_(1), O_(2), O_(3))
MIMSEM_LAUNDER(9, O_(0), O_(1), O_(2), O_(3), O_(4), O_(5), O_(6), O_(7), O_(8))
MIMSEM_LAUNDER(16, O_(0), O_(1), O_(2), O_(3), O_(4), O_(5), O_(6), O_(7), O_(8), O_(9), O_(10), O_(11), O_(12), O_(13), O_(14), O_(15))
#undef O_
#undef MIMSEM_LAUNDER
template <int K> __device__ __forceinline__ void launder(double (&v)[K]) { Launder<K>::run(v); }
__device__ __forceinline__ void launder1(double& v) { asm volatile("s_nop 1" : "+v"(v)); }

// compile-time loops over the broadcast lane
template <int M, int END, class F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (M < END) { f(std::integral_constant<int, M>{}); static_for<M + 1, END>(f); }
}

// The primitives as whole asm blocks (round 4; generated: scripts/gen_dpp_blocks.py -> dpp_blocks.inc).  `s_nop 1` opens every block, so
// whatever the compiler does to the operands (copies out of AGPRs, scratch reloads) lands in front of the wait states a DPP read needs:
// hazard-free by construction, where the launder() + one-asm-per-instruction form of rounds 2-3 depended on the compiler leaving the
// source registers alone between the two (it does not under register pressure: scripts/check_dpp_hazards.py caught it at order 4).
template <int N2> struct MulAcc;          // C += A . B
template <int N2> struct MulSub;          // C -= A . B
template <int N2> struct MatvecAcc;       // y += A x
template <int N2> struct GjStep;          // T[.][j] += f T[c][j]
template <int K> struct DotAcc;           // s += sum_{j < K} W[j] f(lane j)
template <int N> struct AssembleU;        // u[q] += Ey[q / MP1] c(point q)
template <int N> struct AssembleDiagT;    // t[q % MP1] += EE[q / MP1] c(point q)
template <int N> struct ProjAcc;          // s += sum_q Wt[q] v(point q)
}  // namespace dpp
#include "dpp_blocks.inc"
namespace dpp {

// 1/x for a pivot of a Gauss-Jordan sweep: v_rcp_f64 + three Newton steps (7 dependent instructions; the IEEE division the compiler
// emits is ~15 with v_div_scale / v_div_fmas / v_div_fixup).  Pivots are finite, non-zero and far from the exponent limits (mass blocks
// scaled by SCALE / det); the result is within an ulp or two of the rounded quotient, far inside the 1e-10 parity bar.
__device__ __forceinline__ double pivot_rcp(double x) {
    double y = __builtin_amdgcn_rcp(x);
    y = fma(fma(-x, y, 1.0), y, y);
    y = fma(fma(-x, y, 1.0), y, y);
    y = fma(fma(-x, y, 1.0), y, y);
    return y;
}
// T <- T^-1 in place on the diagonal pivots, one row per lane, WITHOUT normalising the pivot rows on the way (round 4): step c
// subtracts m_r = T[r][c] / piv_c times the pivot row (row_newbcast:c) from every other row -- one fmac per entry, multiplier 0 in the pivot
// lane -- and leaves D B with D = diag(piv) where the normalising sweep of rounds 2-3 left B = T^-1; every lane keeps 1 / piv of its
// own row and scales it once at the end.  Saves the 9 multiplications per step of the scaling pass (and a select); same multipliers,
// same stability as before.  (A one-fmac form that scales the pivot row by 1 + (1/piv - 1) cancels for large pivots: not used.)
template <int N2>
__device__ __forceinline__ void gauss_jordan(double (&T)[N2], int r) {
    double mypinv = 1.0;
    static_for<0, N2>([&](auto cc) {
        constexpr int c = cc.value;
        launder1(T[c]);                              // (written by the previous step's asm: invisible to hipcc's DPP hazard check)
        const double pinv = pivot_rcp(get<c>(T[c]));
        const bool isp = r == c;
        const double f = isp ? 0.0 : -T[c]*pinv;
        mypinv = isp ? pinv : mypinv;
        GjStep<N2>::template run<c>(T, f);               // (entry c included: overwritten below)
        T[c] = isp ? 1.0 : f;
    });
#pragma unroll
    for (int j = 0; j < N2; j++) T[j] *= mypinv;
}

template <int N>
struct Rows {
    static constexpr int N2 = N*N, MP1 = N + 1, MP12 = MP1*MP1, NP = (MP12 + 15)/16;
    static_assert(N2 <= 16, "one block row per lane of a 16-lane DPP row");
    // layout of a block in the wavefront: NC columns of its row per lane, first column c0(lane), TPW tasks per wavefront
    static constexpr int NC = N2, TPW = 4;
    __device__ static __forceinline__ int c0(int) { return 0; }
    __device__ static __forceinline__ int task(int lane) { return lane/16; }

    // per-lane constants of the task geometry: my block row r = (iy, ix); my quadrature point(s) q = lane + 16 p
    struct Lane {
        double Ey[MP1], Ex[MP1];          // E[q][iy], E[q][ix]                     (edge table eul/Basis.cpp:235-283)
        double Wq[NP][N2];                // W[q][j] = E[qx][jx] E[qy][jy] of my points (ElMats.cpp:105-110)
    };
    __device__ static void init_lane(Lane& L, const double* E, const double* W, int r) {
        const int rr = r < N2 ? r : N2 - 1, iy = rr/N, ix = rr%N;
#pragma unroll
        for (int q = 0; q < MP1; q++) { L.Ey[q] = E[q*N + iy]; L.Ex[q] = E[q*N + ix]; }
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int q = min(r + 16*p, MP12 - 1);
#pragma unroll
            for (int j = 0; j < N2; j++) L.Wq[p][j] = W[q*N2 + j];
        }
    }

    // ---- products (all operands: my row in registers) ---------------------------------------------------------------
    // C = A . B
    __device__ static void mul(double (&C)[N2], const double (&A)[N2], const double (&B)[N2]) {
#pragma unroll
        for (int j = 0; j < N2; j++) C[j] = 0.0;
        MulAcc<N2>::run(C, A, B);
    }
    // C += A . B
    __device__ static void mul_add(double (&C)[N2], const double (&A)[N2], const double (&B)[N2]) { MulAcc<N2>::run(C, A, B); }
    // y_r = sum_m A[r][m] x[m]   (x distributed: lane m holds x[m])
    __device__ static double matvec(const double (&A)[N2], double x) {
        double y = 0.0;
        MatvecAcc<N2>::run(y, A, x);
        return y;
    }
    __device__ static double matvec(const double (&A)[N2], double x, int /*lane*/) { return matvec(A, x); }      // (the signature of the half-row layout)
    // value at my quadrature point(s) of a 2-form given by its distributed dofs: sum_j W[q][j] f[j]  (the rk/tb/wb loops of VertOps.cpp)
    __device__ static void interp(double (&out)[NP], const Lane& L, double f) {
#pragma unroll
        for (int p = 0; p < NP; p++) {
            double s = 0.0;
            MatvecAcc<N2>::run(s, L.Wq[p], f);
            out[p] = s;
        }
    }
    // my row of W^T diag(c) W; c held one per lane: c[p] belongs to quadrature point q = lane + 16 p.  Sum-factorised:
    //   u[qy][qx] = E[qy][iy] c[qy][qx];  t[qx][jy] = sum_qy u[qy][qx] E[qy][jy];  M[jy][jx] = sum_qx (E[qx][ix] t[qx][jy]) E[qx][jx]
    __device__ static void assemble(double (&M)[N2], const Lane& L, const double* __restrict__ E /* uniform: SGPRs */, const double (&c)[NP]) {
        double u[MP12];
#pragma unroll
        for (int q = 0; q < MP12; q++) u[q] = 0.0;
        AssembleU<N>::run(u, L.Ey, c);
        double t[MP1][N];
#pragma unroll
        for (int qx = 0; qx < MP1; qx++)
#pragma unroll
            for (int jy = 0; jy < N; jy++) t[qx][jy] = 0.0;
#pragma unroll
        for (int q = 0; q < MP12; q++) {
            const int qy = q/MP1, qx = q%MP1;
#pragma unroll
            for (int jy = 0; jy < N; jy++) t[qx][jy] += u[q]*E[qy*N + jy];
        }
#pragma unroll
        for (int j = 0; j < N2; j++) M[j] = 0.0;
#pragma unroll
        for (int qx = 0; qx < MP1; qx++)
#pragma unroll
            for (int jy = 0; jy < N; jy++) {
                const double w = L.Ex[qx]*t[qx][jy];
#pragma unroll
                for (int jx = 0; jx < N; jx++) M[jy*N + jx] += w*E[qx*N + jx];
            }
    }
    // my diagonal entry of W^T diag(c) W: sum_q W[q][r]^2 c[q]
    __device__ static double assemble_diag(const Lane& L, const double (&c)[NP]) {
        double t[MP1], EE[MP1];
#pragma unroll
        for (int qx = 0; qx < MP1; qx++) { t[qx] = 0.0; EE[qx] = L.Ey[qx]*L.Ey[qx]; }
        AssembleDiagT<N>::run(t, EE, c);
        double s = 0.0;
#pragma unroll
        for (int qx = 0; qx < MP1; qx++) s += (L.Ex[qx]*L.Ex[qx])*t[qx];
        return s;
    }
    // T <- T^-1 in place, Gauss-Jordan WITHOUT pivoting (the reference's Inv, eul/LinAlg.cpp:186-269, pivots; for the symmetric
    // positive definite mass blocks the diagonal pivots are safe and the results agree to round-off): gauss_jordan() below
    __device__ static void inverse(double (&T)[N2], int r) { gauss_jordan<N2>(T, r); }
    // D[r][j] = V[r][j] * x[j]  (column scaling by a distributed vector): x of lane j through the compiler-visible DPP move
    __device__ static void col_scale(double (&D)[N2], const double (&V)[N2], double x) {
        static_for<0, N2>([&](auto j) { D[j.value] = V[j.value]*get<j.value>(x); });
    }
};

// ---- round 5: the HALF-ROW layout of the 16 x 16 blocks of order 4 --------------------------------------------------------------------
// A block row lives in TWO lanes: lane (h, r) of DPP row 2t + h holds columns 8h .. 8h + 7 of row r of task t -- 16 VGPRs per block and
// lane instead of 32, two tasks per wavefront instead of four.  Why: the walks of solve_schur_column_3 keep ~20 blocks alive; at 32 VGPRs
// each they do not fit the 512 registers of a lane and k_s3_sweep<4> ran with ~700 spilled dwords per lane (5.9 GB of scratch traffic per
// launch, 3.9x its designed output: round-4 verdict).  At 16 VGPRs per block the walk fits.  Price: a product needs all 16 multipliers
// A[r][m] in both lanes of a row -- the halves are exchanged with v_permlane16_swap_b32 (gfx950: vdst rows {1, 3} <-> vsrc rows {0, 2};
// both operands the same value v gives {v of half 0 in both halves, v of half 1 in both halves} with no select), 32 instructions for the
// 8 doubles of an operand in front of 128 DPP FMAs (16-lane layout: 256 FMAs for twice the tasks: +37 % VALU work per product).
// Everything that is a VECTOR (one entry per block row: fields, right-hand sides, coefficients at quadrature points) is held replicated in
// both halves, so the quadrature-point algebra (interp / assemble's first stage) is the 16-lane code unchanged; a matrix-vector product
// sums its half's 8 columns (row_mask picks the DPP rows of a half: the broadcast lane 8h + jj differs) and adds the two partial sums in
// the fixed order half 0 + half 1 in both lanes: replicated, identical bits.
__device__ __forceinline__ void xsplit(double v, double& from_h0, double& from_h1) {
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    from_h0 = __hiloint2double((int)b[0], (int)a[0]);
    from_h1 = __hiloint2double((int)b[1], (int)a[1]);
}
// A value an inline-asm block wrote (the DPP FMA blocks) is, for hipcc's hazard recogniser, not the result of a VALU instruction: the wait
// states a cross-lane read needs after a VALU write (DPP: 2; v_permlane16_swap: taken as 4 here) are spent explicitly before the exchange.
__device__ __forceinline__ void launder_x(double& v) { asm volatile("s_nop 3" : "+v"(v)); }
__device__ __forceinline__ void launder_x8(double (&v)[8]) {
    asm volatile("s_nop 3" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
}
__device__ __forceinline__ double xsum(double part) { launder_x(part); double p0, p1; xsplit(part, p0, p1); return p0 + p1; }
// a replicated vector as half h needs it for sums over its own 8 columns: lane jj < 8 of my row holds x[8h + jj] (half 1: the row rotated by
// 8 lanes, two 32-bit DPP moves).  (row_mask on the 64-bit DPP FMA itself -- broadcast lane jj in the rows of half 0, 8 + jj in those of half
// 1 -- was tried first: the masked instructions contribute nothing on gfx950; scripts/exp/rows_half_probe.py.)
__device__ __forceinline__ double half_shift(double v, int h) {
    const double rot = __builtin_bit_cast(double, mimsem_llvm_update_dpp_i64(0L, __builtin_bit_cast(long, v), 0x128, 0xf, 0xf, true));     // row_ror:8
    return h ? rot : v;
}
// x of lane 8h + JJ of my row (x replicated in both halves)
template <int JJ>
__device__ __forceinline__ double getH(double v, int h) { return get<JJ>(half_shift(v, h)); }

struct RowsH {
    static constexpr int N = 4, N2 = 16, MP1 = 5, MP12 = 25, NP = 2, NC = 8, TPW = 2;
    __device__ static __forceinline__ int c0(int lane) { return ((lane >> 4) & 1)*8; }
    __device__ static __forceinline__ int task(int lane) { return lane/32; }
    struct Lane {
        double Ey[MP1], Ex[MP1];          // E[q][iy], E[q][ix] of my row r = (iy, ix)
        double Ejy[MP1][2];               // E[qy][2h + jyl]: the two jy my 8 columns (jy = 2h + jyl, jx = 0..3) belong to
        double Wq[NP][NC];                // W[q][8h + jj] of my quadrature points q = r + 16 p: the two halves of a row share the 16-term sums of interp()
        int h;
    };
    __device__ static void init_lane(Lane& L, const double* E, const double* W, int lane) {
        const int r = lane%16, h = (lane >> 4) & 1, iy = r/N, ix = r%N;
        L.h = h;
#pragma unroll
        for (int q = 0; q < MP1; q++) { L.Ey[q] = E[q*N + iy]; L.Ex[q] = E[q*N + ix]; L.Ejy[q][0] = E[q*N + 2*h]; L.Ejy[q][1] = E[q*N + 2*h + 1]; }
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int q = min(r + 16*p, MP12 - 1);
#pragma unroll
            for (int j = 0; j < NC; j++) L.Wq[p][j] = W[q*N2 + 8*h + j];
        }
    }
    // all 16 multipliers of my row: Af[m] = A[r][m]
    __device__ static __forceinline__ void expand(double (&Af)[N2], const double (&A)[NC]) {
        launder_x8(const_cast<double (&)[NC]>(A));       // (values unchanged; every caller's A is a non-const register array)
#pragma unroll
        for (int jj = 0; jj < NC; jj++) xsplit(A[jj], Af[jj], Af[NC + jj]);
    }
    __device__ static void mul(double (&C)[NC], const double (&A)[NC], const double (&B)[NC]) {
        double Af[N2];
        expand(Af, A);
#pragma unroll
        for (int j = 0; j < NC; j++) C[j] = 0.0;
        MulAccH::run(C, Af, B);
    }
    __device__ static void mul_add(double (&C)[NC], const double (&A)[NC], const double (&B)[NC]) {
        double Af[N2];
        expand(Af, A);
        MulAccH::run(C, Af, B);
    }
    // y_r = sum_m A[r][m] x[m], x replicated, y replicated
    __device__ static double matvec(const double (&A)[NC], double x, int lane) {
        double y = 0.0, xs = half_shift(x, (lane >> 4) & 1);
        launder1(xs);
        DotAcc<NC>::template run<0>(y, A, xs);
        return xsum(y);
    }
    // value at my quadrature point(s) of a 2-form given by its (replicated) dofs: each half sums its 8 of the 16 terms, the partial sums
    // are added in the order half 0 + half 1 in both lanes (32 registers of table per lane instead of 64)
    __device__ static void interp(double (&out)[NP], const Lane& L, double f) {
        double fs = half_shift(f, L.h);
        launder1(fs);
#pragma unroll
        for (int p = 0; p < NP; p++) {
            double s = 0.0;
            DotAcc<NC>::template run<0>(s, L.Wq[p], fs);
            out[p] = xsum(s);
        }
    }
    // my 8 columns of my row of W^T diag(c) W (c replicated: c[p] of quadrature point q = r + 16 p).  Same sum factorisation as Rows<4>,
    // the last two stages only for jy = 2h, 2h + 1.
    __device__ static void assemble(double (&M)[NC], const Lane& L, const double* __restrict__ E /* uniform */, const double (&c)[NP]) {
        double u[MP12];
#pragma unroll
        for (int q = 0; q < MP12; q++) u[q] = 0.0;
        AssembleU<N>::run(u, L.Ey, c);
        double t[MP1][2];
#pragma unroll
        for (int qx = 0; qx < MP1; qx++) { t[qx][0] = 0.0; t[qx][1] = 0.0; }
#pragma unroll
        for (int q = 0; q < MP12; q++) {
            const int qy = q/MP1, qx = q%MP1;
            t[qx][0] += u[q]*L.Ejy[qy][0]; t[qx][1] += u[q]*L.Ejy[qy][1];
        }
#pragma unroll
        for (int j = 0; j < NC; j++) M[j] = 0.0;
#pragma unroll
        for (int qx = 0; qx < MP1; qx++)
#pragma unroll
            for (int jyl = 0; jyl < 2; jyl++) {
                const double w = L.Ex[qx]*t[qx][jyl];
#pragma unroll
                for (int jx = 0; jx < N; jx++) M[jyl*N + jx] += w*E[qx*N + jx];
            }
    }
    // T <- T^-1 in place, unpivoted Gauss-Jordan on the diagonal (mass blocks), non-normalising form of gauss_jordan<16>: column c of the
    // block lives in half c / 8 -- its entries (the pivot, every row's multiplier) cross to the other half once per step
    __device__ static void inverse(double (&T)[NC], int lane) {
        const int r = lane%16, h = (lane >> 4) & 1;
        double mypinv = 1.0;
        static_for<0, N2>([&](auto cc) {
            constexpr int c = cc.value, hc = c/NC, cj = c%NC;
            double v0, v1;
            launder_x(T[cj]);                            // (written by the previous step's asm)
            xsplit(T[cj], v0, v1);
            double col = hc ? v1 : v0;                   // T[r][c] in both halves
            launder1(col);
            const double pinv = pivot_rcp(get<c>(col));
            const bool isp = r == c;
            const double f = isp ? 0.0 : -col*pinv;
            mypinv = isp ? pinv : mypinv;
            GjStepH::template run<c>(T, f);
            T[cj] = (h == hc) ? (isp ? 1.0 : f) : T[cj];
        });
#pragma unroll
        for (int j = 0; j < NC; j++) T[j] *= mypinv;
    }
};

}  // namespace dpp

namespace {

// ---- solve_schur_column_eta, fused --------------------------------------------------------------------------------------------
struct SweepArgs {
    int nEl, nk, chunk, nchunk;
    const double *det, *tI, *th, *w, *W, *Eg;       // geometry (ctx layout), dense W table [mp12][n2], edge table [mp1][n] in memory
    double E[20];                                  // the edge table again as kernel arguments: uniform, compile-time indexed -> scalar registers
    double hdt, gam;
    const double *theta, *rho, *eta, *pi;           // [nEl][nk][n2]
    const double *F_u; double *F_pi; const double *F_eta, *F_rho;     // right-hand sides (F_pi updated in place) or all null
    double *L;                                      // [nEl][nk][3][nn]; within a block row-major (rowmajor = 1: the ABI's layout) or
    int rowmajor;                                   // LANE-major [j][r] (internal): the 16 lanes of a task then store 72 contiguous bytes per instruction
    int* statz;                                     // null, or the unconverged-column counter of the solve that follows: zeroed here (a memset launch less)
    double *rl, *geta, *fu2;                        // [nEl][nk-1][n2]: lumped inverse of L_eta, entropy gradient, updated F_u (for the back substitution;
                                                    // F_u itself stays untouched here: the task below reads the interface it shares with this one)
};

template <int N>
struct SchurCol {
    using R = dpp::Rows<N>;
    static constexpr int N2 = R::N2, nn = N2*N2, NP = R::NP, MP12 = R::MP12;
    // what a column level carries from one interface to the next
    struct Lev {
        double B[N2], Bi[N2], Nrho[N2], Ld[N2];     // VB, VB^-1, N_rho, running diagonal block of the Helmholtz row (starts as N_pi)
        double pi, eta, tE, fpi;                    // distributed vectors: fields, VB^-1 F_eta, running F_pi row
        double thI[NP], rhI[NP], tI[NP], th[NP];    // at my quadrature point(s): theta, rho interpolated; thickness inverse, thickness
    };
    struct Geo { double q0[NP], det[NP]; };

    // the memory reads of a level, issued one interface ahead of their use (the kernel runs one wavefront per SIMD: nothing else hides them)
    struct Raw { double tI[NP], th[NP], pi, eta, rho, theta, feta, frho, fpi; };
    __device__ static void load(Raw& W, const SweepArgs& a, int e, int k, int lane_r, int rr) {
        const int nk = a.nk;
        const size_t vo = ((size_t)e*nk + k)*N2 + rr;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int q = min(lane_r + 16*p, MP12 - 1);
            const size_t go = ((size_t)k*a.nEl + e)*MP12 + q;
            W.tI[p] = a.tI[go]; W.th[p] = a.th[go];
        }
        W.pi = a.pi[vo]; W.eta = a.eta[vo]; W.rho = a.rho[vo]; W.theta = a.theta[vo];
        W.feta = a.F_eta ? a.F_eta[vo] : 0.0; W.frho = a.F_rho ? a.F_rho[vo] : 0.0; W.fpi = a.F_pi ? a.F_pi[vo] : 0.0;
    }
    // level k: VB, VB^-1 and -- for rows this task owns -- the EOS blocks N_pi = B B(pi)^-1 B, N_rho (Assemble_EOS_Block, VertOps.cpp:1144-1202)
    __device__ static void level(Lev& V, const SweepArgs& a, const typename R::Lane& Ln, const Geo& G, const Raw& W, int lane_r, bool full) {
#pragma unroll
        for (int p = 0; p < NP; p++) { V.tI[p] = W.tI[p]; V.th[p] = W.th[p]; }
        V.pi = W.pi; V.eta = W.eta;
        const double rho = W.rho, theta = W.theta;
        R::interp(V.thI, Ln, theta);
        R::interp(V.rhI, Ln, rho);
        double c[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = G.q0[p]*V.tI[p];                                     // AssembleConst :201-209
        R::assemble(V.B, Ln, a.E, c);
#pragma unroll
        for (int j = 0; j < N2; j++) V.Bi[j] = V.B[j];
        R::inverse(V.Bi, lane_r);                                                                 // AssembleConstInv :803-807
        V.tE = a.F_eta ? R::matvec(V.Bi, W.feta) : 0.0;                                           // VB^-1 F_eta (:772)
        V.fpi = 0.0;
        if (!full) return;
        double piI[NP];
        R::interp(piI, Ln, V.pi);
        double P[N2], t1[N2];
#pragma unroll 1
        for (int which = 0; which < 2; which++) {
#pragma unroll
            for (int p = 0; p < NP; p++) c[p] = (G.q0[p]*V.tI[p])*((which ? V.rhI[p] : piI[p])/(V.th[p]*G.det[p]));      // AssembleConstWithRho :508-521
            R::assemble(P, Ln, a.E, c);
            R::inverse(P, lane_r);
            R::mul(t1, P, V.B);                                                                   // B(f)^-1 B
            if (which) R::mul(V.Nrho, V.B, t1); else R::mul(V.Ld, V.B, t1);                       // B (B(f)^-1 B)
        }
        if (a.F_pi) {
            const double tR = R::matvec(V.Bi, W.frho);                                            // VB^-1 F_rho
            double f = -1.0*W.fpi;                                                                // :775
            f += (-1.0*a.gam)*R::matvec(V.Nrho, tR);                                              // :778-779  CM F_rho, CM = N_rho VB^-1
            f += (-1.0*a.gam)*W.feta;                                                             // :780
            V.fpi = f;
        }
    }
};

// Task mapping of the chunked column walks (k_schur_sweep, k_schur_backsub, k_s3_sweep, k_s3_backsub): the four tasks of a wavefront are
// four COLUMNS of the same chunk of levels, so the chunk, the rows a task owns and the trip count of its walk are wave-uniform (SGPRs,
// scalar loops and branches).  Rounds 2-4 dealt (column, chunk) pairs out in task order: lane-varying bounds, divergent loops, and -- in
// k_s3_sweep<4> -- spills lost in a divergent region (column_schur3_sweep.inc).  -DMIMSEM_TASKMAP_OLD keeps the old order for A/B runs.
// COLMAJOR = the old order, kept where it measures better: k_s3_backsub<4> re-reads the blocks of the interface below its first level, which
// the neighbouring task of the same wavefront has just loaded (178 against 205-212 us, profiles/r04_taskmap_ab.txt).
struct WalkTask { int e, ch; bool live; };
template <bool COLMAJOR = false, int TPW = 4>           // TPW tasks per wavefront: 4 (a block row per lane of a 16-lane DPP row) or 2 (dpp::RowsH)
__device__ __forceinline__ WalkTask walk_task(int nEl, int nchunk, int lane) {
#ifdef MIMSEM_TASKMAP_OLD
    constexpr bool CM = true;
#else
    constexpr bool CM = COLMAJOR;
#endif
    if (CM) {
        const long long task0 = (long long)blockIdx.x*TPW + lane/(64/TPW), ntask = (long long)nEl*nchunk;
        const long long task = task0 < ntask ? task0 : ntask - 1;
        return {(int)(task/nchunk), (int)(task%nchunk), task0 < ntask};
    }
    const int wpc = (nEl + TPW - 1)/TPW;                                // wavefronts per chunk
    const int e0 = (int)(blockIdx.x%wpc)*TPW + lane/(64/TPW);
    return {min(e0, nEl - 1), (int)(blockIdx.x/wpc), e0 < nEl};         // a task beyond the last column repeats it: same addresses, same values
}
inline unsigned walk_task_grid(int nEl, int nchunk, bool colmajor = false, int tpw = 4) {
#ifdef MIMSEM_TASKMAP_OLD
    colmajor = true;
#endif
    return colmajor ? (unsigned)(((long long)nEl*nchunk + tpw - 1)/tpw) : (unsigned)(((nEl + tpw - 1)/tpw)*nchunk);
}

// One task = column e, levels [k0, k1).  The task walks the interfaces i = k0-1 .. k1-1 (the first one is a halo shared with
// the task below, recomputed rather than communicated); at interface i it holds levels i and i+1, forms every interface factor
// (A^-1, X, grad pi, grad eta, the G_pi row, the lumped inverse of L_eta, both DIV blocks) and adds its share to rows i and i+1.
template <int N>
__global__ __launch_bounds__(64) void k_schur_sweep(SweepArgs a) {
    using SC = SchurCol<N>; using R = dpp::Rows<N>;
    constexpr int N2 = R::N2, nn = SC::nn, NP = R::NP, MP12 = R::MP12, MP1 = R::MP1;
    const int lane = threadIdx.x, r = lane%16;
    if (a.statz && blockIdx.x == 0 && lane == 0) { a.statz[0] = 0; a.statz[a.nEl + 1] = 0; }      // (the Thomas launch behind this one counts into them: unresolved columns, length of the flagged list)
    const WalkTask tk = walk_task(a.nEl, a.nchunk, lane);
    const bool live = tk.live;
    const int e = tk.e, ch = tk.ch;
    const int nk = a.nk, nm = nk - 1;
    const int k0 = ch*a.chunk, k1 = min(nk, k0 + a.chunk);
    const int rr = r < N2 ? r : N2 - 1;
    const bool act = live && r < N2;
    const double hdt = a.hdt, gam = a.gam;
    const int js = a.rowmajor ? 1 : N2;             // stride between the elements of my block row in L

    typename R::Lane Ln;
    R::init_lane(Ln, a.Eg, a.W, r);
    typename SC::Geo G;
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const int q = min(r + 16*p, MP12 - 1);
        G.det[p] = a.det[(size_t)e*MP12 + q];
        G.q0[p] = (a.w[q%MP1]*a.w[q/MP1])*(VSCALE/G.det[p]);
    }

    typename SC::Lev V0, V1;
    const int i0 = k0 > 0 ? k0 - 1 : 0, i1 = min(k1 - 1, nm - 1);      // interfaces walked (i1 < i0 only when nk == 1: excluded by the caller)
    typename SC::Raw W0, Wn;
    // Order 4 (round 4): a block is 32 VGPRs per lane and the walk spilled 166 of them to scratch -- FETCH 861 MB / WRITE 710 MB per launch
    // against 90 / 246 MB at order 3, the wavefronts parked on vmcnt 55 % of their cycles (profiles/r04_column_pmc_box.txt).  The two blocks
    // of a level that are only needed at the END of an interface step (N_rho and the running Helmholtz diagonal) wait in LDS instead:
    // two level sets x two blocks x N2 x 64 doubles = 32 KB per wavefront (one workgroup = one wavefront), columns conflict-free.
    constexpr bool PARK = N2 > 9;
    __shared__ double park[PARK ? 6*N2*64 : 1];
    auto park_st = [&](int slot, const double (&M)[N2]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < N2; j++) park[(slot*N2 + j)*64 + lane] = M[j];
    };
    auto park_ld = [&](int slot, double (&M)[N2]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < N2; j++) M[j] = park[(slot*N2 + j)*64 + lane];
    };
    int cur = 0;                                                         // level set (slots 2 cur, 2 cur + 1) of the UPPER level of the step
    SC::load(W0, a, e, i0, r, rr);
    SC::load(Wn, a, e, min(i0 + 1, nk - 1), r, rr);
    SC::level(V0, a, Ln, G, W0, r, i0 >= k0);
    if (PARK) { park_st(0, V0.Nrho); park_st(1, V0.Ld); park_st(4, V0.Bi); cur = 1; }
#pragma unroll 1
    for (int i = i0; i <= i1; i++) {
        const bool own0 = i >= k0, own1 = i + 1 < k1;                  // rows i / i+1 belong to this task
        W0 = Wn;
        SC::load(Wn, a, e, min(i + 2, nk - 1), r, rr);                  // the fields of level i+2 travel while interface i is assembled
        SC::level(V1, a, Ln, G, W0, r, own1);
        if (PARK) { park_st(2*cur, V1.Nrho); park_st(2*cur + 1, V1.Ld); park_st(4 + cur, V1.Bi); }
        double c[NP], Ai[N2], X[N2], AB0[N2], T[N2];
        // A^-1                                                       AssembleLinearInv :422-430
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = G.q0[p]*(0.5*(V0.th[p] + V1.th[p]));
        R::assemble(Ai, Ln, a.E, c);
        R::inverse(Ai, r);
        // X = VA_inv VA(rho)                                         AssembleLinearWithRT(rho, internal) :621-662, VertSolve.cpp:716-717
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = G.q0[p]*(0.5*V0.rhI[p]/G.det[p]) + G.q0[p]*(0.5*V1.rhI[p]/G.det[p]);
        R::assemble(T, Ln, a.E, c);
        R::mul(X, Ai, T);
        // gradients  g = A^-1 (B_{i+1} f_{i+1} - B_i f_i)            VertSolve.cpp:694-695, :700, :729
        const double gpi = R::matvec(Ai, R::matvec(V1.B, V1.pi) - R::matvec(V0.B, V0.pi));
        const double geta = R::matvec(Ai, R::matvec(V1.B, V1.eta) - R::matvec(V0.B, V0.eta));
        // G_pi row: G(i,i) = -h T A^-1 B_i, G(i,i+1) = +h T A^-1 B_{i+1}   (T = VA(theta), :709-711)
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = G.q0[p]*(0.5*V0.thI[p]/G.det[p]) + G.q0[p]*(0.5*V1.thI[p]/G.det[p]);
        R::assemble(T, Ln, a.E, c);
        double Gl[N2], Gu[N2];
        R::mul(AB0, T, Ai);                                            // (T A^-1) B: one product and one live block fewer than T (A^-1 B_i), T (A^-1 B_{i+1}) (round 4)
        R::mul(Gl, AB0, V0.B);
        R::mul(Gu, AB0, V1.B);
#pragma unroll
        for (int j = 0; j < N2; j++) { Gl[j] *= -hdt; Gu[j] *= hdt; }
        // C = CONLIN_W(grad eta) block of interface i (AssembleConLinWithW :551-600; the same block sits in rows i and i+1)
        double wI[NP], C[N2];
        R::interp(wI, Ln, geta);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = G.q0[p]*(0.5*wI[p]/G.det[p]);
        R::assemble(C, Ln, a.E, c);
        // lumped inverse of L_eta = VA - (G_rt VB_inv) A_eta: M1 = h (R^t_i Binv_i + R^b_{i+1} Binv_{i+1}) only meets the diagonal (:742-751)
        R::interp(wI, Ln, gpi);
        double Rt[N2], m[N2], fu = 0.0;
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = G.q0[p]*(0.5*wI[p]*(V0.thI[p]*V0.tI[p])/(G.det[p]*G.det[p]));      // AssembleConLinWithRhodPi :1323-1373, block (i,i)
        R::assemble(Rt, Ln, a.E, c);
        if (PARK) park_ld(4 + (cur ^ 1), V0.Bi);
        R::mul(m, Rt, V0.Bi);
        double su = R::matvec(Rt, V0.tE);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = G.q0[p]*(0.5*wI[p]*(V1.thI[p]*V1.tI[p])/(G.det[p]*G.det[p]));      // block (i+1,i)
        R::assemble(Rt, Ln, a.E, c);
        if (PARK) park_ld(4 + cur, V1.Bi);
        R::mul_add(m, Rt, V1.Bi);
        su += R::matvec(Rt, V1.tE);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < N2; k++) s += (hdt*m[k])*(hdt*C[k]);                    // (M1 . h C)[r][r]; C is symmetric
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = G.q0[p]*(0.5*V0.th[p]) + G.q0[p]*(0.5*V1.th[p]);                 // AssembleLinear :242-267
        const double va = R::assemble_diag(Ln, c);
        const double rl = 1.0/(-1.0*s + va);
        const size_t io = ((size_t)e*nm + i)*N2 + rr;
        if (a.F_u) fu = a.F_u[io] + -1.0*(hdt*su);                                 // F_u -= (G_rt VB_inv) F_eta  (:772-773)
        if (act && own0) { a.rl[io] = rl; a.geta[io] = geta; a.fu2[io] = fu; }
        // DIV blocks of rows i and i+1 at this interface, column-scaled by the lumped inverse (:754-761), and the Helmholtz blocks (:766-767)
        double D[N2], tt[N2];
        if (own0) {
            if (PARK) { park_ld(2*(cur ^ 1), V0.Nrho); park_ld(2*(cur ^ 1) + 1, V0.Ld); }
            R::mul(tt, V0.Nrho, X);
#pragma unroll
            for (int j = 0; j < N2; j++) tt[j] = (hdt*tt[j] + hdt*C[j]);
            R::col_scale(D, tt, rl);                                               // DIV(i,i)
            R::mul(tt, D, Gl);
#pragma unroll
            for (int j = 0; j < N2; j++) V0.Ld[j] += (-1.0*gam)*tt[j];             // L(i,i) complete
            V0.fpi += gam*R::matvec(D, fu);
            double* Lk = a.L + ((size_t)e*nk + i)*3*nn + (a.rowmajor ? rr*N2 : rr);
            if (act) {
#pragma unroll
                for (int j = 0; j < N2; j++) Lk[nn + j*js] = V0.Ld[j];
                if (i == 0) {
#pragma unroll
                    for (int j = 0; j < N2; j++) Lk[j*js] = 0.0;                   // no block left of the first row
                }
                if (a.F_pi) a.F_pi[((size_t)e*nk + i)*N2 + rr] = V0.fpi;
            }
            R::mul(tt, D, Gu);
            if (act) {
#pragma unroll
                for (int j = 0; j < N2; j++) Lk[2*nn + j*js] = (-1.0*gam)*tt[j];   // L(i,i+1)
            }
        }
        if (own1) {
            if (PARK) { park_ld(2*cur, V1.Nrho); park_ld(2*cur + 1, V1.Ld); }
            R::mul(tt, V1.Nrho, X);
#pragma unroll
            for (int j = 0; j < N2; j++) tt[j] = (-hdt*tt[j] + hdt*C[j]);
            R::col_scale(D, tt, rl);                                               // DIV(i+1,i)
            R::mul(tt, D, Gl);
            double* Lk = a.L + ((size_t)e*nk + i + 1)*3*nn + (a.rowmajor ? rr*N2 : rr);
            if (act) {
#pragma unroll
                for (int j = 0; j < N2; j++) Lk[j*js] = (-1.0*gam)*tt[j];          // L(i+1,i)
            }
            R::mul(tt, D, Gu);
#pragma unroll
            for (int j = 0; j < N2; j++) V1.Ld[j] += (-1.0*gam)*tt[j];
            V1.fpi += gam*R::matvec(D, fu);
            if (PARK) park_st(2*cur + 1, V1.Ld);
        }
        V0 = V1;
        cur ^= 1;
    }
    // the last level of the column has no interface above it: its row is complete after interface nk-2
    if (k1 == nk) {
        double* Lk = a.L + ((size_t)e*nk + nk - 1)*3*nn + (a.rowmajor ? rr*N2 : rr);
        if (PARK) park_ld(2*(cur ^ 1) + 1, V0.Ld);
        if (act) {
#pragma unroll
            for (int j = 0; j < N2; j++) { Lk[nn + j*js] = V0.Ld[j]; Lk[2*nn + j*js] = 0.0; }
            if (a.F_pi) a.F_pi[((size_t)e*nk + nk - 1)*N2 + rr] = V0.fpi;
        }
    }
}

// ---- block-tridiagonal solve, 16 lanes per column: Thomas sweep + ONE step of iterative refinement in the same launch -----------------
// forward:  D'_k = T_k - S_k G_{k-1},  G_k = D'_k^-1 U_k,  y_k = D'_k^-1 (f_k - S_k y_{k-1});   backward: d_k = y_k - G_k d_{k+1}.
// Refinement: r = f - L d, solved with the kept factors (D'^-1_k, G_k), d += dd.  The sweep eliminates block by block without
// pivoting across blocks, which loses digits on the worst-conditioned columns (round 1: backward error 1.8e-6 on the worst of
// 3 456 random columns at cond ~ 2e7); the refinement step restores them (tests hold the result to 1e-10 against an
// extended-precision solve).  Inside a block the Gauss-Jordan sweep pivots by rows (the running diagonal blocks are not symmetric).
template <int N2>
struct ThomasCol {
    // T <- T^-1 by Gauss-Jordan on the diagonal pivots: pure DPP (lane c broadcasts the pivot row at step c).  The running diagonal
    // blocks D'_k are not symmetric, so this is a choice, not a theorem: a row-pivoted variant (pivot search by DPP rotations, row
    // exchange by bpermute) was built and measured -- 295 us instead of 205 us per sweep and NO gain in accuracy: with the
    // refinement step below both give 1.6e-12 against an extended-precision solve on rough random columns at cond(L) = 2e8
    // (tests/test_gpu_fullsize_oracle.py prints the budget), and all 3 456 columns of the full-size residual test stay below 1e-9.
    __device__ static void inverse_nopivot(double (&T)[N2], int r) { dpp::gauss_jordan<N2>(T, r); }
};

template <int N2>
__global__ __launch_bounds__(64) void k_thomas_dpp(int nEl, int nk, int refine, const double* __restrict__ L, const double* __restrict__ f,
                                                   double* __restrict__ d, double* __restrict__ Gws, double* __restrict__ Dws, double* __restrict__ yws,
                                                   int* __restrict__ stat, double* __restrict__ ratio) {
    constexpr int nn = N2*N2;
    const int lane = threadIdx.x, r = lane%16;
    const int e0 = blockIdx.x*4 + lane/16;
    const int e = e0 < nEl ? e0 : nEl - 1, rr = r < N2 ? r : N2 - 1;
    const bool act = e0 < nEl && r < N2;
    // blocks are stored LANE-major ([j][r]): element j of every row of a block is one contiguous run
    const double* Le = L + (size_t)e*nk*3*nn + rr;
    double* Ge = Gws + (size_t)e*nk*nn + rr;
    double* De = Dws + (size_t)e*nk*nn + rr;
    double* ye = yws + (size_t)e*nk*N2 + rr;
    const double* fe = f + (size_t)e*nk*N2 + rr;
    double* de = d + (size_t)e*nk*N2 + rr;
    auto mulsub = [&](double (&C)[N2], const double (&A)[N2], double (&B)[N2]) { dpp::MulSub<N2>::run(C, A, B); };       // C -= A . B
    auto matvec = [&](const double (&A)[N2], double x) {
        double y = 0.0;
        dpp::MatvecAcc<N2>::run(y, A, x);
        return y;
    };
    // ---- forward elimination, factors kept ----
    double S[N2], T[N2], U[N2], Gp[N2], Sn[N2], Tn[N2], Un[N2], fk, fn, yp = 0.0;
    auto fetch = [&](int k) {
        const double* row = Le + (size_t)k*3*nn;
#pragma unroll
        for (int j = 0; j < N2; j++) { Sn[j] = row[j*N2]; Tn[j] = row[nn + j*N2]; Un[j] = row[2*nn + j*N2]; }
        fn = fe[(size_t)k*N2];
    };
    fetch(0);
#pragma unroll 1
    for (int k = 0; k < nk; k++) {
#pragma unroll
        for (int j = 0; j < N2; j++) { S[j] = Sn[j]; T[j] = Tn[j]; U[j] = Un[j]; }
        fk = fn;
        if (k + 1 < nk) fetch(k + 1);
        if (k > 0) { mulsub(T, S, Gp); fk -= matvec(S, yp); }
        ThomasCol<N2>::inverse_nopivot(T, r);
#pragma unroll
        for (int j = 0; j < N2; j++) Gp[j] = 0.0;
        dpp::MulAcc<N2>::run(Gp, T, U);
        yp = matvec(T, fk);
        if (act) {
#pragma unroll
            for (int j = 0; j < N2; j++) { Ge[(size_t)k*nn + j*N2] = Gp[j]; De[(size_t)k*nn + j*N2] = T[j]; }
            ye[(size_t)k*N2] = yp;
        }
    }
    // ---- back substitution (the factors of level k-1 are fetched while level k is multiplied) ----
    double dn = yp;
    if (act) de[(size_t)(nk - 1)*N2] = dn;
    double Gk[N2], Gn[N2], yk, yn = 0.0;
    auto fetch_back = [&](int k) {
#pragma unroll
        for (int j = 0; j < N2; j++) Gn[j] = Ge[(size_t)k*nn + j*N2];
        yn = ye[(size_t)k*N2];
    };
    if (nk >= 2) fetch_back(nk - 2);
#pragma unroll 1
    for (int k = nk - 2; k >= 0; k--) {
#pragma unroll
        for (int j = 0; j < N2; j++) Gk[j] = Gn[j];
        yk = yn;
        if (k > 0) fetch_back(k - 1);
        dn = yk - matvec(Gk, dn);
        if (act) de[(size_t)k*N2] = dn;
    }
    // ---- iterative refinement, `refine` steps: r = f - L d;  y'_k = D'^-1_k (r_k - S_k y'_{k-1});  dd_k = y'_k - G_k dd_{k+1};  d += dd ----
    // (each lane re-reads only what it stored itself -- its own element of d and y, its own block rows: plain program order)
    double Di[N2], Dn[N2], dpn = 0.0;
    auto fetch_ref = [&](int k) {
        fetch(k);
#pragma unroll
        for (int j = 0; j < N2; j++) Dn[j] = De[(size_t)k*nn + j*N2];
        dpn = k + 1 < nk ? de[(size_t)(k + 1)*N2] : 0.0;
    };
    bool conv = false; double last = -1.0;
#pragma unroll 1
    for (int it = 0; it < refine; it++) {
        double dm = 0.0, dk = de[0], dp;
        yp = 0.0;
        fetch_ref(0);
#pragma unroll 1
        for (int k = 0; k < nk; k++) {
#pragma unroll
            for (int j = 0; j < N2; j++) { S[j] = Sn[j]; T[j] = Tn[j]; U[j] = Un[j]; Di[j] = Dn[j]; }
            double rk = fn;
            dp = dpn;
            if (k + 1 < nk) fetch_ref(k + 1);
            if (k > 0) rk -= matvec(S, dm);
            rk -= matvec(T, dk);
            if (k + 1 < nk) rk -= matvec(U, dp);
            if (k > 0) rk -= matvec(S, yp);
            yp = matvec(Di, rk);
            if (act) ye[(size_t)k*N2] = yp;
            dm = dk; dk = dp;
        }
        dn = yp;
        double dtop = de[(size_t)(nk - 1)*N2] + dn;
        if (act) de[(size_t)(nk - 1)*N2] = dtop;
        double s_dd = dn*dn, s_d = dtop*dtop;                      // this lane's share of |dd|^2 and |d|^2 over the column
        if (nk >= 2) fetch_back(nk - 2);
#pragma unroll 1
        for (int k = nk - 2; k >= 0; k--) {
#pragma unroll
            for (int j = 0; j < N2; j++) Gk[j] = Gn[j];
            yk = yn;
            if (k > 0) fetch_back(k - 1);
            dn = yk - matvec(Gk, dn);
            const double dnew = de[(size_t)k*N2] + dn;
            if (act) de[(size_t)k*N2] = dnew;
            s_dd += dn*dn; s_d += dnew*dnew;
        }
        // stop as soon as the correction of this column is below 1e-10 of the solution (uniform over the 16-lane row)
        double t_dd = 0.0, t_d = 0.0;
        dpp::static_for<0, N2>([&](auto m) { t_dd += dpp::get<m.value>(s_dd); t_d += dpp::get<m.value>(s_d); });
        conv = t_dd <= 1.0e-20*t_d;
        last = t_d > 0.0 ? sqrt(t_dd/t_d) : 0.0;
        if (conv) break;
    }
    // status of the column: 0 = the last correction was below 1e-10 of the solution; 1 = `refine` steps did not get there (the sweep
    // does not pivot across blocks: a column that ill-conditioned needs the caller's attention); 2 = no refinement asked for.
    // ratio = |last correction| / |solution|: how far the refinement got
    if (stat && r == 0 && e0 < nEl) { const int st = refine <= 0 ? 2 : (conv ? 0 : 1); stat[1 + e] = st; ratio[e] = last; if (st == 1) { const int pos = atomicAdd(stat + nEl + 1, 1); stat[nEl + 2 + pos] = e; atomicAdd(stat, 1); } }
}

// ---- the same solve TWO-SIDED (round 3): the top half of a column is eliminated downwards and the bottom half upwards at the same time ----
// k_thomas_dpp is a chain of nk dependent block steps per column with one wavefront per SIMD: VALU-active 17 %, the rest issue stalls
// and waits (profiles/r02_column_pmc.txt).  The twisted factorisation halves the chain: DPP rows 2c and 2c+1 of a wavefront hold the
// two halves of column c (two columns per wavefront, twice as many wavefronts, half as many steps each), written in SWEEP ORDER --
// step i works on level i (top) or nk-1-i (bottom), "previous" coupling block P = S (top) or U (bottom), "next" coupling Q = U or S --
// so both halves run the very same instructions:
//   forward   D'_i = T - P G_{i-1},  G_i = D'^-1 Q,  y_i = D'^-1 (f - P y_{i-1})              i = 0 .. m-1,  m = nk/2
//   middle    the two boundary unknowns a = d_{m-1}, b = d_m:  a = y_a - G_a b,  b = y_b - G_b a   =>   each half solves
//             (I - G_me G_other) x = y_me - G_me y_other   (the other half's G and y arrive by one cross-row exchange)
//   backward  d_i = y_i - G_i d_{i+1}                                                         i = m-2 .. 0
// Refinement as in k_thomas_dpp (r = f - L d with the neighbour across the middle taken from the other row), per-column status likewise.
// Even nk only (both halves the same length; odd nk keeps the one-sided kernel).
#ifndef MIMSEM_TD2_WPE
#define MIMSEM_TD2_WPE 1          // wavefronts per SIMD the two-sided sweep is compiled for.  Measured (scripts/ab_thomas.sh, 3 456 columns x
#endif                            // 30 levels): 1 (362 VGPRs at p = 3) 246 us; 2 (256 VGPRs, 101 spilled) 264 us; the one-sided sweep 344 us
// DEPTH: register slots of the forward elimination / steps per batch of the refinement (loads in flight ahead of their use); WPE: the
// wavefronts per SIMD the kernel is compiled for.  <3, 1> is round 3's form (362 VGPRs at p = 3: ONE wavefront per SIMD, so the 1 728
// wavefronts of 3 456 columns run as two rounds on the chip's 1 024 SIMDs); <2, 2> (round 5) gives up one slot of look-ahead to fit 256
// VGPRs without spilling: every wavefront is resident at once and a SIMD's second wavefront fills the first one's waits.
template <int N2, int DEPTH = 3, int WPE = MIMSEM_TD2_WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE, 8))) void k_thomas_dpp2(int nEl, int nk, int refine_and_flags, const double* __restrict__ L, const double* __restrict__ f,
                                                    double* __restrict__ d, double* __restrict__ Gws, double* __restrict__ Dws, double* __restrict__ yws,
                                                    int* __restrict__ stat, double* __restrict__ ratio) {
    constexpr int nn = N2*N2;
    const bool triage = (refine_and_flags & 0x100) != 0;               // bit 8: triage flagged columns here (the pivoted fallback is on)
    const int refine = refine_and_flags & 0xff;
    const int lane = threadIdx.x, r = lane%16, row = lane/16, h = row & 1;
    const int e0 = blockIdx.x*2 + row/2;
    const int e = e0 < nEl ? e0 : nEl - 1, rr = r < N2 ? r : N2 - 1;
    const bool act = e0 < nEl && r < N2;
    const int m = nk/2;
    const int kb = h ? nk - 1 : 0, ks = h ? -1 : 1;                   // level of sweep step i: kb + i ks
    const int oP = h ? 2*nn : 0, oQ = h ? 0 : 2*nn;                    // previous / next coupling block of a level's row {S, T, U}
    // blocks are stored LANE-major ([j][r]): element j of every row of a block is one contiguous run
    const double* Le = L + ((size_t)e*nk + kb)*3*nn + rr;
    double* Ge = Gws + ((size_t)e*nk + kb)*nn + rr;
    double* De = Dws + ((size_t)e*nk + kb)*nn + rr;
    double* ye = yws + ((size_t)e*nk + kb)*N2 + rr;
    const double* fe = f + ((size_t)e*nk + kb)*N2 + rr;
    double* de = d + ((size_t)e*nk + kb)*N2 + rr;
    const long long sL = (long long)ks*3*nn, sB = (long long)ks*nn, sV = (long long)ks*N2;      // strides of one sweep step
    auto mulsub = [&](double (&C)[N2], const double (&A)[N2], double (&B)[N2]) { dpp::MulSub<N2>::run(C, A, B); };       // C -= A . B
    auto matvec = [&](const double (&A)[N2], double x) {
        double y = 0.0;
        dpp::MatvecAcc<N2>::run(y, A, x);
        return y;
    };
    auto other = [&](double v) { return __shfl_xor(v, 16); };          // the same lane of the column's other half
    // Memory latency is what this kernel waits for (one wavefront per SIMD, a block row per step from L2 / Infinity Cache: SQ_WAIT_ANY 40 %
    // of the wave-cycles in the one-sided form), so every loop keeps SEVERAL steps' loads in flight:
    //   forward elimination   three register slots in rotation: the blocks of step i+2 are requested before step i is computed;
    //   back substitution     the factors of four steps requested together, then the four (dependent) mat-vecs;
    //   refinement            the blocks of three steps requested together, then the three residual / forward-solve steps.
    // ---- forward elimination of both halves, factors kept ----
    double Gp[N2], yp = 0.0;
    {
        double Pb[DEPTH][N2], Tb[DEPTH][N2], Qb[DEPTH][N2], fb[DEPTH];
        auto load = [&](int slot, int i) {                              // (slot is a compile-time constant wherever this is called)
            const double* rw = Le + (long long)i*sL;
#pragma unroll
            for (int j = 0; j < N2; j++) { Pb[slot][j] = rw[oP + j*N2]; Tb[slot][j] = rw[nn + j*N2]; Qb[slot][j] = rw[oQ + j*N2]; }
            fb[slot] = fe[(long long)i*sV];
        };
#pragma unroll
        for (int sl = 0; sl < DEPTH - 1; sl++) if (sl < m) load(sl, sl);
#pragma unroll 1
        for (int i0 = 0; i0 < m; i0 += DEPTH) {
#pragma unroll
            for (int sl = 0; sl < DEPTH; sl++) {
                const int i = i0 + sl;
                if (i < m) {                                            // wave-uniform
                    if (i + DEPTH - 1 < m) load((sl + DEPTH - 1)%DEPTH, i + DEPTH - 1);
                    double (&P)[N2] = Pb[sl]; double (&T)[N2] = Tb[sl]; double (&Q)[N2] = Qb[sl];
                    double fk = fb[sl];
                    if (i > 0) { mulsub(T, P, Gp); fk -= matvec(P, yp); }
                    ThomasCol<N2>::inverse_nopivot(T, r);
#pragma unroll
                    for (int j = 0; j < N2; j++) Gp[j] = 0.0;
                    dpp::MulAcc<N2>::run(Gp, T, Q);
                    yp = matvec(T, fk);
                    if (act) {
#pragma unroll
                        for (int j = 0; j < N2; j++) { Ge[(long long)i*sB + j*N2] = Gp[j]; De[(long long)i*sB + j*N2] = T[j]; }
                        ye[(long long)i*sV] = yp;
                    }
                }
            }
        }
    }
    // ---- the middle: (I - G_me G_other) x = y_me - G_me y_other; both G's stay in registers for the refinement ----
    double Gb[N2], Mi[N2];
    {
        double Go[N2], t[N2];
#pragma unroll
        for (int j = 0; j < N2; j++) { Gb[j] = Gp[j]; Go[j] = other(Gp[j]); t[j] = 0.0; }
        dpp::MulAcc<N2>::run(t, Gb, Go);
#pragma unroll
        for (int j = 0; j < N2; j++) Mi[j] = (j == rr ? 1.0 : 0.0) - t[j];
        ThomasCol<N2>::inverse_nopivot(Mi, r);
    }
    auto middle = [&](double y_me) { return matvec(Mi, y_me - matvec(Gb, other(y_me))); };
    double dbnd = middle(yp);                                           // this half's boundary unknown (step m-1)
    if (act) de[(long long)(m - 1)*sV] = dbnd;
    // ---- back substitution of both halves: d_i = y_i - G_i d_{i+1}, i = m-2 .. 0, four steps' factors requested at a time.
    // update = false: d_i is stored; update = true (refinement): the result is a correction, d_i += it, and the norms are collected ----
    double s_dd = 0.0, s_d = 0.0;
    auto backsub = [&](double dn, bool update) {
#pragma unroll 1
        for (int i0 = m - 2; i0 >= 0; i0 -= 4) {
            double Gq[4][N2], yq[4], oq[4];
#pragma unroll
            for (int sl = 0; sl < 4; sl++) {
                const int i = i0 - sl >= 0 ? i0 - sl : 0;               // (below the first step: a valid address, the value is not used)
#pragma unroll
                for (int j = 0; j < N2; j++) Gq[sl][j] = Ge[(long long)i*sB + j*N2];
                yq[sl] = ye[(long long)i*sV];
                oq[sl] = update ? de[(long long)i*sV] : 0.0;
            }
#pragma unroll
            for (int sl = 0; sl < 4; sl++) {
                const int i = i0 - sl;
                if (i >= 0) {                                           // wave-uniform
                    dn = yq[sl] - matvec(Gq[sl], dn);
                    const double dnew = oq[sl] + dn;
                    if (act) de[(long long)i*sV] = dnew;
                    s_dd += dn*dn; s_d += dnew*dnew;
                }
            }
        }
    };
    backsub(dbnd, false);
    // ---- iterative refinement: r = f - L d;  y'_i = D'^-1_i (r_i - P_i y'_{i-1});  middle;  dd_i = y'_i - G_i dd_{i+1};  d += dd ----
    // (a lane re-reads from memory only what it stored itself; what crosses the middle travels through `other`)
    bool conv = false; double last = -1.0;
#pragma unroll 1
    for (int it = 0; it < refine; it++) {
        const double dacross = other(dbnd);                            // d of the level on the far side of the middle
        double dlast = 0.0;                                            // d of the step before the batch
        yp = 0.0;
#pragma unroll 1
        for (int i0 = 0; i0 < m; i0 += DEPTH) {
            double Pq[DEPTH][N2], Tq[DEPTH][N2], Qq[DEPTH][N2], Dq[DEPTH][N2], fq[DEPTH], dq[DEPTH + 1];
#pragma unroll
            for (int sl = 0; sl < DEPTH; sl++) {
                const int i = i0 + sl < m ? i0 + sl : m - 1;
                const double* rw = Le + (long long)i*sL;
#pragma unroll
                for (int j = 0; j < N2; j++) { Pq[sl][j] = rw[oP + j*N2]; Tq[sl][j] = rw[nn + j*N2]; Qq[sl][j] = rw[oQ + j*N2];
                                               Dq[sl][j] = De[(long long)i*sB + j*N2]; }
                fq[sl] = fe[(long long)i*sV];
                dq[sl] = de[(long long)i*sV];
            }
            dq[DEPTH] = de[(long long)(i0 + DEPTH < m ? i0 + DEPTH : m - 1)*sV];
#pragma unroll
            for (int sl = 0; sl < DEPTH; sl++) {
                const int i = i0 + sl;
                if (i < m) {                                            // wave-uniform
                    const double dm = sl > 0 ? dq[sl - 1] : dlast, dk = dq[sl], dp = i + 1 < m ? dq[sl + 1] : dacross;
                    double rk = fq[sl];
                    if (i > 0) rk -= matvec(Pq[sl], dm);
                    rk -= matvec(Tq[sl], dk);
                    rk -= matvec(Qq[sl], dp);
                    if (i > 0) rk -= matvec(Pq[sl], yp);
                    yp = matvec(Dq[sl], rk);
                    if (act) ye[(long long)i*sV] = yp;
                }
            }
            dlast = dq[DEPTH - 1];
        }
        const double dn = middle(yp);
        dbnd += dn;
        if (act) de[(long long)(m - 1)*sV] = dbnd;
        s_dd = dn*dn; s_d = dbnd*dbnd;                                 // this lane's share of |dd|^2 and |d|^2 over its half
        backsub(dn, true);
        // stop as soon as the correction of this column is below 1e-10 of the solution (uniform over the column's two rows)
        double t_dd = 0.0, t_d = 0.0;
        dpp::static_for<0, N2>([&](auto mm) { t_dd += dpp::get<mm.value>(s_dd); t_d += dpp::get<mm.value>(s_d); });
        t_dd += other(t_dd); t_d += other(t_d);
        conv = t_dd <= 1.0e-20*t_d;
        const double prev = last;
        last = t_d > 0.0 ? sqrt(t_dd/t_d) : 0.0;
        if (conv) break;
        // a correction that no longer shrinks has reached the floor the column's conditioning sets (cond eps): further steps return the same
        // ratio -- and the wavefronts that run them are the tail of the launch (round 5)
        if (it > 0 && last > 0.5*prev) break;
    }
    int st = refine <= 0 ? 2 : (conv ? 0 : 1);
    // ---- triage of a column the refinement left above 1e-10 (round 5: moved here from the fallback kernel, column_pivot.inc, whose launch then
    // finds its counter at zero and leaves).  Most such columns are limited by their CONDITIONING, not by the unpivoted elimination: the normwise
    // backward error |f - L d| / (|L|_F |d| + |f|) of the solution they have is at round-off level -- a pivoted LU would return the same.  They
    // become status 4 and are not counted; a column whose backward error says the elimination itself went wrong keeps status 1 for the
    // pivoted LU behind this launch.  One more pass over the bands, only in wavefronts that hold such a column (the slowest of the launch
    // already: they ran every refinement step).
    if (triage && __ballot(st == 1) != 0ull) {
        double r2 = 0.0, a2 = 0.0, x2 = 0.0, f2 = 0.0;
        const double dacross = other(dbnd);
        const double w = r < N2 ? 1.0 : 0.0;                            // (lanes beyond the block's rows mirror row N2 - 1)
        double dlast = 0.0;                                            // d of the step before the batch
#pragma unroll 1
        for (int i0 = 0; i0 < m; i0 += DEPTH) {                         // DEPTH steps' blocks requested together, as in the refinement: the
            double Pq[DEPTH][N2], Tq[DEPTH][N2], Qq[DEPTH][N2], fq[DEPTH], dq[DEPTH + 1];      // wavefronts that come here are the launch's tail
#pragma unroll
            for (int sl = 0; sl < DEPTH; sl++) {
                const int i = i0 + sl < m ? i0 + sl : m - 1;
                const double* rw = Le + (long long)i*sL;
#pragma unroll
                for (int j = 0; j < N2; j++) { Pq[sl][j] = rw[oP + j*N2]; Tq[sl][j] = rw[nn + j*N2]; Qq[sl][j] = rw[oQ + j*N2]; }
                fq[sl] = fe[(long long)i*sV];
                dq[sl] = de[(long long)i*sV];
            }
            dq[DEPTH] = de[(long long)(i0 + DEPTH < m ? i0 + DEPTH : m - 1)*sV];
#pragma unroll
            for (int sl = 0; sl < DEPTH; sl++) {
                const int i = i0 + sl;
                if (i < m) {                                            // wave-uniform
                    const double dm = sl > 0 ? dq[sl - 1] : dlast, dk = dq[sl], dp = i + 1 < m ? dq[sl + 1] : dacross;
                    double rk = fq[sl] - matvec(Tq[sl], dk) - matvec(Qq[sl], dp);
                    if (i > 0) rk -= matvec(Pq[sl], dm);
                    double sq = 0.0;
#pragma unroll
                    for (int j = 0; j < N2; j++) sq += Tq[sl][j]*Tq[sl][j] + Qq[sl][j]*Qq[sl][j] + (i > 0 ? Pq[sl][j]*Pq[sl][j] : 0.0);
                    r2 += w*rk*rk; a2 += w*sq; x2 += w*dk*dk; f2 += w*fq[sl]*fq[sl];
                }
            }
            dlast = dq[DEPTH - 1];
        }
        double t_r = 0.0, t_a = 0.0, t_x = 0.0, t_f = 0.0;
        dpp::static_for<0, N2>([&](auto mm) { t_r += dpp::get<mm.value>(r2); t_a += dpp::get<mm.value>(a2); t_x += dpp::get<mm.value>(x2); t_f += dpp::get<mm.value>(f2); });
        t_r += other(t_r); t_a += other(t_a); t_x += other(t_x); t_f += other(t_f);
        const double eta0 = sqrt(t_r)/(sqrt(t_a)*sqrt(t_x) + sqrt(t_f));
        if (st == 1 && eta0 <= BANDLU_ACCEPT) st = 4;                   // (NaN fails)
    }
    if (stat && r == 0 && h == 0 && e0 < nEl) { stat[1 + e] = st; ratio[e] = last; if (st == 1) { const int pos = atomicAdd(stat + nEl + 1, 1); stat[nEl + 2 + pos] = e; atomicAdd(stat, 1); } }
}

// ---- back substitution of solve_schur_column_eta (VertSolve.cpp:792-815) from recomputed factors ---------------------------------------
//   F_u <- -(F_u + G_pi d_pi),  d_u = lump . F_u;   F_eta <- -(F_eta + A_eta d_u),  d_eta = VB^-1 F_eta;
//   F_rho <- -(F_rho + h VB (V10 X d_u)),  d_rho = VB^-1 F_rho.
// One task = column e, levels [k0, k1): walks interfaces k0-1 .. k1-1 (the first and last are shared with the neighbouring tasks and
// recomputed), every product is a chain of mat-vecs: G(i,i) p = -h T (A^-1 (B_i p)), X du = A^-1 (VA(rho) du).
struct BacksubArgs {
    int nEl, nk, chunk, nchunk;
    const double *det, *tI, *th, *w, *W, *Eg;
    double E[20];
    double hdt;
    const double *theta, *rho, *rl, *geta, *d_pi, *fu2;   // fu2: F_u after the update of the sweep (:772-773)
    double *F_u, *F_eta, *F_rho, *d_u, *d_eta, *d_rho;
};
template <int N>
__global__ __launch_bounds__(64) void k_schur_backsub(BacksubArgs a) {
    using R = dpp::Rows<N>;
    constexpr int N2 = R::N2, NP = R::NP, MP12 = R::MP12, MP1 = R::MP1;
    const int lane = threadIdx.x, r = lane%16;
    const WalkTask tk = walk_task(a.nEl, a.nchunk, lane);
    const bool live = tk.live;
    const int e = tk.e, ch = tk.ch;
    const int nk = a.nk, nm = nk - 1;
    const int k0 = ch*a.chunk, k1 = min(nk, k0 + a.chunk);
    const int rr = r < N2 ? r : N2 - 1;
    const bool act = live && r < N2;
    const double hdt = a.hdt;
    typename R::Lane Ln;
    R::init_lane(Ln, a.Eg, a.W, r);
    double q0[NP], det[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const int q = min(r + 16*p, MP12 - 1);
        det[p] = a.det[(size_t)e*MP12 + q];
        q0[p] = (a.w[q%MP1]*a.w[q/MP1])*(VSCALE/det[p]);
    }
    struct Lv { double B[N2]; double th[NP], thI[NP], rhI[NP]; double dpi; };
    struct Rw { double th[NP], tI[NP], theta, rho, dpi; };
    auto load = [&](Rw& W, int k) {
        const size_t vo = ((size_t)e*nk + k)*N2 + rr;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int q = min(r + 16*p, MP12 - 1);
            const size_t go = ((size_t)k*a.nEl + e)*MP12 + q;
            W.th[p] = a.th[go]; W.tI[p] = a.tI[go];
        }
        W.theta = a.theta[vo]; W.rho = a.rho[vo]; W.dpi = a.d_pi[vo];
    };
    auto level = [&](Lv& V, const Rw& W) {
        double c[NP];
#pragma unroll
        for (int p = 0; p < NP; p++) { V.th[p] = W.th[p]; c[p] = q0[p]*W.tI[p]; }
        R::assemble(V.B, Ln, a.E, c);
        R::interp(V.thI, Ln, W.theta);
        R::interp(V.rhI, Ln, W.rho);
        V.dpi = W.dpi;
    };
    // per interface: d_u and the two vectors rows i, i+1 need from it:  cd = h C d_u,  xd = X d_u
    Lv V0, V1;
    const int i0 = k0 > 0 ? k0 - 1 : 0, i1 = min(k1 - 1, nm - 1);
    Rw W0, Wn;
    load(W0, i0); load(Wn, min(i0 + 1, nk - 1));
    level(V0, W0);
    double cd_below = 0.0, xd_below = 0.0;            // contributions of interface k-1 to row k, carried upwards
    bool have_below = false;
    // interface vectors, fetched one interface ahead as well
    double fu_n = a.fu2[((size_t)e*nm + i0)*N2 + rr], rl_n = a.rl[((size_t)e*nm + i0)*N2 + rr], ge_n = a.geta[((size_t)e*nm + i0)*N2 + rr];
#pragma unroll 1
    for (int i = i0; i <= i1; i++) {
        W0 = Wn;
        load(Wn, min(i + 2, nk - 1));
        // the row's right-hand sides are needed at the END of the step: requested here, they arrive under the step's arithmetic
        const double fe_in = a.F_eta[((size_t)e*nk + i)*N2 + rr], fr_in = a.F_rho[((size_t)e*nk + i)*N2 + rr];
        const double fu_i = fu_n, rl_i = rl_n, ge_i = ge_n;
        { const size_t in = ((size_t)e*nm + min(i + 1, nm - 1))*N2 + rr; fu_n = a.fu2[in]; rl_n = a.rl[in]; ge_n = a.geta[in]; }
        level(V1, W0);
        double c[NP], Ai[N2], T[N2];
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = q0[p]*(0.5*(V0.th[p] + V1.th[p]));
        R::assemble(Ai, Ln, a.E, c);
        R::inverse(Ai, r);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = q0[p]*(0.5*V0.thI[p]/det[p]) + q0[p]*(0.5*V1.thI[p]/det[p]);
        R::assemble(T, Ln, a.E, c);
        // G_pi d_pi at interface i = h T A^-1 (B_{i+1} p_{i+1} - B_i p_i)
        const double gp = hdt*R::matvec(T, R::matvec(Ai, R::matvec(V1.B, V1.dpi) - R::matvec(V0.B, V0.dpi)));
        const size_t io = ((size_t)e*nm + i)*N2 + rr;
        double fu = fu_i + gp;                        // :792-795
        fu *= -1.0;
        const double du = rl_i*fu;
        const bool own = i >= k0;                      // the task that owns level i stores interface i
        if (act && own) { a.F_u[io] = fu; a.d_u[io] = du; }
        // what rows i and i+1 need: h C d_u (A_eta d_u, :807) and X d_u (:812)
        double wI[NP];
        R::interp(wI, Ln, ge_i);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = q0[p]*(0.5*wI[p]/det[p]);
        double C[N2];
        R::assemble(C, Ln, a.E, c);
        const double cd = hdt*R::matvec(C, du);
#pragma unroll
        for (int p = 0; p < NP; p++) c[p] = q0[p]*(0.5*V0.rhI[p]/det[p]) + q0[p]*(0.5*V1.rhI[p]/det[p]);
        R::assemble(T, Ln, a.E, c);
        const double xd = R::matvec(Ai, R::matvec(T, du));
        if (own) {
            // row i is complete: interfaces i-1 (carried) and i
            double Bi[N2];
#pragma unroll
            for (int j = 0; j < N2; j++) Bi[j] = V0.B[j];
            R::inverse(Bi, r);
            const size_t vo = ((size_t)e*nk + i)*N2 + rr;
            double fe = fe_in + ((have_below ? cd_below : 0.0) + cd);
            fe *= -1.0;
            const double de = R::matvec(Bi, fe);
            double fr = fr_in + hdt*R::matvec(V0.B, xd - (have_below ? xd_below : 0.0));     // (V10 X d_u)_k = X_k du_k - X_{k-1} du_{k-1}
            fr *= -1.0;
            const double dr = R::matvec(Bi, fr);
            if (act) { a.F_eta[vo] = fe; a.d_eta[vo] = de; a.F_rho[vo] = fr; a.d_rho[vo] = dr; }
        }
        cd_below = cd; xd_below = xd; have_below = true;
        V0 = V1;
    }
    if (k1 == nk) {                                   // top level: only the interface below it
        double Bi[N2];
#pragma unroll
        for (int j = 0; j < N2; j++) Bi[j] = V0.B[j];
        R::inverse(Bi, r);
        const size_t vo = ((size_t)e*nk + nk - 1)*N2 + rr;
        double fe = a.F_eta[vo] + (have_below ? cd_below : 0.0);
        fe *= -1.0;
        const double de = R::matvec(Bi, fe);
        double fr = a.F_rho[vo] + hdt*R::matvec(V0.B, -(have_below ? xd_below : 0.0));
        fr *= -1.0;
        const double dr = R::matvec(Bi, fr);
        if (act) { a.F_eta[vo] = fe; a.d_eta[vo] = de; a.F_rho[vo] = fr; a.d_rho[vo] = dr; }
    }
}

// levels per task: enough tasks to put ~one wavefront on every SIMD of the chip (256 CUs x 4), no more -- every extra task recomputes an interface
int sweep_chunk(const mimsem_ctx* c, int waves_per_simd = 1, int slots4 = 768, int tpw = 4) {
    if (const char* ev = exp_env("MIMSEM_SWEEP_CHUNK")) { const int v = atoi(ev); if (v > 0) return std::min(std::max(v, 2), std::max(c->nk, 1)); }      // (>= 2 levels per task: the workspaces are sized for <= nk/2 + 1 tasks per column)
    // (the sweep kernels hold ~20 blocks in registers: ONE wavefront per SIMD, so a task beyond 1024 waves does not run beside the
    //  others but after them -- split a column only while the extra tasks find idle SIMDs)
    const long long waves1 = ((long long)c->nEl + tpw - 1)/tpw;     // one task per column
    long long slots = 1024LL*waves_per_simd;         // 256 CUs x 4 SIMDs x the waves of this kernel a SIMD holds
    if (waves_per_simd == 1 && c->es.n == 4) slots = slots4;       // k_schur_sweep<4> parks six blocks in LDS (48 KB): three workgroups per CU (k_s3_sweep<4>: 32 KB, four)
    long long nch = waves1 >= slots ? 1 : slots/waves1;
    nch = std::max(1LL, std::min(nch, (long long)c->nk/2));
    return (int)((c->nk + nch - 1)/nch);
}

template <class A> void fill_geo(const mimsem_ctx* c, A& a, int waves_per_simd = 1, int slots4 = 768, int tpw = 4) {
    a.nEl = c->nEl; a.nk = c->nk; a.chunk = sweep_chunk(c, waves_per_simd, slots4, tpw); a.nchunk = (c->nk + a.chunk - 1)/a.chunk;
    a.det = c->d_det; a.tI = c->d_tI; a.th = c->d_th; a.w = c->d_w; a.W = c->d_W; a.Eg = c->d_E;
    for (int i = 0; i < 20; i++) a.E[i] = i < (int)c->tab.E.size() ? c->tab.E[i] : 0.0;
}

bool sweep_supported(const mimsem_ctx* c) { return c->es.n >= 1 && c->es.n <= 4 && c->nk >= 2; }

using mimsem::SweepWS;

int launch_sweep(mimsem_ctx* c, const SweepArgs& a) {
    const unsigned grid = walk_task_grid(a.nEl, a.nchunk);
    if (int rc = for_order<1, 2, 3, 4>(c->es.n, [&](auto N) { hipLaunchKernelGGL((k_schur_sweep<N()>), dim3(grid), dim3(64), 0, c->stream, a); })) return rc;
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}
// per-column status of a column solve (mimsem_column_solve_status): [0] = columns whose refinement did not converge (the fallback counts it
// down), [1 + e] = status of column e, [nEl + 1] = length of the FLAGGED LIST, [nEl + 2 + i] = the i-th column a solve kernel flagged (in the
// order the flags were raised; the list is what the fallback's wavefronts deal out among themselves: immutable while they run).
// Allocated at the first solve -- never inside a stream capture (hipMalloc is illegal there: warm the solve up outside the capture)
int ensure_colstat(mimsem_ctx* c) {
    if (c->d_colstat) return MIMSEM_OK;
    if (c->is_capturing()) return MIMSEM_ERR_STATE;
    if (int rc = c->alloc((void**)&c->d_colstat, (2*(size_t)c->nEl + 2)*sizeof(int))) return rc;
    return c->alloc((void**)&c->d_colratio, (size_t)c->nEl*sizeof(double));
}
int launch_thomas_dpp(mimsem_ctx* c, int refine, const double* L, const double* f, double* d, double* G, double* D, double* y, bool counter_zeroed = false) {
    if (int rc = ensure_colstat(c)) return rc;
    if (!counter_zeroed) { MIMSEM_HIP_TRY(hipMemsetAsync(c->d_colstat, 0, sizeof(int), c->stream)); MIMSEM_HIP_TRY(hipMemsetAsync(c->d_colstat + c->nEl + 1, 0, sizeof(int), c->stream)); }      // (the fused solve has its sweep kernel zero them)
    const bool two_sided = !(exp_env("MIMSEM_THOMAS2") && atoi(exp_env("MIMSEM_THOMAS2")) == 0);      // (read per call: tests compare both forms in one process)
    if (two_sided && c->nk >= 4 && c->nk%2 == 0 && c->es.n2e <= 16) {
        const unsigned grid = (unsigned)((c->nEl + 1)/2);
        // the two-sided kernel triages its flagged columns itself when the pivoted fallback is on (mode 1; MIMSEM_THOMAS_TRIAGE=0: leave it to the
        // fallback kernel as before)
        if (refine > 0xff) refine = 0xff;
        if (c->pivot_fallback == 1 && !(exp_env("MIMSEM_THOMAS_TRIAGE") && atoi(exp_env("MIMSEM_THOMAS_TRIAGE")) == 0)) refine |= 0x100;
        // A/B forms (round 5, profiles/r05_thomas_wps_ab.txt): order 3 at TWO wavefronts per SIMD (one slot of look-ahead less: 252 VGPRs, no
        // spill, all 1 728 wavefronts of 3 456 columns resident at once) -- 229 us against 205 us: the kernel moves 887 MB per launch and is
        // bound by that traffic (4.2-4.3 TB/s; a plain copy reaches 4.9), not by residency; order 4 with two slots instead of three (no spill)
        const int wps = exp_env("MIMSEM_THOMAS_WPS") ? atoi(exp_env("MIMSEM_THOMAS_WPS")) : 1;
        const int depth = exp_env("MIMSEM_THOMAS_DEPTH") ? atoi(exp_env("MIMSEM_THOMAS_DEPTH")) : 3;
#ifdef MIMSEM_WITH_EXPERIMENTS
        if (c->es.n2e == 9 && wps == 2) hipLaunchKernelGGL((k_thomas_dpp2<9, 2, 2>), dim3(grid), dim3(64), 0, c->stream, c->nEl, c->nk, refine, L, f, d, G, D, y, c->d_colstat, c->d_colratio);
        else if (c->es.n2e == 16 && depth == 2) hipLaunchKernelGGL((k_thomas_dpp2<16, 2, 1>), dim3(grid), dim3(64), 0, c->stream, c->nEl, c->nk, refine, L, f, d, G, D, y, c->d_colstat, c->d_colratio);
        else
#endif
        if (int rc = for_order<1, 4, 9, 16>(c->es.n2e, [&](auto N) {
                hipLaunchKernelGGL((k_thomas_dpp2<N()>), dim3(grid), dim3(64), 0, c->stream, c->nEl, c->nk, refine, L, f, d, G, D, y, c->d_colstat, c->d_colratio); })) return rc;
        MIMSEM_HIP_TRY(hipGetLastError());
        return MIMSEM_OK;
    }
    const unsigned grid = (unsigned)((c->nEl + 3)/4);
    if (int rc = for_order<1, 4, 9, 16>(c->es.n2e, [&](auto N) {
            hipLaunchKernelGGL((k_thomas_dpp<N()>), dim3(grid), dim3(64), 0, c->stream, c->nEl, c->nk, refine, L, f, d, G, D, y, c->d_colstat, c->d_colratio); })) return rc;
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}
int launch_backsub(mimsem_ctx* c, const BacksubArgs& a) {
    const unsigned grid = walk_task_grid(a.nEl, a.nchunk);
    if (int rc = for_order<1, 2, 3, 4>(c->es.n, [&](auto N) { hipLaunchKernelGGL((k_schur_backsub<N()>), dim3(grid), dim3(64), 0, c->stream, a); })) return rc;
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

// the Helmholtz operator alone (mimsem_column_helmholtz_blocks)
int sweep_helmholtz(mimsem_ctx* c, double dt, const double* theta, const double* rho, const double* eta, const double* pi, double* out) {
    SweepWS w;
    int rc = plan_col(c, w);
    if (rc) return rc;
    SweepArgs a{};
    fill_geo(c, a);
    a.hdt = 0.5*dt; a.gam = RD/CV; a.theta = theta; a.rho = rho; a.eta = eta; a.pi = pi;
    a.F_u = nullptr; a.F_pi = nullptr; a.F_eta = nullptr; a.F_rho = nullptr;
    a.L = out; a.rowmajor = 1; a.rl = w.rl; a.geta = w.geta; a.fu2 = w.fu2;
    return launch_sweep(c, a);
}

// solve_schur_column_eta in three launches
int sweep_solve_eta(mimsem_ctx* c, double dt, const double* theta, const double* rho, const double* eta, const double* pi,
                    double* F_u, double* F_rho, double* F_eta, double* F_pi, double* d_u, double* d_rho, double* d_eta, double* d_pi) {
    SweepWS w;
    int rc = plan_col(c, w);
    if (rc) return rc;
    SweepArgs a{};
    fill_geo(c, a);
    a.hdt = 0.5*dt; a.gam = RD/CV; a.theta = theta; a.rho = rho; a.eta = eta; a.pi = pi;
    a.F_u = F_u; a.F_pi = F_pi; a.F_eta = F_eta; a.F_rho = F_rho;
    a.L = w.L; a.rowmajor = 0; a.rl = w.rl; a.geta = w.geta; a.fu2 = w.fu2;
    if ((rc = ensure_colstat(c))) return rc;
    a.statz = c->d_colstat;
    if ((rc = launch_sweep(c, a))) return rc;
    // up to four refinement steps, each column stops once its correction is below 1e-10 of its solution (most stop after the first): the
    // sweep eliminates block by block without pivoting across blocks; on 3 456 rough random columns the worst relative residual is
    // 1e-5 after the sweep and at LAPACK's level (eps |L| |d| / |f|) after one or two steps -- scripts/diag_thomas_residual.py
    if ((rc = launch_thomas_dpp(c, refine_steps(), w.L, F_pi, d_pi, w.G, w.D, w.y, true))) return rc;
    if ((rc = launch_band_lu_flagged(c, 1, w.L, false, F_pi, d_pi))) return rc;       // (opt-in: flagged columns by a pivoted band LU, column_pivot.inc)
    BacksubArgs b{};
    fill_geo(c, b, exp_env("MIMSEM_BACKSUB_WPS") ? std::max(1, atoi(exp_env("MIMSEM_BACKSUB_WPS"))) : 2);      // 192 VGPRs: two waves per SIMD, the second hides the first one's memory waits (A/B knob)
    b.hdt = 0.5*dt; b.theta = theta; b.rho = rho; b.rl = w.rl; b.geta = w.geta; b.d_pi = d_pi; b.fu2 = w.fu2;
    b.F_u = F_u; b.F_eta = F_eta; b.F_rho = F_rho; b.d_u = d_u; b.d_eta = d_eta; b.d_rho = d_rho;
    return launch_backsub(c, b);
}

}  // namespace
