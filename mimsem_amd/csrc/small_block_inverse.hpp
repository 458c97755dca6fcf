// mimsem_amd/csrc/small_block_inverse.hpp -- the Gauss-Jordan sweeps of the small dense blocks, each spelled once (device only, all inlined).
//
//   sweep                                   pivoting / tie-breaking                          callers
//   A serial_pivot_inverse                  full, LinAlg.cpp:186-269: the LAST entry of the  k_block_inverse (thread-minor LDS),
//     one thread per block                  row-major scan attaining the maximum             slow path of k_block_inverse_reg (private array)
//   B wave_pivot_inverse                    the same pivots and the same operations per      k_block_inverse_wave (run-time n),
//     lane = row, block in LDS, odd stride  entry as A: the same bits                        elem_block_pc_body (constexpr n, error dropped)
//   C k_block_inverse_rows (column_kernels.hip, its only copy): A's pivots, lane = row, rows in registers
//   D reg_inverse                           none (natural order); reports a pivot below      k_block_inverse_reg, k_eos_block_thread
//     one thread per block, registers       1e-8 x the largest diagonal entry or 1e-12
//   E WaveBlocks<N2>::inverse (column_kernels.hip, its only copy): partial (column maximum, first row attaining it) on [D | Di], one
//     wavefront, LDS                                                                         k_block_thomas_wave, k_schur_levels / _interfaces
//   F rows_gauss_jordan                     implicit row pivoting: the unused lane with the  k_block_thomas_rows, RowBlocks<N>::inverse
//     one row per lane, 16 or 32 lanes      largest |T[c]|, ties -> the lowest lane
//
// Two callers of one sweep run the same floating-point operations in the same order by construction.  The other inverses of the column layer
// are decompositions of their own with one copy each: dpp::gauss_jordan (column_dpp.inc, pivot_rcp), private_inverse and the workgroup sweep
// of k_block_thomas.
#pragma once
#include <hip/hip_runtime.h>

namespace mimsem {

// hand-off between the lanes of ONE wavefront (no s_barrier)
__device__ __forceinline__ void wsync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// the same hand-off when only LDS data crosses lanes: the fences name the local address space, so outstanding GLOBAL loads /
// stores (the prefetch of the next level, the stores of G and D^-1) are not waited for
__device__ __forceinline__ void wsync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
// rotate within each row of 16 lanes (DPP row_ror: a VALU modifier, no LDS crossbar trip like ds_bpermute)
template <int N> __device__ __forceinline__ int row_ror(int v) {
    return __builtin_amdgcn_update_dpp(v, v, 0x120 + N, 0xF, 0xF, false);
}
template <int N> __device__ __forceinline__ double row_ror(double v) {
    return __hiloint2double(row_ror<N>(__double2hiint(v)), row_ror<N>(__double2loint(v)));
}

// element k of an array that is interleaved with those of the other threads: p[k*stride + off]
template <class T>
struct Strided {
    T* p; int stride, off;
    __device__ __forceinline__ T& operator[](int k) const { return p[k*stride + off]; }
};

// ---- A: in-place inverse of the n x n block A[i*n + j], one thread, exactly LinAlg.cpp:186-269 (pivot search, swaps, elimination, column
// un-permutation).  A, ipiv, indxr, indxc: anything with operator[] (plain pointers, Strided).  Returns the reference's error code.
template <class Mat, class Idx>
__device__ __forceinline__ int serial_pivot_inverse(int n, Mat A, Idx ipiv, Idx indxr, Idx indxc) {
    for (int j = 0; j < n; j++) ipiv[j] = 0;
    int err = 0, irow = 0, icol = 0;
    for (int i = 0; i < n; i++) {
        double big = 0.0;
        for (int j = 0; j < n; j++) {
            if (ipiv[j] == 1) continue;
            for (int k = 0; k < n; k++) {
                if (ipiv[k] == 0) {
                    const double v = fabs(A[j*n + k]);
                    if (v >= big) { big = v; irow = j; icol = k; }
                } else if (ipiv[k] > 1) err = 1;
            }
        }
        ++ipiv[icol];
        if (irow != icol)
            for (int l = 0; l < n; l++) { const double tmp = A[irow*n + l]; A[irow*n + l] = A[icol*n + l]; A[icol*n + l] = tmp; }
        indxr[i] = irow; indxc[i] = icol;
        if (fabs(A[icol*n + icol]) < 1.0e-12) err = 2;
        const double pivinv = 1.0/A[icol*n + icol];
        A[icol*n + icol] = 1.0;
        for (int l = 0; l < n; l++) A[icol*n + l] *= pivinv;
        for (int ll = 0; ll < n; ll++) {
            if (ll == icol) continue;
            const double dum = A[ll*n + icol];
            A[ll*n + icol] = 0.0;
            for (int l = 0; l < n; l++) A[ll*n + l] -= A[icol*n + l]*dum;
        }
    }
    for (int l = n - 1; l >= 0; l--) {
        const int ir = indxr[l], ic = indxc[l];
        if (ir == ic) continue;
        for (int k = 0; k < n; k++) { const double tmp = A[k*n + ir]; A[k*n + ir] = A[k*n + ic]; A[k*n + ic] = tmp; }
    }
    return err;
}

// ---- B: the same inverse by the 64 lanes of a one-wavefront workgroup: lane = row of the elimination (and column of the row swap / scaling),
// the block A[i*ns + j] in LDS with an ODD row stride ns (conflict-free row and column walks), ipiv[n] zeroed and published by the caller.
// Returns A's error code (a caller that drops it pays nothing for it).
__device__ __forceinline__ int wave_pivot_inverse(double* A, int n, int ns, int* ipiv, int* indxr, int* indxc, int lane) {
    int err = 0;
    for (int i = 0; i < n; i++) {
        // pivot search: my row, then the wavefront.  Sequential semantics of the reference: the last (j, k) in row-major order with |a| == max
        double big = -1.0; int kk = 0;
        if (lane < n && ipiv[lane] != 1)
            for (int k = 0; k < n; k++) {
                const int pk = ipiv[k];
                if (pk == 0) { const double v = fabs(A[lane*ns + k]); if (v >= big) { big = v; kk = k; } }
                else if (pk > 1) err = 1;
            }
        double vmax = big;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, off));
        int jsel = (big == vmax && big >= 0.0) ? lane : -1;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) jsel = max(jsel, __shfl_xor(jsel, off));
        if (jsel < 0) { err = 2; jsel = 0; }           // (nothing left to pivot on / NaN: reported like a vanishing pivot)
        const int irow = jsel, icol = __shfl(kk, jsel);
        __syncthreads();
        if (lane == 0) { ++ipiv[icol]; indxr[i] = irow; indxc[i] = icol; }
        if (irow != icol && lane < n) { const double t0 = A[irow*ns + lane]; A[irow*ns + lane] = A[icol*ns + lane]; A[icol*ns + lane] = t0; }
        __syncthreads();
        const double piv = A[icol*ns + icol];
        if (fabs(piv) < 1.0e-12) err = 2;
        const double pivinv = 1.0/piv;
        __syncthreads();
        if (lane < n) A[icol*ns + lane] = (lane == icol ? 1.0 : A[icol*ns + lane])*pivinv;
        __syncthreads();
        if (lane < n && lane != icol) {
            const double dum = A[lane*ns + icol];
            A[lane*ns + icol] = 0.0;
            for (int l = 0; l < n; l++) A[lane*ns + l] -= A[icol*ns + l]*dum;
        }
        __syncthreads();
    }
    for (int l = n - 1; l >= 0; l--) {
        const int ir = indxr[l], ic = indxc[l];
        if (ir != ic && lane < n) { const double t0 = A[lane*ns + ir]; A[lane*ns + ir] = A[lane*ns + ic]; A[lane*ns + ic] = t0; }
        __syncthreads();
    }
    return err;
}

// ---- D: in place, one thread, every entry in a register; returns false when a natural-order pivot is too small (caller falls back)
template <int N2>
__device__ __forceinline__ bool reg_inverse(double (&P)[N2*N2]) {
    double dmax = 0.0;
#pragma unroll
    for (int i = 0; i < N2; i++) dmax = fmax(dmax, fabs(P[i*N2 + i]));
    bool ok = true;
#pragma unroll
    for (int p = 0; p < N2; p++) {
        const double piv = P[p*N2 + p];
        if (!(fabs(piv) >= 1.0e-8*dmax) || !(fabs(piv) >= 1.0e-12)) ok = false;
        const double pinv = 1.0/piv;
        P[p*N2 + p] = 1.0;
#pragma unroll
        for (int cc = 0; cc < N2; cc++) P[p*N2 + cc] *= pinv;
#pragma unroll
        for (int r = 0; r < N2; r++) {
            if (r == p) continue;
            const double d = P[r*N2 + p];
            P[r*N2 + p] = 0.0;
#pragma unroll
            for (int cc = 0; cc < N2; cc++) P[r*N2 + cc] -= P[p*N2 + cc]*d;
        }
    }
    return ok;
}

// ---- F: one round of the arg-max over a row of 16 lanes: rotation by K (ties -> lowest lane, so every lane agrees)
template <int K> __device__ __forceinline__ void row_argmax(double& cand, int& bl) {
    const double oc = row_ror<K>(cand); const int ol = row_ror<K>(bl);
    if (oc > cand || (oc == cand && ol < bl)) { cand = oc; bl = ol; }
}
// in-place Gauss-Jordan inverse with ONE ROW PER LANE (row r of the block in lane r of each group of GW lanes, idle lanes !act), implicit
// row pivoting: rows are never swapped -- the lane chosen at step c keeps the row and remembers c (myc); piv[c] is the pivot lane of
// step c.  The in-place result then satisfies  D^-1[myc of lane l][piv[c]] = T[c] of lane l, which is how the callers scatter it into LDS.
template <int N2, int GW>
__device__ __forceinline__ void rows_gauss_jordan(double (&T)[N2], int r, bool act, int& myc, int (&piv)[N2]) {
    static_assert(N2 <= GW && (GW == 16 || GW == 32), "one lane per block row; 16 or 32 lanes per block");
    bool used = !act;
    myc = 0;
#pragma unroll
    for (int c = 0; c < N2; c++) {
        double cand = used ? -1.0 : fabs(T[c]);
        int bl = r;
        row_argmax<1>(cand, bl); row_argmax<2>(cand, bl); row_argmax<4>(cand, bl); row_argmax<8>(cand, bl);
        if constexpr (GW == 32) {            // the two 16-lane rows of the block compare notes
            const double oc = __shfl_xor(cand, 16, 32); const int ol = __shfl_xor(bl, 16, 32);
            if (oc > cand || (oc == cand && ol < bl)) { cand = oc; bl = ol; }
        }
        piv[c] = bl;
        double pr[N2];
#pragma unroll
        for (int j = 0; j < N2; j++) pr[j] = __shfl(T[j], bl, GW);
        const double pinv = 1.0/pr[c];
#pragma unroll
        for (int j = 0; j < N2; j++) pr[j] *= pinv;          // the scaled pivot row: what its lane keeps and the others subtract
        if (r == bl) {
#pragma unroll
            for (int j = 0; j < N2; j++) T[j] = pr[j];
            T[c] = pinv; used = true; myc = c;
        } else {
            const double fct = T[c];
#pragma unroll
            for (int j = 0; j < N2; j++) T[j] -= fct*pr[j];
            T[c] = -fct*pinv;
        }
    }
}

}  // namespace mimsem
