// elem_unit.hpp -- the frame of a point-per-lane element kernel: what the fused element passes of elem_kernels.hip (energetics.inc,
// flux_rhs.inc, momentum_forcing.inc, zonal_stats.inc, log_entropy.inc, k_interp_quad) have around their arithmetic; a new pass starts from here (DESIGN.md
// 4.3).  bernoulli.inc and tsw_kernels.hip spell the same frame out themselves (profiles/elem_unit_layer.txt section 4 says why).
// Layout: a unit is one (level, element); LPE lanes carry it, lane q owns quadrature point q and, where q is small enough, DoF q / the
// edge pair q.  LPE divides 64, so an element's lanes share a wave: hand-offs through LDS rows need wave_lds_sync() only; the edge table
// sE belongs to the block and needs one __syncthreads() after stage_edge_table.
// Bounds, once for every user: a lane that is not `act` or is past the element's DoFs / points loads and stores nothing (the slot, staging
// and metric helpers are called under the caller's q < n1e / n2e / mp12); an active unit has (lev, e) < (nlev, nEl), so e*n1e + q,
// e*n2e + q, e*mp12 + q index inside the context's tables, whose slots were checked when the context was made.  thickInv is
// [nk][nEl][mp12]: point_metric's lev must be below the CONTEXT's nk; k_interp_quad, whose entry does not bound nlev by it, passes 0.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "ctx.hpp"

namespace {

template <int N> struct Dims {
    static constexpr int n = N, np1 = N + 1, mp1 = N + 1, mp12 = mp1*mp1;
    static constexpr int n0e = np1*np1, n1e = np1*N, n2e = N*N;
    static constexpr int LPE = (mp12 <= 4) ? 4 : (mp12 <= 16 ? 16 : (mp12 <= 32 ? 32 : 64));
    static constexpr int BLOCK = 256, EPB = BLOCK/LPE;
};

enum Space { S0 = 0, S1 = 1, S2 = 2, SN = 3, SQ = 4, SQ2 = 5 };   // SQ/SQ2: scalar / interleaved vector on the quad-point grid

// Lanes of one element never span wavefronts (LPE divides 64), so the LDS hand-offs between the lanes of
// an element need only wave-level ordering, not s_barrier: LDS operations of one wave execute in order.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// value(s) of a staged field at quad point (qx,qy): collocated tables => short 1-D sums
template <int N, Space SP>
__device__ __forceinline__ void interp_point(const double* dofs, const double* sE, int q, int qx, int qy,
                                             double& u, double& v) {
    using D = Dims<N>;
    u = 0.0; v = 0.0;
    if constexpr (SP == S1) {           // Geom::interp1_l eul/Geom.cpp:342-361 with l_j(x_q) = delta_jq
#pragma unroll
        for (int j = 0; j < N; j++) {
            u += dofs[j*D::np1 + qx]*sE[qy*N + j];
            v += dofs[D::n1e + qy*N + j]*sE[qx*N + j];
        }
    } else if constexpr (SP == S2) {    // Geom::interp2_l :363-376
#pragma unroll
        for (int jy = 0; jy < N; jy++)
#pragma unroll
            for (int jx = 0; jx < N; jx++)
                u += dofs[jy*N + jx]*(sE[qx*N + jx]*sE[qy*N + jy]);
    } else if constexpr (SP == S0 || SP == SQ) {    // Geom::interp0 :328-340 (collocated) / a quad-grid value
        u = dofs[q];
    } else if constexpr (SP == SQ2) {
        u = dofs[q]; v = dofs[D::mp12 + q];
    }
}

// the ten context tables every such kernel reads; per-kernel argument structs embed one (elem_tables fills it)
struct ElemTables {
    int nEl;
    const int *i1x, *i1y, *i2;           // element slot tables (i2 null: element-contiguous 2-forms)
    const double *J, *det, *tI, *E, *w;  // metric [nEl][4][mp12], [nEl][mp12]; inverse thickness [nk][nEl][mp12]; edge table [mp1][n]; GLL weights
    const int* i0;                       // node slots (elem_tables checks them for the callers that say NEED_I0)
};

// the lane: element el of the block, point / DoF q = (qx, qy)
struct Lane { int el, q, qx, qy; };
template <int N, int LPE = Dims<N>::LPE>
__device__ __forceinline__ Lane lane_of_thread() {
    const int tid = threadIdx.x, q = tid%LPE;
    return Lane{tid/LPE, q, q%Dims<N>::mp1, q/Dims<N>::mp1};
}

// the unit: index eg = blockIdx.x*EPB + el of a one-shot kernel, base + el of a fixed-stride walk; units number (level, element)
struct Unit { bool act; int lev, e; };
__device__ __forceinline__ Unit unit_of(long long eg, int nEl, int nlev) {
    const bool act = eg < (long long)nEl*nlev;
    return Unit{act, act ? (int)(eg/nEl) : 0, act ? (int)(eg%nEl) : 0};
}

// the block's edge table; the caller's next block-level barrier covers it
template <int N>
__device__ __forceinline__ void stage_edge_table(double* sE, const double* E) {
    if (threadIdx.x < Dims<N>::mp1*N) sE[threadIdx.x] = E[threadIdx.x];
}

// the vector slots of the x edge q and the y edge q of element e; for the lanes q < n1e
template <int N>
__device__ __forceinline__ int2 form1_slots(const ElemTables& t, int e, int q) {
    return make_int2(t.i1x[e*Dims<N>::n1e + q], t.i1y[e*Dims<N>::n1e + q]);
}

// one level row of a 1-form through those slots into the LDS row [2*LPE]: x edges, then y edges; for the lanes q < n1e
template <int N>
__device__ __forceinline__ void stage_form1(int2 s, int q, const double* row, double* dst) {
    dst[q] = row[s.x]; dst[Dims<N>::n1e + q] = row[s.y];
}

// the vector slot of 2-form DoF q of element e; for the lanes q < n2e
template <int N>
__device__ __forceinline__ size_t form2_slot(const int* i2, int e, int q) {
    return i2 ? (size_t)i2[(size_t)e*Dims<N>::n2e + q] : (size_t)e*Dims<N>::n2e + q;
}

// the metric at the lane's point (q < mp12): Jacobian, determinant, inverse thickness of the level, Q = w_qx w_qy.  Straight-line on
// purpose: a branch in here lets the optimiser sink the loads in reverse order, which changes the operand ranks and with them which product
// of an a*b + c*d the backend fuses -- other bits.  A caller that uses some members only relies on the compiler to drop the other loads
// (all in bounds under the rules above); profiles/elem_unit_layer.txt checks that it does (equal global_ counts).
struct PointMetric { double J00, J01, J10, J11, det, tI, Q; };
template <int N>
__device__ __forceinline__ PointMetric point_metric(const ElemTables& t, int lev, int e, int q) {
    using D = Dims<N>;
    const size_t gq = (size_t)e*D::mp12 + q;
    const double* Je = t.J + (size_t)e*4*D::mp12;
    PointMetric g;
    g.J00 = Je[0*D::mp12 + q]; g.J01 = Je[1*D::mp12 + q]; g.J10 = Je[2*D::mp12 + q]; g.J11 = Je[3*D::mp12 + q];
    g.det = t.det[gq]; g.tI = t.tI[(size_t)lev*((size_t)t.nEl*D::mp12) + gq];
    g.Q = t.w[q%D::mp1]*t.w[q/D::mp1];
    return g;
}

// W^T: 2-form DoF q of the element from the point values c [mp12]  (sum_p W[p][q] c_p, fixed order)
template <int N>
__device__ __forceinline__ double project2(const double* sE, const double* c, int q) {
    using D = Dims<N>;
    const int jx = q%N, jy = q/N;
    double y = 0.0;
#pragma unroll
    for (int py = 0; py < D::mp1; py++)
#pragma unroll
        for (int px = 0; px < D::mp1; px++) y += (sE[px*N + jx]*sE[py*N + jy])*c[py*D::mp1 + px];
    return y;
}

// Ut^T / Vt^T: the x edge q and the y edge q of the element from the point values cx, cy [mp12] (collocated nodes: mp1 terms each)
template <int N>
__device__ __forceinline__ void project1(const double* sE, const double* cx, const double* cy, int q, double& yx, double& yy) {
    using D = Dims<N>;
    const int ixx = q%D::np1, iyx = q/D::np1;     // x-normal edge: node in x, edge fn in y
    const int ixy = q%N,      iyy = q/N;          // y-normal edge: edge fn in x, node in y
    yx = 0.0; yy = 0.0;
#pragma unroll
    for (int k = 0; k < D::mp1; k++) {
        yx += sE[k*N + iyx]*cx[k*D::mp1 + ixx];
        yy += sE[k*N + ixy]*cy[iyy*D::mp1 + k];
    }
}

// host side
enum : unsigned { NEED_I0 = 1u, NEED_G1 = 2u };           // the optional tables of elem_tables' state check

// the context's tables, or MIMSEM_ERR_STATE where one is missing (`need`: which of d_i0, d_g1 the caller reads as well)
inline int elem_tables(const mimsem_ctx* c, unsigned need, ElemTables& t) {
    if (!c->d_J || !c->d_det || !c->d_tI || !c->d_E || !c->d_w || !c->d_i1x || !c->d_i1y) return MIMSEM_ERR_STATE;
    if (((need & NEED_I0) && !c->d_i0) || ((need & NEED_G1) && !c->d_g1)) return MIMSEM_ERR_STATE;
    t = ElemTables{c->nEl, c->d_i1x, c->d_i1y, c->d_i2, c->d_J, c->d_det, c->d_tI, c->d_E, c->d_w, c->d_i0};
    return MIMSEM_OK;
}

// f(std::integral_constant<int, N>{}) for N == n in LO .. HI, MIMSEM_ERR_UNSUPPORTED for every other n
template <int LO, int HI, class F>
int for_order(int n, F&& f) {
    if constexpr (LO > HI) return MIMSEM_ERR_UNSUPPORTED;
    else return n == LO ? f(std::integral_constant<int, LO>{}) : for_order<LO + 1, HI>(n, f);
}

// one 256-thread block per EPB = 256/LPE units
template <int N, class A>
int launch_units(mimsem_ctx* c, void (*kernel)(A), long long units, const A& a) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((units + Dims<N>::EPB - 1)/Dims<N>::EPB)), dim3(256), 0, c->stream, a);
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

}  // namespace
