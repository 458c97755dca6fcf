// log_entropy.inc -- mimsem_euler_log_entropy (include/mimsem_hip.h): the entropy of the box twin's energetics line, slot 11
// (box/Euler_2.cpp:979-997), in ONE element pass plus a small fixed-order final pass.  A fused element pass on the unit layer of
// elem_unit.hpp, as a fixed-stride walk -- k_energetics_horiz with one field and a logarithm.
//
//   out = factor sum_rows lz[row] sum_e sum_q Q_q log((W theta_row)_q)               (:986-991; the reference's factor is CP, :997)
//
// (W theta)_q is the LOCAL 2-form interpolant at the point (interp_point<N, S2>; Ax_b with vert->vo->W at :987): no 1/det, no thickness --
// what mimsem_interp_quad gives without MIMSEM_INTERP_GLOBAL.  Q_q = w_qx w_qy (vert->vo->Q).
//
// Work item = (row, element) as k_interp_quad numbers them; lane q owns quadrature point q.  A unit reads theta once as a contiguous
// 2-form block (n2e doubles: 72 bytes at p = 3, 128 at p = 4), lz[row] once, and no metric: the kernel touches theta, lz, the edge table
// and the GLL weights only.  `nrows` is not bound by the context's nk (the box passes nk + 1 interfaces): nothing here is indexed by level
// but theta and lz themselves.
//
// Idle lanes: a lane with q >= mp12 and every lane of an inactive unit of the last block skips the interpolation AND the logarithm (the
// branch below), so its accumulator stays the 0.0 it started with -- log is never taken of an LDS word that was not staged.
//
// Reduction, no atomics, as energetics.inc: a block walks its units with a fixed stride and every lane accumulates its own points in that
// order; the 64 lanes of a wave are summed by the shuffle tree (en_wave_sum), the four waves as (w0 + w1) + (w2 + w3), and the block leaves
// ONE partial in the context's reduction workspace.  A second launch of one wave, k_energetics_final<1>, sums the partials (lane l takes
// partials l, l + 64, .., then the same tree) and applies the factor.  The grid depends on (nEl, nrows, order) only: two calls on the same
// input give the same bits.
namespace {

struct LogEntropyArgs {
    ElemTables t;
    int nrows;
    const double* th; long long hs;
    const double* lz;                    // [nrows]
    double* part;                        // [gridDim.x]
};

template <int N>
__global__ __launch_bounds__(256) void k_log_entropy(LogEntropyArgs a) {
    using D = Dims<N>;
    constexpr int LPE = D::LPE, EPB = D::EPB;
    __shared__ double sE[D::mp1*N];
    __shared__ double s_h[EPB][LPE];
    __shared__ double red[4];
    const Lane ln = lane_of_thread<N>();
    const int tid = threadIdx.x, el = ln.el, q = ln.q, qx = ln.qx, qy = ln.qy;
    stage_edge_table<N>(sE, a.t.E);
    const double Q = q < D::mp12 ? a.t.w[qx]*a.t.w[qy] : 0.0;        // once per lane, not per unit of the walk
    const long long total = (long long)a.t.nEl*a.nrows;
    double s = 0.0;
    __syncthreads();                     // sE (the only block-level barrier of the loop: an element's lanes share a wave)
    for (long long base = (long long)blockIdx.x*EPB; base < total; base += (long long)gridDim.x*EPB) {      // (block-uniform trip count)
        const Unit un = unit_of(base + el, a.t.nEl, a.nrows);
        const bool act = un.act;
        const int row = un.lev, e = un.e;
        if (act && q < D::n2e) s_h[el][q] = a.th[(size_t)row*a.hs + form2_slot<N>(a.t.i2, e, q)];
        wave_lds_sync();
        if (act && q < D::mp12) {
            double h, dmy;
            interp_point<N, S2>(s_h[el], sE, q, qx, qy, h, dmy);
            s += a.lz[row]*(Q*log(h));                                // :990
        }
        wave_lds_sync();                 // the unit's row is read before the next unit's is stored
    }
    const int lane = tid & 63, wave = tid >> 6;
    s = en_wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (tid == 0) a.part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

template <int N>
int log_entropy_n(mimsem_ctx* c, LogEntropyArgs& a, double factor, double* out) {
    using D = Dims<N>;
    const long long total = (long long)a.t.nEl*a.nrows;
    const int nb = (int)std::max<long long>(1, std::min<long long>(EN_MAX_BLOCKS, (total + D::EPB - 1)/D::EPB));
    const int rc = c->ensure_kry(nb);                                 // (grows outside a capture only: MIMSEM_ERR_STATE inside one)
    if (rc) return rc;
    a.part = c->d_kry;
    hipLaunchKernelGGL((k_log_entropy<N>), dim3(nb), dim3(256), 0, c->stream, a);
    MIMSEM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_energetics_final<1>, dim3(1), dim3(64), 0, c->stream, nb, (const double*)c->d_kry, factor, 0.0, 0.0, 0.0, out);   // one wave, one term
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

}  // namespace

// the entropy of box/Euler_2.cpp:979-997: theta on the nk + 1 interfaces in the horizontal layout, lz the layer weights of :988
extern "C" int mimsem_euler_log_entropy(mimsem_ctx* c, int nrows, const double* theta, long long theta_pitch, const double* lz, double factor,
                                        double* out) {
    if (!c || !theta || !lz || !out) return MIMSEM_ERR_ARG;
    if (nrows < 1 || theta_pitch < 0 || (theta_pitch > 0 && theta_pitch < c->n2)) return MIMSEM_ERR_ARG;      // (rows that overlap: refused)
    LogEntropyArgs a{};
    if (int rc = elem_tables(c, 0, a.t)) return rc;
    a.nrows = nrows;
    a.th = theta; a.hs = theta_pitch; a.lz = lz;
    return for_order<1, 7>(c->es.n, [&](auto n) { return log_entropy_n<decltype(n)::value>(c, a, factor, out); });
}
