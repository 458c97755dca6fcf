// elem_block_pc.inc -- mimsem_elem_block_pc_build and mimsem_elem_block_pc_build_levels (include/mimsem_hip.h): the element-block
// preconditioner of a 1-form mass operator (the levels entry: of every row of a batch, UTMAT_H included) in ONE capturable launch.  Included at the end of elem_kernels.hip, whose per-point coefficient functor (qpoint_op), field staging (stage_dofs,
// interp_point) and element-matrix sums (k_elmats) it shares, so that every entry is formed by the same operations in the same order.
//
// Reference: PCSetUp of ksp1h after M1h->assemble(h) (src/ThermalSW_EEC_2.cpp:253-268) -- the PCBJACOBI blocks of mimsem_ksp_set_pc_bjacobi,
// out_e = D_e (A_e)^-1 D_e with A_e the element's dense 2 n1e x 2 n1e block and D_e = 1 / (elements sharing the edge).  That builder composes
// launch_elmats -> k_em_to_block -> mimsem_block_inverse -> k_scale_blocks with device allocations and a synchronisation; here one wavefront
// per element does all four steps in LDS:
//   1. the per-point coefficients (aa, ab, bb) of the operator, as k_elmats probes them;
//   2. the block, entry (i, j) = sum_q (B_i(q) c(q)) B_j(q) over the points in ascending order (k_elmats' sum), written straight into the
//      [2 n1e][2 n1e] layout of k_em_to_block (rows and columns: x edges, then y edges);
//   3. Gauss-Jordan with full pivoting, lane = row: wave_pivot_inverse (small_block_inverse.hpp), the sweep k_block_inverse_wave runs
//      (LinAlg.cpp:186-269: the last entry of the row-major scan attaining the maximum, normalise, eliminate, un-permute the columns);
//   4. out = A^-1 * (d_i d_j), as k_scale_blocks forms it.
// Same operations in the same order: the same bits as mimsem_ksp_set_pc_bjacobi's blocks.  The block sits in LDS with an odd row stride
// (conflict-free row and column walks); the basis tables U, V beside it.  At p = 5: 60 x 61 doubles + 2 x 36 x 30 = 47 KB per workgroup.
namespace {

// the body of both kernels below: element blockIdx.x of row `row` (geometry level a.lev + row lev_step, field row a.f + row f_stride)
template <int N, int OP>
__device__ __forceinline__ void elem_block_pc_body(const ElmatArgs& a, const double* __restrict__ dw, int row, int lev_step, long long f_stride) {
    using D = Dims<N>;
    using T = OpTraits<OP>;
    static_assert(OP == MIMSEM_OP_UMAT || OP == MIMSEM_OP_UHMAT || OP == MIMSEM_OP_UTMAT_H, "1-form mass operators");
    constexpr int n1e = D::n1e, ND = 2*n1e, NS = ND | 1, MP = D::mp12;
    static_assert(ND <= 64 && MP <= 64, "one lane per block row and per quadrature point");
    __shared__ double sA[ND*NS];
    __shared__ double sU[MP*n1e], sV[MP*n1e];
    __shared__ double sE[D::mp1*N];
    __shared__ double s_f[2*64];
    __shared__ double c0[MP], c1[MP], c2[MP];
    __shared__ int ipiv[ND], indxr[ND], indxc[ND];
    const int e = blockIdx.x, lane = threadIdx.x;
    if (e >= a.nEl) return;                                      // (workgroup-uniform)
    const int glev = a.lev + row*lev_step;
    for (int t = lane; t < D::mp1*N; t += 64) sE[t] = a.E[t];
    for (int t = lane; t < MP*n1e; t += 64) { sU[t] = a.U[t]; sV[t] = a.V[t]; }
    if constexpr (T::cf != SN) {
        ElemArgs ea{}; ea.i0 = a.i0; ea.i1x = a.i1x; ea.i1y = a.i1y; ea.i2 = a.i2;
        stage_dofs<N, T::cf>(ea, a.f + (size_t)row*f_stride, e, lane, s_f);
    }
    if (lane < ND) ipiv[lane] = 0;
    __syncthreads();
    // 1. coefficients at the points (k_elmats)
    if (lane < MP) {
        const int q = lane, qx = q%D::mp1, qy = q/D::mp1;
        QPoint g;
        const double* Je = a.J + (size_t)e*4*MP;
        g.J00 = Je[q]; g.J01 = Je[MP + q]; g.J10 = Je[2*MP + q]; g.J11 = Je[3*MP + q];
        g.det = a.det[(size_t)e*MP + q];
        const size_t gl = ((size_t)glev*a.nEl + e)*MP + q;
        g.tI = a.tI[gl]; g.th0 = a.th[gl]; g.th1 = 1.0;
        g.Q = a.w[qx]*a.w[qy];
        g.tI0 = a.tI[(size_t)e*MP + q]; g.param = a.param;
        double fu = 0.0, fv = 0.0;
        if constexpr (T::cf != SN) interp_point<N, T::cf>(s_f, sE, q, qx, qy, fu, fv);
        double a10, b10, a01, b01;
        qpoint_op<OP>(g, a.scale, a.flags, 1.0, 0.0, fu, fv, a10, b10);
        qpoint_op<OP>(g, a.scale, a.flags, 0.0, 1.0, fu, fv, a01, b01);
        c0[q] = a10; c1[q] = a01; c2[q] = b01;
    }
    __syncthreads();
    // 2. the dense block (UtQU UtQV / VtQU VtQV)
    for (int t = lane; t < ND*ND; t += 64) {
        const int i = t/ND, j = t%ND;
        const int rowV = i >= n1e, colV = j >= n1e, ii = i - rowV*n1e, jj = j - colV*n1e;
        const double* Br = rowV ? sV : sU;
        const double* Bc = colV ? sV : sU;
        const double* cq = (!rowV && !colV) ? c0 : ((rowV && colV) ? c2 : c1);
        double s = 0.0;
        for (int qq = 0; qq < MP; qq++) s += (Br[qq*n1e + ii]*cq[qq])*Bc[qq*n1e + jj];
        sA[i*NS + j] = s;
    }
    __syncthreads();
    // 3. the inverse (error code dropped: PCSetUp does not report it)
    (void)mimsem::wave_pivot_inverse(sA, ND, NS, ipiv, indxr, indxc, lane);
    // 4. D_e A_e^-1 D_e, row-major, coalesced
    const double* de = dw + (size_t)e*ND;
    double* oe = a.out + ((size_t)row*a.nEl + e)*ND*ND;
    for (int t = lane; t < ND*ND; t += 64) {
        const int i = t/ND, j = t%ND;
        oe[t] = sA[i*NS + j]*(de[i]*de[j]);
    }
}

// mimsem_elem_block_pc_build: one row, one wavefront per element
template <int N, int OP>
__global__ __launch_bounds__(64) void k_elem_block_pc(ElmatArgs a, const double* __restrict__ dw) {
    elem_block_pc_body<N, OP>(a, dw, 0, 0, 0);
}
// mimsem_elem_block_pc_build_levels: the row is the grid's second dimension, nlev x nEl wavefronts
template <int N, int OP>
__global__ __launch_bounds__(64) void k_elem_block_pc_rows(ElmatArgs a, const double* __restrict__ dw, int lev_step, long long f_stride) {
    elem_block_pc_body<N, OP>(a, dw, blockIdx.y, lev_step, f_stride);
}

template <int N>
int elem_block_pc_n(mimsem_ctx* c, int op, const ElmatArgs& a, const double* dw) {
    if (op == MIMSEM_OP_UMAT) hipLaunchKernelGGL((k_elem_block_pc<N, MIMSEM_OP_UMAT>), dim3(a.nEl), dim3(64), 0, c->stream, a, dw);
    else hipLaunchKernelGGL((k_elem_block_pc<N, MIMSEM_OP_UHMAT>), dim3(a.nEl), dim3(64), 0, c->stream, a, dw);
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}
template <int N>
int elem_block_pc_rows_n(mimsem_ctx* c, int op, const ElmatArgs& a, const double* dw, int nlev, int lev_step, long long f_stride) {
    const dim3 grid(a.nEl, nlev);
    if (op == MIMSEM_OP_UMAT) hipLaunchKernelGGL((k_elem_block_pc_rows<N, MIMSEM_OP_UMAT>), grid, dim3(64), 0, c->stream, a, dw, lev_step, f_stride);
    else if (op == MIMSEM_OP_UHMAT) hipLaunchKernelGGL((k_elem_block_pc_rows<N, MIMSEM_OP_UHMAT>), grid, dim3(64), 0, c->stream, a, dw, lev_step, f_stride);
    else hipLaunchKernelGGL((k_elem_block_pc_rows<N, MIMSEM_OP_UTMAT_H>), grid, dim3(64), 0, c->stream, a, dw, lev_step, f_stride);
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

}  // namespace

int mimsem_pc_edge_weights(mimsem_ctx* c, const double** dw);      // ksp.hip

// the blocks of `nlev` rows in one launch: row r at geometry level geom_lev0 + r lev_step with the field row f + r f_stride (arguments checked
// by the two entries below); rows = false: the single-level entry's own kernel
static int elem_block_pc_rows(mimsem_ctx* c, int op, int geom_lev0, int lev_step, int nlev, double scale, unsigned flags,
                              const double* f, long long f_stride, double* out, bool rows) {
    if (c->nEl == 0 || nlev == 0) return MIMSEM_OK;
    if (!c->d_J || !c->d_det || !c->d_tI || !c->d_th || !c->d_U || !c->d_V) return MIMSEM_ERR_STATE;
    const double* dw = nullptr;
    int rc = mimsem_pc_edge_weights(c, &dw);                     // made once per context (outside a capture)
    if (rc) return rc;
    ElmatArgs a{};
    a.nEl = c->nEl; a.lev = geom_lev0; a.flags = flags; a.scale = scale;
    a.J = c->d_J; a.det = c->d_det; a.tI = c->d_tI; a.th = c->d_th; a.E = c->d_E; a.w = c->d_w;
    a.U = c->d_U; a.V = c->d_V; a.W = c->d_W; a.P = c->d_P;
    a.i0 = c->d_i0; a.i1x = c->d_i1x; a.i1y = c->d_i1y; a.i2 = c->d_i2;
    a.f = f; a.out = out;
    switch (c->es.n) {
    case 2: return rows ? elem_block_pc_rows_n<2>(c, op, a, dw, nlev, lev_step, f_stride) : elem_block_pc_n<2>(c, op, a, dw);
    case 3: return rows ? elem_block_pc_rows_n<3>(c, op, a, dw, nlev, lev_step, f_stride) : elem_block_pc_n<3>(c, op, a, dw);
    case 4: return rows ? elem_block_pc_rows_n<4>(c, op, a, dw, nlev, lev_step, f_stride) : elem_block_pc_n<4>(c, op, a, dw);
    case 5: return rows ? elem_block_pc_rows_n<5>(c, op, a, dw, nlev, lev_step, f_stride) : elem_block_pc_n<5>(c, op, a, dw);
    default: return MIMSEM_ERR_UNSUPPORTED;
    }
}

extern "C" int mimsem_elem_block_pc_build(mimsem_ctx* c, int op, int geom_lev, double scale, unsigned flags, const double* f, double* out) {
    if (!c || !out) return MIMSEM_ERR_ARG;
    if (op != MIMSEM_OP_UMAT && op != MIMSEM_OP_UHMAT) return MIMSEM_ERR_UNSUPPORTED;
    if (flags != 0u || c->es.n < 2 || c->es.n > 5) return MIMSEM_ERR_UNSUPPORTED;
    if ((op == MIMSEM_OP_UHMAT && !f) || geom_lev < 0 || geom_lev >= c->nk) return MIMSEM_ERR_ARG;
    return elem_block_pc_rows(c, op, geom_lev, 0, 1, scale, flags, f, 0, out, false);
}

// Euler::HorizPotVort (eul/Euler_2.cpp:1079-1092: M1t->assemble_h(i, SCALE, rho_h) + PCSetUp per interface) and HorizSolve::diagVertVort
// (eul/HorizSolve.cpp:843-855: F->assemble(rho_h, 0, false, SCALE) + PCSetUp per interface): every interface's blocks in one launch
extern "C" int mimsem_elem_block_pc_build_levels(mimsem_ctx* c, int op, int geom_lev0, int geom_lev_step, int nlev, double scale, unsigned flags,
                                                 const double* f, long long f_stride, double* out) {
    if (!c || !out) return MIMSEM_ERR_ARG;
    if (op != MIMSEM_OP_UMAT && op != MIMSEM_OP_UHMAT && op != MIMSEM_OP_UTMAT_H) return MIMSEM_ERR_UNSUPPORTED;
    if (flags != 0u || c->es.n < 2 || c->es.n > 5) return MIMSEM_ERR_UNSUPPORTED;
    if (geom_lev_step != 0 && geom_lev_step != 1) return MIMSEM_ERR_ARG;
    if (nlev < 0 || nlev > 65535 || f_stride < 0 || (op != MIMSEM_OP_UMAT && !f)) return MIMSEM_ERR_ARG;      // (rows are the grid's y dimension)
    if (geom_lev0 < 0 || geom_lev0 + (nlev > 0 ? (nlev - 1)*geom_lev_step : 0) >= c->nk) return MIMSEM_ERR_ARG;
    return elem_block_pc_rows(c, op, geom_lev0, geom_lev_step, nlev, scale, flags, f, f_stride, out, true);
}
