// energetics.inc -- mimsem_euler_energetics_horiz (include/mimsem_hip.h): the four horizontal integrals of Euler::diagnostics
// (eul/Euler_2.cpp:600-744) over all levels in ONE element pass plus a small fixed-order final pass.  A fused element pass on the
// unit layer of elem_unit.hpp, as a fixed-stride walk.
//
//   keh  = 1/2 sum_k velx_k . F(rho_k, k, vert) velx_k / SCALE      (:630-636; coefficients Uhmat::assemble eul/Assembly.cpp:432-448)
//   ie   = CV/CP sum_k rt_k . M2(k, vert) exner_k / SCALE           (:667-673; Wmat::assemble eul/Assembly.cpp:347-353)
//   entr = 1/2 sum_k theta_k . M2(k, vert) rt_k / SCALE             (:706-711)
//   mass = sum_k int2(rho_k)                                        (:570-598, :686-690)
//
// Every term is a sum over elements of a sum over quadrature points: the 1-form term is the quadratic form sum_e x_e^T A_e x_e (no
// scatter), 2-forms are discontinuous.  With t = thickInv[k][q], w = w_qx w_qy, d = det[e][q], J = [[a, b], [c, e]] and the LOCAL
// interpolants (u, v) of velx (before the Piola map, as Uhmat has them) and r, T, P, h of rho, rt, exner, theta at the point:
//   keh_q = u (caa u + cab v) + v (cab u + cbb v),   caa = (r/d t)(a^2 + c^2) w/d t,  cab = (r/d t)(a b + c e) w/d t,  cbb = (r/d t)(b^2 + e^2) w/d t
//   ie_q  = T P w/d t        entr_q = h T w/d t        mass_q = d w (r/d)
// (the SCALE of the assembled matrices and the reference's 1/SCALE cancel).
//
// Work item = (level, element) as k_interp_quad numbers them; lane q owns quadrature point q.  A unit reads velx once through the 1-form
// maps (2 n1e doubles), rho, rt, exner, theta once as contiguous 2-form blocks (4 n2e), J, det, thickInv once (6 mp12): at p = 3
// 24 + 36 + 96 = 156 doubles = 1 248 bytes, at p = 4 40 + 64 + 150 = 254 doubles = 2 032 bytes.
//
// Reduction, no atomics: a block walks its units with a fixed stride and every lane accumulates its own points in that order; the 64
// lanes of a wave are summed by the shuffle tree (offsets 32, 16, .., 1), the four waves as (w0 + w1) + (w2 + w3), and the block leaves ONE
// partial 4-vector in the context's reduction workspace.  A second launch of four waves sums the partials of one term each (lane l takes
// partials l, l + 64, .., then the same tree) and applies the constant factor.  The grid depends on (nEl, nlev, order) only: two calls on
// the same input give the same bits.
namespace {

constexpr int EN_MAX_BLOCKS = 2048;      // 8 workgroups of 256 on each of the 256 CUs; more units than that: blocks take several

struct EnergeticsArgs {
    ElemTables t;
    int nlev;
    const double* u; long long us;
    const double* rho; long long rs;
    const double* rt; long long ts;
    const double* ex; long long es;
    const double* th; long long hs;
    double* part;                        // [gridDim.x][4]
};

__device__ __forceinline__ double en_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

template <int N>
__global__ __launch_bounds__(256) void k_energetics_horiz(EnergeticsArgs a) {
    using D = Dims<N>;
    constexpr int LPE = D::LPE, EPB = D::EPB;
    __shared__ double sE[D::mp1*N];
    __shared__ double s_u[EPB][2*LPE];
    __shared__ double s_r[EPB][LPE], s_t[EPB][LPE], s_p[EPB][LPE], s_h[EPB][LPE];
    __shared__ double red[4][4];
    const Lane ln = lane_of_thread<N>();
    const int tid = threadIdx.x, el = ln.el, q = ln.q, qx = ln.qx, qy = ln.qy;
    stage_edge_table<N>(sE, a.t.E);
    const double Q = q < D::mp12 ? a.t.w[qx]*a.t.w[qy] : 0.0;        // once per lane, not per unit of the walk (PointMetric::Q is not used)
    const long long total = (long long)a.t.nEl*a.nlev;
    double keh = 0.0, ie = 0.0, en = 0.0, ms = 0.0;
    __syncthreads();                     // sE (the only block-level barrier of the loop: an element's lanes share a wave)
    for (long long base = (long long)blockIdx.x*EPB; base < total; base += (long long)gridDim.x*EPB) {      // (block-uniform trip count)
        const Unit un = unit_of(base + el, a.t.nEl, a.nlev);
        const bool act = un.act;
        const int lev = un.lev, e = un.e;
        if (act) {
            if (q < D::n1e) stage_form1<N>(form1_slots<N>(a.t, e, q), q, a.u + (size_t)lev*a.us, s_u[el]);
            if (q < D::n2e) {
                const size_t s = form2_slot<N>(a.t.i2, e, q);
                s_r[el][q] = a.rho[(size_t)lev*a.rs + s]; s_t[el][q] = a.rt[(size_t)lev*a.ts + s];
                s_p[el][q] = a.ex[(size_t)lev*a.es + s]; s_h[el][q] = a.th[(size_t)lev*a.hs + s];
            }
        }
        wave_lds_sync();
        if (act && q < D::mp12) {
            const PointMetric g = point_metric<N>(a.t, lev, e, q);
            double u, v, r, T, P, h, dmy;
            interp_point<N, S1>(s_u[el], sE, q, qx, qy, u, v);
            interp_point<N, S2>(s_r[el], sE, q, qx, qy, r, dmy);
            interp_point<N, S2>(s_t[el], sE, q, qx, qy, T, dmy);
            interp_point<N, S2>(s_p[el], sE, q, qx, qy, P, dmy);
            interp_point<N, S2>(s_h[el], sE, q, qx, qy, h, dmy);
            const double det = g.det, tI = g.tI, sd = 1.0/det;
            const double rq = r/det;                                  // interp2_g
            const double hi = rq*tI;
            const double caa = hi*(g.J00*g.J00 + g.J10*g.J10)*Q*sd*tI;        // Uhmat::assemble, vert_scale
            const double cab = hi*(g.J00*g.J01 + g.J10*g.J11)*Q*sd*tI;
            const double cbb = hi*(g.J01*g.J01 + g.J11*g.J11)*Q*sd*tI;
            const double c2 = Q*sd*tI;                                // Wmat::assemble, vert_scale
            keh += u*(caa*u + cab*v) + v*(cab*u + cbb*v);
            ie += T*(c2*P);
            en += h*(c2*T);
            ms += det*Q*rq;                                           // int2
        }
        wave_lds_sync();                 // the unit's rows are read before the next unit's are stored
    }
    const int lane = tid & 63, wave = tid >> 6;
    keh = en_wave_sum(keh); ie = en_wave_sum(ie); en = en_wave_sum(en); ms = en_wave_sum(ms);
    if (lane == 0) { red[wave][0] = keh; red[wave][1] = ie; red[wave][2] = en; red[wave][3] = ms; }
    __syncthreads();
    if (tid < 4) a.part[(size_t)blockIdx.x*4 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// wave t sums term t of the nb partial NT-vectors in a fixed order and applies its constant factor (NT waves; log_entropy.inc has NT = 1)
template <int NT>
__global__ __launch_bounds__(64*NT) void k_energetics_final(int nb, const double* __restrict__ part, double f0, double f1, double f2, double f3,
                                                            double* __restrict__ out) {
    const int lane = threadIdx.x & 63, t = threadIdx.x >> 6;
    double s = 0.0;
    for (int i = lane; i < nb; i += 64) s += part[(size_t)i*NT + t];
    s = en_wave_sum(s);
    if (lane == 0) out[t] = s*(t == 0 ? f0 : (t == 1 ? f1 : (t == 2 ? f2 : f3)));
}

template <int N>
int energetics_horiz_n(mimsem_ctx* c, EnergeticsArgs& a, double* out) {
    using D = Dims<N>;
    const long long total = (long long)a.t.nEl*a.nlev;
    const int nb = (int)std::max<long long>(1, std::min<long long>(EN_MAX_BLOCKS, (total + D::EPB - 1)/D::EPB));
    const int rc = c->ensure_kry((long long)nb*4);                    // (grows outside a capture only: MIMSEM_ERR_STATE inside one)
    if (rc) return rc;
    a.part = c->d_kry;
    hipLaunchKernelGGL((k_energetics_horiz<N>), dim3(nb), dim3(256), 0, c->stream, a);
    MIMSEM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_energetics_final<4>, dim3(1), dim3(256), 0, c->stream, nb, (const double*)c->d_kry, 0.5, 717.5/1004.5, 0.5, 1.0, out);      // CV/CP eul/Euler_2.cpp:29-30
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

// ---- the column half: kev, k2p, p2k, pe (eul/Euler_2.cpp:638-664, :675-684) in one pass over velz, rho and zv ------------------------
//
//   kev = 1/2 sum_e rho_e . CONLIN_W(velz_e) velz_e / SCALE       k2p = sum_e gi_e . (V01 zv_e) / SCALE
//   p2k = sum_e (V10 gi_e) . zv_e / SCALE                         pe  = sum_e zv_e . rho_e / SCALE
//   gi_e = LINEAR_INV LINEAR_RT(rho_e, vert) velz_e               (AssembleLinearInv / AssembleLinearWithRT eul/VertOps.cpp:422-430, :621-662)
//
// all in the vertical layout (velz [nEl][(nk-1) n2e], rho and zv [nEl][nk n2e]).  The W^T diag(c) W blocks of CONLIN_W and LINEAR_RT are
// never formed: with R_k, V_i the interpolants of rho_k, velz_i at quadrature point q (wint of column_kernels.hip) and q0 = SCALE w_q / det_q
//   rho_k . (CONLIN_W(velz) velz)_k = sum_q R_k q0 (1/2 V_{k-1}/det) V_{k-1} + R_k q0 (1/2 V_k/det) V_k          (VertOps.cpp:551-600)
//   (LINEAR_RT(rho) velz)_i[j]      = sum_q W[q][j] (q0 (1/2 R_i/det) + q0 (1/2 R_{i+1}/det)) V_i                (do_internal: no thickness)
// LINEAR_INV is the one factor that is not a quadrature sum: its blocks [nEl][nk-1][n2e][n2e] are READ (the ones mimsem_colop_blocks made
// once per mesh, VertSolve keeps the same), not recomputed -- a fully pivoted Gauss-Jordan of an n2e x n2e block per interface and call
// would cost n2e^3 dependent flops where the read costs n2e^2 doubles, and the cached blocks keep gi equal to the composed route's.
//
// Work item = column (element), lanes and groups as k_energetics_horiz: lane q of a group of LPE owns quadrature point q and, for q < n2e,
// DoF q.  Levels are walked in order; at level k the lane holds R_{k-1}, V_{k-1} in registers, so interface k-1 is finished there:
// t_q -> LDS, b = W^T t (lane j, mp12 terms), gi_{k-1}[j] = LINEAR_INV[k-1][j][:] . b; gi of the previous interface and zv of the previous
// level stay in registers, so (V10 gi)_{k-1} = gi_{k-1} - gi_{k-2} and (V01 zv)_{k-1} = zv_k - zv_{k-1} need no global intermediate.  Every
// input is read once.  Blocks are ONE wave (64 threads, 64/LPE columns): a column is a serial walk of nk levels, so many small blocks
// spread the columns over the CUs (3 456 columns at the bench mesh are 864 blocks; 256-thread blocks would leave 40 CUs idle).
// Reduction as above: fixed-stride walk over the columns, shuffle tree 32..1, one partial 4-vector per block, k_energetics_final.
constexpr double EN_SCALE = 1.0e+8;      // eul/VertOps.cpp:21

struct EnColumnArgs {
    int nEl, nk;
    const double *det, *E, *w;
    const double *velz, *rho, *zv, *Ainv;
    double* part;                        // [gridDim.x][4]
};

template <int N>
__global__ __launch_bounds__(64) void k_energetics_column(EnColumnArgs a) {
    using D = Dims<N>;
    constexpr int LPE = D::LPE, EPB = 64/LPE, n2 = D::n2e, nn = n2*n2;
    __shared__ double sE[D::mp1*N];
    __shared__ double s_r[EPB][LPE], s_v[EPB][LPE], s_t[EPB][LPE], s_b[EPB][LPE];
    const Lane ln = lane_of_thread<N>();
    const int tid = threadIdx.x, el = ln.el, q = ln.q, qx = ln.qx, qy = ln.qy;
    stage_edge_table<N>(sE, a.E);
    const double Q = q < D::mp12 ? a.w[qx]*a.w[qy] : 0.0;
    const int nk = a.nk, ni = a.nk - 1;
    double kev = 0.0, k2p = 0.0, p2k = 0.0, pe = 0.0;
    wave_lds_sync();                     // sE (a block is one wave)
    for (int base = blockIdx.x*EPB; base < a.nEl; base += gridDim.x*EPB) {        // (block-uniform trip count)
        const int e = base + el;
        const bool act = e < a.nEl, pt = act && q < D::mp12, dof = act && q < n2;
        const double det = pt ? a.det[(size_t)e*D::mp12 + q] : 1.0;
        const double q0 = Q*(EN_SCALE/det);
        const double* ve = a.velz + (size_t)e*ni*n2;
        const double* re = a.rho + (size_t)e*nk*n2;
        const double* ze = a.zv + (size_t)e*nk*n2;
        const double* Ae = a.Ainv + (size_t)e*ni*nn + (size_t)q*n2;  // row q of the column's first block
        double Rp = 0.0, Vp = 0.0, zp = 0.0, gp = 0.0;                // level / interface k - 1: R, V at the point; zv, gi at the DoF
        for (int k = 0; k < nk; k++) {
            double zk = 0.0;
            if (dof) {
                const double rk = re[k*n2 + q];
                zk = ze[k*n2 + q];
                s_r[el][q] = rk; s_v[el][q] = k < ni ? ve[k*n2 + q] : 0.0;
                pe += zk*rk;
            }
            wave_lds_sync();
            double R = 0.0, V = 0.0, dmy;
            if (pt) {
                interp_point<N, S2>(s_r[el], sE, q, qx, qy, R, dmy);
                interp_point<N, S2>(s_v[el], sE, q, qx, qy, V, dmy);
                kev += R*((q0*(0.5*Vp/det))*Vp + (q0*(0.5*V/det))*V);             // rho_k . (CONLIN_W(velz) velz)_k
                if (k > 0) s_t[el][q] = (q0*(0.5*Rp/det) + q0*(0.5*R/det))*Vp;    // LINEAR_RT(rho, vert) of interface k - 1 times V_{k-1}
            }
            wave_lds_sync();             // s_r, s_v read; s_t stored
            if (k > 0) {
                if (dof) s_b[el][q] = project2<N>(sE, s_t[el], q);
                wave_lds_sync();
                if (dof) {
                    const double* Ar = Ae + (size_t)(k - 1)*nn;
                    double g = 0.0;
#pragma unroll
                    for (int m = 0; m < n2; m++) g += Ar[m]*s_b[el][m];
                    k2p += g*(zk - zp);                               // gi_{k-1} . (V01 zv)_{k-1}
                    p2k += (g - gp)*zp;                               // (V10 gi)_{k-1} . zv_{k-1}
                    gp = g;
                }
            }
            Rp = R; Vp = V; zp = zk;
        }
        p2k += (0.0 - gp)*zp;                                         // (V10 gi)_{nk-1} = -gi_{nk-2}
        wave_lds_sync();                 // the column's last s_b reads are done before the next column's stores
    }
    kev = en_wave_sum(kev); k2p = en_wave_sum(k2p); p2k = en_wave_sum(p2k); pe = en_wave_sum(pe);
    if (tid == 0) {
        double* o = a.part + (size_t)blockIdx.x*4;
        o[0] = kev; o[1] = k2p; o[2] = p2k; o[3] = pe;
    }
}

template <int N>
int energetics_column_n(mimsem_ctx* c, EnColumnArgs& a, double* out) {
    constexpr int EPB = 64/Dims<N>::LPE;
    const int nb = std::max(1, std::min(EN_MAX_BLOCKS, (a.nEl + EPB - 1)/EPB));
    const int rc = c->ensure_kry((long long)nb*4);                    // (grows outside a capture only: MIMSEM_ERR_STATE inside one)
    if (rc) return rc;
    a.part = c->d_kry;
    hipLaunchKernelGGL((k_energetics_column<N>), dim3(nb), dim3(64), 0, c->stream, a);
    MIMSEM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_energetics_final<4>, dim3(1), dim3(256), 0, c->stream, nb, (const double*)c->d_kry, 0.5/EN_SCALE, 1.0/EN_SCALE, 1.0/EN_SCALE,
                       1.0/EN_SCALE, out);
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

}  // namespace

// Euler::diagnostics' column sums (eul/Euler_2.cpp:638-664 kev, k2p, p2k; :675-684 pe), which the reference forms column by column with
// AssembleConLinWithW / AssembleLinearWithRT / AssembleLinearInv + MatMult + VecDot
extern "C" int mimsem_euler_energetics_column(mimsem_ctx* c, const double* velz, const double* rho, const double* zv, const double* linear_inv,
                                              double* out) {
    if (!c || !velz || !rho || !zv || !linear_inv || !out) return MIMSEM_ERR_ARG;
    if (c->nk < 2) return MIMSEM_ERR_ARG;
    if (c->es.n > 4) return MIMSEM_ERR_UNSUPPORTED;
    if (!c->d_det || !c->d_E || !c->d_w) return MIMSEM_ERR_STATE;
    EnColumnArgs a{};
    a.nEl = c->nEl; a.nk = c->nk;
    a.det = c->d_det; a.E = c->d_E; a.w = c->d_w;
    a.velz = velz; a.rho = rho; a.zv = zv; a.Ainv = linear_inv;
    return for_order<1, 4>(c->es.n, [&](auto n) { return energetics_column_n<decltype(n)::value>(c, a, out); });
}

extern "C" int mimsem_euler_energetics_horiz(mimsem_ctx* c, int nlev, const double* velx, long long ldu, const double* rho, long long ldr,
                                             const double* rt, long long ldt, const double* exner, long long lde,
                                             const double* theta, long long ldth, double* out) {
    if (!c || !velx || !rho || !rt || !exner || !theta || !out) return MIMSEM_ERR_ARG;
    if (nlev < 1 || nlev > c->nk || ldu < 0 || ldr < 0 || ldt < 0 || lde < 0 || ldth < 0) return MIMSEM_ERR_ARG;
    EnergeticsArgs a{};
    if (int rc = elem_tables(c, 0, a.t)) return rc;
    a.nlev = nlev;
    a.u = velx; a.us = ldu; a.rho = rho; a.rs = ldr; a.rt = rt; a.ts = ldt; a.ex = exner; a.es = lde; a.th = theta; a.hs = ldth;
    return for_order<1, 7>(c->es.n, [&](auto n) { return energetics_horiz_n<decltype(n)::value>(c, a, out); });
}
