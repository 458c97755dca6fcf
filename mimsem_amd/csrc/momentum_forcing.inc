// momentum_forcing.inc -- mimsem_horiz_momentum_forcing (include/mimsem_hip.h): the element-local forcing of HorizSolve::momentum_rhs
// (eul/HorizSolve.cpp:496-635, box/HorizSolve.cpp:412-526) for EVERY level in one element pass plus the 1-form gather.  Included at the end
// of elem_kernels.hip after flux_rhs.inc, whose lane-per-quadrature-point layout (Dims), LDS-staged edge table, interp_point and
// launch_gather_sum it shares.
//
// The reference adds three assembled operators into the level's right-hand side:
//   out_k (+)= R(q_k; level k, scale) a_k                              RotMat::assemble  (eul/Assembly.cpp:1051-1065, box/Assembly.cpp:826-882)
//            + F(th_k; level k, const_vert per flag) g_k               Uhmat::assemble   (eul/Assembly.cpp:432-448,  box/Assembly.cpp:273-326)
//            + 1/2 sum_{i in {k-1, k}, 0 <= i <= nk-2} Rh(dz_i; scale) v_i   UtQWmat::assemble (eul/Assembly.cpp:1504-1517, box/Assembly.cpp:1359-1410)
// Every one is Ut^T / Vt^T diag(c) B with the same 1-form test basis, so the three integrands are summed at the quadrature point before ONE
// projection.  With t = thickInv[k][q], d = det[e][q], J the Jacobian, Q = w_qx w_qy, m = scale Q / d,
//   Gaa = J00^2 + J10^2, Gab = J00 J01 + J10 J11, Gbb = J01^2 + J11^2, D = J00 J11 - J01 J10,
// (a_x, a_y), (g_x, g_y), (z_x, z_y)_i the LOCAL interpolants of a, g, dz_i (interp1_l, before the Piola map), q the nodal value of the
// 0-form at the (collocated) point, h the local interpolant of th and w_i that of v_i (interp2_l):
//   r        = m t^2 q D                                  rotational term:   (-r a_y, +r a_x)
//   f        = m t (h / d) (t with MIMSEM_FLAG_VERT)      pressure gradient: f (Gaa g_x + Gab g_y, Gab g_x + Gbb g_y)
//   s_i      = 1/2 m w_i / d  (no thickness)              second vorticity:  s_i (Gaa z_x + Gab z_y, Gab z_x + Gbb z_y)_i
//   ye_x[e,j] = sum_q Ut[j][q] c_x(q)    ye_y[e,j] = sum_q Vt[j][q] c_y(q)
// Ut[j][q] is l_jx(x_qx) e_jy(y_qy) with collocated nodes, so each sum has mp1 terms.  The element-local results [nk][nEl][2 n1e] go to the
// context's element workspace; launch_gather_sum(c, 1, ..) adds the (at most two) contributions of every edge slot in the plan's order, onto
// out with MIMSEM_FLAG_ACCUM.  Two launches, no atomics, a fixed summation order: two calls give the same bits.
//
// Each of the pairs (q, a), (th, g), (dz, v) may be absent (both NULL): a kernel-argument branch, uniform over the grid, skips its loads
// and its integrand.  The loads of an inactive lane (a unit past the end, a lane past the element's DoFs or points) and of the interfaces
// -1 and nk-1 sit inside their branch: nothing is loaded from a clamped address and thrown away.
//
// Work item = (level, element) as k_horiz_flux_rhs numbers them; lane q owns quadrature point q and, for q < n1e, the x edge q and the
// y edge q of the element.  Byte model of the element pass with all three terms: a unit reads a, g and the dz of its (at most) two
// interfaces once through the 1-form maps (4 * 2 n1e doubles), th and the two v as contiguous 2-form blocks (3 n2e), q at the points
// (mp12), J, det, thickInv once (6 mp12) and writes 2 n1e doubles: at p = 3  4*24 + 3*9 + 16 + 96 = 235 doubles read, 24 written = 2 072
// bytes; at p = 4  4*40 + 3*16 + 25 + 150 = 383 read, 40 written = 3 384 bytes.  The gather reads the 2 n1e again and writes (with ACCUM:
// reads and writes) the n1 slots of the level.  The nine composed launches move the metric three times and the 1-form result five times.
namespace {

struct MomForcingArgs {
    int nEl, nk, vert;
    const int *i0, *i1x, *i1y, *i2;
    const double *J, *det, *tI, *E, *w;
    const double *q, *a, *th, *g, *dz, *v;
    long long n0, n1, n2;                                   // packed rows: the row strides are the context's vector lengths
    double scale;
    double* ye; long long yes;
};

template <int N>
__global__ __launch_bounds__(256) void k_horiz_momentum_forcing(MomForcingArgs a) {
    using D = Dims<N>;
    constexpr int LPE = D::LPE, EPB = D::EPB;
    __shared__ double sE[D::mp1*N];
    __shared__ double s_a[EPB][2*LPE], s_g[EPB][2*LPE], s_z[2][EPB][2*LPE];
    __shared__ double s_h[EPB][LPE], s_w[2][EPB][LPE], s_x[EPB][LPE], s_y[EPB][LPE];
    const int tid = threadIdx.x, el = tid/LPE, q = tid%LPE;
    const int qx = q%D::mp1, qy = q/D::mp1;
    if (tid < D::mp1*N) sE[tid] = a.E[tid];
    const long long total = (long long)a.nEl*a.nk;
    const long long eg = (long long)blockIdx.x*EPB + el;
    const bool act = eg < total;
    const int lev = act ? (int)(eg/a.nEl) : 0, e = act ? (int)(eg%a.nEl) : 0;
    const bool rot = a.q != nullptr, pgf = a.th != nullptr, vor = a.dz != nullptr;          // (uniform: kernel arguments)
    const bool lo = vor && lev > 0, hi = vor && lev < a.nk - 1;                             // the interfaces lev-1 and lev of this level
    if (act) {
        if (q < D::n1e) {
            const int ix = a.i1x[e*D::n1e + q], iy = a.i1y[e*D::n1e + q];
            if (rot) { const double* r = a.a + (size_t)lev*a.n1; s_a[el][q] = r[ix]; s_a[el][D::n1e + q] = r[iy]; }
            if (pgf) { const double* r = a.g + (size_t)lev*a.n1; s_g[el][q] = r[ix]; s_g[el][D::n1e + q] = r[iy]; }
            if (lo) { const double* r = a.dz + (size_t)(lev - 1)*a.n1; s_z[0][el][q] = r[ix]; s_z[0][el][D::n1e + q] = r[iy]; }
            if (hi) { const double* r = a.dz + (size_t)lev*a.n1; s_z[1][el][q] = r[ix]; s_z[1][el][D::n1e + q] = r[iy]; }
        }
        if (q < D::n2e && (pgf || vor)) {
            const size_t slot = a.i2 ? (size_t)a.i2[e*D::n2e + q] : (size_t)e*D::n2e + q;
            if (pgf) s_h[el][q] = a.th[(size_t)lev*a.n2 + slot];
            if (lo) s_w[0][el][q] = a.v[(size_t)(lev - 1)*a.n2 + slot];
            if (hi) s_w[1][el][q] = a.v[(size_t)lev*a.n2 + slot];
        }
    }
    __syncthreads();                     // sE; the unit's rows (an element's lanes share a wave, but sE is the block's)
    if (act && q < D::mp12) {
        const size_t gq = (size_t)e*D::mp12 + q;
        const double* Je = a.J + (size_t)e*4*D::mp12;
        const double J00 = Je[0*D::mp12 + q], J01 = Je[1*D::mp12 + q], J10 = Je[2*D::mp12 + q], J11 = Je[3*D::mp12 + q];
        const double det = a.det[gq], tI = a.tI[(size_t)lev*((size_t)a.nEl*D::mp12) + gq];
        const double Q = a.w[qx]*a.w[qy];
        const double sd = 1.0/det, m = (a.scale*Q)*sd;
        double U = 0.0, V = 0.0;                                                   // the part that goes through G = J^T J
        double cx = 0.0, cy = 0.0;
        double u, v, h, dmy;
        if (pgf) {
            interp_point<N, S1>(s_g[el], sE, q, qx, qy, u, v);
            interp_point<N, S2>(s_h[el], sE, q, qx, qy, h, dmy);
            double f = (h*sd)*(m*tI);                                              // interp2_g; Uhmat's own thickness factor
            if (a.vert) f *= tI;
            U = f*u; V = f*v;
        }
        if (lo) {
            interp_point<N, S1>(s_z[0][el], sE, q, qx, qy, u, v);
            interp_point<N, S2>(s_w[0][el], sE, q, qx, qy, h, dmy);
            const double s = (0.5*h)*(m*sd);
            U += s*u; V += s*v;
        }
        if (hi) {
            interp_point<N, S1>(s_z[1][el], sE, q, qx, qy, u, v);
            interp_point<N, S2>(s_w[1][el], sE, q, qx, qy, h, dmy);
            const double s = (0.5*h)*(m*sd);
            U += s*u; V += s*v;
        }
        if (pgf || vor) {
            const double Gaa = J00*J00 + J10*J10, Gab = J00*J01 + J10*J11, Gbb = J01*J01 + J11*J11;
            cx = Gaa*U + Gab*V;
            cy = Gab*U + Gbb*V;
        }
        if (rot) {
            interp_point<N, S1>(s_a[el], sE, q, qx, qy, u, v);
            const double vort = a.q[(size_t)lev*a.n0 + a.i0[e*D::n0e + q]];       // interp0 at a collocated node (n0e == mp12)
            const double r = (vort*(J00*J11 - J01*J10))*(m*tI*tI);
            cx -= r*v;
            cy += r*u;
        }
        s_x[el][q] = cx;
        s_y[el][q] = cy;
    }
    wave_lds_sync();
    if (act && q < D::n1e) {
        const int ixx = q%D::np1, iyx = q/D::np1;     // x-normal edge: node in x, edge fn in y
        const int ixy = q%N,      iyy = q/N;          // y-normal edge: edge fn in x, node in y
        double yx = 0.0, yy = 0.0;
#pragma unroll
        for (int k = 0; k < D::mp1; k++) {
            yx += sE[k*N + iyx]*s_x[el][k*D::mp1 + ixx];
            yy += sE[k*N + ixy]*s_y[el][iyy*D::mp1 + k];
        }
        double* o = a.ye + (size_t)lev*a.yes + (size_t)e*2*D::n1e;                // (lev, e) < (nk, nEl): inside the nk * yes doubles ensured
        o[q] = yx; o[D::n1e + q] = yy;
    }
}

template <int N>
int horiz_momentum_forcing_n(mimsem_ctx* c, const MomForcingArgs& a) {
    constexpr int EPB = Dims<N>::EPB;
    const long long total = (long long)a.nEl*a.nk;
    hipLaunchKernelGGL((k_horiz_momentum_forcing<N>), dim3((unsigned)((total + EPB - 1)/EPB)), dim3(256), 0, c->stream, a);
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

}  // namespace

extern "C" int mimsem_horiz_momentum_forcing(mimsem_ctx* c, int nk, unsigned flags, double scale, const double* q, const double* a,
                                             const double* th, const double* g, const double* dz, const double* v, double* out) {
    if (!c || !out) return MIMSEM_ERR_ARG;
    if (nk < 1 || nk > c->nk || (flags & ~(MIMSEM_FLAG_VERT | MIMSEM_FLAG_ACCUM))) return MIMSEM_ERR_ARG;
    if (!q != !a || !th != !g || !dz != !v) return MIMSEM_ERR_ARG;                // a pair is given or absent as a whole
    if (nk == 1 && dz) return MIMSEM_ERR_ARG;                                      // one level has no interface
    if (out == q || out == a || out == th || out == g || out == dz || out == v) return MIMSEM_ERR_ARG;
    if (c->es.n < 1 || c->es.n > 7) return MIMSEM_ERR_UNSUPPORTED;
    if (!c->d_J || !c->d_det || !c->d_tI || !c->d_E || !c->d_w || !c->d_i0 || !c->d_i1x || !c->d_i1y || !c->d_g1) return MIMSEM_ERR_STATE;
    if (c->nEl == 0) return MIMSEM_OK;
    const int accum = (flags & MIMSEM_FLAG_ACCUM) ? 1 : 0;
    if (!q && !th && !dz) {                                                        // nothing to add: out = 0 unless it accumulates
        if (!accum) MIMSEM_HIP_TRY(hipMemsetAsync(out, 0, sizeof(double)*(size_t)nk*(size_t)c->n1, c->stream));
        return MIMSEM_OK;
    }
    const long long per = (long long)c->nEl*2*c->es.n1e;
    int rc = c->ensure_ye(per*nk);                                       // (grows outside a capture only: MIMSEM_ERR_STATE inside one)
    if (rc) return rc;
    MomForcingArgs p{};
    p.nEl = c->nEl; p.nk = nk; p.vert = (flags & MIMSEM_FLAG_VERT) ? 1 : 0;
    p.i0 = c->d_i0; p.i1x = c->d_i1x; p.i1y = c->d_i1y; p.i2 = c->d_i2;
    p.J = c->d_J; p.det = c->d_det; p.tI = c->d_tI; p.E = c->d_E; p.w = c->d_w;
    p.q = q; p.a = a; p.th = th; p.g = g; p.dz = dz; p.v = v;
    p.n0 = c->n0; p.n1 = c->n1; p.n2 = c->n2;
    p.scale = scale; p.ye = c->d_ye; p.yes = per;
    switch (c->es.n) {
    case 1: rc = horiz_momentum_forcing_n<1>(c, p); break;
    case 2: rc = horiz_momentum_forcing_n<2>(c, p); break;
    case 3: rc = horiz_momentum_forcing_n<3>(c, p); break;
    case 4: rc = horiz_momentum_forcing_n<4>(c, p); break;
    case 5: rc = horiz_momentum_forcing_n<5>(c, p); break;
    case 6: rc = horiz_momentum_forcing_n<6>(c, p); break;
    default: rc = horiz_momentum_forcing_n<7>(c, p); break;
    }
    if (rc) return rc;
    return launch_gather_sum(c, 1, nk, c->d_ye, per, accum, out, c->n1);
}
