// flux_rhs.inc -- mimsem_horiz_flux_rhs (include/mimsem_hip.h): the mass-flux right-hand side of HorizSolve::diagnose_fluxes
// (eul/HorizSolve.cpp:298-306) and HorizSolve::momentum_rhs (:538-547) for EVERY level in one element pass plus the 1-form gather.
// Included at the end of elem_kernels.hip after bernoulli.inc, whose lane-per-quadrature-point layout (Dims), LDS-staged edge table and
// interp_point it shares.
//
// The reference sums four Uvec::assemble_hu(k, scale, u_a, h_b, false, c_ab) calls (eul/Assembly.cpp:2198-2279), c_11 = c_22 = 1/3,
// c_12 = c_21 = 1/6, into the local vector and scatters it with ADD_VALUES.  Every call is Ut^T / Vt^T diag(c) with the same test basis, so
// the four coefficients are summed at the quadrature point before ONE projection.  With t = thickInv[k][q], d = det[e][q], J the Jacobian,
// Q = w_qx w_qy, (u_a, v_a) the LOCAL interpolants of u_a (interp1_l, before the Piola map) and r_b the interpolant of h_b over d (interp2_g):
//   m        = scale Q t^2 / d           Gaa = J00^2 + J10^2, Gab = J00 J01 + J10 J11, Gbb = J01^2 + J11^2
//   (U, V)   = r1 (u1/3 + u2/6, v1/3 + v2/6) + r2 (u1/6 + u2/3, v1/6 + v2/3)
//   c_x(q)   = m (Gaa U + Gab V)         c_y(q) = m (Gab U + Gbb V)
//   ye_x[e,j] = sum_q Ut[j][q] c_x(q)    ye_y[e,j] = sum_q Vt[j][q] c_y(q)
// Ut[j][q] is l_jx(x_qx) e_jy(y_qy) with collocated nodes, so each sum has mp1 terms.  The element-local results [nk][nEl][2 n1e] go to the
// context's element workspace; launch_gather_sum(c, 1, ..) adds the (at most two) contributions of every edge slot in the plan's order.
// Two launches, no atomics, a fixed summation order: two calls give the same bits.
//
// Work item = (level, element) as k_horiz_bernoulli numbers them; lane q owns quadrature point q and, for q < n1e, the x edge q and the
// y edge q of the element.  Byte model of the element pass: a unit reads u1, u2 once through the 1-form maps (2 * 2 n1e doubles), h1, h2
// as contiguous 2-form blocks (2 n2e), J, det, thickInv once (6 mp12) and writes 2 n1e doubles: at p = 3  2*24 + 2*9 + 6*16 = 162 doubles
// read, 24 written = 1 488 bytes.  The gather reads those 24 again and writes the n1 slots of the level.
namespace {

struct FluxRhsArgs {
    int nEl, nk;
    const int *i1x, *i1y, *i2;
    const double *J, *det, *tI, *E, *w;
    const double *u1, *u2; long long us;
    const double *h1, *h2; long long hs;
    double scale;
    double* ye; long long yes;
};

template <int N>
__global__ __launch_bounds__(256) void k_horiz_flux_rhs(FluxRhsArgs a) {
    using D = Dims<N>;
    constexpr int LPE = D::LPE, EPB = D::EPB;
    __shared__ double sE[D::mp1*N];
    __shared__ double s_u1[EPB][2*LPE], s_u2[EPB][2*LPE];
    __shared__ double s_h1[EPB][LPE], s_h2[EPB][LPE], s_a[EPB][LPE], s_b[EPB][LPE];
    const int tid = threadIdx.x, el = tid/LPE, q = tid%LPE;
    const int qx = q%D::mp1, qy = q/D::mp1;
    if (tid < D::mp1*N) sE[tid] = a.E[tid];
    const long long total = (long long)a.nEl*a.nk;
    const long long eg = (long long)blockIdx.x*EPB + el;
    const bool act = eg < total;
    const int lev = act ? (int)(eg/a.nEl) : 0, e = act ? (int)(eg%a.nEl) : 0;
    if (act) {
        if (q < D::n1e) {
            const int ix = a.i1x[e*D::n1e + q], iy = a.i1y[e*D::n1e + q];
            const double* r1 = a.u1 + (size_t)lev*a.us; const double* r2 = a.u2 + (size_t)lev*a.us;
            s_u1[el][q] = r1[ix]; s_u1[el][D::n1e + q] = r1[iy];
            s_u2[el][q] = r2[ix]; s_u2[el][D::n1e + q] = r2[iy];
        }
        if (q < D::n2e) {
            const size_t slot = a.i2 ? (size_t)a.i2[e*D::n2e + q] : (size_t)e*D::n2e + q;
            s_h1[el][q] = a.h1[(size_t)lev*a.hs + slot]; s_h2[el][q] = a.h2[(size_t)lev*a.hs + slot];
        }
    }
    __syncthreads();                     // sE; the unit's rows (an element's lanes share a wave, but sE is the block's)
    if (act && q < D::mp12) {
        const size_t gq = (size_t)e*D::mp12 + q;
        const double* Je = a.J + (size_t)e*4*D::mp12;
        const double J00 = Je[0*D::mp12 + q], J01 = Je[1*D::mp12 + q], J10 = Je[2*D::mp12 + q], J11 = Je[3*D::mp12 + q];
        const double det = a.det[gq], tI = a.tI[(size_t)lev*((size_t)a.nEl*D::mp12) + gq];
        const double Q = a.w[qx]*a.w[qy];
        double u1, v1, u2, v2, r1, r2, dmy;
        interp_point<N, S1>(s_u1[el], sE, q, qx, qy, u1, v1);
        interp_point<N, S1>(s_u2[el], sE, q, qx, qy, u2, v2);
        interp_point<N, S2>(s_h1[el], sE, q, qx, qy, r1, dmy);
        interp_point<N, S2>(s_h2[el], sE, q, qx, qy, r2, dmy);
        const double sd = 1.0/det;
        r1 *= sd; r2 *= sd;                                                      // interp2_g
        const double U = r1*(u1*(1.0/3.0) + u2*(1.0/6.0)) + r2*(u1*(1.0/6.0) + u2*(1.0/3.0));
        const double V = r1*(v1*(1.0/3.0) + v2*(1.0/6.0)) + r2*(v1*(1.0/6.0) + v2*(1.0/3.0));
        const double m = (a.scale*Q)*(tI*tI)*sd;
        const double Gaa = J00*J00 + J10*J10, Gab = J00*J01 + J10*J11, Gbb = J01*J01 + J11*J11;
        s_a[el][q] = m*(Gaa*U + Gab*V);
        s_b[el][q] = m*(Gab*U + Gbb*V);
    }
    wave_lds_sync();
    if (act && q < D::n1e) {
        const int ixx = q%D::np1, iyx = q/D::np1;     // x-normal edge: node in x, edge fn in y
        const int ixy = q%N,      iyy = q/N;          // y-normal edge: edge fn in x, node in y
        double yx = 0.0, yy = 0.0;
#pragma unroll
        for (int k = 0; k < D::mp1; k++) {
            yx += sE[k*N + iyx]*s_a[el][k*D::mp1 + ixx];
            yy += sE[k*N + ixy]*s_b[el][iyy*D::mp1 + k];
        }
        double* o = a.ye + (size_t)lev*a.yes + (size_t)e*2*D::n1e;                // (lev, e) < (nk, nEl): inside the nk * yes doubles ensured
        o[q] = yx; o[D::n1e + q] = yy;
    }
}

template <int N>
int horiz_flux_rhs_n(mimsem_ctx* c, const FluxRhsArgs& a) {
    constexpr int EPB = Dims<N>::EPB;
    const long long total = (long long)a.nEl*a.nk;
    hipLaunchKernelGGL((k_horiz_flux_rhs<N>), dim3((unsigned)((total + EPB - 1)/EPB)), dim3(256), 0, c->stream, a);
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

}  // namespace

extern "C" int mimsem_horiz_flux_rhs(mimsem_ctx* c, int nk, const double* u1, const double* u2, long long ldu,
                                     const double* h1, const double* h2, long long ldh, double scale, double* out, long long ldo) {
    if (!c || !u1 || !u2 || !h1 || !h2 || !out) return MIMSEM_ERR_ARG;
    if (nk < 1 || nk > c->nk || ldu < 0 || ldh < 0 || ldo < 0) return MIMSEM_ERR_ARG;
    if (out == u1 || out == u2 || out == h1 || out == h2) return MIMSEM_ERR_ARG;
    if (c->es.n < 1 || c->es.n > 7) return MIMSEM_ERR_UNSUPPORTED;
    if (!c->d_J || !c->d_det || !c->d_tI || !c->d_E || !c->d_w || !c->d_i1x || !c->d_i1y || !c->d_g1) return MIMSEM_ERR_STATE;
    if (c->nEl == 0) return MIMSEM_OK;
    const long long per = (long long)c->nEl*2*c->es.n1e;
    int rc = c->ensure_ye(per*nk);                                       // (grows outside a capture only: MIMSEM_ERR_STATE inside one)
    if (rc) return rc;
    FluxRhsArgs a{};
    a.nEl = c->nEl; a.nk = nk;
    a.i1x = c->d_i1x; a.i1y = c->d_i1y; a.i2 = c->d_i2;
    a.J = c->d_J; a.det = c->d_det; a.tI = c->d_tI; a.E = c->d_E; a.w = c->d_w;
    a.u1 = u1; a.u2 = u2; a.us = ldu; a.h1 = h1; a.h2 = h2; a.hs = ldh;
    a.scale = scale; a.ye = c->d_ye; a.yes = per;
    switch (c->es.n) {
    case 1: rc = horiz_flux_rhs_n<1>(c, a); break;
    case 2: rc = horiz_flux_rhs_n<2>(c, a); break;
    case 3: rc = horiz_flux_rhs_n<3>(c, a); break;
    case 4: rc = horiz_flux_rhs_n<4>(c, a); break;
    case 5: rc = horiz_flux_rhs_n<5>(c, a); break;
    case 6: rc = horiz_flux_rhs_n<6>(c, a); break;
    default: rc = horiz_flux_rhs_n<7>(c, a); break;
    }
    if (rc) return rc;
    return launch_gather_sum(c, 1, nk, c->d_ye, per, 0, out, ldo);
}
