// flux_rhs.inc -- mimsem_horiz_flux_rhs (include/mimsem_hip.h): the mass-flux right-hand side of HorizSolve::diagnose_fluxes
// (eul/HorizSolve.cpp:298-306) and HorizSolve::momentum_rhs (:538-547) for EVERY level in one element pass plus the 1-form gather.
// A fused element pass on the unit layer of elem_unit.hpp.
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
    ElemTables t;
    int nk;
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
    const Lane ln = lane_of_thread<N>();
    const int el = ln.el, q = ln.q, qx = ln.qx, qy = ln.qy;
    stage_edge_table<N>(sE, a.t.E);
    const Unit un = unit_of((long long)blockIdx.x*EPB + el, a.t.nEl, a.nk);
    const bool act = un.act;
    const int lev = un.lev, e = un.e;
    if (act) {
        if (q < D::n1e) {
            const int2 s1 = form1_slots<N>(a.t, e, q);
            stage_form1<N>(s1, q, a.u1 + (size_t)lev*a.us, s_u1[el]);
            stage_form1<N>(s1, q, a.u2 + (size_t)lev*a.us, s_u2[el]);
        }
        if (q < D::n2e) {
            const size_t slot = form2_slot<N>(a.t.i2, e, q);
            s_h1[el][q] = a.h1[(size_t)lev*a.hs + slot]; s_h2[el][q] = a.h2[(size_t)lev*a.hs + slot];
        }
    }
    __syncthreads();                     // sE; the unit's rows
    if (act && q < D::mp12) {
        const PointMetric g = point_metric<N>(a.t, lev, e, q);
        double u1, v1, u2, v2, r1, r2, dmy;
        interp_point<N, S1>(s_u1[el], sE, q, qx, qy, u1, v1);
        interp_point<N, S1>(s_u2[el], sE, q, qx, qy, u2, v2);
        interp_point<N, S2>(s_h1[el], sE, q, qx, qy, r1, dmy);
        interp_point<N, S2>(s_h2[el], sE, q, qx, qy, r2, dmy);
        const double sd = 1.0/g.det;
        r1 *= sd; r2 *= sd;                                                      // interp2_g
        const double U = r1*(u1*(1.0/3.0) + u2*(1.0/6.0)) + r2*(u1*(1.0/6.0) + u2*(1.0/3.0));
        const double V = r1*(v1*(1.0/3.0) + v2*(1.0/6.0)) + r2*(v1*(1.0/6.0) + v2*(1.0/3.0));
        const double m = (a.scale*g.Q)*(g.tI*g.tI)*sd;
        const double Gaa = g.J00*g.J00 + g.J10*g.J10, Gab = g.J00*g.J01 + g.J10*g.J11, Gbb = g.J01*g.J01 + g.J11*g.J11;
        s_a[el][q] = m*(Gaa*U + Gab*V);
        s_b[el][q] = m*(Gab*U + Gbb*V);
    }
    wave_lds_sync();
    if (act && q < D::n1e) {
        double yx, yy;
        project1<N>(sE, s_a[el], s_b[el], q, yx, yy);
        double* o = a.ye + (size_t)lev*a.yes + (size_t)e*2*D::n1e;                // inside the nk * yes doubles ensured
        o[q] = yx; o[D::n1e + q] = yy;
    }
}

}  // namespace

extern "C" int mimsem_horiz_flux_rhs(mimsem_ctx* c, int nk, const double* u1, const double* u2, long long ldu,
                                     const double* h1, const double* h2, long long ldh, double scale, double* out, long long ldo) {
    if (!c || !u1 || !u2 || !h1 || !h2 || !out) return MIMSEM_ERR_ARG;
    if (nk < 1 || nk > c->nk || ldu < 0 || ldh < 0 || ldo < 0) return MIMSEM_ERR_ARG;
    if (out == u1 || out == u2 || out == h1 || out == h2) return MIMSEM_ERR_ARG;
    if (c->es.n < 1 || c->es.n > 7) return MIMSEM_ERR_UNSUPPORTED;
    FluxRhsArgs a{};
    if (int rc = elem_tables(c, NEED_G1, a.t)) return rc;
    if (c->nEl == 0) return MIMSEM_OK;
    const long long per = (long long)c->nEl*2*c->es.n1e;
    int rc = c->ensure_ye(per*nk);                                       // (grows outside a capture only: MIMSEM_ERR_STATE inside one)
    if (rc) return rc;
    a.nk = nk;
    a.u1 = u1; a.u2 = u2; a.us = ldu; a.h1 = h1; a.h2 = h2; a.hs = ldh;
    a.scale = scale; a.ye = c->d_ye; a.yes = per;
    rc = for_order<1, 7>(c->es.n, [&](auto n) { return launch_units<decltype(n)::value>(c, k_horiz_flux_rhs<decltype(n)::value>, (long long)a.t.nEl*a.nk, a); });
    if (rc) return rc;
    return launch_gather_sum(c, 1, nk, c->d_ye, per, 0, out, ldo);
}
