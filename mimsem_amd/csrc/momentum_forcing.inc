// momentum_forcing.inc -- mimsem_horiz_momentum_forcing (include/mimsem_hip.h): the element-local forcing of HorizSolve::momentum_rhs
// (eul/HorizSolve.cpp:496-635, box/HorizSolve.cpp:412-526) for EVERY level in one element pass plus the 1-form gather.  A fused
// element pass on the unit layer of elem_unit.hpp.
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
// and its integrand; the loads of the interfaces -1 and nk-1 sit inside their branch as well.
//
// Work item = (level, element) as k_horiz_flux_rhs numbers them; lane q owns quadrature point q and, for q < n1e, the x edge q and the
// y edge q of the element.  Byte model of the element pass with all three terms: a unit reads a, g and the dz of its (at most) two
// interfaces once through the 1-form maps (4 * 2 n1e doubles), th and the two v as contiguous 2-form blocks (3 n2e), q at the points
// (mp12), J, det, thickInv once (6 mp12) and writes 2 n1e doubles: at p = 3  4*24 + 3*9 + 16 + 96 = 235 doubles read, 24 written = 2 072
// bytes; at p = 4  4*40 + 3*16 + 25 + 150 = 383 read, 40 written = 3 384 bytes.  The gather reads the 2 n1e again and writes (with ACCUM:
// reads and writes) the n1 slots of the level.  The nine composed launches move the metric three times and the 1-form result five times.
namespace {

struct MomForcingArgs {
    ElemTables t;
    int nk, vert;
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
    const Lane ln = lane_of_thread<N>();
    const int el = ln.el, q = ln.q, qx = ln.qx, qy = ln.qy;
    stage_edge_table<N>(sE, a.t.E);
    const Unit un = unit_of((long long)blockIdx.x*EPB + el, a.t.nEl, a.nk);
    const bool act = un.act;
    const int lev = un.lev, e = un.e;
    const bool rot = a.q != nullptr, pgf = a.th != nullptr, vor = a.dz != nullptr;          // (uniform: kernel arguments)
    const bool lo = vor && lev > 0, hi = vor && lev < a.nk - 1;                             // the interfaces lev-1 and lev of this level
    if (act) {
        if (q < D::n1e) {
            const int2 s1 = form1_slots<N>(a.t, e, q);
            if (rot) stage_form1<N>(s1, q, a.a + (size_t)lev*a.n1, s_a[el]);
            if (pgf) stage_form1<N>(s1, q, a.g + (size_t)lev*a.n1, s_g[el]);
            if (lo) stage_form1<N>(s1, q, a.dz + (size_t)(lev - 1)*a.n1, s_z[0][el]);
            if (hi) stage_form1<N>(s1, q, a.dz + (size_t)lev*a.n1, s_z[1][el]);
        }
        if (q < D::n2e && (pgf || vor)) {
            const size_t slot = form2_slot<N>(a.t.i2, e, q);
            if (pgf) s_h[el][q] = a.th[(size_t)lev*a.n2 + slot];
            if (lo) s_w[0][el][q] = a.v[(size_t)(lev - 1)*a.n2 + slot];
            if (hi) s_w[1][el][q] = a.v[(size_t)lev*a.n2 + slot];
        }
    }
    __syncthreads();                     // sE; the unit's rows
    if (act && q < D::mp12) {
        const PointMetric p = point_metric<N>(a.t, lev, e, q);
        const double tI = p.tI;
        const double sd = 1.0/p.det, m = (a.scale*p.Q)*sd;
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
            const double Gaa = p.J00*p.J00 + p.J10*p.J10, Gab = p.J00*p.J01 + p.J10*p.J11, Gbb = p.J01*p.J01 + p.J11*p.J11;
            cx = Gaa*U + Gab*V;
            cy = Gab*U + Gbb*V;
        }
        if (rot) {
            interp_point<N, S1>(s_a[el], sE, q, qx, qy, u, v);
            const double vort = a.q[(size_t)lev*a.n0 + a.t.i0[e*D::n0e + q]];     // interp0 at a collocated node (n0e == mp12)
            const double r = (vort*(p.J00*p.J11 - p.J01*p.J10))*(m*tI*tI);
            cx -= r*v;
            cy += r*u;
        }
        s_x[el][q] = cx;
        s_y[el][q] = cy;
    }
    wave_lds_sync();
    if (act && q < D::n1e) {
        double yx, yy;
        project1<N>(sE, s_x[el], s_y[el], q, yx, yy);
        double* o = a.ye + (size_t)lev*a.yes + (size_t)e*2*D::n1e;                // inside the nk * yes doubles ensured
        o[q] = yx; o[D::n1e + q] = yy;
    }
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
    MomForcingArgs p{};
    if (int rc = elem_tables(c, NEED_I0 | NEED_G1, p.t)) return rc;
    if (c->nEl == 0) return MIMSEM_OK;
    const int accum = (flags & MIMSEM_FLAG_ACCUM) ? 1 : 0;
    if (!q && !th && !dz) {                                                        // nothing to add: out = 0 unless it accumulates
        if (!accum) MIMSEM_HIP_TRY(hipMemsetAsync(out, 0, sizeof(double)*(size_t)nk*(size_t)c->n1, c->stream));
        return MIMSEM_OK;
    }
    const long long per = (long long)c->nEl*2*c->es.n1e;
    int rc = c->ensure_ye(per*nk);                                       // (grows outside a capture only: MIMSEM_ERR_STATE inside one)
    if (rc) return rc;
    p.nk = nk; p.vert = (flags & MIMSEM_FLAG_VERT) ? 1 : 0;
    p.q = q; p.a = a; p.th = th; p.g = g; p.dz = dz; p.v = v;
    p.n0 = c->n0; p.n1 = c->n1; p.n2 = c->n2;
    p.scale = scale; p.ye = c->d_ye; p.yes = per;
    rc = for_order<1, 7>(c->es.n, [&](auto n) { return launch_units<decltype(n)::value>(c, k_horiz_momentum_forcing<decltype(n)::value>, (long long)p.t.nEl*p.nk, p); });
    if (rc) return rc;
    return launch_gather_sum(c, 1, nk, c->d_ye, per, accum, out, c->n1);
}
