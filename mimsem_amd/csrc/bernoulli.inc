// bernoulli.inc -- mimsem_horiz_bernoulli (include/mimsem_hip.h): HorizSolve::diagnose_Phi (eul/HorizSolve.cpp:419-470), the horizontal
// Bernoulli function of momentum_rhs_ec, for EVERY level in ONE launch.  Dims, interp_point and wave_lds_sync come from elem_unit.hpp; the
// rest of the frame is spelled out here: on that header's unit layer the call measured 0.5 % slower (profiles/elem_unit_layer.txt 4).
//
// The reference forms Phi_k from three K (WtQUmat) and three M2h (Whmat, no vertical scaling) products:
//   Phi_k = 1/3 (K(u1) u1 + K(u1) u2 + K(u2) u2) + 1/6 (M2h(z1) z1 + M2h(z1) z2 + M2h(z2) z2)
//   z_a   = 1/2 velz_a[k-1] (k > 0) + 1/2 velz_a[k] (k < nk-1)                                           (:451-459)
// Every product is W^T diag(c) B with the same 2-form test basis W, so the six coefficients are summed at the quadrature point before
// ONE W^T step.  With t = thickInv[k][q], d = det[e][q], J the Jacobian, Q = w_qx w_qy, (u_a, v_a) the local interpolants of velx_a,
// U_a = J (u_a, v_a)^T / d and s_a the local interpolant of z_a (WtQUmat::assemble eul/Assembly.cpp:951-966, Whmat::assemble :1268-1281):
//   c_q        = SCALE Q [ t^2/6 (U1.U1 + U1.U2 + U2.U2) + t/(6 d^2) (s1^2 + s1 s2 + s2^2) ]
//   Phi_k[e,j] = sum_q W[q][j] c_q
// A 2-form is discontinuous: the result is element-local, nothing is scattered, no atomics, no workspace; the sum over q runs in a fixed
// order, so two calls give the same bits.
//
// Work item = (level, element) as k_energetics_horiz numbers them; lane q owns quadrature point q and, for q < n2e, DoF q.  A unit reads
// velx1, velx2 once through the 1-form maps (2 * 2 n1e doubles), the up to four velz rows as contiguous 2-form blocks (4 n2e; averaged in
// the DoFs before interpolating, the missing boundary interface is not read), J, det, thickInv once (6 mp12), and writes n2e doubles: at
// p = 3  2*24 + 4*9 + 96 = 180 doubles read, 9 written = 1 512 bytes.
namespace {

struct BernoulliArgs {
    int nEl, nk;
    const int *i1x, *i1y, *i2;
    const double *J, *det, *tI, *E, *w;
    const double *u1, *u2; long long us;
    const double *z1, *z2; long long zs;
    double scale;
    double* out; long long os;
};

template <int N>
__global__ __launch_bounds__(256) void k_horiz_bernoulli(BernoulliArgs a) {
    using D = Dims<N>;
    constexpr int LPE = D::LPE, EPB = D::EPB;
    __shared__ double sE[D::mp1*N];
    __shared__ double s_u1[EPB][2*LPE], s_u2[EPB][2*LPE];
    __shared__ double s_z1[EPB][LPE], s_z2[EPB][LPE], s_c[EPB][LPE];
    const int tid = threadIdx.x, el = tid/LPE, q = tid%LPE;
    const int qx = q%D::mp1, qy = q/D::mp1;
    if (tid < D::mp1*N) sE[tid] = a.E[tid];
    const long long total = (long long)a.nEl*a.nk;
    const long long eg = (long long)blockIdx.x*EPB + el;
    const bool act = eg < total;
    const int lev = act ? (int)(eg/a.nEl) : 0, e = act ? (int)(eg%a.nEl) : 0;
    size_t slot = 0;
    if (act) {
        if (q < D::n1e) {
            const int ix = a.i1x[e*D::n1e + q], iy = a.i1y[e*D::n1e + q];
            const double* r1 = a.u1 + (size_t)lev*a.us; const double* r2 = a.u2 + (size_t)lev*a.us;
            s_u1[el][q] = r1[ix]; s_u1[el][D::n1e + q] = r1[iy];
            s_u2[el][q] = r2[ix]; s_u2[el][D::n1e + q] = r2[iy];
        }
        if (q < D::n2e) {
            slot = a.i2 ? (size_t)a.i2[e*D::n2e + q] : (size_t)e*D::n2e + q;
            double z1 = 0.0, z2 = 0.0;                                // (:451-459: the boundary levels have one interface only)
            if (lev > 0) { z1 += 0.5*a.z1[(size_t)(lev - 1)*a.zs + slot]; z2 += 0.5*a.z2[(size_t)(lev - 1)*a.zs + slot]; }
            if (lev < a.nk - 1) { z1 += 0.5*a.z1[(size_t)lev*a.zs + slot]; z2 += 0.5*a.z2[(size_t)lev*a.zs + slot]; }
            s_z1[el][q] = z1; s_z2[el][q] = z2;
        }
    }
    __syncthreads();                     // sE; the unit's rows (an element's lanes share a wave, but sE is the block's)
    if (act && q < D::mp12) {
        const size_t gq = (size_t)e*D::mp12 + q;
        const double* Je = a.J + (size_t)e*4*D::mp12;
        const double J00 = Je[0*D::mp12 + q], J01 = Je[1*D::mp12 + q], J10 = Je[2*D::mp12 + q], J11 = Je[3*D::mp12 + q];
        const double det = a.det[gq], tI = a.tI[(size_t)lev*((size_t)a.nEl*D::mp12) + gq];
        const double Q = a.w[qx]*a.w[qy];
        double u1, v1, u2, v2, s1, s2, dmy;
        interp_point<N, S1>(s_u1[el], sE, q, qx, qy, u1, v1);
        interp_point<N, S1>(s_u2[el], sE, q, qx, qy, u2, v2);
        interp_point<N, S2>(s_z1[el], sE, q, qx, qy, s1, dmy);
        interp_point<N, S2>(s_z2[el], sE, q, qx, qy, s2, dmy);
        const double sd = 1.0/det;
        const double a1 = (J00*u1 + J01*v1)*sd, b1 = (J10*u1 + J11*v1)*sd;      // interp1_g (Piola)
        const double a2 = (J00*u2 + J01*v2)*sd, b2 = (J10*u2 + J11*v2)*sd;
        const double kin = (a1*a1 + b1*b1) + (a1*a2 + b1*b2) + (a2*a2 + b2*b2);
        const double ver = (s1*s1 + s1*s2 + s2*s2)*(sd*sd);
        s_c[el][q] = (a.scale*Q)*((tI*tI*(1.0/6.0))*kin + (tI*(1.0/6.0))*ver);
    }
    wave_lds_sync();
    if (act && q < D::n2e) {
        const int jx = q%N, jy = q/N;
        double y = 0.0;
#pragma unroll
        for (int py = 0; py < D::mp1; py++)
#pragma unroll
            for (int px = 0; px < D::mp1; px++) y += (sE[px*N + jx]*sE[py*N + jy])*s_c[el][py*D::mp1 + px];
        a.out[(size_t)lev*a.os + slot] = y;
    }
}

template <int N>
int horiz_bernoulli_n(mimsem_ctx* c, const BernoulliArgs& a) {
    constexpr int EPB = Dims<N>::EPB;
    const long long total = (long long)a.nEl*a.nk;
    hipLaunchKernelGGL((k_horiz_bernoulli<N>), dim3((unsigned)((total + EPB - 1)/EPB)), dim3(256), 0, c->stream, a);
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

}  // namespace

extern "C" int mimsem_horiz_bernoulli(mimsem_ctx* c, int nk, const double* velx1, const double* velx2, long long ldu,
                                      const double* velz1, const double* velz2, long long ldz, double scale, double* out, long long ldo) {
    if (!c || !velx1 || !velx2 || !velz1 || !velz2 || !out) return MIMSEM_ERR_ARG;
    if (nk < 2 || nk > c->nk || ldu < 0 || ldz < 0 || ldo < 0) return MIMSEM_ERR_ARG;
    if (!c->d_J || !c->d_det || !c->d_tI || !c->d_E || !c->d_w || !c->d_i1x || !c->d_i1y) return MIMSEM_ERR_STATE;
    BernoulliArgs a{};
    a.nEl = c->nEl; a.nk = nk;
    a.i1x = c->d_i1x; a.i1y = c->d_i1y; a.i2 = c->d_i2;
    a.J = c->d_J; a.det = c->d_det; a.tI = c->d_tI; a.E = c->d_E; a.w = c->d_w;
    a.u1 = velx1; a.u2 = velx2; a.us = ldu; a.z1 = velz1; a.z2 = velz2; a.zs = ldz;
    a.scale = scale; a.out = out; a.os = ldo;
    switch (c->es.n) {
    case 1: return horiz_bernoulli_n<1>(c, a);
    case 2: return horiz_bernoulli_n<2>(c, a);
    case 3: return horiz_bernoulli_n<3>(c, a);
    case 4: return horiz_bernoulli_n<4>(c, a);
    case 5: return horiz_bernoulli_n<5>(c, a);
    case 6: return horiz_bernoulli_n<6>(c, a);
    case 7: return horiz_bernoulli_n<7>(c, a);
    default: return MIMSEM_ERR_UNSUPPORTED;
    }
}
