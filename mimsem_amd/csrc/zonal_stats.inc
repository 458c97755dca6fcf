// zonal_stats.inc -- mimsem_zonal_plan_build / mimsem_euler_zonal_moments (include/mimsem_hip.h): the binned first and second moments of
// the physical fields of a 3-D state, level by level, in ONE launch that stays on the device -- what a Held-Suarez run (eul/HeldSuarez.cpp)
// is averaged into.  Of the unit layer of elem_unit.hpp it takes the tables, the metric and the dispatch: its work mapping is its own.
//
// Fields at the quadrature point q of element e on level k, those of Geom::write1 / write2(vert_scale = true) (eul/Geom.cpp:474-631) as
// Euler.quad_fields states them: with (ul, vl), rl, hl, pl the LOCAL interpolants of velx_k, rho_k, rt_k, exner_k (interp_point),
// J = [[J00, J01], [J10, J11]], d = det[e][q], t = thickInv[k][e][q]
//   u = ((J00 ul + J01 vl) / d) t     v = ((J10 ul + J11 vl) / d) t              interp1_g / thick
//   r = (rl / d) t     H = (hl / d) t     P = (pl / d) t                         interp2_g / thick
//   T = H P / (CP r)   (the Exner function carries CP: compute_k_T, eul/VertOps.cpp:1564);  r > 0 is required: T = NaN otherwise
// Weight a = Q_q d (the mass_q = d w of energetics.inc): every element adds its own share of a shared point.  Nine moments per
// (level, band): the sums of a {1, u, v, T, uu, vv, uv, vT, TT} over the band's points; acc [9][nlev][nb] += them.
//
// The plan (host, mimsem_zonal_plan_build): the caller's table band[nEl][mp12] in [-1, nb) is validated, the kept points e mp12 + q are
// sorted by (band, e, q) into one list with the offsets of the NON-EMPTY bands -- an empty band has no work item, nothing is loaded for it
// and its entries of acc are not touched (acc + 0.0).  The kernel reads no index the library has not checked.
//
// Work item = (non-empty band, level): a block of 256; lane l takes the points l, l + 256, .. of the band's list.  The sort puts the
// lanes of one element next to each other: they gather the same DoFs and the same index rows, from the same cache lines.  A lane reads,
// per point, N entries of each 1-form map and 2 N DoFs of velx, 3 N^2 DoFs of rho, rt, exner (through the 2-form map where the context has
// one), J (4), det, thickInv and evaluates with the basis rows of the LDS-staged edge table; every load sits inside the branch of a live
// list entry.  Requested bytes per point and level at p = 3: 6 + 27 + 6 doubles and 6 + 1 ints = 340 bytes; the compulsory bytes of a
// sample are every state array, J, det and thickInv once (DESIGN.md 8 has the model): an element's DoFs are re-read by its 16 lanes, from L1.
//
// Reduction, no atomics: a lane sums its points in list order, the 64 lanes of a wave by the shuffle tree (en_wave_sum), the four waves as
// (w0 + w1) + (w2 + w3); lanes 0 .. 8 then add the nine finished sums to acc -- the one writer of those nine entries in the launch.  Grid
// and order depend on (plan, nlev, order) only: base + sample is reproducible to the bit.  No workspace: capturable as it is.
namespace {

constexpr int ZN_MOM = 9;
constexpr double ZN_CP = 1004.5;         // eul/Euler_2.cpp:29

struct ZonalArgs {
    ElemTables t;
    int nlev, nb;
    const double *u, *rho, *rt, *ex;
    long long n1, n2;                    // packed rows: the row strides are the context's vector lengths
    const int *band, *off, *pt;          // plan: [nne] band of the work item, [nne + 1] offsets, [npts] e mp12 + q
    double* acc;                         // [9][nlev][nb]
};

template <int N>
__global__ __launch_bounds__(256) void k_zonal_moments(ZonalArgs a) {
    using D = Dims<N>;
    __shared__ double sE[D::mp1*N], sW[D::mp1];
    __shared__ double red[4][ZN_MOM];
    const int tid = threadIdx.x, lev = blockIdx.y;
    stage_edge_table<N>(sE, a.t.E);
    if (tid < D::mp1) sW[tid] = a.t.w[tid];
    const int beg = a.off[blockIdx.x], end = a.off[blockIdx.x + 1];              // (blockIdx.x < nne: inside the nne + 1 offsets)
    const double* uv = a.u + (size_t)lev*a.n1;
    const double* rho = a.rho + (size_t)lev*a.n2;
    const double* rt = a.rt + (size_t)lev*a.n2;
    const double* ex = a.ex + (size_t)lev*a.n2;
    double s[ZN_MOM];
#pragma unroll
    for (int m = 0; m < ZN_MOM; m++) s[m] = 0.0;
    __syncthreads();                     // sE, sW
    for (int i = beg + tid; i < end; i += 256) {                                 // the lane's points, in list order
        const int p = a.pt[i], e = p/D::mp12, q = p - e*D::mp12;                 // (validated by the plan: e < nEl)
        const int qx = q%D::mp1, qy = q/D::mp1;
        const int* ix = a.t.i1x + (size_t)e*D::n1e;
        const int* iy = a.t.i1y + (size_t)e*D::n1e;
        double ul = 0.0, vl = 0.0;       // interp_point<N, S1>, the DoFs straight from global memory
#pragma unroll
        for (int j = 0; j < N; j++) {
            ul += uv[ix[j*D::np1 + qx]]*sE[qy*N + j];
            vl += uv[iy[qy*N + j]]*sE[qx*N + j];
        }
        double rl = 0.0, hl = 0.0, pl = 0.0;                                      // interp_point<N, S2> of the three 2-forms
#pragma unroll
        for (int jy = 0; jy < N; jy++)
#pragma unroll
            for (int jx = 0; jx < N; jx++) {
                const size_t slot = form2_slot<N>(a.t.i2, e, jy*N + jx);
                const double w = sE[qx*N + jx]*sE[qy*N + jy];
                rl += rho[slot]*w; hl += rt[slot]*w; pl += ex[slot]*w;
            }
        const PointMetric g = point_metric<N>(a.t, lev, e, q);
        const double det = g.det, t = g.tI;                                       // (the weight comes from sW: g.Q is not used)
        const double u = ((g.J00*ul + g.J01*vl)/det)*t, v = ((g.J10*ul + g.J11*vl)/det)*t;
        const double r = (rl/det)*t, H = (hl/det)*t, P = (pl/det)*t;
        const double T = r > 0.0 ? (H*P)/(ZN_CP*r) : __builtin_nan("");           // r <= 0 or NaN: the entry says so
        const double wa = (sW[qx]*sW[qy])*det;
        s[0] += wa; s[1] += wa*u; s[2] += wa*v; s[3] += wa*T;
        s[4] += wa*(u*u); s[5] += wa*(v*v); s[6] += wa*(u*v); s[7] += wa*(v*T); s[8] += wa*(T*T);
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int m = 0; m < ZN_MOM; m++) {
        const double t = en_wave_sum(s[m]);
        if (lane == 0) red[wave][m] = t;
    }
    __syncthreads();
    if (tid < ZN_MOM) {                                                           // (lev, band) < (nlev, nb): inside the 9 nlev nb doubles
        double* o = a.acc + ((size_t)tid*a.nlev + lev)*a.nb + a.band[blockIdx.x];
        *o = *o + ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]));
    }
}

bool zonal_overlap(const double* a, size_t na, const double* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na*sizeof(double), b0 = (uintptr_t)b, b1 = b0 + nb*sizeof(double);
    return a0 < b1 && b0 < a1;
}

}  // namespace

// band_host [nEl][mp12] in [-1, nb) -> the context's plan (ctx.hpp ZonalPlan).  The new tables are complete on the device before the
// context names them; the ones they replace are retired (a recording may hold their addresses)
extern "C" int mimsem_zonal_plan_build(mimsem_ctx* c, const int* band_host, int nb) {
    if (!c || !band_host || nb <= 0) return MIMSEM_ERR_ARG;
    if (c->is_capturing()) return MIMSEM_ERR_STATE;
    const size_t total = (size_t)c->nEl*c->es.mp12;
    if (total > (size_t)0x7fffffff) return MIMSEM_ERR_UNSUPPORTED;                // a list entry is an int
    std::vector<int> count(nb, 0);
    for (size_t i = 0; i < total; i++) {
        const int b = band_host[i];
        if (b < -1 || b >= nb) return MIMSEM_ERR_ARG;
        if (b >= 0) count[b]++;
    }
    std::vector<int> bands, off(1, 0), start(nb, 0);
    for (int b = 0; b < nb; b++) {
        if (!count[b]) continue;
        start[b] = off.back();
        bands.push_back(b);
        off.push_back(off.back() + count[b]);
    }
    std::vector<int> pt(off.back());
    for (size_t i = 0; i < total; i++)                                            // ascending e mp12 + q inside every band
        if (band_host[i] >= 0) pt[start[band_host[i]]++] = (int)i;
    ZonalPlan z;
    z.nb = nb; z.nne = (int)bands.size(); z.npts = (int)pt.size();
    if (int rc = c->alloc((void**)&z.band, bands.size()*sizeof(int))) return rc;
    if (int rc = c->alloc((void**)&z.off, off.size()*sizeof(int))) return rc;
    if (int rc = c->alloc((void**)&z.pt, pt.size()*sizeof(int))) return rc;
    if (!bands.empty()) MIMSEM_HIP_TRY(hipMemcpy(z.band, bands.data(), bands.size()*sizeof(int), hipMemcpyHostToDevice));
    MIMSEM_HIP_TRY(hipMemcpy(z.off, off.data(), off.size()*sizeof(int), hipMemcpyHostToDevice));
    if (!pt.empty()) MIMSEM_HIP_TRY(hipMemcpy(z.pt, pt.data(), pt.size()*sizeof(int), hipMemcpyHostToDevice));
    c->zon = z;
    return MIMSEM_OK;
}

extern "C" int mimsem_euler_zonal_moments(mimsem_ctx* c, int nlev, const double* velx, const double* rho, const double* rt,
                                          const double* exner, double* acc) {
    if (!c || !velx || !rho || !rt || !exner || !acc) return MIMSEM_ERR_ARG;
    if (c->zon.nb <= 0 || nlev < 1 || nlev > c->nk) return MIMSEM_ERR_ARG;
    const size_t na = (size_t)ZN_MOM*nlev*c->zon.nb, n1 = (size_t)nlev*c->n1, n2 = (size_t)nlev*c->n2;
    if (zonal_overlap(acc, na, velx, n1) || zonal_overlap(acc, na, rho, n2) || zonal_overlap(acc, na, rt, n2) || zonal_overlap(acc, na, exner, n2))
        return MIMSEM_ERR_ARG;
    if (c->es.n < 1 || c->es.n > 7) return MIMSEM_ERR_UNSUPPORTED;
    ZonalArgs a{};
    if (int rc = elem_tables(c, 0, a.t)) return rc;
    if (c->zon.nne == 0) return MIMSEM_OK;                                        // every point left out: acc + 0.0
    a.nlev = nlev; a.nb = c->zon.nb;
    a.u = velx; a.rho = rho; a.rt = rt; a.ex = exner; a.n1 = c->n1; a.n2 = c->n2;
    a.band = c->zon.band; a.off = c->zon.off; a.pt = c->zon.pt;
    a.acc = acc;
    return for_order<1, 7>(c->es.n, [&](auto n) {             // work item = (non-empty band, level)
        hipLaunchKernelGGL((k_zonal_moments<decltype(n)::value>), dim3((unsigned)c->zon.nne, (unsigned)nlev), dim3(256), 0, c->stream, a);
        MIMSEM_HIP_TRY(hipGetLastError());
        return (int)MIMSEM_OK;
    });
}
