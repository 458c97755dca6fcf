// mimsem_amd/csrc/elem_wave.inc -- included by elem_kernels.hip (inside its anonymous namespace).
//
// k_apply_wave<N, OP, LCT, ACCUM>: the 1-form -> 1-form operators without upwinding (Umat, Uhmat, RotMat, Ut_mat,
// Ut_mat::assemble_h; eul/Assembly.cpp:66-153, 425-470, 1037-1083, 1330-1430) with the scatter-add fused at WAVEFRONT level (round 2).
//
// What bounds this kernel (PMC, profiles/r02_umat_pmc.txt): neither HBM nor the ALUs -- the texture addresser / data path of the CU
// is busy 85 % of the launch while VALU and LDS pipes sit below 10 %: an element kernel issues one vector-memory instruction per
// ~25 useful bytes, and a wave-instruction costs the TA ~30 cycles whatever its width.  Everything here is about issuing FEWER of them:
//  * work item = one wavefront = (wave-group of EPW = 64/LPE neighbouring elements -- 2 x 2 at p <= 3 --, chunk of <= WLC levels).
//  * ONE 16-byte load per level brings every DoF of the group: the reference numbers x- and y-edge DoFs alternately, so the group's
//    distinct slots are covered by <= 64 aligned slot pairs (build_wave_plan); each loaded value is staged to the one or two elements
//    that use it (the two-pass kernel gathers 24 DoFs per element with two 8-byte loads per level and element).
//  * ONE 16-byte store per level: results that meet inside the group are summed through a per-wave LDS strip; a pair of slots
//    complete in the group goes straight into y, every other slot leaves a partial sum in a dense workspace row (k_wave_perim
//    finishes those) -- the element-local result buffer of the two-pass form (192 B per unit written, then read again) is gone.
//  * the metric arrives as ONE record {gaa, gab, gbb, 1/det} = Q/det J^T J (two 16-byte loads instead of five 8-byte ones), the
//    edge-basis table through LDS once per workgroup, every level of the chunk is loaded up front (one latency per work item).
//  * no workgroup barrier after the table load; hand-offs are between lanes of one wavefront, whose LDS operations execute in
//    order: a compiler-level fence is all the synchronisation there is.  Levels go through the phases in lock-step pairs.
//  * the body is BRANCH-FREE: idle lanes run the same instructions on valid dummy addresses and land in dump positions (LDS strips,
//    a tail of the workspace row) that nothing reads; straight-line code lets the compiler count outstanding loads exactly
//    (s_waitcnt vmcnt(n)) -- with exec-mask branches it fell back to vmcnt(0), which on gfx9 also waits for the previous stores.
//  * everything a wavefront shares is SCALAR (wave index through readfirstlane): row bases live in SGPRs, loads take the
//    `saddr + 32-bit lane offset` form; the write-out pointer of a lane is formed once and advanced by its row stride.
// Arithmetic: c = fac * G with fac the operator's level factor (scale, thickness, interpolated field) -- the reference's
// coefficient expressions regrouped (differences ~1e-16 relative; parity tests at 1e-10 against the oracle).
// Round 3: an optional FINISHING PHASE at the end of the kernel (a.wfin, MIMSEM_WAVE_FIN=1) completes the perimeter slots inside the
// launch -- the group that reaches a side second adds the two partial sums -- instead of k_wave_perim.  Bit-exact and measured
// 2.4x slower (the hand-off has to be coherent across XCDs: DESIGN 4.6, profiles/r03_fin_experiments.txt); off by default.
// Build-time A/B knobs: MIMSEM_WNW, MIMSEM_WAHEAD, MIMSEM_WLB, MIMSEM_NO_TPAIR, MIMSEM_WAVE_NT (non-temporal streaming accesses:
// slower), MIMSEM_PLC (levels per thread of the perimeter pass: no effect), MIMSEM_STAMPS (s_memtime stamps of a wave's phases).
#ifndef MIMSEM_WNW
#define MIMSEM_WNW 4
#endif
#ifndef MIMSEM_WAHEAD
#define MIMSEM_WAHEAD 2         // level batches k_apply_wave requests ahead of the one it computes (A/B knob)
#endif
#ifndef MIMSEM_WLB
#define MIMSEM_WLB 2            // levels a wavefront of k_apply_wave takes in lock-step (A/B knob: scripts/ab_wlb.sh)
#endif
constexpr int WNW = MIMSEM_WNW;    // wavefronts per workgroup of k_apply_wave
constexpr int WLC = 8;              // compile-time bound on the levels of one work item (LCT = 1 serves single-level calls)

typedef __attribute__((address_space(1))) double gdouble;     // global address space spelled out: a pointer chosen per lane between two
                                                              // buffers and advanced in a loop otherwise degrades to FLAT stores
typedef __attribute__((address_space(1))) char gchar;

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Level ranges: a wavefront whose work item has `left` <= 0 levels left ENDS (wave-uniform: `left` is an SGPR).  The stores of its last
// batch are issued (program order: the statement is volatile and clobbers memory) and complete on their own; the loads still in flight
// went to valid addresses and are abandoned: no s_waitcnt is ISSUED for them.  (That is a statement about instructions, not latency:
// the hardware drains a wave's outstanding memory counters at s_endpgm, so the wave's slot stays held until those loads have returned.)
// To the compiler this is ONE opaque instruction, so the ring of batches stays one basic block: written as a C++ branch out of the
// ring, the three exits cost the owner kernel its register allocation (168 VGPRs and 14 spilled, against 150 and none).
// The compiler does not know that the kernel can end here: whatever the kernel does BEHIND the level loop is skipped by a wavefront
// that leaves this way.  Only the form with nothing behind the loop may use it (OWN: see the tail of k_apply_wave).
__device__ __forceinline__ void wave_exit_if_done(int left) {
    asm volatile("s_cmp_gt_i32 %0, 0\n\ts_cbranch_scc1 .Lwave_goes_on%=\n\ts_endpgm\n.Lwave_goes_on%=:" :: "s"(left) : "scc", "memory");
}

// 64-bit value of another lane of the same DPP row (16 lanes = one element at p = 3): two v_mov_b32_dpp.  CTRL: quad_perm [j,j,j,j] =
// j*0x55 (lane j of the caller's quad), row_ror:n = 0x120 + n (lane L reads lane (L - n) mod 16 of its row).  The compiler owns the
// hazard handling of these builtins (unlike the inline-asm DPP FMAs of the column kernels).
template <int CTRL>
__device__ __forceinline__ double dpp64(double x) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// y = sum_k c[k] * (x of the lane k rows of the 4 x 4 point grid below, cyclically): lane (qx, qy) reads (qx, (qy - k) mod 4)
__device__ __forceinline__ double dpp_rows(const double (&c)[4], double x) {
    double r = c[0]*x;                                   // explicit fma chain: the same bits from every instantiation of the kernel
    r = fma(c[1], dpp64<0x124>(x), r);
    r = fma(c[2], dpp64<0x128>(x), r);
    r = fma(c[3], dpp64<0x12C>(x), r);
    return r;
}
// y = sum_j c[j] * (x of lane j of the caller's quad): lane (qx, qy) reads (j, qy)
template <int NJ>
__device__ __forceinline__ double dpp_quad(const double* c, double x) {
    double r = c[0]*dpp64<0x00>(x);
    r = fma(c[1], dpp64<0x55>(x), r);
    r = fma(c[2], dpp64<0xAA>(x), r);
    if constexpr (NJ > 3) r = fma(c[3], dpp64<0xFF>(x), r);
    return r;
}

// 16-byte accesses that are coherent across the chip (`sc1`: written through / read past this CU's L1): what the finishing phase of
// k_apply_wave hands from one wavefront to another, possibly on another XCD, inside one launch
typedef unsigned int wave_u4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) wave_u4 gwave_u4;
__device__ __forceinline__ void store_pair_agent(gdouble* p, double a, double b) {
    wave_u4 v;
    v.x = (unsigned)__double2loint(a); v.y = (unsigned)__double2hiint(a); v.z = (unsigned)__double2loint(b); v.w = (unsigned)__double2hiint(b);
    __builtin_amdgcn_global_store_b128((gwave_u4*)p, v, "agent");
}
__device__ __forceinline__ double2 load_pair_agent(const double* p) {
    const wave_u4 v = __builtin_amdgcn_global_load_b128((gwave_u4*)p, "agent");
    double2 r; r.x = __hiloint2double((int)v.y, (int)v.x); r.y = __hiloint2double((int)v.w, (int)v.z);
    return r;
}

// streaming accesses of the level loop (x, thickInv, y): MIMSEM_WAVE_NT=1 marks them non-temporal so that the level-invariant tables and
// the metric stay in the XCD's L2 from one launch to the next (A/B knob, scripts/build_variant.sh)
#ifndef MIMSEM_WAVE_NT
#define MIMSEM_WAVE_NT 0
#endif
typedef double wave_d2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) wave_d2 gwave_d2;
#if MIMSEM_WAVE_NT
__device__ __forceinline__ double2 wload2(const void* p) { const wave_d2 v = __builtin_nontemporal_load((const wave_d2*)p); double2 r; r.x = v.x; r.y = v.y; return r; }
#else
__device__ __forceinline__ double2 wload2(const void* p) { return *(const double2*)p; }
#endif
#define WLOAD(T, p) wload2(p)

#ifdef MIMSEM_STAMPS      // diagnostic build only (scripts/stamp_wave.sh): s_memtime stamps of one wave's phases, written by lane 0
#define WSTAMP(k) do { if (a.wstamps && lane == 0) a.wstamps[(size_t)item*16 + (k)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#else
#define WSTAMP(k) do { } while (0)
#endif

// TILE (round 5, a.wtfin): the four wavefronts of a workgroup are the four wave-groups of a TILE (2 x 2 groups = 4 x 4 elements at p = 3);
// the partial sums of the slots two groups of the tile share go into the workgroup's LDS instead of the workspace row, and after ONE
// barrier per work item the workgroup adds the pairs and stores the slots straight into y -- the perimeter pass then only sees the tile's
// OUTER perimeter (half the partial sums, half the slots).  Round 1's workgroup-level form had a barrier per LEVEL (+27 % on the element
// kernel); this one has a barrier per <= 32 levels.
// OWN (round 7, a.wgh; build_wave_own): owner-computes.  Every store pair has one owner group, which also computes the contribution of
// the neighbour element across each of its (<= 4) GHOST SIDES (round 7: a second, virtual element row of the wavefront per side, laid
// out as the neighbour's lanes, running the element's whole DPP algebra per level; round 9: packed ghost lanes, below), with the
// neighbour's DoFs (one 8-byte gather per lane and level), metric and thickInv.  At p = 3 a slot on a side depends on the side's 4 points
// only, so the side's slots come out with the neighbour's bits; they join the group's sums in the strip.  Every pair is written
// finished into y by its owner: no partial sums and no perimeter pass.
// Round 9: PACKED ghost lanes.  A ghost lane is one (side, point along it, level): ONE ghost pass covers two levels, in four DPP rows
// -- x-normal sides of level 0 | y-normal sides of level 0 | the same for level 1 -- (round 7 ran a whole 64-lane element row per side
// and level, 16 of 64 lanes producing slots).  In an x-normal row the side is the column (qx) and the point along it the row (qy); in
// a y-normal row the point is the column and the side the row: the point along the side then sits where the element's coefficients
// of that point are (cu, cp in qy; Ex, pq in qx), and the along-side operations ARE the element's -- dpp_rows for x-normal sides,
// dpp_quad for y-normal ones, the same rotations, broadcasts and fma order.  The plan gathers, per side point, its 3 cross-edge DoFs in
// the order the neighbour's chain reads them and its DoF on the side: one 16-byte-aligned quadruple, two ds_read_b128.  The cross-side
// interpolation is a local chain of the 3 cross DoFs.  Every slot comes out of the very fma sequence of the neighbour's own lanes.
template <int N, int OP, int LCT, bool ACCUM, bool TILE = false, bool OWN = false>
__global__ __launch_bounds__(64*WNW) __attribute__((amdgpu_waves_per_eu(OWN ? 3 : (OpTraits<OP>::cf == SN ? 4 : 3), 8))) void k_apply_wave(ElemArgs a) {
    using D = Dims<N>;
    using T = OpTraits<OP>;
    static_assert(T::in == S1 && T::out == S1 && !T::up && T::cf2 == SN, "1-form -> 1-form operators without upwinding");
    constexpr int LPE = D::LPE, EPW = 64/LPE, ND = 2*D::n1e, NW = WNW;
    constexpr int NACC = EPW*ND, ZERO = NACC + 128;
    constexpr int RS = D::mp1 + (D::mp1 & 1);            // padded row of the y-edge DoFs: 16-byte aligned rows
    constexpr int XT = D::n1e + D::mp1*RS;               // staged DoFs of an element; XT of element 0 is the staging dump
    constexpr int SXE = XT + 2*(LPE - D::n1e) + ((XT + 2*(LPE - D::n1e)) & 1);       // (build_wave_plan uses the same numbers)
    constexpr int WGR = NACC + 136;                      // owner-computes: the ghost results of a level, side*4 + point (build_wave_own uses the same number)
    constexpr int SW = (EPW*SXE > WGR + (OWN ? 32 : 0)) ? EPW*SXE : WGR + (OWN ? 32 : 0);     // strip of one level: staged x, later its summed results
    constexpr int LB = LCT >= MIMSEM_WLB ? MIMSEM_WLB : (LCT >= 2 ? 2 : LCT);      // levels in lock-step
    static_assert(LCT%LB == 0, "whole batches");
    __shared__ double sE[NW][D::mp1*N];                  // edge-basis table, wave-private copy (written from SGPRs: no load, no barrier)
    __shared__ double s_x[NW][LB][SW];                   // x of a level; after the interpolation: results | dump strips | a zero
    constexpr bool LDSF = (T::cf == S2) && (N != 3), LDSAB = (N != 3);      // p = 3 moves these through DPP instead
    __shared__ double s_f[LDSF ? NW : 1][LDSF ? LB : 1][LDSF ? EPW : 1][LDSF ? LPE : 1];
    __shared__ double s_a[LDSAB ? NW : 1][LDSAB ? LB : 1][LDSAB ? EPW : 1][LDSAB ? LPE : 1];
    __shared__ double s_b[LDSAB ? NW : 1][LDSAB ? LB : 1][LDSAB ? EPW : 1][LDSAB ? LPE : 1];
    static_assert(!TILE || NW == 4, "a tile is the four wavefronts of a workgroup");
    __shared__ double s_t[TILE ? MIMSEM_WTLEV : 1][TILE ? MIMSEM_WTP : 2];      // tile mode: pairs of partial sums of the inner slots, per level of the work item
    static_assert(!OWN || (N == 3 && OP == MIMSEM_OP_UMAT && !TILE), "owner-computes: Umat at p = 3");
    constexpr int WGX = MIMSEM_WGX;
    __shared__ __attribute__((aligned(16))) double s_g[OWN ? NW : 1][OWN ? LB : 1][OWN ? WGX : 1];      // owner-computes: the gathered ghost DoFs of a level (16 B quadruples)

#ifdef MIMSEM_STAMPS
    const long long t_entry = (long long)__builtin_amdgcn_s_memtime();
#endif
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63, el = lane/LPE, q = lane%LPE;
    // a work item = (wave-group, first level, number of levels): tables, metric and basis values are loaded once for all of them.  Level
    // RANGES (a.wnp > 0; the owner form always): the group's wnp parts of whole level pairs (ElemArgs::wnp); otherwise `wcpp` consecutive
    // chunks of a.lch levels
    const bool ranged = OWN || a.wnp > 0;                // wave-uniform (kernel argument)
    const unsigned nchunk = ranged ? (unsigned)a.wnp
                                   : ((unsigned)((a.nlev + a.lch - 1)/a.lch) + (unsigned)a.wcpp - 1)/(unsigned)a.wcpp;     // parts per group
    const unsigned nitems = (unsigned)a.wgroups*nchunk;                        // < 2^31: checked by the launcher
    const unsigned bid = xcd_swizzle(blockIdx.x, gridDim.x, a.swz & 1);
    const unsigned item = bid*NW + (unsigned)wv;
    if (item >= nitems) return;                          // wave-uniform
    unsigned g, ch;
    if (!TILE && (a.swz & 2)) { g = item/nchunk; ch = item%nchunk; }            // group-major: the chunks of a group are neighbours
    else           { g = item%(unsigned)a.wgroups; ch = item/(unsigned)a.wgroups; }       // (tile mode: wgroups is a multiple of 4, so a workgroup = one tile, one chunk)
    g += (unsigned)a.wg0;                                // a launch over a sub-range of the groups (interior / boundary split)
    int lbeg, lend;                                      // the item's levels [lbeg, lend): SGPRs
    if (ranged) { lbeg = 2*((int)ch*a.wpb + min((int)ch, a.wpr)); lend = min(a.nlev, lbeg + 2*(a.wpb + ((int)ch < a.wpr ? 1 : 0))); }
    else        { lbeg = (int)ch*a.lch*a.wcpp; lend = min(a.nlev, lbeg + a.lch*a.wcpp); }
#ifdef MIMSEM_STAMPS
    if (a.wstamps && lane == 0) a.wstamps[(size_t)item*16 + 0] = t_entry;
#endif
    const int4 wl = a.wlane[(size_t)g*64 + lane];        // {element, load pair, its staging positions}
    const int4 wp = a.wplan[(size_t)g*64 + lane];        // {store pair destination, result positions}
    // owner-computes: the lane's packed ghost lane -- DPP row 2*gl + y-normal, level gl of a pass (LB = 1: rows 2, 3 repeat rows 0, 1)
    // {metric record of the neighbour's point, its element*16 + point, qy0 (y-normal) or qx0 (x-normal) = 3 << 1 | no side DoF << 2,
    // position of its quadruple in the gathered strip | of its result (WGR + ..) << 8} -- and the slot the lane gathers per level
    constexpr int NGP = (LB + 1)/2;                      // ghost passes per batch (two levels each)
    const bool gyn = ((lane >> 4) & 1) != 0;
    const int gl = LB >= 2 ? (lane >> 5) : 0;
    int4 gh = {0, 0, 0, 0}; int gxs = 0;
    double2 h01 = {0.0, 0.0}, h23 = {0.0, 0.0};
    if constexpr (OWN) {
        gh = a.wgh[(size_t)g*32 + (lane & 31)]; gxs = a.wgx[(size_t)g*64 + lane];
        const double2* hp = (const double2*)(a.wG + (size_t)gh.x*4);
        h01 = hp[0]; h23 = hp[1];
    }
    const bool gsz = (gh.z & 4) != 0;
    const int gc0 = (gh.z & 2) ? 3 : 0;
    const unsigned gxo = 8u*(unsigned)gxs, gqg = (unsigned)gh.y;
    // the metric is stored in wave-group order: its address needs no table, so it travels together with the tables
    double gaa = 0.0, gab = 0.0, gbb = 0.0, rdet = 0.0, rr = 0.0;
    if constexpr (OP == MIMSEM_OP_ROTMAT) rr = a.scale*a.wR[(size_t)g*64 + lane];
    else {
        const double2* gp = (const double2*)(a.wG + ((size_t)g*64 + lane)*4);
        const double2 g01 = gp[0], g23 = gp[1];
        gaa = a.scale*g01.x; gab = a.scale*g01.y; gbb = a.scale*g23.x; rdet = g23.y;
    }
    const int e = wl.x;
    const int qq = min(q, D::mp12 - 1);                  // lanes beyond the point grid repeat its last point (results unused)
    const int qd = min(q, D::n1e - 1);                   // lanes beyond the edge functions repeat the last one
    const int qx = qq%D::mp1, qy = qq/D::mp1;
    const unsigned gq = (unsigned)e*D::mp12 + (unsigned)qq;                     // nEl*mp12*8 < 2^32: checked by the launcher
    constexpr bool DPP = (N == 3);
    unsigned fo = 0;
    if constexpr (T::cf == S2 && DPP) { const int ff = (qx < 3 && qy < 3) ? qy*3 + qx : 0; fo = 8u*(unsigned)(a.i2 ? a.i2[e*D::n2e + ff] : e*D::n2e + ff); }
    else if constexpr (T::cf == S2) { const int qf = min(q, D::n2e - 1); fo = 8u*(unsigned)(a.i2 ? a.i2[e*D::n2e + qf] : e*D::n2e + qf); }
    if constexpr (T::cf == S0) fo = 8u*(unsigned)a.wnode[(size_t)g*64 + lane];
    const unsigned xo = 8u*(unsigned)wl.y;
    // thickInv pair of the lane's point: [element][point] table, or (experiment, MIMSEM_WAVE_TNODE=1) the nodal one through the lane's node slot
    const unsigned to = a.tnode ? 16u*(unsigned)a.wnode[(size_t)g*64 + lane] : 16u*gq;
    // the level loads need nothing but the lane table: they are requested BEFORE the basis table is staged and the level-invariant
    // registers are set up (s_memtime stamps of the cache-resident launch: 70 % of a wavefront's life was the chain tables -> set-up ->
    // first level loads -> first data; the set-up now runs under the loads)
    // ---- level loads, software-pipelined: two batches in flight ahead of the one being computed.  All waves of a CU start together;
    // issuing every level up front put the whole launch's loads in front of the texture addresser before anybody computed
    // (s_memtime stamps: 5.7k of a wave's 20k cycles went into ISSUING 16 loads) ----
    double2 px[LCT]; double pf0[T::cf != SN ? LCT : 1], pt0[LCT], pt1[OP == MIMSEM_OP_UTMAT ? LCT : 1];
    double pg[OWN ? LCT : 1], ptg[OWN ? (LCT/LB)*((LB + 1)/2) : 1];     // owner-computes: the lane's gathered ghost DoF; thickInv of its ghost lane (per pass)
    const size_t lstride = (size_t)a.nEl*D::mp12;
    // the loads run AHEAD batches in front of the computed one, circularly over the LCT levels of a chunk and on into the next chunk
    // of the work item (register r holds level lbeg + r of this chunk, or lbeg + LCT + r of the next once level r is consumed)
#ifdef MIMSEM_NO_TPAIR                                      // A/B build (scripts/ab_tpair.sh)
    constexpr bool TPAIR = false;
#else
    constexpr bool TPAIR = (LB%2 == 0) && OP != MIMSEM_OP_UTMAT;
#endif
    // TPAIR: thickInv of the two lock-step levels in ONE 16-byte load (ctx.d_tIp)
    auto load_batch = [&](int r0, int lev0_) {
        if constexpr (TPAIR) {
#pragma unroll
            for (int i = 0; i < LB; i += 2) {
                const int L = a.lev0 + min(lev0_ + i, a.nlev - 1);   // (a level beyond the range reads a valid pair; nothing is stored for it)
                const double2 tp = WLOAD(double2, (const char*)(a.tIp + ((size_t)(L & 1)*a.tnp + (size_t)(L >> 1))*(size_t)a.tps) + to);
                pt0[r0 + i] = tp.x; pt0[r0 + i + 1] = tp.y;
            }
            if constexpr (OWN) {                             // ONE load per ghost pass: the ghost lane's level, from the pair table
#pragma unroll
                for (int t = 0; t < NGP; t++) {
                    const int L = a.lev0 + min(lev0_ + 2*t, a.nlev - 1);
                    ptg[(r0/LB)*NGP + t] = *(const double*)((const char*)(a.tIp + ((size_t)(L & 1)*a.tnp + (size_t)(L >> 1))*(size_t)a.tps) + 16u*gqg + 8u*(unsigned)gl);
                }
            }
        } else if constexpr (OWN) {                          // the ghost lane's level only
#pragma unroll
            for (int t = 0; t < NGP; t++) {
                const int lev = min(lev0_ + 2*t + gl, a.nlev - 1);
                ptg[(r0/LB)*NGP + t] = *(const double*)((const char*)(a.tI + (size_t)(a.lev0 + lev)*lstride) + 8u*gqg);
            }
        }
#pragma unroll
        for (int i = 0; i < LB; i++) {
            const int r = r0 + i;
            const int lev = min(lev0_ + i, a.nlev - 1);      // beyond the last level: re-read it (nothing is stored for it)
            px[r] = WLOAD(double2, (const char*)(a.x + (size_t)lev*a.xs) + xo);
            if constexpr (T::cf != SN) pf0[r] = *(const double*)((const char*)(a.f + (size_t)lev*a.fs) + fo);
            if constexpr (OP == MIMSEM_OP_UTMAT) {
                const char* tb = (const char*)(a.th + (size_t)(a.lev0 + lev)*lstride);
                pt0[r] = *(const double*)(tb + 8u*gq); pt1[r] = *(const double*)(tb + 8*lstride + 8u*gq);
            } else if constexpr (!TPAIR) pt0[r] = *(const double*)((const char*)(a.tI + (size_t)(a.lev0 + lev)*lstride) + 8u*gq);
            if constexpr (OWN) pg[r] = *(const double*)((const char*)(a.x + (size_t)lev*a.xs) + gxo);
        }
    };
    constexpr int AHEAD = (LCT/LB > MIMSEM_WAHEAD) ? MIMSEM_WAHEAD : LCT/LB - 1;      // batches requested ahead of the computed one
#pragma unroll
    for (int b = 0; b < (AHEAD ? AHEAD : 1); b++) { load_batch(b*LB, lbeg + b*LB); __builtin_amdgcn_sched_barrier(0); }   // in THIS order: vmcnt is in-order
    {   // kernel arguments sit in SGPRs: one lane copies the table into the wave's LDS strip
        double* se = sE[wv];
#pragma unroll
        for (int k = 0; k < D::mp1*N; k++) se[k] = a.Etab[k];
    }
    wave_fence();
    WSTAMP(1);                                           // tables and metric requested, basis table staged

    // ---- level-invariant registers: metric, basis values, write-out plan ----
    const bool vert = (a.flags & MIMSEM_FLAG_VERT) != 0;
    double Ex[N], Ey[N];             // E[qx][j], E[qy][j]: interpolation to this lane's point
    double Pa[D::mp1], Pb[D::mp1];   // alpha E[k][iyx], alpha E[k][ixy]: projection onto this lane's two edge functions
#pragma unroll
    for (int j = 0; j < N; j++) { Ex[j] = sE[wv][qx*N + j]; Ey[j] = sE[wv][qy*N + j]; }
    const int ixx = qd%D::np1, iyx = qd/D::np1;   // x-normal edge: node in x, edge function in y
    const int ixy = qd%N,      iyy = qd/N;        // y-normal edge: edge function in x, node in y
#pragma unroll
    for (int k = 0; k < D::mp1; k++) { Pa[k] = a.alpha*sE[wv][k*N + iyx]; Pb[k] = a.alpha*sE[wv][k*N + ixy]; }
    // p = 3: an element is one DPP row (lane = qy*4 + qx), so interpolation and projection move data between lanes by row rotations
    // (the y direction) and quad broadcasts (the x direction) instead of through LDS; per-lane coefficients of the rotated terms:
    //   cu[k] = E[qy][(qy-k) mod 4]      u = sum_j E[qy][j] ux[j][qx],  ux[j][qx] held by lane (qx, j), j < 3
    //   cp[k] = alpha E[(qy-k) mod 4][qy]  y_x(dof (qx, qy)) = sum_k E[k][qy] a(qx, k),  qy < 3
    double cu[4] = {0.0, 0.0, 0.0, 0.0}, cp[4] = {0.0, 0.0, 0.0, 0.0}, pq[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (DPP) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = (qy - k) & 3;
            cu[k] = j < 3 ? sE[wv][qy*N + j] : 0.0;
            cp[k] = qy < 3 ? a.alpha*sE[wv][j*N + qy] : 0.0;
            pq[k] = qx < 3 ? a.alpha*sE[wv][k*N + qx] : 0.0;            // y_y(dof (qx, qy)) = sum_k E[k][qx] b(k, qy),  qx < 3
        }
    }
    // owner-computes, per packed ghost lane: the element's own coefficients of its point serve the along-side terms (see the header); the
    // cross chain over the lane's 3 gathered cross DoFs takes kc = E[c0][t], t the edge function of the operand, in the neighbour's
    // order (x-normal: Y(t, point), dpp_quad; y-normal: X(point, t), dpp_rows rotation order from row c0, the zero row-3 term folded into
    // the chain's start: +0 instead of the -0 that makes fma(k, x, -0) the plain product); gm0, gm1 = the metric pair of the side's
    // slots, {gaa, gab} (ra, x-normal) or {gab, gbb} (rb, y-normal), times scale
    double kc[3] = {0.0, 0.0, 0.0}, gm0 = 0.0, gm1 = 0.0;
    const double* sgl = nullptr;                          // the ghost lane's quadruple {cross 0, cross 1, cross 2, side DoF}
    double* sgr = nullptr;                                // where its result goes: WGR + side block*4 + point of its level's strip
    if constexpr (OWN) {
        const double hgaa = a.scale*h01.x, hgab = a.scale*h01.y, hgbb = a.scale*h23.x;
        gm0 = gyn ? hgab : hgaa; gm1 = gyn ? hgbb : hgab;
#pragma unroll
        for (int t = 0; t < 3; t++) {
            const int tt = !gyn ? t : (gc0 == 0 ? (t == 0 ? 0 : 3 - t) : 2 - t);
            kc[t] = sE[wv][gc0*N + tt];
        }
        sgl = &s_g[wv][gl][gh.w & 0xFF];
        sgr = &s_x[wv][gl][WGR + (gh.w >> 8)];
    }
    const int xd00 = wl.z & 0xFFFF, xd01 = (wl.z >> 16) & 0xFFFF, xd10 = wl.w & 0xFFFF, xd11 = (wl.w >> 16) & 0xFFFF;
    const bool hasx = q < D::n1e;
    // result positions in the wave's strip: x-edge DoF q at lane q; y-edge DoF at lane q (LDS form) or, DPP form, DoF qy*3 + qx at
    // lane (qx < 3, qy)
    const int aci0 = hasx ? el*ND + q : NACC + lane;
    const int aci1 = DPP ? (qx < 3 ? el*ND + D::n1e + qy*3 + qx : NACC + 64 + lane) : (hasx ? el*ND + D::n1e + q : NACC + 64 + lane);
    const int ldx = q < D::n1e ? q : 0, ldy = D::n1e + qy*RS + (qx < 3 ? qx : 0);     // DPP form: the lane's own two DoFs in the staging strip
    const bool okx = q < D::n1e, oky = qx < 3, okf = qx < 3 && qy < 3;
    const int wp00 = wp.y & 0xFFFF, wp01 = (wp.y >> 16) & 0xFFFF, wp10 = wp.z & 0xFFFF, wp11 = (wp.z >> 16) & 0xFFFF;
    const bool wy = wp.x >= 0;
    const bool tin = TILE && wp.w > 0;                  // my pair goes into the tile's LDS row (its global store lands in the dump tail)
    const int tpo = tin ? wp.w - 1 : 0;
    gchar* wo = (gchar*)(tin ? (a.out + a.wdump + 2*lane) : (wy ? (a.y + (size_t)lbeg*a.ys + wp.x) : (a.out + (size_t)lbeg*a.os + (-wp.x - 2))));
    const long long wst = tin ? 0 : 8*(wy ? a.ys : a.os);
    // optional 8-byte round (MIMSEM_WAVE_SINGLES=1): complete slots without a complete partner, straight into y
    int sp0 = ZERO, sp1 = ZERO; gchar* so = nullptr;
    if (!OWN && a.wsing) {
        const int2 w = a.wsing[(size_t)g*64 + lane];
        sp0 = w.y & 0xFFFF; sp1 = (w.y >> 16) & 0xFFFF;
        so = (gchar*)(w.x >= 0 ? a.y + (size_t)lbeg*a.ys + w.x : a.out + a.wdump + lane);
    }
    const long long sst = (a.wsing && so != (gchar*)(a.out + a.wdump + lane)) ? 8*a.ys : 0;

    WSTAMP(2);                                           // tables, metric and basis values requested
    WSTAMP(3);                                           // level loads issued
    static_assert(ZERO >= EPW*SXE && ZERO < SW, "the zero entry lies beyond the staged x and the results: written once");
#pragma unroll
    for (int i = 0; i < LB; i++) s_x[wv][i][ZERO] = 0.0;     // every lane, same value: the second operand of single-contributor sums
    gchar* const dumpp = (gchar*)(a.out + a.wdump + 2*lane);   // tail of the first partial-sum row
    gchar* const dumps = (gchar*)(a.out + a.wdump + lane);
    // one trip = the ring of LCT levels (a chunk form's item holds whole chunks of LCT levels, or a single shorter one)
    for (int cc = 0; lbeg < lend; cc++, lbeg += LCT) {   // wave-uniform
    const int nl = lend - lbeg;                          // levels the item still has: the ring's levels l >= nl store into the dump tail
#pragma unroll
    for (int b0 = 0; b0 < LCT; b0 += LB) {
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (AHEAD > 0) load_batch((b0 + AHEAD*LB)%LCT, lbeg + b0 + AHEAD*LB);
        __builtin_amdgcn_sched_barrier(0);               // keep the requests ahead of this batch's work, and behind the earlier ones
#pragma unroll
        for (int i = 0; i < LB; i++) {
            double* st = s_x[wv][i];
            st[xd00] = px[b0 + i].x; st[xd01] = px[b0 + i].x; st[xd10] = px[b0 + i].y; st[xd11] = px[b0 + i].y;
            if constexpr (T::cf == S2 && !DPP) s_f[wv][i][el][q] = pf0[b0 + i];
            if constexpr (OWN) s_g[wv][i][lane] = pg[b0 + i];
        }
        wave_fence();
        double yxr[LB], yyr[LB];
#pragma unroll
        for (int i = 0; i < LB; i++) {
            const int l = b0 + i;
            const double* sx = s_x[wv][i] + el*SXE;
            double u = 0.0, v = 0.0, fu = 0.0, ra, rb;
            if constexpr (DPP) {
                double X = sx[ldx], Y = sx[ldy];         // the lane's own x-edge DoF (rows qy < 3) and y-edge DoF (columns qx < 3)
                if (!okx) X = 0.0;
                if (!oky) Y = 0.0;
                u = dpp_rows(cu, X);                      // Geom::interp1_l eul/Geom.cpp:342-361, collocated nodal table
                v = dpp_quad<3>(Ex, Y);
                if constexpr (T::cf == S2) {              // Geom::interp2_l :363-376, x direction in the quad, y direction over the rows
                    double F = okf ? pf0[l] : 0.0;
                    fu = dpp_rows(cu, dpp_quad<3>(Ex, F));
                } else if constexpr (T::cf == S0) fu = pf0[l];
            } else {
#pragma unroll
                for (int j = 0; j < N; j++) {               // Geom::interp1_l eul/Geom.cpp:342-361, collocated nodal table
                    u = fma(sx[j*D::np1 + qx], Ey[j], u);
                    v = fma(sx[D::n1e + qy*RS + j], Ex[j], v);
                }
                if constexpr (T::cf == S2) {                // Geom::interp2_l :363-376
                    const double* sf = s_f[wv][i][el];
#pragma unroll
                    for (int jy = 0; jy < N; jy++)
#pragma unroll
                        for (int jx = 0; jx < N; jx++)
                            fu = fma(sf[jy*N + jx], Ex[jx]*Ey[jy], fu);
                } else if constexpr (T::cf == S0) fu = pf0[l];   // interp0 at a collocated node: the lane's own value
            }
            // level factor of the operator (the coefficient loops of Assembly.cpp:99-113, 432-448, 1051-1065, 1352-1364, 1402-1413)
            double fac;
            if constexpr (OP == MIMSEM_OP_UMAT) fac = vert ? pt0[l] : 1.0;
            else if constexpr (OP == MIMSEM_OP_UHMAT) { double hi = fu*rdet; if (vert) hi *= pt0[l]; fac = hi*pt0[l]; }
            else if constexpr (OP == MIMSEM_OP_UTMAT) fac = 0.5*(pt0[l] + pt1[l]);
            else if constexpr (OP == MIMSEM_OP_UTMAT_H) fac = fu*rdet;
            else fac = (fu*pt0[l])*pt0[l];              // RotMat: vorticity * thickInv, coefficient * thickInv
            if constexpr (OP == MIMSEM_OP_ROTMAT) { const double c = fac*rr; ra = c*v; rb = -c*u; }
            else { ra = fac*fma(gab, v, gaa*u); rb = fac*fma(gbb, v, gab*u); }      // explicit fma: identical bits in every instantiation
            if constexpr (DPP) { yxr[i] = dpp_rows(cp, ra); yyr[i] = dpp_quad<4>(pq, rb); }
            else { s_a[wv][i][el][q] = ra; s_b[wv][i][el][q] = rb; }
        }
        double gyr[NGP];
#pragma unroll
        for (int t = 0; t < (OWN ? NGP : 0); t++) {       // the ghost passes: every side point of two levels at once
            const double2 c01 = *(const double2*)(sgl + 2*t*WGX), c2s = *(const double2*)(sgl + 2*t*WGX + 2);
            const double S = gsz ? 0.0 : c2s.y;           // (x-normal: the side's point 3 has no DoF; the neighbour's lane holds a zero)
            double C = fma(kc[0], c01.x, gyn ? 0.0 : -0.0);   // across the side: the lane's own operands
            C = fma(kc[1], c01.y, C);
            C = fma(kc[2], c2s.x, C);
            const double Ar = dpp_rows(cu, S), Aq = dpp_quad<3>(Ex, S);      // along the side: the element's interpolation
            const double gu_ = gyn ? C : Ar, gv_ = gyn ? Aq : C;
            const double gf = vert ? ptg[(b0/LB)*NGP + t] : 1.0;
            const double gr = gf*fma(gm1, gv_, gm0*gu_);   // ra (x-normal) or rb (y-normal) of the neighbour's point
            const double Pr = dpp_rows(cp, gr), Pq = dpp_quad<4>(pq, gr);    // ... and its projection
            gyr[t] = gyn ? Pq : Pr;
        }
        wave_fence();                                     // (DPP form: every lane has read its DoFs: the strips may take the results)
#pragma unroll
        for (int i = 0; i < LB; i++) {
            double yx = 0.0, yy = 0.0;
            if constexpr (DPP) { yx = yxr[i]; yy = yyr[i]; }
            else {
                const double* sa = s_a[wv][i][el];
                const double* sb = s_b[wv][i][el];
#pragma unroll
                for (int k = 0; k < D::mp1; k++) {
                    yx = fma(Pa[k], sa[k*D::mp1 + ixx], yx);
                    yy = fma(Pb[k], sb[iyy*D::mp1 + k], yy);
                }
            }
            double* sacc = s_x[wv][i];                    // the level's x is spent: its strip takes the results
            sacc[aci0] = yx; sacc[aci1] = yy;
        }
#pragma unroll
        for (int t = 0; t < (OWN ? NGP : 0); t++) sgr[2*t*SW] = gyr[t];     // the neighbour's contribution to the side slot of this ghost lane
        wave_fence();
#pragma unroll
        for (int i = 0; i < LB; i++) {
            const int l = b0 + i;
            const double* sacc = s_x[wv][i];
            double2 val;
            val.x = sacc[wp00] + sacc[wp01]; val.y = sacc[wp10] + sacc[wp11];
            // a level the ragged last chunk does not have stores into the dump tail (a select, not a branch: see the header)
            gdouble* o = (gdouble*)(l < nl ? wo : dumpp);
            if constexpr (ACCUM) { double o0 = o[0], o1 = o[1]; if (!wy) { o0 = 0.0; o1 = 0.0; } val.x += o0; val.y += o1; }
#if MIMSEM_WAVE_NT
            { wave_d2 vv; vv.x = val.x; vv.y = val.y; __builtin_nontemporal_store(vv, (__attribute__((address_space(1))) wave_d2*)o); }
#else
            if constexpr (TILE) { if (!tin) { o[0] = val.x; o[1] = val.y; } }       // (an inner pair has no global destination: a dump address shared by every wavefront of the launch is an L2 hot spot)
            else { o[0] = val.x; o[1] = val.y; }          // (partial sums: the row lives in uncached memory when a finishing phase follows)
#endif
            if constexpr (TILE) {                         // (a level the ragged last chunk does not have lands in a row nobody finishes)
                if (tin) { double* td = &s_t[cc*a.lch + l][tpo]; td[0] = val.x; td[1] = val.y; }      // an LDS store under the lane's mask: no vmcnt involved
            }
            wo += wst;
            if (!OWN && a.wsing) {                        // wave-uniform; off by default
                const double v1 = sacc[sp0] + sacc[sp1];
                gdouble* o1 = (gdouble*)(l < nl ? so : dumps);
                if constexpr (ACCUM) *o1 = (sst ? *o1 : 0.0) + v1; else *o1 = v1;
                so += sst;
            }
        }
        wave_fence();        // the strips are free again before the next batch lands in them
        WSTAMP(4 + b0/LB);                                // batch done (its stores issued)
        // level ranges: the item ends with the batch that holds its last level -- a scalar branch on a wave-uniform value, behind the
        // batch's stores.  The requests still in flight went to valid addresses (load_batch clamps) and are abandoned: no wait is issued
        // for them (s_endpgm itself lets them drain).  (The ring's last batch leaves through the loop condition.)
#ifdef MIMSEM_STAMPS
        if constexpr (OWN) { if (b0 + LB < LCT && b0 + LB >= nl) goto levels_done; }
#else
        if constexpr (OWN) { if (b0 + LB < LCT) wave_exit_if_done(nl - (b0 + LB)); }
#endif
    }
    }
#ifdef MIMSEM_STAMPS
levels_done: ;
#endif
    // NOTE (OWN): an owner-form wavefront whose item ends inside the ring never gets here -- wave_exit_if_done ends it in the loop (the
    // MIMSEM_STAMPS build jumps to the label above instead, for its final stamp).  Everything below is `if constexpr (TILE)` or `!OWN`;
    // code added behind the loop for OWN would run for some wavefronts only: give OWN a real branch out of the ring first.
    // ---- tile mode: the slots the groups of this tile share, from the workgroup's LDS straight into y ----
    if constexpr (TILE) {
        __syncthreads();                                   // every wavefront of the workgroup has stored its pairs (same chunk, same trip counts)
        const int lb0 = (int)ch*a.lch*a.wcpp;
        const int nlv = min(a.nlev - lb0, a.lch*a.wcpp);
        const int4* tf = a.wtfin + (size_t)((g - (unsigned)a.wg0)/4u)*a.wtile;
        for (int idx = threadIdx.x; idx < a.wtile*nlv; idx += 64*NW) {
            const int k = idx%a.wtile, li = idx/a.wtile;
            const int4 r = tf[k];
            if (r.x < 0) continue;
            double v = s_t[li][r.y] + s_t[li][r.z];       // part A + part B: the order of the perimeter pass
            gdouble* yp = (gdouble*)(a.y + (size_t)(lb0 + li)*a.ys + r.x);
            if constexpr (ACCUM) v += *yp;
            *yp = v;
        }
    }
    // ---- finishing phase (round 3): the perimeter slots, inside the same launch ----
    // The partial sums are laid out per SIDE (the <= 16 entries two wave-groups share: their common perimeter slots and the complete
    // slots either of them cannot write as a 16-byte pair; build_wave_plan) in UNCACHED memory: a plain store of the level loop is
    // acknowledged by the memory side.  A wavefront that has all its stores acknowledged adds 1 to the counter of each of its sides;
    // whoever finds the other group's arrival there sums part A + part B in that fixed order -- the same bits whichever of the two
    // finishes, and the same as k_wave_perim's -- and writes the slots of the side for every level of the work item: per 8 entries one
    // 16-byte load and one 8-byte store per lane (64 lanes = 4 entry pairs x 8 levels x 2 parts).  Nobody waits for anybody: a group
    // that arrives first simply leaves.  The finishing wave sets the counter back to 0.  Every y slot is written by exactly one
    // wavefront of the launch (a complete pair by its group, an entry of a side by the side's finisher).
    if (!OWN && a.wfin) {                                  // wave-uniform (the owner-computes form has nothing to finish)
        WSTAMP(11);                                        // chunks done, stores issued
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // (round 4, the fifth way: plain memory + ONE release fence -- buffer_wbl2 sc1, the XCD's dirty lines written back in bulk -- instead of
        //  a coherent access per store; the finisher reads through agent-scope loads as before.  MIMSEM_WAVE_FIN_FENCE=1 MIMSEM_WPART_MEM=plain)
        if (a.wfence) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        WSTAMP(12);                                        // own stores acknowledged
        const int4 wf = a.wfin[(size_t)g*8 + (lane & 7)];  // {side, arrivals that complete it, entries of the side, 0}
        int* const cp = a.wcnt + ((size_t)max(wf.x, 0)*nchunk + ch);
        int old = -2;
        if (lane < 8 && wf.x >= 0) old = __hip_atomic_fetch_add(cp, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool won = lane < 8 && wf.x >= 0 && old == wf.y - 1;
        if (won) __hip_atomic_store(cp, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned long long wm = __ballot(won);
        WSTAMP(13);                                        // arrival counted
        const int fl = (lane >> 2) & 7, ab = lane >> 5;
        const int l0 = (int)ch*a.lch*a.wcpp;
        while (wm) {                                       // wave-uniform: the sides this wave finishes
            const int k = __builtin_ctzll(wm); wm &= wm - 1;
            const int sid = __builtin_amdgcn_readlane(wf.x, k), need = __builtin_amdgcn_readlane(wf.y, k), nent = __builtin_amdgcn_readlane(wf.z, k);
            for (int j0 = 0; j0 < nent; j0 += 8) {         // wave-uniform
                const int j = j0 + 2*(lane & 3);           // entry pair of this lane
                const int slot = a.wsslot[(size_t)sid*16 + j + ab];
                const double* prt = a.out + (size_t)sid*32 + ab*16 + j;
                for (int cc = 0; cc < a.wcpp; cc++) {
                    const int lev = l0 + cc*a.lch + fl;
                    const bool ok = fl < a.lch && lev < a.nlev;
                    double2 v = load_pair_agent(prt + (size_t)(ok ? lev : l0)*a.os);
                    if (need == 1 && ab == 1) { v.x = 0.0; v.y = 0.0; }            // a side of the group's own: nobody writes part B
                    const double ox = __shfl_xor(v.x, 32), oy = __shfl_xor(v.y, 32);
                    double val = ab ? oy + v.y : v.x + ox;                          // part A + part B (lanes 32.. hold B)
                    if (ok && slot >= 0) {
                        double* yp = a.y + (size_t)lev*a.ys + slot;
                        if constexpr (ACCUM) val += *yp;
                        *yp = val;
                    }
                }
            }
        }
        WSTAMP(14);                                        // sides finished (stores issued)
    }
#ifdef MIMSEM_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    WSTAMP(15);                                          // stores acknowledged
#endif
}

// own4::k_apply_wave<3, UMAT, 8, ACCUM>: the owner-computes form of k_apply_wave<3, UMAT, 8, ACCUM, false, true> with ONE ghost pass per
// FOUR levels (build_wave_own, gh4).  The packed pass above lays two levels out as x-normal | y-normal rows, each with room for 4
// sides, but a group has at most 4 ghost sides in all: half of its lanes idle.  Here ghost side b IS DPP row b and the row's other
// direction holds the four levels m of a double batch (x-normal: qx = m, qy = point; y-normal: qy = m, qx = point), so the point along
// the side still sits where the element keeps that point's coefficients and every slot comes out of the fma sequence above -- the
// same bits.  The pass runs at the EVEN batches of the ring, for the batch being computed and the next one: the next batch's gathered
// DoFs are staged one batch early (their wait moves with them), a lane of the second batch (m >= 2) keeps its result in a register
// and puts it into its level's strip in the next batch's result phase; the lanes with nothing to put write to a dump position.  An
// item with an odd number of batches runs its last pass half empty, on the clamped loads of the batch it does not have.  Everything
// else -- the element's algebra, the level pipeline, the stores, the exits -- is the kernel above, written out for its one case.
namespace own4 {
// LIST: the item is read from the planned list a.witems (wave_balance.hpp: balanced level ranges) -- its own entry point,
// k_apply_wave_list, so that the kernel of the default rule keeps its prologue of one wait for the kernel arguments.
template <int N, int OP, int LCT, bool ACCUM, bool LIST>
__device__ __forceinline__ void apply_wave_body(const ElemArgs& a) {
    using D = Dims<N>;
    static_assert(N == 3 && OP == MIMSEM_OP_UMAT && LCT == 8 && MIMSEM_WLB == 2 && MIMSEM_WAHEAD == 2, "owner-computes Umat at p = 3, rings of four batches of two levels");
    constexpr int LPE = D::LPE, EPW = 64/LPE, ND = 2*D::n1e, NW = WNW;
    constexpr int NACC = EPW*ND, ZERO = NACC + 128;
    constexpr int RS = D::mp1 + (D::mp1 & 1);
    constexpr int XT = D::n1e + D::mp1*RS;
    constexpr int SXE = XT + 2*(LPE - D::n1e) + ((XT + 2*(LPE - D::n1e)) & 1);
    constexpr int WGR = NACC + 136;                      // the ghost results of a level, side*4 + point; behind them 16 dump positions
    constexpr int SW = (EPW*SXE > WGR + 32) ? EPW*SXE : WGR + 32;
    constexpr int LB = 2, AHEAD = 2, WGX = MIMSEM_WGX;
    static_assert(LPE == 16 && EPW == 4 && ZERO >= EPW*SXE && ZERO < SW, "an element is one DPP row; the zero entry lies beyond the staged x and the results");
    __shared__ double sE[NW][D::mp1*N];
    __shared__ double s_x[NW][LB][SW];
    __shared__ __attribute__((aligned(16))) double s_g[NW][2*LB][WGX];      // the gathered ghost DoFs of the four levels of a pass

    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63, el = lane/LPE, q = lane%LPE;
    const unsigned nchunk = (unsigned)a.wnp;
    const unsigned nitems = LIST ? (unsigned)a.wnitems : (unsigned)a.wgroups*nchunk;
    const unsigned bid = xcd_swizzle(blockIdx.x, gridDim.x, a.swz & 1);
    const unsigned item = bid*NW + (unsigned)wv;
    const int4* const wit = a.witems;
    if constexpr (LIST) asm volatile("" :: "s"(wit));    // (the list's address arrives with the other kernel arguments, not behind the exit below)
    if (item >= nitems) return;                          // wave-uniform
    unsigned g;
    int lbeg, lend_;
    if constexpr (LIST) {                                // a planned item {group, first level, end level, 0}: its first three ints, by scalar loads
        typedef const __attribute__((address_space(4))) int cint;        // (constant address space: a scalar load whatever stands before it)
        cint* const it = (cint*)(unsigned long long)(wit + item);
        g = (unsigned)it[0]; lbeg = it[1]; lend_ = it[2];
    } else {
        // item = quotient*dv + rest without a division: a.wcpp carries floor((2^32 - 1)/dv) (dispatch_apply_wave), whose high product
        // is the quotient or one less for every 32-bit item -- one wave-uniform correction makes it exact
        const bool gmaj = (a.swz & 2) != 0;              // group-major: the parts of a group are neighbours
        const unsigned dv = gmaj ? nchunk : (unsigned)a.wgroups;
        unsigned qt = __umulhi(item, (unsigned)a.wcpp), rs = item - qt*dv;
        if (rs >= dv) { qt++; rs -= dv; }
        const unsigned ch = gmaj ? rs : qt;
        g = (gmaj ? qt : rs) + (unsigned)a.wg0;
        lbeg = 2*((int)ch*a.wpb + min((int)ch, a.wpr));
        lend_ = min(a.nlev, lbeg + 2*(a.wpb + ((int)ch < a.wpr ? 1 : 0)));
    }
    const int lend = lend_;
#ifdef MIMSEM_STAMPS
    const int lbeg0 = lbeg;
#define WSTAMP4(k) do { if constexpr (!LIST) WSTAMP(k); } while (0)      // (the stamps have a slot per item of the default rule)
#else
#define WSTAMP4(k) do { } while (0)
#endif
    WSTAMP4(0);                                          // entry: the item is known
    const int4 wl = a.wlane[(size_t)g*64 + lane];
    const int4 wp = a.wplan[(size_t)g*64 + lane];
    const int4 gh = a.wgh4[(size_t)g*64 + lane];
    const int gxs = a.wgx[(size_t)g*64 + lane];
    // the group's tables are REQUESTED; the rows' start addresses are formed under them (from `lbeg` as it stands behind this line)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" : "+s"(lbeg));
    WSTAMP4(2);                                          // tables requested
    const double2* hp = (const double2*)(a.wG + (size_t)gh.x*4);
    const double2 h01 = hp[0], h23 = hp[1];
    const bool gyn = (gh.z & 1) != 0, gsz = (gh.z & 4) != 0, gidle = (gh.z & 8) != 0;
    const int gc0 = (gh.z & 2) ? 3 : 0;
    const int gm = gyn ? (lane >> 2) & 3 : lane & 3;     // the ghost lane's level of the double batch
    const unsigned gxo = 8u*(unsigned)gxs;
    // thickInv of the ghost lane: its level's half of a pair; a lane of the second batch takes the NEXT pair row (same parity, the
    // batch's first level + 2) -- only where the call has that level: otherwise it stays on the first batch's row, for nothing
    const unsigned tgo = 16u*(unsigned)gh.y + 8u*(unsigned)(gm & 1), ghi = gm >= 2 ? 0xFFFFFFFFu : 0u;
    const double2* gp = (const double2*)(a.wG + ((size_t)g*64 + lane)*4);
    const double2 g01 = gp[0], g23 = gp[1];
    const double gaa = a.scale*g01.x, gab = a.scale*g01.y, gbb = a.scale*g23.x;
    const int e = wl.x;
    const int qx = q%D::mp1, qy = q/D::mp1;
    const unsigned gq = (unsigned)e*D::mp12 + (unsigned)q;
    const unsigned xo = 8u*(unsigned)wl.y;
    const unsigned to = 16u*gq;
    double2 px[LCT]; double pt0[LCT], pg[LCT], ptg[LCT/(2*LB)];
    // The batches are requested in level order, two levels further each time, so the rows are STEPPED, not computed: wave-uniform
    // byte pointers to the next x row and the next thickInv pair row, set here once.  A level l stands for min(l, nlev - 1) (beyond
    // the last level: re-read it -- a valid address; nothing is stored for it): `ahead` counts the levels from the next batch's first
    // to the call's last, an x row moves on while a level is left and stays otherwise, a pair row (whose parity the step of two
    // keeps) moves on while two are left and otherwise becomes the last level's row -- that one may be of the other parity.
    const auto tip_row = [&](int l) { const int L = a.lev0 + l; return (const char*)(a.tIp + ((size_t)(L & 1)*a.tnp + (size_t)(L >> 1))*(size_t)a.tps); };
    const char* xrow = (const char*)(a.x + (size_t)min(lbeg, a.nlev - 1)*a.xs);
    const char* trow = tip_row(min(lbeg, a.nlev - 1));
    const char* const tlast = tip_row(a.nlev - 1);
    const long long xsb = 8*a.xs, tpb = 8*a.tps;
    int ahead = a.nlev - 1 - lbeg;
    auto load_batch = [&](int r0) {
        const bool two = ahead >= 2;                         // wave-uniform: the call has the level two beyond this batch's first
        {
            const double2 tp = WLOAD(double2, trow + to);
            pt0[r0] = tp.x; pt0[r0 + 1] = tp.y;
            if ((r0/LB)%2 == 0) {                            // ONE load per ghost pass
                const unsigned nx = two ? (unsigned)tpb : 0u;
                ptg[r0/(2*LB)] = *(const double*)(trow + (tgo + (ghi & nx)));
            }
            trow = two ? trow + tpb : tlast;
        }
#pragma unroll
        for (int i = 0; i < LB; i++) {
            const int r = r0 + i;
            px[r] = WLOAD(double2, xrow + xo);
            pg[r] = *(const double*)(xrow + gxo);
            xrow += ahead >= 1 + i ? xsb : 0;
        }
        ahead -= LB;
    };
#pragma unroll
    for (int b = 0; b < AHEAD; b++) { load_batch(b*LB); __builtin_amdgcn_sched_barrier(0); }   // in THIS order: vmcnt is in-order
    WSTAMP4(3);                                          // level loads issued
    {
        double* se = sE[wv];
#pragma unroll
        for (int k = 0; k < D::mp1*N; k++) se[k] = a.Etab[k];
    }
    wave_fence();

    // ---- level-invariant registers (as above) ----
    const bool vert = (a.flags & MIMSEM_FLAG_VERT) != 0;
    double Ex[N];
#pragma unroll
    for (int j = 0; j < N; j++) Ex[j] = sE[wv][qx*N + j];
    double cu[4], cp[4], pq[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {                        // every entry is READ, at a clamped index, and the unused ones are then replaced
        const int j = (qy - k) & 3;                      // by +0.0: selects, so that the LDS reads go out together (no exec-mask regions)
        const double eu = sE[wv][qy*N + min(j, 2)], ep = a.alpha*sE[wv][j*N + min(qy, 2)], eq = a.alpha*sE[wv][k*N + min(qx, 2)];
        cu[k] = j < 3 ? eu : 0.0;
        cp[k] = qy < 3 ? ep : 0.0;
        pq[k] = qx < 3 ? eq : 0.0;
    }
    double kc[3];
    const double hgaa = a.scale*h01.x, hgab = a.scale*h01.y, hgbb = a.scale*h23.x;
    const double gm0 = gyn ? hgab : hgaa, gm1 = gyn ? hgbb : hgab;
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const int tt = !gyn ? t : (gc0 == 0 ? (t == 0 ? 0 : 3 - t) : 2 - t);
        kc[t] = sE[wv][gc0*N + tt];
    }
    const double* const sgl = &s_g[wv][gm][gh.w & 0xFF];  // the ghost lane's quadruple {cross 0, cross 1, cross 2, side DoF} at its level
    // where its result goes: WGR + side*4 + point of its level's strip -- in the pass's own batch (m < 2) or in the next one (m >= 2);
    // in the other of the two, and on an idle lane in both, a dump position behind the results
    double* const sdump = &s_x[wv][(lane >> 5) & 1][WGR + 16 + (lane & 15)];
    double* const sgr0 = (!gidle && gm < 2) ? &s_x[wv][gm & 1][WGR + (gh.w >> 8)] : sdump;
    double* const sgr1 = (!gidle && gm >= 2) ? &s_x[wv][gm & 1][WGR + (gh.w >> 8)] : sdump;
    const int xd00 = wl.z & 0xFFFF, xd01 = (wl.z >> 16) & 0xFFFF, xd10 = wl.w & 0xFFFF, xd11 = (wl.w >> 16) & 0xFFFF;
    const bool hasx = q < D::n1e;
    const int aci0 = hasx ? el*ND + q : NACC + lane;
    const int aci1 = qx < 3 ? el*ND + D::n1e + qy*3 + qx : NACC + 64 + lane;
    const int ldx = q < D::n1e ? q : 0, ldy = D::n1e + qy*RS + (qx < 3 ? qx : 0);
    const bool okx = q < D::n1e, oky = qx < 3;
    const int wp00 = wp.y & 0xFFFF, wp01 = (wp.y >> 16) & 0xFFFF, wp10 = wp.z & 0xFFFF, wp11 = (wp.z >> 16) & 0xFFFF;
    const bool wy = wp.x >= 0;
    // (both rows are wave-uniform: two scalar candidates and a select per lane, not a branch around each row's arithmetic)
    const unsigned long long wyr = (unsigned long long)(a.y + (size_t)lbeg*a.ys), wor = (unsigned long long)(a.out + (size_t)lbeg*a.os);
    gchar* wo = (gchar*)((wy ? wyr : wor) + 8ull*(unsigned long long)(long long)(wy ? wp.x : -wp.x - 2));
    const long long wst = 8*(wy ? a.ys : a.os);
#pragma unroll
    for (int i = 0; i < LB; i++) s_x[wv][i][ZERO] = 0.0;
    gchar* const dumpp = (gchar*)(a.out + a.wdump + 2*lane);
    double gkeep = 0.0;                                  // the ghost result of a lane of the pass's second batch
    for (; lbeg < lend; lbeg += LCT) {                   // wave-uniform: one trip = the ring of LCT levels
    const int nl = lend - lbeg;
#pragma unroll
    for (int b0 = 0; b0 < LCT; b0 += LB) {
        const bool pass = (b0/LB)%2 == 0;                // (unrolled: a constant)
        __builtin_amdgcn_sched_barrier(0);
        load_batch((b0 + AHEAD*LB)%LCT);                 // (the levels lbeg + b0 + AHEAD*LB ...: the stepped rows stand there)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < LB; i++) {
            double* st = s_x[wv][i];
            st[xd00] = px[b0 + i].x; st[xd01] = px[b0 + i].x; st[xd10] = px[b0 + i].y; st[xd11] = px[b0 + i].y;
        }
        if (pass) {
#pragma unroll
            for (int i = 0; i < 2*LB; i++) s_g[wv][i][lane] = pg[b0 + i];
        }
        wave_fence();
        double yxr[LB], yyr[LB];
#pragma unroll
        for (int i = 0; i < LB; i++) {
            const int l = b0 + i;
            const double* sx = s_x[wv][i] + el*SXE;
            double X = sx[ldx], Y = sx[ldy];
            if (!okx) X = 0.0;
            if (!oky) Y = 0.0;
            const double u = dpp_rows(cu, X);
            const double v = dpp_quad<3>(Ex, Y);
            const double fac = vert ? pt0[l] : 1.0;
            const double ra = fac*fma(gab, v, gaa*u), rb = fac*fma(gbb, v, gab*u);
            yxr[i] = dpp_rows(cp, ra); yyr[i] = dpp_quad<4>(pq, rb);
        }
        double gyr = 0.0;
        if (pass) {                                       // the ghost pass: every side point of four levels at once
            const double2 c01 = *(const double2*)sgl, c2s = *(const double2*)(sgl + 2);
            const double S = gsz ? 0.0 : c2s.y;
            double C = fma(kc[0], c01.x, gyn ? 0.0 : -0.0);
            C = fma(kc[1], c01.y, C);
            C = fma(kc[2], c2s.x, C);
            const double Ar = dpp_rows(cu, S), Aq = dpp_quad<3>(Ex, S);
            const double gu_ = gyn ? C : Ar, gv_ = gyn ? Aq : C;
            const double gf = vert ? ptg[b0/(2*LB)] : 1.0;
            const double gr = gf*fma(gm1, gv_, gm0*gu_);
            const double Pr = dpp_rows(cp, gr), Pq = dpp_quad<4>(pq, gr);
            gyr = gyn ? Pq : Pr;
        }
        wave_fence();
#pragma unroll
        for (int i = 0; i < LB; i++) { double* sacc = s_x[wv][i]; sacc[aci0] = yxr[i]; sacc[aci1] = yyr[i]; }
        if (pass) { *sgr0 = gyr; gkeep = gyr; }
        else *sgr1 = gkeep;
        wave_fence();
#pragma unroll
        for (int i = 0; i < LB; i++) {
            const int l = b0 + i;
            const double* sacc = s_x[wv][i];
            double2 val;
            val.x = sacc[wp00] + sacc[wp01]; val.y = sacc[wp10] + sacc[wp11];
            gdouble* o = (gdouble*)(l < nl ? wo : dumpp);
            if constexpr (ACCUM) { double o0 = o[0], o1 = o[1]; if (!wy) { o0 = 0.0; o1 = 0.0; } val.x += o0; val.y += o1; }
            // y is the one stream nobody in the launch reads back (ACCUM reads a pair before it stores it, with the default policy): its
            // 16-byte store is NON-TEMPORAL -- still ONE global_store_dwordx4 per level.  Measured (profiles/umat_store_policy_ab.txt,
            // _pmc.txt): the launch's trace 12.5 -> 11.9 us, 8 spheres out of cache 87 -> 78 us, FETCH_SIZE -5 %, WRITE_SIZE +10 %.  x, the
            // gathers and thickInv keep the default policy: thickInv as `nt` costs 3 us per launch.
            { wave_d2 vv; vv.x = val.x; vv.y = val.y; __builtin_nontemporal_store(vv, (gwave_d2*)o); }
            wo += wst;
        }
        wave_fence();
#ifdef MIMSEM_STAMPS
        if (4 + (lbeg - lbeg0 + b0)/LB < 11) WSTAMP4(4 + (lbeg - lbeg0 + b0)/LB);      // batch computed, its stores issued (the first seven)
#endif
        if (b0 + LB < LCT) wave_exit_if_done(nl - (b0 + LB));     // (nothing follows the level loop: see wave_exit_if_done)
    }
    }
}
template <int N, int OP, int LCT, bool ACCUM>
__global__ __launch_bounds__(64*WNW) __attribute__((amdgpu_waves_per_eu(3, 8))) void k_apply_wave(ElemArgs a) { apply_wave_body<N, OP, LCT, ACCUM, false>(a); }
template <int N, int OP, int LCT, bool ACCUM>
__global__ __launch_bounds__(64*WNW) __attribute__((amdgpu_waves_per_eu(3, 8))) void k_apply_wave_list(ElemArgs a) { apply_wave_body<N, OP, LCT, ACCUM, true>(a); }
#undef WSTAMP4
}  // namespace own4

// k_apply_wave2<OP, LCT, ACCUM>: the 2-form-valued operators at p = 3 -- Wmat, Whmat (2-form in), WtQUmat, WtQdUdz_mat (1-form in, 1-form
// coefficient field; eul/Assembly.cpp:330-360, 1262-1290, 940-1000, 1585-1640) -- on the same footing as k_apply_wave: one wavefront per
// (wave-group of 2 x 2 elements, chunks of 8 levels), the packed metric record, the level pipeline, a branch-free body, and ALL of the
// element's algebra through DPP (an element = one DPP row): faces are never shared, so there is no scatter, no plan and no second
// pass; Wmat / Whmat touch LDS only for the basis table, WtQUmat additionally to stage its two gathered 1-forms (16-byte slot pairs).
//   coefficient at a point, from the record G = Q/det J^T J and 1/det (the reference's expressions regrouped):
//     Wmat     c = scale Q/det [tI]                       a = c u
//     Whmat    c = scale Q/det tI (f/det [tI])            a = c u
//     WtQUmat  a = 1/2 tI^2 scale/det ((gaa fu + gab fv) u + (gab fu + gbb fv) v)      (f = the velocity that weights, u = the one applied to)
//     WtQdUdz  a =            scale/det ((gaa fu + gab fv) u + (gab fu + gbb fv) v)
template <int OP, int LCT, bool ACCUM>
__global__ __launch_bounds__(64*WNW) __attribute__((amdgpu_waves_per_eu(3, 8))) void k_apply_wave2(ElemArgs a) {
    constexpr int N = 3;
    using D = Dims<N>;
    using T = OpTraits<OP>;
    static_assert(T::out == S2 && !T::up, "2-form-valued operators");
    constexpr bool IN1 = (T::in == S1);                  // WtQUmat family: two gathered 1-forms
    constexpr int LPE = 16, EPW = 4, NW = WNW;
    constexpr int RS = D::mp1 + (D::mp1 & 1), XT = D::n1e + D::mp1*RS;
    constexpr int SXE = XT + 2*(LPE - D::n1e) + ((XT + 2*(LPE - D::n1e)) & 1);
    constexpr int SW = EPW*SXE + 8;
    constexpr int LB = LCT >= 2 ? 2 : LCT;
    __shared__ double sE[NW][D::mp1*N];
    __shared__ double s_x[IN1 ? NW : 1][IN1 ? LB : 1][IN1 ? 2 : 1][IN1 ? SW : 1];     // staged x and f of a level (WtQUmat family)

    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63, el = lane/LPE, q = lane%LPE;
    const unsigned nchunk = ((unsigned)((a.nlev + a.lch - 1)/a.lch) + (unsigned)a.wcpp - 1)/(unsigned)a.wcpp;
    const unsigned nitems = (unsigned)a.wgroups*nchunk;
    const unsigned bid = xcd_swizzle(blockIdx.x, gridDim.x, a.swz & 1);
    const unsigned item = bid*NW + (unsigned)wv;
    if (item >= nitems) return;
    unsigned g, ch;
    if (a.swz & 2) { g = item/nchunk; ch = item%nchunk; }
    else           { g = item%(unsigned)a.wgroups; ch = item/(unsigned)a.wgroups; }
    g += (unsigned)a.wg0;
    int lbeg = (int)ch*a.lch*a.wcpp;
    const int4 wl = a.wlane[(size_t)g*64 + lane];
    const double2* gp = (const double2*)(a.wG + ((size_t)g*64 + lane)*4);
    const double2 g01 = gp[0], g23 = gp[1];
    const int e = wl.x;
    const int qx = q%4, qy = q/4;
    const double rdet = g23.y;                           // 0 for the lanes of a padding element (their metric record is zero): they store nothing
    const bool okf = qx < 3 && qy < 3 && rdet != 0.0, okx = q < D::n1e, oky = qx < 3;
    const unsigned gq = (unsigned)e*D::mp12 + (unsigned)q;
    const int ff = okf ? qy*3 + qx : 0;                                          // the lane's face of the element
    const unsigned fo2 = 8u*(unsigned)(a.i2 ? a.i2[e*D::n2e + ff] : e*D::n2e + ff);
    const unsigned xo = 8u*(unsigned)wl.y;                                       // WtQUmat family: the lane's load pair
    // level loads first (they need the lane table only), the set-up of the level-invariant registers under them: as in k_apply_wave
    double px[IN1 ? LCT : 1][2], pf[IN1 ? LCT : 1][2], ps[IN1 ? 1 : LCT], pf0[(OP == MIMSEM_OP_WHMAT) ? LCT : 1], pt0[LCT];
    const size_t lstride = (size_t)a.nEl*D::mp12;
    auto load_batch = [&](int r0, int lev0_) {
#pragma unroll
        for (int i = 0; i < LB; i++) {
            const int r = r0 + i;
            const int lev = min(lev0_ + i, a.nlev - 1);
            if constexpr (IN1) {
                const double2 vx = *(const double2*)((const char*)(a.x + (size_t)lev*a.xs) + xo);
                const double2 vf = *(const double2*)((const char*)(a.f + (size_t)lev*a.fs) + xo);
                px[r][0] = vx.x; px[r][1] = vx.y; pf[r][0] = vf.x; pf[r][1] = vf.y;
            } else {
                ps[r] = *(const double*)((const char*)(a.x + (size_t)lev*a.xs) + fo2);
                if constexpr (OP == MIMSEM_OP_WHMAT) pf0[r] = *(const double*)((const char*)(a.f + (size_t)lev*a.fs) + fo2);
            }
            pt0[r] = *(const double*)((const char*)(a.tI + (size_t)(a.lev0 + lev)*lstride) + 8u*gq);
        }
    };
    constexpr int AHEAD = (LCT/LB > 2) ? 2 : (LCT/LB > 1 ? 1 : 0);
#pragma unroll
    for (int b = 0; b < (AHEAD ? AHEAD : 1); b++) { load_batch(b*LB, lbeg + b*LB); __builtin_amdgcn_sched_barrier(0); }
    {
        double* se = sE[wv];
#pragma unroll
        for (int k = 0; k < D::mp1*N; k++) se[k] = a.Etab[k];
    }
    wave_fence();
    const bool vert = (a.flags & MIMSEM_FLAG_VERT) != 0;
    const double gaa = g01.x, gab = g01.y, gbb = g23.x;
    // GLL weights sit in SGPRs (kernel arguments): selects, not an indexed load
    const double wx = qx == 0 ? a.Wq[0] : (qx == 1 ? a.Wq[1] : (qx == 2 ? a.Wq[2] : a.Wq[3]));
    const double wy_ = qy == 0 ? a.Wq[0] : (qy == 1 ? a.Wq[1] : (qy == 2 ? a.Wq[2] : a.Wq[3]));
    const double c0 = a.scale*(wx*wy_)*rdet;                                     // Wmat family: scale Q / det
    double Ex[3], cu[4], cp[4], pq[4];
#pragma unroll
    for (int j = 0; j < 3; j++) Ex[j] = sE[wv][qx*N + j];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = (qy - k) & 3;
        cu[k] = j < 3 ? sE[wv][qy*N + j] : 0.0;                                  // interpolation along y
        cp[k] = qy < 3 ? a.alpha*sE[wv][j*N + qy] : 0.0;                         // projection along y (alpha folded in once)
        pq[k] = qx < 3 ? sE[wv][k*N + qx] : 0.0;                                 // projection along x
    }
    const int xd00 = wl.z & 0xFFFF, xd01 = (wl.z >> 16) & 0xFFFF, xd10 = wl.w & 0xFFFF, xd11 = (wl.w >> 16) & 0xFFFF;
    const int ldx = el*SXE + (okx ? q : 0), ldy = el*SXE + D::n1e + qy*RS + (oky ? qx : 0);
    gchar* wo = (gchar*)(a.out + (size_t)lbeg*a.os) + fo2;
    const long long wst = 8*a.os;
    gchar* const dumpp = (gchar*)(a.y + lane);           // a.y: the workspace (dump for lanes without a face and for a ragged last chunk)

    for (int cc = 0; cc < a.wcpp; cc++, lbeg += a.lch) {
    const int nl = min(a.nlev - lbeg, a.lch);
    if (nl <= 0) break;
#pragma unroll
    for (int b0 = 0; b0 < LCT; b0 += LB) {
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (AHEAD > 0) load_batch((b0 + AHEAD*LB)%LCT, lbeg + b0 + AHEAD*LB);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (IN1) {
#pragma unroll
            for (int i = 0; i < LB; i++) {
                double* sx = s_x[wv][i][0]; double* sf = s_x[wv][i][1];
                sx[xd00] = px[b0 + i][0]; sx[xd01] = px[b0 + i][0]; sx[xd10] = px[b0 + i][1]; sx[xd11] = px[b0 + i][1];
                sf[xd00] = pf[b0 + i][0]; sf[xd01] = pf[b0 + i][0]; sf[xd10] = pf[b0 + i][1]; sf[xd11] = pf[b0 + i][1];
            }
            wave_fence();
        }
#pragma unroll
        for (int i = 0; i < LB; i++) {
            const int l = b0 + i;
            const double tI = pt0[l];
            double aq;
            if constexpr (IN1) {
                double X = s_x[wv][i][0][ldx], Y = s_x[wv][i][0][ldy], FX = s_x[wv][i][1][ldx], FY = s_x[wv][i][1][ldy];
                if (!okx) { X = 0.0; FX = 0.0; }
                if (!oky) { Y = 0.0; FY = 0.0; }
                const double u = dpp_rows(cu, X), v = dpp_quad<3>(Ex, Y);        // Geom::interp1_l of the applied field
                const double fu = dpp_rows(cu, FX), fv = dpp_quad<3>(Ex, FY);    // ... and of the weighting velocity
                const double t0 = fma(gab, fv, gaa*fu), t1 = fma(gbb, fv, gab*fu);
                const double s2 = fma(t1, v, t0*u);
                if constexpr (OP == MIMSEM_OP_WTQUMAT) aq = ((0.5*a.scale*rdet)*(tI*tI))*s2;
                else aq = (a.scale*rdet)*s2;
            } else {
                double X = okf ? ps[l] : 0.0;
                const double u = dpp_rows(cu, dpp_quad<3>(Ex, X));               // Geom::interp2_l
                if constexpr (OP == MIMSEM_OP_WMAT) aq = (c0*(vert ? tI : 1.0))*u;
                else {
                    double F = okf ? pf0[l] : 0.0;
                    double p = dpp_rows(cu, dpp_quad<3>(Ex, F))*rdet;
                    if (vert) p *= tI;
                    aq = ((p*c0)*tI)*u;
                }
            }
            const double y2 = dpp_rows(cp, dpp_quad<4>(pq, aq));                 // W^T: x direction in the quad, y direction over the rows
            gdouble* o = (gdouble*)((okf && l < nl) ? wo : dumpp);
            if constexpr (ACCUM) *o = *o + y2; else *o = y2;
            wo += wst;
        }
        if constexpr (IN1) wave_fence();
    }
    }
}

// Perimeter pass of the wave-level form: y[slot] = (+=) the one or two partial sums the wave-groups left for it.  One thread per slot
// and chunk of PLC levels; the slot's record {slot, p0, p1} is one 16-byte load, every level's partials are requested before the
// first is used (branch-free: a missing second partial re-reads the first and is masked out), stores follow.
#ifndef MIMSEM_PLC
#define MIMSEM_PLC 8
#endif
constexpr int PLC = MIMSEM_PLC;     // levels per thread of the perimeter pass
template <bool ACCUM>
__global__ __launch_bounds__(256) void k_wave_perim(const double* __restrict__ yp, long long yps, const int4* __restrict__ rec, int nps,
                                                    int nlev, double* __restrict__ y, long long ys) {
    const int i = blockIdx.x*256 + threadIdx.x;
    if (i >= nps) return;
    const int4 r = rec[i];
    const bool has0 = r.y >= 0, has1 = r.z >= 0;
    const unsigned o0 = 8u*(unsigned)(has0 ? r.y : 0), o1 = 8u*(unsigned)(has1 ? r.z : (has0 ? r.y : 0));
    const int l0 = blockIdx.y*PLC;
    double a0[PLC], a1[PLC], old[ACCUM ? PLC : 1];
#pragma unroll
    for (int l = 0; l < PLC; l++) {
        const int lev = min(l0 + l, nlev - 1);
        const char* src = (const char*)(yp + (size_t)lev*yps);
        a0[l] = *(const double*)(src + o0); a1[l] = *(const double*)(src + o1);
        if constexpr (ACCUM) old[l] = y[(size_t)lev*ys + r.x];
    }
#pragma unroll
    for (int l = 0; l < PLC; l++) {
        if (l0 + l < nlev) {
            double acc = has0 ? a0[l] : 0.0;
            if (has1) acc += a1[l];
            if constexpr (ACCUM) acc += old[l];
            y[(size_t)(l0 + l)*ys + r.x] = acc;
        }
    }
}
