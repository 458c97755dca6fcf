// owned_blocks.hip -- the reference's PCBJACOBI: exact inverses of the assembled OWNED diagonal blocks (mimsem_owned_blocks_* of include/mimsem_hip.h).
//
// Reference: every mass solve runs GMRES with PCBJACOBI and PCBJacobiSetTotalBlocks(size*nElsX*nElsX) (ksp1, eul/HorizSolve.cpp:77-96; ksp, ksp0,
// ksp0h, src/SWEqn_Picard.cpp:85-113).  PETSc cuts the global numbering into equal contiguous chunks; with the element-contiguous numbering of the
// 1-forms (mimsem_amd/mesh.py) chunk k is exactly the 2 n^2 edges element k OWNS: its x-edges of columns 0..n-1 and its y-edges of rows 0..n-1 (its
// west and south sides and its interior -- the east and north sides are the neighbours' west / south sides, also across the rotated panel seams of
// the cubed sphere).  Each chunk's block is the diagonal block of the ASSEMBLED matrix; Umat::assemble inserts every element block whole
// (eul/Assembly.cpp:128-131), so the block's pattern is full, ILU(0) drops no fill and the sub-solve is the exact inverse of the block.
//
// Ownership is read off the element tables (the position of a slot inside its element), not off the numbering: row r of block k is the r-th
// smallest slot element k owns -- for the global numbering the chunk's own order.  Per owned row one 16-byte entry {slot, position of the slot in
// the owner's element-local results, position in the other element's (-1: none), 0}: positions e * nde + j index the element-local layout of
// mimsem_op_element_matrices and of the element pass (nde = 2 n1e for 1-forms, n2e for 2-forms).  The 1-form positions are those of the context's
// gather plan, so the block pass of the Chebyshev solve gathers the operator result through them.
//   set-up   k_owned_assemble: block (k, r, c) = the owner's element entry + the other element's entry when both slots are shared with the same
//            neighbour -- a fixed order, no atomics: two builds give the same bits.
//   apply    k_owned_pass<ND, LC, 0>: one (block, chunk of levels) per group of lanes, the lane of row r holds that row of the block in registers
//            (ND <= 64; above: read from memory), x of the block through LDS; every owned slot written exactly once, no gather plan, no partial sums.
//   solve    k_owned_pass<ND, LC, 1|2>: the block pass of a Chebyshev step reads b - A x through the plan, applies B_k^-1 and updates p and x at the
//            block's own slots -- the step is {element pass, owned-block pass}: two launches where the element-block form needs three.
#include <algorithm>
#include <vector>
#include <hip/hip_runtime.h>
#include "ctx.hpp"
#include "../../include/mimsem_hip.h"

namespace {

struct OwnedArgs {
    int nEl, nlev, lch;
    const int4* plan;                                  // [nEl][ND] {slot, owner position, other position, 0}
    const double* B; long long bls;                    // inverse blocks, row-major [nEl][ND][ND] per level, bls doubles apart (0: shared)
    const double* x; long long xs;                     // apply: input
    double* y; long long ys;                           // apply: output
    const double* ye; long long yes;                   // solve: element-local operator results
    const double* b; long long bs;                     // solve: right-hand side
    double* p; long long ps;                           // solve: direction
    double* xo; long long xos;                         // solve: iterate
    double* upd; long long us;                         // solve: z (may be null)
    double alpha, beta;
};

__device__ __forceinline__ void owned_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// one entry of an assembled owned block: out[(k*ND + r)*ND + c], from the element matrices of ONE level (form 1: [nEl][4][n1e][n1e] =
// UtQU UtQV VtQU VtQV; form 2: [nEl][n2e][n2e])
__global__ __launch_bounds__(256) void k_owned_assemble(long long total, int nd, int form, int n1e, int nde, const int4* __restrict__ plan,
                                                        const double* __restrict__ em, double* __restrict__ out) {
    const long long t = (long long)blockIdx.x*256 + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t%nd); const long long kr = t/nd; const int r = (int)(kr%nd); const long long k = kr/nd;
    const int4 tr = plan[k*nd + r], tc = plan[k*nd + c];
    const int qr[2] = {tr.y, tr.z}, qc[2] = {tc.y, tc.z};
    const long long esz = form == 1 ? 4LL*n1e*n1e : (long long)nde*nde;
    double v = 0.0;
    for (int i = 0; i < 2; i++) {                      // the owner's entry first, then the neighbour's
        if (qr[i] < 0) continue;
        const int e = qr[i]/nde, la = qr[i]%nde;
        for (int j = 0; j < 2; j++) {
            if (qc[j] < 0 || qc[j]/nde != e) continue;
            const int lb = qc[j]%nde;
            const double* E = em + (size_t)e*esz;
            v += form == 1 ? E[(((la/n1e)*2 + lb/n1e)*n1e + la%n1e)*n1e + lb%n1e] : E[(size_t)la*nde + lb];
        }
    }
    out[t] = v;
}

// KIND 0: y = B_k x at the block's slots.  KIND 1: z = B_k (b - gather(ye)), p = z + beta p, x += alpha p.  KIND 2: the first step of a solve from
// x = 0 (operator result zero, nothing read but b): z = B_k b, p = z, x = alpha z.
template <int ND, int LC, int KIND>
__global__ __launch_bounds__(256) void k_owned_pass(OwnedArgs a) {
    constexpr int LPE = ND <= 16 ? 16 : (ND <= 32 ? 32 : 64), EPB = 256/LPE, RPL = (ND + LPE - 1)/LPE;
    constexpr bool REG = RPL == 1;                     // block rows in registers up to 64 rows (orders <= 5 of the 1-forms)
    __shared__ double s_x[2][EPB][RPL*LPE];
    const int tid = threadIdx.x, el = tid/LPE, lane = tid%LPE;
    const int nchunk = (a.nlev + a.lch - 1)/a.lch;
    const long long item = (long long)blockIdx.x*EPB + el;
    const bool eact = item < (long long)a.nEl*nchunk;
    const int k = eact ? (int)(item%a.nEl) : 0;
    const int l0 = eact ? (int)(item/a.nEl)*a.lch : 0, l1 = eact ? min(a.nlev, l0 + a.lch) : 0;
    bool act[RPL]; int slot[RPL], q0[RPL], q1[RPL];
#pragma unroll
    for (int j = 0; j < RPL; j++) {
        const int r = lane + j*LPE;
        act[j] = eact && r < ND;
        const int4 t = act[j] ? a.plan[(size_t)k*ND + r] : make_int4(0, -1, -1, 0);
        slot[j] = t.x; q0[j] = t.y; q1[j] = t.z;
    }
    const double* Bk = a.B + (size_t)l0*a.bls + (size_t)k*ND*ND;      // (a level stride forces chunks of one level: l0 is THE level)
    double brow[REG ? ND : 1];
    if constexpr (REG) {
        const double* Br = Bk + (size_t)(act[0] ? lane : 0)*ND;        // (idle lanes: a row of the block in range)
#pragma unroll
        for (int c = 0; c < ND; c++) brow[c] = act[0] ? Br[c] : 0.0;
    }
    // every level of the chunk requested before the first is used; idle lanes and levels past the chunk read clamped addresses
    double v[LC][RPL];
#pragma unroll
    for (int l = 0; l < LC; l++) {
        const int lev = min(l0 + l, max(a.nlev - 1, 0));
#pragma unroll
        for (int j = 0; j < RPL; j++) {
            if constexpr (KIND == 0) v[l][j] = a.x[(size_t)lev*a.xs + slot[j]];
            else {
                double acc = 0.0;
                if constexpr (KIND == 1) {
                    const double* src = a.ye + (size_t)lev*a.yes;
                    const double y0 = src[q0[j] >= 0 ? q0[j] : 0], y1 = src[q1[j] >= 0 ? q1[j] : 0];
                    if (act[j] && q0[j] >= 0) acc += y0;
                    if (act[j] && q1[j] >= 0) acc += y1;
                }
                v[l][j] = a.b[(size_t)lev*a.bs + slot[j]] - acc;
            }
        }
    }
#pragma unroll
    for (int l = 0; l < LC; l++) {
        const int lev = l0 + l;
        double* sx = s_x[l & 1][el];
#pragma unroll
        for (int j = 0; j < RPL; j++) sx[lane + j*LPE] = act[j] ? v[l][j] : 0.0;
        owned_wave_sync();
#pragma unroll
        for (int j = 0; j < RPL; j++) {
            double s = 0.0;
            if constexpr (REG) {
#pragma unroll
                for (int c = 0; c < ND; c++) s += brow[c]*sx[c];
            } else if (act[j]) {
                const double* Br = Bk + (size_t)(lane + j*LPE)*ND;
                for (int c = 0; c < ND; c++) s += Br[c]*sx[c];
            }
            if (!(act[j] && lev < l1)) continue;
            const size_t o = (size_t)slot[j];
            if constexpr (KIND == 0) a.y[(size_t)lev*a.ys + o] = s;
            else {
                double* pp = a.p + (size_t)lev*a.ps + o;
                double* xp = a.xo + (size_t)lev*a.xos + o;
                const double pn = KIND == 2 ? s : fma(a.beta, *pp, s);
                *pp = pn;
                *xp = KIND == 2 ? a.alpha*pn : fma(a.alpha, pn, *xp);
                if (a.upd) a.upd[(size_t)lev*a.us + o] = s;
            }
        }
    }
}

template <int ND>
int launch_owned_nd(mimsem_ctx* c, int kind, OwnedArgs a) {
    constexpr int LPE = ND <= 16 ? 16 : (ND <= 32 ? 32 : 64), EPB = 256/LPE;
    // levels per work item: the block row stays in registers over the chunk (shared blocks); one level per item when every level has its own
    // blocks.  ~6 workgroups per CU as the other block passes, rounded DOWN to 1, 2, 4 or 8 levels: the kernel's compile-time level count is the
    // chunk's, so a work item loads and multiplies no level it does not write (only the ragged last chunk of a call has fewer)
    int lch = 1;
    if (!a.bls) {
        long long want = std::min<long long>(std::min(a.nlev, 8), ((long long)(c->nEl + EPB - 1)/EPB)*a.nlev/(256*6));
        if (c->lch_override > 0) want = std::min(std::min(a.nlev, 8), c->lch_override);       // mimsem_ctx_set_level_chunk: a request replaces the rule
        while (2*lch <= want) lch *= 2;
    }
    a.lch = lch;
    const long long items = (long long)c->nEl*((a.nlev + lch - 1)/lch);
    const dim3 grid((unsigned)((items + EPB - 1)/EPB));
#define MIMSEM_OWNED_LAUNCH(LC) \
    if (kind == 0) hipLaunchKernelGGL((k_owned_pass<ND, LC, 0>), grid, dim3(256), 0, c->stream, a); \
    else if (kind == 1) hipLaunchKernelGGL((k_owned_pass<ND, LC, 1>), grid, dim3(256), 0, c->stream, a); \
    else hipLaunchKernelGGL((k_owned_pass<ND, LC, 2>), grid, dim3(256), 0, c->stream, a);
    switch (lch) {
    case 1: MIMSEM_OWNED_LAUNCH(1) break;
    case 2: MIMSEM_OWNED_LAUNCH(2) break;
    case 4: MIMSEM_OWNED_LAUNCH(4) break;
    default: MIMSEM_OWNED_LAUNCH(8) break;
    }
#undef MIMSEM_OWNED_LAUNCH
    MIMSEM_HIP_TRY(hipGetLastError());
    return MIMSEM_OK;
}

int launch_owned(mimsem_ctx* c, int nd, int kind, const OwnedArgs& a) {
    switch (nd) {
    // 1-forms, orders 1..7 (2 n^2 rows)
    case 2: return launch_owned_nd<2>(c, kind, a);
    case 8: return launch_owned_nd<8>(c, kind, a);
    case 18: return launch_owned_nd<18>(c, kind, a);
    case 32: return launch_owned_nd<32>(c, kind, a);
    case 50: return launch_owned_nd<50>(c, kind, a);
    case 72: return launch_owned_nd<72>(c, kind, a);
    case 98: return launch_owned_nd<98>(c, kind, a);
    // 2-forms, orders 1..7 (n^2 rows; no count is shared with the 1-forms)
    case 1: return launch_owned_nd<1>(c, kind, a);
    case 4: return launch_owned_nd<4>(c, kind, a);
    case 9: return launch_owned_nd<9>(c, kind, a);
    case 16: return launch_owned_nd<16>(c, kind, a);
    case 25: return launch_owned_nd<25>(c, kind, a);
    case 36: return launch_owned_nd<36>(c, kind, a);
    case 49: return launch_owned_nd<49>(c, kind, a);
    }
    return MIMSEM_ERR_UNSUPPORTED;
}

int owned_rows(const mimsem_ctx* c, int form) { return form == 1 ? 2*c->es.n*c->es.n : c->es.n2e; }

// the per-owner row tables of form 1 / 2, built once per context from the element tables (set-up: not inside a capture)
int owned_tables(mimsem_ctx* c, int form) {
    if (c->d_own[form]) return MIMSEM_OK;
    if (c->is_capturing()) return MIMSEM_ERR_STATE;
    const int n = c->es.n, n1e = c->es.n1e, n2e = c->es.n2e, nEl = c->nEl, nd = owned_rows(c, form);
    const int nslots = form == 1 ? c->n1 : c->n2;
    std::vector<int4> tab((size_t)nEl*nd);
    std::vector<int> owner(nslots, -1);
    if (form == 1) {
        if ((long long)c->h_e1x.size() != (long long)nEl*n1e || (long long)c->h_e1y.size() != (long long)nEl*n1e) return MIMSEM_ERR_STATE;
        std::vector<int> g1((size_t)c->n1*2);
        if (c->n1) {
            MIMSEM_HIP_TRY(hipMemcpyAsync(g1.data(), c->d_g1, g1.size()*sizeof(int), hipMemcpyDeviceToHost, c->stream));
            MIMSEM_HIP_TRY(hipStreamSynchronize(c->stream));
        }
        std::vector<std::pair<int, int>> rows;
        for (int e = 0; e < nEl; e++) {
            rows.clear();
            for (int l = 0; l < n1e; l++) {
                if (l%(n + 1) < n) rows.push_back({c->h_e1x[(size_t)e*n1e + l], l});                  // x-edge (row l / (n+1), column l % (n+1))
                if (l/n < n) rows.push_back({c->h_e1y[(size_t)e*n1e + l], n1e + l});                  // y-edge (row l / n, column l % n)
            }
            std::sort(rows.begin(), rows.end());
            for (int r = 0; r < nd; r++) {
                const int s = rows[r].first, q = e*2*n1e + rows[r].second;
                if (s < 0 || s >= nslots || owner[s] >= 0) return MIMSEM_ERR_ARG;                     // two owners: not a partition of the slots
                owner[s] = e;
                const int a = g1[(size_t)s*2], b = g1[(size_t)s*2 + 1];
                if (a != q && b != q) return MIMSEM_ERR_STATE;
                tab[(size_t)e*nd + r] = make_int4(s, q, a == q ? b : a, 0);
            }
        }
    } else {
        std::vector<int> i2((size_t)nEl*n2e);
        if (c->inds2_contig || !c->d_i2) for (size_t i = 0; i < i2.size(); i++) i2[i] = (int)i;
        else {
            MIMSEM_HIP_TRY(hipMemcpyAsync(i2.data(), c->d_i2, i2.size()*sizeof(int), hipMemcpyDeviceToHost, c->stream));
            MIMSEM_HIP_TRY(hipStreamSynchronize(c->stream));
        }
        std::vector<std::pair<int, int>> rows(n2e);
        for (int e = 0; e < nEl; e++) {
            for (int l = 0; l < n2e; l++) rows[l] = {i2[(size_t)e*n2e + l], l};
            std::sort(rows.begin(), rows.end());
            for (int r = 0; r < nd; r++) {
                const int s = rows[r].first;
                if (s < 0 || s >= nslots || owner[s] >= 0) return MIMSEM_ERR_ARG;
                owner[s] = e;
                tab[(size_t)e*nd + r] = make_int4(s, e*n2e + rows[r].second, -1, 0);
            }
        }
    }
    int uncovered = 0;
    for (int o : owner) uncovered += o < 0;
    int4* d = nullptr;
    if (!tab.empty()) {
        if (int rc = c->alloc((void**)&d, tab.size()*sizeof(int4))) return rc;
        if (hipMemcpyAsync(d, tab.data(), tab.size()*sizeof(int4), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) { c->release(d); return MIMSEM_ERR_HIP; }
    }
    c->d_own[form] = d; c->own_uncovered[form] = uncovered;
    return MIMSEM_OK;
}

int owned_form(int op) {
    switch (op) {
    case MIMSEM_OP_UMAT: case MIMSEM_OP_UHMAT: case MIMSEM_OP_UTMAT: case MIMSEM_OP_UTMAT_H: return 1;
    case MIMSEM_OP_WMAT: case MIMSEM_OP_WHMAT: return 2;
    case MIMSEM_OP_PMAT: case MIMSEM_OP_PHMAT: return 0;
    }
    return -1;
}
}  // namespace

// for ksp.hip: 1 when every slot of the form lies in some block (a solve over the whole vector is then preconditioned everywhere)
int mimsem_owned_covers_all(mimsem_ctx* c, int form) {
    if (form != 1 && form != 2) return 0;
    if (owned_tables(c, form)) return 0;
    return c->own_uncovered[form] == 0;
}

extern "C" {

int mimsem_owned_blocks_build(mimsem_ctx* c, int op, int geom_lev0, int nlev, double scale, unsigned flags,
                              const double* f, long long fs, double* out) {
    if (!c || nlev < 0 || geom_lev0 < 0 || (flags & ~MIMSEM_FLAG_VERT)) return MIMSEM_ERR_ARG;
    const int form = owned_form(op);
    if (form < 0) return MIMSEM_ERR_ARG;
    if (form == 0) return MIMSEM_ERR_UNSUPPORTED;                  // M0 is diagonal: Jacobi is exact (mimsem_ksp_set_pc_bjacobi)
    if (nlev == 0 || c->nEl == 0) return MIMSEM_OK;
    if (!out || geom_lev0 + nlev > c->nk) return MIMSEM_ERR_ARG;
    if ((op == MIMSEM_OP_UHMAT || op == MIMSEM_OP_UTMAT_H || op == MIMSEM_OP_WHMAT) && !f) return MIMSEM_ERR_ARG;
    if (c->is_capturing()) return MIMSEM_ERR_STATE;
    int rc;
    if ((rc = owned_tables(c, form))) return rc;
    const int nd = owned_rows(c, form), n1e = c->es.n1e, nde = form == 1 ? 2*n1e : c->es.n2e;
    const int esz = mimsem_op_elmat_size(c, op);
    if (esz != (form == 1 ? 4*n1e*n1e : nde*nde)) return MIMSEM_ERR_UNSUPPORTED;
    const long long per = (long long)c->nEl*nd*nd;
    double* em = nullptr;
    MIMSEM_HIP_TRY(hipMalloc((void**)&em, (size_t)c->nEl*esz*sizeof(double)));
    for (int l = 0; l < nlev && !rc; l++) {
        if ((rc = mimsem_op_element_matrices(c, op, geom_lev0 + l, scale, flags, f ? f + (size_t)l*fs : nullptr, em))) break;
        hipLaunchKernelGGL(k_owned_assemble, dim3((unsigned)((per + 255)/256)), dim3(256), 0, c->stream, per, nd, form, n1e, nde, c->d_own[form],
                           em, out + (size_t)l*per);
        if (hipGetLastError() != hipSuccess) rc = MIMSEM_ERR_HIP;
    }
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = MIMSEM_ERR_HIP;      // (em is freed below)
    (void)hipFree(em);
    return rc;
}

int mimsem_owned_blocks_apply(mimsem_ctx* c, int form, int nlev, const double* blocks, long long bls,
                              const double* x, long long xs, double* y, long long ys) {
    if (!c || nlev < 0 || bls < 0 || form < 0 || form > 2) return MIMSEM_ERR_ARG;
    if (form == 0) return MIMSEM_ERR_UNSUPPORTED;
    if (nlev == 0 || c->nEl == 0) return MIMSEM_OK;
    if (!blocks || !x || !y || x == y) return MIMSEM_ERR_ARG;
    const long long n = form == 1 ? c->n1 : c->n2;
    if (nlev > 1 && (xs < n || ys < n)) return MIMSEM_ERR_ARG;
    int rc;
    if ((rc = owned_tables(c, form))) return rc;
    OwnedArgs a{};
    a.nEl = c->nEl; a.nlev = nlev; a.plan = c->d_own[form]; a.B = blocks; a.bls = bls;
    a.x = x; a.xs = xs; a.y = y; a.ys = ys;
    return launch_owned(c, owned_rows(c, form), 0, a);
}

int mimsem_owned_block_chebyshev_solve(mimsem_ctx* c, int op, int geom_lev0, int nlev, double scale, unsigned flags,
                                       const double* blocks, long long bls, const double* b, long long bs, int nsteps, const double* coef,
                                       double* x, long long xs, double* pb, long long pbs, double* upd, long long upds) {
    if (!c || nlev < 0 || bls < 0 || nsteps < 1 || !coef || (flags & ~MIMSEM_FLAG_VERT)) return MIMSEM_ERR_ARG;
    if (op != MIMSEM_OP_UMAT) return MIMSEM_ERR_UNSUPPORTED;
    if (c->es.n > 5) return MIMSEM_ERR_UNSUPPORTED;                // the element pass of the solve (as mimsem_block_chebyshev_solve)
    if (nlev == 0 || c->nEl == 0) return MIMSEM_OK;
    if (!b || !blocks || !x || x == b || geom_lev0 < 0 || geom_lev0 + nlev > c->nk) return MIMSEM_ERR_ARG;
    if (nlev > 1 && (xs < c->n1 || bs < c->n1 || (pb && pbs < c->n1) || (upd && upds < c->n1))) return MIMSEM_ERR_ARG;
    int rc;
    if ((rc = owned_tables(c, 1))) return rc;
    if (c->own_uncovered[1]) return MIMSEM_ERR_UNSUPPORTED;        // a slot outside every block would keep an undefined iterate
    const ElemSizes& es = c->es;
    const long long per = (long long)c->nEl*2*es.n1e, n1 = c->n1;
    if ((rc = c->ensure_ye(per*nlev))) return rc;
    if ((rc = c->ensure_cheb(n1*nlev))) return rc;
    ElemArgs e{};
    e.nEl = c->nEl; e.nlev = nlev; e.lev0 = geom_lev0; e.total = c->nEl*nlev;
    e.flags = flags; e.scale = scale; e.alpha = 1.0;
    e.J = c->d_J; e.det = c->d_det; e.tI = c->d_tI; e.th = c->d_th; e.tIp = c->d_tIp; e.tnp = c->nk/2 + 1; e.tps = (long long)c->nEl*es.mp12*2; e.tnode = 0;
    e.E = c->d_E; e.w = c->d_w;
    e.i0 = c->d_i0; e.i1x = c->d_i1x; e.i1y = c->d_i1y; e.i2 = c->d_i2; e.iq = c->d_iq; e.xn = c->d_xn;
    e.lch = mimsem_op_level_chunk(c, nlev); e.swz = 0;          // (the element pass's levels per work item)
    e.out = c->d_ye; e.os = per;
    c->ev_k1[0] = c->ev_k1[1] = c->ev_k2[0] = c->ev_k2[1] = nullptr;
    OwnedArgs a{};
    a.nEl = c->nEl; a.nlev = nlev; a.plan = c->d_own[1]; a.B = blocks; a.bls = bls;
    a.ye = c->d_ye; a.yes = per; a.b = b; a.bs = bs; a.p = c->d_cheb; a.ps = n1; a.xo = x; a.xos = xs;
    const int nd = owned_rows(c, 1);
    for (int k = 0; k < nsteps; k++) {
        if (k > 0) {                                                // A x into the element-local workspace (the gather happens in the block pass)
            e.x = x; e.xs = xs;
            if ((rc = launch_elem_apply(c, MIMSEM_OP_UMAT, e))) return rc;
        }
        a.alpha = coef[2*k]; a.beta = coef[2*k + 1];
        // the check vectors: pb = z_0, upd = z_{nsteps-1}; a one-step solve has one z for both
        a.upd = k == nsteps - 1 && upd ? upd : (k == 0 ? pb : nullptr); a.us = k == nsteps - 1 && upd ? upds : pbs;
        if ((rc = launch_owned(c, nd, k == 0 ? 2 : 1, a))) return rc;
    }
    if (nsteps == 1 && upd && pb)
        for (int l = 0; l < nlev; l++) MIMSEM_HIP_TRY(hipMemcpyAsync(pb + (size_t)l*pbs, upd + (size_t)l*upds, (size_t)n1*sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return MIMSEM_OK;
}

}  // extern "C"
