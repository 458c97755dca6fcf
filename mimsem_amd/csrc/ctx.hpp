// mimsem_amd/csrc/ctx.hpp -- device context shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <utility>
#include <vector>
#include "../../include/mimsem_hip.h"
#include "basis_host.hpp"
#include <cstdlib>

// CLOSED EXPERIMENTS: the variants that were built, measured and declined (their records are under profiles/).
//   default build           their switches do not exist (exp_env is a compile-time null) and the kernel families only they launch are not
//                           compiled in (kExperiments: the fused-scatter element kernels, the tile mode of k_apply_wave, the 16-lane order-4
//                           walk of solve_schur_column_3, the residency variants of k_thomas_dpp2, the row-parallel 9 x 9 inverse);
//   -DMIMSEM_WITH_EXPERIMENTS  (scripts/build_variant.sh exp "-DMIMSEM_WITH_EXPERIMENTS" -> build_ab/libmimsem_hip_exp.so, MIMSEM_LIB=...)
//                           everything is compiled in and the switches are read when MIMSEM_EXPERIMENTS=1 is set in the environment -- what
//                           scripts/ab_*.sh and the variants' parity tests run against.
constexpr int MIMSEM_RD_COUNTERS = 8;
#ifdef MIMSEM_WITH_EXPERIMENTS
constexpr bool kExperiments = true;
inline const char* exp_env(const char* name) {
    static const bool on = std::getenv("MIMSEM_EXPERIMENTS") && std::atoi(std::getenv("MIMSEM_EXPERIMENTS")) != 0;
    return on ? std::getenv(name) : nullptr;
}
#else
constexpr bool kExperiments = false;
inline const char* exp_env(const char*) { return nullptr; }
#endif

namespace mimsem {
extern thread_local std::string g_last_hip_error;
int hip_fail(hipError_t e, const char* what);
}

#define MIMSEM_HIP_TRY(call)                                                        \
    do { hipError_t e__ = (call);                                                   \
         if (e__ != hipSuccess) return mimsem::hip_fail(e__, #call); } while (0)

// element sizes for order n (quadrature collocated: m == n)
struct ElemSizes {
    int n, np1, mp1, mp12, n0e, n1e, n2e;
    explicit ElemSizes(int order = 1)
        : n(order), np1(order + 1), mp1(order + 1), mp12((order + 1)*(order + 1)),
          n0e((order + 1)*(order + 1)), n1e((order + 1)*order), n2e(order*order) {}
};

// The wave-level plan of a context (k_apply_wave, elem_wave.inc): wave-groups of 64/LPE neighbouring elements.  setup_wave (api.hip) builds
// a whole new value from build_wave_plan / build_wave_own and assigns it only when every table is on the device; the tables of the plan it
// replaces stay allocated until the context goes (a captured graph may hold their addresses).
struct WaveTables {
    bool on = false;                    // the context has a plan (MIMSEM_WAVE=0, orders > 4 and numberings the plan does not fit: none)
    int ngroups = 0, nsing = 0, nps = 0, npart = 0, ndirect = 0;
    int npwritten = 0;                  // partial sums a level really gets (npart is the padded row: nsides x 2 x 16)
    // in-kernel completion of the perimeter (round 3, elem_wave.inc "finishing phase"): the partial sums are laid out per SIDE (the
    // slots two wave-groups share), and the group that arrives second at a side's counter finishes its slots -- no second launch
    bool can_fin = false;               // the plan supports it (MIMSEM_WAVE_FIN=0 keeps the perimeter pass)
    int nsides = 0;
    int4* fin = nullptr;                // [ngroups][8] {side, arrivals that complete it (2; 1: a side of the group's own), entries, 0} or {-1, 0, 0, 0}
    int* sslot = nullptr;               // [nsides][16] y slot of entry j of the side (-1: none)
    int* cnt = nullptr;                 // [nsides][nk] arrival counters, zero between launches (the finishing wave resets its own)
    int nbgroups = 0, nbrec = 0; bool split = false;     // interior / boundary split (mimsem_ctx_set_halo_slots): boundary prefix sizes
    int4* lane = nullptr;               // [ngroups][64] {element of the lane, load pair: even slot b, staging positions of x[b] and of x[b+1]
                                        //   (two 16-bit positions each; the dump position where nobody wants the value)}
    // owner-computes form (round 7, build_wave_own; Umat at p = 3, default, MIMSEM_WAVE_OWN=0: off, =1: ghost pass per batch): every store pair written finished by
    // its one owner group, which computes the neighbour's contribution across its ghost sides -- one launch, no perimeter pass
    bool own = false;
    int4* oplan = nullptr;              // [ngroups][64] store pairs of the form (as plan; every destination in y)
    int4* gh = nullptr;                 // [ngroups][16] packed ghost lanes (side*4 + point; round 9)
    int* gx = nullptr;                  // [ngroups][64] slot the lane gathers per level (16 per ghost side)
    int4* gh4 = nullptr;                // [ngroups][64] ghost lanes of the four-level pass (own4::k_apply_wave: DPP row = ghost side), or
                                        //   null: MIMSEM_WAVE_OWN=1 keeps the pass per batch of two levels for every call
    int4* tfin = nullptr; int ntiles = 0, ninner = 0;      // tile mode (round 5): [ntiles][64] {slot, LDS position of part A, of part B, 0}
    int4* plan = nullptr;               // [ngroups][64] store pair {dst, result positions of its first and second slot (2 x 16 bit, the
                                        //   strip's zero for a missing contributor), 0}: dst >= 0: y[dst], y[dst+1]; dst <= -2: partial sums
                                        //   -(dst+2), +1 of the workspace row (unused lanes: its dump tail)
    int2* sing = nullptr;               // [ngroups][64] optional 8-byte store round {slot or -1, positions} (MIMSEM_WAVE_SINGLES=1)
    int* node = nullptr;                // [ngroups][64] node slot of the lane's quadrature point (RotMat's vorticity)
    double* G = nullptr;                // [ngroups][64][4] {gaa, gab, gbb, 1/det} of the lane's point: Q/det J^T J, in WAVE-GROUP order
    double* R = nullptr;                // [ngroups][64]    (-J00 J11 + J01 J10) Q/det: RotMat
    int4* prec = nullptr;               // [nps] {slot, partial 0, partial 1 (-1: none), 0}: slots finished by k_wave_perim (and slots no element
                                        //   touches: no partial at all, written as 0)
};

enum class Mem { Plain, Uncached, FineGrained };      // kinds of device memory mimsem_ctx::alloc hands out

// The band plan of mimsem_zonal_plan_build (zonal_stats.inc): the kept quadrature points sorted by (band, element, point).  A whole new
// value is assigned once its three tables are on the device; the tables it replaces stay allocated until the context goes.
struct ZonalPlan {
    int nb = 0, nne = 0, npts = 0;      // bands of the caller's table (0: no plan), non-empty bands, kept points
    int* band = nullptr;                // [nne]     band of work item i
    int* off = nullptr;                 // [nne + 1] its points are pt[off[i]] .. pt[off[i+1] - 1]
    int* pt = nullptr;                  // [npts]    e mp12 + q, every entry checked against nEl mp12 by the builder
};

struct mimsem_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t cap_stream = nullptr, cap_saved = nullptr; bool cap_active = false, cap_swapped = false;      // mimsem_graph_begin / _end
    hipStream_t own_stream = nullptr;          // mimsem_ctx_use_own_stream
    void* h_pin = nullptr;                     // 4 KB of pinned host memory: small read-backs (mimsem_memcpy_d2h) skip the pageable-copy path
    ElemSizes es;
    int nEl = 0, nk = 0, n0 = 0, n1 = 0, n2 = 0;
    bool inds2_contig = true;
    mimsem::BasisTables tab;

    // ---- HBM-resident data (layout: DESIGN.md "Data layout in HBM") ----
    double* d_E = nullptr;      // [mp1][n]   edge basis at quad points
    double* d_w = nullptr;      // [mp1]      GLL weights
    double* d_xn = nullptr;     // [np1]      nodal (GLL) points, for Lagrange evaluation at departure points
    double* d_U = nullptr;      // dense tables for the element-matrix kernels
    double* d_V = nullptr;
    double* d_W = nullptr;
    double* d_P = nullptr;
    double* d_J = nullptr;      // [nEl][4][mp12]  component-major per element (coalesced per component)
    double* d_det = nullptr;    // [nEl][mp12]
    double* d_th = nullptr;     // [nk][nEl][mp12] thickness at the element's own quad points
    double* d_tI = nullptr;     // [nk][nEl][mp12] inverse thickness
    bool cheb_pend = false;     // MIMSEM_CHEB_PEND=1 (experiments build): mimsem_block_chebyshev_solve in two launches per step
    bool blocks_mfma = false;   // block pass of the Chebyshev / Richardson sweeps on the matrix cores (default at p = 4, MIMSEM_BLOCKS_MFMA=0|1 at context creation overrides; p <= 3: register-row form)
    double* d_tIp = nullptr;    // [2][nk/2 + 1][nEl][mp12][2]: the same in level PAIRS {L, L+1}, first index = parity of L (k_apply_wave: one 16-byte load per two levels)
    double* d_tIn = nullptr;    // [2][nk/2 + 1][n0][2]: the same per NODE (MIMSEM_WAVE_TNODE=1; null unless every element holds the same value at a shared node)
    bool have_levels = false;
    int* d_i0 = nullptr;        // [nEl][n0e]
    int* d_i1x = nullptr;       // [nEl][n1e]
    int* d_i1y = nullptr;       // [nEl][n1e]
    int* d_i2 = nullptr;        // [nEl][n2e] or null (contiguous)
    int* d_iq = nullptr;        // [nEl][mp12] quad-grid slots (projection operators), may be null
    int nq = 0;
    // deterministic scatter-add plans: vector slot -> up to K element-local result slots (-1 = none)
    int* d_g1 = nullptr;        // [n1][2]   into ye1[e*2*n1e + j]  (j<n1e: x edge, else y edge)
    int* d_bplan = nullptr;     // [nEl][2 n1e][4] = {slot, d_g1[slot][0], d_g1[slot][1], 0}: the block passes' view of d_g1, one 16-byte load per block row
    int* d_g0 = nullptr;        // [n0][G0]  into ye0[e*n0e + j]
    int G0 = 4;
    // fused scatter-add of 1-form results: element groups = workgroups, group-local slot ids
    bool fused1 = false;
    int f_ngroups = 0, f_lmax = 0, f_nps = 0, f_npart = 0;
    int* d_fperm = nullptr;             // [ngroups][EPB] element of each lane group (-1 = padding)
    unsigned short* d_flid = nullptr;   // [ngroups][lmax][2] positions (el*2*n1e + dof) of the 1-2 contributions of each local slot
    int* d_fslot = nullptr;             // [ngroups][lmax] vector slot (>=0, complete in group) or -(partial index+1)
    int* d_fcnt = nullptr;              // [ngroups] local ids in use
    int* d_pslot = nullptr;             // [nps] perimeter slots
    int* d_ppart = nullptr;             // [nps][2] their partial-sum indices (-1 = none)
    // wave-level fused scatter-add (k_apply_wave, elem_wave.inc): the plan is `wv` (WaveTables above); what follows are the tuning knobs
    WaveTables wv;
    ZonalPlan zon;                      // mimsem_zonal_plan_build
    int wave_order = 3;                 // bit 0: XCD-contiguous block order, bit 1: group-major items (MIMSEM_WAVE_ORDER)
    int wave_lch = 0;                   // MIMSEM_WAVE_LCH override of the levels per chunk
    int wave2_mode = 1;                 // MIMSEM_WAVE2: 2-form-valued operators on k_apply_wave2 (p = 3): 0 none, 1 Whmat / WtQUmat / WtQdUdz, 2 also Wmat
    int wave_cpp = 0;                   // MIMSEM_WAVE_CPP override of the chunks per work item (0: heuristic)
    int wave_part = 0;                  // mimsem_ctx_set_wave_split: levels of a part of the owner form's level ranges (0: the items of the chunk form)
    // balanced level ranges of the owner form's four-level kernel (wave_balance.hpp): one planned item list per (levels, groups,
    // workgroups), made on the first such call outside a capture and kept for the context's life
    int dev_ncu = 0;                    // hipDeviceProp_t::multiProcessorCount of the context's device
    int bal_ncu = -1, bal_k = 2;        // CUs the planner deals over (< 0: off, the default; 0: the device's -- MIMSEM_WAVE_BALANCE=k) and workgroups per CU
    struct BalList { int nlev, ngroups, nwg; const int4* items; int nitems, longest; };      // items {group, first level, end level, 0}; null: the planner refused
    std::vector<BalList> bal;
    long long bal_launches = 0;         // launches of own4::k_apply_wave_list so far (mimsem_ctx_wave_balance_launches)
    int w_partmem = 0;                  // memory kind of d_wpart: 0 uncached, 1 fine-grained, 2 plain (MIMSEM_WPART_MEM, experiments)
    double* d_wpart = nullptr;          // [nlev][wv.npart + 128] partial sums of the finishing phase: UNCACHED device memory (plain stores go
    long long wpart_doubles = 0;        //   through to the memory side: visible to a finishing wave on another XCD once acknowledged)
    // a split apply (mimsem_op_apply_part): its partial sums live in a buffer no other entry point uses, and the pending BOUNDARY part
    // is remembered so that only the matching INTERIOR part can consume it
    double* d_wsplit = nullptr; long long wsplit_doubles = 0;
    struct { bool pending = false; int op = 0, lev0 = 0, nlev = 0; unsigned flags = 0; const double* y = nullptr; long long ys = 0; } split;
    std::vector<int> h_i1x, h_i1y, h_i0; std::vector<double> h_J, h_det;      // host copies of the mesh for re-deriving the plan
    std::vector<int> h_e0;              // element -> 0-form slot lists (node multiplicities, likewise)
    std::vector<int> h_e1x, h_e1y;      // element -> 1-form slot lists, kept on EVERY context (edge multiplicities of the PCBJACOBI builders, ksp.hip)
    // workspace
    double* d_ye = nullptr;     // [nk_ws][nEl][max(2*n1e, n0e)] element-local results
    long long ye_doubles = 0;
    // owned-block preconditioner (owned_blocks.hip): per form 1 / 2, [nEl][rows] {slot, owner position, other position, 0}, built on first use
    int4* d_own[3] = {nullptr, nullptr, nullptr}; int own_uncovered[3] = {0, 0, 0};      // slots of the form that no element owns
    double* d_pcw = nullptr;    // [nEl][2 n1e] 1 / edge multiplicity of the element-local 1-form DoFs (mimsem_elem_block_pc_build), made on first use
    double* d_cheb = nullptr; long long cheb_doubles = 0;      // mimsem_block_chebyshev_solve: the second iterate and two direction vectors, [3][nlev][n1]
    int *d_d0 = nullptr, *d_d1x = nullptr, *d_d1y = nullptr;   // direct-write slots (single-contributor DoFs), see ElemArgs
    int *d_sh0 = nullptr, *d_sh1 = nullptr; int nsh0 = 0, nsh1 = 0;   // slots with >= 2 contributors: the only ones pass 2 visits
    bool direct = false;
    bool colstat_valid = false;
    double* d_colratio = nullptr;   // [nEl] |last correction| / |solution| of that solve
    int* d_colstat = nullptr;   // [1 + nEl] status of the last block-tridiagonal column solve (mimsem_column_solve_status)
    double* d_col = nullptr;    // column-solver workspace
    unsigned* d_rdcnt = nullptr;   // [MIMSEM_RD_COUNTERS] arrival counters of the one-launch rowdot (krylov_kernels.hip: k_rowdot_fused, calls of up to 8 rows), zero between calls
    std::vector<void*> graphs;  // the recordings (mimsem_graph*) made on this context and still alive: orphaned by mimsem_ctx_destroy
    bool rd_two = false;           // MIMSEM_ROWDOT_TWO (experiments build): the two-launch rowdot, for the A/B of round 6
    bool memset_node = false; int blu_stop = 0;      // MIMSEM_MEMSET_NODE / MIMSEM_BLU_STOP, read once at creation
    std::vector<char> h_halo1;  // [n1] 1 = the 1-form slot takes part in a halo exchange (mimsem_ctx_set_halo_slots): its second element lives on another rank
    int* d_forceflag = nullptr; int n_forceflag = 0;      // mimsem_column_flag_for_test: columns the next solve treats as flagged (one-shot)
    int pivot_fallback = 1;     // mimsem_column_set_pivot_fallback: flagged columns are re-solved by a band LU with partial pivoting (column_pivot.inc)
    double* d_lu = nullptr;     // its workspace: per wavefront of the fallback's grid, the rows of U and the multipliers of one column
    long long lu_doubles = 0;
    long long col_doubles = 0;
    double col_param = 0.0;             // scalar argument of the *_ex column operators (dt_fric / dt)
    const double* col_uh = nullptr;     // horizontal velocity [nk][n1] of the *_up column operators
    long long col_uhs = 0;
    int swz = 1;                   // MIMSEM_NOSWZ=1 disables the XCD-aware block order (tuning)
    int lch_override = 0;          // mimsem_ctx_set_level_chunk; MIMSEM_LCH in the experiments build (tuning and tests): 0 = the library's rules
    // measurement hook: event triples (start, mid, end) around pass 1 / pass 2 of mimsem_op_apply
    bool profiling = false;
    int prof_every = 1; long long prof_count = 0;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    hipEvent_t next_event();
    hipEvent_t ev_k1[2] = {nullptr, nullptr};   // start/stop events of the next element kernel (null = not profiling)
    hipEvent_t ev_k2[2] = {nullptr, nullptr};   // ... of the next gather-sum kernel
    std::vector<char> ev_has2;                  // per profiled apply: a second kernel recorded its pair (pooled events keep OLD stamps otherwise)
    void mark_k2() { if (ev_k2[0] && !ev_has2.empty()) ev_has2.back() = 1; }

    // ---- device memory: ONE owner.  Everything the context allocates comes from alloc() and is freed by mimsem_ctx_destroy from `owned`;
    // `bytes` (mimsem_ctx_workspace_bytes) is the sum of what is in the list.  A buffer that is outgrown or replaced is RETIRED: the context
    // stops naming it and nothing else happens -- a hipGraph captured earlier has its address baked into kernel arguments and must keep
    // working on it.  release() is for the few buffers no recording can hold.
    std::vector<std::pair<void*, size_t>> owned;
    long long bytes = 0;
    int alloc(void** p, size_t nbytes, Mem kind = Mem::Plain);      // at least one byte; *p is written on success only
    // alloc's book-keeping.  Its one other caller is mimsem_ksp::ensure (ksp.hip), which retires the handle's outgrown workspace to the context
    void adopt(void* p, size_t nbytes) { owned.emplace_back(p, nbytes); bytes += (long long)nbytes; }
    void release(void* p);                                          // frees p and drops it from the list (the caller has synchronised)
    bool is_capturing() const;           // the context's stream is inside a hipGraph capture (workspaces must not grow there)
    // workspaces only ever grow: a new buffer of `doubles` when `have` is less (MIMSEM_ERR_STATE inside a capture), the old one retired
    int grow(double*& buf, long long& have, long long doubles, Mem kind = Mem::Plain);
    int ensure_ye(long long n)     { return grow(d_ye, ye_doubles, n); }
    int ensure_col(long long n)    { return grow(d_col, col_doubles, n); }
    int ensure_cheb(long long n)   { return grow(d_cheb, cheb_doubles, n); }
    int ensure_wsplit(long long n) { return n > wsplit_doubles && split.pending ? MIMSEM_ERR_STATE : grow(d_wsplit, wsplit_doubles, n); }
    // UNCACHED device memory: a plain store is acknowledged by the memory side, not by the storing XCD's L2 (MIMSEM_WPART_MEM=finegrained |
    // plain select other kinds for experiments; `plain` is NOT coherent across XCDs inside one launch)
    int ensure_wpart(long long n)  { return grow(d_wpart, wpart_doubles, n, w_partmem == 2 ? Mem::Plain : (w_partmem == 1 ? Mem::FineGrained : Mem::Uncached)); }
    int ensure_kry(long long n);         // ... and, once, the arrival counters of the one-launch rowdot
    int gs_fused = -1;                  // second Gram-Schmidt pass + normalisation in two launches (mimsem_krylov_gs_control; -1: from the environment)
    int* gs_flag = nullptr;             // caller's word (device or pinned host), set to 1 when that form's Pythagorean norm would cancel
    double* d_kry = nullptr;            // partial sums of the Krylov multi-dot
    long long kry_doubles = 0;
};

// tile mode of the wave-level kernel (round 5): finishing entries per tile, doubles of a tile's LDS row, levels the LDS rows hold
constexpr int MIMSEM_WTF = 64, MIMSEM_WTP = 64, MIMSEM_WTLEV = 32;
// owner-computes form of the wave-level kernel (round 7): gathered ghost DoFs of a wave-group (one 8-byte gather per lane and level;
// round 9: 16 per ghost side, a quadruple per side point)
constexpr int MIMSEM_WGX = 64;

// kernels (elem_kernels.hip / column_kernels.hip) ---------------------------------------------------
struct ElemArgs {
    int nEl, nlev, lev0, total;
    int swz;                       // XCD-aware work-item order on/off
    int lch;                       // levels handled by one work item (level-invariant data stays in registers)
    unsigned flags;
    double scale, alpha;
    const double *J, *det, *tI, *th, *E, *w;
    const double* tIp; int tnp;          // level-pair copy of tI, pairs per parity
    long long tps; int tnode;            // doubles between two pair rows of tIp; tnode: tIp is the NODAL table (entry = node slot of the point, wnode) instead of [element][point]
    const int *i0, *i1x, *i1y, *i2, *iq;
    const double* f; long long fs;
    const double* f2; long long f2s;   // second coefficient field (velocity of the upwinded operators)
    double param;                       // tau of the upwinded operators
    const double* xn;                   // nodal points
    const double* x; long long xs;
    double* out; long long os;     // element-local results (or the 2-form output vector itself); fused: partial sums
    // fused 1-form scatter-add
    const int* fperm; const unsigned short* flid; const int* fslot; const int* fcnt; int ngroups, lmax;
    double* y; long long ys; int accum;
    // wave-level fused scatter-add (k_apply_wave)
    const int4* wlane; const int4* wplan; const int2* wsing; const int* wnode; const double* wG; const double* wR; int wgroups; int wg0; int wdump; int wcpp;
    const int4* wfin; const int* wsslot; int* wcnt;      // finishing phase (null: the perimeter pass follows)
    const int4* wtfin; int wtile;                        // tile mode: finishing entries per tile (stride wtile), or null
    const int4* wgh; const int* wgx;                     // owner-computes form: packed ghost lanes, gathered slots (build_wave_own), or null
    // level ranges (round 10, wave_level_parts): wnp > 0 -- every group is cut into wnp parts of whole level PAIRS, part k = levels
    // 2 (k wpb + min(k, wpr)) .. + 2 (wpb + (k < wpr)), clipped to nlev; a wavefront leaves at the first batch boundary at or beyond its
    // last level.  0: the chunk arithmetic (lch, wcpp).  own4::k_apply_wave has no use for wcpp as a count: dispatch_apply_wave puts
    // floor((2^32 - 1)/divisor) there, with which the kernel splits an item into group and part by a multiplication
    int wnp, wpb, wpr;
    int wfence;                      // finishing phase, experiment: partial sums in PLAIN memory, one agent-scope release fence per wavefront before its arrival
    double Etab[20];                 // edge-basis table E[mp1][n] by value (orders <= 4): SGPRs, no load in the kernel
    double Wq[5];                    // GLL weights by value (orders <= 4)
    long long* wstamps;              // diagnostic build (MIMSEM_STAMPS): 16 s_memtime stamps per work item, else null
    // direct path: DoFs touched by exactly ONE element are written straight into y (no ye round trip, no pass 2 for them)
    const int *d0, *d1x, *d1y;       // [nEl][n0e|n1e]: the slot when the element is its only contributor, else -1 (null = off)
    int lstep = 1;                   // geometry level of row r: lev0 + r lstep; 0 = every row at lev0 (mimsem_op_apply_levels, k_elem_apply only)
    const int4* wgh4 = nullptr;      // owner-computes form: ghost lanes of the four-level pass (build_wave_own), or null: the pass per batch
    // ... its planned items (wave_balance.hpp), four consecutive ones a workgroup: {group, first level, end level, 0}; null: wnp, wpb, wpr
    const int4* witems = nullptr; int wnitems = 0;
    // KNOWN SENSITIVITY: the wave kernels' prologues wait for a handful of these fields by scalar loads, and how the compiler groups those
    // loads depends on the fields' offsets -- adding the two above moved the headline step by -0.27 us, a prologue with the loads behind
    // a branch by +0.5 us.  After a change to this struct, look at the first waits of own4::k_apply_wave in the assembly
    // (one s_waitcnt before the exit test) and measure the loop of profiles/umat_balance_ab.txt.
};

// The vector update a Chebyshev step still owes (mimsem_block_chebyshev_solve: the gather epilogue of step k folded into the element pass of
// step k + 1).  For the slots of its element a lane forms  z = sum of the element-local P r through the plan (the epilogue's order),
// p = z + beta p_in,  x = x_in + alpha p  and applies the operator to THAT x; the slot's first contributor stores x and p into the OTHER
// pair of buffers (the other elements of the slot read the old values in this same launch).  first: x_in = 0 and p_in are not read.
struct ElemPending {
    const int* plan; const double* ze; long long zes;
    double alpha, beta; int first;
    const double* p_in; double* p_out; long long ps;                     // [nlev][n1] rows (x_in is ElemArgs::x, stride ElemArgs::xs)
    double* x_out; long long xos;
    double* upd; long long us;                                           // receives z if given
};
// pass 2 with an epilogue (the Richardson sweeps): what happens to the gathered sum `acc` of a slot
struct GatherEpilogue {
    int mode;                        // 1, 5: d = dinv*(b - acc) ; 2, 3: d = acc.   1, 2: x += d.   3, 5: p = d + beta p ; x += alpha p.   upd = d if given
    const double* b; long long bs;
    const double* dinv; long long ds;
    double* upd; long long us;
    double alpha = 1.0, beta = 0.0;  // mode 3 (Chebyshev semi-iteration)
    double* p = nullptr; long long ps = 0;
    const double* escale = nullptr; long long ess = 0;      // block pass: per (level, element) factor of the element blocks
    // mode 4 (round 5): the vector algebra of a Chebyshev step on B = P A with acc = (B d)[s]:  x += d;  r -= acc;  d = alpha d + beta r.
    // d lives in p (in/out), r in cr
    double* cr = nullptr; long long crs = 0;
    int zero = 0;                    // modes 3, 5, first step of a solve from x = 0: p = d, x = alpha d -- neither is read (mimsem_block_chebyshev_solve, mimsem_sw_dual_chebyshev)
    int noacc = 0;                   // ... and the operator result is zero: acc = 0, ye is not read (mode 5 without a block pass in between)
};
// two independent Chebyshev sweeps in the same launches (elem_kernels.hip: k_sw_pair): the block pass and the gather epilogue of one level
struct PairBlocks { int nEl, lch; const int *i1x, *i1y, *plan; const double *B, *ye; long long yes; const double* b; double* ze; long long zes; const int4* bplan; };
struct PairGather { const double* ye; long long yes; const int* plan; int nslots; GatherEpilogue g; double* x; };
// phase PA of the 1-form mass sweep (0 element pass, 1 block pass, 2 gather epilogue) and phase PB of the upwinded 0-form sweep (0 element
// pass, 1 gather epilogue) in ONE launch; orders 2..4
int launch_sw_pair(mimsem_ctx* c, int PA, int PB, const ElemArgs& ea, const PairBlocks& ba, const PairGather& ga, const ElemArgs& eq, const PairGather& gq);
int launch_gather_epilogue(mimsem_ctx* c, int form, int nlev, const double* ye, long long ye_stride, const GatherEpilogue& g,
                           double* x, long long xs);
int launch_blocks_residual(mimsem_ctx* c, int nlev, const double* B, const double* ye, long long yes,
                           const double* b, long long bs, double* ze, long long zes,
                           const double* escale = nullptr, long long ess = 0);
int launch_elem_apply(mimsem_ctx* c, int op, const ElemArgs& a);
int launch_elem_apply_pending(mimsem_ctx* c, const ElemArgs& a, const ElemPending& pd);      // Umat with the owed Chebyshev update (orders <= 5)
int launch_gather_perim(mimsem_ctx* c, int nlev, const double* yp, long long yps, int accum, double* y, long long ys,
                        const int* pslot = nullptr, const int* ppart = nullptr, int nps = -1);
int launch_apply_wave(mimsem_ctx* c, int op, const ElemArgs& a);
int wave_workgroup_waves();          // wavefronts per workgroup of the wave-level kernels
int launch_apply_wave2(mimsem_ctx* c, int op, const ElemArgs& a);
int launch_wave_perim(mimsem_ctx* c, int nlev, const double* yp, long long yps, int accum, double* y, long long ys, int r0 = 0, int r1 = -1);
int launch_gather_sum(mimsem_ctx* c, int form, int nlev, const double* ye, long long ye_stride, int accum,
                      double* y, long long ys, bool shared_only = false);
int launch_blocks_apply(mimsem_ctx* c, int form, int nlev, int transposed, const double* B, long long bstride_lev,
                        const double* x, long long xs, double* y, long long ys, double alpha, int accum,
                        const double* escale = nullptr, long long escale_stride = 0);
int launch_halo_segments(mimsem_ctx* c, const int* idx, int nseg, const int* seg_off, int s_begin, int s_end, int nlev, int mode,
                         double* buf, double* v, long long vs);
int launch_elmats(mimsem_ctx* c, int op, int lev, double scale, unsigned flags, const double* f, double* out,
                  const double* f2 = nullptr, double param = 0.0);
int launch_incidence(mimsem_ctx* c, int which, int nlev, const double* x, long long xs, double* y, long long ys);
int launch_interp_quad(mimsem_ctx* c, int form, int global, int nlev, const double* x, long long xs, double* out, long long os);
int launch_sw_operator(mimsem_ctx* c, int nlev, double a, double grav, double H, const double* f0, long long f0s,
                       const double* x, long long xs, double* y, long long ys);
int launch_sw_blocks_apply(mimsem_ctx* c, int nlev, const double* B, const double* x, long long xs, double* y, long long ys);
int launch_sw_operator_precond_chebyshev(mimsem_ctx* c, int nlev, double a, double grav, double H, const double* f0, long long f0s,
                                         const double* B, double ca, double cb, double* x, long long xs, double* r, long long rs, double* d, long long ds);
int launch_sw_chebyshev_step2(mimsem_ctx* c, int nlev, double a, double grav, double H, const double* f0, long long f0s, const double* B,
                              int pending, double pca, double pcb, double ca, double cb, double* x, long long xs,
                              const double* r_in, const double* d_in, double* r_out, double* d_out, double* rh, double* dh, long long vs);
int launch_sw_chebyshev_flush(mimsem_ctx* c, int nlev, double ca, double cb, double* x, long long xs, double* r, double* d, long long vs);
int launch_sw_operator_precond(mimsem_ctx* c, int nlev, double a, double grav, double H, const double* f0, long long f0s,
                               const double* B, const double* x, long long xs, double* z, long long zs,
                               const double** unassembled = nullptr /* nlev == 1: skip the 1-form gather of z, return the element-local results */);
int launch_halo_pack(mimsem_ctx* c, const int* idx, int count, int nlev, const double* v, long long vs, double* buf);
int launch_halo_unpack(mimsem_ctx* c, const int* idx, int count, int nlev, int mode, const double* buf, double* v, long long vs);

// column_kernels.hip internals used by api.hip
int mimsem_block_inverse_inplace(mimsem_ctx* c, long long nblocks, int n, double* blocks, int* err = nullptr);
int mimsem_colop_block_inverse_apply(mimsem_ctx* c, int op, int geom_lev0, int nlev, double scale, unsigned flags,
                                     const double* f, long long fs, const double* x, long long xs,
                                     double* y, long long ys, double alpha);
