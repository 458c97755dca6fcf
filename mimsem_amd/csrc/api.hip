// mimsem_amd/csrc/api.hip -- C-ABI entry points of libmimsem_hip.so (include/mimsem_hip.h):
// context lifetime, HBM layout, scatter-add plans, horizontal-operator dispatch.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <cstring>
#include "ctx.hpp"
#include "wave_balance.hpp"

namespace mimsem {
thread_local std::string g_last_hip_error;
int hip_fail(hipError_t e, const char* what) {
    g_last_hip_error = std::string(what) + ": " + hipGetErrorString(e);
    return MIMSEM_ERR_HIP;
}
}  // namespace mimsem

namespace {

template <class T>
int upload(T** dst, const T* src, size_t count, mimsem_ctx* c) {
    if (int rc = c->alloc((void**)dst, count*sizeof(T))) return rc;
    if (count) MIMSEM_HIP_TRY(hipMemcpy(*dst, src, count*sizeof(T), hipMemcpyHostToDevice));
    return MIMSEM_OK;
}

// slot -> list of element-local result positions, ascending element order (deterministic sums)
int build_plan(int nslots, int nEl, int per_el, const std::vector<const int*>& maps, const std::vector<int>& offs,
               int counts, int K, std::vector<int>& plan) {
    plan.assign((size_t)nslots*K, -1);
    std::vector<int> fill(nslots, 0);
    for (int e = 0; e < nEl; e++)
        for (size_t m = 0; m < maps.size(); m++)
            for (int j = 0; j < counts; j++) {
                const int s = maps[m][(size_t)e*counts + j];
                if (s < 0 || s >= nslots) return MIMSEM_ERR_ARG;
                if (fill[s] >= K) return MIMSEM_ERR_UNSUPPORTED;
                plan[(size_t)s*K + fill[s]++] = e*per_el + offs[m] + j;
            }
    return MIMSEM_OK;
}

// Element groups (= workgroups of the fused kernel) grown greedily over shared edge slots, and the group-local
// slot tables: a slot whose every contributor sits in one group is summed in LDS and written once; the others
// ("perimeter") leave one partial sum per group and are finished by k_gather_perim.
struct FusedPlan {
    int ngroups = 0, lmax = 0, nps = 0, npart = 0;
    std::vector<int> perm, fslot, fcnt, pslot, ppart;
    std::vector<unsigned short> lid;
};
int build_fused_plan(int n1, int nEl, int n1e, int G, const int* ix, const int* iy, FusedPlan& P) {
    const int nd = 2*n1e;
    auto slot_of = [&](int e, int j) { return j < n1e ? ix[(size_t)e*n1e + j] : iy[(size_t)e*n1e + j - n1e]; };
    std::vector<int> own((size_t)n1*2, -1), cnt(n1, 0);
    for (int e = 0; e < nEl; e++) for (int j = 0; j < nd; j++) {
        const int s = slot_of(e, j);
        if (cnt[s] >= 2) return MIMSEM_ERR_UNSUPPORTED;
        own[(size_t)s*2 + cnt[s]++] = e;
    }
    P.ngroups = (nEl + G - 1)/G; P.lmax = G*nd;
    P.perm.assign((size_t)P.ngroups*G, -1);
    std::vector<char> assigned(nEl, 0);
    std::vector<int> score(nEl, 0), touched;
    int next_seed = 0;
    for (int g = 0; g < P.ngroups; g++) {
        for (int t : touched) score[t] = 0;
        touched.clear();
        for (int k = 0; k < G; k++) {
            int best = -1;
            for (int t : touched) if (!assigned[t] && (best < 0 || score[t] > score[best] || (score[t] == score[best] && t < best))) best = t;
            if (best < 0) { while (next_seed < nEl && assigned[next_seed]) next_seed++; if (next_seed >= nEl) break; best = next_seed; }
            assigned[best] = 1; P.perm[(size_t)g*G + k] = best;
            for (int j = 0; j < nd; j++) {
                const int s = slot_of(best, j);
                for (int w = 0; w < 2; w++) { const int o = own[(size_t)s*2 + w]; if (o >= 0 && o != best && !assigned[o]) { if (!score[o]) touched.push_back(o); score[o]++; } }
            }
        }
    }
    // per group: its distinct slots in ASCENDING slot order (coalesced write-out); for each the one or two
    // element-local result positions (k*nd + j inside the group) that feed it, in element order
    P.lid.assign((size_t)P.ngroups*P.lmax*2, 0xFFFF);
    P.fslot.assign((size_t)P.ngroups*P.lmax, 0); P.fcnt.assign(P.ngroups, 0);
    std::vector<int> part((size_t)n1*2, -1);
    std::vector<int> ingroup(n1, 0);
    for (int g = 0; g < P.ngroups; g++) {
        std::vector<std::pair<int, int>> contrib;                      // (slot, position in group)
        for (int k = 0; k < G; k++) { const int e = P.perm[(size_t)g*G + k]; if (e < 0) continue;
            for (int j = 0; j < nd; j++) { const int s = slot_of(e, j); ingroup[s]++; contrib.push_back({s, k*nd + j}); } }
        std::sort(contrib.begin(), contrib.end());
        int nl = 0;
        for (size_t i = 0; i < contrib.size(); ) {
            const int s = contrib[i].first;
            size_t j = i; while (j < contrib.size() && contrib[j].first == s) j++;
            P.lid[((size_t)g*P.lmax + nl)*2 + 0] = (unsigned short)contrib[i].second;
            if (j - i > 1) P.lid[((size_t)g*P.lmax + nl)*2 + 1] = (unsigned short)contrib[i + 1].second;
            if (ingroup[s] == cnt[s]) P.fslot[(size_t)g*P.lmax + nl] = s;
            else { const int pi = P.npart++; P.fslot[(size_t)g*P.lmax + nl] = -(pi + 1);
                   if (part[(size_t)s*2] < 0) part[(size_t)s*2] = pi; else part[(size_t)s*2 + 1] = pi; }
            nl++; i = j;
        }
        P.fcnt[g] = nl;
        for (auto& c2 : contrib) ingroup[c2.first] = 0;
    }
    for (int s = 0; s < n1; s++) if (part[(size_t)s*2] >= 0) { P.pslot.push_back(s); P.ppart.push_back(part[(size_t)s*2]); P.ppart.push_back(part[(size_t)s*2 + 1]); }
    P.nps = (int)P.pslot.size();
    return MIMSEM_OK;
}

// Wave-groups of the wave-level fused kernel (k_apply_wave): G = 64/LPE elements grown over shared edge slots so that they form a
// compact patch (2 x 2 at p <= 3: the candidate sharing the most slots with the group wins, ties go to a neighbour of the SEED, which
// turns the third pick perpendicular to the second and lets the fourth close the square), and per group three lane tables.  The
// element kernels are bound by the number of vector-memory instructions a wave issues (TA/TD busy 85 %, profiles/r02_umat_pmc.txt),
// so both tables are built around 16-BYTE accesses:
//   load pairs : the group's distinct slots covered by aligned pairs {2k, 2k+1} (the reference numbers an element's x- and y-edge
//                DoFs alternately, so a pair is usually two wanted values): ONE dwordx4 load per level brings every DoF of the
//                group; each loaded value is staged to the one or two elements that use it.
//   store pairs: a pair of slots that are both COMPLETE in the group (every contributor inside it) is summed in LDS and written
//                once, straight into y, as one 16-byte store; so is a complete slot whose pair partner is a perimeter slot of the same
//                group (the partner's half of the store carries 0 and is overwritten by the perimeter pass later in the stream);
//                every other slot of the group (its perimeter, and complete slots whose partner is outside the group) leaves a
//                partial sum in a densely packed row of the workspace -- again in pairs -- that k_wave_perim finishes.
//                MIMSEM_WAVE_SINGLES=1: no mixed pairs, unpaired complete slots in a second, 8-byte store round instead.
constexpr int WMP = 16;     // entries of a side (its slots, padded): 8 pairs x 8 levels x 2 parts = two 64-lane rounds of the finishing phase
constexpr int WNS = 8;      // sides a wave-group can take part in
struct WavePlan {
    int ngroups = 0, nps = 0, npart = 0, npwritten = 0, nsing = 0, ndirect = 0, nbgroups = 0, nbrec = 0, nsides = 0;
    bool fin_ok = true;
    std::vector<int> perm, pslot, ppart, node, sslot;
    std::vector<int4> lane, plan;
    std::vector<int2> sing;
    std::vector<int4> fin;
    // round 5, tile mode: four consecutive wave-groups = one workgroup = a tile; the partial sums of the slots two groups of a tile share
    // meet in the workgroup's LDS instead of the workspace (tfin: [ntiles][WTF] {slot, LDS position of part A, of part B, 0}, -1 padded)
    int ntiles = 0, tpmax = 0, ninner = 0;
    std::vector<int4> tfin;
};
constexpr int WTF = MIMSEM_WTF;      // finishing entries a tile can hold (4 x 4 elements at p = 3: 24 inner slots)
constexpr int WTP = MIMSEM_WTP;      // doubles of a tile's LDS row (pairs of partial sums)
// Round 3: the partial sums are laid out per SIDE -- the (<= WMP) perimeter slots two wave-groups share, in ascending slot order; row
// of a level = [side][part A (lower group) | part B][WMP] -- so that whichever group reaches a side second can finish its slots inside
// the same launch (elem_wave.inc, finishing phase): no second kernel, no second trip of the partial sums through HBM.  A complete
// slot that cannot be written in a 16-byte pair (its partner lies outside the group) rides along as an extra entry of one of the
// group's sides (the other part of that entry is written as 0).  The perimeter records (k_wave_perim: split applies, MIMSEM_WAVE_FIN=0)
// address the same layout.
int build_wave_plan(int order, int n1, int nEl, int n1e, int n0e, int G, const int* ix, const int* iy, const int* i0, bool singles, bool mixed,
                    const char* marked /* [n1] halo slots or null */, WavePlan& P, bool tile = false) {
    const int nd = 2*n1e, lpe = 64/G, mp1 = order + 1;
    const int RS = mp1 + (mp1 & 1), XT = n1e + mp1*RS, sxe0 = XT + 2*(lpe - n1e), SXE = sxe0 + (sxe0 & 1);     // as k_apply_wave
    const unsigned NACC = (unsigned)(G*nd), ZERO = NACC + 128, DUMPX = (unsigned)XT;
    if (G*SXE > 0xFFFE || n1 < 2) return MIMSEM_ERR_UNSUPPORTED;
    auto slot_of = [&](int e, int j) { return j < n1e ? ix[(size_t)e*n1e + j] : iy[(size_t)e*n1e + j - n1e]; };
    auto xpos = [&](int k, int j) { return (unsigned)(k*SXE + (j < n1e ? j : n1e + ((j - n1e)/order)*RS + (j - n1e)%order)); };
    std::vector<int> own((size_t)n1*2, -1), cnt(n1, 0);
    for (int e = 0; e < nEl; e++) for (int j = 0; j < nd; j++) {
        const int s = slot_of(e, j);
        if (s < 0 || s >= n1) return MIMSEM_ERR_ARG;
        if (cnt[s] >= 2) return MIMSEM_ERR_UNSUPPORTED;
        own[(size_t)s*2 + cnt[s]++] = e;
    }
    P.ngroups = (nEl + G - 1)/G;
    P.perm.assign((size_t)P.ngroups*G, -1);
    std::vector<char> assigned(nEl, 0), seedn(nEl, 0);
    std::vector<int> score(nEl, 0), touched;
    int next_seed = 0;
    for (int g = 0; g < P.ngroups; g++) {
        for (int t : touched) { score[t] = 0; seedn[t] = 0; }
        touched.clear();
        for (int k = 0; k < G; k++) {
            int best = -1;
            auto better = [&](int t, int b) {
                if (score[t] != score[b]) return score[t] > score[b];
                if (seedn[t] != seedn[b]) return seedn[t] > seedn[b];
                return t < b; };
            for (int t : touched) if (!assigned[t] && (best < 0 || better(t, best))) best = t;
            if (best < 0) { while (next_seed < nEl && assigned[next_seed]) next_seed++; if (next_seed >= nEl) break; best = next_seed; }
            assigned[best] = 1; P.perm[(size_t)g*G + k] = best;
            for (int j = 0; j < nd; j++) {
                const int s = slot_of(best, j);
                for (int w = 0; w < 2; w++) {
                    const int o = own[(size_t)s*2 + w];
                    if (o >= 0 && o != best && !assigned[o]) { if (!score[o]) touched.push_back(o); score[o]++; if (k == 0) seedn[o] = 1; }
                }
            }
        }
    }
    // interior / boundary split (mimsem_ctx_set_halo_slots): groups that touch a slot taking part in a halo exchange come FIRST, so
    // that "the boundary part" of an apply is a prefix of the launch (and a prefix of the perimeter records, below)
    P.nbgroups = 0;
    if (marked) {
        std::vector<int> bnd, inn;
        for (int g = 0; g < P.ngroups; g++) {
            bool b = false;
            for (int k = 0; k < G && !b; k++) { const int e = P.perm[(size_t)g*G + k]; if (e < 0) continue;
                for (int j = 0; j < nd && !b; j++) b = marked[slot_of(e, j)] != 0; }
            (b ? bnd : inn).push_back(g);
        }
        std::vector<int> perm2; perm2.reserve(P.perm.size());
        for (int g : bnd) perm2.insert(perm2.end(), P.perm.begin() + (size_t)g*G, P.perm.begin() + (size_t)(g + 1)*G);
        for (int g : inn) perm2.insert(perm2.end(), P.perm.begin() + (size_t)g*G, P.perm.begin() + (size_t)(g + 1)*G);
        P.perm.swap(perm2); P.nbgroups = (int)bnd.size();
    }
    // ---- tile mode (round 5): wave-groups in fours, each four = the wavefronts of one workgroup.  Grown over the group adjacency (shared
    // perimeter slots) with one step of look-ahead so that the fours come out as 2 x 2 squares of groups where the mesh allows (a square
    // keeps 4 sides inside, a line of four only 3); a four that cannot be filled is padded with empty groups.
    tile = tile && mixed && !singles && !marked;
    if (tile) {
        std::vector<int> g0(nEl, -1);
        for (int g = 0; g < P.ngroups; g++) for (int k = 0; k < G; k++) { const int e = P.perm[(size_t)g*G + k]; if (e >= 0) g0[e] = g; }
        std::vector<std::vector<std::pair<int, int>>> adj(P.ngroups);       // (neighbour group, shared slots)
        {
            std::vector<std::pair<std::pair<int, int>, int>> pr;
            for (int sl = 0; sl < n1; sl++) if (cnt[sl] == 2) {
                const int a = g0[own[(size_t)sl*2]], b = g0[own[(size_t)sl*2 + 1]];
                if (a != b) { pr.push_back({{a, b}, 1}); pr.push_back({{b, a}, 1}); }
            }
            std::sort(pr.begin(), pr.end());
            for (size_t i = 0; i < pr.size();) { size_t j = i; while (j < pr.size() && pr[j].first == pr[i].first) j++;
                adj[pr[i].first.first].push_back({pr[i].first.second, (int)(j - i)}); i = j; }
        }
        std::vector<char> done(P.ngroups, 0);
        auto shared_with = [&](const std::vector<int>& t, int h) { int w = 0; for (int m : t) for (auto& e : adj[m]) if (e.first == h) w += e.second; return w; };
        std::vector<int> perm2;
        for (int seed = 0; seed < P.ngroups; seed++) {
            if (done[seed]) continue;
            std::vector<int> t{seed}; done[seed] = 1;
            while ((int)t.size() < 4) {
                int best = -1, bw = 0, bl = -1;
                for (int m : t) for (auto& e : adj[m]) {
                    const int h = e.first;
                    if (done[h]) continue;
                    const int w = shared_with(t, h);
                    int look = 0;                                       // the most a fourth / next group could share with the tile grown by h
                    if ((int)t.size() < 3) { std::vector<int> t2(t); t2.push_back(h);
                        for (int m2 : t2) for (auto& e2 : adj[m2]) if (!done[e2.first] && e2.first != h) look = std::max(look, shared_with(t2, e2.first)); }
                    if (w > bw || (w == bw && look > bl) || (w == bw && look == bl && h < best)) { best = h; bw = w; bl = look; }
                }
                if (best < 0) break;
                t.push_back(best); done[best] = 1;
            }
            for (int m : t) perm2.insert(perm2.end(), P.perm.begin() + (size_t)m*G, P.perm.begin() + (size_t)(m + 1)*G);
            for (int k = (int)t.size(); k < 4; k++) perm2.insert(perm2.end(), (size_t)G, -1);
            P.ntiles++;
        }
        P.perm.swap(perm2); P.ngroups = 4*P.ntiles;
    }
    std::vector<int> grp(nEl, -1);
    for (int g = 0; g < P.ngroups; g++) for (int k = 0; k < G; k++) { const int e = P.perm[(size_t)g*G + k]; if (e >= 0) grp[e] = g; }
    P.lane.assign((size_t)P.ngroups*64, int4{0, 0, 0, 0});
    P.plan.resize((size_t)P.ngroups*64);
    P.node.resize((size_t)P.ngroups*64);
    if (singles) P.sing.assign((size_t)P.ngroups*64, int2{-1, (int)(ZERO | (ZERO << 16))});
    struct Use { int nx = 0; unsigned x[2] = {0, 0}; int na = 0; unsigned a[2] = {0, 0}; };      // staging / result positions of a slot in the group
    std::vector<Use> use(n1);
    std::vector<std::vector<int4>> entries(P.ngroups);
    std::vector<std::vector<int>> extras(P.ngroups), gsides(P.ngroups), routed_of(P.ngroups);
    // the slots of group g with their positions in its staging / result strips (filled, used, cleared per group)
    auto mark_group = [&](int g, std::vector<int>& slots) {
        slots.clear();
        for (int k = 0; k < G; k++) { const int e = P.perm[(size_t)g*G + k]; if (e < 0) continue;
            for (int j = 0; j < nd; j++) {
                const int s = slot_of(e, j); Use& u = use[s];
                if (!u.nx) slots.push_back(s);
                u.x[u.nx++] = xpos(k, j); u.a[u.na++] = (unsigned)(k*nd + j);
            } }
        std::sort(slots.begin(), slots.end());
    };
    auto in_group = [&](int s) { return s >= 0 && s < n1 && use[s].nx > 0; };
    auto complete = [&](int s) { return in_group(s) && use[s].nx == cnt[s]; };
    auto xpack = [&](int s) { unsigned a0 = DUMPX, a1 = DUMPX; if (in_group(s)) { a0 = use[s].x[0]; if (use[s].nx > 1) a1 = use[s].x[1]; } return (int)(a0 | (a1 << 16)); };
    auto apack = [&](int s) { unsigned a0 = ZERO, a1 = ZERO; if (in_group(s)) { a0 = use[s].a[0]; if (use[s].na > 1) a1 = use[s].a[1]; } return (int)(a0 | (a1 << 16)); };
    // sides: (lower group, upper group) -> the perimeter slots they share
    std::vector<std::pair<std::pair<int, int>, int>> shared;               // ((gA, gB), slot): every perimeter slot is reported by both groups
    std::vector<int> slots;
    for (int g = 0; g < P.ngroups; g++) {
        mark_group(g, slots);
        // lane table: element + node slot of every lane, load pair of the first lanes
        for (int l = 0; l < 64; l++) {
            const int pe = P.perm[(size_t)g*G + l/lpe], e = pe >= 0 ? pe : 0, q = l%lpe;
            P.lane[(size_t)g*64 + l] = int4{e, 0, (int)(DUMPX | (DUMPX << 16)), (int)(DUMPX | (DUMPX << 16))};
            P.node[(size_t)g*64 + l] = i0[(size_t)e*n0e + std::min(q, n0e - 1)];
        }
        int nload = 0; int last = -1;
        for (int s : slots) {
            if (s <= last) continue;                                  // covered by the previous pair
            int b = s & ~1; if (b + 1 >= n1) b = n1 - 2;
            if (nload >= 64) return MIMSEM_ERR_UNSUPPORTED;
            int4& L = P.lane[(size_t)g*64 + nload++];
            L.y = b; L.z = xpack(b); L.w = xpack(b + 1);
            last = b + 1;
        }
        for (int l = nload; l < 64 && nload; l++) P.lane[(size_t)g*64 + l].y = P.lane[(size_t)g*64].y;   // idle loader lanes re-read the first pair
        // store pairs written straight into y
        std::vector<int> routed;
        for (size_t i = 0; i < slots.size(); i++) {
            const int s = slots[i];
            if (!(s & 1) && s + 1 < n1 && complete(s) && complete(s + 1)) { entries[g].push_back(int4{s, apack(s), apack(s + 1), 0}); P.ndirect += 2; i++; continue; }
            if (mixed && !(s & 1) && in_group(s + 1) && complete(s) != complete(s + 1) && !singles) {
                // MIXED pair (MIMSEM_WAVE_MIXED=1: round 2's form, perimeter pass only), both slots in the group: the complete one is
                // written in a full 16-byte store whose other half carries 0 (accumulate form: adds 0).  That half belongs to a
                // perimeter slot NO group writes directly -- its value comes from k_wave_perim, strictly later in the stream --, so the
                // store clobbers nothing.  Inside ONE launch nothing orders that 0 -- dirty in the storing XCD's L2 until the kernel
                // ends -- before the value a finishing wave on another XCD writes: with the finishing phase such a complete slot rides
                // through the side as an extra entry instead.  (A complete slot whose partner is not in the group at all stays
                // routed: the partner may be written directly by its own group at the same time.)
                const int zz = (int)(ZERO | (ZERO << 16));
                entries[g].push_back(int4{s, complete(s) ? apack(s) : zz, complete(s + 1) ? apack(s + 1) : zz, 0});
                P.ndirect += 1;
                routed.push_back(complete(s) ? s + 1 : s);
                i++; continue;
            }
            routed.push_back(s);
        }
        if (singles) {                                                 // complete slots without a complete partner: 8-byte stores
            std::vector<int> keep; int ns = 0;
            for (int s : routed) {
                if (complete(s)) { if (ns >= 64) return MIMSEM_ERR_UNSUPPORTED; P.sing[(size_t)g*64 + ns++] = int2{s, apack(s)}; }
                else keep.push_back(s);
            }
            routed.swap(keep); P.nsing += ns; P.ndirect += ns;
        }
        routed_of[g] = routed;
        for (int s : routed) {
            if (mixed) break;                                          // dense layout below: no sides
            if (complete(s)) { extras[g].push_back(s); continue; }
            int go = -1;
            for (int w = 0; w < 2; w++) { const int o = own[(size_t)s*2 + w]; if (o >= 0 && grp[o] != g) go = grp[o]; }
            if (go < 0) return MIMSEM_ERR_STATE;                       // (cannot happen: an incomplete slot has a contributor elsewhere)
            shared.push_back({{std::min(g, go), std::max(g, go)}, s});
        }
        for (int s : slots) use[s] = Use();
    }
    std::sort(shared.begin(), shared.end());
    shared.erase(std::unique(shared.begin(), shared.end()), shared.end());
    struct Side { int ga, gb; std::vector<int> slots; };
    std::vector<Side> sides;
    for (size_t i = 0; i < shared.size(); i++) {
        const bool fresh = sides.empty() || sides.back().ga != shared[i].first.first || sides.back().gb != shared[i].first.second ||
                           (int)sides.back().slots.size() >= WMP;
        if (fresh) { sides.push_back(Side{shared[i].first.first, shared[i].first.second, {}});
                     gsides[shared[i].first.first].push_back((int)sides.size() - 1); gsides[shared[i].first.second].push_back((int)sides.size() - 1); }
        sides.back().slots.push_back(shared[i].second);
    }
    for (int g = 0; g < P.ngroups; g++)
        for (int s : extras[g]) {
            int sd = -1;
            for (int t : gsides[g]) if ((int)sides[t].slots.size() < WMP) { sd = t; break; }
            if (sd < 0) { sides.push_back(Side{g, -1, {}}); sd = (int)sides.size() - 1; gsides[g].push_back(sd); }     // a side of the group's own
            sides[sd].slots.push_back(s);
        }
    P.nsides = (int)sides.size();
    P.npart = P.nsides*2*WMP;
    P.sslot.assign((size_t)P.nsides*WMP, -1);
    P.fin.assign((size_t)P.ngroups*WNS, int4{-1, 0, 0, 0});
    std::vector<int> part((size_t)n1*2, -1);
    for (int t = 0; t < P.nsides; t++)
        for (size_t j = 0; j < sides[t].slots.size(); j++) P.sslot[(size_t)t*WMP + j] = sides[t].slots[j];
    if (mixed) {
        // round 2's dense layout (the default: the perimeter pass finishes every slot): the routed slots of a group in pairs, one after
        // the other in the row -- 26 values in three cache lines per group and level
        P.npart = 0;
        std::vector<int> tpos(std::max(P.ntiles, 1), 0), tpart;             // doubles used in a tile's LDS row; LDS positions of an inner slot's two parts
        if (tile) { tpart.assign((size_t)n1*2, -1); P.tfin.assign((size_t)P.ntiles*WTF, int4{-1, 0, 0, 0}); }
        std::vector<int> tcount(std::max(P.ntiles, 1), 0);
        for (int g = 0; g < P.ngroups; g++) {
            if (routed_of[g].empty()) continue;
            mark_group(g, slots);
            std::vector<int> routed, inner;
            for (int s : routed_of[g]) {
                bool in = false;
                if (tile && cnt[s] == 2) { const int a = grp[own[(size_t)s*2]], b = grp[own[(size_t)s*2 + 1]]; in = a != b && a/4 == b/4; }
                (in ? inner : routed).push_back(s);
            }
            for (size_t i = 0; i < routed.size(); i += 2) {
                const int s0 = routed[i], s1 = i + 1 < routed.size() ? routed[i + 1] : -1;
                const int pi = P.npart; P.npart += 2; P.npwritten += 2;
                auto reg = [&](int s, int idx) { if (s < 0) return; if (part[(size_t)s*2] < 0) part[(size_t)s*2] = idx; else part[(size_t)s*2 + 1] = idx; };
                reg(s0, pi); reg(s1, pi + 1);
                entries[g].push_back(int4{-(pi + 2), apack(s0), apack(s1), 0});
            }
            // the slots this group shares with another group of its tile: pairs of partial sums into the tile's LDS row (w = position + 1;
            // x = INT_MIN: the lane's global store goes to the dump tail)
            const int T = g/4;
            for (size_t i = 0; i < inner.size(); i += 2) {
                const int s0 = inner[i], s1 = i + 1 < inner.size() ? inner[i + 1] : -1;
                const int tp = tpos[T]; tpos[T] += 2;
                if (tpos[T] > WTP) return MIMSEM_ERR_UNSUPPORTED;
                auto reg = [&](int s, int pos) {
                    if (s < 0) return;
                    if (tpart[(size_t)s*2] < 0) { tpart[(size_t)s*2] = pos; return; }
                    if (tcount[T] >= WTF) return;                         // (checked below)
                    P.tfin[(size_t)T*WTF + tcount[T]] = int4{s, tpart[(size_t)s*2], pos, 0};       // part A = the lower group, as in the perimeter pass
                    tcount[T]++; P.ninner++;
                };
                reg(s0, tp); reg(s1, tp + 1);
                entries[g].push_back(int4{INT_MIN, apack(s0), apack(s1), tp + 1});
            }
            if (entries[g].size() > 64) return MIMSEM_ERR_UNSUPPORTED;
            for (int s : slots) use[s] = Use();
        }
        if (tile) {
            for (int T = 0; T < P.ntiles; T++) { if (tcount[T] >= WTF) return MIMSEM_ERR_UNSUPPORTED; P.tpmax = std::max(P.tpmax, tpos[T]); }
            for (int s = 0; s < n1; s++) if (tpart[(size_t)s*2] >= 0) {       // every inner slot must have found its second part
                bool found = false;
                for (int k = 0; k < WTF && !found; k++) { const int4& r = P.tfin[(size_t)(grp[own[(size_t)s*2]]/4)*WTF + k]; found = r.x == s; }
                if (!found) return MIMSEM_ERR_STATE;
            }
        }
    }
    for (int g = 0; g < P.ngroups && !mixed; g++) {
        if ((int)gsides[g].size() > WNS) P.fin_ok = false;
        if (gsides[g].empty()) continue;
        mark_group(g, slots);
        for (size_t k = 0; k < gsides[g].size(); k++) {
            const int t = gsides[g][k]; const Side& S = sides[t];
            const int base = t*2*WMP + (g == S.ga ? 0 : WMP);
            if (k < (size_t)WNS) P.fin[(size_t)g*WNS + k] = int4{t, S.gb < 0 ? 1 : 2, (int)S.slots.size(), 0};
            // the whole 128-byte part, padding included, by ONE store instruction (8 lanes x 16 bytes): a full line travels to the
            // uncached row as one write -- partial-line writes are read-modify-writes at the memory side (measured: 23 scattered
            // 16-byte pairs per group and level made the launch 3x slower)
            size_t need = 0;                                              // (groups with many sides: no room for the padding pairs)
            for (size_t k2 = k; k2 < gsides[g].size(); k2++) need += (sides[gsides[g][k2]].slots.size() + 1)/2;
            const bool whole = entries[g].size() + (gsides[g].size() - k)*(WMP/2) <= 64 || entries[g].size() + need + (WMP/2 - (S.slots.size() + 1)/2) > 64 ? 
                               entries[g].size() + (gsides[g].size() - k)*(WMP/2) <= 64 : false;
            for (size_t j = 0; j < (whole ? (size_t)WMP : S.slots.size()); j += 2) {
                const int s0 = j < S.slots.size() ? S.slots[j] : -1, s1 = j + 1 < S.slots.size() ? S.slots[j + 1] : -1;
                entries[g].push_back(int4{-(base + (int)j + 2), apack(s0), apack(s1), 0});     // a slot the group has no share of: 0
                if (s0 >= 0) P.npwritten += 2;
            }
            for (size_t j = 0; j < S.slots.size(); j++)
                if (in_group(S.slots[j])) { const int s = S.slots[j], idx = base + (int)j;
                    if (part[(size_t)s*2] < 0) part[(size_t)s*2] = idx;
                    else if (idx < part[(size_t)s*2]) { part[(size_t)s*2 + 1] = part[(size_t)s*2]; part[(size_t)s*2] = idx; }
                    else part[(size_t)s*2 + 1] = idx; }               // part A first: the perimeter pass and the finishing phase add A + B
        }
        if (entries[g].size() > 64) return MIMSEM_ERR_UNSUPPORTED;
        for (int s : slots) use[s] = Use();
    }
    // unused lanes REPEAT one of the group's own entries (same address, same value: the duplicates merge in the store instruction and
    // touch no extra cache line); a group without any entry (padding only) stores into the dump tail of the partial-sum row
    for (int g = 0; g < P.ngroups; g++) {
        const int ne = (int)entries[g].size();
        for (int t = 0; t < 64; t++)
            P.plan[(size_t)g*64 + t] = ne ? entries[g][t%ne]
                                          : int4{-(P.npart + 2*t + 2), (int)(ZERO | (ZERO << 16)), (int)(ZERO | (ZERO << 16)), 0};
    }
    // perimeter records: those of marked (halo) slots first; inside each segment in SLOT order (coalesced y accesses; ordering by
    // the first partial sum instead was measured: the pass went from 30 to 38 us on the 829 440-unit launch)
    P.nbrec = 0;
    for (int pass = 0; pass < 2; pass++) {
        std::vector<std::pair<int, int>> seg;                         // (first partial or INT_MAX, slot)
        for (int s = 0; s < n1; s++) {
            const bool m = marked && marked[s];
            if ((pass == 0) != m) continue;
            if (cnt[s] == 0) P.fin_ok = false;                        // a slot no element touches: only the perimeter pass zeroes it
            if (part[(size_t)s*2] >= 0 || cnt[s] == 0) seg.push_back({s, s});
        }
        std::sort(seg.begin(), seg.end());
        for (auto& e : seg) { const int s = e.second; P.pslot.push_back(s); P.ppart.push_back(part[(size_t)s*2]); P.ppart.push_back(part[(size_t)s*2 + 1]); }
        if (pass == 0) P.nbrec = (int)seg.size();
    }
    P.nps = (int)P.pslot.size();
    if (singles || mixed) P.fin_ok = false;
    return MIMSEM_OK;
}

// Owner-computes form (k_apply_wave<3, UMAT, LCT, ACCUM, false, true>, p = 3): every aligned store pair {2k, 2k+1} gets exactly ONE
// owner group, and the owner computes the contribution of a neighbour element to the pair's slots itself, so that it writes the FINISHED
// value straight into y -- no partial sums, no perimeter pass.  At p = 3 the quadrature points are the GLL nodes: an edge slot on a side
// of an element depends on the 4 points of that side only (its 3 side DoFs, the 12 cross-edge DoFs of the point rows, metric and thickInv
// at the 4 points).  A "ghost side" = (neighbour element, which of its 4 sides); the kernel computes its 4 points on PACKED ghost lanes:
// per level one DPP row of the x-normal sides (side = column, point = row) and one of the y-normal sides (point = column, side = row),
// so that the along-side operations are the element's own.  Side block b = the side's index in the group's list.
//   gh [g][32] lane of the x-normal row (qy*4 + qx = point*4 + side), then of the y-normal row (side*4 + point): {metric record of the
//              neighbour's point (wave-group order), element*16 + point, its qy0 (x-normal: qx0) = 3 << 1 | the point has no side
//              DoF << 2, position b*16 + point*4 of its quadruple in the gathered strip | its result position (b*4 + point; an idle
//              lane: 16 + its lane of the row) << 8}
//   gx [g][64] slot gathered into position b*16 + point*4 + t of the level's strip (one 8-byte gather per lane and level): t < 3 the
//              point's cross-edge DoFs in the order the neighbour's fma chain reads them, t = 3 the point's DoF on the side
// The side's slots come out of the ghost lanes with the bits of the neighbour's own lanes; the owner's store pair adds them to its own
// contribution (position WGR + b*4 + point of the level's strip).
// FOUR-LEVEL pass (own4::k_apply_wave, LCT = 8): a group has at most 4 ghost sides whatever their kinds, so side b takes DPP row b and
// the row's other direction holds the four levels m of a DOUBLE batch -- x-normal: lane point*4 + m, y-normal: lane m*4 + point, the
// point along the side where the element keeps that point's coefficients, as above.  One pass serves two batches.
//   gh4 [g][64] lane b*16 + (point, m): {metric record, element*16 + point, y-normal | qy0 (qx0) = 3 << 1 | no side DoF << 2 | idle
//               lane << 3, position of the quadruple | result position b*4 + point << 8}; gx and the store entries are shared
constexpr int WGX = MIMSEM_WGX;     // gathered DoFs of a group: 16 per ghost side
constexpr int WGS = 4;              // ghost sides of a group: 16-position blocks of the gathered strip
struct WaveOwn {
    std::vector<int4> plan, gh, gh4; std::vector<int> gx;
    int ndirect = 0, nsides = 0, maxsides = 0, maxgx = 0, nfull = 0;      // nfull: groups with 4 ghost sides of both kinds
    int mix[4] = {0, 0, 0, 0};          // groups by their x-normal + y-normal ghost sides: 2 + 2, 4 + 0, 0 + 4, anything else
};
int build_wave_own(int order, int n1, int nEl, int n1e, int G, const int* ix, const int* iy, const WavePlan& P, WaveOwn& W) {
    if (order != 3 || G != 4 || n1e != 12 || (n1 & 1) || P.ntiles || P.nbgroups) return MIMSEM_ERR_UNSUPPORTED;
    const int nd = 2*n1e, lpe = 16;
    const unsigned ZERO = (unsigned)(G*nd + 128), WGR = (unsigned)(G*nd + 136);      // as k_apply_wave: the strip's zero, ghost results
    auto slot_of = [&](int e, int j) { return j < n1e ? ix[(size_t)e*n1e + j] : iy[(size_t)e*n1e + j - n1e]; };
    std::vector<int> own((size_t)n1*2, -1), ownj((size_t)n1*2, -1), cnt(n1, 0), grp(nEl, -1), kin(nEl, -1);
    for (int e = 0; e < nEl; e++) for (int j = 0; j < nd; j++) {
        const int s = slot_of(e, j);
        if (s < 0 || s >= n1 || cnt[s] >= 2) return MIMSEM_ERR_UNSUPPORTED;
        own[(size_t)s*2 + cnt[s]] = e; ownj[(size_t)s*2 + cnt[s]] = j; cnt[s]++;
    }
    for (int s = 0; s < n1; s++) if (!cnt[s]) return MIMSEM_ERR_UNSUPPORTED;      // a slot nobody touches: only the perimeter pass zeroes it
    for (int g = 0; g < P.ngroups; g++) for (int k = 0; k < G; k++) { const int e = P.perm[(size_t)g*G + k]; if (e >= 0) { grp[e] = g; kin[e] = k; } }
    // side of local DoF j (-1: interior).  Sides: 0 / 1 the x-normal ones at qx = 0 / 3 (x-edge DoFs j = row*4 + col), 2 / 3 the
    // y-normal ones at qy = 0 / 3 (y-edge DoFs j - 12 = row*3 + col)
    auto side_of = [&](int j) {
        if (j < n1e) { const int col = j%4; return col == 0 ? 0 : (col == 3 ? 1 : -1); }
        const int row = (j - n1e)/3; return row == 0 ? 2 : (row == 3 ? 3 : -1);
    };
    // ---- ownership: the candidate owners of a pair are the groups of its contributors; the one needing the fewest new ghost sides
    // wins (then the one with fewer sides so far, then the lower group) ----
    std::vector<std::vector<int>> gsides(P.ngroups);            // ghost side keys e*4 + side
    std::vector<int> owner(n1/2, -1);
    auto need = [&](int p, int g, int* keys) {                  // new ghost sides pair p needs in group g (-1: impossible)
        int nk = 0;
        for (int t = 0; t < 4; t++) {
            const int s = 2*p + t/2, e = own[(size_t)s*2 + t%2]; if (e < 0 || grp[e] == g) continue;
            const int sd = side_of(ownj[(size_t)s*2 + t%2]);
            if (sd < 0) return -1;
            const int key = e*4 + sd;
            if (std::find(gsides[g].begin(), gsides[g].end(), key) == gsides[g].end() && std::find(keys, keys + nk, key) == keys + nk) keys[nk++] = key;
        }
        return nk;
    };
    for (int p = 0; p < n1/2; p++) {
        int best = -1, bnew = 0, bsz = 0, keys[4];
        for (int c = 0; c < 4; c++) {
            const int e = own[(size_t)(2*p + c/2)*2 + c%2]; if (e < 0) continue;
            const int g = grp[e], nnew = need(p, g, keys), sz = (int)gsides[g].size();
            if (nnew < 0 || sz + nnew > WGS) continue;
            if (best < 0 || nnew < bnew || (nnew == bnew && (sz < bsz || (sz == bsz && g < best)))) { best = g; bnew = nnew; bsz = sz; }
        }
        if (best < 0) return MIMSEM_ERR_UNSUPPORTED;           // (a numbering this form does not fit: the caller keeps the two launches)
        owner[p] = best;
        const int nnew = need(p, best, keys);
        gsides[best].insert(gsides[best].end(), keys, keys + nnew);
    }
    // ---- per group: ghost rows, gathered DoFs, store entries ----
    W.plan.assign((size_t)P.ngroups*64, int4{0, 0, 0, 0});
    W.gh.assign((size_t)P.ngroups*32, int4{0, 0, 0, 0});
    W.gh4.assign((size_t)P.ngroups*64, int4{0, 0, 0, 0});
    W.gx.assign((size_t)P.ngroups*64, 0);
    std::vector<std::vector<int>> owned(P.ngroups);
    for (int p = 0; p < n1/2; p++) owned[owner[p]].push_back(p);
    for (int g = 0; g < P.ngroups; g++) {
        std::vector<int>& sides = gsides[g];
        std::sort(sides.begin(), sides.end());
        const int e0 = std::max(P.perm[(size_t)g*G], 0);
        const int lane0slot = P.lane[(size_t)g*64].y;
        for (int l = 0; l < 32; l++)                               // idle lanes: points of the group's first element, results into a dump
            W.gh[(size_t)g*32 + l] = int4{g*64 + l%lpe, e0*lpe + l%lpe, 0, (16 + l%lpe) << 8};
        for (int l = 0; l < 64; l++) W.gh4[(size_t)g*64 + l] = int4{g*64 + l%lpe, e0*lpe + l%lpe, 8, 0};
        int nxs = 0, nys = 0;                                      // x-normal sides (columns of their row), y-normal ones (rows)
        for (int l = 0; l < 64; l++) W.gx[(size_t)g*64 + l] = lane0slot;     // positions nobody reads re-read a pair of the group
        for (size_t si = 0; si < sides.size(); si++) {
            const int e = sides[si]/4, sd = sides[si]%4;
            const bool yn = sd >= 2; const int c0 = (sd & 1) ? 3 : 0;          // qx0 (x-normal) or qy0 (y-normal)
            for (int pt = 0; pt < 4; pt++) {
                const int q = yn ? c0*4 + pt : pt*4 + c0;                       // the neighbour's lane of the side point
                const int l = yn ? 16 + nys*4 + pt : pt*4 + nxs;
                W.gh[(size_t)g*32 + l] = int4{grp[e]*64 + kin[e]*lpe + q, e*lpe + q, (c0 == 3 ? 2 : 0) | (!yn && pt == 3 ? 4 : 0),
                                              (int)(si*16 + pt*4) | (int)(si*4 + pt) << 8};
                for (int m = 0; m < 4; m++)                                     // the four-level pass: row si, the levels across the side
                    W.gh4[(size_t)g*64 + si*16 + (yn ? m*4 + pt : pt*4 + m)] =
                        int4{grp[e]*64 + kin[e]*lpe + q, e*lpe + q, (yn ? 1 : 0) | (c0 == 3 ? 2 : 0) | (!yn && pt == 3 ? 4 : 0),
                             (int)(si*16 + pt*4) | (int)(si*4 + pt) << 8};
                int* gxp = &W.gx[(size_t)g*64 + si*16 + pt*4];
                for (int t = 0; t < 3; t++) {
                    // x-normal: Y(t, pt) for t = 0, 1, 2 (dpp_quad order); y-normal: X(pt, row) in dpp_rows rotation order from row c0
                    // (the row-3 zero dropped): rows 0, 2, 1 (c0 = 0) or 2, 1, 0 (c0 = 3)
                    const int row = c0 == 0 ? (t == 0 ? 0 : 3 - t) : 2 - t;
                    gxp[t] = yn ? slot_of(e, row*4 + pt) : slot_of(e, n1e + pt*3 + t);
                }
                if (pt < 3) gxp[3] = yn ? slot_of(e, n1e + c0*3 + pt) : slot_of(e, pt*4 + c0);
            }
            (yn ? nys : nxs)++;
        }
        // store entries of the owned pairs; a contribution from outside the group comes from a lane of its ghost row
        std::vector<int4> ent;
        auto contrib = [&](int s, int w) -> unsigned {
            const int e = own[(size_t)s*2 + w]; if (e < 0) return ZERO;
            const int j = ownj[(size_t)s*2 + w];
            if (grp[e] == g) return (unsigned)(kin[e]*nd + j);
            const int si = (int)(std::find(sides.begin(), sides.end(), e*4 + side_of(j)) - sides.begin());
            const int pt = j < n1e ? j/4 : (j - n1e)%3;      // the DoF's point along the side: its ghost lane holds the result
            return WGR + (unsigned)(si*4 + pt);
        };
        for (int p : owned[g]) {
            ent.push_back(int4{2*p, (int)(contrib(2*p, 0) | contrib(2*p, 1) << 16), (int)(contrib(2*p + 1, 0) | contrib(2*p + 1, 1) << 16), 0});
            W.ndirect += 2;
        }
        // unused lanes repeat one of the group's own entries (same address, same value); a group owning no pair is not expected
        if (ent.empty() || ent.size() > 64) return MIMSEM_ERR_UNSUPPORTED;
        for (int t = 0; t < 64; t++) W.plan[(size_t)g*64 + t] = ent[t%ent.size()];
        W.nsides += (int)sides.size(); W.maxsides = std::max(W.maxsides, (int)sides.size());
        if (sides.size() == 4 && nxs > 0 && nys > 0) W.nfull++;
        W.mix[nxs == 2 && nys == 2 ? 0 : (nxs == 4 && nys == 0 ? 1 : (nxs == 0 && nys == 4 ? 2 : 3))]++;
        W.maxgx = std::max(W.maxgx, 16*(int)sides.size());
    }
    return MIMSEM_OK;
}

// levels per work item of the element kernel: keep >= ~6 workgroups per CU in flight, otherwise amortise as much as possible
int level_chunk(const mimsem_ctx* c, int nlev) {
    const ElemSizes& es = c->es;
    const int epb = 256/(es.mp12 <= 4 ? 4 : (es.mp12 <= 16 ? 16 : (es.mp12 <= 32 ? 32 : 64)));
    const long long blocks1 = ((long long)c->nEl + epb - 1)/epb;          // workgroups per single level
    long long lch = (blocks1*nlev)/(256*6);
    if (lch < 1) lch = 1;
    if (lch > nlev) lch = nlev;
    if (lch > 8) lch = 8;
    if (c->lch_override > 0) lch = std::min(c->lch_override, nlev);
    return (int)std::max(1LL, lch);
}

// levels per work item of the wave-level kernel: its compile-time bound WLC = 8 whenever the call has that many levels.  A wavefront's
// fixed costs (kernel arguments, tables, metric, the dispatch of the wave itself: ~25 cycles per wave and XCD) are what the
// 103 680-unit launch is made of (scripts/wave_size_sweep.py, s_memtime stamps of scripts/stamp_wave.sh), and the chunk form computes
// all WLC levels of a work item whether the chunk has them or not -- so: as many levels per wave as there are.  (The owner-computes
// form walks level ranges instead: wave_level_parts.)
int wave_level_chunk(const mimsem_ctx* c, int nlev) {
    if (c->wave_lch > 0) return std::max(1, std::min(std::min(c->wave_lch, 8), nlev));
    return std::max(1, std::min(8, nlev));
}

// chunks of 8 levels one wavefront works through (tables and metric loaded once, the level pipeline running on across the chunk
// boundary): as many as leave ~2 wavefronts per SIMD -- fewer, longer-lived waves cost less dispatch and set-up, which is what the
// cache-resident launches are made of
int wave_chunks_per_item(const mimsem_ctx* c, int nlev, int lch, int ngroups) {
    const int nch = (nlev + lch - 1)/lch;
    if (lch != 8 || nch <= 1) return 1;
    if (c->wave_cpp > 0) return std::min(c->wave_cpp, nch);
    int nparts = std::min(nch, std::max(1, (1536 + ngroups - 1)/std::max(ngroups, 1)));
    // EQUAL parts where the chunk count allows: the launch ends with its longest work item (p = 4 box, 8 chunks: 3 parts of 3 + 3 + 2
    // chunks took 17.2 us, 4 parts of 2 take 14.0 us -- round 3)
    for (int np = nparts; np <= nch; np++) if (nch%np == 0) { nparts = np; break; }
    return (nch + nparts - 1)/nparts;
}

// Level RANGES of the owner-computes form (round 10): every group is cut into `np` parts of whole level pairs, and the kernel walks
// exactly the batches a part has (elem_wave.inc: the wavefront ends behind its last batch), so no batch is computed for nothing.
// By default the parts ARE the chunk form's work items -- first level k L, L = wave_level_chunk x wave_chunks_per_item levels, the last
// one whatever is left (30 levels on 864 groups: 16 + 14; 11 levels: 8 + 3; 30 levels on 6 912 groups: one part of 30) -- so a context
// reports one number of levels per item (mimsem_op_wave_stats out[4]) whichever of its two forms runs, and the two rules move together
// or not at all.  Measured on the 864-group sphere x 30 levels (profiles/r10_wave_ranges_ab.txt, us per back-to-back step):
// 30: 15.5, 16 + 14: 12.8, 10 x 3: 12.5, 8 + 8 + 8 + 6: 14.1, 6 x 5: 14.6.
// A requested part length (mimsem_ctx_set_wave_split; MIMSEM_WAVE_LCH x MIMSEM_WAVE_CPP in the experiments build) is dealt EVENLY
// instead: ceil(pairs / pairs of the request) parts whose lengths differ by at most one pair, the longer ones first (an odd nlev leaves
// the last part one level short) -- 10 + 10 + 10, 8 + 8 + 8 + 6, and 33 levels by 8 as 8 + 8 + 6 + 6 + 5.
struct WaveParts { int np, pb, pr, longest; };     // parts per group, level pairs of a part, parts that hold one pair more, levels of the longest part
WaveParts wave_level_parts(const mimsem_ctx* c, int nlev, int ngroups) {
    const int pairs = (nlev + 1)/2;
    const int lch = wave_level_chunk(c, nlev);
    const int asked = c->wave_part > 0 ? c->wave_part : ((c->wave_lch > 0 || c->wave_cpp > 0) ? lch*std::max(c->wave_cpp, 1) : 0);
    const int tp = ((asked > 0 ? asked : lch*wave_chunks_per_item(c, nlev, lch, ngroups)) + 1)/2;      // pairs of a full part, >= 1
    WaveParts w;
    w.np = (pairs + tp - 1)/tp;
    if (asked > 0) { w.pb = pairs/w.np; w.pr = pairs%w.np; }
    else           { w.pb = tp; w.pr = 0; }
    w.longest = std::min(nlev, 2*(w.pb + (w.pr ? 1 : 0)));
    return w;
}

// BALANCED level ranges (wave_balance.hpp): the default rule deals whole parts, wnw to a workgroup, and the workgroups land 1 or 2 to a CU
// (864 groups x 30 levels: 432 on 256 CUs, the launch ending with the CUs that hold 120 wave-levels of a mean of 101).  Where the
// default rule's workgroups are all resident at once (at most 3 per CU: the register bound) and are no multiple of the CU count, the
// planner deals bal_k x CUs workgroups of equal level-pair totals instead.  Not for a requested split, single-level calls or a call
// that does not cover all the groups of the plan (the parts of a boundary / interior apply).  Returns the number of workgroups to plan,
// 0: the default rule.
int wave_balance_workgroups(const mimsem_ctx* c, int nlev, int ngroups, const WaveParts& wp) {
    if (!c->wv.own || ngroups != c->wv.ngroups) return 0;
    const int ncu = c->bal_ncu > 0 ? c->bal_ncu : (c->bal_ncu == 0 ? c->dev_ncu : 0);
    if (ncu < 1 || nlev < 2 || c->wave_part > 0 || c->wave_lch > 0 || c->wave_cpp > 0) return 0;
    const int wnw = wave_workgroup_waves();
    const long long wgs = ((long long)ngroups*wp.np + wnw - 1)/wnw;
    if (wgs > 3LL*ncu || wgs%ncu == 0 || (long long)c->bal_k*ncu >= (1LL << 24)) return 0;
    return c->bal_k*ncu;
}
// the context's list for that call, or null: none yet.  A list depends on (levels, groups, workgroups) alone -- its items name groups by
// index -- so it outlives mimsem_ctx_set_levels, a re-plan and the setter, and the cache holds one list per triple ever asked for.
const mimsem_ctx::BalList* wave_balance_find(const mimsem_ctx* c, int nlev, int ngroups, int nwg) {
    for (const mimsem_ctx::BalList& b : c->bal) if (b.nlev == nlev && b.ngroups == ngroups && b.nwg == nwg) return &b;
    return nullptr;
}
// ... planned and uploaded (never inside a capture: the caller has looked).  A count the planner refuses is remembered as an empty list.
int wave_balance_make(mimsem_ctx* c, int nlev, int ngroups, int nwg, const WaveParts& wp) {
    std::vector<mimsem::WaveItem> items;
    mimsem_ctx::BalList b{nlev, ngroups, nwg, nullptr, 0, 0};
    if (mimsem::plan_wave_balance(ngroups, nlev, wave_workgroup_waves(), nwg, wp.longest, items) == mimsem::WAVE_BALANCE_OK) {
        std::vector<int4> rec(items.size());
        for (size_t i = 0; i < items.size(); i++) {
            rec[i] = int4{items[i].group, items[i].lev0, items[i].lev0 + items[i].nlev, 0};
            b.longest = std::max(b.longest, items[i].nlev);
        }
        int4* d = nullptr;
        if (int rc = upload(&d, rec.data(), rec.size(), c)) return rc;
        b.items = d; b.nitems = (int)rec.size();
    }
    c->bal.push_back(b);
    return MIMSEM_OK;
}

int op_spaces(int op, int* in, int* cf, int* out) {
    switch (op) {
    case MIMSEM_OP_UMAT: case MIMSEM_OP_UTMAT:   *in = 1; *cf = -1; *out = 1; return 0;
    case MIMSEM_OP_UHMAT: case MIMSEM_OP_UTMAT_H: *in = 1; *cf = 2; *out = 1; return 0;
    case MIMSEM_OP_ROTMAT:  *in = 1; *cf = 0; *out = 1; return 0;
    case MIMSEM_OP_WMAT: case MIMSEM_OP_WMATINV:  *in = 2; *cf = -1; *out = 2; return 0;
    case MIMSEM_OP_WHMAT: case MIMSEM_OP_WHMATINV: *in = 2; *cf = 2; *out = 2; return 0;
    case MIMSEM_OP_PMAT:    *in = 0; *cf = -1; *out = 0; return 0;
    case MIMSEM_OP_PHMAT:   *in = 0; *cf = 2; *out = 0; return 0;
    case MIMSEM_OP_WTQUMAT: case MIMSEM_OP_WTQDUDZ: *in = 1; *cf = 1; *out = 2; return 0;
    case MIMSEM_OP_UTQWMAT: *in = 2; *cf = 1; *out = 1; return 0;
    case MIMSEM_OP_WTQ: *in = 3; *cf = -1; *out = 2; return 0;
    case MIMSEM_OP_PTQ: *in = 3; *cf = -1; *out = 0; return 0;
    case MIMSEM_OP_UTQ: *in = 3; *cf = -1; *out = 1; return 0;
    case MIMSEM_OP_PHMAT_UP:  *in = 0; *cf = 2; *out = 0; return 0;
    case MIMSEM_OP_ROTMAT_UP: *in = 1; *cf = 0; *out = 1; return 0;
    case MIMSEM_OP_UMAT_UP:   *in = 1; *cf = 1; *out = 1; return 0;
    case MIMSEM_OP_UHMAT_UP: case MIMSEM_OP_UVEC_HU_UP: case MIMSEM_OP_UMAT_RAY: case MIMSEM_OP_UMAT_FRIC: *in = 1; *cf = 2; *out = 1; return 0;
    }
    return 1;
}

}  // namespace

// The context's device memory (ctx.hpp: one owner).  The count is the bytes asked for; an empty table still gets an address.
int mimsem_ctx::alloc(void** p, size_t nbytes, Mem kind) {
    void* q = nullptr;
    const size_t sz = std::max<size_t>(nbytes, 1);
    if (kind == Mem::Plain) MIMSEM_HIP_TRY(hipMalloc(&q, sz));
    else MIMSEM_HIP_TRY(hipExtMallocWithFlags(&q, sz, kind == Mem::FineGrained ? hipDeviceMallocFinegrained : hipDeviceMallocUncached));
    adopt(q, nbytes);
    *p = q;
    return MIMSEM_OK;
}
void mimsem_ctx::release(void* p) {
    const auto it = std::find_if(owned.begin(), owned.end(), [p](const std::pair<void*, size_t>& o) { return o.first == p; });
    if (it == owned.end()) return;
    bytes -= (long long)it->second;
    owned.erase(it);
    (void)hipFree(p);
}
bool mimsem_ctx::is_capturing() const {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess) return false;
    return st != hipStreamCaptureStatusNone;
}
int mimsem_ctx::grow(double*& buf, long long& have, long long doubles, Mem kind) {
    if (doubles <= have) return MIMSEM_OK;
    if (is_capturing()) return MIMSEM_ERR_STATE;          // growing = hipMalloc, illegal on a capturing stream: warm up outside the capture
    if (int rc = alloc((void**)&buf, (size_t)doubles*sizeof(double), kind)) return rc;      // (on failure buf still names the old, smaller buffer)
    have = doubles;                                       // (the old buffer is retired: `owned` keeps it for the recordings that hold it)
    return MIMSEM_OK;
}
int mimsem_ctx::ensure_kry(long long doubles) {
    if (doubles <= kry_doubles) return MIMSEM_OK;
    if (int rc = grow(d_kry, kry_doubles, doubles)) return rc;
    if (!d_rdcnt) {                                                 // arrival counters of the one-launch rowdot: zeroed once, every call leaves them zero
        if (int rc = alloc((void**)&d_rdcnt, MIMSEM_RD_COUNTERS*sizeof(unsigned))) return rc;
        MIMSEM_HIP_TRY(hipMemsetAsync(d_rdcnt, 0, MIMSEM_RD_COUNTERS*sizeof(unsigned), stream));
    }
    return MIMSEM_OK;
}

hipEvent_t mimsem_ctx::next_event() {
    if (ev_used == ev_pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); ev_pool.push_back(e); }
    return ev_pool[ev_used++];
}

// packed metric of the wave kernel: {gaa, gab, gbb, 1/det} = Q/det J^T J per quadrature point (16-byte loads) and the
// rotational factor (-J00 J11 + J01 J10) Q/det of RotMat, in wave-group order
static void pack_wave_metric(const mimsem_ctx* c, const WavePlan& P, int lpe, std::vector<double>& G, std::vector<double>& Rv) {
    const ElemSizes& es = c->es;
    G.assign((size_t)P.ngroups*64*4, 0.0); Rv.assign((size_t)P.ngroups*64, 0.0);
    const int gsz = 64/lpe;
    for (int g = 0; g < P.ngroups; g++)
        for (int l = 0; l < 64; l++) {
            const int e = P.perm[(size_t)g*gsz + l/lpe], q = l%lpe;
            if (e < 0 || q >= es.mp12) continue;                 // padding element / lane beyond the point grid: zeros
            const double* Jq = c->h_J.data() + ((size_t)e*es.mp12 + q)*4;
            const double det = c->h_det[(size_t)e*es.mp12 + q];
            const double Q = c->tab.quad.w[q%es.mp1]*c->tab.quad.w[q/es.mp1];
            double* o = &G[((size_t)g*64 + l)*4];
            o[0] = (Jq[0]*Jq[0] + Jq[2]*Jq[2])*Q/det; o[1] = (Jq[0]*Jq[1] + Jq[2]*Jq[3])*Q/det;
            o[2] = (Jq[1]*Jq[1] + Jq[3]*Jq[3])*Q/det; o[3] = 1.0/det;
            Rv[(size_t)g*64 + l] = (-Jq[0]*Jq[3] + Jq[1]*Jq[2])*Q/det;
        }
}

// (re)build the wave-level plan of a context from its host copies of the mesh; `marked` [n1] flags the 1-form slots that take part
// in a halo exchange (null: none).  The context takes the new plan only when all of it is on the device (on failure it keeps the one it had);
// the tables of the plan it replaces are retired, not freed (a captured graph may still hold them).
static int setup_wave(mimsem_ctx* c, const char* marked) {
    const ElemSizes& es = c->es;
    WavePlan P;
    const int lpe = es.mp12 <= 4 ? 4 : (es.mp12 <= 16 ? 16 : (es.mp12 <= 32 ? 32 : 64));
    const bool singles = exp_env("MIMSEM_WAVE_SINGLES") && atoi(exp_env("MIMSEM_WAVE_SINGLES")) != 0;
    // MIMSEM_WAVE_FIN=1: the experimental in-kernel finishing phase (side layout of the partial sums, no mixed pairs); default: round 2's
    // dense layout with mixed pairs + the perimeter pass (measured faster: DESIGN 4.6)
    const bool want_fin = exp_env("MIMSEM_WAVE_FIN") && atoi(exp_env("MIMSEM_WAVE_FIN")) != 0;
    const bool mixed = !want_fin && !(exp_env("MIMSEM_WAVE_MIXED") && atoi(exp_env("MIMSEM_WAVE_MIXED")) == 0);
    // round 5: TILE mode -- four wave-groups per workgroup, the partial sums of the slots they share meet in LDS behind ONE barrier per work
    // item instead of travelling through the workspace to the perimeter pass (MIMSEM_WAVE_TILE=0 | 1; orders 3 and 4, no halo split)
    const bool want_tile = (es.n == 3 || es.n == 4) && !marked && exp_env("MIMSEM_WAVE_TILE") && atoi(exp_env("MIMSEM_WAVE_TILE")) != 0;
    int rc = build_wave_plan(es.n, c->n1, c->nEl, es.n1e, es.n0e, 64/lpe, c->h_i1x.data(), c->h_i1y.data(), c->h_i0.data(), singles, mixed, marked, P, want_tile);
    if (rc && want_tile) {                                             // a numbering the tiles do not fit: the plain plan
        P = WavePlan();
        rc = build_wave_plan(es.n, c->n1, c->nEl, es.n1e, es.n0e, 64/lpe, c->h_i1x.data(), c->h_i1y.data(), c->h_i0.data(), singles, mixed, marked, P, false);
    }
    if (rc) return rc;
    // owner-computes form on the same groups (Umat at p = 3, no halo split; MIMSEM_WAVE_OWN=0: today's two launches)
    WaveOwn W;
    const bool want_own = !marked && es.n == 3 && !want_fin && !want_tile && !singles && mixed &&
                          !(getenv("MIMSEM_WAVE_OWN") && atoi(getenv("MIMSEM_WAVE_OWN")) == 0);
    // ... and which ghost pass the LCT = 8 kernel runs: unset -- one pass per four levels (own4::k_apply_wave); MIMSEM_WAVE_OWN=1 -- the pass
    // per batch of two levels for every call (the A/B partner; single-level calls always run it)
    const bool own4 = !getenv("MIMSEM_WAVE_OWN");
    const bool own = want_own && build_wave_own(es.n, c->n1, c->nEl, es.n1e, 64/lpe, c->h_i1x.data(), c->h_i1y.data(), P, W) == MIMSEM_OK;
    WaveTables t;
    const size_t mark = c->owned.size();
    rc = [&]() -> int {
        int rc;
        if ((rc = upload(&t.lane, P.lane.data(), P.lane.size(), c))) return rc;
        if ((rc = upload(&t.plan, P.plan.data(), P.plan.size(), c))) return rc;
        std::vector<int4> rec(P.pslot.size());
        for (size_t i = 0; i < rec.size(); i++) rec[i] = int4{P.pslot[i], P.ppart[2*i], P.ppart[2*i + 1], 0};
        if ((rc = upload(&t.prec, rec.data(), rec.size(), c))) return rc;
        if ((rc = upload(&t.node, P.node.data(), P.node.size(), c))) return rc;
        if (own) {
            if ((rc = upload(&t.oplan, W.plan.data(), W.plan.size(), c))) return rc;
            if ((rc = upload(&t.gh, W.gh.data(), W.gh.size(), c))) return rc;
            if ((rc = upload(&t.gx, W.gx.data(), W.gx.size(), c))) return rc;
            if (own4 && (rc = upload(&t.gh4, W.gh4.data(), W.gh4.size(), c))) return rc;
        }
        if (P.nsing && (rc = upload(&t.sing, P.sing.data(), P.sing.size(), c))) return rc;
        if ((rc = upload(&t.fin, P.fin.data(), P.fin.size(), c))) return rc;
        if ((rc = upload(&t.sslot, P.sslot.data(), P.sslot.size(), c))) return rc;
        if (P.ntiles > 0 && (rc = upload(&t.tfin, P.tfin.data(), P.tfin.size(), c))) return rc;
        // arrival counters of the finishing phase: one per (side, work item of a group), zero between launches
        const size_t n = (size_t)std::max(P.nsides, 1)*(size_t)std::max(c->nk, 1);
        if ((rc = c->alloc((void**)&t.cnt, n*sizeof(int)))) return rc;
        MIMSEM_HIP_TRY(hipMemset(t.cnt, 0, n*sizeof(int)));
        std::vector<double> G, Rv;
        pack_wave_metric(c, P, lpe, G, Rv);
        if ((rc = upload(&t.G, G.data(), G.size(), c))) return rc;
        return upload(&t.R, Rv.data(), Rv.size(), c);
    }();
    if (rc) { while (c->owned.size() > mark) c->release(c->owned.back().first); return rc; }      // (nothing has seen these tables)
    t.on = true; t.own = own; t.can_fin = P.fin_ok && want_fin; t.split = marked != nullptr;
    t.ndirect = P.ndirect; t.ngroups = P.ngroups; t.nsing = P.nsing; t.nps = P.nps; t.npart = P.npart; t.npwritten = P.npwritten; t.nsides = P.nsides;
    if (P.ntiles > 0) { t.ntiles = P.ntiles; t.ninner = P.ninner; }
    t.nbgroups = P.nbgroups; t.nbrec = P.nbrec;
    c->wv = t;
    if (const char* kind = exp_env("MIMSEM_WPART_MEM")) c->w_partmem = !strcmp(kind, "plain") ? 2 : (!strcmp(kind, "finegrained") ? 1 : 0);
    if (const char* ev = exp_env("MIMSEM_WAVE_ORDER")) c->wave_order = atoi(ev);
    if (const char* ev = exp_env("MIMSEM_WAVE_LCH")) c->wave_lch = atoi(ev);
    if (const char* ev = exp_env("MIMSEM_WAVE_CPP")) c->wave_cpp = atoi(ev);
    if (const char* ev = exp_env("MIMSEM_WAVE2")) c->wave2_mode = atoi(ev);
    if (getenv("MIMSEM_VERBOSE"))
        fprintf(stderr, "[mimsem] wave plan: %d groups of %d elements (%d on the halo boundary), %d perimeter slots (%d partials in %d sides) of %d; "
                        "in-kernel finishing %s; tiles %d (%d inner slots finished in LDS, widest LDS row %d doubles)\n", P.ngroups, 64/lpe, P.nbgroups, P.nps,
                P.npwritten, P.nsides, c->n1, c->wv.can_fin ? "on" : "off", P.ntiles, P.ninner, P.tpmax);
    if (getenv("MIMSEM_VERBOSE") && own)
        fprintf(stderr, "[mimsem] owner-computes form: %d pairs, %d ghost sides (at most %d per group; %d groups with 4 of both kinds), "
                        "at most %d gathered DoFs per group; side mixes (x-normal + y-normal): %d groups 2 + 2, %d groups 4 + 0, %d groups 0 + 4, "
                        "%d other; ghost pass per %s\n", c->n1/2, W.nsides, W.maxsides, W.nfull, W.maxgx, W.mix[0], W.mix[1], W.mix[2], W.mix[3],
                own4 ? "four levels" : "batch");
    return MIMSEM_OK;
}

extern "C" {

int mimsem_ctx_set_profiling(mimsem_ctx* c, int on) {
    if (!c) return MIMSEM_ERR_ARG;
    // on = n > 0: time every n-th mimsem_op_apply (n = 1: all of them); 0 = off
    c->profiling = on != 0; c->prof_every = on > 0 ? on : 1; c->prof_count = 0; c->ev_used = 0; c->ev_has2.clear();
    // the events of the first ~128 sampled applies are created HERE, not inside the caller's timed region (bench.py's headline region used to pay
    // a hipEventCreate x 4 per sampled step: its `value` sat 10-18 % under the median of the unprofiled repeats of the same region)
    if (on) { MIMSEM_HIP_TRY(hipSetDevice(c->device)); while (c->ev_pool.size() < 512) { hipEvent_t e; MIMSEM_HIP_TRY(hipEventCreate(&e)); c->ev_pool.push_back(e); } }
    return MIMSEM_OK;
}
int mimsem_ctx_profile_read(mimsem_ctx* c, double* ms1, double* ms2, long long* launches) {
    if (!c) return MIMSEM_ERR_ARG;
    MIMSEM_HIP_TRY(hipStreamSynchronize(c->stream));
    double a = 0.0, b = 0.0;
    for (size_t i = 0; i + 3 < c->ev_used; i += 4) {
        float t = 0.f;
        MIMSEM_HIP_TRY(hipEventElapsedTime(&t, c->ev_pool[i], c->ev_pool[i + 1])); a += t;
        if (i/4 < c->ev_has2.size() && c->ev_has2[i/4]) {                                          // only when THIS apply recorded its second pair
            if (hipEventElapsedTime(&t, c->ev_pool[i + 2], c->ev_pool[i + 3]) == hipSuccess) b += t;
            else (void)hipGetLastError();
        }
    }
    if (ms1) *ms1 = a;
    if (ms2) *ms2 = b;
    if (launches) *launches = (long long)(c->ev_used/4);
    c->ev_used = 0; c->ev_has2.clear();
    return MIMSEM_OK;
}

int mimsem_abi_version(void) { return MIMSEM_ABI_VERSION; }
int mimsem_build_has_experiments(void) { return kExperiments ? 1 : 0; }

const char* mimsem_strerror(int code) {
    switch (code) {
    case MIMSEM_OK: return "ok";
    case MIMSEM_ERR_ARG: return "invalid argument";
    case MIMSEM_ERR_UNSUPPORTED: return "unsupported configuration (order must be 1..7 with quadrature order == element order)";
    case MIMSEM_ERR_HIP: return "HIP runtime error";
    case MIMSEM_ERR_STATE: return "context state does not allow this call";
    case MIMSEM_ERR_SINGULAR: return "singular block";
    }
    return "unknown error";
}
const char* mimsem_last_hip_error(void) { return mimsem::g_last_hip_error.c_str(); }

int mimsem_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mimsem_ctx_create(const mimsem_mesh_desc* d, int device, mimsem_ctx** out) {
    if (!d || !out) return MIMSEM_ERR_ARG;
    *out = nullptr;
    if (d->elOrd < 1 || d->elOrd > 7 || d->quadOrd != d->elOrd) return MIMSEM_ERR_UNSUPPORTED;
    if (d->nEl < 0 || d->nk < 1 || d->n0 < 0 || d->n1 < 0 || d->n2 < 0) return MIMSEM_ERR_ARG;
    if (!d->inds0 || !d->inds1x || !d->inds1y || !d->det || !d->J) return MIMSEM_ERR_ARG;
    MIMSEM_HIP_TRY(hipSetDevice(device));

    mimsem_ctx* c = new mimsem_ctx();
    c->device = device;
    {   // the CUs the balanced level ranges are dealt over (wave_balance_workgroups).  The form is OPT-IN (it did not separate from the
        // default rule on the headline step: DESIGN 4.8): MIMSEM_WAVE_BALANCE=k, k = 1 .. 3 workgroups per CU, or mimsem_ctx_set_wave_balance
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->dev_ncu = prop.multiProcessorCount;
        const char* ev = getenv("MIMSEM_WAVE_BALANCE");
        const int k = ev ? atoi(ev) : 0;
        if (k >= 1 && k <= 3) { c->bal_ncu = 0; c->bal_k = k; }
    }
    if (const char* ev = exp_env("MIMSEM_LCH")) c->lch_override = atoi(ev);
    if (const char* ev = exp_env("MIMSEM_NOSWZ")) c->swz = atoi(ev) ? 0 : 1;
    c->es = ElemSizes(d->elOrd);
    c->nEl = d->nEl; c->nk = d->nk; c->n0 = d->n0; c->n1 = d->n1; c->n2 = d->n2;
    const ElemSizes& es = c->es;
    if (!c->tab.init(d->elOrd, d->quadOrd) || !c->tab.collocated) { delete c; return MIMSEM_ERR_UNSUPPORTED; }
    if (d->n2 < d->nEl*es.n2e && !d->inds2) { delete c; return MIMSEM_ERR_ARG; }

    int rc = MIMSEM_OK;
    auto fail = [&](int code) { mimsem_ctx_destroy(c); return code; };
    if ((rc = upload(&c->d_E, c->tab.E.data(), c->tab.E.size(), c))) return fail(rc);
    if ((rc = upload(&c->d_w, c->tab.quad.w.data(), c->tab.quad.w.size(), c))) return fail(rc);
    if ((rc = upload(&c->d_xn, c->tab.nodes.x.data(), c->tab.nodes.x.size(), c))) return fail(rc);
    if ((rc = upload(&c->d_U, c->tab.U.data(), c->tab.U.size(), c))) return fail(rc);
    if ((rc = upload(&c->d_V, c->tab.V.data(), c->tab.V.size(), c))) return fail(rc);
    if ((rc = upload(&c->d_W, c->tab.W.data(), c->tab.W.size(), c))) return fail(rc);
    if ((rc = upload(&c->d_P, c->tab.P.data(), c->tab.P.size(), c))) return fail(rc);

    // metric: [e][q][4] -> component-major [e][4][q] so that one lane-per-point load is contiguous
    {
        std::vector<double> Js((size_t)d->nEl*4*es.mp12);
        for (int e = 0; e < d->nEl; e++)
            for (int q = 0; q < es.mp12; q++)
                for (int k = 0; k < 4; k++)
                    Js[((size_t)e*4 + k)*es.mp12 + q] = d->J[((size_t)e*es.mp12 + q)*4 + k];
        if ((rc = upload(&c->d_J, Js.data(), Js.size(), c))) return fail(rc);
    }
    if ((rc = upload(&c->d_det, d->det, (size_t)d->nEl*es.mp12, c))) return fail(rc);
    if ((rc = upload(&c->d_i0, d->inds0, (size_t)d->nEl*es.n0e, c))) return fail(rc);
    if ((rc = upload(&c->d_i1x, d->inds1x, (size_t)d->nEl*es.n1e, c))) return fail(rc);
    if ((rc = upload(&c->d_i1y, d->inds1y, (size_t)d->nEl*es.n1e, c))) return fail(rc);
    if (d->inds2) {
        bool contig = true;
        for (size_t i = 0; i < (size_t)d->nEl*es.n2e && contig; i++) contig = (d->inds2[i] == (int)i);
        for (size_t i = 0; i < (size_t)d->nEl*es.n2e; i++) if (d->inds2[i] < 0 || d->inds2[i] >= d->n2) return fail(MIMSEM_ERR_ARG);
        c->inds2_contig = contig;
        if (!contig && (rc = upload(&c->d_i2, d->inds2, (size_t)d->nEl*es.n2e, c))) return fail(rc);
    }

    if (d->indsq) {
        if (d->nq <= 0) return fail(MIMSEM_ERR_ARG);
        for (size_t i = 0; i < (size_t)d->nEl*es.mp12; i++) if (d->indsq[i] < 0 || d->indsq[i] >= d->nq) return fail(MIMSEM_ERR_ARG);
        c->nq = d->nq;
        if ((rc = upload(&c->d_iq, d->indsq, (size_t)d->nEl*es.mp12, c))) return fail(rc);
    }
    // scatter-add plans
    {
        std::vector<int> plan;
        rc = build_plan(d->n1, d->nEl, 2*es.n1e, {d->inds1x, d->inds1y}, {0, es.n1e}, es.n1e, 2, plan);
        if (rc) return fail(rc);
        if ((rc = upload(&c->d_g1, plan.data(), plan.size(), c))) return fail(rc);
        {
            // the block passes' own view of that plan (round 6, late): per (element, block row) {slot, first contributor, second contributor}
            // as ONE 16-byte entry -- the row's chain of dependent loads is {this entry -> the gathered values} instead of {edge map -> plan ->
            // values}; at the ~3 500 elements of the shallow-water drivers a block pass IS its chain of memory latencies
            const int nd = 2*es.n1e;
            std::vector<int> bp((size_t)d->nEl*nd*4, 0);
            for (int e = 0; e < d->nEl; e++)
                for (int r = 0; r < nd; r++) {
                    const int slot = r < es.n1e ? d->inds1x[(size_t)e*es.n1e + r] : d->inds1y[(size_t)e*es.n1e + r - es.n1e];
                    int* o = &bp[((size_t)e*nd + r)*4];
                    o[0] = slot; o[1] = plan[(size_t)slot*2]; o[2] = plan[(size_t)slot*2 + 1]; o[3] = 0;
                }
            if ((rc = upload(&c->d_bplan, bp.data(), bp.size(), c))) return fail(rc);
        }
        c->G0 = 4;
        rc = build_plan(d->n0, d->nEl, es.n0e, {d->inds0}, {0}, es.n0e, 4, plan);
        if (rc == MIMSEM_ERR_UNSUPPORTED) { c->G0 = 8; rc = build_plan(d->n0, d->nEl, es.n0e, {d->inds0}, {0}, es.n0e, 8, plan); }
        if (rc) return fail(rc);
        if ((rc = upload(&c->d_g0, plan.data(), plan.size(), c))) return fail(rc);
    }
    // direct-write tables: a DoF with a single contributing element needs no scatter-add at all
    {
        auto build = [&](int nslots, const std::vector<const int*>& maps, int counts, std::vector<std::vector<int>>& dir, std::vector<int>& shared) {
            std::vector<int> cnt(nslots, 0);
            for (const int* m : maps) for (size_t i = 0; i < (size_t)d->nEl*counts; i++) cnt[m[i]]++;
            dir.assign(maps.size(), std::vector<int>((size_t)d->nEl*counts));
            for (size_t k = 0; k < maps.size(); k++)
                for (size_t i = 0; i < (size_t)d->nEl*counts; i++) dir[k][i] = (cnt[maps[k][i]] == 1) ? maps[k][i] : -1;
            shared.clear();
            for (int sl = 0; sl < nslots; sl++) if (cnt[sl] != 1) shared.push_back(sl);     // incl. untouched slots (written as 0)
        };
        std::vector<std::vector<int>> dir; std::vector<int> sh;
        build(d->n1, {d->inds1x, d->inds1y}, es.n1e, dir, sh);
        if ((rc = upload(&c->d_d1x, dir[0].data(), dir[0].size(), c))) return fail(rc);
        if ((rc = upload(&c->d_d1y, dir[1].data(), dir[1].size(), c))) return fail(rc);
        if ((rc = upload(&c->d_sh1, sh.data(), sh.size(), c))) return fail(rc);
        c->nsh1 = (int)sh.size();
        build(d->n0, {d->inds0}, es.n0e, dir, sh);
        if ((rc = upload(&c->d_d0, dir[0].data(), dir[0].size(), c))) return fail(rc);
        if ((rc = upload(&c->d_sh0, sh.data(), sh.size(), c))) return fail(rc);
        c->nsh0 = (int)sh.size();
        // measured SLOWER on MI355X (pass 1 14.9 -> 17.4 us: the single-contributor stores are scattered, the ye stores coalesce;
        // pass 2 over the shared-slot list 7.4 -> 8.2 us), profiles/r01_direct_interior_ab.txt: opt-in only
        c->direct = exp_env("MIMSEM_DIRECT") != nullptr;
    }
    // Fused single-barrier scatter-add (group-local sums in LDS + perimeter pass): measured SLOWER than the two-pass
    // form on MI355X in round 1 (profiles/r01_fused_scatter_ab.txt), so it is opt-in (MIMSEM_FUSE=1) for further tuning.
    if (exp_env("MIMSEM_FUSE")) {
        FusedPlan P;
        const int epb = 256/(es.mp12 <= 4 ? 4 : (es.mp12 <= 16 ? 16 : (es.mp12 <= 32 ? 32 : 64)));
        rc = build_fused_plan(d->n1, d->nEl, es.n1e, epb, d->inds1x, d->inds1y, P);
        if (rc == MIMSEM_OK && P.lmax < 0x8000) {
            if ((rc = upload(&c->d_fperm, P.perm.data(), P.perm.size(), c))) return fail(rc);
            if ((rc = upload(&c->d_flid, P.lid.data(), P.lid.size(), c))) return fail(rc);
            if ((rc = upload(&c->d_fslot, P.fslot.data(), P.fslot.size(), c))) return fail(rc);
            if ((rc = upload(&c->d_fcnt, P.fcnt.data(), P.fcnt.size(), c))) return fail(rc);
            if ((rc = upload(&c->d_pslot, P.pslot.data(), P.pslot.size(), c))) return fail(rc);
            if ((rc = upload(&c->d_ppart, P.ppart.data(), P.ppart.size(), c))) return fail(rc);
            c->f_ngroups = P.ngroups; c->f_lmax = P.lmax; c->f_nps = P.nps; c->f_npart = P.npart; c->fused1 = true;
            if (getenv("MIMSEM_VERBOSE")) {
                long long tot = 0; for (int v : P.fcnt) tot += v;
                fprintf(stderr, "[mimsem] fused plan: %d groups of %d elements, %.1f local slots/group, %d perimeter slots (%d partials) of %d\n",
                        P.ngroups, epb, (double)tot/std::max(P.ngroups, 1), P.nps, P.npart, d->n1);
            }
        }
    }
    // Wave-level fused scatter-add of the 1-form -> 1-form operators (k_apply_wave): the default since round 2
    // (MIMSEM_WAVE=0 selects the two-pass form for every operator).  Host copies of the index maps and the metric stay with the
    // context: mimsem_ctx_set_halo_slots re-derives the plan with the boundary groups first.
    // block pass of the Chebyshev / Richardson sweeps on the matrix cores: the default at p = 4 (40 x 40 blocks: 32.1 us against 32.8 us for
    // the register-row form on the config-5 grid, profiles/r03_mfma_p4_ab.txt), off at p <= 3 (24 x 24: 25.3 against 23.8 us);
    // MIMSEM_BLOCKS_MFMA=0 | 1 overrides
    c->cheb_pend = exp_env("MIMSEM_CHEB_PEND") && atoi(exp_env("MIMSEM_CHEB_PEND")) != 0;
    c->blocks_mfma = exp_env("MIMSEM_BLOCKS_MFMA") ? atoi(exp_env("MIMSEM_BLOCKS_MFMA")) != 0 : es.n == 4;
    if (d->nEl > 0) { c->h_e1x.assign(d->inds1x, d->inds1x + (size_t)d->nEl*es.n1e); c->h_e1y.assign(d->inds1y, d->inds1y + (size_t)d->nEl*es.n1e);
                      c->h_e0.assign(d->inds0, d->inds0 + (size_t)d->nEl*es.n0e); }
    c->memset_node = exp_env("MIMSEM_MEMSET_NODE") && atoi(exp_env("MIMSEM_MEMSET_NODE")) != 0;      // (read once: mimsem_memset is a hot call of the recorded solves)
    c->rd_two = exp_env("MIMSEM_ROWDOT_TWO") && atoi(exp_env("MIMSEM_ROWDOT_TWO")) != 0;
    c->blu_stop = exp_env("MIMSEM_BLU_STOP") ? atoi(exp_env("MIMSEM_BLU_STOP")) : 0;
    c->pivot_fallback = getenv("MIMSEM_COLUMN_PIVOT_FALLBACK") ? std::min(2, std::max(0, atoi(getenv("MIMSEM_COLUMN_PIVOT_FALLBACK")))) : 1;      // on by default since round 5 (mimsem_column_set_pivot_fallback)
    if (!(getenv("MIMSEM_WAVE") && atoi(getenv("MIMSEM_WAVE")) == 0) && !c->fused1 && !c->direct && d->nEl > 0 && es.n <= 4) {
        c->h_i1x.assign(d->inds1x, d->inds1x + (size_t)d->nEl*es.n1e); c->h_i1y.assign(d->inds1y, d->inds1y + (size_t)d->nEl*es.n1e);
        c->h_i0.assign(d->inds0, d->inds0 + (size_t)d->nEl*es.n0e);
        c->h_J.assign(d->J, d->J + (size_t)d->nEl*es.mp12*4); c->h_det.assign(d->det, d->det + (size_t)d->nEl*es.mp12);
        rc = setup_wave(c, nullptr);
        if (rc == MIMSEM_ERR_ARG || rc == MIMSEM_ERR_HIP) return fail(rc);
        rc = MIMSEM_OK;
    }
    {
        const size_t cnt = (size_t)d->nk*d->nEl*es.mp12;
        if ((rc = c->alloc((void**)&c->d_th, cnt*sizeof(double))) || (rc = c->alloc((void**)&c->d_tI, cnt*sizeof(double)))) return fail(rc);
        if (es.n <= 4 && (rc = c->alloc((void**)&c->d_tIp, 2*(size_t)(d->nk/2 + 1)*d->nEl*es.mp12*2*sizeof(double)))) return fail(rc);
    }
    if ((rc = mimsem_ctx_set_levels(c, d->thick, d->thickInv))) return fail(rc);
    // two element-local buffers + one packed [1-form | 2-form] row per level: the largest request of any entry point at nlev <= nk
    if ((rc = c->ensure_ye((long long)d->nk*(2LL*d->nEl*std::max(2*es.n1e, es.n0e) + d->n1 + d->n2)))) return fail(rc);
    *out = c;
    return MIMSEM_OK;
}

struct mimsem_graph;
static void orphan_graphs(mimsem_ctx* c);
void mimsem_ctx_destroy(mimsem_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    orphan_graphs(c);
    for (const auto& o : c->owned) (void)hipFree(o.first);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->cap_stream) (void)hipStreamDestroy(c->cap_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->h_pin) (void)hipHostFree(c->h_pin);
    delete c;
}

int mimsem_ctx_set_stream(mimsem_ctx* c, void* s) {
    if (!c) return MIMSEM_ERR_ARG;
    if (c->cap_active) return MIMSEM_ERR_STATE;                          // (between mimsem_graph_begin and _end the stream is the capture's)
    c->stream = (hipStream_t)s;
    return MIMSEM_OK;
}
// a stream of the context's own for hosts that cannot create one (no HIP headers): non-blocking, so nothing this context launches orders itself
// against the legacy default stream any more
int mimsem_ctx_use_own_stream(mimsem_ctx* c) {
    if (!c) return MIMSEM_ERR_ARG;
    if (c->cap_active) return MIMSEM_ERR_STATE;
    MIMSEM_HIP_TRY(hipSetDevice(c->device));
    if (!c->own_stream) MIMSEM_HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    return MIMSEM_OK;
}
// ---- hipGraph capture for hosts without a HIP toolchain (include/mimsem_hip.h) -----------------------------------------------------
// A recording belongs to the context it was made on (advisor, round 5): it replays on the context's CURRENT stream -- so that "in stream order
// with the context's other work" stays true after mimsem_ctx_set_stream / _use_own_stream -- except that a recording made on the capture
// stream a default-stream context was lent keeps that stream (the legacy default stream cannot launch graphs in order with it either way);
// mimsem_ctx_destroy orphans the recordings still alive: their launch returns MIMSEM_ERR_STATE instead of using a destroyed stream.
struct mimsem_graph { hipGraph_t g = nullptr; hipGraphExec_t x = nullptr; hipStream_t stream = nullptr; int nodes = 0; mimsem_ctx* c = nullptr; bool lent = false; };
int mimsem_graph_begin(mimsem_ctx* c) {
    if (!c) return MIMSEM_ERR_ARG;
    if (c->cap_active || c->is_capturing()) return MIMSEM_ERR_STATE;
    MIMSEM_HIP_TRY(hipSetDevice(c->device));
    c->cap_swapped = false;
    if (c->stream == nullptr) {                                          // the legacy default stream cannot capture: a blocking stream of the
        if (!c->cap_stream) MIMSEM_HIP_TRY(hipStreamCreateWithFlags(&c->cap_stream, hipStreamDefault));   // context's own keeps its order with it
        c->cap_saved = c->stream; c->stream = c->cap_stream; c->cap_swapped = true;
    }
    const hipError_t he = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
    if (he != hipSuccess) {
        if (c->cap_swapped) { c->stream = c->cap_saved; c->cap_swapped = false; }
        return mimsem::hip_fail(he, "hipStreamBeginCapture");
    }
    c->cap_active = true;
    return MIMSEM_OK;
}
int mimsem_graph_end(mimsem_ctx* c, mimsem_graph** out) {
    if (!c || !out) return MIMSEM_ERR_ARG;
    if (!c->cap_active) return MIMSEM_ERR_STATE;
    *out = nullptr;
    hipGraph_t g = nullptr;
    const hipError_t he = hipStreamEndCapture(c->stream, &g);
    const hipStream_t used = c->stream;
    c->cap_active = false;
    if (c->cap_swapped) { c->stream = c->cap_saved; c->cap_swapped = false; }
    if (he != hipSuccess || !g) { (void)hipGetLastError(); return he == hipSuccess ? MIMSEM_ERR_STATE : mimsem::hip_fail(he, "hipStreamEndCapture"); }
    mimsem_graph* gr = new mimsem_graph();
    gr->g = g; gr->stream = used; gr->c = c; gr->lent = used != c->stream;
    size_t nn = 0;
    if (hipGraphGetNodes(g, nullptr, &nn) == hipSuccess) gr->nodes = (int)nn;
    const hipError_t hi = hipGraphInstantiate(&gr->x, g, nullptr, nullptr, 0);
    if (hi != hipSuccess) { (void)hipGraphDestroy(g); delete gr; return mimsem::hip_fail(hi, "hipGraphInstantiate"); }
    c->graphs.push_back(gr);
    *out = gr;
    return MIMSEM_OK;
}
int mimsem_graph_launch(mimsem_graph* g) {
    if (!g || !g->x) return MIMSEM_ERR_ARG;
    if (!g->c) return MIMSEM_ERR_STATE;                                  // its context is gone
    MIMSEM_HIP_TRY(hipGraphLaunch(g->x, (g->lent || g->c->stream == nullptr) ? g->stream : g->c->stream));
    return MIMSEM_OK;
}
int mimsem_graph_num_nodes(const mimsem_graph* g) { return g ? g->nodes : MIMSEM_ERR_ARG; }
static void orphan_graphs(mimsem_ctx* c) { for (void* p : c->graphs) ((mimsem_graph*)p)->c = nullptr; c->graphs.clear(); }
void mimsem_graph_destroy(mimsem_graph* g) {
    if (!g) return;
    if (g->c) { auto& v = g->c->graphs; v.erase(std::remove(v.begin(), v.end(), (void*)g), v.end()); }
    if (g->x) (void)hipGraphExecDestroy(g->x);
    if (g->g) (void)hipGraphDestroy(g->g);
    delete g;
}
int mimsem_ctx_sync(mimsem_ctx* c) { if (!c) return MIMSEM_ERR_ARG; MIMSEM_HIP_TRY(hipStreamSynchronize(c->stream)); return MIMSEM_OK; }
long long mimsem_ctx_workspace_bytes(const mimsem_ctx* c) { return c ? c->bytes : 0; }
int mimsem_op_level_chunk(const mimsem_ctx* c, int nlev) { return (c && nlev > 0) ? level_chunk(c, nlev) : MIMSEM_ERR_ARG; }
int mimsem_op_wave_stats(const mimsem_ctx* c, int nlev, int out[5]) {
    if (!c || !out || nlev < 1) return MIMSEM_ERR_ARG;
    for (int i = 0; i < 5; i++) out[i] = 0;
    if (!c->wv.on) return 0;
    out[0] = c->wv.ngroups; out[1] = c->wv.ndirect; out[2] = c->wv.npwritten; out[3] = c->wv.nps;
    if (c->wv.own) { out[1] = c->n1; out[2] = 0; out[3] = 0; }     // the headline operator's form: every slot written once, no partial sums
    if (c->wv.own && c->es.n == 3 && c->wv.ntiles == 0 && !c->d_tIn) {
        const WaveParts wp = wave_level_parts(c, nlev, c->wv.ngroups);
        out[4] = wp.longest;                              // the longest item's levels: of the default rule, or of the planned list once a call has made it
        const int nwg = c->wv.gh4 ? wave_balance_workgroups(c, nlev, c->wv.ngroups, wp) : 0;
        const mimsem_ctx::BalList* b = nwg > 0 ? wave_balance_find(c, nlev, c->wv.ngroups, nwg) : nullptr;
        if (b && b->items) out[4] = b->longest;
    }
    else { const int lch = wave_level_chunk(c, nlev); out[4] = lch*wave_chunks_per_item(c, nlev, lch, c->wv.ngroups); }
    return 1;
}

int mimsem_ctx_set_wave_split(mimsem_ctx* c, int part_levels, int order) {
    if (!c || part_levels < 0 || order < -1 || order > 3) return MIMSEM_ERR_ARG;
    if (c->is_capturing()) return MIMSEM_ERR_STATE;
    c->wave_part = part_levels;
    if (order >= 0) c->wave_order = order;
    return MIMSEM_OK;
}

int mimsem_ctx_set_level_chunk(mimsem_ctx* c, int lch) {
    if (!c || lch < 0 || lch > 8) return MIMSEM_ERR_ARG;
    if (c->is_capturing()) return MIMSEM_ERR_STATE;
    c->lch_override = lch;                                // (level_chunk, launch_blocks_apply, launch_owned_nd read it at every launch)
    return MIMSEM_OK;
}

int mimsem_ctx_set_wave_balance(mimsem_ctx* c, int ncu, int wgs_per_cu) {
    if (!c || ncu > (1 << 20) || (ncu >= 0 && (wgs_per_cu < 1 || wgs_per_cu > 3))) return MIMSEM_ERR_ARG;
    if (c->is_capturing()) return MIMSEM_ERR_STATE;
    c->bal_ncu = ncu < 0 ? -1 : ncu;
    if (ncu >= 0) c->bal_k = wgs_per_cu;
    return MIMSEM_OK;                                     // (the lists made so far stay: they are kept by workgroup count)
}
long long mimsem_ctx_wave_balance_launches(const mimsem_ctx* c) { return c ? c->bal_launches : MIMSEM_ERR_ARG; }

int mimsem_ctx_set_levels(mimsem_ctx* c, const double* thick, const double* thickInv) {
    if (!c) return MIMSEM_ERR_ARG;
    if (c->is_capturing()) return MIMSEM_ERR_STATE;
    MIMSEM_HIP_TRY(hipStreamSynchronize(c->stream));        // (a non-blocking stream does not order itself against the synchronous copies below)
    const size_t cnt = (size_t)c->nk*c->nEl*c->es.mp12;
    std::vector<double> th(cnt, 1.0), ti(cnt, 1.0);
    if (thick) std::memcpy(th.data(), thick, cnt*sizeof(double));
    if (thickInv) std::memcpy(ti.data(), thickInv, cnt*sizeof(double));
    else if (thick) for (size_t i = 0; i < cnt; i++) ti[i] = 1.0/th[i];     // Geom.cpp:761
    else if (false) {}
    if (cnt) {
        MIMSEM_HIP_TRY(hipMemcpy(c->d_th, th.data(), cnt*sizeof(double), hipMemcpyHostToDevice));
        MIMSEM_HIP_TRY(hipMemcpy(c->d_tI, ti.data(), cnt*sizeof(double), hipMemcpyHostToDevice));
    }
    if (cnt && c->d_tIp) {
        // level pairs for the wave-level kernels: entry (parity, m) holds levels L = 2m + parity and L + 1 (beyond the last level: the last again)
        const size_t row = (size_t)c->nEl*c->es.mp12, np = (size_t)c->nk/2 + 1;
        std::vector<double> tp(2*np*row*2);
        for (int par = 0; par < 2; par++) for (size_t m = 0; m < np; m++) {
            const size_t L0 = std::min<size_t>(2*m + par, c->nk - 1), L1 = std::min<size_t>(2*m + par + 1, c->nk - 1);
            double* o = tp.data() + ((size_t)par*np + m)*row*2;
            const double *a0 = ti.data() + L0*row, *a1 = ti.data() + L1*row;
            for (size_t i = 0; i < row; i++) { o[2*i] = a0[i]; o[2*i + 1] = a1[i]; }
        }
        MIMSEM_HIP_TRY(hipMemcpy(c->d_tIp, tp.data(), tp.size()*sizeof(double), hipMemcpyHostToDevice));
        // the same table per NODE (experiment, MIMSEM_WAVE_TNODE=1): the reference's thickInv lives on the nodes (eul/Geom.cpp:143-146, :761) and
        // the ABI takes it gathered per element: 16 values per element at p = 3 of which 9 are distinct per element on average.  Only when
        // every element holds the same bits at a shared node (and quadrature points are the nodes: mp12 == n0e)
        if (c->d_tIn) { c->release(c->d_tIn); c->d_tIn = nullptr; }
        if (exp_env("MIMSEM_WAVE_TNODE") && atoi(exp_env("MIMSEM_WAVE_TNODE")) == 1 && c->es.mp12 == c->es.n0e && !c->h_i0.empty() && c->n0 > 0) {
            const size_t n0 = (size_t)c->n0;
            std::vector<double> nod((size_t)c->nk*n0, 1.0), tn(2*np*n0*2, 1.0);
            std::vector<unsigned char> seen(n0);
            bool same = true;
            for (size_t L = 0; L < (size_t)c->nk && same; L++) {
                std::fill(seen.begin(), seen.end(), 0);
                const double* a0 = ti.data() + L*row;
                double* nl = nod.data() + L*n0;
                for (size_t i = 0; i < row; i++) {
                    const size_t nd = (size_t)c->h_i0[i];
                    if (nd >= n0 || (seen[nd] && std::memcmp(&nl[nd], &a0[i], 8))) { same = false; break; }
                    nl[nd] = a0[i]; seen[nd] = 1;
                }
            }
            for (int par = 0; par < 2 && same; par++) for (size_t m = 0; m < np; m++) {
                const size_t L0 = std::min<size_t>(2*m + par, c->nk - 1), L1 = std::min<size_t>(2*m + par + 1, c->nk - 1);
                double* o = tn.data() + ((size_t)par*np + m)*n0*2;
                for (size_t nd = 0; nd < n0; nd++) { o[2*nd] = nod[L0*n0 + nd]; o[2*nd + 1] = nod[L1*n0 + nd]; }
            }
            if (same) {
                if (int rc = c->alloc((void**)&c->d_tIn, tn.size()*sizeof(double))) return rc;
                MIMSEM_HIP_TRY(hipMemcpy(c->d_tIn, tn.data(), tn.size()*sizeof(double), hipMemcpyHostToDevice));
            }
        }
    }
    c->have_levels = (thick != nullptr) || (thickInv != nullptr);
    return MIMSEM_OK;
}

int mimsem_malloc(void** dev, long long bytes) {
    if (!dev || bytes < 0) return MIMSEM_ERR_ARG;
    MIMSEM_HIP_TRY(hipMalloc(dev, (size_t)std::max<long long>(bytes, 8)));
    return MIMSEM_OK;
}
int mimsem_free(void* dev) { if (dev) MIMSEM_HIP_TRY(hipFree(dev)); return MIMSEM_OK; }
int mimsem_memcpy_h2d(mimsem_ctx* c, void* dev, const void* host, long long bytes) {
    if (!c || !dev || !host || bytes < 0) return MIMSEM_ERR_ARG;
    MIMSEM_HIP_TRY(hipMemcpyAsync(dev, host, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    MIMSEM_HIP_TRY(hipStreamSynchronize(c->stream));
    return MIMSEM_OK;
}
int mimsem_memcpy_d2h(mimsem_ctx* c, void* host, const void* dev, long long bytes) {
    if (!c || !dev || !host || bytes < 0) return MIMSEM_ERR_ARG;
    if (bytes > 0 && bytes <= 4096 && !c->is_capturing()) {                   // a handful of scalars (check norms, counters): through pinned memory
        if (!c->h_pin) MIMSEM_HIP_TRY(hipHostMalloc(&c->h_pin, 4096, hipHostMallocDefault));
        MIMSEM_HIP_TRY(hipMemcpyAsync(c->h_pin, dev, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
        MIMSEM_HIP_TRY(hipStreamSynchronize(c->stream));
        std::memcpy(host, c->h_pin, (size_t)bytes);
        return MIMSEM_OK;
    }
    MIMSEM_HIP_TRY(hipMemcpyAsync(host, dev, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    MIMSEM_HIP_TRY(hipStreamSynchronize(c->stream));
    return MIMSEM_OK;
}
namespace {
__global__ __launch_bounds__(256) void k_fill64(long long n, unsigned long long v, unsigned long long* __restrict__ out) {
    const long long i = (long long)blockIdx.x*256 + threadIdx.x;
    if (i < n) out[i] = v;
}
}  // namespace
// (8-byte-aligned fills go through a kernel: inside a recorded graph a memset NODE costs tens of microseconds on this runtime, a kernel node
// two or three -- the fixed-length solves of the shallow-water step clear five vectors per Picard iteration)
int mimsem_memset(mimsem_ctx* c, void* dev, int byte, long long bytes) {
    if (!c || !dev || bytes < 0) return MIMSEM_ERR_ARG;
    if (bytes == 0) return MIMSEM_OK;
    if (bytes % 8 == 0 && ((uintptr_t)dev & 7u) == 0 && !c->memset_node) {
        const unsigned long long v = 0x0101010101010101ull*(unsigned long long)(unsigned char)byte;
        const long long n = bytes/8;
        hipLaunchKernelGGL(k_fill64, dim3((unsigned)((n + 255)/256)), dim3(256), 0, c->stream, n, v, (unsigned long long*)dev);
        MIMSEM_HIP_TRY(hipGetLastError());
        return MIMSEM_OK;
    }
    MIMSEM_HIP_TRY(hipMemsetAsync(dev, byte, (size_t)bytes, c->stream));
    return MIMSEM_OK;
}

// ---- horizontal operators --------------------------------------------------------------------
// one operator apply as the entry points state it: the arguments of mimsem_op_apply, then what only some entries have
struct ApplyCall {
    int op, lev0, nlev; double scale; unsigned flags;
    const double* f; long long fs; const double* x; long long xs; double* y; long long ys; double alpha;
    const double* f2 = nullptr; long long f2s = 0; double param = 0.0;      // second coefficient field and tau (mimsem_op_apply_up)
    const GatherEpilogue* epi = nullptr; const double* blocks = nullptr;   // the Richardson / Chebyshev sweeps
    int part = 0;                                                          // mimsem_op_apply_part
    int lev_step = 1;                                                      // mimsem_op_apply_levels
};
static int op_apply_core(mimsem_ctx* c, const ApplyCall& k);
static bool is_up_op(int op);

int mimsem_op_apply(mimsem_ctx* c, int op, int geom_lev0, int nlev, double scale, unsigned flags,
                    const double* f, long long fs, const double* x, long long xs,
                    double* y, long long ys, double alpha) {
    if (is_up_op(op)) return MIMSEM_ERR_ARG;   // need mimsem_op_apply_up
    return op_apply_core(c, {op, geom_lev0, nlev, scale, flags, f, fs, x, xs, y, ys, alpha});
}

// HorizSolve::diagVertVort (eul/HorizSolve.cpp:842-850) assembles M2 and F at level 0 for EVERY interface: geom_lev_step 0 evaluates every
// row at geom_lev0 (the two-pass form: element pass + gather); 1 is mimsem_op_apply
int mimsem_op_apply_levels(mimsem_ctx* c, int op, int geom_lev0, int geom_lev_step, int nlev, double scale, unsigned flags,
                           const double* f, long long fs, const double* x, long long xs,
                           double* y, long long ys, double alpha) {
    if (geom_lev_step == 1) return mimsem_op_apply(c, op, geom_lev0, nlev, scale, flags, f, fs, x, xs, y, ys, alpha);
    if (geom_lev_step != 0) return MIMSEM_ERR_ARG;
    if (op != MIMSEM_OP_WMAT && op != MIMSEM_OP_UHMAT) return MIMSEM_ERR_UNSUPPORTED;
    ApplyCall k{op, geom_lev0, nlev, scale, flags, f, fs, x, xs, y, ys, alpha};
    k.lev_step = 0;
    return op_apply_core(c, k);
}

static bool is_up_op(int op) {
    return op == MIMSEM_OP_PHMAT_UP || op == MIMSEM_OP_ROTMAT_UP || op == MIMSEM_OP_UMAT_UP || op == MIMSEM_OP_UHMAT_UP ||
           op == MIMSEM_OP_UVEC_HU_UP || op == MIMSEM_OP_UMAT_RAY || op == MIMSEM_OP_UMAT_FRIC;
}
int mimsem_ctx_set_halo_slots(mimsem_ctx* c, int form, const int* slots, int n) {
    if (!c || form != 1 || n < 0 || (n && !slots)) return MIMSEM_ERR_ARG;
    if (c->is_capturing() || c->split.pending) return MIMSEM_ERR_STATE;      // (a pending BOUNDARY part belongs to the plan in force)
    c->d_pcw = nullptr;      // (retired.  The element-block weights count halo edges twice: remade on next use)
    if (!c->wv.on && c->h_i1x.empty()) {      // two-pass form: nothing to reorder (the split degenerates, see mimsem_op_apply_part); the marks are kept all the same
        c->h_halo1.assign(c->n1, 0);
        for (int i = 0; i < n; i++) { if (slots[i] < 0 || slots[i] >= c->n1) return MIMSEM_ERR_ARG; c->h_halo1[slots[i]] = 1; }
        return MIMSEM_OK;
    }
    std::vector<char> marked(std::max(c->n1, 1), 0);
    for (int i = 0; i < n; i++) { if (slots[i] < 0 || slots[i] >= c->n1) return MIMSEM_ERR_ARG; marked[slots[i]] = 1; }
    c->h_halo1.assign(marked.begin(), marked.begin() + c->n1);        // (kept: the block preconditioners weight shared edges by their GLOBAL multiplicity, csrc/ksp.hip)
    MIMSEM_HIP_TRY(hipStreamSynchronize(c->stream));
    const int rc = setup_wave(c, marked.data());
    return rc == MIMSEM_ERR_UNSUPPORTED ? MIMSEM_OK : rc;      // numbering without a wave-level plan: the two-pass form stays, the split degenerates
}

int mimsem_op_apply_part(mimsem_ctx* c, int op, int geom_lev0, int nlev, double scale, unsigned flags,
                         const double* f, long long fs, const double* x, long long xs,
                         double* y, long long ys, double alpha, int part) {
    if (is_up_op(op) || part < MIMSEM_PART_ALL || part > MIMSEM_PART_INTERIOR) return MIMSEM_ERR_ARG;
    ApplyCall k{op, geom_lev0, nlev, scale, flags, f, fs, x, xs, y, ys, alpha};
    k.part = part;
    return op_apply_core(c, k);
}

int mimsem_op_apply_part_reset(mimsem_ctx* c) {
    if (!c) return MIMSEM_ERR_ARG;
    c->split.pending = false;
    return MIMSEM_OK;
}

int mimsem_op_apply_up(mimsem_ctx* c, int op, int geom_lev0, int nlev, double scale, double tau, unsigned flags,
                       const double* f, long long fs, const double* u, long long us,
                       const double* x, long long xs, double* y, long long ys, double alpha) {
    if (!is_up_op(op) || !u) return MIMSEM_ERR_ARG;
    if ((flags & MIMSEM_FLAG_TRANSPOSE) && op != MIMSEM_OP_UMAT_UP && op != MIMSEM_OP_UHMAT_UP) return MIMSEM_ERR_ARG;
    return op_apply_core(c, {op, geom_lev0, nlev, scale, flags, f, fs, x, xs, y, ys, alpha, u, us, tau});
}

}  // extern "C"

// The arguments every element and wave kernel shares; a route then sets only what its kernel reads -- everything else is zero or null.
static ElemArgs elem_args(const mimsem_ctx* c, int lev0, int nlev, unsigned flags, double scale, double alpha) {
    ElemArgs a{};
    a.nEl = c->nEl; a.nlev = nlev; a.lev0 = lev0; a.total = c->nEl*nlev;
    a.flags = flags; a.scale = scale; a.alpha = alpha;
    a.J = c->d_J; a.det = c->d_det; a.tI = c->d_tI; a.th = c->d_th; a.E = c->d_E; a.w = c->d_w; a.xn = c->d_xn;
    a.tIp = c->d_tIp; a.tnp = c->nk/2 + 1; a.tps = (long long)c->nEl*c->es.mp12*2;
    a.i0 = c->d_i0; a.i1x = c->d_i1x; a.i1y = c->d_i1y; a.i2 = c->d_i2; a.iq = c->d_iq;
    a.lch = level_chunk(c, nlev);      // (swz stays 0: the natural order already keeps all level-chunks of an element on one XCD, profiles/r01_swizzle_ab.txt)
    return a;
}
// the edge basis and the GLL weights by value (the wave-level kernels, orders <= 4)
static void basis_by_value(const mimsem_ctx* c, ElemArgs& a) {
    for (size_t k = 0; k < 20; k++) a.Etab[k] = k < c->tab.E.size() ? c->tab.E[k] : 0.0;
    for (size_t k = 0; k < 5; k++) a.Wq[k] = k < c->tab.quad.w.size() ? c->tab.quad.w[k] : 0.0;
}
// the wave kernels address their rows with 32-bit byte offsets: vectors / metric beyond 4 GB per level stay on the two-pass form
// (the 2-form-valued kernel touches no node table: `nodes` false leaves n0 out)
static bool fits_32bit(const mimsem_ctx* c, bool nodes) {
    const long long lim = 1LL << 28;
    return (long long)c->n1 < lim && (!nodes || (long long)c->n0 < lim) && (long long)c->n2 < lim && (long long)c->nEl*c->es.mp12 < lim;
}

#ifdef MIMSEM_STAMPS      // diagnostic build: per-phase s_memtime stamps of every work item of a wave launch, summarised on stderr
static long long* g_stamps = nullptr; static size_t g_stamp_items = 0;
static size_t stamps_begin(mimsem_ctx* c, int nlev, ElemArgs& a) {
    const size_t items = (size_t)c->wv.ngroups*std::max((nlev + a.lch - 1)/a.lch, a.wnp);     // (the kernel stamps item < wgroups x parts: never fewer slots than that)
    if (!std::getenv("MIMSEM_WAVE_STAMPS")) return items;      // (a diagnostic build of its own: not one of the closed experiments)
    if (items > g_stamp_items) { if (g_stamps) (void)hipFree(g_stamps); (void)hipMalloc((void**)&g_stamps, items*16*8); g_stamp_items = items; }
    (void)hipMemsetAsync(g_stamps, 0, items*16*8, c->stream);
    a.wstamps = g_stamps;
    return items;
}
static void stamps_report(mimsem_ctx* c, const ElemArgs& a, size_t items) {
    if (!a.wstamps) return;
    (void)hipStreamSynchronize(c->stream);
    std::vector<long long> h(items*16);
    (void)hipMemcpy(h.data(), g_stamps, items*16*8, hipMemcpyDeviceToHost);
    long long t0 = h[0], t1 = 0;
    for (size_t i = 0; i < items; i++) { t0 = std::min(t0, h[i*16]); t1 = std::max(t1, h[i*16 + 15]); }
    fprintf(stderr, "[stamps] items %zu lch %d  first entry -> last done: %lld ticks\n", items, a.lch, t1 - t0);
    const char* names[16] = {"entry(rel. first)", "barrier", "tables requested", "level loads issued", "batch0", "batch1", "batch2", "batch3",
                             "b4", "b5", "b6", "chunks done", "fin: stores acked", "fin: arrival counted", "fin: sides finished", "stores acked"};
    for (int k = 0; k < 16; k++) {
        std::vector<long long> v;
        for (size_t i = 0; i < items; i++) if (h[i*16 + k]) v.push_back(k == 0 ? h[i*16] - t0 : h[i*16 + k] - h[i*16]);
        if (v.empty()) continue;
        std::sort(v.begin(), v.end());
        fprintf(stderr, "[stamps] %-20s min %8lld  p10 %8lld  median %8lld  p90 %8lld  max %8lld   (ticks since the wave's entry)\n", names[k],
                v.front(), v[v.size()/10], v[v.size()/2], v[v.size()*9/10], v.back());
    }
}
#endif

// ---- the routes of an apply: each gets the shared arguments `a` of the router and fills in what its kernels read ----

// p = 3: the wave-level kernel of the 2-form-valued operators (no scatter: one launch)
static int apply_wave2(mimsem_ctx* c, const ApplyCall& k, ElemArgs& a) {
    if (int rc = c->ensure_ye(64)) return rc;
    a.wlane = c->wv.lane; a.wgroups = c->wv.ngroups; a.wG = c->wv.G; a.wR = c->wv.R;
    a.lch = wave_level_chunk(c, k.nlev); a.wcpp = wave_chunks_per_item(c, k.nlev, a.lch, c->wv.ngroups); a.swz = c->wave_order;
    a.accum = (k.flags & MIMSEM_FLAG_ACCUM) ? 1 : 0; a.y = c->d_ye;       // a.y: the dump for idle lanes
    basis_by_value(c, a);
    return launch_apply_wave2(c, k.op, a);
}

// Richardson sweep: element pass into the workspace, then the gather with the update epilogue (y is the iterate);
// with `blocks` the element-block preconditioner runs in between on the second half of the workspace
static int apply_epilogue(mimsem_ctx* c, const ApplyCall& k, ElemArgs& a, int outsp) {
    const long long per = (long long)c->nEl*(outsp == 1 ? 2*c->es.n1e : c->es.n0e);
    int rc;
    if ((rc = c->ensure_ye(per*k.nlev*(k.blocks ? 2 : 1)))) return rc;
    a.out = c->d_ye; a.os = per;
    if ((rc = launch_elem_apply(c, k.op, a))) return rc;
    const double* src = c->d_ye;
    if (k.blocks) {
        double* ze = c->d_ye + per*k.nlev;
        if ((rc = launch_blocks_residual(c, k.nlev, k.blocks, c->d_ye, per, k.epi->b, k.epi->bs, ze, per, k.epi->escale, k.epi->ess))) return rc;
        src = ze;
    }
    return launch_gather_epilogue(c, outsp, k.nlev, src, per, *k.epi, k.y, k.ys);
}

// fused path (experiments): group-local sums in LDS, complete slots written straight to y, perimeter partials to the workspace
static int apply_fused(mimsem_ctx* c, const ApplyCall& k, ElemArgs& a) {
    if (int rc = c->ensure_ye((long long)std::max(c->f_npart, 1)*k.nlev)) return rc;
    a.fperm = c->d_fperm; a.flid = c->d_flid; a.fslot = c->d_fslot; a.fcnt = c->d_fcnt;
    a.ngroups = c->f_ngroups; a.lmax = c->f_lmax;
    a.y = k.y; a.ys = k.ys; a.out = c->d_ye; a.os = c->f_npart;
    const int rc = launch_elem_apply(c, k.op, a);
    return rc ? rc : launch_gather_perim(c, k.nlev, c->d_ye, c->f_npart, a.accum, k.y, k.ys);
}

// wave-level fused path: complete slots straight into y, one partial per perimeter slot into the workspace, perimeter pass
static int apply_wave1(mimsem_ctx* c, const ApplyCall& k, ElemArgs& a, bool splits) {
    const WaveTables& w = c->wv;
    const ElemSizes& es = c->es;
    const int nlev = k.nlev;
    // owner-computes (Umat at p = 3, a whole apply): one launch; the workspace row keeps only its dump tail (a ragged last chunk)
    const bool own = w.own && !splits && k.op == MIMSEM_OP_UMAT && es.n == 3 && !c->d_tIn && w.ntiles == 0;
    const long long prow = (own ? 0LL : (long long)w.npart) + 128;  // partial sums of a level + the dump tail (64 lanes x 16 bytes)
    int g0 = 0, g1 = w.ngroups, r0 = 0, r1 = w.nps;
    if (splits && k.part == MIMSEM_PART_BOUNDARY) { g1 = w.nbgroups; r1 = w.nbrec; }
    if (splits && k.part == MIMSEM_PART_INTERIOR) { g0 = w.nbgroups; r0 = w.nbrec; }
    a.wlane = w.lane; a.wplan = own ? w.oplan : w.plan; a.wgroups = g1 - g0; a.wg0 = g0; a.wdump = own ? 0 : w.npart;
    a.wgh = own ? w.gh : nullptr; a.wgx = w.gx;
    // (the four-level pass adds a pair row to a 32-bit lane offset of the thickInv pair table: half the range of fits_32bit)
    a.wgh4 = (own && (long long)c->nEl*es.mp12 < (1LL << 27)) ? w.gh4 : nullptr;
    a.wsing = w.nsing ? w.sing : nullptr; a.wnode = w.node; a.wG = w.G; a.wR = w.R;
    if (c->d_tIn) { a.tIp = c->d_tIn; a.tps = (long long)c->n0*2; a.tnode = 1; }     // (MIMSEM_WAVE_TNODE=1: thickInv per node)
    a.lch = wave_level_chunk(c, nlev);
    a.wcpp = wave_chunks_per_item(c, nlev, a.lch, g1 - g0);
    if (own) {                                                       // level ranges instead of chunks (wave_level_parts)
        const WaveParts wp = wave_level_parts(c, nlev, g1 - g0);
        a.wnp = wp.np; a.wpb = wp.pb; a.wpr = wp.pr;
        a.lch = nlev == 1 ? 1 : 8; a.wcpp = 1;                         // (lch only picks the instantiation: single-level calls have their own)
        if (const int nwg = a.wgh4 ? wave_balance_workgroups(c, nlev, g1 - g0, wp) : 0) {      // balanced ranges: a planned list instead
            const mimsem_ctx::BalList* b = wave_balance_find(c, nlev, g1 - g0, nwg);
            if (!b && !c->is_capturing()) {               // (no upload inside a capture: such a call keeps the default rule)
                if (int rc = wave_balance_make(c, nlev, g1 - g0, nwg, wp)) return rc;
                b = &c->bal.back();
            }
            if (b && b->items) { a.witems = b->items; a.wnitems = b->nitems; }
        }
    }
    a.swz = c->wave_order;
    if (w.ntiles > 0) {                                              // tile mode (never together with a halo split: setup_wave)
        if (splits) return MIMSEM_ERR_STATE;
        a.wtfin = w.tfin; a.wtile = WTF;
        a.wcpp = std::min(a.wcpp, MIMSEM_WTLEV/8);                   // the tile's LDS rows hold MIMSEM_WTLEV levels
        a.swz &= ~2;                                                 // group-minor work items: the four waves of a workgroup = the four groups of a tile
    }
    // the whole operator in ONE launch: each side of the perimeter is finished by the group that reaches it second (not for the
    // parts of a split apply: their partial sums wait for the other part, and the perimeter pass finishes them)
    const bool fin = !own && w.can_fin && !splits && !a.wtfin && (nlev + a.lch*a.wcpp - 1)/(a.lch*a.wcpp) <= std::max(c->nk, 1);
    a.wfin = fin ? w.fin : nullptr; a.wsslot = w.sslot; a.wcnt = w.cnt;
    a.wfence = (fin && c->w_partmem == 2 && exp_env("MIMSEM_WAVE_FIN_FENCE") && atoi(exp_env("MIMSEM_WAVE_FIN_FENCE")) != 0) ? 1 : 0;
    if (splits) {
        // the pending BOUNDARY part and its INTERIOR part must match; nothing else can consume or overwrite the partial sums
        if (k.part == MIMSEM_PART_BOUNDARY) {
            if (c->split.pending) return MIMSEM_ERR_STATE;
        } else if (!c->split.pending || c->split.op != k.op || c->split.lev0 != k.lev0 || c->split.nlev != nlev ||
                   c->split.flags != k.flags || c->split.y != k.y || c->split.ys != k.ys) return MIMSEM_ERR_STATE;
    }
    int rc;
    if ((rc = fin ? c->ensure_wpart(prow*nlev) : (splits ? c->ensure_wsplit(prow*nlev) : c->ensure_ye(prow*nlev)))) return rc;
    double* const prt = fin ? c->d_wpart : (splits ? c->d_wsplit : c->d_ye);
    a.y = k.y; a.ys = k.ys; a.out = prt; a.os = prow;
    basis_by_value(c, a);
#ifdef MIMSEM_STAMPS
    const size_t stamp_items = stamps_begin(c, nlev, a);
#endif
    rc = a.wgroups > 0 ? launch_apply_wave(c, k.op, a) : MIMSEM_OK;
#ifdef MIMSEM_STAMPS
    stamps_report(c, a, stamp_items);
#endif
    if (!rc && !fin && !own) rc = launch_wave_perim(c, nlev, prt, prow, a.accum, k.y, k.ys, r0, r1);
    if (splits && !rc) {
        if (k.part == MIMSEM_PART_BOUNDARY) { c->split.pending = true; c->split.op = k.op; c->split.lev0 = k.lev0; c->split.nlev = nlev;
                                              c->split.flags = k.flags; c->split.y = k.y; c->split.ys = k.ys; }
        else c->split.pending = false;
    }
    return rc;
}

// the plain form: element pass into the workspace, gather-sum pass
static int apply_two_pass(mimsem_ctx* c, const ApplyCall& k, ElemArgs& a, int outsp) {
    const long long per = (long long)c->nEl*(outsp == 1 ? 2*c->es.n1e : c->es.n0e);
    if (int rc = c->ensure_ye(per*k.nlev)) return rc;
    a.out = c->d_ye; a.os = per;
    if (c->direct) { a.d0 = c->d_d0; a.d1x = c->d_d1x; a.d1y = c->d_d1y; a.y = k.y; a.ys = k.ys; }
    const int rc = launch_elem_apply(c, k.op, a);
    return rc ? rc : launch_gather_sum(c, outsp, k.nlev, c->d_ye, per, a.accum, k.y, k.ys, c->direct);
}

// validates a call, picks its route and arms the profiling events around it
static int op_apply_core(mimsem_ctx* c, const ApplyCall& k) {
    if (!c || k.nlev < 0) return MIMSEM_ERR_ARG;
    const int op = k.op, nlev = k.nlev;
    // interior / boundary split: only the wave-level form with marked halo slots really splits; everything else runs whole as
    // "the boundary part" and has nothing left for "the interior part", so callers can always issue both
    const bool wave_op = op == MIMSEM_OP_UMAT || op == MIMSEM_OP_UHMAT || op == MIMSEM_OP_ROTMAT || op == MIMSEM_OP_UTMAT || op == MIMSEM_OP_UTMAT_H;
    const bool fits = fits_32bit(c, true);
    const bool splits = k.part != 0 && c->wv.on && c->wv.split && wave_op && !k.epi && fits;
    if (k.part == MIMSEM_PART_INTERIOR && !splits) return MIMSEM_OK;
    int in, cf, outsp;
    if (op_spaces(op, &in, &cf, &outsp)) return MIMSEM_ERR_ARG;
    if (nlev == 0 || c->nEl == 0) return MIMSEM_OK;       // empty batch: nothing to do (pointers of empty arrays may be null)
    if (!k.x || !k.y) return MIMSEM_ERR_ARG;
    if (cf >= 0 && !k.f) return MIMSEM_ERR_ARG;
    if (k.lev0 < 0 || k.lev0 + (k.lev_step ? nlev : 1) > c->nk) return MIMSEM_ERR_ARG;
    if (op == MIMSEM_OP_UTMAT && k.lev0 + nlev > c->nk - 1) return MIMSEM_ERR_ARG;   // needs thick[lev+1]
    if (op == MIMSEM_OP_WMATINV || op == MIMSEM_OP_WHMATINV)
        return mimsem_colop_block_inverse_apply(c, op, k.lev0, nlev, k.scale, k.flags, k.f, k.fs, k.x, k.xs, k.y, k.ys, k.alpha);
    if (in == 3 && !c->d_iq) return MIMSEM_ERR_STATE;     // projection operators need mimsem_mesh_desc::indsq

    ElemArgs a = elem_args(c, k.lev0, nlev, k.flags, k.scale, k.alpha);
    a.f = k.f; a.fs = k.fs; a.x = k.x; a.xs = k.xs; a.f2 = k.f2; a.f2s = k.f2s; a.param = k.param;
    a.lstep = k.lev_step;               // 0 (mimsem_op_apply_levels): the forms that walk consecutive levels are passed over
    const bool walks = k.lev_step == 1;
    if (outsp != 2) { a.accum = (k.flags & MIMSEM_FLAG_ACCUM) ? 1 : 0; a.flags = k.flags & ~MIMSEM_FLAG_ACCUM; }      // (the scatter passes accumulate, not the element pass)
    if (c->profiling && (c->prof_count++ % c->prof_every) == 0) { c->ev_k1[0] = c->next_event(); c->ev_k1[1] = c->next_event(); c->ev_k2[0] = c->next_event(); c->ev_k2[1] = c->next_event(); c->ev_has2.push_back(0); }
    int rc;
    if (outsp == 2) {
        a.out = k.y; a.os = k.ys;
        // Wmat itself stays on k_elem_apply by default: measured 9.3e9 applies/s there against 8.2e9 on the DPP kernel (its element algebra
        // is four DPP stages for 9 values); Whmat +3 %, WtQUmat +14 % (profiles/r02_wave_ab.txt).  MIMSEM_WAVE2=2 includes Wmat, 0 none.
        const bool wave2_op = (op == MIMSEM_OP_WMAT && c->wave2_mode == 2) || op == MIMSEM_OP_WHMAT || op == MIMSEM_OP_WTQUMAT || op == MIMSEM_OP_WTQDUDZ;
        if (c->wv.on && c->es.n == 3 && wave2_op && fits_32bit(c, false) && k.part == 0 && c->wave2_mode != 0 && walks) rc = apply_wave2(c, k, a);
        else rc = launch_elem_apply(c, op, a);
    }
    else if (k.epi) rc = apply_epilogue(c, k, a, outsp);
    else if (outsp == 1 && c->fused1 && op < MIMSEM_OP_UMAT_UP && op != MIMSEM_OP_UMAT_RAY && walks) rc = apply_fused(c, k, a);
    else if (c->wv.on && fits && wave_op && walks) rc = apply_wave1(c, k, a, splits);
    else rc = apply_two_pass(c, k, a, outsp);
    c->ev_k1[0] = c->ev_k1[1] = c->ev_k2[0] = c->ev_k2[1] = nullptr;
    return rc;
}

extern "C" {

int mimsem_op_elmat_size(const mimsem_ctx* c, int op) {
    if (!c) return MIMSEM_ERR_ARG;
    const ElemSizes& es = c->es;
    switch (op) {
    case MIMSEM_OP_UMAT: case MIMSEM_OP_UHMAT: case MIMSEM_OP_UTMAT: case MIMSEM_OP_UTMAT_H: case MIMSEM_OP_UMAT_RAY:
    case MIMSEM_OP_UMAT_FRIC:
        return 4*es.n1e*es.n1e;
    case MIMSEM_OP_ROTMAT: return 2*es.n1e*es.n1e;
    case MIMSEM_OP_WMAT: case MIMSEM_OP_WHMAT: case MIMSEM_OP_WMATINV: case MIMSEM_OP_WHMATINV: return es.n2e*es.n2e;
    case MIMSEM_OP_PMAT: case MIMSEM_OP_PHMAT: return es.n0e*es.n0e;
    case MIMSEM_OP_WTQUMAT: case MIMSEM_OP_WTQDUDZ: case MIMSEM_OP_UTQWMAT: return 2*es.n2e*es.n1e;
    }
    return MIMSEM_ERR_ARG;
}

int mimsem_op_element_matrices_ex(mimsem_ctx* c, int op, int geom_lev, double scale, double tau, unsigned flags,
                                  const double* f, const double* u, double* out) {
    if (!c || !out || !f || !u) return MIMSEM_ERR_ARG;
    if (op != MIMSEM_OP_UMAT_RAY && op != MIMSEM_OP_UMAT_FRIC) return MIMSEM_ERR_ARG;
    if (geom_lev < 0 || geom_lev >= c->nk) return MIMSEM_ERR_ARG;
    return launch_elmats(c, op, geom_lev, scale, flags, f, out, u, tau);
}

int mimsem_op_element_matrices(mimsem_ctx* c, int op, int geom_lev, double scale, unsigned flags,
                               const double* f, double* out) {
    if (!c || !out) return MIMSEM_ERR_ARG;
    if (is_up_op(op)) return MIMSEM_ERR_ARG;
    int in, cf, outsp;
    if (op_spaces(op, &in, &cf, &outsp)) return MIMSEM_ERR_ARG;
    if (cf >= 0 && !f) return MIMSEM_ERR_ARG;
    if (geom_lev < 0 || geom_lev >= c->nk) return MIMSEM_ERR_ARG;
    if (op == MIMSEM_OP_UTMAT && geom_lev + 1 >= c->nk) return MIMSEM_ERR_ARG;
    if (op == MIMSEM_OP_WMATINV || op == MIMSEM_OP_WHMATINV) {
        // Wmat/Whmat blocks with the inverse ops' fixed flags, then batched Gauss-Jordan (LinAlg.cpp:186-269)
        const int base = (op == MIMSEM_OP_WMATINV) ? MIMSEM_OP_WMAT : MIMSEM_OP_WHMAT;
        int rc = launch_elmats(c, base, geom_lev, scale, MIMSEM_FLAG_VERT, f, out);
        if (rc) return rc;
        return mimsem_block_inverse_inplace(c, c->nEl, c->es.n2e, out);
    }
    return launch_elmats(c, op, geom_lev, scale, flags, f, out);
}

int mimsem_block_inverse(mimsem_ctx* c, long long nblocks, int n, double* blocks) {
    if (!c || nblocks < 0 || n < 1 || (nblocks && !blocks)) return MIMSEM_ERR_ARG;
    return mimsem_block_inverse_inplace(c, nblocks, n, blocks);      // MIMSEM_ERR_UNSUPPORTED when one block no longer fits a workgroup's LDS
}

// the same, and the number of blocks in which LinAlg::Inv would have returned its error (a pivot below 1e-12 after full pivoting,
// eul/LinAlg.cpp:243-246): MIMSEM_OK with *n_singular > 0 -- the blocks are inverted as the reference inverts them, garbage included
int mimsem_block_inverse_status(mimsem_ctx* c, long long nblocks, int n, double* blocks, int* n_singular) {
    if (!c || !n_singular || nblocks < 0 || n < 1 || (nblocks && !blocks)) return MIMSEM_ERR_ARG;
    *n_singular = 0;
    if (c->is_capturing()) return MIMSEM_ERR_STATE;                  // (reads a counter back)
    int* d_err = nullptr;
    MIMSEM_HIP_TRY(hipMalloc((void**)&d_err, sizeof(int)));
    int rc = MIMSEM_OK;
    if (hipMemsetAsync(d_err, 0, sizeof(int), c->stream) != hipSuccess) rc = MIMSEM_ERR_HIP;
    if (!rc) rc = mimsem_block_inverse_inplace(c, nblocks, n, blocks, d_err);
    if (!rc && hipMemcpyAsync(n_singular, d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = MIMSEM_ERR_HIP;
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = MIMSEM_ERR_HIP;
    (void)hipFree(d_err);
    return rc;
}

int mimsem_elem_blocks_apply(mimsem_ctx* c, int form, int nlev, unsigned flags, const double* blocks, long long blocks_level_stride,
                             const double* elem_scale, long long elem_scale_stride,
                             const double* x, long long xs, double* y, long long ys, double alpha) {
    if (!c || !blocks || !x || !y || form < 0 || form > 2 || nlev < 0) return MIMSEM_ERR_ARG;
    return launch_blocks_apply(c, form, nlev, (flags & MIMSEM_FLAG_TRANSPOSE) ? 1 : 0, blocks, blocks_level_stride,
                               x, xs, y, ys, alpha, (flags & MIMSEM_FLAG_ACCUM) ? 1 : 0, elem_scale, elem_scale_stride);
}

int mimsem_incidence_apply(mimsem_ctx* c, int which, int nlev, const double* x, long long xs, double* y, long long ys) {
    if (!c || !x || !y || which < 0 || which > 3 || nlev < 0) return MIMSEM_ERR_ARG;
    return launch_incidence(c, which, nlev, x, xs, y, ys);
}

int mimsem_interp_quad(mimsem_ctx* c, int form, unsigned flags, int nlev, const double* x, long long xs, double* out, long long os) {
    if (!c || form < 0 || form > 2 || nlev < 0 || (flags & ~MIMSEM_INTERP_GLOBAL)) return MIMSEM_ERR_ARG;
    if (nlev == 0 || c->nEl == 0) return MIMSEM_OK;
    if (!x || !out) return MIMSEM_ERR_ARG;
    const long long per = (long long)c->nEl*c->es.mp12*(form == 1 ? 2 : 1);
    if (nlev > 1 && os < per) return MIMSEM_ERR_ARG;
    return launch_interp_quad(c, form, (flags & MIMSEM_INTERP_GLOBAL) ? 1 : 0, nlev, x, xs, out, os);
}

int mimsem_sw_operator_apply(mimsem_ctx* c, int nlev, double a, double grav, double H, const double* f0, long long f0s,
                             const double* x, long long xs, double* y, long long ys) {
    if (!c || nlev < 0) return MIMSEM_ERR_ARG;
    if (nlev == 0 || c->nEl == 0) return MIMSEM_OK;
    if (!f0 || !x || !y || x == y) return MIMSEM_ERR_ARG;
    const long long n = (long long)c->n1 + c->n2;
    if (nlev > 1 && (xs < n || ys < n)) return MIMSEM_ERR_ARG;
    return launch_sw_operator(c, nlev, a, grav, H, f0, f0s, x, xs, y, ys);
}

int mimsem_sw_blocks_apply(mimsem_ctx* c, int nlev, const double* blocks, const double* x, long long xs, double* y, long long ys) {
    if (!c || nlev < 0) return MIMSEM_ERR_ARG;
    if (nlev == 0 || c->nEl == 0) return MIMSEM_OK;
    if (!blocks || !x || !y || x == y) return MIMSEM_ERR_ARG;
    const long long n = (long long)c->n1 + c->n2;
    if (nlev > 1 && (xs < n || ys < n)) return MIMSEM_ERR_ARG;
    return launch_sw_blocks_apply(c, nlev, blocks, x, xs, y, ys);
}

int mimsem_op_richardson_sweep(mimsem_ctx* c, int op, int geom_lev0, int nlev, double scale, double tau, unsigned flags,
                               const double* f, long long fs, const double* u, long long us,
                               const double* b, long long bs, const double* dinv, long long ds,
                               double* x, long long xs, double* upd, long long upds) {
    if (!c || !b || !dinv || !x || (flags & MIMSEM_FLAG_ACCUM)) return MIMSEM_ERR_ARG;
    int in, cf, outsp;
    if (op_spaces(op, &in, &cf, &outsp) || outsp == 2 || in != outsp) return MIMSEM_ERR_ARG;     // square operators on gathered spaces
    if (is_up_op(op) && !u) return MIMSEM_ERR_ARG;
    GatherEpilogue g{1, b, bs, dinv, ds, upd, upds};
    return op_apply_core(c, {op, geom_lev0, nlev, scale, flags, f, fs, x, xs, x, xs, 1.0, u, us, tau, &g});
}

// the Chebyshev form of mimsem_op_richardson_sweep: z = dinv (b - Op x);  p = z + beta p;  x += alpha p  (two launches)
int mimsem_op_chebyshev_sweep(mimsem_ctx* c, int op, int geom_lev0, int nlev, double scale, double tau, unsigned flags,
                              const double* f, long long fs, const double* u, long long us,
                              const double* b, long long bs, const double* dinv, long long ds, double alpha, double beta,
                              double* p, long long ps, double* x, long long xs, double* upd, long long upds) {
    if (!c || !b || !dinv || !x || !p || (flags & MIMSEM_FLAG_ACCUM)) return MIMSEM_ERR_ARG;
    int in, cf, outsp;
    if (op_spaces(op, &in, &cf, &outsp) || outsp == 2 || in != outsp) return MIMSEM_ERR_ARG;     // square operators on gathered spaces
    if (is_up_op(op) && !u) return MIMSEM_ERR_ARG;
    GatherEpilogue g{5, b, bs, dinv, ds, upd, upds};
    g.alpha = alpha; g.beta = beta; g.p = p; g.ps = ps;
    return op_apply_core(c, {op, geom_lev0, nlev, scale, flags, f, fs, x, xs, x, xs, 1.0, u, us, tau, &g});
}

int mimsem_block_richardson_sweep(mimsem_ctx* c, int op, int geom_lev0, int nlev, double scale, unsigned flags,
                                  const double* f, long long fs, const double* blocks,
                                  const double* b, long long bs, double* x, long long xs, double* upd, long long upds) {
    if (!c || !b || !blocks || !x || (flags & MIMSEM_FLAG_ACCUM)) return MIMSEM_ERR_ARG;
    int in, cf, outsp;
    if (op_spaces(op, &in, &cf, &outsp) || outsp != 1 || in != 1 || is_up_op(op)) return MIMSEM_ERR_ARG;
    if (c->es.n > 5) return MIMSEM_ERR_UNSUPPORTED;
    GatherEpilogue g{2, b, bs, nullptr, 0, upd, upds};
    return op_apply_core(c, {op, geom_lev0, nlev, scale, flags, f, fs, x, xs, x, xs, 1.0, nullptr, 0, 0.0, &g, blocks});
}

int mimsem_block_chebyshev_sweep(mimsem_ctx* c, int op, int geom_lev0, int nlev, double scale, unsigned flags,
                                 const double* f, long long fs, const double* blocks, const double* elem_scale, long long es_stride,
                                 const double* b, long long bs, double alpha, double beta, double* p, long long ps,
                                 double* x, long long xs, double* upd, long long upds) {
    if (!c || !b || !blocks || !x || !p || (flags & MIMSEM_FLAG_ACCUM)) return MIMSEM_ERR_ARG;
    int in, cf, outsp;
    if (op_spaces(op, &in, &cf, &outsp) || outsp != 1 || in != 1 || is_up_op(op)) return MIMSEM_ERR_ARG;
    if (c->es.n > 5) return MIMSEM_ERR_UNSUPPORTED;
    GatherEpilogue g{3, b, bs, nullptr, 0, upd, upds};
    g.alpha = alpha; g.beta = beta; g.p = p; g.ps = ps; g.escale = elem_scale; g.ess = es_stride;
    return op_apply_core(c, {op, geom_lev0, nlev, scale, flags, f, fs, x, xs, x, xs, 1.0, nullptr, 0, 0.0, &g, blocks});
}

// A whole fixed-length Chebyshev solve of  Umat x = b  from x = 0 in ONE call (round 6): the first step has no element pass (Op 0 = 0: the block
// pass takes b as its residual) and writes x and p instead of updating them, so neither needs clearing; steps 1 .. nsteps - 1 are the three
// launches of mimsem_block_chebyshev_sweep.  The same bits as nsteps calls of that entry on x = 0, p = anything finite (up to the sign of a zero).
// EXPERIMENT (experiments build, MIMSEM_CHEB_PEND=1): two launches per step -- the gather epilogue of step k folded into the element pass of
// step k + 1 (body_elem_apply<..., PEND>), x and p alternating between two buffers.  Bit-equal and SLOWER (8.22 against 7.07 ms per HorizSolve
// evaluation): the folded update turns the epilogue's coalesced slot-order accesses into 96 gathers per unit on 12 of 32 lanes.
}  // extern "C"

// eop: the operator of the element pass -- MIMSEM_OP_UMAT, or MIMSEM_OP_UMAT_FRIC with its two exner fields and tau (mimsem_fric_chebyshev_solve)
static int block_chebyshev_solve_core(mimsem_ctx* c, int op, int eop, int geom_lev0, int nlev, double scale, unsigned flags,
                                      const double* ef, long long efs, const double* ef2, double tau,
                                      const double* blocks, const double* elem_scale, long long es_stride,
                                      const double* b, long long bs, int nsteps, const double* coef,
                                      double* x, long long xs, double* pb, long long pbs, double* upd, long long upds) {
    if (!c || nlev < 0 || nsteps < 1 || !coef || (flags & ~MIMSEM_FLAG_VERT)) return MIMSEM_ERR_ARG;
    if (op != MIMSEM_OP_UMAT) return MIMSEM_ERR_UNSUPPORTED;
    if (c->es.n > 5) return MIMSEM_ERR_UNSUPPORTED;
    if (nlev == 0 || c->nEl == 0) return MIMSEM_OK;
    if (!b || !blocks || !x || x == b || geom_lev0 < 0 || geom_lev0 + nlev > c->nk) return MIMSEM_ERR_ARG;
    if (nlev > 1 && (xs < c->n1 || bs < c->n1 || (pb && pbs < c->n1) || (upd && upds < c->n1))) return MIMSEM_ERR_ARG;
    const ElemSizes& es = c->es;
    const long long per = (long long)c->nEl*2*es.n1e, n1 = c->n1;
    const bool pend = kExperiments && c->cheb_pend && nsteps > 1 && eop == MIMSEM_OP_UMAT;      // (the owed update rides in Umat's element pass only)
    int rc;
    if ((rc = c->ensure_ye(per*nlev*2))) return rc;
    if ((rc = c->ensure_cheb((pend ? 3 : 1)*n1*nlev))) return rc;
    double* ye = c->d_ye; double* ze = c->d_ye + per*nlev;
    ElemArgs a = elem_args(c, geom_lev0, nlev, flags, scale, 1.0);
    a.f = ef; a.fs = efs; a.f2 = ef2; a.param = tau;
    a.out = ye; a.os = per;
    c->ev_k1[0] = c->ev_k1[1] = c->ev_k2[0] = c->ev_k2[1] = nullptr;
    // step 0: z_0 = P b
    if ((rc = launch_blocks_residual(c, nlev, blocks, nullptr, per, b, bs, ze, per, elem_scale, es_stride))) return rc;
    GatherEpilogue g{3, b, bs, nullptr, 0, nullptr, 0};
    if (!pend) {
        double* p = c->d_cheb;
        g.p = p; g.ps = n1;
        for (int k = 0; k < nsteps; k++) {
            if (k > 0) {
                a.x = x; a.xs = xs;
                if ((rc = launch_elem_apply(c, eop, a))) return rc;
                if ((rc = launch_blocks_residual(c, nlev, blocks, ye, per, b, bs, ze, per, elem_scale, es_stride))) return rc;
            }
            g.alpha = coef[2*k]; g.beta = coef[2*k + 1]; g.zero = k == 0;
            // the check vectors: pb = z_0, upd = z_{nsteps-1}; a one-step solve has one z for both
            g.upd = k == nsteps - 1 && upd ? upd : (k == 0 ? pb : nullptr); g.us = k == nsteps - 1 && upd ? upds : pbs;
            if ((rc = launch_gather_epilogue(c, 1, nlev, ze, per, g, x, xs))) return rc;
        }
        if (nsteps == 1 && upd && pb)
            for (int l = 0; l < nlev; l++) MIMSEM_HIP_TRY(hipMemcpyAsync(pb + (size_t)l*pbs, upd + (size_t)l*upds, (size_t)n1*sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        return MIMSEM_OK;
    }
    // after nsteps - 1 alternations the iterate must sit in the caller's x
    double* X[2]; long long XS[2];
    const int cx = (nsteps - 1) & 1;
    X[cx] = x; XS[cx] = xs; X[cx ^ 1] = c->d_cheb; XS[cx ^ 1] = n1;
    double* P[2] = {c->d_cheb + n1*nlev, c->d_cheb + 2*n1*nlev};
    int cur = 0;
    for (int k = 1; k < nsteps; k++) {
        ElemPending pd;
        pd.plan = c->d_g1; pd.ze = ze; pd.zes = per; pd.alpha = coef[2*(k - 1)]; pd.beta = coef[2*(k - 1) + 1]; pd.first = k == 1;
        pd.p_in = P[cur]; pd.p_out = P[cur ^ 1]; pd.ps = n1;
        pd.x_out = X[cur ^ 1]; pd.xos = XS[cur ^ 1];
        pd.upd = k == 1 ? pb : nullptr; pd.us = pbs;
        a.x = X[cur]; a.xs = XS[cur];
        if ((rc = launch_elem_apply_pending(c, a, pd))) return rc;
        cur ^= 1;
        if ((rc = launch_blocks_residual(c, nlev, blocks, ye, per, b, bs, ze, per, elem_scale, es_stride))) return rc;
    }
    g.upd = upd; g.us = upds;
    g.alpha = coef[2*(nsteps - 1)]; g.beta = coef[2*(nsteps - 1) + 1]; g.p = P[cur]; g.ps = n1;
    return launch_gather_epilogue(c, 1, nlev, ze, per, g, X[cur], XS[cur]);
}

extern "C" {

int mimsem_block_chebyshev_solve(mimsem_ctx* c, int op, int geom_lev0, int nlev, double scale, unsigned flags,
                                 const double* f, long long fs, const double* blocks, const double* elem_scale, long long es_stride,
                                 const double* b, long long bs, int nsteps, const double* coef,
                                 double* x, long long xs, double* pb, long long pbs, double* upd, long long upds) {
    (void)f; (void)fs;
    return block_chebyshev_solve_core(c, op, MIMSEM_OP_UMAT, geom_lev0, nlev, scale, flags, nullptr, 0, nullptr, 0.0, blocks, elem_scale, es_stride,
                                      b, bs, nsteps, coef, x, xs, pb, pbs, upd, upds);
}

// (M1 + M1ray(tau)) x = b, Euler_2.cpp:1431-1456: the same sweep with MIMSEM_OP_UMAT_FRIC as its element pass -- x, thickInv and the metric are
// read once per step, plus the two exner rows.  Without friction (tau == 0 or no exner) it IS the entry above.
int mimsem_fric_chebyshev_solve(mimsem_ctx* c, int op, int geom_lev0, int nlev, double scale, unsigned flags,
                                const double* f, long long fs, const double* blocks, const double* elem_scale, long long es_stride,
                                const double* b, long long bs, int nsteps, const double* coef,
                                double* x, long long xs, double* pb, long long pbs, double* upd, long long upds,
                                double tau, const double* exner, long long exner_stride, const double* exner_s) {
    if (tau == 0.0 || !exner)
        return mimsem_block_chebyshev_solve(c, op, geom_lev0, nlev, scale, flags, f, fs, blocks, elem_scale, es_stride, b, bs, nsteps, coef,
                                            x, xs, pb, pbs, upd, upds);
    if (!c || flags != MIMSEM_FLAG_VERT || !exner_s || !(tau > 0.0) || (nlev > 1 && exner_stride < c->n2)) return MIMSEM_ERR_ARG;
    return block_chebyshev_solve_core(c, op, MIMSEM_OP_UMAT_FRIC, geom_lev0, nlev, scale, flags, exner, exner_stride, exner_s, tau, blocks, elem_scale,
                                      es_stride, b, bs, nsteps, coef, x, xs, pb, pbs, upd, upds);
}

int mimsem_sw_operator_precond_apply(mimsem_ctx* c, int nlev, double a, double grav, double H, const double* f0, long long f0s,
                                     const double* blocks, const double* x, long long xs, double* z, long long zs) {
    if (!c || nlev < 0) return MIMSEM_ERR_ARG;
    if (nlev == 0 || c->nEl == 0) return MIMSEM_OK;
    if (!f0 || !blocks || !x || !z || x == z) return MIMSEM_ERR_ARG;
    const long long n = (long long)c->n1 + c->n2;
    if (nlev > 1 && (xs < n || zs < n)) return MIMSEM_ERR_ARG;
    return launch_sw_operator_precond(c, nlev, a, grav, H, f0, f0s, blocks, x, xs, z, zs);
}

int mimsem_sw_operator_precond_chebyshev(mimsem_ctx* c, int nlev, double a, double grav, double H, const double* f0, long long f0s,
                                         const double* blocks, double ca, double cb, double* x, long long xs, double* r, long long rs,
                                         double* d, long long ds) {
    if (!c || nlev < 0) return MIMSEM_ERR_ARG;
    if (nlev == 0 || c->nEl == 0) return MIMSEM_OK;
    if (!f0 || !blocks || !x || !r || !d || x == r || x == d || r == d) return MIMSEM_ERR_ARG;
    const long long n = (long long)c->n1 + c->n2;
    if (nlev > 1 && (xs < n || rs < n || ds < n)) return MIMSEM_ERR_ARG;
    return launch_sw_operator_precond_chebyshev(c, nlev, a, grav, H, f0, f0s, blocks, ca, cb, x, xs, r, rs, d, ds);
}

int mimsem_sw_chebyshev_step2(mimsem_ctx* c, int nlev, double a, double grav, double H, const double* f0, long long f0s, const double* blocks,
                              int pending, double pca, double pcb, double ca, double cb, double* x, long long xs,
                              const double* r_in, const double* d_in, double* r_out, double* d_out, double* rh, double* dh, long long vs) {
    if (!c || nlev < 0) return MIMSEM_ERR_ARG;
    if (nlev == 0 || c->nEl == 0) return MIMSEM_OK;
    if (!f0 || !blocks || !x || !r_in || !d_in || !rh || !dh) return MIMSEM_ERR_ARG;
    if (pending && (!r_out || !d_out || r_out == r_in || d_out == d_in || r_out == d_in || d_out == r_in)) return MIMSEM_ERR_ARG;   // (the other elements of a slot read the old values in the same launch)
    const long long n = (long long)c->n1 + c->n2;
    if (nlev > 1 && (xs < n || vs < n)) return MIMSEM_ERR_ARG;
    return launch_sw_chebyshev_step2(c, nlev, a, grav, H, f0, f0s, blocks, pending, pca, pcb, ca, cb, x, xs, r_in, d_in, r_out, d_out, rh, dh, vs);
}
int mimsem_sw_chebyshev_flush(mimsem_ctx* c, int nlev, double ca, double cb, double* x, long long xs, double* r, double* d, long long vs) {
    if (!c || nlev < 0) return MIMSEM_ERR_ARG;
    if (nlev == 0 || c->nEl == 0) return MIMSEM_OK;
    if (!x || !r || !d || x == r || x == d || r == d) return MIMSEM_ERR_ARG;
    return launch_sw_chebyshev_flush(c, nlev, ca, cb, x, xs, r, d, vs);
}

// Two independent fixed-length Chebyshev solves of a shallow-water Picard iteration, both from x = 0, in SHARED launches (round 6;
// csrc/elem_kernels.hip: k_sw_pair): exactly the sequence
//     for k < nA: mimsem_block_chebyshev_sweep(ctx, MIMSEM_OP_UMAT, 0, 1, 1.0, 0, NULL, 0, blocks1, NULL, 0, b1, 0, coefA[2k], coefA[2k+1], p1, 0, x1, 0, k == nA-1 ? upd1 : (k == 0 ? pb1 : NULL), 0)
//     for k < nB: mimsem_op_chebyshev_sweep(ctx, MIMSEM_OP_PHMAT_UP, 0, 1, 1.0, tau, 0, h, 0, u, 0, b0, 0, dinv, 0, coefB[2k], coefB[2k+1], p0, 0, x0, 0, k == nB-1 ? upd0 : (k == 0 ? pb0 : NULL), 0)
// on x1 = x0 = 0 -- the same kernels' bodies, the same bits (up to the sign of a zero) -- with launch k of the first chain and launch k of the second in
// one grid.  Late in round 6 the chains lost what a zero start makes superfluous: no operator pass in either first step (the block pass takes b1 as its
// residual, the first q update is dinv b0), x and p WRITTEN there instead of updated (nothing to clear), and the first steps' preconditioned
// residuals -- P b1 and dinv b0, the reference norms of the checks -- come out as pb1 / pb0 instead of being computed again by the caller:
// 3 nA - 1 and 2 nB - 1 launches, 8 launches and fills fewer per Picard iteration around them.
int mimsem_sw_dual_chebyshev(mimsem_ctx* c, int nA, const double* coefA, const double* blocks1, const double* b1, double* p1, double* x1, double* upd1, double* pb1,
                             int nB, const double* coefB, double tau, const double* h, const double* u, const double* b0, const double* dinv,
                             double* p0, double* x0, double* upd0, double* pb0) {
    if (!c || nA < 1 || nB < 1 || !coefA || !coefB || !blocks1 || !b1 || !p1 || !x1 || !h || !u || !b0 || !dinv || !p0 || !x0) return MIMSEM_ERR_ARG;
    if ((pb1 && nA < 2 && upd1) || (pb0 && nB < 2 && upd0)) return MIMSEM_ERR_ARG;      // (a one-step solve has ONE preconditioned residual: ask for it once)
    if (c->nEl == 0) return MIMSEM_OK;
    const ElemSizes& es = c->es;
    if (es.n < 2 || es.n > 4) return MIMSEM_ERR_UNSUPPORTED;
    const long long per1 = (long long)c->nEl*2*es.n1e, per0 = (long long)c->nEl*es.n0e;
    int rc = c->ensure_ye(2*per1 + per0);
    if (rc) return rc;
    double *yeA = c->d_ye, *zeA = c->d_ye + per1, *yeQ = c->d_ye + 2*per1;
    // the element passes of two single-level sweeps on the src/ flavour (scale 1, no thickness), as apply_epilogue runs them
    ElemArgs ea = elem_args(c, 0, 1, 0, 1.0, 1.0), eq = ea;
    ea.x = x1; ea.out = yeA; ea.os = per1;
    eq.f = h; eq.f2 = u; eq.param = tau; eq.x = x0; eq.out = yeQ; eq.os = per0;
    PairBlocks ba{c->nEl, 1, c->d_i1x, c->d_i1y, c->d_g1, blocks1, yeA, per1, b1, zeA, per1, (const int4*)c->d_bplan};
    PairGather ga{zeA, per1, c->d_g1, c->n1, GatherEpilogue{3, b1, 0, nullptr, 0, nullptr, 0}, x1};
    PairGather gq{yeQ, per0, c->d_g0, c->n0, GatherEpilogue{5, b0, 0, dinv, 0, nullptr, 0}, x0};
    ga.g.p = p1; ga.g.ps = 0; gq.g.p = p0; gq.g.ps = 0;
    c->ev_k1[0] = c->ev_k1[1] = c->ev_k2[0] = c->ev_k2[1] = nullptr;
    // chain A: {block pass on a zero result, epilogue that writes} then (nA - 1) x {element pass, block pass, epilogue};  chain q: {epilogue that
    // writes, no operator result} then (nB - 1) x {element pass, epilogue}
    const int LA = 3*nA - 1, LB = 2*nB - 1, L = std::max(LA, LB);
    for (int k = 0; k < L; k++) {
        int PA = -1, PB = -1;
        if (k < LA) {
            PA = k == 0 ? 3 : (k == 1 ? 2 : (k - 2)%3);
            if (PA == 2) {
                const int st = k == 1 ? 0 : 1 + (k - 2)/3;
                ga.g.alpha = coefA[2*st]; ga.g.beta = coefA[2*st + 1]; ga.g.zero = st == 0; ga.g.us = 0;
                ga.g.upd = st == nA - 1 && upd1 ? upd1 : (st == 0 ? pb1 : nullptr);
            }
        }
        if (k < LB) {
            PB = k == 0 ? 1 : (k - 1)%2;
            if (PB == 1) {
                const int st = k == 0 ? 0 : 1 + (k - 1)/2;
                gq.g.alpha = coefB[2*st]; gq.g.beta = coefB[2*st + 1]; gq.g.zero = st == 0; gq.g.noacc = st == 0; gq.g.us = 0;
                gq.g.upd = st == nB - 1 && upd0 ? upd0 : (st == 0 ? pb0 : nullptr);
            }
        }
        if (PA >= 0 && PB >= 0) rc = launch_sw_pair(c, PA, PB, ea, ba, ga, eq, gq);
        else if (PA == 0) rc = launch_elem_apply(c, MIMSEM_OP_UMAT, ea);                                  // (the longer chain's tail: its own kernels)
        else if (PA == 1) rc = launch_blocks_residual(c, 1, blocks1, yeA, per1, b1, 0, zeA, per1, nullptr, 0);
        else if (PA == 3) rc = launch_blocks_residual(c, 1, blocks1, nullptr, per1, b1, 0, zeA, per1, nullptr, 0);
        else if (PA == 2) rc = launch_gather_epilogue(c, 1, 1, zeA, per1, ga.g, x1, 0);
        else if (PB == 0) rc = launch_elem_apply(c, MIMSEM_OP_PHMAT_UP, eq);
        else rc = launch_gather_epilogue(c, 0, 1, yeQ, per0, gq.g, x0, 0);
        if (rc) return rc;
    }
    return MIMSEM_OK;
}

int mimsem_halo_pack(mimsem_ctx* c, const int* idx, int count, int nlev, const double* v, long long vs, double* buf) {
    if (!c || count < 0 || nlev < 0) return MIMSEM_ERR_ARG;
    if (count == 0 || nlev == 0) return MIMSEM_OK;        // empty message: pointers of empty arrays may be null
    if (!idx || !v || !buf) return MIMSEM_ERR_ARG;
    return launch_halo_pack(c, idx, count, nlev, v, vs, buf);
}
int mimsem_halo_unpack(mimsem_ctx* c, const int* idx, int count, int nlev, int mode, const double* buf, double* v, long long vs) {
    if (!c || count < 0 || nlev < 0) return MIMSEM_ERR_ARG;
    if (count == 0 || nlev == 0) return MIMSEM_OK;
    if (!idx || !v || !buf) return MIMSEM_ERR_ARG;
    return launch_halo_unpack(c, idx, count, nlev, mode, buf, v, vs);
}

// all neighbours in one launch; buf is segment-major [segment][level][slot]
int mimsem_halo_segments(mimsem_ctx* c, const int* idx, int nseg, const int* seg_off, int seg_begin, int seg_end, int nlev, int mode,
                         double* buf, double* v, long long vs) {
    if (!c || !idx || !seg_off || !buf || !v || nseg < 0 || nseg > MIMSEM_HALO_MAX_SEGMENTS || nlev < 0 || mode < 0 || mode > 2)
        return MIMSEM_ERR_ARG;
    if (seg_begin < 0 || seg_end < seg_begin || seg_end > nseg) return MIMSEM_ERR_ARG;
    for (int i = 0; i < nseg; i++) if (seg_off[i + 1] < seg_off[i]) return MIMSEM_ERR_ARG;
    return launch_halo_segments(c, idx, nseg, seg_off, seg_begin, seg_end, nlev, mode, buf, v, vs);
}

}  // extern "C"
