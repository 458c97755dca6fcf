// mimsem_amd/csrc/wave_balance.hpp -- host planner of the owner form's level ranges (own4::k_apply_wave): which ranges exist
// and which WNW of them share a workgroup, so that every workgroup of a launch carries the same number of level pairs.  Host only, no
// HIP: api.hip uploads the list, tests/cpp/wave_balance_cli.cpp checks it with a plain C++ compiler.
//
// The (group, level pair) cells of a call form one sequence, group-major.  Workgroup w takes the cells between two cuts near
// w T / W and (w + 1) T / W (T cells, W workgroups), and its stretch is cut again into exactly `wnw` items, none across a group boundary.
// The cuts are chosen by a small dynamic programme over (workgroup, distance of the cut from its ideal place): every workgroup total
// lies in [A, A + 2] pairs, every item has minlen .. maxlen pairs, and among the plans that do the sum of squared item lengths is
// least -- near-equal items, no needlessly long one.
#pragma once
#include <algorithm>
#include <climits>
#include <vector>

namespace mimsem {

struct WaveItem { int group, lev0, nlev; };      // levels lev0 .. lev0 + nlev of a wave-group; lev0 is even

enum { WAVE_BALANCE_OK = 0, WAVE_BALANCE_ARG = 1, WAVE_BALANCE_INFEASIBLE = 2 };

namespace wave_balance_detail {
// a stretch of `len` cells that begins `off` cells into a group of `P`: the fewest and the most items it can be cut into (0, 0: none),
// every item inside one group and of lo .. hi cells
inline void item_bounds(long long off, long long len, int P, int lo, int hi, int* kmin, int* kmax) {
    int a = 0, b = 0;
    while (len > 0) {
        const long long piece = std::min<long long>(len, P - off);
        if ((piece + hi - 1)/hi > piece/lo) { *kmin = *kmax = 0; return; }
        a += (int)((piece + hi - 1)/hi); b += (int)(piece/lo);
        len -= piece; off = 0;
    }
    *kmin = a; *kmax = b;
}
// ... cut into exactly k items, as equal as the group boundaries allow: the pieces' item lengths, in order
inline long long cut_stretch(long long off, long long len, int P, int lo, int hi, int k, std::vector<int>* out) {
    std::vector<int> piece, cnt;
    while (len > 0) { const int p = (int)std::min<long long>(len, P - off); piece.push_back(p); cnt.push_back((p + hi - 1)/hi); len -= p; off = 0; }
    int have = 0;
    for (int c : cnt) have += c;
    for (; have < k; have++) {                           // one more item for the piece whose items are longest now
        int best = -1;
        for (size_t i = 0; i < piece.size(); i++)
            if ((cnt[i] + 1)*lo <= piece[i] && (best < 0 || (long long)piece[i]*cnt[best] > (long long)piece[best]*cnt[i])) best = (int)i;
        cnt[best]++;
    }
    long long cost = 0;
    for (size_t i = 0; i < piece.size(); i++)
        for (int j = 0; j < cnt[i]; j++) {               // lengths one apart, the longer ones first
            const int l = piece[i]/cnt[i] + (j < piece[i]%cnt[i] ? 1 : 0);
            cost += (long long)l*l;
            if (out) out->push_back(l);
        }
    return cost;
}
}  // namespace wave_balance_detail

// Plans `nwg` workgroups of `wnw` items for `ngroups` wave-groups x `nlev` levels; `default_longest` is the longest item (levels) of the
// default rule, which no item here exceeds by more than a pair.  On WAVE_BALANCE_OK `items` holds wnw x nwg items in launch order with
//   - every (group, level) in exactly one item, an item inside one group, the items of a group neighbours in the order,
//   - every item from an even level over whole level pairs (an odd nlev leaves a group's last item one level short),
//   - the level-pair totals of any two workgroups at most 2 apart,
//   - no item of a single pair unless nlev < 4.
// A workgroup count the call cannot fill that way is WAVE_BALANCE_INFEASIBLE, and `items` comes back empty.
inline int plan_wave_balance(int ngroups, int nlev, int wnw, int nwg, int default_longest, std::vector<WaveItem>& items) {
    using namespace wave_balance_detail;
    items.clear();
    if (ngroups < 1 || nlev < 1 || wnw < 1 || nwg < 1 || default_longest < 1) return WAVE_BALANCE_ARG;
    const int P = (nlev + 1)/2;                           // level pairs of a group
    const long long T = (long long)ngroups*P;
    if ((long long)nwg*wnw >= (1LL << 30) || T >= (1LL << 40)) return WAVE_BALANCE_ARG;
    const int lo = nlev < 4 ? 1 : 2, hi = (default_longest + 1)/2 + 1;
    if ((long long)nwg*wnw*lo > T || (long long)nwg*wnw*hi < T) return WAVE_BALANCE_INFEASIBLE;
    constexpr int D = 2, ND = 2*D + 1;                   // a cut lies within D cells of its ideal place
    auto ideal = [&](int w) { return (long long)(((__int128)T*w + nwg/2)/nwg); };
    constexpr long long INF = LLONG_MAX/4;
    std::vector<long long> cost;
    std::vector<signed char> from;
    // workgroup totals A .. A + 2 around the mean: the window with the mean in its middle first, then the others that hold it
    const long long up = (T + nwg - 1)/nwg;
    const long long windows[3] = {up - 1, up - 2, T%nwg == 0 ? up : -1};
    bool found = false;
    for (int wi = 0; wi < 3 && !found; wi++) {
        const long long A = windows[wi];
        if (A < 0) continue;
        cost.assign((size_t)(nwg + 1)*ND, INF);
        from.assign((size_t)(nwg + 1)*ND, -1);
        cost[D] = 0;                                     // cut 0 at cell 0
        for (int w = 0; w < nwg; w++)
            for (int d = 0; d < ND; d++) {
                if (cost[(size_t)w*ND + d] >= INF) continue;
                const long long beg = ideal(w) + d - D;
                for (int e = 0; e < ND; e++) {
                    const long long end = ideal(w + 1) + e - D, len = end - beg;
                    if ((w + 1 == nwg && e != D) || end > T || len < A || len > A + 2 || len < 1) continue;
                    int kmin, kmax;
                    item_bounds(beg%P, len, P, lo, hi, &kmin, &kmax);
                    if (kmin < 1 || kmin > wnw || kmax < wnw) continue;
                    const long long cs = cost[(size_t)w*ND + d] + cut_stretch(beg%P, len, P, lo, hi, wnw, nullptr);
                    if (cs < cost[(size_t)(w + 1)*ND + e]) { cost[(size_t)(w + 1)*ND + e] = cs; from[(size_t)(w + 1)*ND + e] = (signed char)d; }
                }
            }
        found = cost[(size_t)nwg*ND + D] < INF;
    }
    if (!found) return WAVE_BALANCE_INFEASIBLE;
    std::vector<long long> cut(nwg + 1);
    for (int w = nwg, d = D; w >= 0; w--) { cut[w] = ideal(w) + d - D; if (w) d = from[(size_t)w*ND + d]; }
    items.reserve((size_t)nwg*wnw);
    std::vector<int> lens;
    for (int w = 0; w < nwg; w++) {
        lens.clear();
        cut_stretch(cut[w]%P, cut[w + 1] - cut[w], P, lo, hi, wnw, &lens);
        long long cell = cut[w];
        for (int l : lens) {
            const int p0 = (int)(cell%P);
            items.push_back(WaveItem{(int)(cell/P), 2*p0, std::min(nlev, 2*(p0 + l)) - 2*p0});
            cell += l;
        }
    }
    return WAVE_BALANCE_OK;
}

}  // namespace mimsem
