// tests/cpp/col_workspace_cli.cpp -- runs every plan of csrc/col_workspace.hpp for tests/test_col_workspace_cpu.py (host only, no HIP).
//   col_workspace_cli NEL NK N2 MP12
// Every plan and path is counted, then carved on a host buffer of exactly the counted doubles.  stdout, per plan and path:
//   plan NAME PATH COUNT              PATH: the carve flags as 0/1 digits ("-" if none)
//   m NAME OFFSET NEED ALIAS          one line per member: OFFSET in doubles from the buffer (-1: null), NEED the doubles its shape
//                                     (BA: nEl ns nn, Band: nEl nr nb nn) says the kernels index (-1: a plain vector), ALIAS the member it
//                                     deliberately shares memory with ("-": none)
// A small buffer is real memory and the first and last double of every member's extent (up to the next member) are written, so that a
// sanitizer build notices a member outside it; a large one is reserved address space that is never touched.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <sys/mman.h>
#include "../../mimsem_amd/csrc/col_workspace.hpp"

using namespace mimsem;

namespace {

struct Member { std::string name; const double* p; long long need; std::string alias; };

struct Run {
    ColDims d;
    std::vector<Member> ms;
    void v(const char* name, const double* p, const char* alias = "-") { ms.push_back({name, p, -1, alias}); }
    void b(const char* name, const BA& x) { ms.push_back({name, x.p, x.p ? d.nEl*x.ns*d.nn() : -1, "-"}); }
    void b(const char* name, const Band& x, const char* alias = "-") { ms.push_back({name, x.p, x.p ? d.nEl*x.nr*x.nb*d.nn() : -1, alias}); }
};

constexpr long long REAL_MAX = 1LL << 22;      // doubles: above this the buffer is address space only

// counts the plan, carves it on exactly that many doubles, lists its members (`list` fills r.ms from the carved plan)
template <class Plan, class List, class... Path>
int run_plan(const char* name, const char* path, const ColDims& d, List list, Path... flags) {
    Plan p;
    ColArena count;
    p.carve(count, d, flags...);
    if (count.bad) { printf("plan %s %s -1\n", name, path); return 1; }
    const long long n = count.off;
    const bool real = n <= REAL_MAX;
    double* buf = nullptr;
    size_t bytes = (size_t)std::max(n, 1LL)*sizeof(double);
    if (real) buf = new double[(size_t)std::max(n, 1LL)];
    else {
        void* m = mmap(nullptr, bytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (m == MAP_FAILED) { perror("mmap"); return 2; }
        buf = (double*)m;
    }
    ColArena a(buf);
    p.carve(a, d, flags...);
    if (a.bad || a.off != n) { fprintf(stderr, "%s %s: the two runs of the plan disagree\n", name, path); return 2; }
    Run r{d, {}};
    list(r, p);
    printf("plan %s %s %lld\n", name, path, n);
    std::vector<long long> offs;
    for (const Member& m : r.ms) if (m.p) offs.push_back((long long)(m.p - buf));
    offs.push_back(n);
    std::sort(offs.begin(), offs.end());
    for (const Member& m : r.ms) {
        const long long off = m.p ? (long long)(m.p - buf) : -1;
        printf("m %s %lld %lld %s\n", m.name.c_str(), off, m.need, m.alias.c_str());
        if (real && m.p && off >= 0 && off < n) {          // (off == n: a member of zero doubles at the buffer's end)
            const long long next = *std::upper_bound(offs.begin(), offs.end(), off);
            const long long len = m.need >= 0 ? m.need : next - off;
            if (len > 0) { buf[off] = 1.0; buf[off + len - 1] = 2.0; }
        }
    }
    if (real) delete[] buf; else munmap(buf, bytes);
    return 0;
}

std::string bits(std::initializer_list<bool> f) { std::string s; for (bool b : f) s += b ? '1' : '0'; return s; }

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "overflow") {      // two takes whose offsets cannot both be held: the second is refused, nothing wraps
        double one = 0.0;
        ColArena a(&one), count;
        const long long big = LLONG_MAX/8 - 5;
        const bool first = a.take(0) == &one && count.take(big) == nullptr && !count.bad && count.off == big;
        const bool second = count.take(6) == nullptr && count.bad && count.off == big && count.take(-1) == nullptr;
        printf("overflow %d\n", first && second ? 1 : 0);
        return 0;
    }
    if (argc < 5) { fprintf(stderr, "usage: %s nEl nk n2 mp12 | overflow\n", argv[0]); return 2; }
    const ColDims d{atoll(argv[1]), atoll(argv[2]), atoll(argv[3]), atoll(argv[4])};
    int rc = 0;
    for (bool rhs : {false, true})
        rc |= run_plan<ColopWS>("colop", bits({rhs}).c_str(), d, [](Run& r, const ColopWS& w) { r.v("cq", w.cq); r.v("tmpM", w.tmpM); r.v("M", w.M); r.v("frt", w.frt); }, rhs);
    rc |= run_plan<QuadWS>("quad", "-", d, [](Run& r, const QuadWS& w) { r.v("q", w.q); });
    for (long long nlev : {1LL, d.nk})
        rc |= run_plan<BlockInvWS>("blockinv", nlev == 1 ? "0" : "1", d, [](Run& r, const BlockInvWS& w) { r.v("cq", w.cq); r.v("M", w.M); }, nlev);
    rc |= run_plan<SchurWS>("schur", "-", d, [](Run& r, const SchurWS& w) {
        r.v("cq", w.cq); r.v("tmpM", w.tmpM);
        r.b("B", w.B); r.b("Binv", w.Binv); r.b("Ainv", w.Ainv); r.b("T", w.T); r.b("Rr", w.Rr); r.b("X", w.X); r.b("Npi", w.Npi); r.b("Nrho", w.Nrho);
        r.b("M1", w.M1); r.b("G", w.G); r.b("AB0", w.AB0); r.b("AB1", w.AB1); r.b("R2", w.R2); r.b("C2", w.C2); r.b("DIVl", w.DIVl); r.b("DIVu", w.DIVu);
        r.b("Gl", w.Gl); r.b("Gu", w.Gu); r.b("L", w.L);
        r.v("gpi", w.gpi); r.v("geta", w.geta); r.v("rlump", w.rlump); r.v("tA", w.tA); r.v("tB", w.tB); r.v("tC", w.tC);
        r.v("Gws", w.Gws, "G"); r.v("Dinv", w.Dinv, "Npi"); r.v("th_y", w.th_y, "tB"); r.v("th_r", w.th_r, "tA"); r.v("th_dd", w.th_dd, "tC");
    });
    rc |= run_plan<SweepWS>("sweep", "-", d, [](Run& r, const SweepWS& w) {
        r.v("L", w.L); r.v("G", w.G); r.v("D", w.D); r.v("y", w.y); r.v("rl", w.rl); r.v("geta", w.geta); r.v("fu2", w.fu2); });
    for (bool with_wF : {false, true})
        rc |= run_plan<NewtonWS>("newton", bits({with_wF}).c_str(), d, [](Run& r, const NewtonWS& w) {
            r.v("F", w.F); r.v("G", w.G); r.v("u", w.u); r.v("wF", w.wF); r.v("fwA", w.fwA); }, with_wF);
    if (d.nk < 4) return rc;                             // the _3 solve takes nk >= 4
    rc |= run_plan<S3FusedWS>("s3fused", "-", d, [](Run& r, const S3FusedWS& w) {
        r.v("L", w.L); r.v("Fac", w.Fac); r.v("GGl", w.GGl); r.v("GGu", w.GGu); r.v("Mui", w.Mui); r.v("X", w.X); r.v("Binv", w.Binv); r.v("Brti", w.Brti);
        r.v("yws", w.yws); r.v("fu2", w.fu2); r.v("dump", w.dump); });
    for (int f = 0; f < 16; f++) {
        const bool dpp = f & 8, own_cv = f & 4, penta = f & 2, rows = f & 1;
        rc |= run_plan<Schur3WS>("schur3", bits({dpp, own_cv, penta, rows}).c_str(), d, [&](Run& r, const Schur3WS& w) {
            r.v("Tm", w.Tm); r.v("cq", w.cq); r.v("tmpM", w.tmpM);
            r.b("B", w.B); r.b("Ainv", w.Ainv); r.b("V01", w.V01); r.b("V10", w.V10); r.b("Muinv", w.Muinv); r.b("Mrhoinv", w.Mrhoinv); r.b("Npiinv", w.Npiinv);
            r.v("tA", w.tA); r.v("tB", w.tB); r.v("tC", w.tC); r.v("rr", w.rr, "tA");
            r.b("VBA", w.VBA); r.b("Brinv", w.Brinv); r.b("T", w.T); r.b("Rr", w.Rr); r.b("Brt", w.Brt); r.b("Brtinv", w.Brtinv); r.b("Bth", w.Bth); r.b("X", w.X);
            r.b("Cv", w.Cv, dpp && !own_cv ? "VBA" : "-");
            r.b("Drho", w.Drho); r.b("Nrt", w.Nrt); r.b("QM", w.QM); r.b("GN", w.GN); r.b("GG", w.GG); r.b("DDM", w.DDM); r.b("L", w.L);
            r.b("VAB", w.VAB); r.b("t_a", w.t_a); r.b("G_rt", w.G_rt); r.b("DTV1", w.DTV1); r.b("AinvDTV1", w.AinvDTV1); r.b("G_pi", w.G_pi); r.b("DX", w.DX);
            r.b("D_rt", w.D_rt); r.b("t_d", w.t_d); r.b("Q", w.Q); r.b("GNN", w.GNN); r.b("QMD", w.QMD); r.b("DD", w.DD); r.b("DGG", w.DGG);
            r.b("Mrt", w.Mrt, "B");
            r.v("Fac", w.Fac); r.v("yws", w.yws); r.v("fpad", w.fpad); r.v("dpad", w.dpad); r.v("Gws", w.Gws); r.v("Dinv", w.Dinv);
        }, dpp, own_cv, penta, rows);
    }
    return rc;
}
