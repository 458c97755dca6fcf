// tests/cpp/test_horiz_sharded_peer.cpp -- the right-hand sides of the horizontal dynamics (row N2) on SEVERAL RANKS driven from C++ over the
// ONE-SIDED halo transport: mimsem_host::HorizSolve over a Shard on Shard::use_peer, eager launches (the exchanges are kernels; nothing is
// recorded here), the transport's status folded into verify()'s one all-reduce.  The ranks are separate PROCESSES of this binary
// (process_ranks.hpp); the case files are those of test_horiz_sharded.cpp, and so is the output (fu, dG, k2i per rank).
//   usage: test_horiz_sharded_peer <world> <rank> <rendezvous file> <case prefix> <out prefix>
#include <chrono>
#include <cstdio>
#include <string>
#include "../../mimsem_amd/host/mimsem_horizsolve.hpp"
#include "../../mimsem_amd/host/sw_io.hpp"
#include "process_ranks.hpp"

using namespace mimsem_host;
using process_ranks::World;

namespace {
struct Counted { World* w; long reductions = 0; };
int allreduce(void* user, double* v, int n) { Counted* c = (Counted*)user; c->reductions++; return c->w->allreduce(v, n); }
}  // namespace

int main(int argc, char** argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: test_horiz_sharded_peer world rank rendezvous case_prefix out_prefix\n"); return process_ranks::EXIT_USAGE; }
    const int world = std::atoi(argv[1]), rank = std::atoi(argv[2]);
    if (world < 2 || world > 6) return process_ranks::EXIT_USAGE;
    World W(world, rank, argv[3]);
    Counted rc{&W};
    try {
        const std::string in = std::string(argv[4]) + std::to_string(rank) + ".arr";
        const ArrayFile a = read_arrays(in.c_str());
        const mimsem_mesh_desc d = desc_of(a);
        Mesh mesh(d);
        if ((int)a.ints("ranks").size() != world - 1) throw std::runtime_error("this driver expects every rank to neighbour every other");
        Shard sh(&mesh, a.ints("ranks"), a.ints("ghost1"), a.ints("ghost1_off"), a.ints("mirror1"), a.ints("mirror1_off"),
                 a.ints("ghost0"), a.ints("ghost0_off"), a.ints("mirror0"), a.ints("mirror0_off"), a.reals("own0"), a.reals("own1"), &allreduce, &rc);
        sh.use_peer(rank, &World::allgather_cb, &W, world);
        const size_t s1 = (size_t)d.nk*d.n1, s2 = (size_t)d.nk*d.n2;
        auto dev = [&](const char* k) { const auto& v = a.reals(k); return mesh.to_device(v.data(), v.size()); };
        double *fg = dev("fg"), *u1 = dev("u1"), *u2 = dev("u2"), *h1 = dev("h1"), *h2 = dev("h2"), *th = dev("theta"), *Pi = dev("Pi"), *vz = dev("velz"), *dudz = dev("dudz");
        double *dF = mesh.device_alloc(s2), *dG = mesh.device_alloc(s2), *Fk = mesh.device_alloc(s1), *Gk = mesh.device_alloc(s1), *fu = mesh.device_alloc(s1);
        HorizSolve hs(&mesh, fg, (long long)a.reals("params").at(0), true, &sh);
        const long r_setup = rc.reductions, x0 = sh.exchanges;
        const auto t0 = std::chrono::steady_clock::now();
        hs.advection_rhs_ec(u1, u2, h1, h2, th, dF, dG, Fk, Gk);
        hs.momentum_rhs_ec(th, dudz, dudz, vz, vz, Pi, u1, u2, h1, h2, fu, Fk, nullptr, nullptr, nullptr, Fk, hs.last_grad_theta());
        const long r_solves = rc.reductions - r_setup, exch = sh.exchanges - x0;      // all-reduces INSIDE the evaluation: must be none
        const bool ok = hs.verify();
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const double k2i = hs.k2i();
        std::vector<double> hf(s1), hg(s2);
        mesh.to_host(hf.data(), fu, s1); mesh.to_host(hg.data(), dG, s2);
        const std::string out = std::string(argv[5]) + std::to_string(rank) + ".bin";
        FILE* g = std::fopen(out.c_str(), "wb");
        if (!g) throw std::runtime_error("cannot write " + out);
        std::fwrite(hf.data(), 8, s1, g); std::fwrite(hg.data(), 8, s2, g); std::fwrite(&k2i, 8, 1, g);
        std::fclose(g);
        const int timeouts = sh.peer_timeouts();
        std::printf("rank %d: %d Chebyshev steps per mass solve, %d solves checked (worst %.2e), all-reduces: set-up %ld, inside the evaluation %ld; "
                    "exchanges per evaluation %ld; uncached %d, peer_timeouts %d, evaluations/s %.1f, k2i %.12e\n", rank, hs.cheb_steps, hs.solves_checked,
                    hs.worst_rel, r_setup, r_solves, exch, sh.uncached() ? 1 : 0, timeouts, seconds > 0.0 ? 1.0/seconds : 0.0, k2i);
        const bool good = ok && r_solves == 0 && hs.solves_checked >= 6 && timeouts == 0;
        if (!good) std::printf("rank %d FAIL\n", rank);
        std::fflush(stdout);
        W.barrier();                                          // (no rank frees its receive buffers while a neighbour may still write them)
        for (double* p : {fg, u1, u2, h1, h2, th, Pi, vz, dudz, dF, dG, Fk, Gk, fu}) mimsem_free(p);
        if (!good) return process_ranks::EXIT_FAIL;
    } catch (const HaloTimeout& e) {
        std::printf("rank %d: HaloTimeout: %s\n", rank, e.what());
        std::fflush(stdout);
        W.fail(process_ranks::EXIT_HALO_TIMEOUT);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rank %d FAIL: %s\n", rank, e.what());
        W.fail(process_ranks::EXIT_FAIL);
    }
    std::printf("rank %d DONE\n", rank);
    return process_ranks::EXIT_OK;
}
