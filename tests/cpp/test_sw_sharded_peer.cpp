// tests/cpp/test_sw_sharded_peer.cpp -- the shallow-water Picard step (row N3) on SEVERAL RANKS driven from C++ over the ONE-SIDED halo transport:
// src::SWEqn of mimsem_amd/host/mimsem_sweqn.hpp over a Shard on Shard::use_peer (hipIpc-opened receive buffers, pack and unpack as kernels
// only), so every Picard iteration after the first of its kind is a replay of ONE recorded hipGraph per rank.  The ranks are separate
// PROCESSES of this binary (process_ranks.hpp: hipIpc cannot open a process's own buffers); the all-gather of the buffer handles and the
// all-reduce of the check norms go through the rendezvous file.  The case files are those of test_sw_sharded.cpp (one per rank).
//   usage: test_sw_sharded_peer <world> <rank> <rendezvous file> <case prefix> <out prefix> <nsteps> [mark]
//   mark: rank 1 writes a time-out into its pair plan's error word after its first step (mimsem_halo_peer_mark_for_test) -- every rank must
//         then stop with HaloTimeout after the next Picard iteration's all-reduce, exit code process_ranks::EXIT_HALO_TIMEOUT.
#include <chrono>
#include <cstdio>
#include <string>
#include "../../mimsem_amd/host/mimsem_sweqn.hpp"
#include "../../mimsem_amd/host/sw_io.hpp"
#include "process_ranks.hpp"

using namespace mimsem_host;
using process_ranks::World;

namespace {
struct Counted { World* w; long reductions = 0; };
int allreduce(void* user, double* v, int n) { Counted* c = (Counted*)user; c->reductions++; return c->w->allreduce(v, n); }
}  // namespace

int main(int argc, char** argv) {
    if (argc < 7) { std::fprintf(stderr, "usage: test_sw_sharded_peer world rank rendezvous case_prefix out_prefix nsteps [mark]\n"); return process_ranks::EXIT_USAGE; }
    const int world = std::atoi(argv[1]), rank = std::atoi(argv[2]), nsteps = std::atoi(argv[6]);
    const bool mark = argc > 7 && std::string(argv[7]) == "mark";
    if (world < 2 || world > 6 || nsteps < 1) return process_ranks::EXIT_USAGE;
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
        double* fg = mesh.to_device(a.reals("fg").data(), a.reals("fg").size());
        double *un = mesh.to_device(a.reals("u").data(), a.reals("u").size()), *hn = mesh.to_device(a.reals("h").data(), a.reals("h").size());
        const auto& par = a.reals("params");              // dt, nits, q_exact
        src::SWEqn sw(&mesh, fg, &sh);
        long red_setup = 0, red_steps = 0, iters = 0, iters_all = 0;
        double seconds = 0.0;
        try {
            for (int s = 0; s < nsteps; s++) {
                const long r0 = rc.reductions;
                if (s == 1) W.barrier();                      // (the timed steps start together)
                const auto t0 = std::chrono::steady_clock::now();
                sw.solve(un, hn, par[0], false, (int)par[1], par[2] != 0.0);
                double probe = 0.0;
                mesh.to_host(&probe, hn, 1);                  // (waits for the step's last copies)
                if (s > 0) seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                iters_all += (long)sw.history.size();
                if (s == 0) red_setup = rc.reductions - r0;   // (the first step estimates the spectral regions: inner products, all-reduced)
                else { red_steps += rc.reductions - r0; iters += (long)sw.history.size(); }
                if (mark && s == 0 && rank == 1) check(mimsem_halo_peer_mark_for_test(sh.pair, 1), "mimsem_halo_peer_mark_for_test");
            }
        } catch (const HaloTimeout& e) {
            std::printf("rank %d: HaloTimeout: %s\n", rank, e.what());
            std::fflush(stdout);
            W.barrier();                                      // (every rank has stopped: nobody's buffers are in use any more)
            std::_Exit(process_ranks::EXIT_HALO_TIMEOUT);
        }
        std::vector<double> u(mesh.n1), h(mesh.n2);
        mesh.to_host(u.data(), un, u.size()); mesh.to_host(h.data(), hn, h.size());
        const std::string out = std::string(argv[5]) + std::to_string(rank) + ".bin";
        FILE* g = std::fopen(out.c_str(), "wb");
        if (!g) throw std::runtime_error("cannot write " + out);
        std::fwrite(u.data(), 8, u.size(), g); std::fwrite(h.data(), 8, h.size(), g);
        std::fclose(g);
        const int timeouts = sh.peer_timeouts();
        std::printf("rank %d: chebyshev steps [%d, %d, %d], recalibrations %d, fallbacks %d, Picard iterations %ld, graph_nodes first %d later %d, replays %ld, "
                    "exchanges per iteration first %ld later %ld, all-reduces in the set-up step %ld, in the %ld Picard iterations after it %ld, "
                    "uncached %d, peer_timeouts %d, steps/s %.1f, |dx|/|x| last %.3e\n",
                    rank, sw.steps_A, sw.steps_M1, sw.steps_q, sw.recalibrations, sw.fallbacks, iters_all, sw.graph_nodes(true), sw.graph_nodes(false), sw.replays,
                    sw.exchanges_per_iteration(true), sw.exchanges_per_iteration(false), red_setup, iters, red_steps, sh.uncached() ? 1 : 0, timeouts,
                    nsteps > 1 && seconds > 0.0 ? (nsteps - 1)/seconds : 0.0, sw.history.empty() ? 0.0 : sw.history.back());
        bool ok = true;
        // the contract of the sharded fixed-length mode: ONE all-reduce per Picard iteration once the regions are known, none inside a solve
        if (nsteps > 1 && red_steps != iters) { std::printf("rank %d FAIL: all-reduces != Picard iterations\n", rank); ok = false; }
        if (sw.fallbacks != 0 || sw.recalibrations != 0) { std::printf("rank %d FAIL: a check missed\n", rank); ok = false; }
        if (timeouts != 0) { std::printf("rank %d FAIL: an exchange timed out\n", rank); ok = false; }
        std::fflush(stdout);
        W.barrier();                                          // (no rank frees its receive buffers while a neighbour may still write them)
        mimsem_free(un); mimsem_free(hn); mimsem_free(fg);
        if (!ok) return process_ranks::EXIT_FAIL;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rank %d FAIL: %s\n", rank, e.what());
        W.fail(process_ranks::EXIT_FAIL);
    }
    std::printf("rank %d DONE\n", rank);
    return process_ranks::EXIT_OK;
}
