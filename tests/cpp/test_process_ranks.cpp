// tests/cpp/test_process_ranks.cpp -- the rendezvous of process_ranks.hpp on its own, no GPU: barriers, an all-gather and all-reduces between
// `world` processes of this binary (tests/test_cpp_peer_build.py starts them).
//   usage: test_process_ranks <world> <rank> <rendezvous file> [fail]
//   fail: the last rank gives up at once; the others must leave their next wait with process_ranks::EXIT_PEER_FAILED.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "process_ranks.hpp"

using process_ranks::World;

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: test_process_ranks world rank rendezvous [fail]\n"); return process_ranks::EXIT_USAGE; }
    const int world = std::atoi(argv[1]), rank = std::atoi(argv[2]);
    World W(world, rank, argv[3]);
    if (argc > 4 && std::string(argv[4]) == "fail") {
        if (rank == world - 1) W.fail(process_ranks::EXIT_FAIL);
        for (;;) W.barrier();                            // (left through EXIT_PEER_FAILED)
    }
    int bad = 0;
    for (int round = 0; round < 200; round++) {
        // all-gather: 3 000 bytes per rank, a pattern that names the rank and the round
        std::vector<unsigned char> mine(3000), all((size_t)world*3000);
        for (size_t i = 0; i < mine.size(); i++) mine[i] = (unsigned char)(rank*31 + round*7 + i);
        if (W.allgather(mine.data(), all.data(), (int)mine.size()) != 0) bad++;
        for (int r = 0; r < world; r++)
            for (size_t i = 0; i < mine.size(); i++) if (all[(size_t)r*3000 + i] != (unsigned char)(r*31 + round*7 + i)) { bad++; break; }
        // all-reduce: values whose sum depends on the order -- every rank must hold the rank-order sum, bit for bit
        std::vector<double> v(257), want(257, 0.0);
        for (int i = 0; i < 257; i++) v[i] = std::ldexp(1.0 + rank, 40*rank) + 0.1*i + round;
        for (int r = 0; r < world; r++) for (int i = 0; i < 257; i++) want[i] += std::ldexp(1.0 + r, 40*r) + 0.1*i + round;
        if (W.allreduce(v.data(), 257) != 0) bad++;
        for (int i = 0; i < 257; i++) if (v[i] != want[i]) { bad++; break; }
        W.barrier();
    }
    // the callbacks the host layer is handed
    double one = 1.0;
    if (World::allreduce_cb(&W, &one, 1) != 0 || one != world) bad++;
    std::printf("rank %d: %s\n", rank, bad ? "FAIL" : "DONE");
    return bad ? process_ranks::EXIT_FAIL : process_ranks::EXIT_OK;
}
