// tests/cpp/process_ranks.hpp -- several RANKS as separate PROCESSES of one driver binary (test_sw_sharded_peer.cpp, test_horiz_sharded_peer.cpp):
// the one-sided halo transport opens the neighbours' receive buffers with hipIpcOpenMemHandle, which a process cannot do on its own buffers, so
// the threads of thread_ranks.hpp cannot run it.  pytest starts `world` fresh processes (no fork after HIP initialisation, no exec) with the
// arguments <world> <rank> <rendezvous file> ...; the rendezvous is a zero-filled file the test creates and every rank maps MAP_SHARED.  It holds
// lock-free std::atomic words for a sense-reversing barrier and byte slots for the all-gather and the all-reduce -- what MPI_Barrier,
// MPI_Allgather and MPI_Allreduce do for a real host.  Every wait is bounded: a rank that does not arrive within LIMIT_S (or that marks the
// rendezvous as failed) ends the waiting ranks with a clear exit code, so a crashed rank cannot leave the others spinning.
// No HIP here: the harness itself runs (and is tested) without a GPU.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace process_ranks {

// exit codes of a rank process (distinct from the shell's 124 / 134 / 137 / 139)
constexpr int EXIT_OK = 0, EXIT_FAIL = 1, EXIT_USAGE = 2, EXIT_HALO_TIMEOUT = 3, EXIT_RENDEZVOUS_TIMEOUT = 4, EXIT_PEER_FAILED = 5;
constexpr int MAX_WORLD = 8;
constexpr size_t GATHER_BYTES = 16384;               // per rank and all-gather
constexpr size_t REDUCE_DOUBLES = 1024;              // per rank and all-reduce
constexpr double LIMIT_S = 120.0;                    // every wait

struct Layout {
    std::atomic<int> arrived;                        // barrier: ranks arrived in the current round
    std::atomic<int> sense;                          // barrier: flips when the round completes
    std::atomic<int> failed;                         // a rank gave up (rank + 1): the others leave at their next wait
    char pad[64 - 3*sizeof(std::atomic<int>)];
    unsigned char gather[MAX_WORLD][GATHER_BYTES];
    double reduce[MAX_WORLD][REDUCE_DOUBLES];
};
static_assert(std::atomic<int>::is_always_lock_free, "the rendezvous needs lock-free atomics (they are shared between processes)");
constexpr size_t FILE_BYTES = sizeof(Layout);

class World {
public:
    World(int size, int rank, const char* path) : size_(size), rank_(rank) {
        if (size < 1 || size > MAX_WORLD || rank < 0 || rank >= size) { std::fprintf(stderr, "process_ranks: bad world %d / rank %d\n", size, rank); std::_Exit(EXIT_USAGE); }
        const int fd = ::open(path, O_RDWR);
        struct stat st {};
        if (fd < 0 || ::fstat(fd, &st) != 0 || (size_t)st.st_size < FILE_BYTES) {
            std::fprintf(stderr, "process_ranks: rendezvous file %s missing or shorter than %zu bytes\n", path, FILE_BYTES); std::_Exit(EXIT_USAGE);
        }
        void* p = ::mmap(nullptr, FILE_BYTES, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        ::close(fd);
        if (p == MAP_FAILED) { std::perror("process_ranks: mmap"); std::_Exit(EXIT_USAGE); }
        L = (Layout*)p;                              // (a zero-filled file: every atomic starts at 0)
    }
    ~World() { ::munmap((void*)L, FILE_BYTES); }
    World(const World&) = delete; World& operator=(const World&) = delete;
    int size() const { return size_; }
    int rank() const { return rank_; }

    // sense-reversing barrier: the last rank to arrive resets the count and flips the sense the others wait for
    void barrier() {
        local_sense_ = 1 - local_sense_;
        if (L->arrived.fetch_add(1, std::memory_order_acq_rel) == size_ - 1) {
            L->arrived.store(0, std::memory_order_relaxed);
            L->sense.store(local_sense_, std::memory_order_release);
            return;
        }
        const auto t0 = std::chrono::steady_clock::now();
        for (long spin = 0; L->sense.load(std::memory_order_acquire) != local_sense_; spin++) {
            if (const int f = L->failed.load(std::memory_order_acquire)) {
                std::fprintf(stderr, "rank %d: rank %d failed, leaving\n", rank_, f - 1); std::fflush(stderr); std::_Exit(EXIT_PEER_FAILED);
            }
            if (spin > 1000) std::this_thread::sleep_for(std::chrono::microseconds(20));
            if ((spin & 1023) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > LIMIT_S) {
                std::fprintf(stderr, "rank %d: the other ranks did not reach the barrier within %.0f s\n", rank_, LIMIT_S); std::fflush(stderr);
                fail(EXIT_RENDEZVOUS_TIMEOUT);
            }
        }
    }
    // MPI_Allgather of `bytes` per rank into all[world][bytes]
    int allgather(const void* mine, void* all, int bytes) {
        if (bytes < 0 || (size_t)bytes > GATHER_BYTES) return 1;
        std::memcpy(L->gather[rank_], mine, (size_t)bytes);
        barrier();
        for (int r = 0; r < size_; r++) std::memcpy((char*)all + (size_t)r*bytes, L->gather[r], (size_t)bytes);
        barrier();                                   // (nobody writes its slot again before everyone has read it)
        return 0;
    }
    // MPI_Allreduce(SUM) of n doubles in place; the sum is formed in rank order on every rank: the same bits everywhere (as thread_ranks.hpp)
    int allreduce(double* v, int n) {
        if (n < 0 || (size_t)n > REDUCE_DOUBLES) return 1;
        std::memcpy(L->reduce[rank_], v, (size_t)n*sizeof(double));
        barrier();
        for (int i = 0; i < n; i++) { double s = 0.0; for (int k = 0; k < size_; k++) s += L->reduce[k][i]; v[i] = s; }
        barrier();
        return 0;
    }
    // this rank gives up: the others leave at their next wait instead of running into the time limit
    [[noreturn]] void fail(int code) {
        int none = 0;
        L->failed.compare_exchange_strong(none, rank_ + 1);
        std::fflush(stdout); std::fflush(stderr);
        std::_Exit(code);
    }

    // the C callbacks of the host layer (user = World*)
    static int allgather_cb(void* user, const void* mine, void* all, int bytes) { return ((World*)user)->allgather(mine, all, bytes); }
    static int allreduce_cb(void* user, double* v, int n) { return ((World*)user)->allreduce(v, n); }

private:
    int size_, rank_, local_sense_ = 0;
    Layout* L = nullptr;
};

}  // namespace process_ranks
