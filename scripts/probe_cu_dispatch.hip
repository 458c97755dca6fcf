// scripts/probe_cu_dispatch.hip -- where does the dispatcher put the workgroups of a launch shaped like own4::k_apply_wave?
// The balanced level ranges assume that a launch of k x CUs workgroups puts exactly k on every CU.  Each workgroup (256 threads, 48 KB of
// LDS: at most 3 resident per CU, the owner kernel's register bound) reads its hardware id, stays ~20 us so that the whole launch is
// resident at once, and writes the id with an ordinary vector store; the host tallies workgroups per (XCC, SE, SH, CU).
//   hipcc -O2 --offload-arch=gfx950 scripts/probe_cu_dispatch.hip -o build_ab/probe_cu_dispatch && build_ab/probe_cu_dispatch 256 432 512 768
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#define TRY(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e__)); return 1; } } while (0)

__global__ __launch_bounds__(256) void k_probe(unsigned* out, int n, long long ticks) {
    extern __shared__ double lds[];
    const unsigned hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));        // HW_ID: CU_ID 11:8, SH_ID 12, SE_ID 15:13
    const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));      // XCC_ID 3:0
    lds[threadIdx.x] = (double)hw;                                         // (the LDS is really the workgroup's)
    const long long t0 = wall_clock64();
    for (int i = 0; i < 100000 && wall_clock64() - t0 < ticks; i++) __builtin_amdgcn_s_sleep(32);      // bounded
    if (threadIdx.x == 0 && (int)blockIdx.x < n) out[blockIdx.x] = ((xcc & 15u) << 16) | (hw & 0xFF00u) | (lds[0] == (double)hw ? 1u : 0u);
}

int main(int argc, char** argv) {
    int rate = 0;
    TRY(hipDeviceGetAttribute(&rate, hipDeviceAttributeWallClockRate, 0));      // kHz
    hipDeviceProp_t prop;
    TRY(hipGetDeviceProperties(&prop, 0));
    const long long ticks = (long long)rate*20/1000;                            // 20 us
    printf("%s, %d CUs; a workgroup stays %lld ticks of %d kHz\n", prop.name, prop.multiProcessorCount, ticks, rate);
    for (int a = 1; a < argc; a++) {
        const int n = atoi(argv[a]);
        if (n < 1 || n > 4096) continue;
        unsigned* d = nullptr;
        TRY(hipMalloc(&d, n*sizeof(unsigned)));
        for (int rep = 0; rep < 3; rep++) {
            TRY(hipMemset(d, 0, n*sizeof(unsigned)));
            hipLaunchKernelGGL(k_probe, dim3(n), dim3(256), 48*1024, 0, d, n, ticks);
            TRY(hipGetLastError());
            TRY(hipDeviceSynchronize());
            std::vector<unsigned> h(n);
            TRY(hipMemcpy(h.data(), d, n*sizeof(unsigned), hipMemcpyDeviceToHost));
            std::map<unsigned, int> per;
            for (unsigned v : h) per[v & ~1u]++;
            std::map<int, int> hist;
            for (auto& kv : per) hist[kv.second]++;
            printf("%4d workgroups, launch %d: %zu CUs used;", n, rep, per.size());
            for (auto& kv : hist) printf("  %d CUs hold %d", kv.second, kv.first);
            printf("\n");
        }
        TRY(hipFree(d));
    }
    return 0;
}
