// scripts/probe_dirty_boundary.hip -- what does a launch shaped like own4::k_apply_wave pay at its end for the bytes it
// leaves dirty in L2, and do non-temporal stores take that away?  432 workgroups of 256 threads write B bytes per launch in 16-byte
// stores per lane -- one 128-byte line per workgroup, a quarter, a half and the whole of a buffer of the size of y (30 x 62 208 x 8 B
// = 14.9 MB) -- with plain stores and with `nt` stores; 2 000 back-to-back launches per cell, the host clock around one synchronise,
// three samples per cell.  Vector stores only: no write-through forms, no fences, no atomics.
//   hipcc -O2 --offload-arch=gfx950 scripts/probe_dirty_boundary.hip -o build_ab/probe_dirty_boundary && build_ab/probe_dirty_boundary
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>

#define TRY(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e__)); return 1; } } while (0)

typedef double d2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) d2 gd2;

constexpr int WGS = 432, TPB = 256;
constexpr long long NVEC = 30LL*62208*8/16;              // 16-byte units of the buffer

// nvec <= NVEC units written per launch, unit i by lane i mod (WGS*TPB); line != 0: lanes 0..7 of a workgroup write its own 128-byte line
template <bool NT>
__global__ __launch_bounds__(TPB) void k_write(double* buf, long long nvec, int line, double v) {
    gd2* const p = (gd2*)buf;
    d2 val; val.x = v; val.y = v + (double)threadIdx.x;
    if (line) {
        if (threadIdx.x >= 8) return;
        const long long i = (long long)blockIdx.x*8 + threadIdx.x;         // < WGS*8 <= NVEC
        if (i >= nvec) return;
        if constexpr (NT) __builtin_nontemporal_store(val, p + i); else p[i] = val;
        return;
    }
    for (long long i = (long long)blockIdx.x*TPB + threadIdx.x; i < nvec; i += (long long)WGS*TPB) {
        if constexpr (NT) __builtin_nontemporal_store(val, p + i); else p[i] = val;
    }
}

int main() {
    hipDeviceProp_t prop;
    TRY(hipGetDeviceProperties(&prop, 0));
    double* buf = nullptr;
    TRY(hipMalloc(&buf, NVEC*16));
    TRY(hipMemset(buf, 0, NVEC*16));
    printf("%s, %d CUs; %d workgroups of %d threads, 2000 back-to-back launches per sample, us per launch\n", prop.name, prop.multiProcessorCount, WGS, TPB);
    struct Cell { const char* name; long long nvec; int line; };
    const Cell cells[4] = {{"one line per workgroup", (long long)WGS*8, 1}, {"quarter", NVEC/4, 0}, {"half", NVEC/2, 0}, {"whole", NVEC, 0}};
    for (const Cell& c : cells) {
        for (int nt = 0; nt < 2; nt++) {
            double us[3];
            for (int s = 0; s < 3; s++) {
                std::chrono::steady_clock::time_point t0;
                for (int i = -50; i < 2000; i++) {          // 50 launches of warm-up, then the timed 2 000
                    if (i == 0) { TRY(hipDeviceSynchronize()); t0 = std::chrono::steady_clock::now(); }
                    if (nt) hipLaunchKernelGGL(k_write<true>, dim3(WGS), dim3(TPB), 0, 0, buf, c.nvec, c.line, (double)i);
                    else    hipLaunchKernelGGL(k_write<false>, dim3(WGS), dim3(TPB), 0, 0, buf, c.nvec, c.line, (double)i);
                }
                TRY(hipGetLastError());
                TRY(hipDeviceSynchronize());
                us[s] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count()/2000.0;
            }
            printf("%-24s %6.2f MB  %-5s  %6.2f %6.2f %6.2f\n", c.name, c.nvec*16/1e6, nt ? "nt" : "plain", us[0], us[1], us[2]);
            fflush(stdout);
        }
    }
    TRY(hipFree(buf));
    return 0;
}
