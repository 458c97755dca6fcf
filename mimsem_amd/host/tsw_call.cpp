// mimsem_amd/host/tsw_call.cpp -- thermal shallow-water steps with the HOST in C++: src::ThermalSW_EEC_2 of mimsem_thermalsw.hpp (solve_rk of
// src/ThermalSW_EEC_2.cpp:859-1004 over the C ABI) on a case mimsem_amd/workloads.py::write_tsw_case wrote (the mesh tables, fg, dt and the
// GalewskyTSW_2 quadrature-grid fields).  init(), then N steps eagerly and N steps recorded (one hipGraph per step, replayed), each from the
// initial state after the same warm-up; every step is timed on the host clock around solve_rk, which ends in the step's one read of its check
// norms (a device synchronisation).  Built by __graft_entry__.build().
//   usage: tsw_call <case> [steps] [warm-up steps]      prints one JSON object
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mimsem_thermalsw.hpp"
#include "sw_io.hpp"

using namespace mimsem_host;
using clk = std::chrono::steady_clock;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: tsw_call case [steps] [warm-up steps]\n"); return 2; }
    const int nsteps = argc > 2 ? std::atoi(argv[2]) : 20, warm = argc > 3 ? std::atoi(argv[3]) : 3;
    try {
        const ArrayFile a = read_arrays(argv[1]);
        const mimsem_mesh_desc d = desc_of(a);
        const double dt = a.reals("dt").at(0);
        Mesh mesh(d);
        double* fg = mesh.to_device(a.reals("fg").data(), (size_t)d.n0);
        double* uq = mesh.to_device(a.reals("uq").data(), 2*(size_t)d.nq);
        double* hq = mesh.to_device(a.reals("hq").data(), (size_t)d.nq);
        double* sq = mesh.to_device(a.reals("sq").data(), (size_t)d.nq);
        double *u = mesh.device_alloc((size_t)d.n1), *h = mesh.device_alloc((size_t)d.n2), *S = mesh.device_alloc((size_t)d.n2);
        std::printf("{\"elements\": %d, \"order\": %d, \"dt\": %g, \"steps\": %d", d.nEl, d.elOrd, dt, nsteps);
        for (int mode = 0; mode < 2; mode++) {
            src::ThermalSW_EEC_2 tsw(&mesh, fg, d.nq);
            tsw.use_graph = mode == 1;
            tsw.init(uq, hq, sq, u, h, S);
            for (int s = 0; s < warm; s++) tsw.solve_rk(u, h, S, dt);
            const long r0 = tsw.host_reads;
            std::vector<double> ms;
            for (int s = 0; s < nsteps; s++) {
                const auto t0 = clk::now();
                tsw.solve_rk(u, h, S, dt);
                ms.push_back(std::chrono::duration<double, std::milli>(clk::now() - t0).count());
            }
            std::vector<double> srt = ms;
            std::sort(srt.begin(), srt.end());
            const double med = srt.size() % 2 ? srt[srt.size()/2] : 0.5*(srt[srt.size()/2 - 1] + srt[srt.size()/2]);
            double sum = 0.0; for (double x : ms) sum += x;
            std::printf(", \"%s\": {\"ms_per_step_median\": %.4f, \"ms_per_step_min\": %.4f, \"ms_per_step_max\": %.4f, \"ms_per_step_mean\": %.4f, "
                        "\"graph_nodes_per_step\": %d, \"host_reads_per_step\": %.2f, \"redone\": %d, \"m1_chebyshev_steps\": %d}",
                        mode == 0 ? "eager" : "recorded", med, srt.front(), srt.back(), sum/ms.size(), tsw.graph_nodes(),
                        (double)(tsw.host_reads - r0)/nsteps, tsw.redone, tsw.steps_M1);
            if (mode == 1) std::printf(", \"launches_per_step\": %d", tsw.graph_nodes());      // (the eager step issues the same launches)
        }
        std::printf("}\n");
        for (double* p : {fg, uq, hq, sq, u, h, S}) mimsem_free(p);
    } catch (const std::exception& e) { std::fprintf(stderr, "tsw_call: %s\n", e.what()); return 1; }
    return 0;
}
