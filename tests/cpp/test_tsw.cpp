// tests/cpp/test_tsw.cpp -- GalewskyTSW_2's main (src/GalewskyTSW_2.cpp) bound to src::ThermalSW_EEC_2 (mimsem_amd/host/mimsem_thermalsw.hpp):
// init() from quadrature-grid fields (or a given start state), nsteps of solve_rk, writeConservation before and after.  The case and the
// results are named-array files (mimsem_amd/workloads.py::write_arrays / read_arrays); tests/test_gpu_cpp_tsw.py writes the case and
// checks the results.
//   usage: test_tsw <case> <results>
//   case:    the mesh tables (sizes, inds*, det, J, thick, thickInv), fg [n0], dt [1], opts = {nsteps, use_graph, m1h_its, from_quad},
//            uq [nq][2], hq, sq [nq] (from_quad = 1) or u0, h0, S0 (from_quad = 0)
//   results: u0 h0 S0 (the start state), u1 h1 S1 (after nsteps), inv [nsteps + 1][6] (mass buoyancy energy enstrophy vorticity entropy),
//            counters = {steps, host_reads, redone, recordings, graph_nodes, steps_M1}
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "../../mimsem_amd/host/mimsem_thermalsw.hpp"
#include "../../mimsem_amd/host/sw_io.hpp"

using namespace mimsem_host;

static void write_arrays(const char* path, const std::map<std::string, std::vector<double>>& d, const std::map<std::string, std::vector<int>>& i) {
    FILE* f = std::fopen(path, "wb");
    if (!f) throw std::runtime_error(std::string("cannot write ") + path);
    const int count = (int)(d.size() + i.size());
    std::fwrite("MSEMARR1", 1, 8, f); std::fwrite(&count, 4, 1, f);
    auto head = [&](const std::string& name, int type, long long n) {
        const int nl = (int)name.size();
        std::fwrite(&nl, 4, 1, f); std::fwrite(name.data(), 1, (size_t)nl, f); std::fwrite(&type, 4, 1, f); std::fwrite(&n, 8, 1, f);
    };
    for (const auto& kv : d) { head(kv.first, 1, (long long)kv.second.size()); std::fwrite(kv.second.data(), 8, kv.second.size(), f); }
    for (const auto& kv : i) { head(kv.first, 0, (long long)kv.second.size()); std::fwrite(kv.second.data(), 4, kv.second.size(), f); }
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: test_tsw case results\n"); return 2; }
    try {
        const ArrayFile a = read_arrays(argv[1]);
        const mimsem_mesh_desc d = desc_of(a);
        const std::vector<int>& opts = a.ints("opts");
        const int nsteps = opts.at(0), from_quad = opts.at(3);
        const double dt = a.reals("dt").at(0);
        Mesh mesh(d);
        double* fg = mesh.to_device(a.reals("fg").data(), (size_t)d.n0);
        std::map<std::string, std::vector<double>> out;
        std::vector<int> counters;
        {
            src::ThermalSW_EEC_2 tsw(&mesh, fg, d.nq);
            tsw.use_graph = opts.at(1) != 0;
            tsw.m1h_its = opts.at(2);
            double *u = mesh.device_alloc((size_t)d.n1), *h = mesh.device_alloc((size_t)d.n2), *S = mesh.device_alloc((size_t)d.n2);
            if (from_quad) {
                double* uq = mesh.to_device(a.reals("uq").data(), 2*(size_t)d.nq);
                double* hq = mesh.to_device(a.reals("hq").data(), (size_t)d.nq);
                double* sq = mesh.to_device(a.reals("sq").data(), (size_t)d.nq);
                tsw.init(uq, hq, sq, u, h, S);
                mimsem_free(uq); mimsem_free(hq); mimsem_free(sq);
            } else {
                check(mimsem_memcpy_h2d(mesh.ctx, u, a.reals("u0").data(), (long long)d.n1*8), "h2d");
                check(mimsem_memcpy_h2d(mesh.ctx, h, a.reals("h0").data(), (long long)d.n2*8), "h2d");
                check(mimsem_memcpy_h2d(mesh.ctx, S, a.reals("S0").data(), (long long)d.n2*8), "h2d");
            }
            auto grab = [&](const char* name, const double* p, int n) { auto& v = out[name]; v.resize((size_t)n); mesh.to_host(v.data(), p, (size_t)n); };
            grab("u0", u, d.n1); grab("h0", h, d.n2); grab("S0", S, d.n2);
            auto& inv = out["inv"];
            auto put = [&](const src::ThermalSW_EEC_2::Invariants& iv) {
                for (double x : {iv.mass, iv.buoyancy, iv.energy, iv.enstrophy, iv.vorticity, iv.entropy}) inv.push_back(x);
            };
            put(tsw.invariants(u, h, S));
            const long reads0 = tsw.host_reads;
            for (int k = 0; k < nsteps; k++) {
                tsw.solve_rk(u, h, S, dt);
                const long r = tsw.host_reads;
                put(tsw.invariants(u, h, S));
                if (tsw.host_reads != r) throw std::runtime_error("invariants() counted as a read of solve_rk");
            }
            grab("u1", u, d.n1); grab("h1", h, d.n2); grab("S1", S, d.n2);
            counters = {tsw.steps, (int)(tsw.host_reads - reads0), tsw.redone, tsw.recordings, tsw.graph_nodes(), tsw.steps_M1};
            std::printf("steps %d  host reads %d  redone %d  recordings %d  graph nodes %d  M1 Chebyshev steps %d\n",
                        counters[0], counters[1], counters[2], counters[3], counters[4], counters[5]);
            mimsem_free(u); mimsem_free(h); mimsem_free(S);
        }
        mimsem_free(fg);
        write_arrays(argv[2], out, {{"counters", counters}});
        std::printf("OK\n");
    } catch (const std::exception& e) { std::fprintf(stderr, "test_tsw: %s\n", e.what()); return 1; }
    return 0;
}
