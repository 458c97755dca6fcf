// tests/cpp/test_vert2.cpp -- the Newton loop of solve_schur_column_3 driven from C++: mimsem_host::VertSolve2 (mimsem_amd/host/mimsem_vertsolve.hpp,
// VertSolve::solve_schur_2, eul/VertSolve.cpp:1059-1246, on the library's fused entry points) on the patch, geopotential and state the pytest
// wrapper wrote: (0) three iterations without forcing, (1) three iterations with the Held-Suarez temperature forcing, the u dw/dx term and a
// horizontal forcing (the callback hands out the arrays of the file), (2) the loop run to its stopping test.  States, theta_h, exner_h, the
// max-norm histories and k2i_z go back to the wrapper, which compares them with the Python loop.
//   usage: test_vert2 <in.arr> <out.bin>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../mimsem_amd/host/mimsem_vertsolve.hpp"
#include "../../mimsem_amd/host/sw_io.hpp"

using namespace mimsem_host;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: test_vert2 in.arr out.bin\n"); return 2; }
    try {
        const ArrayFile a = read_arrays(argv[1]);
        const mimsem_mesh_desc d = desc_of(a);
        Mesh mesh(d);
        const double dt = a.reals("dt").at(0);
        auto dev = [&](const char* k) { const auto& v = a.reals(k); return mesh.to_device(v.data(), v.size()); };
        double *zv = dev("zv"), *lat = dev("lat"), *udwdx = dev("udwdx"), *dFx = dev("dFx"), *dGx = dev("dGx");
        const size_t nl = a.reals("rho").size(), ni = a.reals("velz").size(), nt = nl + (nl - ni);
        FILE* g = std::fopen(argv[2], "wb");
        if (!g) { std::perror(argv[2]); return 2; }
        auto put = [&](const double* p, size_t n) { std::vector<double> h(n); mesh.to_host(h.data(), p, n); std::fwrite(h.data(), 8, n, g); };
        VertSolve2 vs(&mesh, dt);
        for (int run = 0; run < 3; run++) {
            double *velz = dev("velz"), *rho = dev("rho"), *rt = dev("rt"), *exner = dev("exner");
            int ncall = 0;
            vs.horiz_forcing = nullptr;
            if (run == 1) vs.horiz_forcing = [&](const double*, const double*, const double*, double* oF, double* oG) {
                ncall++; mesh.copy(nl, dFx, oF); mesh.copy(nl, dGx, oG); };
            const int its = run == 0 ? vs.solve_schur_2(velz, rho, rt, exner, zv, 3, 0.0)
                          : run == 1 ? vs.solve_schur_2(velz, rho, rt, exner, zv, 3, 0.0, udwdx, lat)
                                     : vs.solve_schur_2(velz, rho, rt, exner, zv, 40, 1.0e-12);
            std::printf("run %d: %d iterations, last norms exner %.3e w %.3e rho %.3e rt %.3e, k2i_z %.6e\n", run, its, vs.history.back().exner,
                        vs.history.back().w, vs.history.back().rho, vs.history.back().rt, vs.k2i_z);
            if ((int)vs.history.size() != its || (run == 1 && ncall != its)) { std::printf("FAIL: history length / forcing calls\n"); return 1; }
            put(velz, ni); put(rho, nl); put(rt, nl); put(exner, nl); put(vs.theta_half(), nt); put(vs.exner_half(), nl);
            const double meta[2] = {(double)its, vs.k2i_z};
            std::fwrite(meta, 8, 2, g);
            for (const auto& h : vs.history) { const double v[4] = {h.exner, h.w, h.rho, h.rt}; std::fwrite(v, 8, 4, g); }
            for (double* p : {velz, rho, rt, exner}) mimsem_free(p);
        }
        std::fclose(g);
        // the stop rule tests THREE norms (:1202): a second "rank" whose rt norm alone is still large keeps this one iterating (the eta loop's
        // two-norm rule would stop); the MAX reduction runs once per iteration, the SUM of k2i_z once per solve
        {
            int nmax = 0, nsum = 0;
            vs.horiz_forcing = nullptr;
            vs.allreduce_max = [&](double* v, int n) { nmax++; if (n == 4) v[3] = std::max(v[3], 1.0); };
            vs.allreduce_sum = [&](double*, int) { nsum++; };
            double *velz = dev("velz"), *rho = dev("rho"), *rt = dev("rt"), *exner = dev("exner");
            const int its = vs.solve_schur_2(velz, rho, rt, exner, zv, 6, 1.0e-2);
            VertSolve2 one(&mesh, dt);
            double *v1 = dev("velz"), *r1 = dev("rho"), *t1 = dev("rt"), *e1 = dev("exner");
            const int its1 = one.solve_schur_2(v1, r1, t1, e1, zv, 6, 1.0e-2);
            if (its != 6 || its1 >= 6 || nmax != 6 || nsum != 1) {
                std::printf("FAIL: three-norm stop rule: alone %d iterations, with an unconverged rt %d, max calls %d, sum calls %d\n", its1, its, nmax, nsum); return 1;
            }
            std::printf("three-norm stop rule: alone %d iterations, with an unconverged rt norm %d\n", its1, its);
            for (double* p : {velz, rho, rt, exner, v1, r1, t1, e1}) mimsem_free(p);
        }
        for (double* p : {zv, lat, udwdx, dFx, dGx}) mimsem_free(p);
    } catch (const std::exception& e) { std::printf("FAIL: %s\n", e.what()); return 1; }
    std::printf("DONE\n");
    return 0;
}
