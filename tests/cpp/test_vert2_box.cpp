// tests/cpp/test_vert2_box.cpp -- the box twin's Newton loop driven from C++: mimsem_host::VertSolve2 (mimsem_amd/host/mimsem_vertsolve.hpp) with
// theta_up, schur3_flags = 3 and rayleigh = 0 (box/VertSolve.cpp:1264-1458) on the box, geopotential and state the pytest wrapper wrote:
// (0) three iterations with udwdx and a vert_mom_vort callback -- the stand-in uuz_j = cc velz_j, which the wrapper's Python loop takes too: what
//     is checked is WHEN the loop calls it, on WHICH iterate, and the time-centring of the term; (1) three iterations with theta_up and the callback
//     but no udwdx: the callback must not be called (the reference's `if(udwdx)`, :1343, :1403); (2) udwdx without a callback: F_w += dt udwdx.
// States, theta_h, exner_h, the max-norm histories and k2i_z go back to the wrapper, which compares them with the Python loop.
//   usage: test_vert2_box <in.arr> <out.bin>
#include <cstdio>
#include <vector>
#include "../../mimsem_amd/host/mimsem_vertsolve.hpp"
#include "../../mimsem_amd/host/sw_io.hpp"

using namespace mimsem_host;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: test_vert2_box in.arr out.bin\n"); return 2; }
    try {
        const ArrayFile a = read_arrays(argv[1]);
        const mimsem_mesh_desc d = desc_of(a);
        Mesh mesh(d);
        const double dt = a.reals("dt").at(0), cc = a.reals("cc").at(0);
        auto dev = [&](const char* k) { const auto& v = a.reals(k); return mesh.to_device(v.data(), v.size()); };
        double *zv = dev("zv"), *udwdx = dev("udwdx");
        const size_t nl = a.reals("rho").size(), ni = a.reals("velz").size(), nt = nl + (nl - ni);
        FILE* g = std::fopen(argv[2], "wb");
        if (!g) { std::perror(argv[2]); return 2; }
        auto put = [&](const double* p, size_t n) { std::vector<double> h(n); mesh.to_host(h.data(), p, n); std::fwrite(h.data(), 8, n, g); };
        VertSolve2 vs(&mesh, dt);
        vs.theta_up = true; vs.schur3_flags = 3; vs.rayleigh = 0.0;
        for (int run = 0; run < 3; run++) {
            double *velz = dev("velz"), *rho = dev("rho"), *rt = dev("rt"), *exner = dev("exner");
            int ncall = 0;
            vs.vert_mom_vort = nullptr;
            if (run < 2) vs.vert_mom_vort = [&](const double* velz_j, double* uuz_j) {
                ncall++; check(mimsem_vec_combine(mesh.ctx, 1, (long long)ni, cc, velz_j, 0, 0, nullptr, 0, 0.0, nullptr, 0, uuz_j, 0), "vec_combine"); };
            const int its = vs.solve_schur_2(velz, rho, rt, exner, zv, 3, 0.0, run == 1 ? nullptr : udwdx);
            std::printf("run %d: %d iterations, %d callback calls, last norms exner %.3e w %.3e rho %.3e rt %.3e, k2i_z %.6e\n", run, its, ncall,
                        vs.history.back().exner, vs.history.back().w, vs.history.back().rho, vs.history.back().rt, vs.k2i_z);
            if ((int)vs.history.size() != its || ncall != (run == 0 ? its : 0)) { std::printf("FAIL: history length / callback calls\n"); return 1; }
            put(velz, ni); put(rho, nl); put(rt, nl); put(exner, nl); put(vs.theta_half(), nt); put(vs.exner_half(), nl);
            const double meta[2] = {(double)its, vs.k2i_z};
            std::fwrite(meta, 8, 2, g);
            for (const auto& h : vs.history) { const double v[4] = {h.exner, h.w, h.rho, h.rt}; std::fwrite(v, 8, 4, g); }
            for (double* p : {velz, rho, rt, exner}) mimsem_free(p);
        }
        std::fclose(g);
        for (double* p : {zv, udwdx}) mimsem_free(p);
    } catch (const std::exception& e) { std::printf("FAIL: %s\n", e.what()); return 1; }
    std::printf("DONE\n");
    return 0;
}
