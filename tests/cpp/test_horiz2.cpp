// tests/cpp/test_horiz2.cpp -- the non-_ec right-hand sides of the horizontal dynamics driven from C++: mimsem_host::HorizSolve::advection_rhs and
// momentum_rhs (mimsem_amd/host/mimsem_horizsolve.hpp; eul/HorizSolve.cpp:330-375, :496-635; theta on the nk + 1 interfaces) on the mesh and fields
// the pytest wrapper wrote, once per setting of the switches: 0 = all off (composed), 1 = fused_hu, 2 = fused_forcing, 3 = fused_phi, 4 = all three.
// Per setting: dF, dG, Fk, Gk; fu with dwdx and Fk, and its k2i; fu without dwdx / Fz / Fk.  The wrapper compares them with the numpy restatement
// tests/strang2_case.py -- the check the Python host gets in tests/test_gpu_horiz_rhs2.py.
//   usage: test_horiz2 <in.arr> <out.bin>
#include <cstdio>
#include <vector>
#include "../../mimsem_amd/host/mimsem_horizsolve.hpp"
#include "../../mimsem_amd/host/sw_io.hpp"

using namespace mimsem_host;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: test_horiz2 in.arr out.bin\n"); return 2; }
    try {
        const ArrayFile a = read_arrays(argv[1]);
        const mimsem_mesh_desc d = desc_of(a);
        Mesh mesh(d);
        const int nk = d.nk, n1 = d.n1, n2 = d.n2;
        auto dev = [&](const char* k) { const auto& v = a.reals(k); return mesh.to_device(v.data(), v.size()); };
        double *fg = dev("fg"), *u1 = dev("u1"), *u2 = dev("u2"), *h1 = dev("h1"), *h2 = dev("h2"), *th = dev("theta_i"), *Pi = dev("Pi");
        double *velz = dev("velz1"), *velz2 = dev("velz2"), *dudz = dev("dudz1"), *dudz2 = dev("dudz2"), *dwdx1 = dev("dwdx1"), *dwdx2 = dev("dwdx2");
        const size_t s1 = (size_t)nk*n1, s2 = (size_t)nk*n2;
        double *dF = mesh.device_alloc(s2), *dG = mesh.device_alloc(s2), *Fk = mesh.device_alloc(s1), *Gk = mesh.device_alloc(s1);
        double *fuA = mesh.device_alloc(s1), *fuB = mesh.device_alloc(s1);
        FILE* g = std::fopen(argv[2], "wb");
        if (!g) { std::perror(argv[2]); return 2; }
        auto put = [&](const double* p, size_t n) { std::vector<double> h(n); mesh.to_host(h.data(), p, n); std::fwrite(h.data(), 8, n, g); };
        HorizSolve hs(&mesh, fg);
        if (hs.fused_hu || hs.fused_forcing || hs.fused_phi) { std::printf("FAIL: a switch is on by default\n"); return 1; }
        for (int mode = 0; mode < 5; mode++) {
            hs.fused_hu = mode == 1 || mode == 4; hs.fused_forcing = mode == 2 || mode == 4; hs.fused_phi = mode == 3 || mode == 4;
            hs.advection_rhs(u1, u2, h1, h2, th, dF, dG, Fk, Gk);
            hs.momentum_rhs(th, dudz, dudz2, velz, velz2, Pi, u1, u2, h1, h2, fuA, nullptr, nullptr, dwdx1, dwdx2, Fk);
            const double k2i = hs.k2i();
            hs.momentum_rhs(th, dudz, dudz2, velz, velz2, Pi, u1, u2, h1, h2, fuB);
            if (hs.k2i() != 0.0) { std::printf("FAIL: k2i without Fk\n"); return 1; }
            if (!hs.verify()) { std::printf("FAIL: a fixed-length 1-form mass solve missed its check (worst %.2e)\n", hs.worst_rel); return 1; }
            std::printf("mode %d: k2i %.16e, %d solves checked, worst %.2e\n", mode, k2i, hs.solves_checked, hs.worst_rel);
            put(dF, s2); put(dG, s2); put(Fk, s1); put(Gk, s1); put(fuA, s1); put(fuB, s1);
            std::fwrite(&k2i, 8, 1, g);
        }
        std::fclose(g);
        for (double* p : {fg, u1, u2, h1, h2, th, Pi, velz, velz2, dudz, dudz2, dwdx1, dwdx2, dF, dG, Fk, Gk, fuA, fuB}) mimsem_free(p);
    } catch (const std::exception& e) { std::printf("FAIL: %s\n", e.what()); return 1; }
    std::printf("DONE\n");
    return 0;
}
