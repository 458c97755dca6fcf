// tests/cpp/test_horiz2_box.cpp -- the box mode of mimsem_host::HorizSolve (mimsem_amd/host/mimsem_horizsolve.hpp; box/HorizSolve.cpp:214-324,
// :382-526) driven from C++ on the uniform-layer box and the fields the pytest wrapper wrote: del2; advection_rhs; momentum_rhs with Fz, dwdx and Fk
// (and its k2i) and without them, for do_visc off / on and the element-local forcing composed / by mimsem_horiz_momentum_forcing.  The wrapper
// compares them with the numpy restatement tests/box_strang_case.py -- the check the Python host gets in tests/test_gpu_box_horiz.py.  Then the
// refusals: the _ec routines and diagnose_q throw, and a mesh whose layers differ is refused by the constructor.
//   usage: test_horiz2_box <in.arr> <out.bin>
#include <cstdio>
#include <vector>
#include "../../mimsem_amd/host/mimsem_horizsolve.hpp"
#include "../../mimsem_amd/host/sw_io.hpp"

using namespace mimsem_host;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: test_horiz2_box in.arr out.bin\n"); return 2; }
    try {
        const ArrayFile a = read_arrays(argv[1]);
        const mimsem_mesh_desc d = desc_of(a);
        Mesh mesh(d);
        const int nk = d.nk, n1 = d.n1, n2 = d.n2;
        const double lx = a.reals("lx").at(0);
        const std::vector<double>& thick = a.reals("thick");
        auto dev = [&](const char* k) { const auto& v = a.reals(k); return mesh.to_device(v.data(), v.size()); };
        double *u1 = dev("u1"), *u2 = dev("u2"), *h1 = dev("h1"), *h2 = dev("h2"), *th = dev("theta_i"), *Pi = dev("Pi"), *Fz = dev("Fz");
        double *velz = dev("velz1"), *velz2 = dev("velz2"), *dudz = dev("dudz1"), *dudz2 = dev("dudz2"), *dwdx1 = dev("dwdx1"), *dwdx2 = dev("dwdx2");
        const size_t s1 = (size_t)nk*n1, s2 = (size_t)nk*n2;
        double *dF = mesh.device_alloc(s2), *dG = mesh.device_alloc(s2), *Fk = mesh.device_alloc(s1), *Gk = mesh.device_alloc(s1);
        double *fuA = mesh.device_alloc(s1), *fuB = mesh.device_alloc(s1);
        FILE* g = std::fopen(argv[2], "wb");
        if (!g) { std::perror(argv[2]); return 2; }
        auto put = [&](const double* p, size_t n) { std::vector<double> h(n); mesh.to_host(h.data(), p, n); std::fwrite(h.data(), 8, n, g); };
        for (int visc = 0; visc < 2; visc++) {
            HorizSolve hs(&mesh, HorizSolve::Box{lx, thick.data(), thick.size()}, visc == 1);
            if (!hs.box_mode() || hs.fused_forcing) { std::printf("FAIL: box mode / default switches\n"); return 1; }
            if (visc == 0) {
                std::fwrite(&hs.del2, 8, 1, g);
                hs.advection_rhs(u1, u2, h1, h2, th, dF, dG, Fk, Gk);
                put(dF, s2); put(dG, s2); put(Fk, s1); put(Gk, s1);
            }
            for (int fused = 0; fused < 2; fused++) {
                hs.fused_forcing = fused == 1;
                hs.momentum_rhs(th, dudz, dudz2, velz, velz2, Pi, u1, u2, nullptr, nullptr, fuA, nullptr, Fz, dwdx1, dwdx2, Fk);
                const double k2i = hs.k2i();
                hs.momentum_rhs(th, dudz, dudz2, velz, velz2, Pi, u1, u2, nullptr, nullptr, fuB);
                if (hs.k2i() != 0.0) { std::printf("FAIL: k2i without Fk\n"); return 1; }
                if (!hs.verify()) { std::printf("FAIL: a fixed-length 1-form mass solve missed its check (worst %.2e)\n", hs.worst_rel); return 1; }
                std::printf("do_visc %d fused_forcing %d: k2i %.16e, %d solves checked, worst %.2e\n", visc, fused, k2i, hs.solves_checked, hs.worst_rel);
                put(fuA, s1); put(fuB, s1);
                std::fwrite(&k2i, 8, 1, g);
            }
            if (visc == 1) {                                                  // no box twin
                int thrown = 0;
                try { hs.advection_rhs_ec(u1, u2, h1, h2, th, dF, dG, Fk, Gk); } catch (const std::runtime_error&) { thrown++; }
                try { hs.momentum_rhs_ec(th, dudz, dudz2, velz, velz2, Pi, u1, u2, h1, h2, fuA); } catch (const std::runtime_error&) { thrown++; }
                try { hs.diagnose_q(h1, u1, fuA); } catch (const std::runtime_error&) { thrown++; }
                if (thrown != 3) { std::printf("FAIL: %d of 3 routines without a box twin threw\n", thrown); return 1; }
            }
        }
        std::fclose(g);
        {                                                                     // layers that differ: refused
            std::vector<double> bad(thick);
            bad[bad.size()/2] *= 1.0 + 1.0e-10;
            bool refused = false;
            try { HorizSolve hs(&mesh, HorizSolve::Box{lx, bad.data(), bad.size()}); } catch (const std::runtime_error& e) { refused = true; std::printf("refused: %s\n", e.what()); }
            if (!refused) { std::printf("FAIL: non-uniform layers accepted\n"); return 1; }
        }
        for (double* p : {u1, u2, h1, h2, th, Pi, Fz, velz, velz2, dudz, dudz2, dwdx1, dwdx2, dF, dG, Fk, Gk, fuA, fuB}) mimsem_free(p);
    } catch (const std::exception& e) { std::printf("FAIL: %s\n", e.what()); return 1; }
    std::printf("DONE\n");
    return 0;
}
