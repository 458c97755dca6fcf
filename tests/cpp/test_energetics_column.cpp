// tests/cpp/test_energetics_column.cpp -- mimsem_host::Euler::energetics_column (mimsem_amd/host/mimsem_shim.hpp) called once on the mesh,
// velz, rho and zv the pytest wrapper wrote (vertical layout); the four sums kev, k2p, p2k, pe go back to the wrapper, which compares them
// with the restatement of tests/energetics_case.py.
//   usage: test_energetics_column <in.arr> <out.bin>
#include <cstdio>
#include <vector>
#include "../../mimsem_amd/host/mimsem_shim.hpp"
#include "../../mimsem_amd/host/sw_io.hpp"

using namespace mimsem_host;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: test_energetics_column in.arr out.bin\n"); return 2; }
    try {
        const ArrayFile a = read_arrays(argv[1]);
        const mimsem_mesh_desc d = desc_of(a);
        Mesh mesh(d);
        auto dev = [&](const char* k) { const auto& v = a.reals(k); return mesh.to_device(v.data(), v.size()); };
        double *velz = dev("velz"), *rho = dev("rho"), *zv = dev("zv");
        // the LINEAR_INV blocks [nEl][nk-1][n2e][n2e]: geometry only, made once (vo->AssembleLinearInv)
        const size_t nEl = (size_t)a.reals("dims").at(0), n2e = (size_t)a.reals("dims").at(1);
        const int nb = mimsem_colop_nblocks(mesh.ctx, MIMSEM_V_LINEAR_INV);
        if (nb < 1) { std::printf("FAIL: %d LINEAR_INV blocks\n", nb); return 1; }
        double* inv = mesh.device_alloc(nEl*nb*n2e*n2e);
        check(mimsem_colop_blocks(mesh.ctx, MIMSEM_V_LINEAR_INV, 0, nullptr, nullptr, inv), "colop_blocks(LINEAR_INV)");
        double* out = mesh.device_alloc(4);
        Euler euler(&mesh);
        euler.energetics_column(velz, rho, zv, inv, out);
        double h[4];
        mesh.to_host(h, out, 4);
        std::printf("kev %.16e k2p %.16e p2k %.16e pe %.16e\n", h[0], h[1], h[2], h[3]);
        FILE* g = std::fopen(argv[2], "wb");
        if (!g) { std::perror(argv[2]); return 2; }
        std::fwrite(h, 8, 4, g);
        std::fclose(g);
        for (double* p : {velz, rho, zv, inv, out}) mimsem_free(p);
    } catch (const std::exception& e) { std::printf("FAIL: %s\n", e.what()); return 1; }
    std::printf("DONE\n");
    return 0;
}
