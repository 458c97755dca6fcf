// tests/cpp/test_box_entropy.cpp -- mimsem_host::Euler::log_entropy (mimsem_amd/host/mimsem_shim.hpp) called from a process without torch on
// the mesh, theta and lz the pytest wrapper wrote: slot 11 of the box's energetics line (box/Euler_2.cpp:979-997) as a C++ host forms it.
// theta holds nrows rows `pitch` doubles apart (pitch >= n2: the wrapper pads the rows); the value of two calls goes back to the wrapper,
// which compares it with Engine.log_entropy and the numpy sum.
//   usage: test_box_entropy <in.arr> <out.bin>        dims = [nrows, pitch, factor]
#include <cstdio>
#include <vector>
#include "../../mimsem_amd/host/mimsem_shim.hpp"
#include "../../mimsem_amd/host/sw_io.hpp"

using namespace mimsem_host;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: test_box_entropy in.arr out.bin\n"); return 2; }
    try {
        const ArrayFile a = read_arrays(argv[1]);
        const mimsem_mesh_desc d = desc_of(a);
        Mesh mesh(d);
        auto dev = [&](const char* k) { const auto& v = a.reals(k); return mesh.to_device(v.data(), v.size()); };
        const int nrows = (int)a.reals("dims").at(0);
        const long long pitch = (long long)a.reals("dims").at(1);
        const double factor = a.reals("dims").at(2);
        if (a.reals("theta").size() < (size_t)(nrows - 1)*pitch + 1 || a.reals("lz").size() != (size_t)nrows) {
            std::printf("FAIL: theta / lz do not hold %d rows\n", nrows); return 1; }
        double *theta = dev("theta"), *lz = dev("lz");
        double* out = mesh.device_alloc(2);
        Euler euler(&mesh);
        euler.log_entropy(nrows, theta, pitch, lz, factor, out);
        euler.log_entropy(nrows, theta, pitch, lz, factor, out + 1);
        double h[2];
        mesh.to_host(h, out, 2);
        std::printf("entropy %.16e %.16e\n", h[0], h[1]);
        FILE* g = std::fopen(argv[2], "wb");
        if (!g) { std::perror(argv[2]); return 2; }
        std::fwrite(h, 8, 2, g);
        std::fclose(g);
        for (double* p : {theta, lz, out}) mimsem_free(p);
    } catch (const std::exception& e) { std::printf("FAIL: %s\n", e.what()); return 1; }
    std::printf("DONE\n");
    return 0;
}
