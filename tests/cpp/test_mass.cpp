// tests/cpp/test_mass.cpp -- the pieces the C++ hosts share (mimsem_amd/host/mimsem_mass.hpp) on their own: FixedMassSolve through the
// whole-solve entry and through sweep calls (the same bits in x and in both logged norms), both against the CG of the library (1e-11, the bar
// of test_horiz.cpp), the log accepting, rejecting after shorten(4), and rejecting a pair whose reference norm is no number.
//   usage: test_mass <mesh.arr> <scale> <vert: 0 | 1>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "../../mimsem_amd/host/mimsem_mass.hpp"
#include "../../mimsem_amd/host/sw_io.hpp"

using namespace mimsem_host;

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: test_mass mesh.arr scale vert\n"); return 2; }
    try {
        const ArrayFile a = read_arrays(argv[1]);
        const mimsem_mesh_desc d = desc_of(a);
        const double scale = std::atof(argv[2]), rtol = 1.0e-14;
        const unsigned flags = std::atoi(argv[3]) ? MIMSEM_FLAG_VERT : 0u;
        Mesh mesh(d);
        const int nk = d.nk, n1 = d.n1;
        const size_t tot = (size_t)nk*n1;
        KspHandle ksp(&mesh, MIMSEM_KSP_CG);
        check(mimsem_ksp_set_operator(ksp, MIMSEM_OP_UMAT, 0, nk, scale, flags, nullptr, 0), "mimsem_ksp_set_operator");
        check(mimsem_ksp_set_pc_bjacobi(ksp), "mimsem_ksp_set_pc_bjacobi");
        check(mimsem_ksp_set_tolerances(ksp, rtol, 1.0e-50, 1000, 0, 2), "mimsem_ksp_set_tolerances");
        const double *blocks = nullptr, *escale = nullptr;
        check(mimsem_ksp_get_pc_blocks(ksp, &blocks, &escale, nullptr), "mimsem_ksp_get_pc_blocks");
        FixedMassSolve m1(&mesh, nk, scale, flags);
        m1.use_blocks(blocks, escale);
        if (!m1.calibrate([&](int steps, double* lo, double* hi, double* im) { check(mimsem_ksp_ritz(ksp, steps, lo, hi, im), "mimsem_ksp_ritz"); }, rtol, 0.10, 0.05)) {
            std::printf("FAIL: no usable spectral interval\n"); return 1;
        }
        // b = M1 v for a random v
        DeviceArrays mem;
        double *v = mem.get(tot), *b = mem.get(tot), *xw = mem.get(tot), *xs = mem.get(tot), *xc = mem.get(tot);
        std::vector<double> hv(tot), hw(tot), hs(tot), hc(tot);
        std::mt19937_64 gen(17); std::normal_distribution<double> nd;
        for (double& x : hv) x = nd(gen);
        check(mimsem_memcpy_h2d(mesh.ctx, v, hv.data(), (long long)tot*8), "h2d");
        check(mimsem_op_apply(mesh.ctx, MIMSEM_OP_UMAT, 0, nk, scale, flags, nullptr, 0, v, n1, b, n1, 1.0), "UMAT");
        CheckLog log(&mesh, 3);
        double n[6];
        if (m1.solve(b, xw, log) != MIMSEM_OK) { std::printf("FAIL: the solve is not supported at this order\n"); return 1; }
        const bool whole = m1.whole_solve;                            // (an order without the whole-solve entry: the solve fell to the sweeps)
        m1.whole_solve = false;
        check(m1.solve(b, xs, log), "FixedMassSolve::solve (sweeps)");
        log.read(n);
        mesh.to_host(hw.data(), xw, tot); mesh.to_host(hs.data(), xs, tot);
        std::printf("order %d, %d levels: %d steps, %s, |P r| / |P b| = %.2e\n", d.elOrd, nk, m1.steps, whole ? "whole solve and sweeps" : "sweeps twice", cheb::relative(n[0], n[1]));
        if (std::memcmp(hw.data(), hs.data(), tot*8) != 0) { std::printf("FAIL: whole solve and sweep calls differ in x\n"); return 1; }
        if (std::memcmp(n, n + 2, 16) != 0) { std::printf("FAIL: whole solve and sweep calls differ in the logged norms\n"); return 1; }
        if (!cheb::accepted(n[0], n[1], 30.0*rtol)) { std::printf("FAIL: the log rejects a full-length solve\n"); return 1; }
        check(mimsem_ksp_solve(ksp, b, n1, xc, n1), "mimsem_ksp_solve");
        mesh.to_host(hc.data(), xc, tot);
        double e2 = 0.0, r2 = 0.0;
        for (size_t i = 0; i < tot; i++) { e2 += (hw[i] - hc[i])*(hw[i] - hc[i]); r2 += hc[i]*hc[i]; }
        std::printf("fixed-length against CG: %.2e\n", std::sqrt(e2/r2));
        if (!(std::sqrt(e2/r2) < 1.0e-11)) { std::printf("FAIL: fixed-length solve against the CG\n"); return 1; }
        // a four-step solve must miss, in both forms
        m1.shorten(4);
        log.rewind();
        m1.whole_solve = whole; check(m1.solve(b, xw, log), "FixedMassSolve::solve");
        m1.whole_solve = false; check(m1.solve(b, xs, log), "FixedMassSolve::solve (sweeps)");
        // ... and so must a pair whose reference norm is no number (written from the host)
        const double bad[2] = {1.0e-30, std::numeric_limits<double>::quiet_NaN()};
        check(mimsem_memcpy_h2d(mesh.ctx, log.claim(), bad, 16), "h2d");
        log.read(n);
        for (int k = 0; k < 3; k++)
            if (cheb::accepted(n[2*k], n[2*k + 1], 30.0*rtol)) { std::printf("FAIL: the log accepts slot %d (%s)\n", k, k < 2 ? "a 4-step solve" : "NaN reference"); return 1; }
        std::printf("4-step solve |P r| / |P b| = %.2e: rejected; NaN reference: rejected\n", cheb::relative(n[0], n[1]));
        bool threw = false;
        try { log.claim(); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("FAIL: a full log took another slot\n"); return 1; }
    } catch (const std::exception& e) { std::printf("FAIL: %s\n", e.what()); return 1; }
    std::printf("OK\n");
    return 0;
}
