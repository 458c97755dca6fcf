// tests/cpp/test_ksp_owned.cpp -- the reference's ksp1 call sequence (eul/HorizSolve.cpp:77-96) with the reference's own preconditioner:
//   KSPCreate(&ksp1); KSPSetOperators(ksp1, M1->M, M1->M); KSPSetTolerances(ksp1, 1.0e-16, 1.0e-50, PETSC_DEFAULT, 1000);
//   KSPSetType(ksp1, KSPGMRES); PCSetType(pc, PCBJACOBI); PCBJacobiSetTotalBlocks(pc, size*nElsX*nElsX, NULL);  KSPSolve(ksp1, b, x)
// over the shim's KSP (setPCBJacobiOwned: exact inverses of the assembled owned blocks) on the whole sphere the pytest wrapper wrote
// (tests/test_gpu_cpp_ksp_owned.py), checked against the wrapper's dense solve of the oracle's assembled M1.
//   usage: test_ksp_owned <in.arr>      (arrays: the mesh tables, "b", "x_dense")
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../mimsem_amd/host/mimsem_shim.hpp"
#include "../../mimsem_amd/host/sw_io.hpp"

using namespace mimsem_host;

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: test_ksp_owned in.arr\n"); return 2; }
    try {
        const ArrayFile a = read_arrays(argv[1]);
        const mimsem_mesh_desc d = desc_of(a);
        Mesh mesh(d);
        const int n1 = d.n1;
        const std::vector<double>& b = a.reals("b");
        const std::vector<double>& want = a.reals("x_dense");
        double *d_b = mesh.to_device(b.data(), n1), *d_x = mesh.device_alloc(n1);
        Umat M1(&mesh, nullptr, nullptr);
        M1.assemble(0, 1.0, false);                              // the src/ flavour: unit scale, no thickness
        KSP ksp1(&mesh);
        ksp1.setOperators(M1);
        ksp1.setTolerances(1.0e-16, 1.0e-50, 1000);
        ksp1.setType(KSP::GMRES);
        ksp1.setPCBJacobiOwned();
        KSPSolve(ksp1, d_b, d_x);
        std::vector<double> x(n1);
        mesh.to_host(x.data(), d_x, n1);
        double num = 0.0, den = 0.0;
        for (int i = 0; i < n1; i++) { num += (x[i] - want[i])*(x[i] - want[i]); den += want[i]*want[i]; }
        const double err = std::sqrt(num/den);
        std::printf("owned PCBJACOBI GMRES: rel L2 = %.3e  (%d iterations, reason %d, rnorm %.3e)\n", err, ksp1.iterations(), ksp1.convergedReason(),
                    ksp1.residualNorm());
        // the element-block default on the same system, for the record
        KSP ksp2(&mesh);
        ksp2.setOperators(M1); ksp2.setTolerances(1.0e-16, 1.0e-50, 1000); ksp2.setType(KSP::GMRES); ksp2.setPCBJacobi();
        KSPSolve(ksp2, d_b, d_x);
        std::printf("element-block PCBJACOBI GMRES: %d iterations\n", ksp2.iterations());
        mimsem_free(d_b); mimsem_free(d_x);
        if (!(err < 1e-12)) { std::printf("FAIL\n"); return 1; }
        std::printf("OK\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
