// tests/cpp/test_euler2.cpp -- the step loop of eul/HeldSuarez.cpp:352 bound to mimsem_host::eul::Euler::Strang (mimsem_amd/host/mimsem_euler.hpp): nsteps
// of Strang on the case the pytest wrapper wrote (mimsem_amd/workloads.py::write_euler_case), the state and what the step carries written back
// after every step (named-array files, read with workloads.read_arrays); tests/test_gpu_cpp_strang2.py checks them.  Case and results as
// tests/cpp/test_euler.cpp has them; newton<s> [its][4] holds the norms of solve_schur_2 (exner, w, rho, rt).
//   usage: test_euler2 <case> <results> [switches]        switches: a word naming HorizSolve's switches for the step, of "hu", "phi", "forcing"
#include <cstdio>
#include <map>
#include <string>
#include <vector>
#include "../../mimsem_amd/host/mimsem_euler.hpp"
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
    if (argc < 3) { std::fprintf(stderr, "usage: test_euler2 case results [hu][phi][forcing]\n"); return 2; }
    try {
        const ArrayFile a = read_arrays(argv[1]);
        const mimsem_mesh_desc d = desc_of(a);
        const std::vector<int>& opts = a.ints("opts");
        const int nsteps = opts.at(0), nk = d.nk;
        Mesh mesh(d);
        DeviceArrays mem;
        auto dev = [&](const char* k, size_t want) {
            const auto& v = a.reals(k);
            if (v.size() != want) throw std::runtime_error(std::string("wrong size: ") + k);
            double* p = mem.get(v.size());
            check(mimsem_memcpy_h2d(mesh.ctx, p, v.data(), (long long)v.size()*8), "h2d");
            return p;
        };
        const size_t s1 = (size_t)nk*d.n1, s2 = (size_t)nk*d.n2, i1 = (size_t)(nk - 1)*d.n1, i2 = (size_t)(nk - 1)*d.n2;
        const size_t mp12 = (size_t)(d.quadOrd + 1)*(d.quadOrd + 1);
        double *fg = dev("fg", (size_t)nk*d.n0), *zv = dev("zv", s2);
        double *velx = dev("velx", s1), *velz = dev("velz", i2), *rho = dev("rho", s2), *rt = dev("rt", s2), *exner = dev("exner", s2);
        eul::Euler::Options o;
        o.hs_forcing = opts.at(1) != 0; o.newton_maxit = opts.at(2); o.do_visc = opts.at(4) != 0; o.newton_tol = a.reals("newton_tol").at(0);
        if (o.hs_forcing) o.hs_lat = dev("hs_lat", (size_t)d.nEl*mp12);
        const std::string sw = argc > 3 ? argv[3] : "";
        o.fused_hu = sw.find("hu") != std::string::npos; o.fused_phi = sw.find("phi") != std::string::npos; o.fused_forcing = sw.find("forcing") != std::string::npos;
        std::map<std::string, std::vector<double>> out;
        std::vector<int> per_step;
        eul::Euler eu(&mesh, a.reals("dt").at(0), fg, zv, o);
        if (opts.at(3) > 0) eu.vort.force_its(opts.at(3));
        if (opts.size() > 5 && opts[5] > 0) eu.horiz.shorten_for_test(opts[5]);      // (an M1 solve that must miss its check)
        auto grab = [&](const std::string& name, const double* p, size_t n) { if (!p) return; auto& v = out[name]; v.resize(n); mesh.to_host(v.data(), p, n); };
        for (int s = 1; s <= nsteps; s++) {
            eu.Strang(velx, velz, rho, rt, exner);
            const std::string t = std::to_string(s);
            grab("velx" + t, velx, s1); grab("velz" + t, velz, i2); grab("rho" + t, rho, s2); grab("rt" + t, rt, s2); grab("exner" + t, exner, s2);
            grab("u_prev" + t, eu.u_prev(), s1); grab("u_curr" + t, eu.u_curr(), s1); grab("uz" + t, eu.uz(), i1); grab("uz_prev" + t, eu.uz_prev(), i1);
            out["values" + t] = eu.values;
            auto& nh = out["newton" + t];
            for (const auto& n : eu.newton_history) for (double x : {n.exner, n.w, n.rho, n.eta}) nh.push_back(x);
            for (int x : {eu.newton_its, eu.redone, eu.vort.fixed_its[eul::VortDiag::UZ], eu.vort.fixed_its[eul::VortDiag::DWDX]}) per_step.push_back(x);
            std::printf("step %d  newton %d  redone %d  vort counts %d %d (last fixed %d %d)  M1 steps %d\n", s, eu.newton_its, eu.redone, eu.vort.m_its[0], eu.vort.m_its[1],
                        eu.vort.fixed_its[0], eu.vort.fixed_its[1], eu.horiz.cheb_steps);
        }
        const std::vector<int> counters = {eu.steps, eu.redone, eu.vort.m_its[0], eu.vort.m_its[1], eu.vort.missed, eu.horiz.solves_checked, eu.horiz.solves_missed};
        write_arrays(argv[2], out, {{"counters", counters}, {"per_step", per_step}});
        std::printf("OK\n");
    } catch (const std::exception& e) { std::fprintf(stderr, "test_euler2: %s\n", e.what()); return 1; }
    return 0;
}
