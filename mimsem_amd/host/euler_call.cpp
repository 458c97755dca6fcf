// mimsem_amd/host/euler_call.cpp -- steps of the 3-D compressible Euler equations with the HOST in C++: mimsem_host::eul::Euler of mimsem_euler.hpp
// (Strang_ec of eul/Euler_2.cpp:1366-1557 or, with --integrator strang, Strang :1146-1364, the integrator of eul/HeldSuarez.cpp, over the C ABI; the loop
// of eul/UMJS14.cpp:347-353) on a case mimsem_amd/workloads.py::write_euler_case wrote (scripts/run_umjs14.py --write-case: the mesh tables, fg, zv, dt
// and the initial state).  A case with `lx` in place of `fg` (scripts/run_bubble.py --write-case) is the doubly periodic box: mimsem_host::box::Euler,
// the box twin's Strang (box/Euler_2.cpp:1306-1477, the loop of box/Bubble.cpp:208-215).  Warm-up steps -- the first finds the
// fixed lengths of the interface solves --, then N steps, each timed on the host clock around Strang_ec, which ends in the read of the
// energetics line (a device synchronisation).  Built by __graft_entry__.build().
//   usage: euler_call <case> [steps] [warm-up steps] [--integrator strang_ec|strang]      prints one JSON object
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "mimsem_euler.hpp"
#include "sw_io.hpp"

using namespace mimsem_host;
using clk = std::chrono::steady_clock;

int main(int argc, char** argv) {
    std::vector<const char*> pos; const char* integrator = "strang_ec";
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--integrator") && i + 1 < argc) integrator = argv[++i]; else pos.push_back(argv[i]);
    }
    const bool strang = !std::strcmp(integrator, "strang");
    if (pos.empty() || (!strang && std::strcmp(integrator, "strang_ec"))) {
        std::fprintf(stderr, "usage: euler_call case [steps] [warm-up steps] [--integrator strang_ec|strang]\n"); return 2; }
    const int nsteps = pos.size() > 1 ? std::atoi(pos[1]) : 20, warm = pos.size() > 2 ? std::atoi(pos[2]) : 2;
    try {
        const ArrayFile a = read_arrays(pos[0]);
        const mimsem_mesh_desc d = desc_of(a);
        const std::vector<int>& opts = a.ints("opts");
        const double dt = a.reals("dt").at(0);
        const int nk = d.nk;
        Mesh mesh(d);
        DeviceArrays mem;
        auto dev = [&](const char* k) { const auto& v = a.reals(k); double* p = mem.get(v.size()); check(mimsem_memcpy_h2d(mesh.ctx, p, v.data(), (long long)v.size()*8), "h2d"); return p; };
        const bool is_box = a.has("lx");
        double *fg = is_box ? nullptr : dev("fg"), *zv = dev("zv"), *velx = dev("velx"), *velz = dev("velz"), *rho = dev("rho"), *rt = dev("rt"), *exner = dev("exner");
        eul::Euler::Options o = is_box ? box::default_options() : eul::Euler::Options();
        o.hs_forcing = opts.at(1) != 0; o.newton_maxit = opts.at(2); o.do_visc = opts.at(4) != 0; o.newton_tol = a.reals("newton_tol").at(0);
        if (o.hs_forcing) o.hs_lat = dev("hs_lat");
        std::unique_ptr<eul::Euler> host;
        box::Euler* bx = nullptr;
        if (is_box) {
            const std::vector<double>& thick = a.reals("thick");
            bx = new box::Euler(&mesh, dt, HorizSolve::Box{a.reals("lx").at(0), thick.data(), thick.size()}, zv, o);
            host.reset(bx);
        } else host.reset(new eul::Euler(&mesh, dt, fg, zv, o));
        eul::Euler& eu = *host;
        auto one_step = [&] {
            if (bx) bx->Strang(velx, velz, rho, rt, exner);                 // (the box has this integrator only)
            else if (strang) eu.Strang(velx, velz, rho, rt, exner);
            else eu.Strang_ec(velx, velz, rho, rt, exner);
        };
        for (int s = 0; s < warm; s++) one_step();
        std::vector<double> ms; long newton = 0;
        for (int s = 0; s < nsteps; s++) {
            const auto t0 = clk::now();
            one_step();
            ms.push_back(std::chrono::duration<double, std::milli>(clk::now() - t0).count());
            newton += eu.newton_its;
        }
        std::vector<double> srt = ms;
        std::sort(srt.begin(), srt.end());
        const double med = srt.size() % 2 ? srt[srt.size()/2] : 0.5*(srt[srt.size()/2 - 1] + srt[srt.size()/2]);
        double sum = 0.0; for (double x : ms) sum += x;
        bool finite = true; for (double v : eu.values) if (!(v == v) || v > 1e300 || v < -1e300) finite = false;
        std::printf("{\"integrator\": \"%s\", \"elements\": %d, \"order\": %d, \"levels\": %d, \"dt\": %g, \"steps\": %d, \"warmup\": %d, \"steps_per_s\": %.3f, \"ms_per_step_median\": %.3f, "
                    "\"ms_per_step_min\": %.3f, \"ms_per_step_max\": %.3f, \"ms_per_step_mean\": %.3f, \"newton_per_step\": %.2f, \"redone\": %d, "
                    "\"vort_fixed_its\": [%d, %d], \"m1_chebyshev_steps\": %d, \"m1_solves_checked\": %d, \"finite\": %s}\n",
                    bx ? "box strang" : integrator, d.nEl, d.elOrd, nk, dt, nsteps, warm, 1.0e3/med, med, srt.front(), srt.back(), sum/ms.size(), (double)newton/nsteps, eu.redone,
                    eu.vort.m_its[0], eu.vort.m_its[1], eu.horiz.cheb_steps, eu.horiz.solves_checked, finite ? "true" : "false");
        return finite ? 0 : 1;
    } catch (const std::exception& e) { std::fprintf(stderr, "euler_call: %s\n", e.what()); return 1; }
}
