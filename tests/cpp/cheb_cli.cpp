// tests/cpp/cheb_cli.cpp -- prints the arithmetic of namespace cheb (mimsem_amd/host/mimsem_mass.hpp: coefficients, margins, step count,
// acceptance rule) for arguments given on the command line ("inf" and "nan" are numbers here).  CPU only, no library: tests/test_cheb.py.
//   cheb_cli ellipse d c2 steps | margins lo hi lo_prev hi_prev cap_lo cap_hi widen | steps l1 l2 rtol | accepted r2 ref2 bound
#include <cstdio>
#include <cstdlib>
#include <string>
#include "../../mimsem_amd/host/mimsem_mass.hpp"

int main(int argc, char** argv) {
    using namespace mimsem_host;
    const std::string what = argc > 1 ? argv[1] : "";
    auto num = [&](int k) { return std::strtod(argv[k], nullptr); };
    if (what == "ellipse" && argc == 5) {
        for (const auto& ab : cheb::ellipse(num(2), num(3), std::atoi(argv[4]))) std::printf("%.17g %.17g\n", ab.first, ab.second);
    } else if (what == "margins" && argc == 9) {
        const auto m = cheb::margins(num(2), num(3), num(4), num(5), num(6), num(7), num(8));
        std::printf("%.17g %.17g\n", m.first, m.second);
    } else if (what == "steps" && argc == 5) {
        std::printf("%d\n", cheb::interval_steps(num(2), num(3), num(4)));
    } else if (what == "accepted" && argc == 5) {
        std::printf("%d\n", cheb::accepted(num(2), num(3), num(4)) ? 1 : 0);
    } else return 2;
    return 0;
}
