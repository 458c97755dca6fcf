// tests/cpp/wave_balance_cli.cpp -- prints the plan of csrc/wave_balance.hpp for tests/test_wave_balance_cpu.py (host only, no HIP).
//   wave_balance_cli NGROUPS NLEV WNW NWG DEFAULT_LONGEST [drop | double]
// stdout: the status, the number of items, then one "group lev0 nlev" line per item in launch order.  `drop` and `double` spoil a
// good plan by one level (the last level of an item in the middle taken away / given to its successor as well): what the test's
// checker must notice.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../mimsem_amd/csrc/wave_balance.hpp"

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: %s ngroups nlev wnw nwg default_longest [drop|double]\n", argv[0]); return 2; }
    std::vector<mimsem::WaveItem> items;
    const int rc = mimsem::plan_wave_balance(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), items);
    if (argc > 6 && rc == mimsem::WAVE_BALANCE_OK) {
        mimsem::WaveItem& it = items[items.size()/2];
        if (!strcmp(argv[6], "drop")) it.nlev -= 1;
        else if (!strcmp(argv[6], "double")) { mimsem::WaveItem& nx = items[items.size()/2 + 1]; if (nx.group == it.group) { nx.lev0 -= 2; nx.nlev += 2; } else it.nlev += 1; }
    }
    printf("%d %zu\n", rc, items.size());
    for (const mimsem::WaveItem& it : items) printf("%d %d %d\n", it.group, it.lev0, it.nlev);
    return 0;
}
