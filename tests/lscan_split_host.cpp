// TEST-ONLY: csrc/lscan_split.h (how run_pipeline cuts the list-driven passes into launch_scan_gated calls) compiled with g++ for the CPU
// suite (tests/test_limits_cpu.py). Reads one pass per line from stdin — "identity gated filtered confirm confirm_walk dense_alt" as 0/1 —
// and prints, per phase, the descriptors of every pass and of every launch, and the plan words:
//   {"per_pass": [[..], [..]], "launches": [[..], [..]], "plan_words": W}
#include <cstdio>
#include <vector>

#include "../pingoo_amd/csrc/lscan_split.h"

namespace L = pwaf::lsplit;

int main() {
    std::vector<L::PassKind> passes;
    int v[6];
    while (scanf("%d %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) == 6)
        passes.push_back(L::PassKind{v[0] != 0, v[1] != 0, v[2] != 0, v[3] != 0, v[4] != 0, v[5] != 0});
    std::vector<uint32_t> per_pass[2], launches[2];
    for (int phase = 0; phase < 2; phase++) {
        for (const L::PassKind &k : passes) per_pass[phase].push_back(L::descriptors(k, phase));
        launches[phase] = L::split(per_pass[phase].data(), per_pass[phase].size());
    }
    auto list = [](const std::vector<uint32_t> &x) {
        printf("[");
        for (size_t i = 0; i < x.size(); i++) printf(i ? ", %u" : "%u", x[i]);
        printf("]");
    };
    printf("{\"per_pass\": [");
    list(per_pass[0]);
    printf(", ");
    list(per_pass[1]);
    printf("], \"launches\": [");
    list(launches[0]);
    printf(", ");
    list(launches[1]);
    printf("], \"plan_words\": %zu, \"max_per_launch\": %u}\n", L::plan_words(launches[0]) + L::plan_words(launches[1]), L::kListLaunchMax);
    return 0;
}
