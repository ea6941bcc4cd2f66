// lscan_split.h — how the list-driven DFA passes of a batch are cut into list-scan launches (host code only).
//
// launch_scan_gated (scan.hip) takes at most kListLaunchMax descriptors: lscan_plan_kernel gives each one of its 256 threads. Phase 0
// (the passes behind a prefilter and the identity passes) holds up to two descriptors per pass — a confirm pass's dense alternative and
// its R-tier walk — so 250 passes can need 500. A phase with more is split into consecutive launches on the batch's stream, each with a
// plan region of its own (2 * count + 1 words: work-item prefix sums and total, then the entries per item of every descriptor). A pass's
// descriptors never straddle two launches. plan_passes (scanplan.cpp) computes the launches when the passes get their roles — at creation
// and after pwaf_engine_tune — and run_pipeline follows them. Compiled by scanplan.cpp, pipeline.cpp and tests/lscan_split_host.cpp (g++: the CPU
// suite checks the split).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace pwaf {
namespace lsplit {

static constexpr uint32_t kListLaunchMax = 256;  // descriptors per launch_scan_gated call (lscan_plan_kernel's threads)

// what run_pipeline needs to know of a pass to build its list-scan descriptors
struct PassKind {
    bool identity;      // a plain pass over a short field: walks the identity list (phase 0)
    bool gated;         // list-driven: walks a prefilter's candidate list or a gap pass's list
    bool filtered;      // ... behind a bigram prefilter (phase 0); else a gated gap pass (phase 1)
    bool confirm;       // the prefilter has a confirm tier
    bool confirm_walk;  // ... some of whose candidates still need the DFA walk
    bool dense_alt;     // ... and the flag-density switch is on: the pass also has its dense alternative
};

// descriptors the pass adds to `phase`, in the order run_pipeline pushes them: the dense alternative, then the walk
inline uint32_t descriptors(const PassKind &k, int phase) {
    if (k.identity) return phase == 0 ? 1u : 0u;
    if (!k.gated || k.filtered != (phase == 0)) return 0u;
    if (phase == 1) return 1u;
    return (k.dense_alt && k.confirm ? 1u : 0u) + (k.confirm && !k.confirm_walk ? 0u : 1u);
}

// One phase's launches: per_pass[i] = the descriptors of pass i (in pass order, at most kListLaunchMax each); returns the descriptor
// count of every launch, in order (none for an empty phase). Greedy: a launch takes whole passes while they fit.
inline std::vector<uint32_t> split(const uint32_t *per_pass, size_t n_passes, uint32_t cap = kListLaunchMax) {
    std::vector<uint32_t> launches;
    uint32_t cur = 0;
    for (size_t i = 0; i < n_passes; i++) {
        if (per_pass[i] == 0) continue;
        if (cur + per_pass[i] > cap) {
            launches.push_back(cur);
            cur = 0;
        }
        cur += per_pass[i];
    }
    if (cur) launches.push_back(cur);
    return launches;
}

// plan words of a set of launches (the list-scan plan regions, one behind the other)
inline size_t plan_words(const std::vector<uint32_t> &launches) {
    size_t w = 0;
    for (uint32_t c : launches) w += 2u * (size_t)c + 1u;
    return w;
}

}  // namespace lsplit
}  // namespace pwaf
