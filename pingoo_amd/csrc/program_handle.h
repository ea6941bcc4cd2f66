// program_handle.h — what a pwaf_program handle holds (include/pwaf.h), and the two host-side calls every unit behind the C ABI shares.
// Host-only: included by program_api.cpp (plain C++) and, through engine_impl.h, by the HIP-compiled units (an engine owns a pwaf_program).
#pragma once
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "program.h"
#include "scanplan.h"

struct pwaf_program {
    std::unique_ptr<pwaf::Program> p;
    std::vector<uint8_t> dump;  // lazily built
    // what the list-scan hooks answer from (pwaf_program_flat_image, pwaf_program_list_scans): the profile of the latest tuning sample
    // (null: never tuned), the mean field lengths the samples so far left, and the plan built from them on the first call
    std::unique_ptr<pwaf::TuneOut> tuned;
    std::vector<double> mean_len;
    std::unique_ptr<pwaf::ProgramScans> scans;
    void keep_tuning(const pwaf::TuneOut &T) {
        tuned.reset(new pwaf::TuneOut(T));
        mean_len.resize(std::max(mean_len.size(), T.mean_len.size()), 0.0);
        for (size_t f = 0; f < T.mean_len.size(); f++)
            if (T.mean_len[f] > 0) mean_len[f] = T.mean_len[f];
        scans.reset();
        dump.clear();
    }
};

namespace pwaf {
int fail(int code, const std::string &msg);  // program_api.cpp: records pwaf_last_error(); also used by loaders.cpp, node.cpp, the planners
#pragma GCC visibility push(hidden)
int validate_batch_header(const pwaf_batch *b);  // program_api.cpp
#pragma GCC visibility pop
}  // namespace pwaf
