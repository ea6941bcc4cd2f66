// verdictplan_host.cpp — TEST-ONLY: csrc/verdictplan.h's verdict_shape over given sizes, as a plain g++ program (no HIP, no device).
//   verdictplan_host < sizes     one line per case: n_cols n_rules n_trig n_lits force_global mode n_passes
//   -> per case: waves lds_bytes lds_tables sparse v_cap per_cu launchable bit_regs blocks_per_304_cus wave_lds_el(v_cap)
// tests/test_verdict_edges_cpu.py sweeps the sizes and checks the answers against the kernel's encoding and a restatement in Python.
#include <cstdio>

#include "../pingoo_amd/csrc/verdictplan.h"

int main() {
    unsigned n_cols, n_rules, n_trig, n_lits, force_global, n_passes;
    int mode;
    while (scanf("%u %u %u %u %u %d %u", &n_cols, &n_rules, &n_trig, &n_lits, &force_global, &mode, &n_passes) == 7) {
        const pwaf::VerdictShape s = pwaf::verdict_shape(n_cols, n_rules, n_trig, n_lits, force_global != 0, mode, n_passes);
        printf("%u %u %u %u %u %u %u %u %u %u\n", s.waves, s.lds_bytes, s.lds_tables, s.sparse, s.v_cap, s.per_cu, pwaf::verdict_launchable(s, n_cols) ? 1u : 0u,
               pwaf::verdict_variant(n_passes) ? 1u : 4u, pwaf::verdict_blocks_sp(s, 304), pwaf::verdict_wave_lds_el(n_cols, n_rules, s.v_cap));
    }
    return 0;
}
