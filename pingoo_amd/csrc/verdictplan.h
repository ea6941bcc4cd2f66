// verdictplan.h — the launch shape of the verdict kernels and the LDS layout it is computed from: entry capacity, waves per workgroup,
// workgroups per CU, program tables in LDS or not. The layout helpers are what the kernels themselves lay their LDS out with (verdict.hip:
// verdict_kernel, verdict2_kernel); verdict_shape and verdict_blocks_sp are host code. No HIP header in here: hipcc compiles it into
// verdict.hip (the helpers then also for the device), g++ into program_api.cpp (pwaf_program_verdict_shape) and tests/verdictplan_host.cpp
// — the CPU suite checks the shape over sizes up to the limits (tests/test_verdict_edges_cpu.py).
#pragma once
#include <stdint.h>

#include <algorithm>

// PWAF_HOST_DEVICE: a plain function for host and device (program.h's definition, repeated for the programs that include this file alone)
#ifndef PWAF_HOST_DEVICE
#if defined(__HIPCC__)
#define PWAF_HOST_DEVICE __host__ __device__
#else
#define PWAF_HOST_DEVICE
#endif
#endif

namespace pwaf {

struct VerdictShape {
    uint32_t waves, lds_bytes, lds_tables;
    uint32_t sparse, v_cap, per_cu;  // sparse: 1 = the sparse column file, 2 = the entry list (verdict2_kernel); (verdict.hip: verdict_kernel<.., SP>): value slots per wave, workgroups per CU
};

PWAF_HOST_DEVICE static inline uint32_t verdict_wave_lds(uint32_t n_cols, uint32_t n_rules) {
    const uint32_t colw = (n_cols + 31) / 32, rulew = (n_rules + 31) / 32;
    return ((n_cols * 8 + colw * 4 + rulew * 4 + n_rules * 2) + 15) & ~15u;  // columns, bitmaps, candidates (also: the list of non-zero columns)
}

// SPARSE column file (verdict_kernel<.., SP = true>): of a rule set's ~1000 - 4500 columns a group of 64 requests dirties a hundred or two,
// yet the dense file costs 8 bytes per COLUMN and wave — 9 KiB of the 1k-rule set's 11.5 KiB per wave, which is what held the kernel at
// one workgroup of 11 waves per CU (under 3 waves per SIMD; 57 % of its wave cycles waiting: VERDICT r4). The sparse file keeps, per 32
// columns, the dirty bits and the number of dirty columns before the word (8 bytes), and one 64-bit value per DIRTY column, at the
// column's rank among the dirty ones: ~4 KiB per wave whatever the rule set, i.e. two workgroups of 12 waves per CU. A group is marked
// twice — bits first (the ranks need all of them), values second — and a value read is two dependent LDS reads instead of one. A group
// with more dirty columns than the value array holds (v_cap) keeps the rest in a per-wave spill array in global memory (same results).
PWAF_HOST_DEVICE static inline uint32_t verdict_wave_lds_sp(uint32_t n_cols, uint32_t n_rules, uint32_t v_cap) {
    const uint32_t colw = (n_cols + 31) / 32, rulew = (n_rules + 31) / 32;
    return ((colw * 8 + v_cap * 8 + rulew * 4 + n_rules * 2) + 15) & ~15u;  // {dirty bits, rank} per 32 columns, values, rule bitmap, candidates
}
PWAF_HOST_DEVICE static inline uint32_t verdict_v_cap(uint32_t n_cols, bool tiny) {
    const uint32_t v = tiny ? 8u : 256u + n_cols / 16u;
    return v < n_cols ? v : n_cols;
}

// ENTRY LIST (verdict2_kernel): vals | rule bitmap | entry columns (u16) | candidates (u16) | slot bytes
PWAF_HOST_DEVICE static inline uint32_t verdict_wave_lds_el(uint32_t n_cols, uint32_t n_rules, uint32_t e_cap) {
    const uint32_t rulew = (n_rules + 31) / 32;
    return (e_cap * 8 + rulew * 4 + ((e_cap * 2 + 3) & ~3u) + ((n_rules * 2 + 3) & ~3u) + ((n_cols + 7) & ~7u) + 15) & ~15u;
}

// LDS-resident copies of the small read-mostly program tables (LT = true): trigger lists, rule headers and DNF literals are
// gathered several times per 64-request group, and each gather from L2 is a ~1 us round trip that the few waves a CU can hold
// (the column files fill LDS) cannot hide.
struct VerdictTables {
    uint32_t bitcol, trig_off, trig_rules, rules, lits, pub, end;  // byte offsets from the start of the table region
};
PWAF_HOST_DEVICE static inline VerdictTables verdict_tables(uint32_t n_cols, uint32_t n_rules, uint32_t n_trig, uint32_t n_lits, bool lt) {
    VerdictTables t;
    t.bitcol = 0;
    t.trig_off = 0;
    t.trig_rules = t.trig_off + (lt ? ((n_cols + 1) * 2 + 3) & ~3u : 0u);
    t.rules = t.trig_rules + (lt ? (n_trig * 2 + 7) & ~7u : 0u);
    t.lits = t.rules + (lt ? n_rules * 8 : 0u);
    t.pub = t.lits + (lt ? n_lits * 4 : 0u);
    t.end = t.pub + (lt ? (n_rules * 2 + 3) & ~3u : 0u);
    return t;
}

// which of the two bitmap-register instantiations a pass count selects (verdict_kernel / verdict2_kernel <.., BR, ..>): 1 = BR 1, up to 64
// passes; 0 = the general one
inline int verdict_variant(uint32_t n_passes) { return n_passes <= 64 ? 1 : 0; }

// Workgroup shape of the verdict kernel: as many waves as LDS (160 KiB) holds column files for, next to one copy of the program
// tables; if the tables do not leave room for at least 4 column files they stay in global memory (LT = false).
// force_global (PWAF_OPT_GLOBAL_VERDICT_TABLES): take the variant whose program tables stay in global memory even when they would fit LDS
// mode: 3 = entry list (default), 4 = entry list with 8 entry slots (PWAF_OPT_TINY_VERDICT_SLOTS: the spill path's test hook); 0 = the dense column file
// (PWAF_OPT_DENSE_VERDICT), 1 = the sparse column file of round 5 (PWAF_OPT_SPARSE_VERDICT), 2 = that with 8 value slots (both flags)
static constexpr uint32_t kLdsPerGroup = 160u * 1024u;
inline VerdictShape verdict_shape(uint32_t n_cols, uint32_t n_rules, uint32_t n_trig, uint32_t n_lits, bool force_global = false, int mode = 3, uint32_t n_passes = 0) {
    VerdictShape s{};
    const uint32_t t_lds = verdict_tables(n_cols, n_rules, n_trig, n_lits, true).end, t_glb = verdict_tables(n_cols, n_rules, n_trig, n_lits, false).end;
    if (mode >= 3) {
        // ENTRY LIST (mode 3; 4 = the test hook with 8 entry slots: every group takes the spill path): as many 12-wave workgroups per CU as
        // LDS holds, and the largest entry capacity that does not cost a wave (a group of the 1k-rule set appends 50-100 entries)
        s.sparse = 2;
        const uint32_t cu_waves = verdict_variant(n_passes) ? 24u : 16u;
        auto fit = [&](uint32_t cap, uint32_t &bw, uint32_t &bk, uint32_t &lt) {
            const uint32_t wave = verdict_wave_lds_el(n_cols, n_rules, cap);
            const bool fits = !force_global && n_trig < 65536 && t_lds + 8 * wave <= kLdsPerGroup;
            const uint32_t tables = fits ? t_lds : t_glb;
            bw = 0; bk = 1; lt = fits ? 1u : 0u;
            for (uint32_t k = 1; k <= 3; k++) {
                const uint32_t share = kLdsPerGroup / k;
                if (share <= tables + wave) continue;
                const uint32_t w = std::min(std::min(12u, cu_waves / k), (share - tables) / wave);
                if (w * k > bw * bk) { bw = w; bk = k; }
            }
        };
        uint32_t cap = 8, bw = 0, bk = 1, lt = 0;
        if (mode == 4) fit(cap, bw, bk, lt);
        else {
            uint32_t w0, k0, l0;
            fit(64, w0, k0, l0);  // the occupancy the smallest capacity reaches ...
            for (uint32_t c : {254u, 224u, 192u, 160u, 128u, 96u, 64u}) {  // ... kept by the largest capacity that still reaches it
                fit(c, bw, bk, lt);
                cap = c;
                if (bw * bk >= w0 * k0) break;
            }
        }
        s.v_cap = cap;
        s.waves = bw;
        s.per_cu = bk;
        s.lds_tables = lt;
        s.lds_bytes = (lt ? t_lds : t_glb) + bw * verdict_wave_lds_el(n_cols, n_rules, cap);
        return s;
    }
    if (mode != 0) {
        // SPARSE column file (mode 1; 2 = the test hook with 8 value slots): as many workgroups of 12 waves per CU as LDS holds (two for
        // the 1k-rule set: 6 waves per SIMD), program tables in LDS when one such workgroup still fits beside them
        s.sparse = 1;
        s.v_cap = verdict_v_cap(n_cols, mode == 2);
        const uint32_t wave = verdict_wave_lds_sp(n_cols, n_rules, s.v_cap);
        const bool fits = !force_global && n_trig < 65536 && t_lds + 8 * wave <= kLdsPerGroup;
        s.lds_tables = fits ? 1 : 0;
        const uint32_t tables = fits ? t_lds : t_glb;
        // (registers: the variant for up to 64 passes is compiled for 6 waves per SIMD = 24 per CU, the general one takes 124 -> 16 per CU)
        const uint32_t cu_waves = verdict_variant(n_passes) ? 24u : 16u;
        uint32_t best_w = 0, best_k = 1;
        for (uint32_t k = 1; k <= 3; k++) {  // k workgroups per CU
            const uint32_t share = kLdsPerGroup / k;
            if (share <= tables + wave) continue;
            const uint32_t w = std::min(std::min(12u, cu_waves / k), (share - tables) / wave);
            if (w * k > best_w * best_k) { best_w = w; best_k = k; }
        }
        s.waves = best_w;
        s.per_cu = best_k;
        s.lds_bytes = tables + s.waves * wave;
        return s;
    }
    const uint32_t wave = verdict_wave_lds(n_cols, n_rules);
    const bool fits = !force_global && n_trig < 65536 && t_lds + 4 * wave <= kLdsPerGroup;
    s.lds_tables = fits ? 1 : 0;
    const uint32_t tables = fits ? t_lds : t_glb;
    uint32_t w = tables + wave <= kLdsPerGroup ? (kLdsPerGroup - tables) / wave : 0;
    if (!fits) w = std::min(w, 4u);  // small workgroups: several share a CU
    s.waves = std::min(w, 16u);
    s.per_cu = 1;
    s.lds_bytes = tables + s.waves * wave;
    return s;
}

// what pwaf_engine_create refuses and launch_verdict never launches: no wave's column file fits LDS, or a column index beyond 16 bits
inline bool verdict_launchable(const VerdictShape &sh, uint32_t n_cols) { return sh.waves != 0 && n_cols < 65536u; }

inline uint32_t verdict_blocks_sp(const VerdictShape &sh, uint32_t n_cus) { return std::max(1u, n_cus) * sh.per_cu; }  // the sparse kernel's persistent grid (sizes the spill array)

}  // namespace pwaf
