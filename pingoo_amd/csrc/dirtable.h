// dirtable.h — the host side of the IPv4 lookup table: run compression of the flat DIR-24 table and the choice of its summary bitmap.
// A pure function of the table dir24_kernel wrote (2^24 entries: class | set << 16, or the escape flag | index), so that the CPU
// suite runs the very code pwaf_engine_create runs (tests/dirtable_host.cpp), next to a scalar restatement of the lookup.
//
// Compressed for the lookups (round 3): 10M uniformly random addresses against the flat 64 MiB table are 10M misses to HBM (the
// batch's own 3 GB of streaming flush every cache level in between). Consecutive /24s mostly share their entry (a /20 prefix
// covers 16 of them), so per /16 the 256 entries are stored as RUNS, 32 /24s per 16-byte record (8 records = one 128-byte line
// per /16): {bitmap of the /24s of this group where a run starts, the entry in force when the group begins, the entry of the
// first run that starts inside it, where the entries of further runs live in `vals`}. One 16-byte gather answers every lookup
// whose /24 lies in the carried-in run or in the first run of its group (nearly all: ~12 runs per /16 over 8 groups); 8 MiB for
// any table: L2 / Infinity-Cache resident. (Measured: the lookup kernel is bound by the NUMBER of scattered load instructions —
// the texture addresser takes them one lane-address at a time — not by bytes or latency: four loads per lookup from one line
// took as long as four from different lines.)
//
// The summary bitmap (round 6; kernels.h: VerdictArgs::dir_summary). Most of the address space holds ONE entry — for a WAF
// rule set the one that says "no list holds this address and no rule asks about its GeoIP record" — so one bit per block
// of /24s answers most lookups from a bitmap small enough to stay in every XCD's L2. Granularity: /20 ... /24 blocks,
// whichever minimises (fraction of the space that still needs the table) + (bitmap bytes / 8 MiB); no summary when more
// than half of the blocks need the table anyway, or when the caller asks for none (PWAF_OPT_NO_DIR_SUMMARY).
//
// The coarse bitmap in front of the summary (kernels.h: VerdictArgs::dir_coarse). The summary lookup is still one scattered global
// load per request — one lane address through the texture addresser and one L1 -> L2 line for one bit — and that NUMBER is what
// bounds the kernel (above). A bitmap over larger blocks fits in LDS, where a gather costs neither: one bit per block of
// 2^coarse_shift /24s, 1 = some /24 of the block differs from `common` (= the OR of the block's summary bits), staged once per
// workgroup by ipres_kernel<.., COARSE>. A clear bit ends the lookup without a global load; a set bit continues with the summary
// exactly as before, so the answers are the same by construction. Built only in front of a summary, with the summary's own rule
// (at most half of the coarse blocks set), at the smallest shift whose bitmap fits the LDS budget of the kernel's launch shape
// (64 KiB: /19 blocks, shift 5; 32 KiB: /18, shift 6); budget 0 = none.
#pragma once
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace pwaf {
namespace dirtable {

static constexpr uint32_t kChunkWords = 32;  // one 128-byte line per /16 (kernels.h: kDirChunkWords)
static constexpr size_t kEntries = (size_t)1 << 24;

struct Compressed {
    std::vector<uint32_t> chunks;   // 65536 x kChunkWords: 8 records of {start bitmap, carried-in entry, first run, index into vals}
    std::vector<uint32_t> vals;     // entries of the second and further runs of a group (never empty: uploads need a byte)
    std::vector<uint32_t> summary;  // one bit per block of 2^shift /24s: 1 = look the table up; empty = no summary
    uint32_t shift = 0, common = 0;  // (meaningful with a summary only: 0 otherwise, as the lookup kernel expects)
    std::vector<uint32_t> coarse;   // one bit per block of 2^coarse_shift /24s: 1 = look the summary up; empty = no coarse level
    uint32_t coarse_shift = 0;
};

static constexpr size_t kCoarseBudget = 64 * 1024;  // bytes of LDS the default launch shape of ipres_kernel gives the coarse bitmap
static constexpr uint32_t kMaxCoarseShift = 12;     // (4096 /24s per bit, a 512-byte bitmap: coarser than any table could use)

inline uint64_t popcount_words(const std::vector<uint32_t> &w) {
    uint64_t n = 0;
    for (uint32_t x : w) n += (uint64_t)__builtin_popcount(x);
    return n;
}

inline void compress(const uint32_t *d24, bool no_summary, Compressed &out, size_t coarse_budget = kCoarseBudget) {
    out.chunks.assign((size_t)65536 * kChunkWords, 0);
    out.vals.clear();
    out.summary.clear();
    out.coarse.clear();
    out.shift = out.common = out.coarse_shift = 0;
    for (uint32_t x = 0; x < 65536; x++) {
        const uint32_t *en = &d24[(size_t)x << 8];
        for (uint32_t w = 0; w < 8; w++) {
            uint32_t *rec = &out.chunks[(size_t)x * kChunkWords + 4 * w];
            uint32_t bm = 0, n_starts = 0;
            for (uint32_t j = 32 * w; j < 32 * w + 32; j++)
                if (j == 0 || en[j] != en[j - 1]) {
                    bm |= 1u << (j & 31);
                    if (n_starts == 1) rec[3] = (uint32_t)out.vals.size();
                    if (n_starts == 0) rec[2] = en[j];
                    else out.vals.push_back(en[j]);
                    n_starts++;
                }
            rec[0] = bm;
            rec[1] = w ? en[32 * w - 1] : 0u;  // (group 0 always starts a run at its first /24)
        }
    }
    if (out.vals.empty()) out.vals.push_back(0);
    if (no_summary) return;
    std::unordered_map<uint32_t, uint64_t> run_len;
    for (size_t x = 0; x < kEntries;) {
        size_t y = x + 1;
        while (y < kEntries && d24[y] == d24[x]) y++;
        run_len[d24[x]] += y - x;
        x = y;
    }
    uint32_t common = 0;
    uint64_t best_len = 0;
    for (const auto &kv : run_len)
        if (kv.second > best_len || (kv.second == best_len && kv.first < common)) { common = kv.first; best_len = kv.second; }
    double best_cost = 1e9;
    uint32_t best_shift = 0;
    std::vector<uint32_t> best_bits;
    for (uint32_t shift = 0; shift <= 4; shift++) {
        const size_t n_blk = kEntries >> shift;
        std::vector<uint32_t> bits(n_blk / 32, 0);
        uint64_t set = 0;
        for (size_t b = 0; b < n_blk; b++) {
            bool other = false;
            for (size_t j = b << shift; j < ((b + 1) << shift) && !other; j++) other = d24[j] != common;
            if (other) { bits[b >> 5] |= 1u << (b & 31); set++; }
        }
        const double cost = (double)set / (double)n_blk + (double)(n_blk / 8) / (8.0 * 1024 * 1024);
        if (cost < best_cost && set * 2 <= n_blk) { best_cost = cost; best_shift = shift; best_bits.swap(bits); }
    }
    if (!best_bits.empty()) {
        out.summary.swap(best_bits);
        out.shift = best_shift;
        out.common = common;
    }
    if (out.summary.empty()) return;
    // the coarse level: the smallest shift above the summary's whose bitmap fits the budget; a coarse bit is the OR of its summary bits
    for (uint32_t cs = out.shift + 1; cs <= kMaxCoarseShift; cs++) {
        const size_t n_blk = kEntries >> cs;
        if (n_blk / 8 > coarse_budget) continue;
        const uint32_t per = 1u << (cs - out.shift);  // summary bits per coarse bit: 2 ... 4096, all inside one or a run of whole words
        std::vector<uint32_t> bits(n_blk / 32, 0);
        uint64_t set = 0;
        for (size_t b = 0; b < n_blk; b++) {
            bool any = false;
            if (per >= 32) {
                for (size_t w = b * (per / 32); w < (b + 1) * (per / 32) && !any; w++) any = out.summary[w] != 0;
            } else {
                const size_t first = b * per;
                any = ((out.summary[first >> 5] >> (first & 31)) & ((1u << per) - 1u)) != 0;
            }
            if (any) { bits[b >> 5] |= 1u << (b & 31); set++; }
        }
        if (set * 2 <= n_blk) { out.coarse.swap(bits); out.coarse_shift = cs; }
        break;
    }
}

}  // namespace dirtable
}  // namespace pwaf
