// TEST-ONLY host build of the coarse level of the IPv4 lookup table (tests/test_addresses_coarse_cpu.py): dirtable::compress of
// csrc/dirtable.h — the very header pwaf_engine_create calls — over a flat table, the exhaustive check of the coarse bitmap against
// it, and a scalar restatement of ipres_kernel<.., COARSE>'s three-level lookup (coarse bit -> summary bit -> 16-byte record -> run)
// that says at which level every lookup ends. Not part of the product.
//
// usage: dirtable_coarse_host IN OUT   (stats as one JSON line on stdout)
// IN (u32 words): 'DIRC', flags (1 = no summary, 2 = call compress() without a budget argument), budget in bytes, number of queries,
//   2^24 table entries, the queried /24s.
// OUT: the coarse bitmap's words, then two words per query: the entry the lookup returns and the level it ended at (0 = coarse bit
//   clear, 1 = summary bit clear, 2 = the table).
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../pingoo_amd/csrc/dirtable.h"

using namespace pwaf;

static uint32_t lookup(const dirtable::Compressed &C, uint32_t x, uint32_t &level, uint64_t &oob) {
    level = 0;
    if (!C.coarse.empty()) {
        const uint32_t blk = x >> C.coarse_shift;
        if (!((C.coarse[blk >> 5] >> (blk & 31u)) & 1u)) return C.common;
    }
    level = 1;
    if (!C.summary.empty()) {
        const uint32_t blk = x >> C.shift;
        if (!((C.summary[blk >> 5] >> (blk & 31u)) & 1u)) return C.common;
    }
    level = 2;
    const uint32_t b2 = x & 0xFFu;
    const uint32_t *rec = &C.chunks[(size_t)(x >> 8) * dirtable::kChunkWords + 4u * (b2 >> 5)];
    const uint32_t rank = (uint32_t)__builtin_popcount(rec[0] & (0xFFFFFFFFu >> (31u - (b2 & 31u))));
    if (rank == 0) return rec[1];
    if (rank == 1) return rec[2];
    const size_t at = (size_t)rec[3] + rank - 2u;
    if (at < C.vals.size()) return C.vals[at];
    oob++;
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: dirtable_coarse_host IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t head[4];
    if (fread(head, 4, 4, f) != 4 || head[0] != 0x43524944u) { fprintf(stderr, "bad input header\n"); return 2; }
    std::vector<uint32_t> d24(dirtable::kEntries), q(head[3]);
    if (fread(d24.data(), 4, d24.size(), f) != d24.size() || (q.size() && fread(q.data(), 4, q.size(), f) != q.size())) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);
    dirtable::Compressed C;
    if (head[1] & 2u) dirtable::compress(d24.data(), head[1] & 1u, C);
    else dirtable::compress(d24.data(), head[1] & 1u, C, head[2]);

    // exhaustively: a coarse bit is 0 exactly when every /24 of its block holds the common entry (one pass over the table)
    uint64_t bit_mismatch = 0, coarse_set = 0, summary_set = 0;
    if (!C.coarse.empty()) {
        const size_t n_blk = dirtable::kEntries >> C.coarse_shift;
        if (C.coarse.size() != n_blk / 32) bit_mismatch = n_blk;
        else
            for (size_t b = 0; b < n_blk; b++) {
                bool other = false;
                for (size_t j = b << C.coarse_shift; j < ((b + 1) << C.coarse_shift); j++) other = other || d24[j] != C.common;
                const bool bit = (C.coarse[b >> 5] >> (b & 31)) & 1u;
                bit_mismatch += bit != other;
                coarse_set += bit;
            }
    }
    for (uint32_t w : C.summary) summary_set += (uint64_t)__builtin_popcount(w);
    // every /24 through the three levels
    uint64_t ends[3] = {0, 0, 0}, lookup_mismatch = 0, oob = 0;
    for (uint32_t x = 0; x < (1u << 24); x++) {
        uint32_t level;
        lookup_mismatch += lookup(C, x, level, oob) != d24[x];
        ends[level]++;
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    if (!C.coarse.empty()) fwrite(C.coarse.data(), 4, C.coarse.size(), o);
    for (uint32_t x : q) {
        uint32_t r[2];
        r[0] = lookup(C, x & 0xFFFFFFu, r[1], oob);
        fwrite(r, 4, 2, o);
    }
    fclose(o);
    std::string s = "{";
    auto kv = [&](const char *name, uint64_t v) { s += std::string(s.size() > 1 ? ", \"" : "\"") + name + "\": " + std::to_string(v); };
    kv("has_summary", C.summary.empty() ? 0 : 1); kv("shift", C.shift); kv("common", C.common); kv("summary_set", summary_set);
    kv("has_coarse", C.coarse.empty() ? 0 : 1); kv("coarse_shift", C.coarse_shift); kv("coarse_bytes", C.coarse.size() * 4); kv("coarse_set", coarse_set);
    kv("bit_mismatch", bit_mismatch); kv("lookup_mismatch", lookup_mismatch); kv("out_of_range", oob);
    kv("ends_coarse", ends[0]); kv("ends_summary", ends[1]); kv("ends_table", ends[2]);
    puts((s + "}").c_str());
    return 0;
}
