// TEST-ONLY host build of the IPv4 lookup table (tests/test_addresses_cpu.py): the flattening dir24_kernel does on the device,
// restated; the run compression and summary choice of csrc/dirtable.h — the very header pwaf_engine_create calls; and a scalar
// restatement of ipres_kernel's lookup (summary bit -> 16-byte record -> rank -> carried / first / further run -> escape pair ->
// remaining trie levels with the byte index both tries share). Not part of the product.
//
// usage: dirtable_host IN OUT   (stats as one JSON line on stdout)
// IN (u32 words): 'DIRT', flags (1 = no summary, 2 = a flat table is given instead of tries, 4 = the program has a GeoIP table,
//   8 = write the per-/24 answers), n_ip_lists, geo_default, then eight sections {count, words...}: GR4, GR6, GNOD, IR4, IR6, INOD
//   (the trie sections of a program dump; an empty root = a family without prefixes), FLAT (2^24 entries or none), ADDR (5 words per
//   address: 16 address bytes, is_v6).
// OUT: with flag 8 two arrays of 2^24 words — the GeoIP and the list entry of every /24 as the lookup leaves phase 4 (leaf | value,
//   or a node to continue from; flat mode: the table entry, then zeros) — then two words per address: the final record and set.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../pingoo_amd/csrc/dirtable.h"

using namespace pwaf;

static constexpr uint32_t LEAF = 0x80000000u, ESCAPE = 0x80000000u;

struct Tables {
    std::vector<uint32_t> gr4, gr6, gnod, ir4, ir6, inod, flat, addr;
    uint32_t flags = 0, n_ip_lists = 0, geo_default = 0;
    bool has_geo() const { return flags & 4u; }
    // (the engine substitutes an all-leaf root for a family without prefixes: the default record / the empty set)
    uint32_t g4(uint32_t t) const { return gr4.empty() ? LEAF | geo_default : gr4[t]; }
    uint32_t g6(uint32_t t) const { return gr6.empty() ? LEAF | geo_default : gr6[t]; }
    uint32_t i4(uint32_t t) const { return ir4.empty() ? LEAF : ir4[t]; }
    uint32_t i6(uint32_t t) const { return ir6.empty() ? LEAF : ir6[t]; }
};

struct Lookup {
    const Tables &T;
    const dirtable::Compressed &C;
    const std::vector<uint32_t> &esc;  // pairs
    bool dir;
    uint64_t oob = 0;

    // phases 1b - 4 for the /24 `x` of an IPv4 address whose first byte is x >> 16
    void table(uint32_t x, uint32_t &eg, uint32_t &ei, uint32_t *raw = nullptr) {
        const uint32_t top16 = x >> 8, b2 = x & 0xFFu;
        uint32_t look = 1;
        if (!C.summary.empty()) {
            const uint32_t blk = x >> C.shift;
            look = (C.summary[blk >> 5] >> (blk & 31u)) & 1u;
        }
        uint32_t e24 = C.common;
        if (look) {
            const uint32_t *rec = &C.chunks[(size_t)top16 * dirtable::kChunkWords + 4u * (b2 >> 5)];
            const uint32_t rank = (uint32_t)__builtin_popcount(rec[0] & (0xFFFFFFFFu >> (31u - (b2 & 31u))));
            if (rank == 0) e24 = rec[1];
            else if (rank == 1) e24 = rec[2];
            else {
                const size_t at = (size_t)rec[3] + rank - 2u;
                if (at < C.vals.size()) e24 = C.vals[at];
                else { oob++; e24 = 0; }
            }
        }
        if (raw) *raw = e24;
        if ((e24 & ESCAPE) && !(T.flags & 2u)) {
            const size_t at = e24 & ~ESCAPE;
            if (2 * at + 1 < esc.size()) { eg = esc[2 * at]; ei = esc[2 * at + 1]; }
            else { oob++; eg = ei = LEAF; }
        } else {
            eg = LEAF | (e24 & 0xFFFFu);
            ei = LEAF | (e24 >> 16);
        }
        const uint32_t b0 = x >> 16;
        const bool geo_walk = T.has_geo() && !(b0 == 127u || (b0 & 0xF0u) == 0xE0u);
        if (!geo_walk) eg = LEAF | T.geo_default;
        if (T.n_ip_lists == 0) ei = LEAF;
    }

    void address(const uint8_t ip[16], bool v6, uint32_t &rec, uint32_t &set) {
        uint32_t eg = LEAF, ei = LEAF, k = 2;
        const uint32_t top16 = (uint32_t)ip[0] << 8 | ip[1];
        if (!v6 && dir) {
            table(top16 << 8 | ip[2], eg, ei);
            k = 3;
        } else {
            bool geo_walk = T.has_geo();
            if (geo_walk && !v6) geo_walk = !(ip[0] == 127u || (ip[0] & 0xF0u) == 0xE0u);
            if (geo_walk && v6) {
                bool loopback = ip[15] == 1;
                for (int j = 0; j < 15; j++) loopback = loopback && ip[j] == 0;
                geo_walk = !(loopback || ip[0] == 0xFFu);
            }
            eg = geo_walk ? (v6 ? T.g6(top16) : T.g4(top16)) : LEAF | T.geo_default;
            ei = T.n_ip_lists ? (v6 ? T.i6(top16) : T.i4(top16)) : LEAF;
        }
        // phase 5: both walks advance together, one byte index for the two tries
        while (!((eg & ei) & LEAF)) {
            const uint32_t byte = ip[k < 16 ? k : 15u];
            const uint32_t ng = (eg & LEAF) ? eg : T.gnod[(size_t)eg * 256 + byte];
            const uint32_t ni = (ei & LEAF) ? ei : T.inod[(size_t)ei * 256 + byte];
            k++;
            eg = ng;
            ei = ni;
        }
        rec = eg & ~LEAF;
        set = ei & ~LEAF;
    }
};

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: dirtable_host IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    Tables T;
    uint32_t head[4];
    if (fread(head, 4, 4, f) != 4 || head[0] != 0x54524944u) { fprintf(stderr, "bad input header\n"); return 2; }
    T.flags = head[1]; T.n_ip_lists = head[2]; T.geo_default = head[3];
    for (std::vector<uint32_t> *v : {&T.gr4, &T.gr6, &T.gnod, &T.ir4, &T.ir6, &T.inod, &T.flat, &T.addr}) {
        uint32_t n = 0;
        if (fread(&n, 4, 1, f) != 1) { fprintf(stderr, "short input\n"); return 2; }
        v->resize(n);
        if (n && fread(v->data(), 4, n, f) != n) { fprintf(stderr, "short input\n"); return 2; }
    }
    fclose(f);
    const bool flat_mode = T.flags & 2u;
    if (flat_mode && T.flat.size() != dirtable::kEntries) { fprintf(stderr, "flat table: 2^24 entries expected\n"); return 2; }
    const bool dir = flat_mode || (T.has_geo() && !T.gr4.empty()) || (T.n_ip_lists && !T.ir4.empty());

    // ---- dir24_kernel restated: first 24 bits of both IPv4 tries, packed when both are leaves with ids that fit ----
    std::vector<uint32_t> d24, esc;
    uint64_t esc_len_geo = 0, esc_len_list = 0, esc_len_both = 0, esc_id_class = 0, esc_id_set = 0;
    if (flat_mode) d24.swap(T.flat);
    else if (dir) {
        d24.resize(dirtable::kEntries);
        for (uint32_t x = 0; x < (1u << 24); x++) {
            uint32_t eg = T.g4(x >> 8);
            if (!(eg & LEAF)) eg = T.gnod[(size_t)eg * 256 + (x & 0xFFu)];
            uint32_t ei = T.i4(x >> 8);
            if (!(ei & LEAF)) ei = T.inod[(size_t)ei * 256 + (x & 0xFFu)];
            const uint32_t vg = eg & ~LEAF, vi = ei & ~LEAF;
            if ((eg & ei & LEAF) && vg < 65536u && vi < 32768u) { d24[x] = vg | (vi << 16); continue; }
            const bool lg = !(eg & LEAF), li = !(ei & LEAF);
            esc_len_geo += lg && !li; esc_len_list += li && !lg; esc_len_both += lg && li;
            esc_id_class += !lg && vg >= 65536u; esc_id_set += !li && vi >= 32768u;
            d24[x] = ESCAPE | (uint32_t)(esc.size() / 2);
            esc.push_back(eg);
            esc.push_back(ei);
        }
    }

    // ---- the shared compression ----
    dirtable::Compressed C;
    uint64_t starts_hist[33] = {0}, cross_hist[8] = {0}, bit0 = 0, bit31 = 0, across16 = 0, summary_set = 0;
    if (dir) {
        dirtable::compress(d24.data(), T.flags & 1u, C);
        for (size_t g = 0; g < (size_t)65536 * 8; g++) {
            const uint32_t bm = C.chunks[4 * g];
            starts_hist[__builtin_popcount(bm)]++;
            if (g % 8) { bit0 += bm & 1u; }
            bit31 += bm >> 31;
        }
        // runs of a /16 by the number of group boundaries they cross; /16 boundaries that a non-zero entry continues across
        for (uint32_t x = 0; x < 65536; x++) {
            const uint32_t *en = &d24[(size_t)x << 8];
            for (uint32_t j = 0; j < 256;) {
                uint32_t e = j + 1;
                while (e < 256 && en[e] == en[j]) e++;
                cross_hist[((e - 1) >> 5) - (j >> 5)]++;
                j = e;
            }
            if (x && en[0] && en[0] == en[-1]) across16++;
        }
        for (uint32_t w : C.summary) summary_set += (uint64_t)__builtin_popcount(w);
    }

    // ---- lookups ----
    Lookup L{T, C, esc, dir};
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    if ((T.flags & 8u) && dir) {
        std::vector<uint32_t> og(dirtable::kEntries), oi(dirtable::kEntries);
        for (uint32_t x = 0; x < (1u << 24); x++) {
            uint32_t raw = 0;
            L.table(x, og[x], oi[x], &raw);
            if (flat_mode) { og[x] = raw; oi[x] = 0; }
        }
        fwrite(og.data(), 4, og.size(), o);
        fwrite(oi.data(), 4, oi.size(), o);
    }
    const size_t n_addr = T.addr.size() / 5;
    std::vector<uint32_t> res(2 * n_addr);
    for (size_t a = 0; a < n_addr && !flat_mode; a++)
        L.address(reinterpret_cast<const uint8_t *>(&T.addr[5 * a]), T.addr[5 * a + 4] != 0, res[2 * a], res[2 * a + 1]);
    fwrite(res.data(), 4, res.size(), o);
    fclose(o);

    std::string s = "{\"dir\": " + std::to_string(dir ? 1 : 0) + ", \"starts_hist\": [";
    for (int k = 0; k < 33; k++) s += (k ? ", " : "") + std::to_string(starts_hist[k]);
    s += "], \"cross_hist\": [";
    for (int k = 0; k < 8; k++) s += (k ? ", " : "") + std::to_string(cross_hist[k]);
    s += "]";
    auto kv = [&](const char *name, uint64_t v) { s += std::string(", \"") + name + "\": " + std::to_string(v); };
    kv("n_vals", C.vals.size()); kv("has_summary", C.summary.empty() ? 0 : 1); kv("shift", C.shift); kv("common", C.common);
    kv("summary_set", summary_set); kv("escapes", esc.size() / 2); kv("esc_len_geo", esc_len_geo); kv("esc_len_list", esc_len_list);
    kv("esc_len_both", esc_len_both); kv("esc_id_class", esc_id_class); kv("esc_id_set", esc_id_set);
    kv("starts_at_bit0", bit0); kv("starts_at_bit31", bit31); kv("runs_across_16", across16); kv("out_of_range", L.oob);
    puts((s + "}").c_str());
    return 0;
}
