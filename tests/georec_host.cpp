// TEST-ONLY host build of the GeoIP ANSWER tables (tests/test_geo_answers_cpu.py): reads the record-leaf GeoIP trie and the records
// out of a program dump (pwaf_program_dump: sections HEAD, GR4, GR6, GNOD, GREC), runs the flattening of csrc/georec.h and the run
// compression / summary choice of csrc/dirtable.h — the very headers pwaf_engine_create calls — and answers with the scalar restatement
// of georec_kernel's lookup (csrc/georec.h). Not part of the product.
//
// usage: georec_host DUMP ADDR OUT FLAGS   (stats as one JSON line on stdout)
// FLAGS: 1 = no summary (PWAF_OPT_NO_DIR_SUMMARY), 8 = write the per-/24 answers.
// ADDR: 20 bytes per address (16 address bytes, IPv4 in bytes 0..3; is_v6 as a 32-bit word).
// OUT: with flag 8 and an IPv4 table 2^24 words — per /24 the record id the whole lookup gives its first address, or
//   0x80000000 | trie node when the /24's table entry escapes — then per address 12 bytes: the record id and the record {asn, country, 0} (pwaf_geo).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../pingoo_amd/csrc/georec.h"

using namespace pwaf;

struct Rec { uint32_t asn; uint16_t country, pad; };

static std::vector<uint8_t> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    std::vector<uint8_t> b;
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + k);
    fclose(f);
    return b;
}

int main(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "usage: georec_host DUMP ADDR OUT FLAGS\n"); return 2; }
    const std::vector<uint8_t> dump = slurp(argv[1]), addr = slurp(argv[2]);
    const uint32_t flags = (uint32_t)atoi(argv[4]);
    if (dump.size() < 8 || memcmp(dump.data(), "PWAFPRG1", 8) != 0) { fprintf(stderr, "bad dump magic\n"); return 2; }
    std::vector<uint32_t> gr4, gr6, gnod;
    std::vector<Rec> recs;
    uint32_t has_geo = 0;
    for (size_t pos = 8; pos + 16 <= dump.size();) {
        uint64_t len;
        memcpy(&len, &dump[pos + 8], 8);
        const uint8_t *pl = &dump[pos + 16];
        if (pos + 16 + len > dump.size()) { fprintf(stderr, "truncated dump\n"); return 2; }
        auto words = [&](std::vector<uint32_t> &v) { v.resize(len / 4); if (len) memcpy(v.data(), pl, len / 4 * 4); };
        if (!memcmp(&dump[pos], "HEAD", 4) && len >= 32) memcpy(&has_geo, pl + 24, 4);
        else if (!memcmp(&dump[pos], "GR4 ", 4)) words(gr4);
        else if (!memcmp(&dump[pos], "GR6 ", 4)) words(gr6);
        else if (!memcmp(&dump[pos], "GNOD", 4)) words(gnod);
        else if (!memcmp(&dump[pos], "GREC", 4)) { recs.resize(len / sizeof(Rec)); if (len) memcpy(recs.data(), pl, recs.size() * sizeof(Rec)); }
        pos = (pos + 16 + len + 7) / 8 * 8;
    }
    if (recs.empty()) recs.push_back(Rec{0u, (uint16_t)('X' | ('X' << 8)), 0u});  // (what the engine uploads for a program without a table)
    if ((!gr4.empty() && gr4.size() != 65536) || (!gr6.empty() && gr6.size() != 65536) || gnod.size() % 256) { fprintf(stderr, "bad trie sections\n"); return 2; }

    // ---- what pwaf_engine_create does with PWAF_OPT_GEO_ANSWERS ----
    georec::View V;
    V.has_geo = has_geo != 0;
    V.root4 = gr4.empty() ? nullptr : gr4.data();
    V.root6 = gr6.empty() ? nullptr : gr6.data();
    V.nodes = gnod.data();
    V.n_nodes = gnod.size() / 256;
    dirtable::Compressed C;
    uint32_t n_esc = 0;
    const bool dir = V.has_geo && !gr4.empty();
    if (dir) {
        std::vector<uint32_t> d24;
        n_esc = georec::flatten(gr4.data(), gnod.data(), d24);
        dirtable::compress(d24.data(), (flags & 1u) != 0, C);
        V.dir = &C;
    }

    FILE *o = fopen(argv[3], "wb");
    if (!o) { perror(argv[3]); return 2; }
    uint64_t bad_ids = 0;
    if ((flags & 8u) && dir) {
        std::vector<uint32_t> per24(dirtable::kEntries);
        for (uint32_t x = 0; x < (1u << 24); x++) {
            const uint32_t t = georec::table_entry(V, x);
            const uint8_t ip[16] = {(uint8_t)(x >> 16), (uint8_t)(x >> 8), (uint8_t)x, 0};
            per24[x] = (t & georec::kEscape) ? t : georec::lookup(V, ip, false);
        }
        fwrite(per24.data(), 4, per24.size(), o);
    }
    const size_t n_addr = addr.size() / 20;
    std::vector<uint32_t> res(3 * n_addr);
    for (size_t a = 0; a < n_addr; a++) {
        uint32_t v6;
        memcpy(&v6, &addr[20 * a + 16], 4);
        uint32_t id = georec::lookup(V, &addr[20 * a], v6 != 0);
        if (id >= recs.size()) { bad_ids++; id = 0; }
        res[3 * a] = id;
        res[3 * a + 1] = recs[id].asn;
        res[3 * a + 2] = recs[id].country;  // (reserved = 0)
    }
    fwrite(res.data(), 4, res.size(), o);
    fclose(o);
    std::string s = "{";
    auto kv = [&](const char *name, uint64_t v) { s += std::string(s.size() > 1 ? ", \"" : "\"") + name + "\": " + std::to_string(v); };
    kv("dir", dir ? 1 : 0); kv("escapes", n_esc); kv("n_vals", dir ? C.vals.size() : 0); kv("has_summary", C.summary.empty() ? 0 : 1); kv("shift", C.shift);
    kv("common", C.common); kv("records", recs.size()); kv("out_of_range", V.out_of_range + bad_ids);
    puts((s + "}").c_str());
    return 0;
}
