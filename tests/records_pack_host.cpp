// records_pack_host.cpp — the packing half of csrc/records.h (export_shape, pack_record, export_host: the HOST mode of pwaf_export_records)
// as a stand-alone program for the sanitizers: tests/test_export_records_cpu.py builds it with g++ -fsanitize=address,undefined and runs it.
//
//   records_pack_host <seed> <rounds>
//
// Every round builds a random batch in heap blocks of EXACTLY the bytes it owns (arenas without slack, offsets that begin above 0 like a
// slab view's, some header descriptors NULL, with or without GeoIP), a random list with duplicates and out-of-range indices, and exports it
// three times: as a size query, into a buffer of exactly bytes_needed bytes, and into one 16 to 4096 bytes short. A read outside a column
// or a write outside the buffer is the sanitizer's to report; the program itself checks every record with the header's own check_record,
// decodes it against the columns and checks the statistics, the prefix rule and PWAF_RECORD_NONE. Prints one JSON line; exit status 0 = ok.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../pingoo_amd/csrc/records.h"

namespace R = pwaf::records;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::printf("{\"ok\": false, \"line\": %d, \"round\": %u}\n", __LINE__, g_round); \
            return false;                                                           \
        }                                                                           \
    } while (0)

static unsigned g_round = 0;

struct Column {
    std::unique_ptr<uint8_t[]> data;      // exactly `bytes` bytes
    std::unique_ptr<uint32_t[]> offsets;  // n + 1
    uint32_t begin = 0;
};

static bool one_round(std::mt19937 &rng) {
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
    const uint32_t n = pick(0, 3) == 0 ? pick(0, 2) : pick(1, 90);
    const uint32_t n_hdr = std::vector<uint32_t>{0, 0, 1, 3, 59, 64, 120}[pick(0, 6)];
    const uint32_t n_cols = PWAF_N_FIELDS + n_hdr;
    const bool geo = pick(0, 1);
    std::vector<Column> cols(n_cols);
    R::PackArgs a{};
    for (uint32_t k = 0; k < n_cols; k++) {
        if (k >= PWAF_N_FIELDS && pick(0, 4) == 0) continue;  // a NULL descriptor: ""
        Column &c = cols[k];
        c.begin = pick(0, 2) ? pick(1, 1000) : 0;
        c.offsets.reset(new uint32_t[n + 1]);
        c.offsets[0] = c.begin;
        const uint32_t kind = pick(0, 3);  // 0: all empty, 1: sparse, 2: short values, 3: some long ones
        for (uint32_t i = 0; i < n; i++) {
            uint32_t len = 0;
            if (kind == 1) len = pick(0, 9) ? 0 : pick(1, 40);
            if (kind == 2) len = pick(0, 33);
            if (kind == 3) len = pick(0, 19) ? pick(0, 18) : pick(1, 70000);
            c.offsets[i + 1] = c.offsets[i] + len;
        }
        const uint32_t end = c.offsets[n];
        c.data.reset(new uint8_t[end ? end : 1]);  // bytes below `begin` belong to the arena but to no request of the slab
        uint32_t x = rng();
        for (uint32_t b = 0; b < end; b++) c.data[b] = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
        a.col[k].data = c.data.get();
        a.col[k].offsets = c.offsets.get();
    }
    std::unique_ptr<uint8_t[]> ip(new uint8_t[16 * n + 1]), v6(new uint8_t[n + 1]), flags(new uint8_t[n + 1]);
    std::unique_ptr<uint16_t[]> port(new uint16_t[n + 1]), country(new uint16_t[n + 1]);
    std::unique_ptr<uint32_t[]> asn(new uint32_t[n + 1]);
    for (uint32_t i = 0; i < n; i++) {
        for (int b = 0; b < 16; b++) ip[16 * i + b] = (uint8_t)rng();
        v6[i] = (uint8_t)pick(0, 1), flags[i] = (uint8_t)pick(0, 1), port[i] = (uint16_t)rng(), asn[i] = rng();
        const uint8_t cc[2] = {(uint8_t)('A' + pick(0, 25)), (uint8_t)('A' + pick(0, 25))};
        memcpy(&country[i], cc, 2);
    }
    a.n = n, a.n_cols = n_cols;
    a.ip = ip.get(), a.ip_is_v6 = v6.get(), a.flags = flags.get(), a.port = port.get();
    a.asn = geo ? asn.get() : nullptr, a.country = geo ? country.get() : nullptr;
    const uint32_t idx_cap = std::vector<uint32_t>{0, 1, 63, 64, 65, 200}[pick(0, 5)];
    std::unique_ptr<uint32_t[]> idx(new uint32_t[idx_cap ? idx_cap : 1]), rec_off(new uint32_t[idx_cap ? idx_cap : 1]);
    for (uint32_t j = 0; j < idx_cap; j++) {
        const uint32_t r = pick(0, 11);
        idx[j] = r == 0 ? n : r == 1 ? n + 1 : r == 2 ? 0xFFFFFFFFu : n ? pick(0, n - 1) : 0xFFFFFFFEu;
    }
    uint32_t n_idx = pick(0, idx_cap + 2);
    const bool with_n = pick(0, 1);
    const uint32_t m = with_n ? (n_idx < idx_cap ? n_idx : idx_cap) : idx_cap;
    a.idx = idx.get(), a.n_idx = with_n ? &n_idx : nullptr, a.idx_cap = idx_cap, a.rec_off = rec_off.get();

    // what the list asks for
    uint64_t want = 0;
    uint32_t n_valid = 0;
    for (uint32_t j = 0; j < m; j++)
        if (idx[j] < n) want += R::export_shape(a, idx[j]).size(), n_valid++;
    pwaf_export_stats q{}, st{};
    uint32_t bad = 0;
    a.stats = &q, a.buf = nullptr, a.buf_cap = 0;
    CHECK(R::export_host(a, &bad));
    CHECK(q.bytes_needed == want && q.n_selected == m && q.n_written == 0);
    for (int pass = 0; pass < 2; pass++) {
        uint64_t cap = want;
        if (pass == 1) {
            if (want < 16) break;
            const uint64_t cut = 16ull * pick(1, 256);
            cap = want - (cut < want ? cut : want);
        }
        std::unique_ptr<uint8_t[]> buf(new uint8_t[cap ? cap : 1]);  // (operator new: 16-byte aligned) exactly cap bytes: one more is the sanitizer's
        memset(buf.get(), 0xA5, cap ? cap : 1);
        for (uint32_t j = 0; j < idx_cap; j++) rec_off[j] = 0x5A5A5A5Au;
        a.stats = &st, a.buf = buf.get(), a.buf_cap = cap;
        CHECK(R::export_host(a, &bad));
        CHECK(st.bytes_needed == want && st.n_selected == m);
        uint64_t used = 0;
        uint32_t written = 0;
        for (uint32_t j = 0; j < idx_cap; j++) {
            if (j >= m) {
                CHECK(rec_off[j] == 0x5A5A5A5Au);  // entries past the list are not written
                continue;
            }
            if (idx[j] >= n) {
                CHECK(rec_off[j] == PWAF_RECORD_NONE);
                continue;
            }
            if (rec_off[j] == PWAF_RECORD_NONE) {
                CHECK(pass == 1);
                continue;
            }
            uint64_t vb = 0;
            CHECK(R::check_record(buf.get(), cap, rec_off[j], n_cols, &vb) == R::kOk);
            const uint8_t *r = buf.get() + rec_off[j];
            pwaf_record_head h;
            R::load_head(r, &h);
            const uint32_t i = idx[j];
            const R::ExportShape s = R::export_shape(a, i);
            CHECK(h.size == s.size() && h.n_values == s.n_values && vb == s.value_bytes);
            CHECK(h.port == port[i] && !memcmp(h.ip, &ip[16 * i], 16) && h.flags == flags[i] && h.ip_is_v6 == v6[i] && h.has_geoip == (geo ? 1 : 0));
            CHECK(h.asn == (geo ? asn[i] : 0u) && !memcmp(h.country, geo ? (const void *)&country[i] : (const void *)"\0\0", 2));
            CHECK(h.reserved[0] == 0 && h.reserved[1] == 0 && h.reserved[2] == 0);
            const uint32_t vo = R::values_offset(h.n_values);
            for (uint32_t b = R::kHead + 4u * h.n_values; b < vo; b++) CHECK(r[b] == 0);
            uint32_t at = vo;
            for (uint32_t k = 0; k < n_cols; k++) {
                const uint32_t len = R::col_len(a.col[k], i);
                CHECK(k < h.n_values ? R::load_len(r, k) == len : len == 0);
                if (len) CHECK(!memcmp(r + at, a.col[k].data + a.col[k].offsets[i], len));
                at += len;
            }
            for (; at < h.size; at++) CHECK(r[at] == 0);
            used += h.size;
            written++;
        }
        CHECK(written == st.n_written && (pass == 1 || written == n_valid));
        // the written records are a prefix of buf without holes: their sizes add up to the end of the last one
        uint64_t top = 0;
        for (uint32_t j = 0; j < m; j++)
            if (rec_off[j] != PWAF_RECORD_NONE) {
                pwaf_record_head h;
                R::load_head(buf.get() + rec_off[j], &h);
                if (rec_off[j] + (uint64_t)h.size > top) top = rec_off[j] + (uint64_t)h.size;
            }
        CHECK(top == used && used <= cap);
        for (uint64_t b = used; b < cap; b++) CHECK(buf[b] == 0xA5);
        if (pass == 1 && n_valid) CHECK(written < n_valid || want == 0);
    }
    // offsets that decrease for a selected request refuse the call and write nothing
    if (m && n >= 1) {
        uint32_t j = 0;
        while (j < m && idx[j] >= n) j++;
        if (j < m) {
            const uint32_t i = idx[j], k = pick(0, PWAF_N_FIELDS - 1);
            const uint32_t keep = cols[k].offsets[i + 1];
            cols[k].offsets[i + 1] = cols[k].offsets[i] - 1u;
            if (cols[k].offsets[i] != 0) {
                pwaf_export_stats untouched;
                memset(&untouched, 0x77, sizeof untouched);
                a.stats = &untouched, a.buf = nullptr, a.buf_cap = 0;
                CHECK(!R::export_host(a, &bad) && bad == j);
                CHECK(untouched.n_selected == 0x77777777u);
            }
            cols[k].offsets[i + 1] = keep;
        }
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: records_pack_host <seed> <rounds>\n");
        return 2;
    }
    std::mt19937 rng((uint32_t)std::strtoul(argv[1], nullptr, 10));
    const unsigned rounds = (unsigned)std::strtoul(argv[2], nullptr, 10);
    for (g_round = 0; g_round < rounds; g_round++)
        if (!one_round(rng)) return 1;
    std::printf("{\"ok\": true, \"rounds\": %u}\n", rounds);
    return 0;
}
