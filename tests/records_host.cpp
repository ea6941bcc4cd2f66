// TEST-ONLY: csrc/records.h (the record layout the engine validates and unpack_records_kernel decodes) compiled with g++ for the CPU suite
// (tests/test_records_cpu.py). `records_host <buf> <rec_off> <n_cols> <out>`: validates the call exactly as pwaf_evaluate_records does; on
// success writes the struct-of-arrays columns the records decode to (per column: n + 1 offsets, then the bytes; then ip, v6, port, flags,
// asn, country) and prints {"ok": true, "has_geoip": ..}; otherwise prints {"ok": false, "index": i, "check": code}.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pingoo_amd/csrc/records.h"

namespace R = pwaf::records;

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) exit(3);
    uint8_t tmp[1 << 16];
    size_t k;
    while ((k = fread(tmp, 1, sizeof tmp, f)) > 0) v.insert(v.end(), tmp, tmp + k);
    fclose(f);
    return v;
}

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const std::vector<uint8_t> buf = slurp(argv[1]), offb = slurp(argv[2]);
    const uint32_t n = (uint32_t)(offb.size() / 4), n_cols = (uint32_t)atoi(argv[3]);
    std::vector<uint32_t> rec_off(n);
    if (n) memcpy(rec_off.data(), offb.data(), (size_t)n * 4);
    // (an exact-size copy: a read past the buffer would be a read past the heap block, which a sanitizer build catches)
    std::vector<uint64_t> totals(n_cols);
    uint32_t bad = 0;
    int geo = 0;
    uint64_t lo = 0, hi = 0;
    const int c = R::validate(buf.data(), buf.size(), rec_off.data(), n, n_cols, totals.data(), &bad, &geo, &lo, &hi);
    if (c != R::kOk) {
        printf("{\"ok\": false, \"index\": %u, \"check\": %d, \"message\": \"%s\"}\n", bad, c, R::check_message(c));
        return 0;
    }
    const size_t stride = (size_t)n + 1;
    std::vector<uint32_t> off(stride * n_cols);
    R::column_offsets(buf.data(), rec_off.data(), n, n_cols, off.data(), stride);
    FILE *o = fopen(argv[4], "wb");
    if (!o) return 3;
    for (uint32_t f = 0; f < n_cols; f++) {
        if (off[f * stride + n] != totals[f]) return 4;
        fwrite(&off[f * stride], 4, stride, o);
        // the device's decode: value f of record i is the bytes behind its lengths, at the prefix of the lengths before it
        std::vector<uint8_t> col(totals[f]);
        for (uint32_t i = 0; i < n; i++) {
            const uint8_t *r = buf.data() + rec_off[i];
            pwaf_record_head h;
            R::load_head(r, &h);
            if (f >= h.n_values) continue;
            uint32_t at = R::values_offset(h.n_values);
            for (uint32_t k = 0; k < f; k++) at += R::load_len(r, k);
            const uint32_t len = R::load_len(r, f);
            if (len) memcpy(col.data() + off[f * stride + i], r + at, len);
        }
        if (!col.empty()) fwrite(col.data(), 1, col.size(), o);
    }
    std::vector<uint8_t> ip((size_t)n * 16), v6(n), flags(n);
    std::vector<uint16_t> port(n), country(n);
    std::vector<uint32_t> asn(n);
    for (uint32_t i = 0; i < n; i++) {
        pwaf_record_head h;
        R::load_head(buf.data() + rec_off[i], &h);
        memcpy(&ip[(size_t)i * 16], h.ip, 16);
        v6[i] = h.ip_is_v6;
        flags[i] = h.flags;
        port[i] = h.port;
        asn[i] = h.asn;
        country[i] = (uint16_t)(h.country[0] | (h.country[1] << 8));
    }
    fwrite(ip.data(), 1, ip.size(), o);
    fwrite(v6.data(), 1, n, o);
    fwrite(port.data(), 2, n, o);
    fwrite(flags.data(), 1, n, o);
    fwrite(asn.data(), 4, n, o);
    fwrite(country.data(), 2, n, o);
    fclose(o);
    printf("{\"ok\": true, \"has_geoip\": %d, \"span\": [%llu, %llu]}\n", geo, (unsigned long long)lo, (unsigned long long)hi);
    return 0;
}
