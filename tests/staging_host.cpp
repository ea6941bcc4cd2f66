// staging_host.cpp — the staging layouts and host-column checks of csrc/staging.h (what pwaf_evaluate_batch and pwaf_evaluate_records*
// compute before they copy anything) as a stand-alone program: tests/test_staging_cpu.py builds it with g++, a second time with
// -fsanitize=address,undefined, and runs both. Links no HIP. Not part of the product.
//
//   staging_host invariants <seed> <cases>   random plans of all four kinds: parts aligned, disjoint, large enough; need = the end
//   staging_host record_cols <seed> <cases>  plan_record_cols / fill_unpack_args against the host path's old take loop, restated below
//   staging_host packed_edges                plan_packed around kPackMax and at a slab view, with and without asn / geo / route
//   staging_host host_columns                check_column_ends / check_host_columns: codes and texts
//
// The first two print one JSON line {"cases", "failures", "first"}; the last two one JSON line per case, for the test to compare.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../pingoo_amd/csrc/staging.h"

using namespace pwaf;

static std::string g_message;
namespace pwaf {
int fail(int code, const std::string &msg) {  // (the product's is program_api.cpp's)
    g_message = msg;
    return code;
}
}  // namespace pwaf

static size_t up256(size_t x) { return (x + 255) / 256 * 256; }

struct Part {
    const char *name;
    size_t at, bytes;  // where the plan puts it, and its payload
};
// every part on a 256-byte boundary and at least its payload, no two overlapping, `end` = the end of the last one (rounded like the rest)
static std::string check_parts(std::vector<Part> parts, size_t end) {
    std::stable_sort(parts.begin(), parts.end(), [](const Part &a, const Part &b) { return a.at < b.at; });
    for (size_t k = 0; k < parts.size(); k++) {
        const Part &p = parts[k];
        if (p.at % 256) return std::string(p.name) + " is not 256-byte aligned";
        const size_t next = k + 1 < parts.size() ? parts[k + 1].at : end;
        if (p.at + p.bytes > next) return std::string(p.name) + " overlaps what follows it";
    }
    if (!parts.empty() && end != up256(parts.back().at + parts.back().bytes)) return "the size is not the end of the last part";
    return "";
}

static const uint32_t kNs[] = {1, 2, 63, 64, 65};
struct Rng {
    std::mt19937_64 g;
    explicit Rng(uint64_t seed) : g(seed) {}
    uint64_t below(uint64_t k) { return g() % k; }
    bool coin() { return g() & 1; }
    uint32_t n() { return below(4) ? kNs[below(5)] : 1 + (uint32_t)below(5000); }
    uint32_t n_fields() { return PWAF_N_FIELDS + (uint32_t)below(65); }  // 0 .. 64 header columns
};

static std::vector<Part> packed_parts(const PackedPlan &p, uint32_t n, uint32_t n_fields, const HostCol *col, bool asn, bool geo, bool route, bool with_columns) {
    std::vector<Part> parts;
    static char names[2 * kMaxCols][16];
    for (uint32_t f = 0; f < n_fields && with_columns; f++) {
        if (!col[f].present) continue;
        snprintf(names[2 * f], 16, "off[%u]", f);
        snprintf(names[2 * f + 1], 16, "data[%u]", f);
        parts.push_back({names[2 * f], p.at_off[f], (size_t)(n + 1) * 4});
        parts.push_back({names[2 * f + 1], p.at_data[f], (size_t)col[f].last + PWAF_ARENA_PAD});
    }
    parts.push_back({"ip", p.at_ip, (size_t)n * 16});
    parts.push_back({"v6", p.at_v6, n});
    parts.push_back({"port", p.at_port, (size_t)n * 2});
    parts.push_back({"flags", p.at_flags, n});
    if (asn) parts.push_back({"asn", p.at_asn, (size_t)n * 4});
    if (asn) parts.push_back({"country", p.at_cc, (size_t)n * 2});
    parts.push_back({"counts", p.at_counts, sizeof(pwaf_counts)});
    parts.push_back({"out", p.at_out, (size_t)n * sizeof(pwaf_verdict)});
    if (geo) parts.push_back({"geo", p.at_geo, (size_t)n * sizeof(pwaf_geo)});
    if (route) parts.push_back({"route", p.at_route, (size_t)n * 4});
    return parts;
}

static int invariants(uint64_t seed, uint32_t cases) {
    Rng r(seed);
    uint32_t failures = 0, packable = 0;
    std::string first;
    const auto note = [&](const char *what, const std::string &why) {
        if (why.empty()) return;
        if (!failures++) first = std::string(what) + ": " + why;
    };
    for (uint32_t c = 0; c < cases; c++) {
        const uint32_t n = r.n(), n_fields = r.n_fields();
        // -- a host batch's packed block
        HostCol col[kMaxCols];
        const uint64_t scale = r.below(3) == 0 ? 200000 : 3000;  // (most batches fit the block, some do not)
        for (uint32_t f = 0; f < n_fields; f++) {
            col[f].present = f < PWAF_N_FIELDS || r.below(4) != 0;  // (absent headers)
            col[f].first = r.below(50) == 0 ? 1 + (uint32_t)r.below(1000) : 0;
            col[f].last = col[f].first + (uint32_t)r.below(scale);
        }
        const bool asn = r.coin(), geo = r.coin(), route = r.coin();
        const PackedPlan p = plan_packed(n, n_fields, col, asn, geo, route);
        packable += p.packable;
        // (a batch that is not packable stopped placing its columns somewhere: the fixed parts are still laid out one after the other)
        note("plan_packed", check_parts(packed_parts(p, n, n_fields, col, asn, geo, route, p.packable), p.need));
        if (p.in_bytes > p.at_out) note("plan_packed", "in_bytes lies behind the verdicts");
        if (p.in_bytes != p.at_counts + up256(sizeof(pwaf_counts))) note("plan_packed", "in_bytes is not the end of the counters");
        if (p.packable && p.need > kPackMax) note("plan_packed", "a packable plan larger than kPackMax");
        // -- the unpacked record batch
        uint64_t totals[kMaxCols];
        std::vector<Part> parts;
        static char names[kMaxCols][16];
        for (uint32_t f = 0; f < n_fields; f++) totals[f] = r.below(20) == 0 ? 0xFFFFFFF0ull - r.below(600) : r.below(5000);
        const bool rgeo = r.coin();
        const RecordColsPlan rc = plan_record_cols(totals, n_fields, n, rgeo);
        for (uint32_t f = 0; f < n_fields; f++) {
            snprintf(names[f], 16, "column %u", f);
            parts.push_back({names[f], (size_t)rc.col_at[f], (size_t)totals[f] + PWAF_ARENA_PAD});
        }
        parts.push_back({"ip", rc.c_ip, (size_t)n * 16});
        parts.push_back({"v6", rc.c_v6, n});
        parts.push_back({"port", rc.c_port, (size_t)n * 2});
        parts.push_back({"flags", rc.c_flags, n});
        if (rgeo) parts.push_back({"asn", rc.c_asn, (size_t)n * 4});
        if (rgeo) parts.push_back({"country", rc.c_cc, (size_t)n * 2});
        note("plan_record_cols", check_parts(parts, rc.size));
        // -- rec_meta of host records
        const size_t span = 16 * (1 + (size_t)r.below(100000));
        const HostRecMeta hm = host_rec_meta(n, n_fields, geo, span);
        parts = {{"record offsets", hm.at_recoff, (size_t)n * 4}, {"column offsets", hm.at_off, hm.off_stride * 4 * n_fields}, {"column places", hm.at_colat, (size_t)n_fields * 8},
                 {"counts", hm.at_counts, sizeof(pwaf_counts)}, {"out", hm.at_out, (size_t)n * sizeof(pwaf_verdict)}, {"records", hm.at_rec, span}};
        if (geo) parts.push_back({"geo", hm.at_geo, (size_t)n * sizeof(pwaf_geo)});
        note("host_rec_meta", check_parts(parts, hm.need));
        if (hm.off_stride < (size_t)n + 1 || hm.off_stride % 64) note("host_rec_meta", "a column's offsets do not fit its stride");
        if (hm.up_bytes != hm.at_out || hm.at_counts + up256(sizeof(pwaf_counts)) != hm.up_bytes) note("host_rec_meta", "the uploaded part does not end with the counters");
        if (hm.at_rec < hm.at_out || (geo && hm.at_rec < hm.at_geo)) note("host_rec_meta", "the records lie in front of what comes back");
        // -- rec_meta of device records
        const DeviceRecMeta dm = device_rec_meta(n, n_fields);
        parts = {{"summary", dm.at_sum, sizeof(records::ScanSummary)}, {"column places", dm.at_colat, (size_t)n_fields * 8}, {"tiles", dm.at_tile, dm.tile_stride * 8 * n_fields},
                 {"column offsets", dm.at_off, dm.off_stride * 4 * n_fields}};
        note("device_rec_meta", check_parts(parts, dm.size));
        if (dm.tile_stride < records::scan_tiles(n) || dm.off_stride < (size_t)n + 1) note("device_rec_meta", "a stride is too short");
    }
    printf("{\"cases\": %u, \"failures\": %u, \"packable\": %u, \"first\": \"%s\"}\n", cases, failures, packable, first.c_str());
    return 0;
}

static int record_cols(uint64_t seed, uint32_t cases) {
    Rng r(seed);
    static const uint64_t kTotals[] = {0, 1, 255, 256, 257, 0xFFFFFFF0ull, 0xFFFFFFEFull, 0xFFFFFF00ull, 0xFFFFFEFFull, 0xFFFFFFF0ull - 240, 0xFFFFFFF0ull - 241};
    uint32_t failures = 0;
    std::string first;
    for (uint32_t c = 0; c < cases; c++) {
        const uint32_t n = r.n(), n_cols = c % 7 == 0 ? kMaxCols : r.n_fields();
        const bool geo = r.coin();
        uint64_t totals[kMaxCols];
        for (uint32_t f = 0; f < n_cols; f++) totals[f] = r.coin() ? kTotals[r.below(sizeof kTotals / sizeof *kTotals)] : r.below(100000);
        // the reference: evaluate_records_impl's take loop as it stood before plan_record_cols replaced it
        size_t used = 0;
        const auto take = [&](size_t bytes) { const size_t at = used; used = (used + bytes + 255) & ~(size_t)255; return at; };
        uint64_t colat[kMaxCols];
        for (uint32_t f = 0; f < n_cols; f++) colat[f] = take(totals[f] + PWAF_ARENA_PAD);
        const size_t c_ip = take((size_t)n * 16), c_v6 = take(n), c_port = take((size_t)n * 2), c_flags = take(n);
        const size_t c_asn = geo ? take((size_t)n * 4) : 0, c_cc = geo ? take((size_t)n * 2) : 0;
        const RecordColsPlan p = plan_record_cols(totals, n_cols, n, geo);
        bool same = !memcmp(colat, p.col_at, 8 * (size_t)n_cols) && p.c_ip == c_ip && p.c_v6 == c_v6 && p.c_port == c_port && p.c_flags == c_flags && p.c_asn == c_asn &&
                    p.c_cc == c_cc && p.size == used && p.geo == geo;
        // ... and the launch arguments built from it: every pointer its place behind `arena`
        records::UnpackArgs ua{};
        uint8_t *const arena = (uint8_t *)(uintptr_t)0x10000000;
        const uint8_t *const rec = (const uint8_t *)(uintptr_t)0x20000000;
        const uint32_t *const rec_off = (const uint32_t *)(uintptr_t)0x30000000, *const off = (const uint32_t *)(uintptr_t)0x50000000;
        const uint64_t *const d_colat = (const uint64_t *)(uintptr_t)0x40000000;
        fill_unpack_args(ua, p, rec, rec_off, n, n_cols, arena, d_colat, off, 4096);
        same = same && ua.rec == rec && ua.rec_off == rec_off && ua.n == n && ua.n_cols == n_cols && ua.arena == arena && ua.col_at == d_colat && ua.off == off && ua.off_stride == 4096 &&
               ua.ip == arena + c_ip && ua.ip_is_v6 == arena + c_v6 && (uint8_t *)ua.port == arena + c_port && ua.flags == arena + c_flags &&
               (geo ? (uint8_t *)ua.asn == arena + c_asn && (uint8_t *)ua.country == arena + c_cc : !ua.asn && !ua.country);
        if (!same && !failures++) first = "case " + std::to_string(c) + " (n " + std::to_string(n) + ", " + std::to_string(n_cols) + " columns)";
    }
    printf("{\"cases\": %u, \"failures\": %u, \"first\": \"%s\"}\n", cases, failures, first.c_str());
    return 0;
}

// One batch of 300 requests, five fields and two header columns, every arena a few KiB but `big`, whose size the case chooses.
struct EdgeCase {
    static constexpr uint32_t n = 300, n_fields = PWAF_N_FIELDS + 2;
    HostCol col[kMaxCols];
    bool asn, geo, route;
    EdgeCase(bool asn_, bool geo_, bool route_) : asn(asn_), geo(geo_), route(route_) {
        const uint32_t last[n_fields] = {3000, 9000, 6000, 1200, 20000, 700, 0};
        for (uint32_t f = 0; f < n_fields; f++) col[f] = HostCol{true, 0, last[f]};
    }
    // the three conditions as the issue states them, in this file's own arithmetic: no column begins past 0; the running size stays within
    // kPackMax after every column; the whole block does
    size_t need = 0;
    bool expect() {
        bool ok = true;
        size_t used = 0;
        for (uint32_t f = 0; f < n_fields; f++) {
            if (col[f].first != 0) ok = false;
            used += up256((size_t)(n + 1) * 4) + up256((size_t)col[f].last + PWAF_ARENA_PAD);
            if (used > kPackMax) ok = false;
        }
        used += up256((size_t)n * 16) + up256(n) + up256((size_t)n * 2) + up256(n);
        if (asn) used += up256((size_t)n * 4) + up256((size_t)n * 2);
        used += up256(sizeof(pwaf_counts)) + up256((size_t)n * sizeof(pwaf_verdict));
        if (geo) used += up256((size_t)n * sizeof(pwaf_geo));
        if (route) used += up256((size_t)n * 4);
        need = used;
        return ok && used <= kPackMax;
    }
    // sizes column `big` so that the whole block is `target` bytes (a multiple of 256)
    void size_to(uint32_t big, size_t target) {
        col[big].last = 256 - PWAF_ARENA_PAD;
        expect();
        col[big].last += (uint32_t)(target - need);
    }
    void print(const char *name) {
        const bool want = expect();
        const PackedPlan p = plan_packed(n, n_fields, col, asn, geo, route);
        uint32_t placed = 0;  // columns that got a place
        for (uint32_t f = 0; f < n_fields; f++) placed += f == 0 ? 1u : (p.at_off[f] != 0 ? 1u : 0u);
        printf("{\"name\": \"%s\", \"asn\": %d, \"geo\": %d, \"route\": %d, \"need\": %zu, \"own_need\": %zu, \"packable\": %s, \"expected\": %s, \"placed\": %u}\n", name, asn, geo, route, p.need,
               need, p.packable ? "true" : "false", want ? "true" : "false", placed);
    }
};

static int packed_edges() {
    for (int mask = 0; mask < 8; mask++) {
        const bool asn = mask & 1, geo = mask & 2, route = mask & 4;
        for (const auto &t : {std::make_pair("exact", kPackMax), std::make_pair("above", kPackMax + 256), std::make_pair("below", kPackMax - 256)}) {
            EdgeCase e(asn, geo, route);
            e.size_to(1, t.second);  // (the url arena; the columns alone stay below kPackMax: only the final test can refuse)
            e.print(t.first);
        }
        {
            EdgeCase e(asn, geo, route);  // a column in the middle passes kPackMax by itself: the running check stops the loop there
            e.col[2].last = (uint32_t)kPackMax;
            e.print("running");
        }
        {
            EdgeCase e(asn, geo, route);  // a slab view of a larger arena: small, but its positions must stay
            e.col[4].first = 1;
            e.print("slab");
        }
    }
    return 0;
}

static void print_check(const char *name, int code) {
    printf("{\"name\": \"%s\", \"code\": %d, \"text\": \"%s\"}\n", name, code, code ? g_message.c_str() : "");
    g_message.clear();
}

static int host_columns() {
    constexpr uint32_t n = 9, n_fields = PWAF_N_FIELDS + 3;  // header columns: 5 present, 6 absent, 7 present (the last present column)
    const auto fresh = [&](std::vector<std::vector<uint32_t>> &o, const uint32_t **ptr) {
        o.assign(n_fields, {});
        for (uint32_t f = 0; f < n_fields; f++) {
            o[f].resize(n + 1);
            for (uint32_t i = 0; i <= n; i++) o[f][i] = 100 + 7 * f + 3 * i;  // (exactly n + 1 entries each: a read past them is the sanitizer's to report)
            ptr[f] = f == 6 ? nullptr : o[f].data();
        }
    };
    std::vector<std::vector<uint32_t>> o;
    const uint32_t *ptr[n_fields];
    std::vector<uint16_t> cc(n, (uint16_t)('F' | 'R' << 8));
    char name[64];
    fresh(o, ptr);
    print_check("ends: ordered", check_column_ends(n, n_fields, ptr));
    print_check("full: ordered", check_host_columns(n, n_fields, ptr, cc.data()));
    print_check("full: ordered, no country", check_host_columns(n, n_fields, ptr, nullptr));
    for (const uint32_t f : {0u, 7u})
        for (const uint32_t i : {0u, 4u, n - 1}) {  // the pair (i, i + 1) descends
            fresh(o, ptr);
            o[f][i + 1] = o[f][i] - 1;
            snprintf(name, sizeof name, "full: column %u pair %u", f, i);
            print_check(name, check_host_columns(n, n_fields, ptr, cc.data()));
        }
    for (const uint32_t f : {0u, 7u}) {
        fresh(o, ptr);
        o[f][n] = o[f][0] - 1;
        snprintf(name, sizeof name, "ends: column %u", f);
        print_check(name, check_column_ends(n, n_fields, ptr));
        snprintf(name, sizeof name, "full: column %u end before begin", f);
        print_check(name, check_host_columns(n, n_fields, ptr, cc.data()));
    }
    fresh(o, ptr);
    for (const char *v : {"@A", "A[", "AA", "ZZ", "fr", "Fr", "fR"})
        for (const uint32_t at : {0u, n - 1}) {
            std::vector<uint16_t> c2 = cc;
            c2[at] = (uint16_t)((uint8_t)v[0] | (uint8_t)v[1] << 8);
            snprintf(name, sizeof name, "country %s at %u", v, at);
            print_check(name, check_host_columns(n, n_fields, ptr, c2.data()));
        }
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if ((what == "invariants" || what == "record_cols") && argc == 4) {
        const uint64_t seed = strtoull(argv[2], nullptr, 10);
        const uint32_t cases = (uint32_t)strtoul(argv[3], nullptr, 10);
        return what == "invariants" ? invariants(seed, cases) : record_cols(seed, cases);
    }
    if (what == "packed_edges" && argc == 2) return packed_edges();
    if (what == "host_columns" && argc == 2) return host_columns();
    fprintf(stderr, "usage: staging_host invariants|record_cols <seed> <cases> | packed_edges | host_columns\n");
    return 2;
}
