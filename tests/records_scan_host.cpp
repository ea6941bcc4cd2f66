// records_scan_host.cpp — the device form of record validation (csrc/records.h: scan_check, first_geo, scan_len, column_too_big,
// place_columns, the failure key; what records_scan.hip's three launches run) as a stand-alone program: tests/test_records_device_cpu.py
// builds it with g++, a second time with -fsanitize=address,undefined, and runs both.
//
//   records_scan_host <n_cols> <buf file> <buf_bytes | -1> [<rec_off file> <n_rec | -1>]...
//
// The buffer is a heap block of EXACTLY buf_bytes bytes (the file's first buf_bytes bytes; -1: all of it) and every offset list a heap
// block of exactly its entries: a read one byte outside either is the sanitizer's to report. For every offset list the program runs the
// three phases as loops over tiles — the grid sized from n, the work cut at m = min(n_rec, n), tile sums and bases per column, phase 2
// in steps of kScanStep tiles — and compares with records::validate and records::column_offsets over the first m entries: the failing
// (index, check), or m, has_geoip, every total, every column place and every offset. One JSON line per list; exit status 0 unless the
// arguments are wrong ("same" carries the verdict).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../pingoo_amd/csrc/records.h"
#include "../pingoo_amd/csrc/staging.h"

namespace R = pwaf::records;

static bool read_file(const char *path, std::vector<uint8_t> &out) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long len = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize((size_t)len);
    const bool ok = len == 0 || std::fread(out.data(), 1, (size_t)len, f) == (size_t)len;
    std::fclose(f);
    return ok;
}

struct Scan {
    uint64_t key = R::kNoFailure;
    uint32_t m = 0, has_geoip = 0;
    std::vector<uint64_t> totals, col_at;
    std::vector<uint32_t> off;  // n_cols x stride
    size_t stride = 0;
};

// the three launches, workgroup by workgroup and lane by lane
static void scan(const uint8_t *buf, uint64_t buf_bytes, const uint32_t *rec_off, uint32_t n, const uint32_t *n_rec, uint32_t n_cols, Scan &s) {
    const uint32_t T = R::kScanTile, grid = R::scan_tiles(n);
    const size_t tile_stride = grid ? grid : 1;
    s.stride = R::offsets_stride(n);
    s.off.assign(s.stride * n_cols, 0xDEADBEEFu);
    s.totals.assign(n_cols, 0);
    s.col_at.assign(n_cols, 0);
    std::vector<uint64_t> tile(tile_stride * n_cols, 0xDEADBEEFDEADBEEFull);
    const uint32_t m = R::records_in_call(n_rec, n);
    // phase 1
    for (uint32_t b = 0; b < grid; b++) {
        if ((uint64_t)b * T >= m) continue;
        const uint32_t geo0 = R::first_geo(buf, buf_bytes, rec_off[0]);
        std::vector<uint64_t> part(n_cols, 0);
        for (uint32_t tid = 0; tid < T; tid++) {
            const uint64_t i = (uint64_t)b * T + tid;
            if (i >= m) continue;
            uint32_t nv = 0;
            const uint32_t o = rec_off[i];
            const int c = R::scan_check(buf, buf_bytes, o, n_cols, geo0, &nv);
            if (c != R::kOk) {
                const uint64_t k = R::fail_key((uint32_t)i, c);
                if (k < s.key) s.key = k;
            }
            for (uint32_t f = 0; f < n_cols; f++) {
                const uint32_t len = R::scan_len(buf + o, nv, f);  // (nv == 0 for a failing record: buf + o is never read through)
                s.off[(size_t)f * s.stride + i + 1] = len;
                part[f] += len;
            }
        }
        for (uint32_t f = 0; f < n_cols; f++) tile[(size_t)f * tile_stride + b] = part[f];
    }
    // phase 2
    const uint32_t n_tiles = R::scan_tiles(m);
    for (uint32_t f = 0; f < n_cols; f++) {
        uint64_t *const t = tile.data() + (size_t)f * tile_stride;
        uint64_t carry = 0;
        uint32_t first_tile = 0xFFFFFFFFu;
        for (uint32_t t0 = 0; t0 < n_tiles; t0 += R::kScanStep) {
            uint64_t run = 0;  // the step's own prefix, then the carry on top: as the workgroup does
            for (uint32_t tid = 0; tid < R::kScanStep && t0 + tid < n_tiles; tid++) {
                const uint64_t x = t[t0 + tid];
                run += x;
                const uint64_t incl = carry + run;
                t[t0 + tid] = incl - x;
                if (R::column_too_big(incl) && !R::column_too_big(incl - x)) first_tile = t0 + tid;
            }
            carry += run;
        }
        s.totals[f] = carry;
        if (first_tile == 0xFFFFFFFFu) continue;
        uint64_t run = t[first_tile];
        for (uint32_t r = 0; r < T; r++) {
            const uint64_t i = (uint64_t)first_tile * T + r;
            const uint64_t x = i < m ? s.off[(size_t)f * s.stride + i + 1] : 0u;
            const uint64_t incl = run + x;
            if (R::column_too_big(incl) && !R::column_too_big(run)) {
                const uint64_t k = R::fail_key((uint32_t)i, R::kColumnTooBig);
                if (k < s.key) s.key = k;
            }
            run = incl;
        }
    }
    // phase 3
    s.m = m;
    s.has_geoip = m ? R::first_geo(buf, buf_bytes, rec_off[0]) : 0u;
    R::place_columns(s.totals.data(), n_cols, s.col_at.data());
    if (s.key != R::kNoFailure) return;
    for (uint32_t b = 0; b < grid; b++) {
        if ((uint64_t)b * T >= m) continue;
        for (uint32_t f = 0; f < n_cols; f++) {
            uint32_t *const off = s.off.data() + (size_t)f * s.stride;
            uint32_t carry = (uint32_t)tile[(size_t)f * tile_stride + b];
            if (b == 0) off[0] = 0;
            for (uint32_t r = 0; r < T; r++) {
                const uint64_t i = (uint64_t)b * T + r;
                if (i >= m) break;
                carry += off[i + 1];
                off[i + 1] = carry;
            }
        }
    }
}

int main(int argc, char **argv) {
    if (argc < 4 || (argc - 4) % 2) {
        std::fprintf(stderr, "usage: records_scan_host <n_cols> <buf file> <buf_bytes | -1> [<rec_off file> <n_rec | -1>]...\n");
        return 2;
    }
    const uint32_t n_cols = (uint32_t)std::strtoul(argv[1], nullptr, 10);
    std::vector<uint8_t> file;
    if (n_cols < PWAF_N_FIELDS || n_cols > R::kMaxValues || !read_file(argv[2], file)) return 2;
    const long long cut = std::strtoll(argv[3], nullptr, 10);
    const uint64_t buf_bytes = cut < 0 ? file.size() : (uint64_t)cut;
    if (buf_bytes > file.size()) return 2;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[buf_bytes ? buf_bytes : 1]);  // (operator new: 16-byte aligned) exactly buf_bytes bytes
    if (buf_bytes) memcpy(buf.get(), file.data(), buf_bytes);
    for (int a = 4; a + 1 < argc; a += 2) {
        std::vector<uint8_t> raw;
        if (!read_file(argv[a], raw) || raw.size() % 4) return 2;
        const uint32_t n = (uint32_t)(raw.size() / 4);
        std::unique_ptr<uint32_t[]> rec_off(new uint32_t[n ? n : 1]);
        if (n) memcpy(rec_off.get(), raw.data(), raw.size());
        const long long nr = std::strtoll(argv[a + 1], nullptr, 10);
        const uint32_t n_rec_value = (uint32_t)nr;
        const uint32_t *const n_rec = nr < 0 ? nullptr : &n_rec_value;
        Scan s;
        scan(buf.get(), buf_bytes, rec_off.get(), n, n_rec, n_cols, s);
        // the host call's way, over the m records the call looks at
        const uint32_t m = nr < 0 ? n : ((uint64_t)nr < n ? (uint32_t)nr : n);
        std::vector<uint64_t> totals(n_cols);
        uint32_t bad = 0;
        int geo = 0;
        uint64_t lo = 0, hi = 0;
        const int chk = R::validate(buf.get(), buf_bytes, rec_off.get(), m, n_cols, totals.data(), &bad, &geo, &lo, &hi);
        bool same = s.m == m;
        if (chk != R::kOk) {
            same = same && s.key != R::kNoFailure && R::key_index(s.key) == bad && R::key_check(s.key) == chk;
        } else {
            same = same && s.key == R::kNoFailure && s.has_geoip == (uint32_t)geo;
            const size_t stride = (size_t)m + 1;
            std::vector<uint32_t> want(stride * n_cols);
            R::column_offsets(buf.get(), rec_off.get(), m, n_cols, want.data(), stride);
            pwaf::Layout cl;  // (the grid the host call places its columns on)
            for (uint32_t f = 0; f < n_cols && same; f++) {
                same = s.totals[f] == totals[f] && s.col_at[f] == cl.take((size_t)totals[f] + PWAF_ARENA_PAD);
                if (m) same = same && !memcmp(s.off.data() + (size_t)f * s.stride, want.data() + (size_t)f * stride, stride * 4);
            }
        }
        const bool failed = s.key != R::kNoFailure;
        std::printf("{\"same\": %s, \"ok\": %s, \"n\": %u, \"m\": %u, \"index\": %u, \"check\": %d, \"ref_ok\": %s, \"ref_index\": %u, \"ref_check\": %d, \"has_geoip\": %u}\n",
                    same ? "true" : "false", failed ? "false" : "true", n, s.m, failed ? R::key_index(s.key) : 0u, failed ? R::key_check(s.key) : 0,
                    chk == R::kOk ? "true" : "false", chk == R::kOk ? 0u : bad, chk, failed ? 0u : s.has_geoip);
    }
    return 0;
}
