// records.h — the request record of include/pwaf.h (pwaf_record_head + lengths + values): layout, validation, decoding, and (second half)
// packing: pwaf_export_records.
//
// One header, compiled three ways, like confirm.h: by records.hip (unpack_records_kernel decodes records on the device), by evaluate_records.cpp
// (pwaf_evaluate_records validates every record and computes the column offsets on the host before anything is launched) and by
// tests/records_host.cpp (g++: the CPU suite checks validation and decoding against RequestBatch's own columns). Validation is what
// guarantees the kernel never reads outside the uploaded buffer: the kernel trusts every head it reads.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "pwaf.h"
#include "service.h"

namespace pwaf {
namespace records {

static constexpr uint32_t kHead = (uint32_t)sizeof(pwaf_record_head);
// PWAF_N_FIELDS + program.h kMaxHeaders (evaluate_records.cpp, which sees both headers, asserts it): sizes the kernel's LDS prefix and async.cpp's
// per-request arrays; pwaf_evaluate_records and pwaf_async_create also refuse an engine with more columns at run time
static constexpr uint32_t kMaxValues = PWAF_N_FIELDS + 120;
static constexpr uint64_t kMaxColumn = 0xFFFFFFF0ull;         // a column's bytes: uint32 offsets, PWAF_ARENA_PAD behind them
static_assert(sizeof(pwaf_record_head) == 36, "pwaf_record_head layout");

// where the values of a record with n_values lengths begin (16-byte aligned inside the record) and the record's size
PWAF_SVC_HD uint32_t values_offset(uint32_t n_values) { return (kHead + 4u * n_values + 15u) & ~15u; }
PWAF_SVC_HD uint64_t record_size(uint32_t n_values, uint64_t value_bytes) { return ((uint64_t)values_offset(n_values) + value_bytes + 15u) & ~(uint64_t)15u; }

// (memcpy: a host buffer is only byte-aligned as far as the C ABI knows)
PWAF_SVC_HD void load_head(const uint8_t *rec, pwaf_record_head *h) { memcpy(h, rec, kHead); }
PWAF_SVC_HD uint32_t load_len(const uint8_t *rec, uint32_t k) {
    uint32_t v;
    memcpy(&v, rec + kHead + 4u * k, 4);
    return v;
}

enum Check : int {
    kOk = 0,
    kMisaligned,   // offset not a multiple of 16
    kPastEnd,      // the head or the record runs past the buffer
    kBadSize,      // size not a multiple of 16, or smaller than the head
    kBadCount,     // n_values outside PWAF_N_FIELDS .. max_values
    kOverflow,     // lengths (and the head) do not fit `size`
    kBadGeoFlag,   // has_geoip neither 0 nor 1
    kBadCountry,   // has_geoip and country not two letters A-Z
    kMixedGeo,     // has_geoip differs from the call's first record
    kColumnTooBig  // a column of the call would exceed 4 GiB
};

inline const char *check_message(int c) {
    switch (c) {
        case kMisaligned: return "record offset is not a multiple of 16";
        case kPastEnd: return "record runs past the end of the buffer";
        case kBadSize: return "record size is not a multiple of 16 or smaller than its head";
        case kBadCount: return "n_values is outside 5 .. 5 + the engine's header count";
        case kOverflow: return "record's lengths overflow its size";
        case kBadGeoFlag: return "has_geoip is neither 0 nor 1";
        case kBadCountry: return "country is not two letters A-Z (pingoo/geoip.rs:128-142)";
        case kMixedGeo: return "has_geoip differs between the records of one call";
        case kColumnTooBig: return "a column of the call would exceed 4 GiB";
        default: return "ok";
    }
}

// One record at byte offset `off` of a buffer of buf_bytes bytes: kOk or what is wrong with it. Reads nothing outside the buffer.
// *value_bytes = the sum of its lengths.
PWAF_SVC_HD int check_record(const uint8_t *buf, uint64_t buf_bytes, uint64_t off, uint32_t max_values, uint64_t *value_bytes) {
    if (off & 15u) return kMisaligned;
    if (off > buf_bytes || buf_bytes - off < kHead) return kPastEnd;
    pwaf_record_head h;
    load_head(buf + off, &h);
    if ((h.size & 15u) || h.size < kHead) return kBadSize;
    if (buf_bytes - off < h.size) return kPastEnd;
    if (h.n_values < PWAF_N_FIELDS || h.n_values > max_values) return kBadCount;
    const uint32_t vo = values_offset(h.n_values);
    if (vo > h.size) return kOverflow;
    uint64_t sum = 0;
    for (uint32_t k = 0; k < h.n_values; k++) sum += load_len(buf + off, k);
    if (sum > (uint64_t)(h.size - vo)) return kOverflow;
    if (h.has_geoip > 1u) return kBadGeoFlag;
    if (h.has_geoip && ((uint32_t)(h.country[0] - 'A') > 25u || (uint32_t)(h.country[1] - 'A') > 25u)) return kBadCountry;
    *value_bytes = sum;
    return kOk;
}

// The whole call (host side): every record checked, has_geoip the same everywhere, totals[f] = column f's bytes (n_cols columns; values
// a record does not carry count as ""). kOk, or the failing check with *bad = the index i of the record (rec_off[i]). *has_geoip = the
// records' common flag. *lo / *hi: the byte span [lo, hi) of buf the records occupy (what has to travel).
inline int validate(const uint8_t *buf, uint64_t buf_bytes, const uint32_t *rec_off, uint32_t n, uint32_t n_cols, uint64_t *totals, uint32_t *bad,
                    int *has_geoip, uint64_t *lo, uint64_t *hi) {
    for (uint32_t f = 0; f < n_cols; f++) totals[f] = 0;
    *lo = n ? UINT64_MAX : 0;
    *hi = 0;
    *has_geoip = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint64_t vb = 0;
        int c = check_record(buf, buf_bytes, rec_off[i], n_cols, &vb);
        if (c == kOk) {
            pwaf_record_head h;
            load_head(buf + rec_off[i], &h);
            if (i == 0) *has_geoip = h.has_geoip;
            else if ((int)h.has_geoip != *has_geoip) c = kMixedGeo;
            if (c == kOk) {
                for (uint32_t k = 0; k < h.n_values; k++) totals[k] += load_len(buf + rec_off[i], k);
                for (uint32_t k = 0; k < h.n_values; k++)
                    if (totals[k] > kMaxColumn) c = kColumnTooBig;
                if (rec_off[i] < *lo) *lo = rec_off[i];
                if (rec_off[i] + (uint64_t)h.size > *hi) *hi = rec_off[i] + (uint64_t)h.size;
            }
        }
        if (c != kOk) {
            *bad = i;
            return c;
        }
    }
    return kOk;
}

// The struct-of-arrays offsets of a VALIDATED call: column f's n + 1 offsets at off[f * stride .. f * stride + n] (request i = the record
// at rec_off[i]; a value the record does not carry is "").
inline void column_offsets(const uint8_t *buf, const uint32_t *rec_off, uint32_t n, uint32_t n_cols, uint32_t *off, size_t stride) {
    for (uint32_t f = 0; f < n_cols; f++) off[f * stride] = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t *r = buf + rec_off[i];
        uint16_t nv;
        memcpy(&nv, r + 4, 2);
        for (uint32_t f = 0; f < n_cols; f++) off[f * stride + i + 1] = off[f * stride + i] + (f < nv ? load_len(r, f) : 0u);
    }
}

// unpack_records_kernel's arguments (records.hip). The device batch it writes is what run_pipeline reads: column f's arena at
// arena + col_at[f] (its offsets at off + f * off_stride, computed by the host: column_offsets), the fixed columns in pwaf_batch layout.
struct UnpackArgs {
    const uint8_t *rec;       // the records' bytes on the device (256-byte aligned)
    const uint32_t *rec_off;  // n: record of request i, relative to rec
    uint32_t n, n_cols;
    uint8_t *arena;
    const uint64_t *col_at;   // n_cols
    const uint32_t *off;      // n_cols x off_stride
    uint32_t off_stride;
    uint8_t *ip, *ip_is_v6, *flags;
    uint16_t *port, *country;  // country: null when the records carry no GeoIP
    uint32_t *asn;
};
int launch_unpack_records(const UnpackArgs &a, void *stream);

// ---- validate + column_offsets for records that lie in DEVICE memory (pwaf_evaluate_records_device): reduce-then-scan over tiles of
// kScanTile records, in three launches (records_scan.hip) that never wait for one another's workgroups:
//   1 check + lengths   every record through scan_check; its lengths (0 where it fails or does not carry the column) into the offsets
//                       array, one slot up; per tile and column a 64-bit sum; the lowest failing (index, check) by atomicMin on a key
//   2 tile bases        per column: the tile sums become exclusive prefixes (kScanStep tiles a step), the last one the column's total; the
//                       first record at which the column's running total exceeds kMaxColumn joins the key as kColumnTooBig
//   3 offsets           every tile rescans its lengths from its base, in place; its first workgroup fills the summary and places the columns
// The per-record and per-column arithmetic below is compiled by the kernels, by evaluate_records.cpp and by tests/records_scan_host.cpp (g++ under
// the sanitizers, the three phases as loops over tiles): what keeps every read inside [buf, buf + buf_bytes) is check_record, as above.
static constexpr uint32_t kScanTile = 256;  // records per tile: one per lane of a phase-1 workgroup
static constexpr uint32_t kScanStep = 256;  // tiles one step of phase 2 takes: one per lane
static constexpr uint64_t kNoFailure = ~0ull;

// the failure key: ordered by (index, check), so that the minimum names what validate()'s loop meets first
PWAF_SVC_HD uint64_t fail_key(uint32_t i, int check) { return ((uint64_t)i << 32) | (uint32_t)check; }
PWAF_SVC_HD uint32_t key_index(uint64_t key) { return (uint32_t)(key >> 32); }
PWAF_SVC_HD int key_check(uint64_t key) { return (int)(uint32_t)key; }

// the records a call looks at: min(*n_rec, n), or n without a count
PWAF_SVC_HD uint32_t records_in_call(const uint32_t *n_rec, uint32_t n) {
    if (!n_rec) return n;
    const uint32_t k = *n_rec;
    return k < n ? k : n;
}
PWAF_SVC_HD uint32_t scan_tiles(uint32_t m) { return m / kScanTile + (m % kScanTile ? 1u : 0u); }
// a column's n + 1 offsets, on a 256-byte grid (evaluate_records_impl's stride)
PWAF_SVC_HD size_t offsets_stride(uint32_t n) { return ((size_t)n + 1 + 63) & ~(size_t)63; }

// has_geoip of the call's first record where its head can be read, else a value no record has (the record then fails at index 0, and
// no kMixedGeo behind it is ever reported)
PWAF_SVC_HD uint32_t first_geo(const uint8_t *buf, uint64_t buf_bytes, uint32_t off0) {
    if ((off0 & 15u) || off0 > buf_bytes || buf_bytes - off0 < kHead) return 0xFFFFFFFFu;
    return buf[(size_t)off0 + offsetof(pwaf_record_head, has_geoip)];
}
// One record of the call, as validate() judges it apart from the column totals: check_record, then has_geoip against the first record's.
// *n_values = the lengths it carries (0 unless kOk).
PWAF_SVC_HD int scan_check(const uint8_t *buf, uint64_t buf_bytes, uint32_t off, uint32_t n_cols, uint32_t geo0, uint32_t *n_values) {
    *n_values = 0;
    uint64_t vb = 0;
    const int c = check_record(buf, buf_bytes, off, n_cols, &vb);
    if (c != kOk) return c;
    const uint8_t *r = buf + off;
    if (r[offsetof(pwaf_record_head, has_geoip)] != geo0) return kMixedGeo;
    uint16_t nv;
    memcpy(&nv, r + offsetof(pwaf_record_head, n_values), 2);
    *n_values = nv;
    return kOk;
}
// the length a record with n_values lengths contributes to column f
PWAF_SVC_HD uint32_t scan_len(const uint8_t *rec, uint32_t n_values, uint32_t f) { return f < n_values ? load_len(rec, f) : 0u; }
// a column's running total, inclusive of a record: validate()'s kColumnTooBig
PWAF_SVC_HD bool column_too_big(uint64_t inclusive_total) { return inclusive_total > kMaxColumn; }
// Where the columns go in the unpacked batch: each total plus PWAF_ARENA_PAD, on the 256-byte grid of staging.h's Layout::take.
// Returns the bytes the columns occupy together (where the fixed columns begin).
PWAF_SVC_HD uint64_t place_columns(const uint64_t *totals, uint32_t n_cols, uint64_t *col_at) {
    uint64_t used = 0;
    for (uint32_t f = 0; f < n_cols; f++) {
        col_at[f] = used;
        used = (used + totals[f] + PWAF_ARENA_PAD + 255u) & ~(uint64_t)255u;
    }
    return used;
}

// What the host reads back, once per call: the failure key (kNoFailure: a valid call), the offset of the record it names, the records
// evaluated, their common has_geoip, and every column's bytes.
struct ScanSummary {
    uint64_t key;
    uint32_t bad_off, m, has_geoip, reserved;
    uint64_t totals[kMaxValues];
};
PWAF_SVC_HD size_t summary_bytes(uint32_t n_cols) { return offsetof(ScanSummary, totals) + 8u * (size_t)n_cols; }

// The three launches' arguments. off / col_at are what UnpackArgs then takes; nothing here is the caller's memory but buf, rec_off, n_rec.
struct ScanArgs {
    const uint8_t *buf;  // the records: exactly buf_bytes bytes, no pad behind them
    uint64_t buf_bytes;
    const uint32_t *rec_off;  // n
    const uint32_t *n_rec;    // nullable
    uint32_t n, n_cols;
    uint32_t *off;  // n_cols x off_stride: slot i + 1 of column f holds record i's length after phase 1, its end offset after phase 3
    uint32_t off_stride;
    uint32_t tile_stride;  // >= scan_tiles(n)
    uint64_t *tile;        // n_cols x tile_stride: tile sums after phase 1, tile bases after phase 2
    uint64_t *col_at;      // n_cols
    ScanSummary *sum;      // (key set to kNoFailure in front of phase 1)
};
extern const char *const kScanKernelNames[3];
int launch_scan_records(int phase /* 1 .. 3 */, const ScanArgs &a, void *stream);

// ---- packing: the inverse (pwaf_export_records). Selected requests of a batch's columns -> records, byte for byte what
// RequestBatch.to_records builds. The same three compilations: pack_records_kernel (records.hip), the HOST mode of the entry point (a loop
// over pack_record: export_host below) and tests/records_pack_host.cpp (g++ under the sanitizers).
static constexpr uint64_t kMaxRecord = 0xFFFFFFF0ull;  // head.size and rec_off are 32 bits wide

// pack_records_kernel's arguments, and export_host's. The column descriptors travel BY VALUE — on the device inside the kernel argument
// block (kMaxValues x 16 = 2000 bytes of the 4 KiB a launch may carry) — so a call owns no scratch and uploads nothing. Column k < 5 is
// field k, column 5 + h header h; a descriptor with a NULL pointer reads as "" for every request.
struct PackArgs {
    pwaf_strcol col[kMaxValues];
    uint32_t n, n_cols;  // requests of the batch; columns in use (PWAF_N_FIELDS + n_headers)
    const uint8_t *ip, *ip_is_v6, *flags;
    const uint16_t *port, *country;  // country / asn: both or has_geoip = 0
    const uint32_t *asn;
    const uint32_t *idx;    // idx_cap entries
    const uint32_t *n_idx;  // nullable: min(*n_idx, idx_cap) entries are looked at
    uint32_t idx_cap;
    uint8_t *buf;
    uint64_t buf_cap;
    uint32_t *rec_off;
    pwaf_export_stats *stats;
};

PWAF_SVC_HD uint32_t selected(const PackArgs &a) { return list_length(a.n_idx, a.idx_cap); }  // (there is always a list: idx NULL only with idx_cap == 0)
// length of column k's value of request i (uint32 arithmetic, as every reader of the offsets does; monotone offsets are export_host's check)
PWAF_SVC_HD uint32_t col_len(const pwaf_strcol &c, uint32_t i) { return c.data && c.offsets ? c.offsets[i + 1] - c.offsets[i] : 0u; }

// What a request's record looks like, from its column lengths: add() them in column order.
struct ExportShape {
    uint32_t n_values = PWAF_N_FIELDS;  // ends after the last non-empty header value
    uint64_t value_bytes = 0;
    PWAF_SVC_HD void add(uint32_t k, uint32_t len) {
        value_bytes += len;
        if (len && k >= PWAF_N_FIELDS) n_values = k + 1;
    }
    PWAF_SVC_HD uint64_t size() const { return record_size(n_values, value_bytes); }
    // a record that cannot be described in 32 bits is not exported (PWAF_RECORD_NONE, not counted)
    PWAF_SVC_HD uint32_t size32() const { return size() > kMaxRecord ? 0u : (uint32_t)size(); }
};
PWAF_SVC_HD ExportShape export_shape(const PackArgs &a, uint32_t i) {
    ExportShape s;
    for (uint32_t k = 0; k < a.n_cols; k++) s.add(k, col_len(a.col[k], i));
    return s;
}

// the head of request i's record (every byte of *h is written: reserved and the GeoIP fields of a batch without GeoIP are 0)
PWAF_SVC_HD void fill_head(const PackArgs &a, uint32_t i, uint32_t n_values, uint32_t size, pwaf_record_head *h) {
    memset(h, 0, kHead);
    h->size = size;
    h->n_values = (uint16_t)n_values;
    h->port = a.port[i];
    memcpy(h->ip, a.ip + (size_t)i * 16, 16);
    h->flags = a.flags[i];
    h->ip_is_v6 = a.ip_is_v6[i];
    if (a.asn && a.country) {
        h->has_geoip = 1;
        h->asn = a.asn[i];
        memcpy(h->country, &a.country[i], 2);
    }
}

// One record, written by one thread: request i with shape s (s.size32() != 0) to dst, s.size() bytes, every one of them written.
PWAF_SVC_HD void pack_record(const PackArgs &a, uint32_t i, const ExportShape &s, uint8_t *dst) {
    const uint32_t size = s.size32(), vo = values_offset(s.n_values);
    pwaf_record_head h;
    fill_head(a, i, s.n_values, size, &h);
    memcpy(dst, &h, kHead);
    uint8_t *at = dst + vo;
    for (uint32_t k = 0; k < s.n_values; k++) {
        const uint32_t len = col_len(a.col[k], i);
        memcpy(dst + kHead + 4u * k, &len, 4);
        if (len) memcpy(at, a.col[k].data + a.col[k].offsets[i], len);
        at += len;
    }
    memset(dst + kHead + 4u * s.n_values, 0, vo - (kHead + 4u * s.n_values));
    memset(at, 0, (size_t)(dst + size - at));
}

// The HOST mode of pwaf_export_records, after the entry point's argument checks: plain C++, no device. First every selected request of the
// batch is checked (offsets that decrease: false with *bad = the list entry j, nothing written), then the records are laid out in list
// order. The rule pack_records_kernel follows too: the byte cursor advances by every valid record, and a record is written iff its whole
// range lies below buf_cap — so the written ones form a prefix of buf without holes.
inline bool export_host(const PackArgs &a, uint32_t *bad) {
    const uint32_t m = selected(a);
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t i = a.idx[j];
        if (i >= a.n) continue;
        for (uint32_t k = 0; k < a.n_cols; k++)
            if (a.col[k].data && a.col[k].offsets && a.col[k].offsets[i + 1] < a.col[k].offsets[i]) {
                *bad = j;
                return false;
            }
    }
    uint64_t cursor = 0;
    uint32_t written = 0;
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t i = a.idx[j];
        a.rec_off[j] = PWAF_RECORD_NONE;
        if (i >= a.n) continue;
        const ExportShape s = export_shape(a, i);
        const uint32_t size = s.size32();
        if (!size) continue;
        if (cursor + size <= a.buf_cap) {
            pack_record(a, i, s, a.buf + cursor);
            a.rec_off[j] = (uint32_t)cursor;
            written++;
        }
        cursor += size;
    }
    a.stats->bytes_needed = cursor;
    a.stats->n_selected = m;
    a.stats->n_written = written;
    return true;
}
int launch_pack_records(const PackArgs &a, void *stream);

}  // namespace records
}  // namespace pwaf
