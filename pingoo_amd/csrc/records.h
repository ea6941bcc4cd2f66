// records.h — the request record of include/pwaf.h (pwaf_record_head + lengths + values): layout, validation, decoding.
//
// One header, compiled three ways, like confirm.h: by records.hip (unpack_records_kernel decodes records on the device), by engine.cpp
// (pwaf_evaluate_records validates every record and computes the column offsets on the host before anything is launched) and by
// tests/records_host.cpp (g++: the CPU suite checks validation and decoding against RequestBatch's own columns). Validation is what
// guarantees the kernel never reads outside the uploaded buffer: the kernel trusts every head it reads.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "pwaf.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define PWAF_RECORD_HD __host__ __device__ inline
#else
#define PWAF_RECORD_HD inline
#endif

namespace pwaf {
namespace records {

static constexpr uint32_t kHead = (uint32_t)sizeof(pwaf_record_head);
// PWAF_N_FIELDS + program.h kMaxHeaders (engine.cpp, which sees both headers, asserts it): sizes the kernel's LDS prefix and async.cpp's
// per-request arrays; pwaf_evaluate_records and pwaf_async_create also refuse an engine with more columns at run time
static constexpr uint32_t kMaxValues = PWAF_N_FIELDS + 120;
static constexpr uint64_t kMaxColumn = 0xFFFFFFF0ull;         // a column's bytes: uint32 offsets, PWAF_ARENA_PAD behind them
static_assert(sizeof(pwaf_record_head) == 36, "pwaf_record_head layout");

// where the values of a record with n_values lengths begin (16-byte aligned inside the record) and the record's size
PWAF_RECORD_HD uint32_t values_offset(uint32_t n_values) { return (kHead + 4u * n_values + 15u) & ~15u; }
PWAF_RECORD_HD uint64_t record_size(uint32_t n_values, uint64_t value_bytes) { return ((uint64_t)values_offset(n_values) + value_bytes + 15u) & ~(uint64_t)15u; }

// (memcpy: a host buffer is only byte-aligned as far as the C ABI knows)
PWAF_RECORD_HD void load_head(const uint8_t *rec, pwaf_record_head *h) { memcpy(h, rec, kHead); }
PWAF_RECORD_HD uint32_t load_len(const uint8_t *rec, uint32_t k) {
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
PWAF_RECORD_HD int check_record(const uint8_t *buf, uint64_t buf_bytes, uint64_t off, uint32_t max_values, uint64_t *value_bytes) {
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

}  // namespace records
}  // namespace pwaf
