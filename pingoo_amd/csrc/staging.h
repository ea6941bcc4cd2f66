// staging.h — where the parts of the entry points' staging blocks lie, and what the host checks of a HOST batch's columns before the
// device reads them: the arithmetic of evaluate.cpp (pwaf_evaluate_batch) and evaluate_records.cpp (pwaf_evaluate_records*), apart from
// the copies it is for. No HIP in here and no environment reads: everything runs, and is tested, without a device
// (tests/staging_host.cpp: g++, also under AddressSanitizer + UBSan; tests/test_staging_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "records.h"
#include "service.h"  // (fail)

#pragma GCC visibility push(hidden)  // (internal to libpwaf.so, like everything of the engine's that several units share: engine_impl.h)
namespace pwaf {

// Parts of one block (the zeroed block, the descriptor block, the staging blocks of the host entry points), each on a 256-byte boundary.
struct Layout {
    size_t used = 0;
    size_t take(size_t bytes) { const size_t at = used; used = (used + bytes + 255) & ~(size_t)255; return at; }
    size_t size() const { return used; }
};

// string columns a batch can have: the five fields and every header column a rule set may name (records.h; evaluate_records.cpp asserts
// it against program.h's kMaxHeaders)
static constexpr uint32_t kMaxCols = records::kMaxValues;

// ---- a HOST batch's columns (pwaf_evaluate_batch) ----

// The ends of every column must be ordered before any size is computed from them (check_host_columns is the full check). offsets[f]:
// column f's n + 1 offsets, null for a header column the batch does not carry.
inline int check_column_ends(uint32_t n, uint32_t n_fields, const uint32_t *const *offsets) {
    for (uint32_t f = 0; f < n_fields; f++)
        if (offsets[f] && offsets[f][n] < offsets[f][0]) return fail(PWAF_E_BATCH, "field offsets are not monotone");
    return PWAF_OK;
}
// What a device cannot report: offsets that decrease, a country that is not two letters A-Z (nullable: the batch carries no GeoIP).
inline int check_host_columns(uint32_t n, uint32_t n_fields, const uint32_t *const *offsets, const uint16_t *country) {
    for (uint32_t f = 0; f < n_fields; f++) {
        const uint32_t *o = offsets[f];
        if (!o) continue;
        uint32_t bad = 0;
        for (uint32_t i = 0; i < n; i++) bad |= (uint32_t)(o[i + 1] < o[i]);  // (branch-free: the loop vectorizes)
        if (bad) return fail(PWAF_E_BATCH, "field offsets are not monotone");
    }
    if (country) {
        uint32_t bad = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t c0 = (country[i] & 0xFFu) - 'A', c1 = ((uint32_t)country[i] >> 8) - 'A';
            bad |= (uint32_t)(c0 > 25u) | (uint32_t)(c1 > 25u);
        }
        if (bad) return fail(PWAF_E_BATCH, "country is not two letters A-Z (pingoo/geoip.rs:128-142)");
    }
    return PWAF_OK;
}

// A SMALL host batch travels as ONE packed block:
// [offsets + arena of every column] [ip] [v6] [port] [flags] [asn] [country] [counters] | [verdicts] [geo] [routes], each 256-byte aligned.
// The micro-batcher's batches and pwaf_evaluate_one's single requests paid ~25 small copies from pageable memory (each a blocking staged
// copy) and two waits per batch; now: memcpy into page-locked memory, one copy in (in_bytes), one out (from at_counts on), one wait.
static constexpr size_t kPackMax = 1u << 20;
struct HostCol {  // one string column of a host batch: offsets[0] and offsets[n]
    bool present = false;
    uint32_t first = 0, last = 0;
};
struct PackedPlan {
    bool packable = true;  // else: the column-by-column path (the places below then mean nothing)
    size_t at_off[kMaxCols] = {}, at_data[kMaxCols] = {};
    size_t at_ip = 0, at_v6 = 0, at_port = 0, at_flags = 0, at_asn = 0, at_cc = 0;
    size_t at_counts = 0;  // (arrive zeroed with the inputs, return with the verdicts)
    size_t in_bytes = 0, at_out = 0;
    size_t at_geo = 0, at_route = 0;  // (return with the verdicts)
    size_t need = 0;
};
inline PackedPlan plan_packed(uint32_t n, uint32_t n_fields, const HostCol *col, bool has_asn, bool want_geo, bool want_route) {
    PackedPlan p;
    Layout pk;
    for (uint32_t f = 0; f < n_fields && p.packable; f++) {
        if (!col[f].present) continue;
        if (col[f].first != 0) { p.packable = false; break; }  // (a slab view of a larger arena keeps its positions: the column-by-column path)
        p.at_off[f] = pk.take((size_t)(n + 1) * 4);
        p.at_data[f] = pk.take((size_t)col[f].last + PWAF_ARENA_PAD);
        if (pk.size() > kPackMax) p.packable = false;
    }
    p.at_ip = pk.take((size_t)n * 16), p.at_v6 = pk.take(n), p.at_port = pk.take((size_t)n * 2), p.at_flags = pk.take(n);
    p.at_asn = has_asn ? pk.take((size_t)n * 4) : 0, p.at_cc = has_asn ? pk.take((size_t)n * 2) : 0;
    p.at_counts = pk.take(sizeof(pwaf_counts));
    p.in_bytes = pk.size();
    p.at_out = pk.take((size_t)n * sizeof(pwaf_verdict));
    p.at_geo = want_geo ? pk.take((size_t)n * sizeof(pwaf_geo)) : 0;
    p.at_route = want_route ? pk.take((size_t)n * 4) : 0;
    p.need = pk.size();
    p.packable = p.packable && p.need <= kPackMax;
    return p;
}

// ---- request records (pwaf_evaluate_records, pwaf_evaluate_records_device) ----

// rec_cols, the unpacked batch of m records: [column arenas, each with its PWAF_ARENA_PAD: records::place_columns] [ip] [v6] [port] [flags]
// [asn] [country] (the last two: records with GeoIP only)
struct RecordColsPlan {
    uint64_t col_at[kMaxCols] = {};
    bool geo = false;
    size_t c_ip = 0, c_v6 = 0, c_port = 0, c_flags = 0, c_asn = 0, c_cc = 0;
    size_t size = 0;
};
inline RecordColsPlan plan_record_cols(const uint64_t *totals, uint32_t n_cols, uint32_t m, bool has_geoip) {
    RecordColsPlan p;
    Layout cl;
    cl.used = (size_t)records::place_columns(totals, n_cols, p.col_at);
    p.geo = has_geoip;
    p.c_ip = cl.take((size_t)m * 16), p.c_v6 = cl.take(m), p.c_port = cl.take((size_t)m * 2), p.c_flags = cl.take(m);
    p.c_asn = has_geoip ? cl.take((size_t)m * 4) : 0, p.c_cc = has_geoip ? cl.take((size_t)m * 2) : 0;
    p.size = cl.size();
    return p;
}
// unpack_records_kernel's arguments for m records at `rec` (their offsets: rec_off) into the batch `p` places at `arena`; col_at / off:
// the column places and offsets where the DEVICE reads them
inline void fill_unpack_args(records::UnpackArgs &ua, const RecordColsPlan &p, const uint8_t *rec, const uint32_t *rec_off, uint32_t m, uint32_t n_cols, uint8_t *arena,
                             const uint64_t *col_at, const uint32_t *off, uint32_t off_stride) {
    ua.rec = rec;
    ua.rec_off = rec_off;
    ua.n = m;
    ua.n_cols = n_cols;
    ua.arena = arena;
    ua.col_at = col_at;
    ua.off = off;
    ua.off_stride = off_stride;
    ua.ip = arena + p.c_ip;
    ua.ip_is_v6 = arena + p.c_v6;
    ua.port = (uint16_t *)(arena + p.c_port);
    ua.flags = arena + p.c_flags;
    ua.asn = p.geo ? (uint32_t *)(arena + p.c_asn) : nullptr;
    ua.country = p.geo ? (uint16_t *)(arena + p.c_cc) : nullptr;
}

// rec_meta of records in HOST memory: [record offsets (relative to the span's start)] [column offsets, n + 1 per column] [column places]
// [counters] — up to here the host writes it (up_bytes) — [verdicts] [geo] [the records' bytes: `span`]. Counters, verdicts and geo come
// back in one copy.
struct HostRecMeta {
    size_t off_stride = 0;
    size_t at_recoff = 0, at_off = 0, at_colat = 0, at_counts = 0, up_bytes = 0, at_out = 0, at_geo = 0, at_rec = 0, need = 0;
};
inline HostRecMeta host_rec_meta(uint32_t n, uint32_t n_cols, bool want_geo, size_t span) {
    HostRecMeta p;
    Layout meta;
    p.off_stride = records::offsets_stride(n);
    p.at_recoff = meta.take((size_t)n * 4), p.at_off = meta.take(p.off_stride * 4 * n_cols), p.at_colat = meta.take((size_t)n_cols * 8);
    p.at_counts = meta.take(sizeof(pwaf_counts)), p.up_bytes = meta.size(), p.at_out = meta.take((size_t)n * sizeof(pwaf_verdict));
    p.at_geo = want_geo ? meta.take((size_t)n * sizeof(pwaf_geo)) : 0;
    p.at_rec = meta.take(span), p.need = meta.size();
    return p;
}
// rec_meta of records in DEVICE memory, from n and n_cols alone: [summary] [column places] [tile sums / bases, per column] [column
// offsets, n + 1 per column]
struct DeviceRecMeta {
    size_t off_stride = 0, tile_stride = 0;
    size_t at_sum = 0, at_colat = 0, at_tile = 0, at_off = 0, size = 0;
};
inline DeviceRecMeta device_rec_meta(uint32_t n, uint32_t n_cols) {
    DeviceRecMeta p;
    Layout meta;
    p.off_stride = records::offsets_stride(n), p.tile_stride = ((size_t)records::scan_tiles(n) + 31) & ~(size_t)31;
    p.at_sum = meta.take(sizeof(records::ScanSummary)), p.at_colat = meta.take((size_t)n_cols * 8), p.at_tile = meta.take(p.tile_stride * 8 * n_cols);
    p.at_off = meta.take(p.off_stride * 4 * n_cols);
    p.size = meta.size();
    return p;
}

}  // namespace pwaf
#pragma GCC visibility pop
