// records_scan.hip — pwaf_evaluate_records_device's validation and column offsets: what records::validate and records::column_offsets do
// on the host for pwaf_evaluate_records, for records that already lie in device memory. Three launches, reduce-then-scan (records.h has
// the scheme and the shared arithmetic); unpack_records_kernel (records.hip, unchanged) then reads what they wrote through UnpackArgs.
//
// No workgroup waits for another: no spin, no look-back, no "last workgroup done" counter. What one phase needs of all workgroups of the
// phase before (tile sums, column totals) crosses a launch boundary. That is also why the column places are computed by phase 3's first
// workgroup and not by phase 2: a column's workgroup there cannot see the other columns' totals without waiting for them.
//
// Reads of the caller's buffer: rec_off[i] for i < m, and record bytes that check_record has found inside [buf, buf + buf_bytes) — the
// head only once 36 bytes are known to be there, the lengths only once `size` is. A record that fails contributes no length, so nothing
// is read through it. Everything written is the engine's own (ScanArgs::off, tile, col_at, sum).
#include <hip/hip_runtime.h>

#include "colscan.h"
#include "records.h"

namespace pwaf {
namespace records {

const char *const kScanKernelNames[3] = {"records_check_kernel", "records_bases_kernel", "records_offsets_kernel"};

namespace {

static_assert(kScanTile % 64 == 0 && kScanStep % 64 == 0 && kScanTile <= 1024 && kScanStep <= 1024, "whole waves, one workgroup");

// Phase 1. One workgroup per tile, one record per lane.
__global__ __launch_bounds__(kScanTile) void records_check_kernel(ScanArgs a) {
    constexpr uint32_t W = kScanTile / 64;
    __shared__ uint64_t part[W][kMaxValues];  // per wave and column: the sum of its 64 records' lengths
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t m = records_in_call(a.n_rec, a.n);
    const uint64_t i = (uint64_t)blockIdx.x * kScanTile + tid;
    if ((uint64_t)blockIdx.x * kScanTile >= m) return;  // (the grid is sized from n: the host does not know m)
    const uint32_t geo0 = first_geo(a.buf, a.buf_bytes, a.rec_off[0]);
    const bool live = i < m;
    uint32_t nv = 0;
    const uint8_t *rec = a.buf;
    uint64_t key = kNoFailure;
    if (live) {
        const uint32_t o = a.rec_off[i];
        const int c = scan_check(a.buf, a.buf_bytes, o, a.n_cols, geo0, &nv);
        if (c != kOk) key = fail_key((uint32_t)i, c);  // (nv == 0: nothing is read through a record that failed)
        rec = a.buf + o;
    }
    if (__ballot(key != kNoFailure)) {
        key = wave_min(key);
        if (lane == 0) atomicMin((unsigned long long *)&a.sum->key, (unsigned long long)key);
    }
    for (uint32_t f = 0; f < a.n_cols; f++) {
        const uint32_t len = scan_len(rec, nv, f);
        if (live) a.off[(size_t)f * a.off_stride + i + 1] = len;
        uint64_t s = 0;
        if (__ballot(len != 0)) s = wave_sum(len);  // (most header columns are empty for all 64 records)
        if (lane == 0) part[wave][f] = s;
    }
    __syncthreads();
    for (uint32_t f = tid; f < a.n_cols; f += kScanTile) {
        uint64_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; w++) s += part[w][f];
        a.tile[(size_t)f * a.tile_stride + blockIdx.x] = s;
    }
}

// Phase 2. One workgroup per column, kScanStep tiles a step, the carry in a register.
__global__ __launch_bounds__(kScanStep) void records_bases_kernel(ScanArgs a) {
    constexpr uint32_t W = kScanStep / 64;
    __shared__ uint64_t wsum[W];
    __shared__ uint32_t first_tile, first_rec;
    const uint32_t tid = threadIdx.x, f = blockIdx.x;
    const uint32_t m = records_in_call(a.n_rec, a.n), n_tiles = scan_tiles(m);
    uint64_t *const tile = a.tile + (size_t)f * a.tile_stride;
    if (tid == 0) first_tile = first_rec = 0xFFFFFFFFu;
    __syncthreads();
    uint64_t carry = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += kScanStep) {
        const uint32_t t = t0 + tid;
        const uint64_t x = t < n_tiles ? tile[t] : 0u;
        uint64_t total;
        const uint64_t incl = carry + block_scan<W>(x, wsum, &total);
        if (t < n_tiles) {
            tile[t] = incl - x;
            if (column_too_big(incl) && !column_too_big(incl - x)) first_tile = t;  // (the totals only grow: one tile crosses the limit)
        }
        carry += total;
    }
    if (tid == 0) a.sum->totals[f] = carry;
    __syncthreads();
    const uint32_t ft = first_tile;
    if (ft == 0xFFFFFFFFu) return;
    // the record inside that tile at which the column crosses the limit: validate() reports kColumnTooBig there
    uint64_t run = tile[ft];
    for (uint32_t r0 = 0; r0 < kScanTile; r0 += kScanStep) {
        const uint64_t i = (uint64_t)ft * kScanTile + r0 + tid;
        const uint64_t x = i < m ? a.off[(size_t)f * a.off_stride + i + 1] : 0u;
        uint64_t total;
        const uint64_t incl = run + block_scan<W>(x, wsum, &total);
        if (column_too_big(incl) && !column_too_big(incl - x)) first_rec = (uint32_t)i;
        run += total;
    }
    __syncthreads();
    if (tid == 0 && first_rec != 0xFFFFFFFFu) atomicMin((unsigned long long *)&a.sum->key, (unsigned long long)fail_key(first_rec, kColumnTooBig));
}

// Phase 3. One workgroup per tile; a wave takes whole columns, 64 records at a time, so no two waves share anything.
__global__ __launch_bounds__(kScanTile) void records_offsets_kernel(ScanArgs a) {
    constexpr uint32_t W = kScanTile / 64;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t m = records_in_call(a.n_rec, a.n);
    const uint64_t key = a.sum->key;
    if (blockIdx.x == 0 && tid == 0) {
        a.sum->m = m;
        a.sum->has_geoip = m ? first_geo(a.buf, a.buf_bytes, a.rec_off[0]) : 0u;
        a.sum->bad_off = key != kNoFailure ? a.rec_off[key_index(key)] : 0u;
        a.sum->reserved = 0;
        place_columns(a.sum->totals, a.n_cols, a.col_at);
    }
    if (key != kNoFailure || (uint64_t)blockIdx.x * kScanTile >= m) return;  // (a refused call: nobody reads the offsets)
    for (uint32_t f = wave; f < a.n_cols; f += W) {
        uint32_t *const off = a.off + (size_t)f * a.off_stride;
        uint32_t carry = (uint32_t)a.tile[(size_t)f * a.tile_stride + blockIdx.x];  // (a valid call: every total is below 2^32)
        if (blockIdx.x == 0 && lane == 0) off[0] = 0;
#pragma unroll
        for (uint32_t c = 0; c < W; c++) {
            const uint64_t i = (uint64_t)blockIdx.x * kScanTile + c * 64u + lane;
            const uint32_t x = wave_scan(i < m ? off[i + 1] : 0u, lane);
            if (i < m) off[i + 1] = carry + x;
            carry += __shfl(x, 63, 64);
        }
    }
}

}  // namespace

int launch_scan_records(int phase, const ScanArgs &a, void *stream) {
    if (a.n == 0 || a.n_cols == 0 || a.n_cols > kMaxValues || a.tile_stride < scan_tiles(a.n)) return -1;
    const hipStream_t s = (hipStream_t)stream;
    if (phase == 1) hipLaunchKernelGGL(records_check_kernel, dim3(scan_tiles(a.n)), dim3(kScanTile), 0, s, a);
    else if (phase == 2) hipLaunchKernelGGL(records_bases_kernel, dim3(a.n_cols), dim3(kScanStep), 0, s, a);
    else if (phase == 3) hipLaunchKernelGGL(records_offsets_kernel, dim3(scan_tiles(a.n)), dim3(kScanTile), 0, s, a);
    else return -1;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace records
}  // namespace pwaf

// TEST HOOK: the shape of the scan, so that tests place their sizes on its real boundaries
extern "C" int pwaf_records_scan_shape(uint32_t out[4]) {
    if (!out) return PWAF_E_INVALID_ARG;
    out[0] = pwaf::records::kScanTile;
    out[1] = pwaf::records::kScanStep;
    out[2] = out[3] = 0;
    return PWAF_OK;
}
