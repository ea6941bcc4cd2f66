// derive.hip — pwaf_derive_batch (include/pwaf.h): the derived host, path and User-Agent columns of a raw batch, with its three kernels for
// a batch in device memory. csrc/derive.h holds what a request costs (the kept slice of a value), the scan's arithmetic and the HOST mode.
//
// Three launches, reduce-then-scan over tiles of kTile requests, as records_scan.hip. The base and the copy kernel keep their own step loop
// and copy loop, which colscan.h has as scan_tile_bases and copy_wave_range (powbody.hip uses those): written on them the three launches
// measured 1.1 % slower on the MI355X. No workgroup waits for another: no spin, no
// look-back, no cooperative launch; what one phase needs of all workgroups of the phase before crosses a launch boundary.
//   derive_span_kernel  one request per lane: the kept slice of its three values (16-byte loads over the whitespace runs and the trailing
//                       slashes, then the at most 256 kept bytes of a header value). Reads the raw columns, the URI hosts and the present
//                       bytes; writes each kept length one slot up in out[c].offsets, where the kept bytes of the host and the User-Agent
//                       begin (scratch `from`) and a 64-bit sum per tile and column (scratch `tile`).
//   derive_base_kernel  one workgroup per column: tile sums -> exclusive bases, kStep tiles a step; slot n_tiles: the column's total.
//   derive_copy_kernel  one workgroup per tile. Per column a wave rescans its 64 lengths from the tile's base, in place, and copies: its
//                       requests' kept bytes are ONE contiguous range of the output, which the lanes take 16 aligned output bytes at a time.
//                       A lane finds the request holding its chunk's first byte by a search in the wave's offsets (LDS), gathers the chunk
//                       from the runs it crosses (one 16-byte load per run at the run's own alignment, cut and shifted into place) and
//                       stores it: one aligned 16-byte store when the whole chunk is the wave's and lies below
//                       cap, else byte by byte — a neighbouring wave owns the rest of a boundary chunk. The last tile writes the pads,
//                       the first offsets[0] and stats. Nothing is stored at or beyond cap.
#include <hip/hip_runtime.h>

#include <string>

#include "colscan.h"
#include "derive.h"

namespace pwaf {
namespace derive {
namespace {

static_assert(kTile % 64 == 0 && kStep % 64 == 0 && kTile <= 1024 && kStep <= 1024 && kCopyGroup == kTile, "whole waves, one workgroup per tile");

// Phase 1. One workgroup per tile, one request per lane.
__global__ __launch_bounds__(kTile) void derive_span_kernel(Args a) {
    constexpr uint32_t W = kTile / 64;
    __shared__ uint64_t part[W][kColumns];  // per wave and column: the sum of its 64 requests' kept lengths
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t i64 = (uint64_t)blockIdx.x * kTile + tid;
    const bool live = i64 < a.n;
    const uint32_t i = (uint32_t)i64;
    uint32_t len[kColumns] = {0, 0, 0};
    if (live) {
        const uint32_t p = present_of(a, i);
#pragma unroll
        for (uint32_t c = 0; c < kColumns; c++) {
            const Kept k = kept_of(a, c, i, p);
            len[c] = k.len;
            a.off[c][(size_t)i + 1] = k.len;
            if (c != kPath) a.from[(size_t)(c == kUserAgent) * a.n + i] = k.at;
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < kColumns; c++) {
        const uint64_t s = wave_sum(len[c]);
        if (lane == 0) part[wave][c] = s;
    }
    __syncthreads();
    if (tid < kColumns) {
        uint64_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; w++) s += part[w][tid];
        a.tile[(size_t)tid * a.tile_stride + blockIdx.x] = s;
    }
}

// Phase 2. One workgroup per column, kStep tiles a step, the carry in a register.
__global__ __launch_bounds__(kStep) void derive_base_kernel(Args a) {
    constexpr uint32_t W = kStep / 64;
    __shared__ uint64_t wsum[W];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nt = tiles(a.n);
    uint64_t *const tile = a.tile + (size_t)blockIdx.x * a.tile_stride;
    uint64_t carry = 0;
    for (uint32_t t0 = 0; t0 < nt; t0 += kStep) {
        const uint32_t t = t0 + tid;  // (nt is at most 2^16: no wrap)
        const uint64_t x = t < nt ? tile[t] : 0u;
        uint64_t incl = wave_scan(x, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint64_t all = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; w++) {
            const uint64_t s = wsum[w];
            if (w < wave) incl += s;
            all += s;
        }
        if (t < nt) tile[t] = carry + incl - x;
        carry += all;
        __syncthreads();  // (wsum is rewritten by the next step)
    }
    if (tid == 0) tile[nt] = carry;
}

// Phase 3. One workgroup per tile (one workgroup when n == 0); a wave shares nothing with the others but the sums of their lengths.
__global__ __launch_bounds__(kCopyGroup) void derive_copy_kernel(Args a) {
    constexpr uint32_t W = kCopyGroup / 64;
    __shared__ uint32_t wtotal[kColumns][W];   // the kept bytes of each wave's 64 requests
    __shared__ uint32_t woff[W][65];           // where request j of the wave begins inside the wave's range; [64]: the range's length
    __shared__ const uint8_t *wsrc[W][64];     // its first kept byte in the source arena
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nt = tiles(a.n);
    const uint64_t i64 = (uint64_t)blockIdx.x * kTile + tid;
    const bool live = i64 < a.n;
    const uint32_t i = (uint32_t)i64;
    const uint32_t present = live ? present_of(a, i) : 0u;
    uint32_t len[kColumns], incl[kColumns];
#pragma unroll
    for (uint32_t c = 0; c < kColumns; c++) {
        len[c] = live ? a.off[c][(size_t)i + 1] : 0u;
        incl[c] = wave_scan(len[c], lane);  // (a wave's kept bytes are below 2^32: every column's total is)
        if (lane == 63) wtotal[c][wave] = incl[c];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t c = 0; c < kColumns; c++) {
        uint8_t *const data = a.data[c];
        const uint64_t cap = a.cap[c];
        uint64_t base = a.tile[(size_t)c * a.tile_stride + blockIdx.x];  // the wave's first output byte
        for (uint32_t w = 0; w < wave; w++) base += wtotal[c][w];
        const uint32_t range = wtotal[c][wave];
        if (live) a.off[c][(size_t)i + 1] = (uint32_t)(base + incl[c]);
        if (blockIdx.x == 0 && tid == 0 && a.off[c]) a.off[c][0] = 0;
        if (range == 0) continue;  // (wave-uniform: a wave whose requests all derive to "")
        woff[wave][lane] = incl[c] - len[c];
        if (lane == 63) woff[wave][64] = range;
        const uint8_t *s = nullptr;
        if (len[c]) s = source_of(a, c, present) + (c == kPath ? a.raw[kPath].offsets[i] : a.from[(size_t)(c == kUserAgent) * a.n + i]);
        wsrc[wave][lane] = s;
        wave_sync();
        // the aligned 16-byte chunks of the output that hold a byte of [base, base + range)
        const uint64_t end = base + range;
        for (uint64_t ck = (base >> 4) + lane; ck * 16u < end; ck += 64) {
            const uint64_t p0 = ck * 16u, lo64 = p0 > base ? p0 : base, hi64 = p0 + 16u < end ? p0 + 16u : end;
            const uint32_t lo = (uint32_t)(lo64 - base), hi = (uint32_t)(hi64 - base), shift = (uint32_t)(lo64 - p0);  // inside the range; the chunk's first own byte
            uint32_t l = 0, h = 64;  // woff[l] <= lo < woff[h]: request l holds byte lo (and is not empty)
            while (h - l > 1) {
                const uint32_t mid = (l + h) >> 1;
                if (woff[wave][mid] <= lo) l = mid;
                else h = mid;
            }
            uint32_t k = l, first = woff[wave][k], next = woff[wave][k + 1];
            const uint8_t *src = wsrc[wave][k];  // byte `first` of the range is src[0]
            unsigned __int128 acc = 0;
            for (uint32_t p = lo; p < hi;) {
                while (p >= next) {  // (p < hi <= range == woff[64]: k stays below 64)
                    k++;
                    first = next;
                    next = woff[wave][k + 1];
                    src = wsrc[wave][k];
                }
                const uint32_t run = (next < hi ? next : hi) - p;
                unsigned __int128 v;
                memcpy(&v, src + (p - first), 16);  // may pass the value's end by fewer than 16 bytes: inside the arena or its pad
                if (run < 16u) v &= ((unsigned __int128)1 << (8u * run)) - 1u;
                acc |= v << (8u * (p - lo + shift));
                p += run;
            }
            if (hi - lo == 16u && p0 + 16u <= cap) {
                uint4 q;
                memcpy(&q, &acc, 16);
                *reinterpret_cast<uint4 *>(data + p0) = q;
            } else {
                for (uint32_t b = shift; b < shift + (hi - lo); b++)
                    if (p0 + b < cap) data[p0 + b] = (uint8_t)(acc >> (8u * b));
            }
        }
        wave_sync();  // (woff and wsrc are rewritten for the next column)
    }
    if (blockIdx.x + 1 == gridDim.x && tid < PWAF_ARENA_PAD) {
#pragma unroll
        for (uint32_t c = 0; c < kColumns; c++) write_pad_byte(a.data[c], a.tile[(size_t)c * a.tile_stride + nt], a.cap[c], tid);
    }
    if (blockIdx.x == 0 && tid == 0) {
        uint64_t total[kColumns];
#pragma unroll
        for (uint32_t c = 0; c < kColumns; c++) total[c] = a.tile[(size_t)c * a.tile_stride + nt];
        fill_stats(a.stats, total, a.cap, a.n);
    }
}

}  // namespace

int launch_derive(int phase, const Args &a, void *stream) {
    if (a.n > kMaxRequests || a.tile_stride <= tiles(a.n) || !a.tile || !a.from) return -1;
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t nt = tiles(a.n);
    if (phase == 1) return nt ? launch_args(derive_span_kernel, nt, kTile, a, s) : 0;
    if (phase == 2) return launch_args(derive_base_kernel, kColumns, kStep, a, s);
    if (phase == 3) return launch_args(derive_copy_kernel, nt ? nt : 1u, kCopyGroup, a, s);
    return -1;
}

}  // namespace derive
}  // namespace pwaf

extern "C" size_t pwaf_derive_scratch_bytes(uint32_t n) { return pwaf::derive::scratch_bytes(n); }

extern "C" int pwaf_derive_batch(const pwaf_batch *raw, const pwaf_raw_columns *extra, pwaf_derived_col out[3], pwaf_derive_stats *stats, void *scratch,
                                 size_t scratch_bytes, void *stream) {
    namespace D = pwaf::derive;
    using pwaf::fail;
    static const char *const kName[4] = {"host", "path", "User-Agent", "URI host"};
    static const uint32_t kField[D::kColumns] = {PWAF_FIELD_HOST, PWAF_FIELD_PATH, PWAF_FIELD_USER_AGENT};
    if (!raw || !out || !stats) return fail(PWAF_E_INVALID_ARG, "pwaf_derive_batch: NULL argument");
    if (int rc = pwaf::check_batch_header(raw)) return rc;
    if (extra && extra->struct_size != sizeof(pwaf_raw_columns)) return fail(PWAF_E_INVALID_ARG, "pwaf_raw_columns.struct_size mismatch");
    if (raw->n > D::kMaxRequests) return fail(PWAF_E_INVALID_ARG, "pwaf_derive_batch: more than 0xFFFFFFF0 / 256 requests (a derived column could pass 32 bits): split the batch");
    if ((uintptr_t)stats & 7u) return fail(PWAF_E_INVALID_ARG, "pwaf_derive_batch: stats is not 8-byte aligned");
    D::Args a{};
    a.n = raw->n;
    for (uint32_t c = 0; c < D::kColumns; c++) {
        const std::string col = std::string("pwaf_derive_batch: ") + kName[c];
        a.raw[c] = raw->field[kField[c]];
        if (a.n && (!a.raw[c].data || !a.raw[c].offsets)) return fail(PWAF_E_INVALID_ARG, col + " column of the raw batch is NULL");
        if (int rc = pwaf::check_derived_col(col + ": out", a.n, out[c])) return rc;
        a.data[c] = out[c].data, a.off[c] = out[c].offsets, a.cap[c] = out[c].cap;
    }
    if (extra) {
        if (extra->uri_host.data && extra->uri_host.offsets) a.uri_host = extra->uri_host;  // (either NULL: no request has one)
        a.present = extra->present;
    }
    a.stats = stats;
    if (raw->memory == PWAF_MEM_HOST) {
        uint32_t bad = 0, col = 0;
        if (!D::derive_host(a, &bad, &col)) return fail(PWAF_E_BATCH, "pwaf_derive_batch: request " + std::to_string(bad) + ": offsets decrease in the " + kName[col] + " column");
        return PWAF_OK;
    }
    if (int rc = pwaf::check_scratch("pwaf_derive_batch", scratch, scratch_bytes, D::scratch_bytes(a.n), "pwaf_derive_scratch_bytes(n)")) return rc;
    static_assert(sizeof(D::Args) <= 4096, "Args travels in the kernel argument block");
    D::scratch_layout(a, scratch);
    for (int phase = 1; phase <= 3; phase++)
        if (D::launch_derive(phase, a, stream)) return fail(PWAF_E_DEVICE, "pwaf_derive_batch: kernel launch failed");
    return PWAF_OK;
}

// TEST HOOK: the shape of the scan, so that tests place their sizes on its real boundaries
extern "C" int pwaf_derive_scan_shape(uint32_t out[4]) {
    if (!out) return PWAF_E_INVALID_ARG;
    out[0] = pwaf::derive::kTile;
    out[1] = pwaf::derive::kStep;
    out[2] = pwaf::derive::kCopyGroup;
    out[3] = 0;
    return PWAF_OK;
}
