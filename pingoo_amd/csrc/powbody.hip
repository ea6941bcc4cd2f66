// powbody.hip — pwaf_parse_pow_bodies and pwaf_parse_pow_body_one (include/pwaf.h): hash and nonce of proof-of-work request bodies, as
// pwaf_verify_pow reads them next on the same stream, with the three kernels for a batch in device memory. csrc/powbody.h holds the
// reader (D-B1 to D-B10), the scan's arithmetic and the HOST mode.
//
// At most one memset and three launches, reduce-then-scan over tiles of kTile requests, as derive.hip. No workgroup waits for another: no
// spin, no look-back, no cooperative launch; what one phase needs of all workgroups of the phase before crosses a launch boundary.
//   powbody_parse_kernel  one entry per lane, one tile of entries per workgroup (with a list: a bounded grid striding over the tiles). A
//                         lane reads its body left to right through 16-byte loads at the body's own alignment (six for a genuine body),
//                         decides it and writes the status, by request the hash row and the nonce's length one slot up in
//                         nonce->offsets, and where the nonce begins in the body arena (scratch `from`). Without a list the entries are
//                         the requests and the workgroup writes its tile's 64-bit sum; with one, the memset in front has zeroed every
//                         length and the base launch sums the tiles. Each workgroup writes its status counts to a slot of its own.
//   powbody_base_kernel   one workgroup: (with a list) each tile's sum, a wave a tile; tile sums -> exclusive bases, kStep tiles a step;
//                         slot tiles(n): the total. Sums the workgroups' status counts.
//   powbody_copy_kernel   one workgroup per tile: copy_wave_range (colscan.h) for one column, as derive_copy_kernel for three. A wave rescans its 64 lengths from the tile's base, in
//                         place, and copies its requests' nonces, ONE contiguous range of the output, 16 aligned output bytes at a time. The
//                         last tile writes the pad, the first offsets[0] and stats. Nothing is stored at or beyond cap.
#include <hip/hip_runtime.h>

#include <new>
#include <string>

#include "colscan.h"
#include "powbody.h"

namespace pwaf {
namespace powbody {
namespace {

static_assert(kTile % 64 == 0 && kStep % 64 == 0 && kTile <= 1024 && kStep <= 1024 && kCopyGroup == kTile, "whole waves, one workgroup per tile");

// Phase 1. One entry per lane; workgroup g takes the tiles g, g + gridDim.x, ... of the entries (without a list: tile g alone).
__global__ __launch_bounds__(kTile) void powbody_parse_kernel(Args a) {
    constexpr uint32_t W = kTile / 64;
    __shared__ uint64_t part[W];      // per wave: the sum of its 64 entries' nonce lengths
    __shared__ uint32_t wcount[W][3];  // per wave: OK / MALFORMED / UNDECIDED over all its tiles
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t m = selected(a);
    uint32_t count[3] = {0, 0, 0};
    uint64_t sum = 0;
    for (uint64_t e0 = (uint64_t)blockIdx.x * kTile; e0 < m; e0 += (uint64_t)gridDim.x * kTile) {
        const uint64_t e64 = e0 + tid;
        uint32_t st = PWAF_BODY_NONE, len = 0;
        if (e64 < m) {
            const uint32_t e = (uint32_t)e64, i = request_of(a, e);
            if (i < a.n) {
                const Body b = parse_entry<Padded>(a, e, i);
                a.from[i] = a.bodies.offsets[i] + b.nonce_at;
                st = b.status, len = b.nonce_len;
            } else {
                a.status[e] = PWAF_BODY_NONE;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) count[k] += (uint32_t)__popcll(__ballot(st == k + 1u));
        sum += len;
    }
    sum = wave_sum(sum);
    if (lane == 0) {
        part[wave] = sum;
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) wcount[wave][k] = count[k];
    }
    __syncthreads();
    if (tid < 3) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; w++) c += wcount[w][tid];
        a.count[(size_t)blockIdx.x * 4u + tid] = c;
    }
    if (tid == 3) {
        a.count[(size_t)blockIdx.x * 4u + 3u] = 0;
        if (!a.idx) {  // the entries are the requests: this workgroup's tile is tile blockIdx.x of the scan
            uint64_t s = 0;
#pragma unroll
            for (uint32_t w = 0; w < W; w++) s += part[w];
            a.tile[blockIdx.x] = s;
        }
    }
}

// Phase 2. One workgroup, kStep tiles a step, the carry in a register.
__global__ __launch_bounds__(kStep) void powbody_base_kernel(Args a) {
    constexpr uint32_t W = kStep / 64;
    __shared__ uint64_t wsum[W];
    __shared__ uint32_t csum[W][3];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nt = tiles(a.n);
    uint64_t *const tile = a.tile;
    if (a.idx) {  // a wave a tile: the sum of its requests' lengths (zero where the list names none)
        for (uint32_t t = wave; t < nt; t += W) {
            uint64_t s = 0;
#pragma unroll
            for (uint32_t k = 0; k < kTile; k += 64) {
                const uint64_t i = (uint64_t)t * kTile + k + lane;
                s += i < a.n ? a.off[i + 1] : 0u;
            }
            s = wave_sum(s);
            if (lane == 0) tile[t] = s;
        }
        __syncthreads();  // (the workgroup's own global writes are visible to it behind the barrier)
    }
    const uint64_t total = scan_tile_bases<W>(tile, nt, wsum);
    if (tid == 0) tile[nt] = total;
    // the status counts of the parse launch's workgroups -> slot 0
    uint32_t c[3] = {0, 0, 0};
    for (uint32_t g = tid; g < a.groups; g += kStep) {
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) c[k] += a.count[(size_t)g * 4u + k];
    }
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        const uint32_t s = (uint32_t)wave_sum(c[k]);
        if (lane == 0) csum[wave][k] = s;
    }
    __syncthreads();  // (every read of a.count above is done)
    if (tid < 3) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; w++) s += csum[w][tid];
        a.count[tid] = s;
    }
    if (tid == 3) a.count[3] = selected(a);
}

// Phase 3. One workgroup per tile (one workgroup when n == 0); a wave shares nothing with the others but the sums of their lengths.
__global__ __launch_bounds__(kCopyGroup) void powbody_copy_kernel(Args a) {
    constexpr uint32_t W = kCopyGroup / 64;
    __shared__ uint32_t wtotal[W];          // the nonce bytes of each wave's 64 requests
    __shared__ uint32_t woff[W][65];        // where request j of the wave begins inside the wave's range; [64]: the range's length
    __shared__ const uint8_t *wsrc[W][64];  // its nonce's first byte in the body arena
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nt = tiles(a.n);
    const uint64_t i64 = (uint64_t)blockIdx.x * kTile + tid;
    const bool live = i64 < a.n;
    const uint32_t i = (uint32_t)i64;
    const uint32_t len = live ? a.off[(size_t)i + 1] : 0u;
    const uint32_t incl = wave_scan(len, lane);  // (a wave's nonce bytes are below 2^32: the column's total is)
    if (lane == 63) wtotal[wave] = incl;
    __syncthreads();
    uint8_t *const data = a.data;
    const uint64_t cap = a.cap;
    const uint64_t total = a.tile[nt];
    uint64_t base = a.tile[blockIdx.x];  // the wave's first output byte
    for (uint32_t w = 0; w < wave; w++) base += wtotal[w];
    const uint32_t range = wtotal[wave];
    if (live) a.off[(size_t)i + 1] = (uint32_t)(base + incl);
    if (blockIdx.x == 0 && tid == 0 && a.off) a.off[0] = 0;
    if (range != 0) {  // (wave-uniform: a wave whose requests all have no nonce copies nothing)
        woff[wave][lane] = incl - len;
        if (lane == 63) woff[wave][64] = range;
        wsrc[wave][lane] = len ? a.bodies.data + a.from[i] : nullptr;
        wave_sync();
        copy_wave_range(data, cap, base, range, woff[wave], wsrc[wave], lane);
    }
    if (blockIdx.x + 1 == gridDim.x && tid < PWAF_ARENA_PAD) write_pad_byte(data, total, cap, tid);
    if (blockIdx.x == 0 && tid == 0) {
        const uint32_t count[4] = {a.count[0], a.count[1], a.count[2], a.count[3]};
        fill_stats(a.stats, total, cap, count);
    }
}

}  // namespace

int launch_parse_pow(const Args &a, void *stream) {
    if (a.n > kMaxRequests || !a.tile || !a.count || !a.from || a.groups != parse_groups(a.n, a.idx != nullptr, a.idx_cap) || a.groups > count_slots(a.n)) return -1;
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t nt = tiles(a.n);
    // with a list: the length of every request the list does not name (the parse launch overwrites those it names)
    if (a.idx && a.n && hipMemsetAsync(a.off, 0, ((size_t)a.n + 1u) * 4u, s) != hipSuccess) return -1;
    if (a.groups && launch_args(powbody_parse_kernel, a.groups, kTile, a, s)) return -1;
    if (launch_args(powbody_base_kernel, 1, kStep, a, s)) return -1;
    return launch_args(powbody_copy_kernel, nt ? nt : 1u, kCopyGroup, a, s);
}

}  // namespace powbody
}  // namespace pwaf

extern "C" size_t pwaf_parse_pow_bodies_scratch_bytes(uint32_t n) { return pwaf::powbody::scratch_bytes(n); }

extern "C" int pwaf_parse_pow_bodies(const pwaf_strcol *bodies, uint32_t n, uint32_t memory, const uint32_t *idx, uint32_t idx_cap, const uint32_t *n_idx, uint8_t *status,
                                     uint8_t *hash, pwaf_derived_col *nonce, pwaf_body_stats *stats, void *scratch, size_t scratch_bytes, void *stream) {
    namespace B = pwaf::powbody;
    using pwaf::fail;
    if (!bodies || !status || !hash || !nonce || !stats) return fail(PWAF_E_INVALID_ARG, "pwaf_parse_pow_bodies: NULL argument");
    if (memory != PWAF_MEM_HOST && memory != PWAF_MEM_DEVICE) return fail(PWAF_E_INVALID_ARG, "pwaf_parse_pow_bodies: memory is neither HOST nor DEVICE");
    if (int rc = pwaf::check_list("pwaf_parse_pow_bodies", idx, idx_cap, n_idx)) return rc;
    if (n > B::kMaxRequests)
        return fail(PWAF_E_INVALID_ARG, "pwaf_parse_pow_bodies: more than 0xFFFFFFF0 / PWAF_POW_BODY_MAX_BYTES requests (the nonce column could pass 32 bits): split the batch");
    if ((uintptr_t)stats & 7u) return fail(PWAF_E_INVALID_ARG, "pwaf_parse_pow_bodies: stats is not 8-byte aligned");
    if (n && (!bodies->data || !bodies->offsets)) return fail(PWAF_E_INVALID_ARG, "pwaf_parse_pow_bodies: the bodies column is NULL");
    if (int rc = pwaf::check_derived_col("pwaf_parse_pow_bodies: nonce", n, *nonce)) return rc;
    B::Args a{};
    a.bodies = *bodies, a.n = n, a.idx = idx, a.n_idx = n_idx, a.idx_cap = idx_cap, a.status = status, a.hash = hash;
    a.data = nonce->data, a.off = nonce->offsets, a.cap = nonce->cap, a.stats = stats;
    if (memory == PWAF_MEM_HOST) {
        uint32_t *from = n ? new (std::nothrow) uint32_t[n] : nullptr;
        if (n && !from) return fail(PWAF_E_NOMEM, "pwaf_parse_pow_bodies: out of memory");
        uint32_t bad = 0;
        const bool ok = B::parse_host(a, from, &bad);
        const uint32_t bad_request = ok ? 0u : idx ? idx[bad] : bad;
        delete[] from;
        if (!ok) return fail(PWAF_E_BATCH, "pwaf_parse_pow_bodies: entry " + std::to_string(bad) + " (request " + std::to_string(bad_request) + "): body offsets decrease");
        return PWAF_OK;
    }
    if (int rc = pwaf::check_scratch("pwaf_parse_pow_bodies", scratch, scratch_bytes, B::scratch_bytes(n), "pwaf_parse_pow_bodies_scratch_bytes(n)")) return rc;
    static_assert(sizeof(B::Args) <= 4096, "Args travels in the kernel argument block");
    B::scratch_layout(a, scratch);
    a.groups = B::parse_groups(n, idx != nullptr, idx_cap);
    if (B::launch_parse_pow(a, stream)) return fail(PWAF_E_DEVICE, "pwaf_parse_pow_bodies: a memset or a kernel launch failed");
    return PWAF_OK;
}

extern "C" int pwaf_parse_pow_body_one(const uint8_t *body, uint32_t len, uint8_t *status, uint8_t hash[32], uint32_t *nonce_at, uint32_t *nonce_len) {
    namespace B = pwaf::powbody;
    if (!status || !hash || !nonce_at || !nonce_len || (len && !body)) return pwaf::fail(PWAF_E_INVALID_ARG, "pwaf_parse_pow_body_one: NULL argument");
    const B::Body b = B::read_body(B::Exact{body}, len);
    *status = (uint8_t)b.status;
    memcpy(hash, b.hash, 32);
    *nonce_at = b.nonce_at, *nonce_len = b.nonce_len;
    return PWAF_OK;
}

// TEST HOOK: the shape of the scan, so that tests place their sizes on its real boundaries
extern "C" int pwaf_parse_pow_scan_shape(uint32_t out[4]) {
    if (!out) return PWAF_E_INVALID_ARG;
    out[0] = pwaf::powbody::kTile;
    out[1] = pwaf::powbody::kStep;
    out[2] = pwaf::powbody::kCopyGroup;
    out[3] = pwaf::powbody::kMinGroups;
    return PWAF_OK;
}
