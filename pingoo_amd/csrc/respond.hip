// respond.hip — pwaf_respond and pwaf_respond_one (include/pwaf.h): which response each request of a batch gets, and the ordered lists of
// request indices by kind of response that the follow-up services take, with the three kernels for a batch in device memory.
// csrc/respond.h holds the decision table, the scan's arithmetic and the HOST mode.
//
// One 64-byte memset and at most three launches, reduce-then-scan over tiles of kTile requests, as powbody.hip and derive.hip. No workgroup
// waits for another: no spin, no look-back, no cooperative launch; what one phase needs of all workgroups of the phase before crosses a
// launch boundary. The launch geometry depends on n alone.
//   respond_classify_kernel  one request per lane, one tile per workgroup. Coalesced loads of the 8-byte verdict, the status byte and the
//                            route word; only a lane whose action is BYPASS (and whose path has the shortest literal's length) reads its
//                            path, two 16-byte loads at the path's own alignment. One 8-byte store of the response. Per list one ballot
//                            per wave, the waves' population counts summed into the tile's word; the nine kinds counted the same way and
//                            added, one atomic per workgroup and non-zero kind, to the counters the memset zeroed.
//   respond_base_kernel      one workgroup: per list the tile counts -> exclusive bases, kStep tiles a step; writes every *n and the counts.
//   respond_scatter_kernel   one workgroup per tile: re-reads the kind bytes, ballots again and stores idx[base + rank] = i below cap.
//                            Not launched when no list has room for an entry.
#include <hip/hip_runtime.h>

#include <string>

#include "colscan.h"
#include "respond.h"

namespace pwaf {
namespace respond {
namespace {

static_assert(kTile % 64 == 0 && kStep % 64 == 0 && kTile <= 1024 && kStep <= 1024 && kTile >= 64, "whole waves");
constexpr uint32_t kNoKind = 0xFFu;  // a lane behind the batch's end

// the lanes of the wave below this one
__device__ __forceinline__ uint32_t rank_below(uint64_t ballot, uint32_t lane) { return (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull)); }

// Phase 1. Workgroup g decides the requests of tile g.
__global__ __launch_bounds__(kTile) void respond_classify_kernel(Args a) {
    constexpr uint32_t W = kTile / 64;
    __shared__ uint32_t wlist[W][PWAF_RESP_MAX_LISTS];  // per wave: the members of each list
    __shared__ uint32_t wkind[W][PWAF_RESP_KINDS];      // per wave: the requests of each kind
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t i64 = (uint64_t)blockIdx.x * kTile + tid;
    const uint32_t kind = i64 < a.n ? respond_request<Padded>(a, (uint32_t)i64) : kNoKind;
    const bool live = kind != kNoKind;
#pragma unroll
    for (uint32_t l = 0; l < PWAF_RESP_MAX_LISTS; l++) {
        const uint32_t c = l < a.n_lists ? (uint32_t)__popcll(__ballot(live && member(a.kinds[l], kind))) : 0u;
        if (lane == 0) wlist[wave][l] = c;
    }
#pragma unroll
    for (uint32_t k = 0; k < PWAF_RESP_KINDS; k++) {
        const uint32_t c = (uint32_t)__popcll(__ballot(kind == k));
        if (lane == 0) wkind[wave][k] = c;
    }
    __syncthreads();
    if (tid < a.n_lists) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; w++) s += wlist[w][tid];
        a.tile[(size_t)tid * tile_stride(a.n) + blockIdx.x] = s;
    }
    if (tid >= 64u && tid < 64u + PWAF_RESP_KINDS) {  // (another wave than the lists': the two tails run side by side)
        const uint32_t k = tid - 64u;
        uint32_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < W; w++) s += wkind[w][k];
        if (s) atomicAdd(a.kcount + k, s);
    }
}

// Phase 2. One workgroup; per list kStep tiles a step, the carry in a register.
__global__ __launch_bounds__(kStep) void respond_base_kernel(Args a) {
    constexpr uint32_t W = kStep / 64;
    __shared__ uint64_t wsum[W];
    const uint32_t tid = threadIdx.x;
    const uint32_t nt = tiles(a.n);
#pragma unroll
    for (uint32_t l = 0; l < PWAF_RESP_MAX_LISTS; l++) {  // (a static index into the argument block)
        if (l >= a.n_lists) break;
        const uint64_t total = scan_tile_bases<W>(a.tile + (size_t)l * tile_stride(a.n), nt, wsum);
        if (tid == 0) *a.cnt[l] = (uint32_t)total;  // (at most n)
    }
    if (a.counts && tid < PWAF_RESP_KINDS) a.counts[tid] = a.kcount[tid];
}

// Phase 3. Workgroup g places the members of tile g.
__global__ __launch_bounds__(kTile) void respond_scatter_kernel(Args a) {
    constexpr uint32_t W = kTile / 64;
    __shared__ uint32_t wlist[W][PWAF_RESP_MAX_LISTS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t i64 = (uint64_t)blockIdx.x * kTile + tid;
    const uint32_t i = (uint32_t)i64;
    const uint32_t kind = i64 < a.n ? a.out[i].kind : kNoKind;
    const bool live = kind != kNoKind;
    uint64_t ballot[PWAF_RESP_MAX_LISTS];
#pragma unroll
    for (uint32_t l = 0; l < PWAF_RESP_MAX_LISTS; l++) {
        ballot[l] = l < a.n_lists ? __ballot(live && member(a.kinds[l], kind)) : 0ull;
        if (lane == 0) wlist[wave][l] = (uint32_t)__popcll(ballot[l]);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t l = 0; l < PWAF_RESP_MAX_LISTS; l++) {
        if (l >= a.n_lists || !((ballot[l] >> lane) & 1ull)) continue;
        uint64_t at = a.tile[(size_t)l * tile_stride(a.n) + blockIdx.x] + rank_below(ballot[l], lane);
#pragma unroll
        for (uint32_t w = 0; w < W; w++) at += w < wave ? wlist[w][l] : 0u;
        if (at < a.cap[l]) a.idx[l][at] = i;
    }
}

}  // namespace

int launch_respond(const Args &a, void *stream) {
    if (!a.kcount || !a.tile || a.n_lists > PWAF_RESP_MAX_LISTS) return -1;
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t nt = tiles(a.n);
    if (hipMemsetAsync(a.kcount, 0, (size_t)kCountWords * 4u, s) != hipSuccess) return -1;
    if (nt && launch_args(respond_classify_kernel, nt, kTile, a, s)) return -1;
    if ((a.n_lists || a.counts) && launch_args(respond_base_kernel, 1, kStep, a, s)) return -1;
    bool room = false;
    for (uint32_t l = 0; l < a.n_lists; l++) room = room || (a.cap[l] && a.kinds[l]);
    if (nt && room && launch_args(respond_scatter_kernel, nt, kTile, a, s)) return -1;
    return 0;
}

}  // namespace respond
}  // namespace pwaf

extern "C" size_t pwaf_respond_scratch_bytes(uint32_t n) { return pwaf::respond::scratch_bytes(n); }

extern "C" int pwaf_respond(const pwaf_batch *in, const pwaf_verdict *verdicts, const uint8_t *cookie_status, const uint32_t *route, pwaf_response *out, uint64_t *counts,
                            const pwaf_resp_list *lists, uint32_t n_lists, void *scratch, size_t scratch_bytes, void *stream) {
    namespace R = pwaf::respond;
    using pwaf::fail;
    if (!in || !verdicts || !out) return fail(PWAF_E_INVALID_ARG, "pwaf_respond: NULL argument");
    if (int rc = pwaf::check_batch_header(in)) return rc;
    const pwaf_strcol &path = in->field[PWAF_FIELD_PATH];
    if (in->n && (!path.data || !path.offsets)) return fail(PWAF_E_INVALID_ARG, "pwaf_respond: pwaf_batch path column is NULL");
    if (n_lists > PWAF_RESP_MAX_LISTS) return fail(PWAF_E_INVALID_ARG, "pwaf_respond: more than PWAF_RESP_MAX_LISTS lists");
    if (n_lists && !lists) return fail(PWAF_E_INVALID_ARG, "pwaf_respond: lists is NULL with n_lists != 0");
    R::Args a{};
    for (uint32_t l = 0; l < n_lists; l++) {
        const pwaf_resp_list &li = lists[l];
        const std::string which = "pwaf_respond: list " + std::to_string(l);
        if (!li.idx && li.cap) return fail(PWAF_E_INVALID_ARG, which + ": idx is NULL with cap != 0");
        if (!li.n) return fail(PWAF_E_INVALID_ARG, which + ": n is NULL");
        if (li.kinds >> PWAF_RESP_KINDS) return fail(PWAF_E_INVALID_ARG, which + ": kinds has a bit at or above PWAF_RESP_KINDS");
        a.kinds[l] = li.kinds, a.cap[l] = li.cap, a.idx[l] = li.idx, a.cnt[l] = li.n;
    }
    a.path = path, a.n = in->n, a.n_lists = n_lists, a.verdicts = verdicts, a.status = cookie_status, a.route = route, a.out = out, a.counts = counts;
    if (in->memory == PWAF_MEM_HOST) {
        uint32_t bad = 0, why = 0;
        if (!R::respond_host(a, &bad, &why)) {
            static const char *const kWhy[3] = {"an action above 3", "a cookie status above 3", "path offsets decrease"};
            return fail(PWAF_E_BATCH, "pwaf_respond: request " + std::to_string(bad) + ": " + kWhy[why]);
        }
        return PWAF_OK;
    }
    if (int rc = pwaf::check_scratch("pwaf_respond", scratch, scratch_bytes, R::scratch_bytes(in->n), "pwaf_respond_scratch_bytes(n)")) return rc;
    static_assert(sizeof(R::Args) <= 4096, "Args travels in the kernel argument block");
    R::scratch_layout(a, scratch);
    if (R::launch_respond(a, stream)) return fail(PWAF_E_DEVICE, "pwaf_respond: the memset or a kernel launch failed");
    return PWAF_OK;
}

extern "C" int pwaf_respond_one(const pwaf_verdict *verdict, uint8_t cookie_status, int has_route, uint32_t route, const char *path, uint32_t path_len, pwaf_response *out) {
    namespace R = pwaf::respond;
    using pwaf::fail;
    if (!verdict || !out || (path_len && !path)) return fail(PWAF_E_INVALID_ARG, "pwaf_respond_one: NULL argument");
    if (verdict->action > 3u) return fail(PWAF_E_BATCH, "pwaf_respond_one: an action above 3");
    if (cookie_status > 3u) return fail(PWAF_E_BATCH, "pwaf_respond_one: a cookie status above 3");
    const R::Decision d = R::decide(verdict->action, verdict->rule_idx, cookie_status, has_route != 0, has_route ? route : PWAF_ROUTE_NONE, R::Exact{(const uint8_t *)path}, path_len);
    out->kind = (uint8_t)d.kind, out->pad[0] = out->pad[1] = out->pad[2] = 0, out->arg = d.arg;
    return PWAF_OK;
}

// TEST HOOK: the shape of the scan, so that tests place their sizes on its real boundaries
extern "C" int pwaf_respond_scan_shape(uint32_t out[4]) {
    if (!out) return PWAF_E_INVALID_ARG;
    out[0] = pwaf::respond::kTile;
    out[1] = pwaf::respond::kStep;
    out[2] = PWAF_RESP_MAX_LISTS;
    out[3] = PWAF_RESP_KINDS;
    return PWAF_OK;
}
