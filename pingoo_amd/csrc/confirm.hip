// confirm.hip — the confirm tier (confirm.h; program.h: ConfirmTable): confirm_kernel settles the literal patterns of the flagged
// chunks the filter stage listed, and appends what only a DFA can settle to the pass's walk list. Pipeline overview: kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "confirm.h"
#include "hitrec.h"
#include "kernels.h"
#include "wave.h"

namespace pwaf {

__global__ __launch_bounds__(256) void confirm_plan_kernel(ConfirmTableDev b, uint32_t *plan /* [count + 1] */) {
    __shared__ uint32_t part[256];
    const uint32_t t = threadIdx.x;
    uint32_t items = 0;
    if (t < b.count) {
        const ConfirmArgs *pa = &b.c[t];
        const bool dense = pa->dense_flag != nullptr && *pa->dense_flag > pa->dense_thresh;  // (walked whole this batch: nothing to confirm)
        items = dense ? 0u : (min(*pa->pair_count, pa->pair_cap) + kConfirmThreads - 1) / kConfirmThreads;
    }
    part[t] = items;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    if (t < b.count) plan[t] = part[t] - items;
    if (t == 0) plan[b.count] = part[255];
}

// A literal atom confirmed for request r, merged into its hit record. Several lanes — other flagged chunks of the same request, in other
// workgroups on other XCDs — may be merging at once, so every access to the shared words is a read-modify-write atomic (performed at
// the device's coherence point; a returned atomic has completed when its value arrives, which orders an overflow entry's words before
// the compare-and-swap that publishes it): no fences — an agent-scope fence writes back and invalidates the whole L2, and two per hit
// took this kernel from 0.3 to 1.5 ms and its neighbours with it. An overflow chain grows like a lock-free stack (entries allocated for
// an attempt that lost its compare-and-swap are leaked: rare, and the pool is sized per batch).
__device__ __noinline__ void merge_atom(PoolEntry *pool, uint32_t *pool_count, uint32_t *status, uint32_t pool_cap, uint32_t *rec, uint32_t atom) {
    auto rmw_read = [](uint32_t *p) { return atomicOr(p, 0u); };
    auto publish = [&](uint32_t idx, uint32_t at, uint32_t next) {
        const uint32_t t0 = atomicExch(&pool[idx].atom, at), t1 = atomicExch(&pool[idx].next, next);
        asm volatile("" ::"v"(t0), "v"(t1));  // (both have been performed before anything below is issued)
    };
    uint32_t old = rmw_read(rec);
    for (;;) {
        uint32_t upd;
        const uint32_t x = atom + 1u;
        if (!(old & REC_OVERFLOW)) {
            const uint32_t a0 = old & 0x7FFFu, a1 = (old >> 15) & 0x7FFFu;
            if (a0 == x || a1 == x) return;
            if (a0 == 0u) upd = old | x;
            else if (a1 == 0u) upd = old | (x << 15);
            else {  // a third atom: the record becomes a chain of all three
                const uint32_t idx = atomicAdd(pool_count, 3u);
                if (idx + 3u > pool_cap) { atomicOr(status, 1u); return; }  // (the host runs the batch again with the pool the allocator asked for)
                publish(idx, a0 - 1u, kNone);
                publish(idx + 1u, a1 - 1u, idx);
                publish(idx + 2u, atom, idx + 1u);
                upd = REC_OVERFLOW | (idx + 2u);
            }
        } else {
            const uint32_t head = old & ~REC_OVERFLOW;
            for (uint32_t i = head; i != kNone; i = rmw_read(&pool[i].next))
                if (rmw_read(&pool[i].atom) == atom) return;
            const uint32_t idx = atomicAdd(pool_count, 1u);
            if (idx >= pool_cap) { atomicOr(status, 1u); return; }
            publish(idx, atom, head);
            upd = REC_OVERFLOW | idx;
        }
        const uint32_t seen = atomicCAS(rec, old, upd);
        if (seen == old) return;
        old = seen;
    }
}

// One lane per (request, flagged chunk) pair; a persistent grid over device-computed work items (one workgroup's worth of pairs of
// one pass each), like the list scan: consecutive items are mostly of one pass, whose tables are staged in LDS once — the filter
// table and the confirm head table (16 KiB each) and, when they fit kConfirmPoolBytes, the comparison tables (entries, value / mask
// bytes, classes); a pass whose tables do not fit reads them from the L2-resident originals through the same (generic) pointers.
//
// Why pairs. A request-per-lane version (this round's first) looped over the request's flagged chunks, their completed windows and
// the windows' entries: 64 lanes in lockstep take the PRODUCT of each level's longest trip, every trip a chain of memory round
// trips, and a wave is as slow as its unluckiest request — measured 0.32 - 0.64 ms for the ~350k benign candidates of a 10M-request
// batch and 4 - 13 ms for the hostile stream's 11M (profiles/r4_confirm_v1_*). A pair is one chunk of text and the one or two
// windows that completed in it: the same small amount of work in every lane, and nothing to do afterwards unless something was
// confirmed.
__global__ __launch_bounds__(kConfirmThreads, 8) void confirm_kernel(ConfirmTableDev b, const uint32_t *plan) {
    __shared__ uint32_t head[kFilterEntries], ftab[kFilterEntries];  // the confirm table's head words; the pass's filter table
    __shared__ uint32_t pool[kConfirmPoolBytes / 4];                 // entries | bytes | classes of the pass (when they fit)
    constexpr uint32_t kConfirmQueue = 1024;
    __shared__ uint32_t app_cnt, app_base, app_queue[kConfirmQueue];  // the workgroup's walk-list appends of the current pass
    __builtin_amdgcn_s_setprio(3);
    if (threadIdx.x == 0) app_cnt = 0;
    const uint32_t total = plan[b.count];
    const uint32_t it0 = (uint32_t)((uint64_t)total * blockIdx.x / gridDim.x), it1 = (uint32_t)((uint64_t)total * (blockIdx.x + 1) / gridDim.x);
    for (uint32_t it = it0; it < it1;) {
        uint32_t ps = 0;
        for (uint32_t lo = 0, hi = b.count; lo + 1 < hi;) {  // the pass of item `it`: the last p with plan[p] <= it (uniform)
            const uint32_t mid = (lo + hi) >> 1;
            if (plan[mid] <= it) lo = mid;
            else hi = mid;
            ps = lo;
        }
        const uint32_t first_item = plan[ps], it_end = min(it1, plan[ps + 1]);
        const ConfirmArgs a = load_descriptor(&b.c[ps]);
        __syncthreads();  // (every wave is done with the previous pass's tables)
        {
            // 16 bytes per lane and load (two 16 KiB tables)
            const uint4 *sh = reinterpret_cast<const uint4 *>(a.c_head), *sf = reinterpret_cast<const uint4 *>(a.ftable);
            constexpr uint32_t kPer = kFilterEntries / 4 / kConfirmThreads;
            uint4 vh[kPer], vf[kPer];
#pragma unroll
            for (uint32_t q = 0; q < kPer; q++) { vh[q] = sh[q * kConfirmThreads + threadIdx.x]; vf[q] = sf[q * kConfirmThreads + threadIdx.x]; }
#pragma unroll
            for (uint32_t q = 0; q < kPer; q++) {
                reinterpret_cast<uint4 *>(head)[q * kConfirmThreads + threadIdx.x] = vh[q];
                reinterpret_cast<uint4 *>(ftab)[q * kConfirmThreads + threadIdx.x] = vf[q];
            }
        }
        // the comparison tables: LDS when they fit (generic pointers: the same comparison code reads either copy)
        const uint32_t e_words = a.n_entries * 3u, b_words = a.n_bytes / 4u, c_words = a.n_class_words;
        const bool in_lds = confirm_tables_fit(a.n_entries, a.n_bytes, a.n_class_words);
        const ConfirmEntry *t_entries = a.c_entries;
        const uint8_t *t_bytes = a.c_bytes;
        const uint32_t *t_classes = a.c_classes;
        if (in_lds) {
            const uint32_t *se = reinterpret_cast<const uint32_t *>(a.c_entries), *sb = reinterpret_cast<const uint32_t *>(a.c_bytes);
            for (uint32_t k = threadIdx.x; k < e_words; k += kConfirmThreads) pool[k] = se[k];
            for (uint32_t k = threadIdx.x; k < b_words; k += kConfirmThreads) pool[e_words + k] = sb[k];
            for (uint32_t k = threadIdx.x; k < c_words; k += kConfirmThreads) pool[e_words + b_words + k] = a.c_classes[k];
            t_entries = reinterpret_cast<const ConfirmEntry *>(pool);
            t_bytes = reinterpret_cast<const uint8_t *>(pool + e_words);
            t_classes = pool + e_words + b_words;
        }
        __syncthreads();
        const ConfirmView cv{nullptr, t_entries, t_bytes, t_classes, a.mul, a.stride, a.init};
        const uint32_t n_p = min(*a.pair_count, a.pair_cap);
        // A lane's chain of dependent loads — pair -> the request's offsets, the chunk's text — is issued one work item AHEAD: the
        // next item's offsets and text (and the pair of the one after) travel while this item's windows are compared. (The kernel is
        // bound by those round trips, not by instructions: 65 % of its wave cycles were waits with everything issued on demand.)
        auto pair_of = [&](const uint32_t item) -> uint2 {
            const uint32_t k = (item - first_item) * kConfirmThreads + threadIdx.x;
            return (item < it_end && k < n_p) ? a.pairs[k] : make_uint2(kNone, 0u);  // (kNone: no pair for this lane)
        };
        uint2 pr_next = pair_of(it), pr_after = pair_of(it + 1u);
        uint32_t fs_next = 0u, fe_next = 0u;
        ConfirmBytes tb_next{};
        if (pr_next.x != kNone) {
            confirm_load64(reinterpret_cast<const uint8_t *>(a.off + pr_next.x), fs_next, fe_next);  // (the request's two offsets: one scattered load)
            tb_next = confirm_chunk_bytes(a.data, pr_next.y, a.total + PWAF_ARENA_PAD);
        }
        for (; it < it_end; it++) {
            const uint2 pr = pr_next;
            const bool live = pr.x != kNone;
            uint32_t r = live ? pr.x : 0u;  // the request that owns the chunk's first byte; a chunk that holds a field boundary also speaks for the next one(s)
            uint32_t fs = fs_next, fe = fe_next;
            const ConfirmBytes tb = tb_next;
            pr_next = pr_after;
            if (pr_next.x != kNone) {
                confirm_load64(reinterpret_cast<const uint8_t *>(a.off + pr_next.x), fs_next, fe_next);
                tb_next = confirm_chunk_bytes(a.data, pr_next.y, a.total + PWAF_ARENA_PAD);
            }
            pr_after = pair_of(it + 2u);
            ConfirmChunk ch{0u, 0ull};
            if (live) ch = confirm_windows_of(cv, tb, 0u, 0xFFFFFFFFu, pr.y, [&](const uint32_t bin) { return ftab[bin]; });  // (every window of the chunk: whose field it lies in is settled below)
            // the completed windows' entries, one comparison per lane and iteration (a lane advances to ITS next entry: the wave runs
            // as long as its longest lane, not the product of the two loops' longest trips)
            uint32_t mask = ch.mask, cnt = 0, j = 0, e0 = 0, pos = 0, widx = 0;
            bool walk = false;  // of request r (the one the lane is at)
            auto settle = [&](const uint32_t rq, const uint32_t need_lits, const bool wk, const bool aggregated) -> bool {
                // what the comparisons found for request rq: gap passes its literal hits call for, the walk list. Returns "append rq to
                // the walk list through the workgroup's aggregated atomic" (the lane's LAST request); an earlier request of the same
                // chunk (rare: the chunk holds a field boundary) is appended directly.
                bool w2 = wk;
                if (need_lits & a.shared_bits) w2 = true;  // a gap pass that shares the walk list learns of the request through the walk
                const uint32_t direct = need_lits & ~a.shared_bits;
                if (direct) enqueue_mask_once(a.gate_lists, a.gate_count, a.n, rq, direct, a.enq_bits, a.enq_words);
                if (!w2 || a.walk_list == nullptr) return false;
                const uint32_t bit = 1u << (rq & 31u);
                if (atomicOr(&a.walk_bits[rq >> 5], bit) & bit) return false;  // already listed
                atomicOr(&a.valid_bits[rq >> 5], bit);
                if (aggregated) return true;
                a.walk_list[atomicAdd(a.walk_count, 1u)] = rq;
                return false;
            };
            uint32_t need = 0;  // gap passes the literal hits of request r call for
            for (;;) {
                if (__ballot(j < cnt || mask != 0u) == 0) break;
                while (j >= cnt && mask != 0u) {
                    const uint32_t k = (uint32_t)__builtin_ctz(mask);
                    mask &= mask - 1u;
                    pos = pr.y * 16u + k;
                    const uint32_t bin = confirm_bin_of(ch, widx++, a.data, pos, a.mul);
                    while (pos >= fe && r + 1u < a.n) {  // the window lies in a later field of the chunk
                        settle(r, need, walk, false);
                        need = 0;
                        walk = false;
                        r++;
                        fs = fe;
                        fe = a.off[r + 1];
                    }
                    if (pos >= fe) continue;  // the bigram starts in the arena's slack (one that starts on the field's last byte may be the window of a short factor: confirm.h)
                    const uint32_t hd = head[bin];
                    e0 = hd & 0xFFFFFu;
                    cnt = hd >> 20;
                    j = 0;
                }
                if (j < cnt) {
                    const uint32_t res = in_lds ? confirm_entry<3>(t_entries, t_bytes, t_classes, e0 + j, a.data, fs, fe, pos)
                                                : confirm_entry<1>(t_entries, t_bytes, t_classes, e0 + j, a.data, fs, fe, pos);
                    j++;
                    if (res == 2u) {
                        walk = true;
                    } else if (res & 1u) {
                        const uint32_t atom = res >> 8;
                        merge_atom(a.pool, a.pool_count, a.status, a.pool_cap, a.rec + r, atom);
                        atomicOr(&a.valid_bits[r >> 5], 1u << (r & 31u));
                        if (a.colmask_local != nullptr) need |= a.colmask_local[atom];
                    }
                }
            }
            // Nothing confirmed (the common case by far): the lane is done and has written nothing.
            const bool append = live && settle(r, need, walk, true);
            // The walk list: the lane parks the request in the workgroup's LDS queue (an LDS atomic, no barrier); the queue is flushed with
            // ONE atomic on the list's length when the workgroup is done with the pass (a returned same-address atomic per request is
            // what DESIGN.md 4.1 measured at 0.5 ms per batch; a barrier per work item cost the 16 waves their independence).
            if (append) {
                const uint32_t slot = atomicAdd(&app_cnt, 1u);
                if (slot < kConfirmQueue) app_queue[slot] = r;
                else a.walk_list[atomicAdd(a.walk_count, 1u)] = r;  // (queue full: directly — rare)
            }
        }
        __syncthreads();
        {
            const uint32_t queued = min(app_cnt, kConfirmQueue);
            if (threadIdx.x == 0 && queued != 0) app_base = atomicAdd(a.walk_count, queued);
            __syncthreads();
            for (uint32_t k = threadIdx.x; k < queued; k += kConfirmThreads) a.walk_list[app_base + k] = app_queue[k];
            __syncthreads();
            if (threadIdx.x == 0) app_cnt = 0;
        }
    }
}

int launch_confirm(const ConfirmArgs *host, uint32_t count, const ConfirmArgs *dev, uint32_t *plan, uint32_t n_cus, void *stream) {
    if (count == 0 || host[0].n == 0) return 0;
    if (count > 256) return (int)hipErrorInvalidValue;
    ConfirmTableDev b{dev, count};
    hipLaunchKernelGGL(confirm_plan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, b, plan);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    // persistent grid: 2 workgroups of 1024 per CU (76 KiB of LDS each: 32 waves per CU), never more than the items a full batch could produce
    uint64_t max_items = 0;
    for (uint32_t k = 0; k < count; k++) max_items += ((uint64_t)host[k].pair_cap + kConfirmThreads - 1) / kConfirmThreads;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(max_items, (uint64_t)std::max(1u, n_cus) * 2u);
    const uint32_t *cplan = plan;
    hipLaunchKernelGGL(confirm_kernel, dim3(blocks), dim3(kConfirmThreads), 0, (hipStream_t)stream, b, cplan);
    return (int)hipGetLastError();
}

}  // namespace pwaf
