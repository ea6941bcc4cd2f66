// hitrec.h — the per-request HIT RECORD as the kernels that write one build it (the scans in scan.hip, fcmp_kernel and residual_kernel in
// kernels.hip, confirm.hip): two atoms inline, more through an overflow chain in the batch's pool (kernels.h: PoolEntry,
// REC_OVERFLOW), and the enqueueing of a finished request into the gap passes its hits call for. Device code only.
#pragma once
#include "kernels.h"
#include "wave.h"

namespace pwaf {

struct Hits {
    uint32_t a0, a1;  // local atom + 1, 0 = empty
    uint32_t ovf;     // head of the overflow chain, kNone = not overflowed
};

// The slow path is ONE out-of-line function that takes and returns the per-request hit state BY VALUE: passing `Hits` or the
// kernel arguments by reference would pin them in scratch memory, and every scratch access in the main loop is a vector
// memory operation whose s_waitcnt vmcnt(0) also drains the prefetched chunk (measured: 5 us per iteration).
struct SlowCtx {
    const uint32_t *list_off;
    const uint16_t *list;
    PoolEntry *pool;
    uint32_t *pool_count;
    uint32_t *status;
    uint32_t pool_cap;
};

__device__ __forceinline__ Hits pool_push(const SlowCtx &c, uint32_t atom, Hits h) {
    const uint32_t idx = atomicAdd(c.pool_count, 1u);
    if (idx >= c.pool_cap) {
        atomicOr(c.status, 1u);
        return h;
    }
    c.pool[idx].atom = atom;
    c.pool[idx].next = h.ovf;
    h.ovf = idx;
    return h;
}

__device__ __forceinline__ Hits record_atom(const SlowCtx &c, uint32_t atom, Hits h) {
    if (h.ovf == kNone) {
        if (h.a0 == atom + 1 || h.a1 == atom + 1) return h;
        if (h.a0 == 0) { h.a0 = atom + 1; return h; }
        if (h.a1 == 0) { h.a1 = atom + 1; return h; }
        const uint32_t x0 = h.a0 - 1, x1 = h.a1 - 1;
        h = pool_push(c, x0, h);
        h = pool_push(c, x1, h);
        return pool_push(c, atom, h);
    }
    // overflowed: the chain holds every atom of this request; de-duplicate against it (this lane is its only writer)
    for (uint32_t i = h.ovf; i != kNone;) {
        const uint32_t at = __hip_atomic_load(&c.pool[i].atom, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (at == atom) return h;
        i = __hip_atomic_load(&c.pool[i].next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return pool_push(c, atom, h);
}

__device__ __noinline__ inline Hits emit_list(const uint32_t *list_off, const uint16_t *list, PoolEntry *pool, uint32_t *pool_count, uint32_t *status,
                                       uint32_t pool_cap, uint32_t id, Hits h) {
    const SlowCtx c{list_off, list, pool, pool_count, status, pool_cap};
    const uint32_t b = list_off[id], e = list_off[id + 1];
    for (uint32_t k = b; k < e; k++) h = record_atom(c, list[k], h);
    return h;
}

#define PWAF_EMIT(id) h = emit_list(a.list_off, a.list, a.pool, a.pool_count, a.status, a.pool_cap, (id), h)

// The hit state a walk starts from when the request's record already holds hits (ListScanArgs::merge_rec).
__device__ __forceinline__ Hits hits_of_record(const uint32_t rv) {
    if (rv & REC_OVERFLOW) return Hits{0, 0, rv & ~REC_OVERFLOW};
    return Hits{rv & 0x7FFFu, (rv >> 15) & 0x7FFFu, kNone};
}
// ... and its inverse: the record a finished walk stores (kernels.h: REC_OVERFLOW).
__device__ __forceinline__ uint32_t record_of_hits(const Hits h) { return h.ovf != kNone ? (REC_OVERFLOW | h.ovf) : (h.a0 | (h.a1 << 15)); }
// The gap passes a finished request's hits call for: OR of the per-atom masks.
__device__ __noinline__ inline uint32_t gate_mask(const uint32_t *colmask_local, const PoolEntry *pool, Hits h) {
    uint32_t need = 0;
    if (h.ovf != kNone) {
        for (uint32_t i = h.ovf; i != kNone;) {
            need |= colmask_local[__hip_atomic_load(&pool[i].atom, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)];
            i = __hip_atomic_load(&pool[i].next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
        if (h.a0) need |= colmask_local[h.a0 - 1];
        if (h.a1) need |= colmask_local[h.a1 - 1];
    }
    return need;
}
// A finished request whose hits include prefilter factors is appended to the lists of the gated passes those factors guard
// (rare: one atomic per request and gated pass).
__device__ __noinline__ inline void enqueue_mask(uint32_t *gate_lists, uint32_t *gate_count, uint32_t n, uint32_t r, uint32_t need) {
    while (need) {
        const uint32_t g = (uint32_t)__builtin_ctz(need);
        need &= need - 1;
        gate_lists[(size_t)g * n + atomicAdd(&gate_count[g], 1u)] = r;
    }
}
// ... once per request and gap pass when the pass's enqueue bitmap is given (a list holds n entries; several chunks of one request — or
// its confirm tier and its walk — may all find a factor).
__device__ __noinline__ inline void enqueue_mask_once(uint32_t *gate_lists, uint32_t *gate_count, uint32_t n, uint32_t r, uint32_t need, uint32_t *enq_bits, uint32_t enq_words) {
    while (need) {
        const uint32_t g = (uint32_t)__builtin_ctz(need);
        need &= need - 1;
        if (enq_bits != nullptr) {
            const uint32_t bit = 1u << (r & 31u);
            if (atomicOr(&enq_bits[(size_t)g * enq_words + (r >> 5)], bit) & bit) continue;
        }
        gate_lists[(size_t)g * n + atomicAdd(&gate_count[g], 1u)] = r;
    }
}
__device__ __forceinline__ void enqueue_gated(const uint32_t *colmask_local, const PoolEntry *pool, uint32_t *gate_lists, uint32_t *gate_count, uint32_t n,
                                              uint32_t r, Hits h) {
    enqueue_mask(gate_lists, gate_count, n, r, gate_mask(colmask_local, pool, h));
}

}  // namespace pwaf
