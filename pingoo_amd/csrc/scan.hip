// scan.hip — the two DFA walkers of the pipeline with their launchers: scan_kernel streams EVERY request of a pass without a usable
// prefilter, lscan_kernel (with lscan_plan_kernel) walks the listed requests of the list-driven passes. Pipeline overview: kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "hitrec.h"
#include "kernels.h"
#include "utf8.h"
#include "wave.h"

namespace pwaf {

static constexpr int kScanThreads = 1024;
static constexpr int kScanWaves = kScanThreads / 64;

static constexpr uint32_t kClsBytes = 1024;  // byte-class map at LDS offset 0: 256 x uint32
// The walk is speculative (see scan_body): a lane that has just read a special cell keeps using it as an address until the
// group of 4 steps is checked, so every address a 16-bit cell can form — (0xFFFF << 1) + a class offset — must stay inside the
// allocation.
uint32_t scan_lds_bytes(uint32_t n_hot, uint32_t stride, uint32_t n_gate_atoms) {
    const uint32_t need = (((n_hot + 1) * stride * 2 + 15) & ~15u) + kClsBytes + n_gate_atoms * 4;
    const uint32_t reach = ((0xFFFFu << 1) + stride * 2 + kClsBytes + 15) & ~15u;
    return need > reach ? need : reach;
}

// -------------------------------------------------------------------------------------------------
// scan
// -------------------------------------------------------------------------------------------------
// One careful DFA step of one lane (out of line, by value): used when the speculative group walk met an emitting row, a cold
// row or a parked lane. `t` is the cell the lane read from LDS for this step.
struct Walk {
    uint32_t row, crow;
    Hits h;
};
// (Arguments are kept few and scalar: beyond the register budget of the calling convention the compiler passes `Hits` through
// scratch memory.)
__device__ __noinline__ Walk careful_step(const PWAF_GLOBAL unsigned char *gtab, const SpecialCell *special, const uint32_t *list_off, const uint16_t *list,
                                          PoolEntry *pool, uint32_t *ctrl /* [0] pool allocator, [1] status */, uint32_t pool_cap, uint32_t hot_emit /* hot_elems | emit_base << 16 */,
                                          uint32_t special_col /* special_base | emit_col2 << 16 */, uint32_t prev, uint32_t crow, uint32_t c2k, uint32_t t, uint32_t a0,
                                          uint32_t a1, uint32_t ovf) {
    const SlowCtx c{list_off, list, pool, ctrl, ctrl + 1, pool_cap};
    const uint32_t hot_elems = hot_emit & 0xFFFFu, emit_base = hot_emit >> 16, special_base = special_col & 0xFFFFu, emit_col2 = special_col >> 16;
    const Hits h{a0, a1, ovf};
    uint32_t cell = t;
    if (prev == hot_elems) cell = *reinterpret_cast<glb_u16_ptr>(gtab + crow + c2k);  // parked: the real (cold) row, from L2
    Walk w{cell, crow, h};
    if (cell >= special_base) {
        // the target row is cold: park on the sentinel row and remember where the real row lives
        const SpecialCell sp = special[cell - special_base];
        w.row = hot_elems;
        w.crow = sp.next_off;
        if (sp.emit) {
            const uint32_t b = list_off[sp.emit - 1], e = list_off[sp.emit];
            for (uint32_t k = b; k < e; k++) w.h = record_atom(c, list[k], w.h);
        }
    } else if (cell >= emit_base) {
        // a hot row that emits: its EMIT cell (LDS) names the match
        const uint32_t code = *reinterpret_cast<lds_u16_ptr>((uintptr_t)((cell << 1) + emit_col2 + kClsBytes));
        if (code & 0x8000u) {
            w.h = record_atom(c, code & 0x7FFFu, w.h);
        } else {
            const uint32_t b = list_off[code - 1], e = list_off[code];
            for (uint32_t k = b; k < e; k++) w.h = record_atom(c, list[k], w.h);
        }
    }
    return w;
}

// Scalar mode of a table (dfa.cpp, utf8.h): does a 16-byte window hold a LEAD byte (>= 0xC0: bits 7 and 6 set)? Asked once per window
// and wave (ASCII traffic: never), so that the class fix-up below costs the common case ten vector instructions per 16 bytes.
__device__ __forceinline__ bool window_has_lead(const u32x4 w) {
    const uint32_t m = (w.x & (w.x << 1)) | (w.y & (w.y << 1)) | (w.z & (w.z << 1)) | (w.w & (w.w << 1));
    return (m & 0x80808080u) != 0u;
}
// The class of the scalar value whose lead byte b0 sits at arena position `at` of a field that ends at `end` (rare path: one unaligned
// load of the three bytes behind it, two dependent table loads).
__device__ __noinline__ uint32_t lead_class(const uint8_t *umap, const uint32_t ill_class, const PWAF_GLOBAL unsigned char *gdata, const uint32_t b0, const uint32_t at, const uint32_t end) {
    const uint32_t next = *reinterpret_cast<const PWAF_GLOBAL uint32_t __attribute__((aligned(1))) *>(gdata + at + 1u);  // (PWAF_ARENA_PAD covers the read behind the arena's end)
    return utf8_class(umap, ill_class, b0, next, end - at);
}

// scalar mode: a window with any byte beyond ASCII takes the class fix-up (lead bytes AND continuation bytes are looked at)
__device__ __forceinline__ bool window_has_high(const u32x4 w) { return ((w.x | w.y | w.z | w.w) & 0x80808080u) != 0u; }
// The class of a CONTINUATION byte at arena position `at` of the field [start, end): the table's own (every transition stays: the
// sequence's symbol was read at its lead byte) when a well-formed sequence holds it, else the ill-formed class (utf8.h: utf8_cont_covered).
__device__ __noinline__ uint32_t cont_class(const uint32_t own_class, const uint32_t ill_class, const PWAF_GLOBAL unsigned char *gdata, const uint32_t at, const uint32_t start, const uint32_t end) {
    const uint32_t back = min(3u, at - start);
    uint32_t prev = 0;
    for (uint32_t d = 1; d <= back; d++) prev |= (uint32_t)gdata[at - d] << (8u * (d - 1u));
    const uint32_t self_next = *reinterpret_cast<const PWAF_GLOBAL uint32_t __attribute__((aligned(1))) *>(gdata + at);  // (PWAF_ARENA_PAD covers the read behind the arena's end)
    return utf8_cont_covered(prev, self_next, back, end - at) ? own_class : ill_class;
}

// CH = 16-byte chunks a lane walks per loop iteration. 2 halves the per-byte cost of the pull / finish logic (a third of the
// vector instructions at CH = 1) but idles a finished lane for up to 31 bytes instead of 15: it pays for long fields (URL,
// User-Agent), not for short ones (host, method). The engine picks it per pass from the tuning sample's mean field length.
// WIDE: a row has more than 127 byte classes, so a class's byte offset inside a row (class * 2) no longer fits the 256 x u8 class
// table; the table is then 256 x u32 (rare: it takes patterns that tell ~128 byte values apart).
template <int CH, bool WIDE>
__device__ __forceinline__ void scan_body(const ScanArgs &a) {
    extern __shared__ __align__(16) unsigned char lds[];
    const uint32_t stride2 = a.stride * 2;
    const uint32_t hot_bytes = a.n_hot * stride2;            // sentinel row starts here
    const uint32_t hot_elems = hot_bytes >> 1;
    const uint32_t tab_bytes = (hot_bytes + stride2 + 15) & ~15u;
    // LDS: [0, kClsBytes) byte -> BYTE offset of its class cell inside a row (class * 2; one dword per byte value: a plain 32-bit load needs no masking), then the
    // hot rows + sentinel row. The kernel has no static LDS, so the dynamic segment starts at LDS address 0 (checked below) and
    // lookups use plain integer addresses: the region bases fold into the ds_read offset fields, a class lookup is one SDWA
    // shift + ds_read_b32, a DFA step is v_lshl_add (cell * 2 + class offset) + ds_read_u16.
    if ((uint32_t)(uintptr_t)(PWAF_LDS unsigned char *)lds != 0u) __builtin_trap();
    // the attribute kernel shares the CUs: scan waves issue first, its waves take the slots they leave (default priority 0)
    __builtin_amdgcn_s_setprio(3);
    const PWAF_GLOBAL unsigned char *gtab = (const PWAF_GLOBAL unsigned char *)a.tab;
    const PWAF_GLOBAL unsigned char *gdata = (const PWAF_GLOBAL unsigned char *)a.data;
    const PWAF_GLOBAL uint32_t *goff = (const PWAF_GLOBAL uint32_t *)a.off;
    const uint32_t tid = threadIdx.x, wave = wave_index(), lane = tid & 63;

    // stage the hot rows, the sentinel row and the byte-class map into LDS (coalesced 16 B per lane)
    for (uint32_t i = tid * 16; i < tab_bytes; i += kScanThreads * 16) {
        uint4 v = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);  // sentinel cells: "special"
        if (i + 16 <= hot_bytes) v = *reinterpret_cast<const uint4 *>(reinterpret_cast<const unsigned char *>(a.tab) + i);
        *reinterpret_cast<uint4 *>(lds + kClsBytes + i) = v;
    }
    __syncthreads();
    if (hot_bytes & 15) {  // the last, partially covered 16-byte slot of the hot rows
        const uint32_t base = hot_bytes & ~15u;
        if (tid < (hot_bytes & 15) / 2) reinterpret_cast<uint16_t *>(lds + kClsBytes + base)[tid] = a.tab[base / 2 + tid];
    }
    if (tid < 256) {
        if (WIDE) reinterpret_cast<uint32_t *>(lds)[tid] = a.classmap[tid] * 2u;
        else lds[tid] = (unsigned char)(a.classmap[tid] * 2u);
    }
    // a pass that owns prefilter factors keeps its atom -> gated-pass bitmask map in LDS too (one lookup per hit of a finished request)
    const uint32_t gate_base = kClsBytes + tab_bytes;
    if (a.colmask_local != nullptr)
        for (uint32_t i = tid; i < a.n_local; i += kScanThreads) reinterpret_cast<uint32_t *>(lds + gate_base)[i] = a.colmask_local[i];
    __syncthreads();

    const uint32_t end_col = a.n_classes + 1;
    // the STAY cell's byte offset, pinned in a vector register: as a scalar it would be re-materialised (v_mov) before every
    // one of the 16 selects, because v_cndmask cannot read a second scalar next to VCC
    uint32_t stay2;
    asm volatile("v_mov_b32 %0, %1" : "=v"(stay2) : "s"(a.n_classes * 2u));
    const uint32_t emit_base = a.emit_base;        // cells >= emit_base: the row emits, or (>= special_base) is cold
    const uint32_t special_base = a.special_base;  // cells >= special_base index the special table
    const uint32_t emit_col2 = (a.n_classes + 2) * 2u;
    // this wave's slab of requests: contiguous, split evenly (rounding 1221 requests per wave up to 1280 would cost 5 % of every scan)
    const uint32_t n_items = a.n;
    const uint32_t total_waves = gridDim.x * kScanWaves;
    const uint32_t per_wave = (n_items + total_waves - 1) / total_waves;
    const uint32_t gw = blockIdx.x * kScanWaves + wave;
    const uint32_t w0 = min(n_items, gw * per_wave), w1 = min(n_items, w0 + per_wave);
    if (w0 >= w1) return;

    const unsigned long long lt_mask = (1ull << lane) - 1;
    const uint32_t start_emit = a.start_emit;

    uint32_t next = w0, blk = w0;
    auto load_off = [&](uint32_t base, uint32_t &lo, uint32_t &hi) {
        const uint32_t i = min(base + lane, n_items - 1);  // base + lane < n_items + 63; clamp keeps the load in bounds
        lo = goff[i];
        hi = goff[i + 1];
    };
    uint32_t o_lo, o_hi, n_lo = 0, n_hi = 0, n_base = kNone;
    load_off(blk, o_lo, o_hi);
    // Software pipeline: while a lane chews on the 16 bytes in `w`, the 16 bytes it will need in the NEXT iteration are
    // already in flight in `wn` — either the next chunk of the same field or, when this is the field's last chunk, the
    // first chunk of the request the lane has just pulled (r2/p2/end2). HBM/L2 latency hides behind 16 DFA steps.
    uint32_t r = kNone, p = 0, end = 0;           // current request
    uint32_t row = 0;                             // current row as a CELL value: its uint16 index in LDS, always even
                                                  // (== hot_elems: parked on the sentinel row, the real row is cold)
    uint32_t crow = 0;                            // byte offset of the current row in the full table while cold
    uint32_t r2 = kNone, p2 = 0, end2 = 0;        // request pulled ahead
    Hits h{0, 0, kNone};
    u32x4 w[CH], wn[CH];
#pragma unroll
    for (int q = 0; q < CH; q++) w[q] = wn[q] = u32x4{0, 0, 0, 0};
    constexpr uint32_t kStep = 16u * CH;  // bytes per iteration

    for (;;) {
        // offsets of the NEXT block of 64 work items: re-requested every iteration (L1 hits) instead of once per block inside a
        // branch, because a load whose result crosses a branch merge forces an immediate s_waitcnt vmcnt(0) — which would
        // also drain the chunk prefetch
        uint32_t f_lo, f_hi;
        const uint32_t f_base = blk + 64;
        load_off(f_base, f_lo, f_hi);
        // ---- 1. pull ahead: lanes on their last chunk (or idle) take the next request of the slab ----
        const bool last = r == kNone || p + kStep >= end;
        const unsigned long long want = __ballot(last && r2 == kNone);
        if (want != 0 && next < w1) {
            const uint32_t avail = min(w1 - next, blk + 64 - next);
            const uint32_t rank = (uint32_t)__builtin_popcountll(want & lt_mask);
            const bool take = last && r2 == kNone && rank < avail;
            const uint32_t j = take ? next + rank - blk : 0;
            const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(j << 2), (int)o_lo);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(j << 2), (int)o_hi);
            if (take) {
                r2 = next + rank;
                p2 = lo;
                end2 = hi;
            }
            next += min((uint32_t)__builtin_popcountll(want), avail);
            if (next == blk + 64 && next < w1) {
                blk += 64;
                if (n_base == blk) {  // requested during an earlier iteration for this very block
                    o_lo = n_lo;
                    o_hi = n_hi;
                } else {              // two block switches in consecutive iterations (very short fields): fetch now
                    load_off(blk, o_lo, o_hi);
                }
            }
        }
        if (__ballot(r != kNone || r2 != kNone) == 0) break;
        {
            // Unconditional (no branch, so no wait is forced here): lanes with nothing to fetch read the arena's first bytes.
            // Unaligned 16-byte load; arenas carry PWAF_ARENA_PAD slack.
            const bool have = last ? (r2 != kNone && p2 < end2) : true;
            const uint32_t np = have ? (last ? p2 : p + kStep) : 0u;
            const uint32_t nend = last ? end2 : end;  // end of the field the next iteration works on
#pragma unroll
            for (int q = 0; q < CH; q++) {
                // a further chunk is fetched only if the field reaches it: reads never go more than PWAF_ARENA_PAD past a field's end
                const uint32_t at = (q == 0 || (have && np + 16u * q < nend)) ? np + 16u * q : 0u;
                wn[q] = *reinterpret_cast<const PWAF_GLOBAL u32x4_u *>(gdata + at);
            }
        }

        // ---- 2. 16 * CH bytes of every active lane's field ----
        const bool act = r != kNone && p < end;
        const uint32_t cnt_all = act ? min(kStep, end - p) : 0u;
#pragma unroll
        for (int q = 0; q < CH; q++) {
        const uint32_t cnt = cnt_all > 16u * q ? min(16u, cnt_all - 16u * q) : 0u;  // valid bytes of this chunk
        const uint32_t wd[4] = {w[q].x, w[q].y, w[q].z, w[q].w};
        uint32_t c2[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint32_t byte = (wd[k >> 2] >> ((k & 3) * 8)) & 0xFFu;
            // byte classes do not depend on the state: all 16 lookups are issued before the dependent chain starts
            const uint32_t c = WIDE ? *reinterpret_cast<lds_u32_ptr>((uintptr_t)(byte << 2)) : (uint32_t)*reinterpret_cast<lds_u8_ptr>((uintptr_t)byte);
            c2[k] = (uint32_t)k < cnt ? c : stay2;  // past the end: the STAY cell
        }
        if (a.umap != nullptr && __ballot(cnt != 0u && window_has_high(w[q])) != 0ull) {  // scalar mode, a byte beyond ASCII in somebody's chunk (rare)
            const uint32_t f_start = r != kNone ? a.off[r] : 0u;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const uint32_t byte = (wd[k >> 2] >> ((k & 3) * 8)) & 0xFFu;
                if (byte >= 0xC0u && (uint32_t)k < cnt) c2[k] = 2u * lead_class(a.umap, a.ill_class, gdata, byte, p + 16u * (uint32_t)q + (uint32_t)k, end);
                else if (byte >= 0x80u && (uint32_t)k < cnt) c2[k] = cont_class(c2[k], 2u * a.ill_class, gdata, p + 16u * (uint32_t)q + (uint32_t)k, f_start, end);
            }
        }
        // The 16 steps run in groups of 4 with ONE check per group: inside a group every lane chains lookup to lookup
        // (v_lshl_add + ds_read_u16, nothing else on the dependent path), treating whatever it reads as the next row. Only if
        // some lane read a cell >= emit_base (it entered an emitting row, left the hot set, or is parked on a cold row) are
        // the group's 4 steps re-walked carefully by the lanes concerned; all other lanes keep their speculative result.
#pragma unroll
        for (int k0 = 0; k0 < 16; k0 += 4) {
            const uint32_t t1 = *reinterpret_cast<lds_u16_ptr>((uintptr_t)((row << 1) + c2[k0] + kClsBytes));
            const uint32_t t2 = *reinterpret_cast<lds_u16_ptr>((uintptr_t)((t1 << 1) + c2[k0 + 1] + kClsBytes));
            const uint32_t t3 = *reinterpret_cast<lds_u16_ptr>((uintptr_t)((t2 << 1) + c2[k0 + 2] + kClsBytes));
            const uint32_t t4 = *reinterpret_cast<lds_u16_ptr>((uintptr_t)((t3 << 1) + c2[k0 + 3] + kClsBytes));
            if (max(max(t1, t2), max(t3, t4)) >= emit_base) {
                // Entering a hot row that emits does not break the chain (its cell is a real row), so the speculative cells stay
                // usable until the lane meets a special cell; the usual case — a match that is already in the request's record, or
                // fits a free slot — is settled from LDS and registers alone.
                uint32_t cur = row;
                bool chain = true;
                auto redo = [&](const uint32_t ts, const uint32_t cls, const bool in_range) {
                    const uint32_t t = chain ? ts : (uint32_t)*reinterpret_cast<lds_u16_ptr>((uintptr_t)((cur << 1) + cls + kClsBytes));
                    if (in_range) {  // (past the end the row does not change)
                        bool slow = t >= special_base;
                        if (!slow && t >= emit_base) {
                            const uint32_t code = *reinterpret_cast<lds_u16_ptr>((uintptr_t)((t << 1) + emit_col2 + kClsBytes));
                            const uint32_t x = (code & 0x7FFFu) + 1;
                            if (!(code & 0x8000u) || h.ovf != kNone) slow = true;  // a list of matches, or the record has overflowed
                            else if (h.a0 == x || h.a1 == x) {}
                            else if (h.a0 == 0) h.a0 = x;
                            else if (h.a1 == 0) h.a1 = x;
                            else slow = true;
                        }
                        if (slow) {
                            const Walk wk = careful_step(gtab, a.special, a.list_off, a.list, a.pool, a.pool_count, a.pool_cap, hot_elems | (emit_base << 16),
                                                         special_base | (emit_col2 << 16), cur, crow, cls, t, h.a0, h.a1, h.ovf);
                            chain = chain && wk.row == t;  // still on a real hot row: the cells read after it remain valid
                            cur = wk.row;
                            crow = wk.crow;
                            h = wk.h;
                        } else {
                            cur = t;
                        }
                    } else {
                        chain = chain && t < special_base;  // (a parked lane past its end reads the sentinel: nothing to reuse)
                    }
                };
                redo(t1, c2[k0], (uint32_t)k0 < cnt);
                redo(t2, c2[k0 + 1], (uint32_t)(k0 + 1) < cnt);
                redo(t3, c2[k0 + 2], (uint32_t)(k0 + 2) < cnt);
                redo(t4, c2[k0 + 3], (uint32_t)(k0 + 3) < cnt);
                row = cur;
            } else {
                row = t4;
            }
        }
        }  // chunks
        p += cnt_all;

        // ---- 3. finished requests: end-of-field matches, the hit record, then switch to the pulled-ahead request ----
        if (r != kNone && p >= end) {
            const uint32_t e = row == hot_elems ? (uint32_t)*reinterpret_cast<glb_u16_ptr>(gtab + crow + (end_col << 1))
                                                : (uint32_t)*reinterpret_cast<lds_u16_ptr>((uintptr_t)(((row + end_col) << 1) + kClsBytes));
            if (e & 0x8000u) {  // a single end-of-field match: settled in registers unless the record is full
                const uint32_t x = (e & 0x7FFFu) + 1;
                if (h.ovf == kNone && (h.a0 == x || h.a1 == x)) {
                } else if (h.ovf == kNone && h.a0 == 0) {
                    h.a0 = x;
                } else if (h.ovf == kNone && h.a1 == 0) {
                    h.a1 = x;
                } else {
                    const SlowCtx sc{a.list_off, a.list, a.pool, a.pool_count, a.status, a.pool_cap};
                    h = record_atom(sc, x - 1, h);
                }
            } else if (e) {
                PWAF_EMIT(e - 1);
            }
            a.rec[r] = record_of_hits(h);
            if (a.colmask_local != nullptr && (h.a0 | (h.ovf + 1u)) != 0) {
                // does any hit of this request gate a later pass? (LDS lookups; the enqueue itself is rare and out of line)
                uint32_t need = 1;  // overflowed record: let the slow path walk the chain
                if (h.ovf == kNone) {
                    need = *reinterpret_cast<lds_u32_ptr>((uintptr_t)(gate_base + (h.a0 - 1) * 4));
                    if (h.a1) need |= *reinterpret_cast<lds_u32_ptr>((uintptr_t)(gate_base + (h.a1 - 1) * 4));
                }
                if (need) enqueue_gated(a.colmask_local, a.pool, a.gate_lists, a.gate_count, a.n, r, h);
            }
            r = kNone;
        }
        if (r == kNone && r2 != kNone) {
            r = r2;
            p = p2;
            end = end2;
            r2 = kNone;
            row = 0;
            h = Hits{0, 0, kNone};
            if (start_emit) PWAF_EMIT(start_emit - 1);
        }
#pragma unroll
        for (int q = 0; q < CH; q++) w[q] = wn[q];
        n_lo = f_lo;
        n_hi = f_hi;
        n_base = f_base;
    }
}

template <int CH, bool WIDE>
__global__ __launch_bounds__(kScanThreads) void scan_kernel(ScanArgs a) { scan_body<CH, WIDE>(a); }

// Every instantiation, named once: launch_scan picks from this table, configure_scan_kernels walks it. [CH = 1 / 2 / 4, + 3 if WIDE]
static const void *const kScanFns[6] = {reinterpret_cast<const void *>(scan_kernel<1, false>), reinterpret_cast<const void *>(scan_kernel<2, false>),
                                        reinterpret_cast<const void *>(scan_kernel<4, false>), reinterpret_cast<const void *>(scan_kernel<1, true>),
                                        reinterpret_cast<const void *>(scan_kernel<2, true>), reinterpret_cast<const void *>(scan_kernel<4, true>)};

int launch_scan(const ScanArgs &a, void *stream) {
    const uint32_t lds = scan_lds_bytes(a.n_hot, a.stride, a.colmask_local ? a.n_local : 0u);
    const bool wide = a.n_classes > 127;
    const int v = (a.chunks == 4 ? 2 : a.chunks == 2 ? 1 : 0) + (wide ? 3 : 0);
    const void *fn = kScanFns[v];
    if (a.n == 0) return 0;
    // at least 256 requests per wave so that work-pulling has something to balance
    uint32_t waves = (a.n + 255) / 256;
    uint32_t blocks = (waves + kScanWaves - 1) / kScanWaves;
#ifdef PWAF_PROFILING
    static const uint32_t forced_cap = getenv("PWAF_SCAN_BLOCKS") ? (uint32_t)atoi(getenv("PWAF_SCAN_BLOCKS")) : 0u;
#else
    const uint32_t forced_cap = 0;
#endif
    const uint32_t cap = forced_cap ? forced_cap : std::max(1u, a.n_cus);  // one persistent workgroup per CU: the table is staged once
    if (blocks > cap) blocks = cap;
    if (blocks == 0) blocks = 1;
    void *args[] = {const_cast<ScanArgs *>(&a)};
    hipError_t e = hipLaunchKernel(fn, dim3(blocks), dim3(kScanThreads), args, lds, (hipStream_t)stream);
    return (int)(e != hipSuccess ? e : hipGetLastError());
}

// lscan_kernel: every list-driven pass of a phase in ONE persistent launch. One listed request per lane, walked byte by byte: per step
// one LDS read for the byte's class (independent of the state: issued ahead) and one dependent read of the cell from the LDS copy of
// the table's hottest rows. (The wave-lockstep walk of scan_kernel, built for streaming EVERY request, took 0.6 ms on the same
// lists: every lane a candidate, its slow paths fire in every group of steps.)
//
// Cold rows: a cell outside the LDS copy lives in the L2-resident flat table (~1 us away) and the wave waits for it. (Round 3 tried
// PARKING such lanes — stop consuming bytes, issue all of a window's cold loads together at its end, resume one byte further: at most
// one round trip per 16-byte window instead of one per step. Measured slower everywhere: benign 0.234 vs 0.177 ms, adversarial 5.3 vs
// 3.9 ms for the filtered passes of the 1k-rule set. The extra selects per step cost more than the waits they save — on adversarial
// traffic the walk is bound by VALU + LDS issue, ~10 instructions per byte and lane, not by latency — and a lane deep in rarely
// visited states, which parks at every byte, became twice as slow and sets the wave's time.)
//
// Work distribution (round 3): the list lengths are only known on the device. lscan_plan_kernel turns them into a prefix sum of work
// items (kListThreads entries of one pass each); the scan launch is a persistent grid in which workgroup b takes the contiguous items
// [total * b / G, total * (b + 1) / G) — consecutive items are mostly of one pass, whose hot rows are staged once. (Round 2 launched
// ceil(n / 512) x passes workgroups, nearly all of which found their list exhausted: 53k launches-and-exits for the 69 filtered
// passes of the 4096-rule set.)
// A work item is one WAVE's share of a list: `epi` entries (a power of two up to 64, per pass: plan[count + 1 + pass]). A long list
// packs 64 walks into a wave; a SHORT one — the few requests whose regex factor the confirm tier found, a gap pass's requests — is
// spread one or a few walks per wave over the waves the launch has: the 64 walks of a wave advance in lockstep and every emit or cold
// cell of one lane sends the whole wave through the slow path of its group of steps, so a wave of 64 true hits (what a dense walk list
// is made of) crawls while the rest of the chip idles (measured: 0.07 -> 0.5 ms for ~10k walks when the lists became dense).
// the list a pass walks in this batch (kernels.h: ListScanArgs::dense_flag)
__device__ __forceinline__ ListOf list_of(const ListScanArgs &a) {
    ListOf l{a.req_list, a.req_list != nullptr ? min(*a.n_list, a.n) : a.n};
    if (a.dense_mode != 0u) {
        const bool dense = *a.dense_flag > a.dense_thresh;
        if (a.dense_mode == 1u && !dense) l.n_l = 0u;
        if (a.dense_mode == 2u && dense) l.n_l = 0u;
        if (a.dense_mode == 3u && dense) l = ListOf{nullptr, a.n};
    }
    return l;
}

// (Round 6: the entries per item also have a floor common to the launch's passes — the power of two with which ALL the passes' entries fit the launch's
// waves once, 16 at most. A pass's own rule alone let six gap passes that ride one walk list of 16k requests make 4 063 four-entry items EACH: 24k items on
// 6 144 waves, four nearly empty items one behind the other per wave, every one the whole dependent chain of a walk — 0.084 ms for 97k entries, most of them
// skipped by their need bit. With the common floor they are 16-entry items, one per wave: lscan_x6 0.084 -> 0.039 ms alone, 0.11 -> 0.05 in the step; the
// 4096-rule set's gap launch 0.094 -> 0.051, its hostile stream's R-tier launch 0.236 -> 0.107. Measured and dropped: the floor counted against the waves of ONE
// workgroup per CU — what is resident beside the attribute kernel — with the items packed into the first workgroups: fewer, fuller waves walk in lockstep
// and are slower — a 1.25M-request share's gap launch 0.033 -> 0.044 ms, nothing gained at 10M.)
__global__ __launch_bounds__(256) void lscan_plan_kernel(GatedTable b, uint32_t *plan /* [2 count + 1] */, uint32_t n_waves) {
    __shared__ uint32_t part[256];
    __shared__ unsigned long long all_entries;
    const uint32_t t = threadIdx.x;
    uint32_t items = 0;
    const uint32_t n_l = t < b.count ? list_of(b.g[t]).n_l : 0u;
    if (t == 0) all_entries = 0ull;
    __syncthreads();
    if (n_l != 0u) atomicAdd(&all_entries, (unsigned long long)n_l);
    __syncthreads();
    if (t < b.count) {
        const uint32_t room = n_waves > b.count ? n_waves - b.count : 1u;  // (every pass may end in a partly filled item)
        const unsigned long long per_wave = (all_entries + room - 1u) / room;
        uint32_t epi = 1;
        while (epi < 16u && epi < per_wave) epi <<= 1;
        while (epi < 64u * kListWalks && (n_l + epi - 1) / epi > n_waves) epi <<= 1;
        items = (n_l + epi - 1) / epi;
        plan[b.count + 1 + t] = epi;
    }
    part[t] = items;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {  // Hillis-Steele inclusive scan (count <= 250)
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    if (t < b.count) plan[t] = part[t] - items;
    if (t == 0) plan[b.count] = part[255];
}

// One step of a walk whose state may lie outside the LDS-resident rows: a DELTA record (kernels.h: ListScanArgs::delta — base row and
// two exception cells, 8 bytes in LDS) or, failing that, the L2-resident flat table. `c` = the byte's class (n_classes + 1: past the
// field's end, the state stays).
__device__ __forceinline__ uint32_t list_step_slow(const uint16_t *hot, const PWAF_GLOBAL uint16_t *flat, const uint64_t *delta, const uint32_t state, const uint32_t c,
                                                   const uint32_t stride, const uint32_t n_hot, const uint32_t n_delta) {
    if (state < n_hot) return hot[state * stride + c];
    const uint32_t k = state - n_hot;
    if (k < n_delta) {
        if (c + 2u == stride) return state;  // the STAY cell
        const uint64_t rec = delta[k];
        const uint32_t lo = (uint32_t)rec, hi = (uint32_t)(rec >> 32);
        if (c == ((lo >> 16) & 0xFFu)) return hi & 0xFFFFu;
        if (c == (lo >> 24)) return hi >> 16;
        return hot[(lo & 0xFFFFu) * stride + c];
    }
    return flat[state * stride + c];
}

// A LONG list (more than an eighth of the batch: hostile traffic — near misses of the rule literals in most requests), walked with the
// cold steps taken TOGETHER. In the lockstep loop below a group of four steps in which ANY of the 64 lanes meets a cold cell (a row
// that is not LDS-resident: an L2 round trip) is re-walked step by step by the whole wave, and although a lane spends under a tenth
// of its steps in cold rows, some lane of the wave does nearly always: measured on the hostile stream of the 1k-rule set, 28 of the
// 36 groups of a wave's walk take the slow path, and those round trips are 85 % of the scan's 3.6 ms. Here every lane keeps its own
// position: per iteration a lane whose next four cells are LDS-resident takes them (the wave's cheap iteration), a lane that is not
// waits — and when half the wave is waiting (or nobody else can move) ONE slow iteration takes the blocked lanes through their
// group, cold cells from L2, while the others wait: a round trip then serves thirty lanes instead of one.
template <uint32_t THREADS>
__device__ __forceinline__ void lscan_async(const ListScanArgs &a, const uint16_t *hot, const unsigned char *cls, const uint64_t *delta, uint32_t it, const uint32_t it_end,
                                            const uint32_t first, const uint32_t n_l, const uint32_t hot_elems, const uint32_t epi) {
    const uint32_t ncls = a.n_classes, stride = ncls + 3u;
    const PWAF_GLOBAL unsigned char *gdata = (const PWAF_GLOBAL unsigned char *)a.data;
    const PWAF_GLOBAL uint16_t *flat = (const PWAF_GLOBAL uint16_t *)a.flat;
    auto record_emit = [&](const uint32_t st, Hits &hh) {
        const uint32_t ei = st * stride + ncls;
        const uint32_t code = ei < hot_elems ? (uint32_t)hot[ei] : (uint32_t)flat[ei];
        const uint32_t x = (code & 0x7FFFu) + 1u;
        bool slow = !(code & 0x8000u) || hh.ovf != kNone;
        if (!slow) {
            if (hh.a0 == x || hh.a1 == x) {}
            else if (hh.a0 == 0) hh.a0 = x;
            else if (hh.a1 == 0) hh.a1 = x;
            else slow = true;
        }
        if (slow) hh = emit_list(a.emit_off, a.emit_list, a.pool, a.pool_count, a.status, a.pool_cap, st, hh);
    };
    for (it += wave_index(); it < it_end; it += THREADS / 64u) {  // (work items are one wave's share of the list: this wave's)
        const uint32_t li = (it - first) * epi + (threadIdx.x & 63u);
        bool live = (threadIdx.x & 63u) < epi && li < n_l;
        if (live && a.need_in != nullptr) live = ((a.need_in[li] >> a.need_bit) & 1u) != 0;  // (a sharing gap pass: none of its factors fired here)
        const uint32_t r = live ? (a.req_list != nullptr ? a.req_list[li] : li) : 0u;
        if (live && a.visited != nullptr) atomicOr(&a.visited[r >> 5], 1u << (r & 31u));
        uint32_t p = live ? a.off[r] : 0u;           // the next byte to read
        const uint32_t end = live ? a.off[r + 1] : 0u;
        uint32_t state = 0, wp = p;                  // wp: where the window in `w` begins (p - wp is a multiple of 4, below 16 after the reload)
        Hits h{0, 0, kNone};
        uint32_t need_init = 0;  // what the record's hits (filter heads, confirm tier) already enqueued
        if (live && a.merge_rec) {
            h = hits_of_record(a.rec[r]);
            if (a.colmask_local != nullptr && (h.a0 | (h.ovf + 1u)) != 0) need_init = gate_mask(a.colmask_local, a.pool, h);
        }
        if (live && a.emit_off[1] != a.emit_off[0]) h = emit_list(a.emit_off, a.emit_list, a.pool, a.pool_count, a.status, a.pool_cap, 0u, h);
        u32x4 w = *reinterpret_cast<const PWAF_GLOBAL u32x4_u *>(gdata + wp);
        u32x4 wn = *reinterpret_cast<const PWAF_GLOBAL u32x4_u *>(gdata + (wp + 16u < end ? wp + 16u : 0u));
        for (;;) {
            const bool active = p < end;
            const unsigned long long am = __ballot(active);
            if (am == 0) break;
            if (active && p - wp >= 16u) {  // this lane's window is used up: the prefetched one takes its place, the one after is requested
                w = wn;
                wp += 16u;
                wn = *reinterpret_cast<const PWAF_GLOBAL u32x4_u *>(gdata + (wp + 16u < end ? wp + 16u : 0u));
            }
            const uint32_t j = (p - wp) >> 2;
            const uint32_t wd = j == 0 ? w.x : j == 1 ? w.y : j == 2 ? w.z : w.w;
            const uint32_t cnt = active ? min(4u, end - p) : 0u;
            uint32_t c[4], t[4], sv[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) c[k] = cls[(wd >> (k * 8)) & 0xFFu];
            asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]));  // (the four class lookups stay unconditional: left alone the compiler sinks each under its "k < cnt" — sixteen exec-mask branches per window, which doubled the walk's time)
            if (a.umap != nullptr && __ballot(active && (wd & 0x80808080u) != 0u) != 0ull) {  // scalar mode, a byte beyond ASCII somewhere (rare): the scalar's class at a lead byte, a stray continuation byte is ill-formed
                const uint32_t f_start = active ? a.off[r] : 0u;
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t byte = (wd >> (k * 8)) & 0xFFu;
                    if (byte >= 0xC0u && k < cnt) c[k] = lead_class(a.umap, a.ill_class, gdata, byte, p + k, end);
                    else if (byte >= 0x80u && k < cnt) c[k] = cont_class(c[k], a.ill_class, gdata, p + k, f_start, end);
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) c[k] = k < cnt ? c[k] : ncls + 1u;
#pragma unroll
            // (A branch-free step that serves row states and delta-record states alike — record, then the cell of the row or of the
            // record's base row, then the two exceptions: two dependent LDS reads for every lane — was measured: 4.9 ms against 3.1
            // for the hostile stream's filtered passes. States without a row in LDS, records included, wait for the slow iteration.)
            for (uint32_t k = 0; k < 4; k++) {
                t[k] = *reinterpret_cast<lds_u16_ptr>((uintptr_t)min(__umul24(k == 0 ? state : sv[k - 1], 2u * stride) + 2u * c[k], 2u * hot_elems));
                sv[k] = t[k] & 0x7FFFu;
            }
            const uint32_t any = t[0] | t[1] | t[2] | t[3], top = max(max(t[0], t[1]), max(t[2], t[3]));
            const bool blocked = active && top == 0xFFFFu;
            const unsigned long long bm = __ballot(blocked);
            const uint32_t n_blocked = (uint32_t)__builtin_popcountll(bm);
            if (n_blocked < 32u && bm != am) {
                // the cheap iteration: every lane whose four cells are LDS-resident takes them
                if (active && !blocked) {
                    if (any & 0x8000u) {
#pragma unroll
                        for (uint32_t k = 0; k < 4; k++)
                            if (t[k] & 0x8000u) record_emit(sv[k], h);
                    }
                    state = sv[3];
                    p += 4u;
                }
            } else if (blocked) {
                // the slow iteration: the blocked lanes' group step by step, cold cells from the L2-resident table
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t tt = list_step_slow(hot, flat, delta, state, c[k], stride, a.n_hot, a.n_delta);
                    state = tt & 0x7FFFu;
                    if (tt & 0x8000u) record_emit(state, h);
                }
                p += 4u;
            }
        }
        if (live) {
            if (a.end_off[state + 1] != a.end_off[state]) h = emit_list(a.end_off, a.end_list, a.pool, a.pool_count, a.status, a.pool_cap, state, h);
            a.rec[r] = record_of_hits(h);
            if (a.colmask_local != nullptr) {
                uint32_t need = 0;
                if ((h.a0 | (h.ovf + 1u)) != 0) need = gate_mask(a.colmask_local, a.pool, h);
                if (a.need_out != nullptr) a.need_out[li] = need;
                need &= ~(a.shared_bits | need_init);
                if (need) enqueue_mask_once(a.gate_lists, a.gate_count, a.n, r, need, a.enq_bits, a.enq_words);
            }
        }
    }
}

// (waves per SIMD: three 512-thread workgroups per CU need 6, i.e. at most 80 vector registers)
template <uint32_t THREADS>
__global__ __launch_bounds__(THREADS, THREADS == 512 ? 6 : 4) void lscan_kernel(GatedTable b, const uint32_t *plan, uint32_t hot_bytes) {
    extern __shared__ uint32_t lscan_lds[];  // [hot_bytes / 4] hot rows + 16 bytes for the sentinel cell, then the 256-byte class map
    __builtin_amdgcn_s_setprio(3);  // on the critical path, beside the attribute kernel's background waves
    if ((uint32_t)(uintptr_t)(PWAF_LDS unsigned char *)lscan_lds != 0u) __builtin_trap();  // (no static LDS in this kernel: the walks address the hot rows by plain integer offsets)
    const uint32_t total = plan[b.count];
    const uint32_t it0 = (uint32_t)((uint64_t)total * blockIdx.x / gridDim.x), it1 = (uint32_t)((uint64_t)total * (blockIdx.x + 1) / gridDim.x);
    const unsigned char *cls = reinterpret_cast<const unsigned char *>(lscan_lds + (hot_bytes + 16u) / 4);
    const uint16_t *hot = reinterpret_cast<const uint16_t *>(lscan_lds);
    for (uint32_t it = it0; it < it1;) {
        // the pass of item `it`: the last p with plan[p] <= it (uniform)
        uint32_t ps = 0;
        for (uint32_t lo = 0, hi = b.count; lo + 1 < hi;) {
            const uint32_t mid = (lo + hi) >> 1;
            if (plan[mid] <= it) lo = mid;
            else hi = mid;
            ps = lo;
        }
        const uint32_t first = plan[ps], it_end = min(it1, plan[ps + 1]), epi = plan[b.count + 1 + ps];
        ListScanArgs a = load_descriptor(&b.g[ps]);
        const ListOf lst = list_of(a);
        a.req_list = lst.req_list;  // (the flag-density switch may have turned a shared list into "every request")
        const uint32_t ncls = a.n_classes, stride = ncls + 3u;  // row: ncls transitions, the EMIT cell, the STAY cell, the END cell
        const uint32_t hot_elems = a.n_hot * stride;
        uint64_t *delta_lds = reinterpret_cast<uint64_t *>(lscan_lds) + (hot_elems * 2u + 2u + 15u) / 16u * 2u;  // (16-byte aligned, behind the sentinel cell)
        __syncthreads();  // (every wave is done with the previous pass's rows)
        {
            // 16 bytes per lane and load, four loads in flight (a dword-per-lane loop of dependent load -> store pairs took a dozen L2
            // round trips per workgroup: as long as the walk of a short list). The flat table is padded to whole 16-byte units.
            const uint4 *src = reinterpret_cast<const uint4 *>(a.flat);
            uint4 *dst = reinterpret_cast<uint4 *>(lscan_lds);
            const uint32_t units = (hot_elems * 2u + 15u) / 16u;
            for (uint32_t k = threadIdx.x; k < units; k += THREADS * 4u) {
                uint4 v[4];
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) v[q] = k + q * THREADS < units ? src[k + q * THREADS] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
                for (uint32_t q = 0; q < 4; q++)
                    if (k + q * THREADS < units) dst[k + q * THREADS] = v[q];
            }
            if (threadIdx.x < 64) lscan_lds[(hot_bytes + 16u) / 4 + threadIdx.x] = reinterpret_cast<const uint32_t *>(a.classmap)[threadIdx.x];  // class map
            // the delta records, behind the rows and the sentinel cell (the engine sized rows + 32 + records to fit hot_bytes)
            for (uint32_t k = threadIdx.x; k < a.n_delta; k += THREADS) delta_lds[k] = a.delta[k];
        }
        __syncthreads();
        // the SENTINEL cell right behind the hot rows (after the barrier: the staging loop's last 16-byte unit may cover it): every
        // index beyond the hot rows is clamped onto it and reads 0xFFFF = "this cell is cold" (no state has id 0x7FFF)
        if (threadIdx.x == 0) reinterpret_cast<uint16_t *>(lscan_lds)[hot_elems] = 0xFFFFu;
        __syncthreads();
        const uint32_t n_l = lst.n_l;
        // (the gap passes' lists stay with the lockstep loop: measured 0.25 -> 0.40 ms with this one on the hostile stream — their walks
        // are short and mostly LDS-resident, and the asynchronous iteration costs more per group)
#ifdef PWAF_PROFILING
        const bool long_list = (b.debug & 1u) ? false : (b.debug & 2u) ? true : (a.behind_filter != 0u && (uint64_t)n_l * 8u >= a.n);  // timing experiments: never / always the asynchronous loop (same results)
#else
        const bool long_list = a.behind_filter != 0u && (uint64_t)n_l * 8u >= a.n;
#endif
        if (long_list) {  // (uniform) a prefilter's candidate list that holds more than an eighth of the batch: lscan_async
            lscan_async<THREADS>(a, hot, cls, delta_lds, it, it_end, first, n_l, hot_elems, epi);
            it = it_end;
            continue;
        }
        const PWAF_GLOBAL unsigned char *gdata = (const PWAF_GLOBAL unsigned char *)a.data;
        const PWAF_GLOBAL uint16_t *flat = (const PWAF_GLOBAL uint16_t *)a.flat;
        // A work item is ONE WAVE's worth of list entries (round 4; it used to be a workgroup's: a short list — the few requests whose
        // regex factor the confirm tier found, a gap pass's requests — then sat in a handful of full waves on a handful of CUs, every
        // wave as slow as the unluckiest of its 64 walks, while the rest of the chip idled: 0.07 -> 0.6 ms when the lists became dense).
        for (uint32_t iw = it + wave_index(); iw < it_end; iw += THREADS / 64u) {
            // kListWalks listed requests per lane, walked in lockstep. Measured with 2 (round 3), in the hope that a lane's two cold cells
            // travelling to L2 together would help hostile traffic (near misses of the rule literals drive most walks deep into states
            // that are not LDS-resident): adversarial filtered passes 3.87 -> 3.41 ms, but benign 0.143 -> 0.204 ms and the gap
            // passes 0.087 -> 0.117 (adversarial 0.24 -> 0.49): a single wave issues an instruction every few cycles at best, so two
            // interleaved chains cost a step twice the issue slots while the list's longest walk — the kernel's critical path on
            // benign traffic — gets no shorter. One walk per lane and as many waves as the LDS copy allows is the better trade.
            uint32_t li[kListWalks], r[kListWalks], p[kListWalks], end[kListWalks], state[kListWalks], need_init[kListWalks];
            bool live[kListWalks];
            Hits h[kListWalks];
            u32x4 w[kListWalks];
#pragma unroll
            for (uint32_t u = 0; u < kListWalks; u++) {
                li[u] = (iw - first) * epi + u * 64u + (threadIdx.x & 63u);
                live[u] = (threadIdx.x & 63u) + u * 64u < epi && li[u] < n_l;
                if (live[u] && a.need_in != nullptr) live[u] = ((a.need_in[li[u]] >> a.need_bit) & 1u) != 0;  // (a sharing gap pass: none of its factors fired here)
                r[u] = live[u] ? (a.req_list != nullptr ? a.req_list[li[u]] : li[u]) : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < kListWalks; u++) {
                if (live[u] && a.visited != nullptr) atomicOr(&a.visited[r[u] >> 5], 1u << (r[u] & 31));
                p[u] = live[u] ? a.off[r[u]] : 0u;
                end[u] = live[u] ? a.off[r[u] + 1] : 0u;
                state[u] = 0;
                h[u] = Hits{0, 0, kNone};
                need_init[u] = 0;
                if (live[u] && a.merge_rec) {  // (the walk of a pass with a confirm tier: the record holds the heads' and the literals' hits)
                    h[u] = hits_of_record(a.rec[r[u]]);
                    if (a.colmask_local != nullptr && (h[u].a0 | (h[u].ovf + 1u)) != 0) need_init[u] = gate_mask(a.colmask_local, a.pool, h[u]);
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < kListWalks; u++) {
                if (live[u] && a.emit_off[1] != a.emit_off[0]) h[u] = emit_list(a.emit_off, a.emit_list, a.pool, a.pool_count, a.status, a.pool_cap, 0u, h[u]);
                w[u] = *reinterpret_cast<const PWAF_GLOBAL u32x4_u *>(gdata + p[u]);
            }
            // what entering state `st` emits rides in its row: a single atom that is already in the record, or fits a free slot, is
            // settled in registers (no memory access at all for a hot row)
            auto record_emit = [&](const uint32_t st, Hits &hh) {
                const uint32_t ei = st * stride + ncls;
                const uint32_t code = ei < hot_elems ? (uint32_t)hot[ei] : (uint32_t)flat[ei];
                const uint32_t x = (code & 0x7FFFu) + 1u;
                bool slow = !(code & 0x8000u) || hh.ovf != kNone;
                if (!slow) {
                    if (hh.a0 == x || hh.a1 == x) {}
                    else if (hh.a0 == 0) hh.a0 = x;
                    else if (hh.a1 == 0) hh.a1 = x;
                    else slow = true;
                }
                if (slow) hh = emit_list(a.emit_off, a.emit_list, a.pool, a.pool_count, a.status, a.pool_cap, st, hh);
            };
            // Per byte the walk is mad -> min -> ds_read -> and, in groups of four steps checked once: a step into a cold row reads the
            // sentinel (and stays there for the rest of the group), a step into an emitting state carries bit 15; bytes past the field's
            // end take the STAY cell, so no step is conditional. Only a group that met a cold cell is re-walked step by step (both walks
            // of the lane together: their L2 loads are issued back to back); emits are recorded after the group, off the chain. The next
            // 16-byte window of each walk is in flight while this one is walked. (Round 2: ~25 instructions and three branches per byte,
            // and a full global round trip per window on the critical path.)
            for (;;) {
                bool more = false;
#pragma unroll
                for (uint32_t u = 0; u < kListWalks; u++) more = more || p[u] < end[u];
                if (!more) break;
                u32x4 wn[kListWalks];
                uint32_t cnt[kListWalks];
                bool lead_here = false;  // scalar mode: some walk's window holds a byte beyond ASCII (wave-uniform after the ballot)
#pragma unroll
                for (uint32_t u = 0; u < kListWalks; u++) {
                    const uint32_t pn = p[u] + 16u;
                    wn[u] = *reinterpret_cast<const PWAF_GLOBAL u32x4_u *>(gdata + (pn < end[u] ? pn : 0u));
                    cnt[u] = p[u] < end[u] ? min(16u, end[u] - p[u]) : 0u;
                    if (a.umap != nullptr) lead_here = lead_here || (cnt[u] != 0u && window_has_high(w[u]));
                }
                const bool fix_classes = a.umap != nullptr && __ballot(lead_here) != 0ull;
#pragma unroll
                for (uint32_t k0 = 0; k0 < 16; k0 += 4) {
                    uint32_t c[kListWalks][4], t[kListWalks][4], sv[kListWalks][4];
#pragma unroll
                    for (uint32_t u = 0; u < kListWalks; u++) {
                        const uint32_t wd = k0 == 0 ? w[u].x : k0 == 4 ? w[u].y : k0 == 8 ? w[u].z : w[u].w;
#pragma unroll
                        for (uint32_t k = 0; k < 4; k++) {
                            const uint32_t cl = cls[(wd >> (k * 8)) & 0xFFu];
                            c[u][k] = k0 + k < cnt[u] ? cl : ncls + 1u;
                        }
                        if (fix_classes) {  // (uniform, rare) a lead byte reads as the class of the scalar value it begins; its continuation bytes stay, a stray one is ill-formed
#pragma unroll
                            for (uint32_t k = 0; k < 4; k++) {
                                const uint32_t byte = (wd >> (k * 8)) & 0xFFu;
                                if (byte >= 0xC0u && k0 + k < cnt[u]) c[u][k] = lead_class(a.umap, a.ill_class, gdata, byte, p[u] + k0 + k, end[u]);
                                else if (byte >= 0x80u && k0 + k < cnt[u]) c[u][k] = cont_class(c[u][k], a.ill_class, gdata, p[u] + k0 + k, live[u] ? a.off[r[u]] : 0u, end[u]);
                            }
                        }
                    }
#pragma unroll
                    for (uint32_t k = 0; k < 4; k++) {
#pragma unroll
                        for (uint32_t u = 0; u < kListWalks; u++) {
                            // per step: v_mad_u32_u24 (a 32-bit multiply is quarter rate) -> v_min -> ds_read_u16 -> v_and, all in BYTE offsets
                    t[u][k] = *reinterpret_cast<lds_u16_ptr>((uintptr_t)min(__umul24(k == 0 ? state[u] : sv[u][k - 1], 2u * stride) + 2u * c[u][k], 2u * hot_elems));  // (the hot rows start at LDS address 0)
                            sv[u][k] = t[u][k] & 0x7FFFu;
                        }
                    }
                    uint32_t any = 0, top = 0;
#pragma unroll
                    for (uint32_t u = 0; u < kListWalks; u++)
#pragma unroll
                        for (uint32_t k = 0; k < 4; k++) { any |= t[u][k]; top = max(top, t[u][k]); }
                    if (any & 0x8000u) {
                        if (top == 0xFFFFu) {
                            // a cold cell: the group step by step for both walks, cold cells from the L2-resident table
#pragma unroll
                            for (uint32_t k = 0; k < 4; k++) {
#pragma unroll
                                for (uint32_t u = 0; u < kListWalks; u++) {
                                    const uint32_t tt = list_step_slow(hot, flat, delta_lds, state[u], c[u][k], stride, a.n_hot, a.n_delta);
                                    state[u] = tt & 0x7FFFu;
                                    if (tt & 0x8000u) record_emit(state[u], h[u]);
                                }
                            }
                        } else {
#pragma unroll
                            for (uint32_t u = 0; u < kListWalks; u++) {
#pragma unroll
                                for (uint32_t k = 0; k < 4; k++)
                                    if (t[u][k] & 0x8000u) record_emit(sv[u][k], h[u]);
                                state[u] = sv[u][3];
                            }
                        }
                    } else {
#pragma unroll
                        for (uint32_t u = 0; u < kListWalks; u++) state[u] = sv[u][3];
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < kListWalks; u++) {
                    if (p[u] < end[u]) p[u] += 16u;
                    w[u] = wn[u];
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < kListWalks; u++) {
                if (!live[u]) continue;
                if (a.end_off[state[u] + 1] != a.end_off[state[u]]) h[u] = emit_list(a.end_off, a.end_list, a.pool, a.pool_count, a.status, a.pool_cap, state[u], h[u]);
                a.rec[r[u]] = record_of_hits(h[u]);
                if (a.colmask_local != nullptr) {
                    uint32_t need = 0;
                    if ((h[u].a0 | (h[u].ovf + 1u)) != 0) need = gate_mask(a.colmask_local, a.pool, h[u]);
                    if (a.need_out != nullptr) a.need_out[li[u]] = need;
                    need &= ~(a.shared_bits | need_init[u]);
                    if (need) enqueue_mask_once(a.gate_lists, a.gate_count, a.n, r[u], need, a.enq_bits, a.enq_words);
                }
            }
        }
        it = it_end;
    }
}

static const void *lscan_fn(bool wide) { return wide ? reinterpret_cast<const void *>(lscan_kernel<1024>) : reinterpret_cast<const void *>(lscan_kernel<512>); }

int launch_scan_gated(const ListScanArgs *host, uint32_t count, const ListScanArgs *dev, uint32_t *plan, const ListShape &shape, void *stream) {
    if (count == 0 || host[0].n == 0) return 0;
    if (count > 256) return (int)hipErrorInvalidValue;
    GatedTable b{dev, count, 0u};
#ifdef PWAF_PROFILING
    static const uint32_t async_mode = getenv("PWAF_LSCAN_ASYNC") ? (uint32_t)atoi(getenv("PWAF_LSCAN_ASYNC")) : 0u;
    b.debug = async_mode;
#endif
    // persistent grid: what the chip holds at this LDS size (the work items are split evenly over it)
    const uint32_t blocks = std::max(1u, host[0].n_cus) * shape.wg_per_cu;
    hipLaunchKernelGGL(lscan_plan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, b, plan, blocks * (shape.threads / 64u));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const uint32_t *cplan = plan;
    uint32_t hot_bytes = list_hot_bytes(shape);
    void *args[] = {&b, &cplan, &hot_bytes};
    const void *fn = lscan_fn(shape.threads == 1024);
    e = hipLaunchKernel(fn, dim3(blocks), dim3(shape.threads), args, shape.hot_bytes + 16 + 256, (hipStream_t)stream);
    return (int)(e != hipSuccess ? e : hipGetLastError());
}

// (LDS budget of the list scan — 160 KiB per CU shared by wg_per_cu workgroups, default 3 x (48 KiB, 512 threads) = 24 waves per CU — and
// the other shapes: list_shape, scanplan.cpp)

// Raises the dynamic-LDS limit of this unit's kernels on the current device (configure_kernels, kernels.hip): every scan_kernel launch
// and lscan_kernel's larger shapes take more than the 64 KiB default.
int configure_scan_kernels() {
    auto raise = [](const void *fn) { return (int)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerGroup); };
    for (const void *fn : kScanFns)
        if (int e = raise(fn)) return e;
    for (const bool wide : {false, true})
        if (int e = raise(lscan_fn(wide))) return e;
    return 0;
}

}  // namespace pwaf
