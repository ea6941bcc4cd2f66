// filter.hip — the bigram prefilter stage (kernels.h: FilterArgs; the tables: filter.cpp): filter_kernel streams the request bytes and
// flags chunks, resolve_kernel turns flagged chunks into candidate requests or (request, chunk) pairs, bitcount_kernel / compact_kernel
// turn the candidate bitmap into a dense list. Kernels first, in pipeline order; their launchers behind them. Pipeline overview: kernels.hip.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "kernels.h"
#include "wave.h"

namespace pwaf {

// -------------------------------------------------------------------------------------------------
// bigram prefilter
// -------------------------------------------------------------------------------------------------
// filter_kernel: the launch that streams the request bytes (kernels.h: the arena as one flat byte stream). Per input byte ONE
// independent LDS lookup — table[hash(fold(b[i]), fold(b[i+1]))] — and two vector ops: state = (state << 8) | mask, seen &= state.
// Nothing on the per-byte path depends on a previous lookup (the DFA walk it replaces chains v_lshl_add -> ds_read_u16 per byte plus
// a class lookup) and nothing depends on where requests begin or end. A zero bit in the top byte of `seen` after a 16-byte chunk =
// "some position of the chunk completed a window of some bucket"; the requests overlapping such chunks become CANDIDATES and are
// walked by the pass's DFA afterwards (lscan_kernel); every other request provably matches no pattern of the pass.
//
// Hash of a position = 12 bits of the 16-bit product fold(pair) * mul (program.h: filter_bin): two positions per v_pk_mul_lo_u16.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// STRIDE = 1: a bigram at every byte. STRIDE = 2: only at the even bytes of the arena stream (FilterArgs::stride, chosen per pass
// by the host: half the lookups; every factor is in the table once per alignment).
// The stream is laid out in ROWS: one iteration = 4 rows of 1 KiB, lane l of row q holds the 16-byte chunk at b + 1024 q + 16 l.
// Every load instruction is one contiguous KiB (round 2 gave every lane its own 64-byte segment: 64 lines per load instruction and
// two more scattered dword loads per lane for the bytes around the segment — the texture addresser, not LDS, bounded that kernel:
// 0.73 ms against 0.68 on the 10M-request batch, and stride 2 was no faster than stride 1); what a chunk needs from its
// neighbours travels through the wave instead of memory:
//   * the byte after the chunk (second half of its last bigram) = the first dword of lane l + 1's chunk (DPP wave_shl:1; lane 63:
//     lane 0 of the next row, a scalar),
//   * the shift-or state it starts from = what the three last bigrams of lane l - 1's chunk leave behind, which that lane computes
//     from its OWN lookups (two v_lshl_or_b32 — the state forgets everything older than four bigrams) and hands on (DPP
//     wave_shr:1; lane 0: lane 63 of the previous row, a scalar carried from row to row and iteration to iteration) —
//     no warm-up lookups at all.
// A row's registers are reloaded with the NEXT iteration's row as soon as its lookups are issued: 16 data registers instead of 36.
template <bool HEADS, int STRIDE>
__device__ __forceinline__ void filter_rows(const FilterArgs &a, const uint32_t blk, const uint32_t wave, const uint32_t lane) {
    const PWAF_GLOBAL unsigned char *gdata = (const PWAF_GLOBAL unsigned char *)a.data;
    const uint32_t rel = blk * kFilterWaves + wave, slab = a.slab0 + rel;
    const uint64_t base64 = (uint64_t)slab * kStreamSlab;
    if (base64 >= a.total) return;
    const uint32_t total = a.total, base0 = (uint32_t)base64, slab_end = (uint32_t)min<uint64_t>(total, base64 + kStreamSlab);
    unsigned long long *my_bits = reinterpret_cast<unsigned long long *>(a.chunk_bits) + (size_t)rel * (kStreamSlab / 1024);  // one 64-bit word per row
    uint32_t n_hit = 0;  // wave-uniform: flagged chunks of the slab
    const uint32_t mul2 = a.mul | (a.mul << 16);
    constexpr uint32_t kRow = 1024;

    auto load_row = [&](const uint32_t b, const uint32_t q) {
        const uint32_t p = b + kRow * q + 16u * lane;
        return *reinterpret_cast<const PWAF_GLOBAL u32x4_u *>(gdata + (p < total ? p : 0u));
    };
    auto dword_at = [&](const uint32_t p) {  // (wave-uniform address)
        return filter_fold4(*reinterpret_cast<const PWAF_GLOBAL uint32_t __attribute__((aligned(1))) *>(gdata + p));
    };
    // LDS byte offset of a bin = (16-bit product >> 4) * 4, for the two products of one v_pk_mul_lo_u16: ONE mask for both halves,
    // then one SDWA shift per half (v_lshrrev_b32 reading WORD_0 / WORD_1 zero-extended) — three instructions per two lookups where
    // a shift and a mask per lookup took four (a quarter of the loop's vector instructions).
    auto slot_lo = [](const uint32_t masked) {
        uint32_t r;
        asm("v_lshrrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(r) : "v"(masked));
        return r;
    };
    auto slot_hi = [](const uint32_t masked) {
        uint32_t r;
        asm("v_lshrrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(r) : "v"(masked));
        return r;
    };
    auto bins4 = [&](const uint32_t x, const uint32_t next, uint32_t (&mm)[4]) {  // the four bigrams that start in (case-folded) dword x
        const uint32_t z = __builtin_amdgcn_alignbit(next, x, 8);
        const uint32_t hx = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, x) * __builtin_bit_cast(u16x2, mul2));
        const uint32_t hz = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, z) * __builtin_bit_cast(u16x2, mul2));
#ifdef PWAF_PROFILING
        if (a.debug & 1u) { mm[0] = hx | 0xFF000000u; mm[1] = hz | 0xFF000000u; mm[2] = (hx >> 3) | 0xFF000000u; mm[3] = (hz >> 5) | 0xFF000000u; return; }
#endif
        const uint32_t kx = hx & 0xFFF0FFF0u, kz = hz & 0xFFF0FFF0u;
        mm[0] = *reinterpret_cast<lds_u32_ptr>((uintptr_t)slot_lo(kx));
        mm[1] = *reinterpret_cast<lds_u32_ptr>((uintptr_t)slot_lo(kz));
        mm[2] = *reinterpret_cast<lds_u32_ptr>((uintptr_t)slot_hi(kx));
        mm[3] = *reinterpret_cast<lds_u32_ptr>((uintptr_t)slot_hi(kz));
    };
    auto bins2 = [&](const uint32_t x, uint32_t (&mm)[2]) {  // the two bigrams at the even bytes of (case-folded) dword x
        const uint32_t hx = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, x) * __builtin_bit_cast(u16x2, mul2));
#ifdef PWAF_PROFILING
        if (a.debug & 1u) { mm[0] = hx | 0xFF000000u; mm[1] = (hx >> 3) | 0xFF000000u; return; }
#endif
        const uint32_t kx = hx & 0xFFF0FFF0u;
        mm[0] = *reinterpret_cast<lds_u32_ptr>((uintptr_t)slot_lo(kx));
        mm[1] = *reinterpret_cast<lds_u32_ptr>((uintptr_t)slot_hi(kx));
    };
    auto push = [](uint32_t &st, const uint32_t m) { asm("v_lshl_or_b32 %0, %1, 8, %2" : "=v"(st) : "v"(st), "v"(m)); };

    // heads: the wave walks the offsets column alongside the bytes; rq = first request that starts at or after the current byte.
    // Software-pipelined so that nothing on this path waits for memory: the offsets of the next 128 requests are requested one
    // iteration ahead; the first 16 bytes of the requests that start inside the current iteration (bytes this wave has just
    // streamed: cache hits) are requested BEFORE the rows are looked up and compared after them. (The first version — a loop of
    // dependent loads per iteration — cost 0.20 ms of a 0.88 ms launch.)
    uint32_t rq = 0, ho[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, hn[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    auto load_offs = [&](const uint32_t r0) {
        // off[n] = the arena's size, which no iteration's limit exceeds: an index clamped to n reads as "starts beyond". A request's
        // end is its right-hand neighbour's start: one load per request, the neighbour's through DPP (lane 63: the next block's first).
        ho[0] = a.off[min(r0 + lane, a.n)];
        ho[1] = a.off[min(r0 + 64u + lane, a.n)];
        const uint32_t e1 = a.off[min(r0 + 128u, a.n)];  // (wave-uniform address)
        hn[0] = (uint32_t)__builtin_amdgcn_update_dpp(__builtin_amdgcn_readfirstlane((int)ho[1]), (int)ho[0], 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
        hn[1] = (uint32_t)__builtin_amdgcn_update_dpp(__builtin_amdgcn_readfirstlane((int)e1), (int)ho[1], 0x130, 0xF, 0xF, false);
    };
    auto head_record = [&](const u32x4 w, const uint32_t flen) {
        uint32_t hrec = 0;
#pragma unroll
        for (int hq = 0; hq < 2; hq++) {
            if ((uint32_t)hq < a.n_heads) {
                const uint32_t diff = ((w.x ^ a.head_w[hq][0]) & a.head_m[hq][0]) | ((w.y ^ a.head_w[hq][1]) & a.head_m[hq][1]) |
                                      ((w.z ^ a.head_w[hq][2]) & a.head_m[hq][2]) | ((w.w ^ a.head_w[hq][3]) & a.head_m[hq][3]);
                const uint32_t hl = a.head_len[hq] & 0xFFu;
                const bool len_ok = (a.head_len[hq] >> 8) ? flen == hl : flen >= hl;
                if (diff == 0 && len_ok) hrec |= a.head_code[hq];
            }
        }
        return hrec;
    };
    const bool heads = HEADS && a.n_heads != 0;
    if (heads) {
        // lower bound of base0 in off[0, n): a 64-ary search like resolve_kernel's — every lane probes one of 64 evenly spaced offsets, a ballot narrows
        // the range 64-fold (4 dependent loads for 10M requests where the binary search took 23)
        uint32_t lo = 0, hi = a.n;  // the answer lies in [lo, hi]
        while (lo < hi) {
            const uint32_t span = hi - lo, step = (span + 63) / 64;
            const uint32_t probe = lo + lane * step;
            const bool ok = probe >= hi || a.off[probe] >= base0;  // monotone in the lane index
            const unsigned long long m = __ballot(ok);
            if (m == 0) {  // all 64 probes fail: the answer lies beyond the last one
                lo += 63u * step + 1u;
                continue;
            }
            const uint32_t f = (uint32_t)__builtin_ctzll(m);
            const uint32_t nh = min(hi, lo + f * step);  // probe f holds (or is past the range)
            lo = f == 0 ? lo : lo + (f - 1u) * step + 1u;  // probe f - 1 fails
            hi = nh;
        }
        rq = lo;
        load_offs(rq);
    }

    // the state the slab's first chunk starts from: the three sampled bigrams before the slab (none at the very start of the arena)
    uint32_t carry = a.init;  // wave-uniform
    if (STRIDE == 1) {
        if (base0 >= 4) {
            uint32_t mw[4];
            bins4(dword_at(base0 - 4), dword_at(base0), mw);
            push(carry, mw[1]); push(carry, mw[2]); push(carry, mw[3]);
        }
    } else if (base0 >= 8) {
        uint32_t m0[2], m1[2];
        bins2(dword_at(base0 - 8), m0);
        bins2(dword_at(base0 - 4), m1);
        push(carry, m0[1]); push(carry, m1[0]); push(carry, m1[1]);
    }
    carry = __builtin_amdgcn_readfirstlane(carry);
    // the dword after the slab (second byte of the slab's last bigram)
    const uint32_t after = (STRIDE == 1 && slab_end < total) ? __builtin_amdgcn_readfirstlane(dword_at(slab_end)) : 0u;

    u32x4 w[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) w[q] = load_row(base0, q);
    for (uint32_t b = base0; b < slab_end; b += kStreamIter) {
        const bool more = b + kStreamIter < slab_end;  // wave-uniform
        u32x4 hw[2];
        uint32_t hlen[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
        uint32_t rq_here = rq;
#ifdef PWAF_PROFILING
        if (heads && !(a.debug & 4u)) {
#else
        if (heads) {
#endif
            const uint32_t lim = min(b + kStreamIter, slab_end);
            const bool in0 = ho[0] < lim;
            const uint32_t c0 = (uint32_t)__builtin_popcountll(__ballot(in0));
            if (in0) {  // (only the lanes that hold a request of this iteration issue an address)
                hw[0] = *reinterpret_cast<const PWAF_GLOBAL u32x4_u *>(gdata + ho[0]);
                hlen[0] = hn[0] - ho[0];
            }
            uint32_t c1 = 0;
            if (c0 == 64) {  // (wave-uniform: the second gather is issued only when more than 64 requests start in these 4 KiB)
                const bool in1 = ho[1] < lim;
                c1 = (uint32_t)__builtin_popcountll(__ballot(in1));
                if (in1) {
                    hw[1] = *reinterpret_cast<const PWAF_GLOBAL u32x4_u *>(gdata + ho[1]);
                    hlen[1] = hn[1] - ho[1];
                }
            }
            rq += c0 + c1;
            if (c0 + c1 == 128) {
                for (;;) {  // more than 128 requests start within 4 KiB (very short fields): the rest synchronously
                    const uint32_t idx = rq + lane;
                    const uint32_t s = a.off[min(idx, a.n)];
                    const bool in = s < lim;
                    const uint32_t cnt = (uint32_t)__builtin_popcountll(__ballot(in));
                    if (in) {
                        a.rec[idx] = head_record(*reinterpret_cast<const PWAF_GLOBAL u32x4_u *>(gdata + s), a.off[idx + 1] - s);
                    }
                    rq += cnt;
                    if (cnt < 64) break;
                }
            }
            load_offs(rq);  // for the next iteration
        }

        unsigned long long hm[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            const uint32_t x0 = filter_fold4(w[q].x), x1 = filter_fold4(w[q].y), x2 = filter_fold4(w[q].z), x3 = filter_fold4(w[q].w);  // (program.h: letters lose their case, nothing below 0x40 moves)
            uint32_t st, seen = 0xFFFFFFFFu, tail;
            if (STRIDE == 1) {
                // lane 63's next dword: lane 0 of the next row (row 0 already holds the NEXT iteration's chunk; the slab's last row: `after`)
                const uint32_t first_next = (q == 3 && !more) ? after : filter_fold4(__builtin_amdgcn_readfirstlane(w[(q + 1) & 3].x));
                const uint32_t x4 = (uint32_t)__builtin_amdgcn_update_dpp((int)first_next, (int)x0, 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
                uint32_t m[16];
                {
                    uint32_t mm[4];
                    bins4(x0, x1, mm); m[0] = mm[0]; m[1] = mm[1]; m[2] = mm[2]; m[3] = mm[3];
                    bins4(x1, x2, mm); m[4] = mm[0]; m[5] = mm[1]; m[6] = mm[2]; m[7] = mm[3];
                    bins4(x2, x3, mm); m[8] = mm[0]; m[9] = mm[1]; m[10] = mm[2]; m[11] = mm[3];
                    bins4(x3, x4, mm); m[12] = mm[0]; m[13] = mm[1]; m[14] = mm[2]; m[15] = mm[3];
                }
#ifdef PWAF_PROFILING
                if (more && !(a.debug & 2u)) w[q] = load_row(b + kStreamIter, q);
#else
                if (more) w[q] = load_row(b + kStreamIter, q);
#endif
                tail = m[13]; push(tail, m[14]); push(tail, m[15]);
                st = (uint32_t)__builtin_amdgcn_update_dpp((int)carry, (int)tail, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
#pragma unroll
                for (int i = 0; i < 16; i++) { push(st, m[i]); seen &= st; }
            } else {
                uint32_t m[8];
                {
                    uint32_t mm[2];
                    bins2(x0, mm); m[0] = mm[0]; m[1] = mm[1];
                    bins2(x1, mm); m[2] = mm[0]; m[3] = mm[1];
                    bins2(x2, mm); m[4] = mm[0]; m[5] = mm[1];
                    bins2(x3, mm); m[6] = mm[0]; m[7] = mm[1];
                }
#ifdef PWAF_PROFILING
                if (more && !(a.debug & 2u)) w[q] = load_row(b + kStreamIter, q);
#else
                if (more) w[q] = load_row(b + kStreamIter, q);
#endif
                tail = m[5]; push(tail, m[6]); push(tail, m[7]);
                st = (uint32_t)__builtin_amdgcn_update_dpp((int)carry, (int)tail, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
#pragma unroll
                for (int i = 0; i < 8; i++) { push(st, m[i]); seen &= st; }
            }
            carry = __builtin_amdgcn_readlane(tail, 63);
            const bool hit = ((~seen) & 0xFF000000u) != 0 && b + kRow * q + 16u * lane < total;
            hm[q] = __ballot(hit);  // bit l = the row's chunk l: the row's word of the pass's chunk bitmap as it is
            __builtin_amdgcn_sched_barrier(0);
        }
        // the iteration's four words: one 32-byte store
        if (lane < 4) my_bits[(b - base0) / kRow + lane] = lane == 0 ? hm[0] : lane == 1 ? hm[1] : lane == 2 ? hm[2] : hm[3];
        n_hit += (uint32_t)(__builtin_popcountll(hm[0]) + __builtin_popcountll(hm[1]) + __builtin_popcountll(hm[2]) + __builtin_popcountll(hm[3]));

        if (heads) {  // the record of EVERY request of the iteration, zero included: nothing clears these records in front of the batch
#pragma unroll
            for (uint32_t q = 0; q < 2; q++)
                if (hlen[q] != 0xFFFFFFFFu) a.rec[rq_here + 64u * q + lane] = head_record(hw[q], hlen[q]);
        }
    }
    // The requests no iteration enumerates start AT off[n]: empty fields at the arena's end. The wave of the arena's last slab writes
    // their (zero) records. (An arena without a slab — every field empty — has no wave: the host clears that pass, engine.cpp.)
#ifdef PWAF_PROFILING
    if (heads && !(a.debug & 4u) && slab_end == total)
#else
    if (heads && slab_end == total)
#endif
        for (uint32_t idx = rq + lane; idx < a.n; idx += 64) a.rec[idx] = 0u;
    // (the arena's last slab: the words of the iterations it does not have read as "no chunk flagged")
    for (uint32_t wd = (slab_end - base0 + kStreamIter - 1) / kStreamIter * 4 + lane; wd < kStreamSlab / kRow; wd += 64) my_bits[wd] = 0;
    if (lane == 0) {
        a.sub_count[rel] = n_hit;
        // where the slab's pairs begin in the pass's pair list: one returned atomic per slab, here at the slab's end (round 6; until then a scan
        // kernel of its own between this launch and resolve_kernel: 7 us + a launch gap on the critical path. The same atomic taken by
        // resolve_kernel's waves as they START held every one of them up for its turn — here the slabs end spread over the launch). The order
        // of a pass's pairs no longer follows the arena; nothing reads it as ordered.
        if (a.pairs != nullptr) a.pair_base[rel] = n_hit ? atomicAdd(a.pair_count, n_hit) : 0u;
    }
}

// ONE launch for every filtered pass, both strides: stride-1 passes are bound by the LDS lookups, stride-2 passes by HBM, so their
// workgroups are INTERLEAVED in proportion (block i is the floor(i * n1 / N)-th stride-1 block if that count steps at i, else the
// next stride-2 block) and every CU holds both kinds at any time — one launch per stride ran them one after the other, each
// phase leaving the other resource idle.
template <bool HEADS>
__global__ __launch_bounds__(kFilterWaves * 64) void filter_kernel(FilterMix M) {
    extern __shared__ __align__(16) unsigned char lds[];
    __builtin_amdgcn_s_setprio(3);
    const uint32_t n_all = M.blocks1 + M.blocks2;
    const uint32_t before = (uint32_t)(((uint64_t)blockIdx.x * M.blocks1) / n_all), upto = (uint32_t)(((uint64_t)(blockIdx.x + 1) * M.blocks1) / n_all);
    const bool one = upto > before;  // a stride-1 block
    const uint32_t blk = one ? before : blockIdx.x - before;
    const FilterArgs *tab = one ? M.f1 : M.f2;
    // which pass of its class this workgroup belongs to (uniform: the last pass whose first_block is <= blk)
    uint32_t k = 0;
    for (uint32_t lo = 0, hi = one ? M.count1 : M.count2; lo + 1 < hi;) {
        const uint32_t mid = (lo + hi) >> 1;
        if (blk >= tab[mid].first_block) lo = mid;
        else hi = mid;
        k = lo;
    }
    const FilterArgs a = load_descriptor(&tab[k]);
    const uint32_t tid = threadIdx.x, wave = wave_index(), lane = tid & 63;
    // (Bank-private replicas of the table — 4 copies, each lane group of 8 with 8 banks of its own — were measured SLOWER: 1.19 ms
    // against 0.89 ms. A ds_read_b32 takes as many cycles as its most loaded bank over all 32 lanes, and the maximum over four
    // groups of 8-in-8 is hardly below 32-in-32, while 64 KiB per workgroup halves the occupancy.)
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.table);
        uint4 *dst = reinterpret_cast<uint4 *>(lds);
        for (uint32_t i = tid; i < kFilterEntries / 4; i += kFilterWaves * 64) dst[i] = src[i];
    }
    __syncthreads();
    // (no static LDS in this kernel: the table starts at LDS address 0 and lookups use plain integer addresses)
    if ((uint32_t)(uintptr_t)(PWAF_LDS unsigned char *)lds != 0u) __builtin_trap();
    if (one) filter_rows<HEADS, 1>(a, blk - a.first_block, wave, lane);
    else filter_rows<HEADS, 2>(a, blk - a.first_block, wave, lane);
}

// (Ahead of the definition on purpose. The instantiations take their attributes from THIS first declaration, which names no __launch_bounds__: the
// definition's (256) does not apply, the kernel is compiled for workgroups of up to 1024 threads. DESIGN.md §0.6.)
template <uint32_t PARTS>
__global__ void resolve_kernel(FilterTable B);
// ... which holds for an instantiation that is first NAMED while that declaration is the only one in sight: named behind the definition it takes
// the definition's bound, and the register allocation changes. So the two instantiations are named here, once; launch_resolve picks from the table. [PARTS == 4]
static const void *const kResolveFns[2] = {reinterpret_cast<const void *>(resolve_kernel<1>), reinterpret_cast<const void *>(resolve_kernel<4>)};

// resolve_kernel: one wave per slab turns the slab's flagged chunks into candidate REQUESTS. Request-driven: the flagged 16-byte
// chunks of the slab become a bitmap in LDS (8192 bits) with per-word prefix counts, then the wave walks the requests that overlap
// the slab — 64 per step, offsets read coalesced — and a request is a candidate when a flagged chunk lies within its bytes extended
// by what a window may reach back (three sampled bigrams) and forward (one byte): two rank queries. Slabs without a hit leave at
// once. (The first version searched the offsets per HIT: 23 dependent loads each and an atomic per marked request — 0.07 ms on
// benign traffic, 1.4 ms when most segments are flagged.)
// PARTS: waves per slab (round 6). A slab's wave walks every request that overlaps its 128 KiB — 64 per step, one round trip each; when the batch's
// slabs do not fill the chip (a 1.25M-request share: 2 700) the launch takes what its longest walk takes, 44 us. With PARTS = 4 every wave ranks the
// whole slab's bitmap (1 KiB) but walks only the requests of ITS quarter and lists only the flagged chunks of its quarter — their places in the pair
// list are ranks within the slab, as before.
template <uint32_t PARTS>
__global__ __launch_bounds__(256) void resolve_kernel(FilterTable B) {
    __builtin_amdgcn_s_setprio(3);
    constexpr uint32_t kChunks = kStreamSlab / 16, kWords = kChunks / 32;  // 8192 chunk bits = 256 words per slab
    constexpr uint32_t kResolveSparse = 128;  // flagged chunks up to which a slab is resolved chunk by chunk (two rounds of 64 lanes)
    __shared__ uint32_t s_bits[4][kWords], s_rank[4][kWords];
    const FilterArgs *pa = &B.f[blockIdx.y];
    if ((uint64_t)(pa->slab0 + blockIdx.x * 4 / PARTS) * kStreamSlab >= pa->total) return;  // (the whole workgroup is past the pass's last slab)
    const FilterArgs a = load_descriptor(pa);
    if (a.dense_flag != nullptr && *a.dense_flag > a.dense_thresh) return;  // (the pass is walked whole this batch: no pairs, no records to reset)
    const uint32_t wave = wave_index(), rel = (blockIdx.x * 4 + wave) / PARTS, part = (blockIdx.x * 4 + wave) % PARTS, slab = a.slab0 + rel, lane = threadIdx.x & 63;
    constexpr uint32_t kPartChunks = kChunks / PARTS;
    if ((uint64_t)slab * kStreamSlab >= a.total) return;
    const uint32_t cnt = a.sub_count[rel];
    if (cnt == 0) return;
    // a slab with few flagged chunks is resolved chunk by chunk (below) by ONE wave, whatever PARTS: the others of its four leave
    const bool sparse = a.pairs != nullptr && cnt <= kResolveSparse;
    if (sparse && part != 0u) return;
    const uint32_t lo_c = sparse ? 0u : part * kPartChunks, hi_c = sparse ? kChunks : lo_c + kPartChunks;  // the wave's chunks of the slab, slab-relative
    const uint32_t *slab_bits = a.chunk_bits + (size_t)rel * kWords;
    uint32_t *bits = s_bits[wave], *rank = s_rank[wave];
    // 1. the slab's part of the pass's chunk bitmap (filter_kernel wrote it, one 64-bit word per KiB row), prefix popcounts per word
#pragma unroll
    for (uint32_t q = 0; q < kWords / 64; q++) bits[q * 64 + lane] = slab_bits[q * 64 + lane];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    {
        uint32_t w[kWords / 64], mine = 0;
#pragma unroll
        for (uint32_t q = 0; q < kWords / 64; q++) {
            w[q] = bits[lane * (kWords / 64) + q];
            mine += (uint32_t)__builtin_popcount(w[q]);
        }
        uint32_t before = wave_scan_add(mine) - mine;
#pragma unroll
        for (uint32_t q = 0; q < kWords / 64; q++) {
            rank[lane * (kWords / 64) + q] = before;
            before += (uint32_t)__builtin_popcount(w[q]);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    auto rank_of = [&](const uint32_t c) {  // flagged chunks among the slab's chunks [0, c), c <= kChunks
        if (c >= kChunks) return rank[kWords - 1] + (uint32_t)__builtin_popcount(bits[kWords - 1]);
        return rank[c >> 5] + (uint32_t)__builtin_popcount(bits[c >> 5] & ((1u << (c & 31u)) - 1u));
    };
    // 2. the requests overlapping the slab's bytes (extended by the reach of a window), in order
    const uint32_t back = 3u * a.stride;
    const uint64_t slab_b0 = (uint64_t)slab * kStreamSlab, b0 = slab_b0 + (uint64_t)lo_c * 16u;  // (b0: the first byte of the wave's part)
    const uint32_t c_first = (uint32_t)(slab_b0 / 16);  // global index of the slab's first chunk
    // first request with off[r + 1] + back > b0: a 64-ary search — every lane probes one of 64 evenly spaced offsets, a ballot
    // narrows the range 64-fold per step (4 dependent loads for 10M requests; the binary search this replaces took 23, about
    // 10 us of every wave's life in a kernel that is nothing but latency)
    uint32_t lo = 0, hi = a.n;  // the answer lies in [lo, hi]; index a.n stands for "none" (treated as satisfying the predicate)
    while (lo < hi) {
        const uint32_t span = hi - lo, step = (span + 63) / 64;
        const uint32_t probe = lo + lane * step;
        const bool ok = probe >= hi || (uint64_t)a.off[probe + 1] + back > b0;  // monotone in the lane index
        const unsigned long long m = __ballot(ok);
        if (m == 0) {  // all 64 probes fail: the answer lies beyond the last one
            lo += 63u * step + 1u;
            continue;
        }
        const uint32_t f = (uint32_t)__builtin_ctzll(m);
        const uint32_t nh = min(hi, lo + f * step);  // probe f holds (or is past the range)
        lo = f == 0 ? lo : lo + (f - 1u) * step + 1u;  // probe f - 1 fails
        hi = nh;
    }
    const uint64_t b1 = slab_b0 + (uint64_t)hi_c * 16u;  // requests starting at or beyond b1 + 16 cannot be reached by this part's chunks
    // A pass with a confirm tier lists its flagged chunks instead of marking candidates: every flagged chunk of the slab becomes ONE pair
    // {the request that owns the chunk's first byte, chunk}. The slab's pairs take a contiguous part of the pass's pair list — it begins
    // where filter_kernel's atomic on the list's length put it as the slab ended (pair_base; the same atomic taken HERE, ~20k returned
    // same-address atomics as these waves start, held every wave up for its turn) — and a chunk's place in it is its rank among the
    // slab's flagged chunks (the prefix counts above): no second walk.
    const uint32_t pair_base = a.pairs != nullptr ? a.pair_base[rel] : 0u;
    const uint32_t begin = __builtin_amdgcn_readfirstlane(a.off[0]);  // != 0: a slab view of a larger arena
    // A slab view keeps absolute arena positions and the filter streams whole slabs: what lies before off[0] in the view's first slab —
    // another view's requests, stale staging bytes — may have flagged chunks that NO request of this batch owns. Their slots of the pair
    // list are filled with "no pair" here (confirm_kernel skips those; left unwritten they would be read as stale {request, chunk}
    // pairs: ADVICE r4). Only the chunks that end at or before off[0]: the chunk that holds off[0] belongs to the first request.
    if (part == 0 && a.pairs != nullptr && (uint64_t)begin > slab_b0) {
        const uint32_t n_before = min((uint32_t)(((uint64_t)begin - slab_b0) >> 4), kChunks);  // chunks [0, n_before) of this slab lie wholly before off[0]
        for (uint32_t w = lane; w * 32u < n_before; w += 64) {
            uint32_t bw = bits[w];
            if (n_before - w * 32u < 32u) bw &= (1u << (n_before - w * 32u)) - 1u;
            const uint32_t word = bits[w];
            while (bw) {
                const uint32_t bit = (uint32_t)__builtin_ctz(bw);
                bw &= bw - 1u;
                const uint32_t at = pair_base + rank[w] + (uint32_t)__builtin_popcount(word & ((1u << bit) - 1u));
                if (at < a.pair_cap) a.pairs[at] = make_uint2(kNone, 0u);
            }
        }
    }
    // CHUNK-DRIVEN (round 6): a slab with few flagged chunks — a benign 10M-request batch of the 1k-rule set leaves 404k pairs in 21 600 slabs, 19 per
    // slab — does not walk its 1 300 - 2 900 requests, 64 per dependent round trip, to find the owners of 19 chunks: lane k takes the slab's k-th flagged
    // chunk (the rank table gives the word, the word the bit), finds the request that holds the chunk's first byte by a binary search of the offsets
    // (within 4096 requests of the slab's first: a dozen dependent loads, all lanes at once), writes the pair at ITS place (pair_base + k) and resets the
    // records of the requests that overlap the chunk. A slab the bounds do not fit (fields shorter than 32 bytes on average, runs of empty fields) falls
    // through to the request-driven walk below, which writes the same values.
    if (sparse) {
        bool redo = false;
        for (uint32_t k = lane; k < cnt; k += 64) {
            uint32_t wlo = 0, whi = kWords;  // the last word w with rank[w] <= k holds the k-th flagged chunk
            while (wlo + 1u < whi) {
                const uint32_t mid = (wlo + whi) >> 1;
                if (rank[mid] <= k) wlo = mid;
                else whi = mid;
            }
            uint32_t word = bits[wlo];
            for (uint32_t skip = k - rank[wlo]; skip != 0u; skip--) word &= word - 1u;
            const uint32_t chunk = c_first + wlo * 32u + (uint32_t)__builtin_ctz(word), byte0 = chunk * 16u;
            if (byte0 + 16u <= begin) continue;  // (wholly before off[0]: "no pair", written above)
            const uint32_t key = max(byte0, begin);  // (the chunk that holds off[0] belongs to the first request that has bytes)
            uint32_t l = lo, h = min(a.n, lo + 4096u);  // the first request with off[r + 1] > key, in [l, h]
            const uint32_t h0 = h;
            while (l < h) {
                const uint32_t mid = (l + h) >> 1;
                if (a.off[mid + 1] > key) h = mid;
                else l = mid + 1u;
            }
            if (l == h0) {  // not within the bound (or no request at all holds the byte: cannot be, the filter flags no chunk at or beyond off[n])
                if (h0 < a.n) { redo = true; continue; }
                if (pair_base + k < a.pair_cap) a.pairs[pair_base + k] = make_uint2(kNone, 0u);
                continue;
            }
            if (pair_base + k < a.pair_cap) a.pairs[pair_base + k] = make_uint2(l, chunk);
            if (a.n_heads == 0) {  // the requests with a byte in the chunk (their records are merged into by confirm_kernel: see below; a pass with heads: all written by filter_kernel)
                uint32_t r = l, steps = 0;
                for (; r < a.n && steps < 48u; r++, steps++) {
                    const uint32_t s = a.off[r];
                    if (s >= byte0 + 16u) break;
                    if (a.off[r + 1] > s) a.rec[r] = 0u;
                }
                if (steps == 48u) redo = true;  // (a run of empty fields)
            }
        }
        if (__ballot(redo) == 0ull) return;
    }
    {
    // (software-pipelined: the offsets of the next 64 requests are in flight while these are ranked)
    uint32_t s_n = 0xFFFFFFFFu, e_n = 0xFFFFFFFFu;
    {
        const uint32_t r = lo + lane;
        if (r < a.n) { s_n = a.off[r]; e_n = a.off[r + 1]; }
    }
    for (uint32_t rb = lo; rb < a.n; rb += 64) {
        const uint32_t r = rb + lane;
        const bool live = r < a.n;
        const uint32_t s = s_n, e = e_n;
        {
            const uint32_t r2 = r + 64;
            s_n = e_n = 0xFFFFFFFFu;
            if (r2 < a.n) { s_n = a.off[r2]; e_n = a.off[r2 + 1]; }
        }
        if (a.pairs != nullptr) {
            // A request with a flagged chunk among its own gets its hit record ZEROED here (confirm_kernel merges hits into it; the verdict
            // kernel only reads records whose valid bit a hit or a walk set — which implies a flagged chunk): one store per such request
            // instead of a memset of the pass's every record (69 passes x 4 MB per batch of the 4096-rule set). A pass with filter
            // heads needs neither: filter_kernel has stored the record of its every request, zero where no head holds, before this launch.
            if (a.n_heads == 0 && live && e > s) {
                const uint32_t g_lo = s >> 4, g_hi = (e - 1u) >> 4;
                if (g_hi >= c_first + lo_c && g_lo < c_first + hi_c) {
                    const uint32_t y0 = g_lo > c_first + lo_c ? g_lo - c_first : lo_c, y1 = min(g_hi - c_first, hi_c - 1u);
                    if (rank_of(y1 + 1u) != rank_of(y0)) a.rec[r] = 0u;
                }
            }
            // the flagged chunks whose first byte lies in this request (clipped to the slab). The chunk that holds off[0] when off[0] is
            // not a multiple of 16 (a slab view) begins before every request: it belongs to the first request that has bytes, which is
            // the one with s == off[0] < e (it used to have no owner, and a factor completing in the view's first bytes was
            // never confirmed).
            if (live && e > s) {
                const uint32_t f_lo = s == begin ? s >> 4 : (s + 15u) >> 4, f_hi = (e - 1u) >> 4;
                if (f_lo <= f_hi && f_hi >= c_first + lo_c && f_lo < c_first + hi_c) {
                    const uint32_t x0 = f_lo > c_first + lo_c ? f_lo - c_first : lo_c, x1 = min(f_hi - c_first, hi_c - 1u);
                    for (uint32_t w = x0 >> 5; w <= (x1 >> 5); w++) {
                        const uint32_t word = bits[w];
                        uint32_t bw = word;
                        if (w == (x0 >> 5)) bw &= ~0u << (x0 & 31u);
                        if (w == (x1 >> 5)) bw &= ~0u >> (31u - (x1 & 31u));
                        while (bw) {
                            const uint32_t bit = (uint32_t)__builtin_ctz(bw);
                            bw &= bw - 1u;
                            const uint32_t at = pair_base + rank[w] + (uint32_t)__builtin_popcount(word & ((1u << bit) - 1u));
                            if (at < a.pair_cap) a.pairs[at] = make_uint2(r, c_first + w * 32u + bit);
                        }
                    }
                }
            }
            if (__ballot(live && (uint64_t)s >= b1) != 0) break;  // (offsets ascend: no later request owns a byte of this slab)
            continue;
        }
        bool mark = false;
        if (live && (uint64_t)s < b1 + 16) {
            // chunks j with 16 j - back < e and 16 j + 16 >= s, clipped to the slab
            const uint32_t j_lo = s == 0 ? 0u : (s - 1u) / 16u, j_hi = (uint32_t)(((uint64_t)e + back - 1u) / 16u);
            const uint32_t x0 = j_lo > c_first + lo_c ? j_lo - c_first : lo_c;
            if (j_hi >= c_first + lo_c && x0 < hi_c) {
                const uint32_t x1 = min(j_hi - c_first, hi_c - 1u);
                mark = x0 <= x1 && rank_of(x1 + 1u) != rank_of(x0);
            }
        }
        // the wave's 64 verdicts as at most three bitmap words (rb is not word-aligned in general)
        const unsigned long long m = __ballot(mark);
        if (m != 0) {
            const uint32_t sh = rb & 31u, w0 = rb >> 5;
            const uint32_t parts[3] = {(uint32_t)(m << sh), (uint32_t)(sh ? m >> (32u - sh) : m >> 32), sh ? (uint32_t)(m >> (64u - sh)) : 0u};
            if (lane < 3 && parts[lane] != 0) atomicOr(&a.bitmap[w0 + lane], parts[lane]);
        }
        if (__ballot(live && (uint64_t)s >= b1 + 16) != 0) break;  // (offsets ascend: nothing further overlaps)
    }
    }
}

// bitcount_kernel / compact_kernel: candidate bitmap -> dense ascending request list. Two launches: candidates per workgroup
// (kCompactWords bitmap words each), then every workgroup sums the counts before it (a few hundred values) and writes its part.
__global__ __launch_bounds__(256) void bitcount_kernel(FilterTable B) {
    __builtin_amdgcn_s_setprio(3);
    __shared__ uint32_t red[256];
    const FilterArgs a = load_descriptor(&B.f[blockIdx.y]);
    const uint32_t words = (a.n + 31) / 32, w0 = blockIdx.x * kCompactWords;
    if (w0 >= words) return;
    uint32_t c = 0;
    for (uint32_t w = w0 + threadIdx.x; w < min(words, w0 + kCompactWords); w += 256) c += (uint32_t)__builtin_popcount(a.bitmap[w]);
    red[threadIdx.x] = c;
    __syncthreads();
    for (uint32_t h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.block_count[blockIdx.x] = red[0];
}

// compact_kernel: a workgroup turns kCompactWords bitmap words into its part of the ascending request list. Each wave owns 512
// consecutive words and takes them 64 at a time — lane = word — so that the lanes of one store instruction write neighbouring list
// entries (the first version gave every thread 8 consecutive words: its stores were 20 entries apart per lane and it took
// 180 us next to the attribute kernel, 8 us alone).
__global__ __launch_bounds__(256) void compact_kernel(FilterTable B) {
    __builtin_amdgcn_s_setprio(3);
    __shared__ uint32_t red[256];
    const FilterArgs a = load_descriptor(&B.f[blockIdx.y]);
    const uint32_t words = (a.n + 31) / 32, w0 = blockIdx.x * kCompactWords, tid = threadIdx.x, wave = wave_index(), lane = tid & 63;
    if (w0 >= words) return;
    const uint32_t n_blocks = (words + kCompactWords - 1) / kCompactWords;
    uint32_t acc = 0;
    for (uint32_t bq = tid; bq < blockIdx.x; bq += 256) acc += a.block_count[bq];
    red[tid] = acc;
    __syncthreads();
    for (uint32_t h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    const uint32_t base = red[0];
    __syncthreads();
    constexpr uint32_t kSteps = kCompactWords / 256;  // 64-word steps per wave
    const uint32_t wave_w0 = w0 + wave * (kSteps * 64);
    uint32_t wv[kSteps], mine = 0;
#pragma unroll
    for (uint32_t q = 0; q < kSteps; q++) {
        const uint32_t w = wave_w0 + q * 64 + lane;
        wv[q] = w < words ? a.bitmap[w] : 0u;
        mine += (uint32_t)__builtin_popcount(wv[q]);
    }
    const uint32_t wave_total = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_add(mine), 63);
    if (lane == 0) red[wave] = wave_total;
    __syncthreads();
    uint32_t pos0 = base;
    for (uint32_t k = 0; k < wave; k++) pos0 += red[k];
#pragma unroll
    for (uint32_t q = 0; q < kSteps; q++) {
        uint32_t w = wv[q];
        const uint32_t pc = (uint32_t)__builtin_popcount(w), incl = wave_scan_add(pc);
        uint32_t pos = pos0 + incl - pc;
        const uint32_t r0 = (wave_w0 + q * 64 + lane) * 32;
        while (w) {
            a.list[pos++] = r0 + (uint32_t)__builtin_ctz(w);
            w &= w - 1;
        }
        pos0 += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (blockIdx.x == n_blocks - 1 && tid == 255) *a.list_count = pos0;
}

// Every instantiation that takes dynamic LDS, named once: launch_filter picks from this table, configure_filter_kernels walks it. [HEADS]
static const void *const kFilterFns[2] = {reinterpret_cast<const void *>(filter_kernel<false>), reinterpret_cast<const void *>(filter_kernel<true>)};

static uint32_t filter_blocks(const FilterArgs *host, uint32_t count, bool *heads) {
    uint32_t blocks = 0;
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t slabs = (uint32_t)(((uint64_t)host[k].total + kStreamSlab - 1) / kStreamSlab) - host[k].slab0;
        blocks += (slabs + kFilterWaves - 1) / kFilterWaves;
        *heads = *heads || host[k].n_heads != 0;
    }
    return blocks;
}

int launch_filter(const FilterArgs *host1, uint32_t count1, const FilterArgs *dev1, const FilterArgs *host2, uint32_t count2, const FilterArgs *dev2, void *stream) {
    // the passes of each stride, first_block numbered within their class by the caller
    bool heads = false;
    FilterMix m{dev1, dev2, count1, count2, filter_blocks(host1, count1, &heads), filter_blocks(host2, count2, &heads)};
    if (m.blocks1 + m.blocks2 == 0) return 0;
    void *args[] = {&m};
    const void *fn = kFilterFns[heads ? 1 : 0];
    hipError_t e = hipLaunchKernel(fn, dim3(m.blocks1 + m.blocks2), dim3(kFilterWaves * 64), args, kFilterEntries * 4, (hipStream_t)stream);
    return (int)(e != hipSuccess ? e : hipGetLastError());
}

int launch_resolve(const FilterArgs *host, uint32_t count, const FilterArgs *dev, void *stream) {
    uint32_t max_slabs = 0;
    uint64_t all_slabs = 0;
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t slabs = (uint32_t)(((uint64_t)host[k].total + kStreamSlab - 1) / kStreamSlab) - host[k].slab0;
        max_slabs = max(max_slabs, slabs);
        all_slabs += slabs;
    }
    if (count == 0 || max_slabs == 0) return 0;
    FilterTable t{dev, count};
    void *args[] = {&t};
    // four waves per slab when one per slab would leave the chip's wave slots empty (resolve_kernel: PARTS)
    const char *forced = getenv("PWAF_RESOLVE_PARTS");  // (measurement / test switch, read per launch: 1 or 4)
    const bool split = forced ? atoi(forced) == 4 : all_slabs < 4096u;  // (measured: 1.25M requests = 2 700 slabs 55 -> 40 us; 2.5M = 5 400 slabs no gain; 10M = 21 600 slabs 123 -> 190 us)
    hipError_t e = split ? hipLaunchKernel(kResolveFns[1], dim3(max_slabs, count), dim3(256), args, 0, (hipStream_t)stream)
                         : hipLaunchKernel(kResolveFns[0], dim3((max_slabs + 3) / 4, count), dim3(256), args, 0, (hipStream_t)stream);
    return (int)(e != hipSuccess ? e : hipGetLastError());
}

int launch_compact(const FilterArgs *host, uint32_t count, const FilterArgs *dev, void *stream) {
    if (count == 0 || host[0].n == 0) return 0;
    const uint32_t words = (host[0].n + 31) / 32, n_blocks = (words + kCompactWords - 1) / kCompactWords;
    FilterTable t{dev, count};
    void *args[] = {&t};
    hipError_t e = hipLaunchKernel(reinterpret_cast<const void *>(bitcount_kernel), dim3(n_blocks, count), dim3(256), args, 0, (hipStream_t)stream);
    if (e == hipSuccess) e = hipLaunchKernel(reinterpret_cast<const void *>(compact_kernel), dim3(n_blocks, count), dim3(256), args, 0, (hipStream_t)stream);
    return (int)(e != hipSuccess ? e : hipGetLastError());
}

// Raises the dynamic-LDS limit of filter_kernel on the current device (configure_kernels, kernels.hip); the other kernels of this unit
// take static LDS only.
int configure_filter_kernels() {
    for (const void *fn : kFilterFns)
        if (int e = (int)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerGroup)) return e;
    return 0;
}

}  // namespace pwaf
