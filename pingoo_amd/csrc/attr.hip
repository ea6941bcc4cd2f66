// attr.hip — everything about a request that is not a string scan: ipres_kernel (address lookups), georec_kernel (GeoIP records),
// attr_kernel ((column, 64-request mask) pairs per group) and dir24_kernel (builds the DIR-24-8 table at engine creation).
// Pipeline overview: kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "kernels.h"
#include "wave.h"

namespace pwaf {

// -------------------------------------------------------------------------------------------------
// attributes: everything about a request that is NOT a string scan — GeoIP record, ip-list membership, country / integer-set
// membership, length / port / asn comparisons — reduced per 64-request group to a list of (column, 64-request mask) pairs
// -------------------------------------------------------------------------------------------------
// The lookups are chains of dependent gathers (DIR-24 / trie levels, membership rows); the kernel keeps only its small constant tables
// in LDS (see the last point below) and does not depend on the scans, so it runs BESIDE them on the engine's side stream at the lowest
// wave priority. One wave = one 64-request group; the verdict kernel only copies the group's pairs into its column file.
//
// What keeps it short (round 2: it had become the longest kernel, 2.8 GB fetched for 0.38 GB of input):
//   * everything that is a function of the GeoIP record — country-table bits, asn-set bits and the asn comparisons — is folded at
//     engine creation into a CLASS row, and records with equal rows share a class (a few hundred classes for 600k records: the
//     table is cache-resident, class 0 = "no predicate holds" needs no row at all);
//   * IPv4: ONE gather into a 2^24 x 4-byte table (DIR-24-8, 64 MiB) yields class | membership-set id << 16; prefixes longer than
//     /24 and oversized ids escape to an 8-byte side table and continue in the 8-bit trie nodes;
//   * a group's inputs are requested TWO groups ahead and its DIR-24 / root entries ONE group ahead, so the long-latency loads of the
//     next groups are in flight while the current group's rows are transposed (few waves per CU: nothing else hides them);
//   * the constant tables the group loop reads AFTER it has issued that prefetch — the (source word, bit) -> column table, the
//     comparison atoms and short literals beyond the 64 held in registers — are staged once per workgroup in LDS. Read from global
//     memory (the stores to the pair list may alias them, so the compiler cannot hoist the loads) each read was followed by a wait for
//     ALL outstanding loads — they return in order — which drained the prefetch once per group: one exposed L2 round trip per present
//     source word on top of it. LDS reads are counted apart from the vector-memory loads, so the prefetch stays in flight.
static constexpr uint32_t DIR_ESCAPE = 0x80000000u;

__device__ __forceinline__ uint32_t ip_byte(const uint32_t w[4], uint32_t k) {
    uint32_t word = k < 4 ? w[0] : k < 8 ? w[1] : k < 12 ? w[2] : w[3];
    return (word >> ((k & 3) * 8)) & 0xFFu;
}

// ipres_kernel (round 3): the address lookups of the attribute path as a kernel of their own — one lane per request, ~20 registers,
// full occupancy. Round 2 did them inside attr_kernel, whose transposes need ~128 registers (4 waves per SIMD) and whose waves each
// walked one 64-request group at a time: every group waited for its own DIR-24 line (a miss to the Infinity Cache / HBM) and then
// for the trie levels of its few IPv6 lanes, with 16 waves per CU to hide it all — 0.44 ms alone for 10M requests, the longest
// kernel of the step. Here 32 waves per CU overlap those waits, and an IPv4 address behind the DIR-24 table costs ONE gather (round 2
// also fetched both 16-bit root entries for every lane and threw them away). Output: the GeoIP CLASS and the ip-list membership SET
// of every request, packed into one word (class | set << 16) when both fit 16 bits (else two words).
//
// COARSE (csrc/dirtable.h; launch shape: ipres_shape()): the workgroup stages the coarse bitmap — one bit per block of
// 2^dir_coarse_shift /24s, at most 64 KiB — in LDS, and an IPv4 lane reads its block's bit there before anything else. Clear = the
// answer is dir_common and the lane issues no global load at all: an LDS gather takes neither a texture-addresser slot nor an
// L1 -> L2 request, which are what bound this kernel. Set = the lookup goes on as without the level. 8 waves per SIMD as before.
template <bool PACKED, bool COARSE>
__global__ __launch_bounds__(COARSE ? 1024 : 256, COARSE ? 8 : 1) void ipres_kernel(VerdictArgs a) {
    // A lookup is a chain of dependent accesses (address bytes -> first level -> run bitmap -> value; IPv6: root -> trie nodes), each an
    // L2 / Infinity-Cache round trip: with one request per lane at a time the kernel was latency-bound even at 32 waves per CU (0.24 ms
    // for 10M requests, 19 chains per lane one after the other). Every lane now walks U = 4 requests in lockstep: each phase issues
    // the loads of all four before any is used.
    constexpr uint32_t U = 4;
    extern __shared__ uint4 ipres_lds[];  // COARSE: the coarse bitmap (dir_coarse_bytes)
    const bool from_row = a.asn == nullptr;
#ifdef PWAF_PROFILING
    // timing experiments (wrong results): bit 16 = no table lookups for IPv4, bit 17 = no trie walks for IPv6
    const bool dir = a.dir_chunks != nullptr && !((a.debug_skip >> 16) & 1u);
    const bool skip_v6 = (a.debug_skip >> 17) & 1u, skip_v4 = (a.debug_skip >> 16) & 1u;
#else
    const bool dir = a.dir_chunks != nullptr;
    constexpr bool skip_v6 = false, skip_v4 = false;
#endif
    const uint32_t T = gridDim.x * blockDim.x;
    uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x;
    uint4 raw[U];
    uint32_t v6b[U];
    // the addresses and families of the lane's four requests (a dead slot re-reads the lane's first request)
    auto load_inputs = [&](uint32_t base) {
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint32_t j = base + u * T < a.n ? base + u * T : base;
            raw[u] = *reinterpret_cast<const uint4 *>(a.ip + (size_t)j * 16);
            v6b[u] = a.ip_is_v6[j];
        }
    };
    bool loaded = false;
    if (COARSE) {
        // Staged BEHIND the first sweep's address loads, so that both share one round trip (loads return in order: the wait for the
        // bitmap's words covers the addresses): 16-byte loads, four in flight per lane — the whole bitmap in one trip at 64 KiB / 1024
        // or 32 KiB / 512 threads. A lane without a request (the last workgroup) stages with the others and loads request 0.
        load_inputs(i0 < a.n ? i0 : 0u);
        loaded = true;
        const uint4 *src = reinterpret_cast<const uint4 *>(a.dir_coarse);
        const uint32_t n16 = a.dir_coarse_bytes >> 4;
        for (uint32_t j = threadIdx.x; j < n16; j += 4u * blockDim.x) {
            uint4 w[4];
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) w[q] = src[min(j + q * blockDim.x, n16 - 1u)];
#pragma unroll
            for (uint32_t q = 0; q < 4; q++)
                if (j + q * blockDim.x < n16) ipres_lds[j + q * blockDim.x] = w[q];
        }
        __syncthreads();
    }
    for (; i0 < a.n; i0 += T * U) {
        uint32_t idx[U], ipw[U][4], eg[U], ei[U], k[U];
        bool live[U], v6[U], geo_walk[U], chunked[U];
        if (!loaded) load_inputs(i0);
        loaded = false;
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            idx[u] = i0 + u * T;
            live[u] = idx[u] < a.n;
        }
        uint32_t first[U], top16[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            ipw[u][0] = raw[u].x; ipw[u][1] = raw[u].y; ipw[u][2] = raw[u].z; ipw[u][3] = raw[u].w;
            v6[u] = v6b[u] != 0;
            // GeoipDB::lookup, pingoo/geoip.rs:73-91: loopback / multicast are "not found"
            geo_walk[u] = false;
            if (from_row && a.has_geo) {
                if (!v6[u]) {
                    const uint32_t b0 = ipw[u][0] & 0xFFu;
                    geo_walk[u] = !(b0 == 127u || (b0 & 0xF0u) == 0xE0u);
                } else {
                    const bool loopback = ipw[u][0] == 0 && ipw[u][1] == 0 && ipw[u][2] == 0 && ipw[u][3] == 0x01000000u;
                    geo_walk[u] = !(loopback || (ipw[u][0] & 0xFFu) == 0xFFu);
                }
            }
            top16[u] = (ip_byte(ipw[u], 0) << 8) | ip_byte(ipw[u], 1);
            // phase 1: the /16's line of the compressed DIR table (IPv4) — bitmap word, run counts, where the values live — or the two
            // 16-bit roots
            eg[u] = ei[u] = TRIE_LEAF;
            chunked[u] = !v6[u] && dir;
            first[u] = 0;
            if (!chunked[u] && !(v6[u] ? skip_v6 : skip_v4)) {
                if (geo_walk[u]) eg[u] = (v6[u] ? a.geo_root6 : a.geo_root4)[top16[u]];  // (the engine substitutes an all-leaf root for a family without prefixes)
                if (a.n_ip_lists) ei[u] = (v6[u] ? a.ip_root6 : a.ip_root4)[top16[u]];
            }
        }
        // phase 1b: the coarse bit of the address's block of /24s (LDS), then for the lanes it leaves the summary bit (L2-resident
        // bitmap): 0 = the table's most common entry, no gather
        uint32_t look[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            look[u] = chunked[u] ? 1u : 0u;
            if (COARSE && chunked[u]) {
                const uint32_t blk = ((top16[u] << 8) | ip_byte(ipw[u], 2)) >> a.dir_coarse_shift;
                look[u] = (reinterpret_cast<const uint32_t *>(ipres_lds)[blk >> 5] >> (blk & 31u)) & 1u;
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            if (look[u] && a.dir_summary != nullptr) {
                const uint32_t blk = ((top16[u] << 8) | ip_byte(ipw[u], 2)) >> a.dir_sum_shift;
                look[u] = (a.dir_summary[blk >> 5] >> (blk & 31u)) & 1u;
            }
        }
        uint4 rec4[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            rec4[u] = make_uint4(0u, 0u, 0u, 0u);
            // ONE 16-byte gather: the record of the address's group of 32 /24s
            if (look[u]) rec4[u] = *reinterpret_cast<const uint4 *>(a.dir_chunks + (size_t)top16[u] * kDirChunkWords + 4u * (ip_byte(ipw[u], 2) >> 5));
        }
        // phase 2: the run's entry — carried into the group, the first run inside it, or (rarely) a further run from dir_vals
        uint32_t e24[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            e24[u] = a.dir_common;
            if (look[u]) {
                const uint32_t rank = (uint32_t)__builtin_popcount(rec4[u].x & (0xFFFFFFFFu >> (31u - (ip_byte(ipw[u], 2) & 31u))));  // run starts at or before the /24, inside its group
                e24[u] = rank == 0 ? rec4[u].y : rank == 1 ? rec4[u].z : a.dir_vals[rec4[u].w + rank - 2u];
            }
        }
        // phase 4: escapes (a prefix longer than /24, or an id too large for the packed entry: rare)
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            k[u] = 2;
            if (!v6[u] && dir) {
                k[u] = 3;
                if (e24[u] & DIR_ESCAPE) {
                    const uint2 esc = a.dir_esc[e24[u] & ~DIR_ESCAPE];
                    eg[u] = esc.x;
                    ei[u] = esc.y;
                } else {
                    eg[u] = TRIE_LEAF | (e24[u] & 0xFFFFu);
                    ei[u] = TRIE_LEAF | (e24[u] >> 16);
                }
            }
            if (!geo_walk[u]) eg[u] = TRIE_LEAF | a.geo_default;  // no lookup: the default record's class
            if (a.n_ip_lists == 0) ei[u] = TRIE_LEAF;
        }
        // phase 5: the remaining trie levels (IPv6, escapes), all four walks advancing together
        for (;;) {
            bool more = false;
#pragma unroll
            for (uint32_t u = 0; u < U; u++) more = more || !((eg[u] & ei[u]) & TRIE_LEAF);
            if (!more) break;
            uint32_t ng[U], ni[U];
#pragma unroll
            for (uint32_t u = 0; u < U; u++) {
                const uint32_t byte = ip_byte(ipw[u], k[u] < 16 ? k[u] : 15u);
                ng[u] = (eg[u] & TRIE_LEAF) ? eg[u] : a.geo_nodes[(size_t)eg[u] * 256 + byte];
                ni[u] = (ei[u] & TRIE_LEAF) ? ei[u] : a.ip_nodes[(size_t)ei[u] * 256 + byte];
            }
#pragma unroll
            for (uint32_t u = 0; u < U; u++) {
                if (!((eg[u] & ei[u]) & TRIE_LEAF)) k[u]++;
                eg[u] = ng[u];
                ei[u] = ni[u];
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            if (!live[u]) continue;
            const uint32_t cls = eg[u] & ~TRIE_LEAF, set_id = ei[u] & ~TRIE_LEAF;
            if (PACKED) a.ipres[idx[u]] = cls | (set_id << 16);
            else reinterpret_cast<uint2 *>(a.ipres)[idx[u]] = make_uint2(cls, set_id);
        }
    }
}

// georec_kernel (PWAF_OPT_GEO_ANSWERS): the GeoIP RECORD of every request — what the reference keeps in its RequestContext and sends
// upstream (http_listener.rs:143-157,183-191; http_proxy_service.rs:174-189). ipres_kernel's shape (one lane per request, no LDS, U = 4
// requests per lane in lockstep, every phase's loads issued before any is used) over ONE table: the record-leaf trie and its own
// compressed IPv4 table (csrc/georec.h: an entry is the record id, or DIR_ESCAPE | the trie node to continue from). One dependent
// 8-byte gather of the record and one 8-byte store end it. A batch that carries asn / country columns gets them echoed.
__global__ __launch_bounds__(256) void georec_kernel(GeoRecArgs a) {
    constexpr uint32_t U = 4;
    const uint32_t T = gridDim.x * 256u;
    if (a.asn != nullptr) {
        for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < a.n; i += T) a.out[i] = make_uint2(a.asn[i], (uint32_t)a.country[i]);
        return;
    }
    const bool dir = a.chunks != nullptr;
    for (uint32_t i0 = blockIdx.x * 256u + threadIdx.x; i0 < a.n; i0 += T * U) {
        uint32_t idx[U], ipw[U][4], e[U], k[U], top16[U], v6b[U];
        bool live[U], chunked[U];
        uint4 raw[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            idx[u] = i0 + u * T;
            live[u] = idx[u] < a.n;
            const uint32_t j = live[u] ? idx[u] : i0;
            raw[u] = *reinterpret_cast<const uint4 *>(a.ip + (size_t)j * 16);
            v6b[u] = a.ip_is_v6[j];
        }
        // family and exclusion (GeoipDB::lookup, pingoo/geoip.rs:73-91: loopback / multicast are "not found"), then phase 1: the 16-bit
        // root (IPv6, or IPv4 without a table)
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            ipw[u][0] = raw[u].x; ipw[u][1] = raw[u].y; ipw[u][2] = raw[u].z; ipw[u][3] = raw[u].w;
            const bool v6 = v6b[u] != 0;
            bool walk = a.has_geo != 0;
            if (!v6) {
                const uint32_t b0 = ipw[u][0] & 0xFFu;
                walk = walk && !(b0 == 127u || (b0 & 0xF0u) == 0xE0u);
            } else {
                const bool loopback = ipw[u][0] == 0 && ipw[u][1] == 0 && ipw[u][2] == 0 && ipw[u][3] == 0x01000000u;
                walk = walk && !(loopback || (ipw[u][0] & 0xFFu) == 0xFFu);
            }
            top16[u] = (ip_byte(ipw[u], 0) << 8) | ip_byte(ipw[u], 1);
            e[u] = TRIE_LEAF;  // record 0: the default
            k[u] = 2;
            chunked[u] = walk && !v6 && dir;
            if (walk && !chunked[u]) e[u] = (v6 ? a.root6 : a.root4)[top16[u]];
        }
        // phase 1b: the summary bit of the address's block of /24s: 0 = the table's most common entry, no gather
        uint32_t look[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            look[u] = chunked[u] ? 1u : 0u;
            if (chunked[u] && a.summary != nullptr) {
                const uint32_t blk = ((top16[u] << 8) | ip_byte(ipw[u], 2)) >> a.sum_shift;
                look[u] = (a.summary[blk >> 5] >> (blk & 31u)) & 1u;
            }
        }
        // ONE 16-byte gather: the record of the address's group of 32 /24s
        uint4 rec4[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            rec4[u] = make_uint4(0u, 0u, 0u, 0u);
            if (look[u]) rec4[u] = *reinterpret_cast<const uint4 *>(a.chunks + (size_t)top16[u] * kDirChunkWords + 4u * (ip_byte(ipw[u], 2) >> 5));
        }
        // phase 2: the run's entry — carried into the group, the first run inside it, or a further run from vals
        uint32_t e24[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            e24[u] = a.common;
            if (look[u]) {
                const uint32_t rank = (uint32_t)__builtin_popcount(rec4[u].x & (0xFFFFFFFFu >> (31u - (ip_byte(ipw[u], 2) & 31u))));
                e24[u] = rank == 0 ? rec4[u].y : rank == 1 ? rec4[u].z : a.vals[rec4[u].w + rank - 2u];
            }
        }
        // phase 4: an escape continues in the trie node the entry names, with the address's last byte
#pragma unroll
        for (uint32_t u = 0; u < U; u++)
            if (chunked[u]) {
                k[u] = 3;
                e[u] = (e24[u] & DIR_ESCAPE) ? (e24[u] & ~DIR_ESCAPE) : (TRIE_LEAF | e24[u]);
            }
        // phase 5: the remaining trie levels (IPv6, escapes), all walks advancing together
        for (;;) {
            bool more = false;
#pragma unroll
            for (uint32_t u = 0; u < U; u++) more = more || !(e[u] & TRIE_LEAF);
            if (!more) break;
            uint32_t ne[U];
#pragma unroll
            for (uint32_t u = 0; u < U; u++) ne[u] = (e[u] & TRIE_LEAF) ? e[u] : a.nodes[(size_t)e[u] * 256 + ip_byte(ipw[u], k[u] < 16 ? k[u] : 15u)];
#pragma unroll
            for (uint32_t u = 0; u < U; u++) {
                k[u]++;
                e[u] = ne[u];
            }
        }
        // the record itself: one 8-byte gather, one 8-byte store
        uint2 r[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) r[u] = reinterpret_cast<const uint2 *>(a.recs)[e[u] & ~TRIE_LEAF];
#pragma unroll
        for (uint32_t u = 0; u < U; u++)
            if (live[u]) a.out[idx[u]] = make_uint2(r[u].x, r[u].y & 0xFFFFu);
    }
}

struct AttrIn {
    uint32_t cls, set_id;
    uint32_t port, len[5], asn, country;
    uint32_t sstart, slen;  // the short-literal field's value: offset and length
};

// (__launch_bounds__(256, 7) — 72 registers, 7 waves per SIMD at the price of 3-5 spilled dwords — was measured: 0.229 ms alone against
// 0.227, nothing.)
// SMALL: the rule set's membership rows fit 4 ip-set words, 2 country words and one word each of port sets, asn sets and asn
// comparisons (a 1k-rule set with 124 CIDR lists does): 9 row registers instead of 36.
// Atoms beyond the 64 that live in registers, staged in LDS for the group loop (the chunks beyond these are re-read from global memory
// per group: a rule set with more than 256 eager comparison atoms or 128 short literals).
static constexpr uint32_t kAttrCmpStaged = 192, kAttrShortStaged = 64;
template <bool PACKED, bool SMALL>
__global__ __launch_bounds__(256) void attr_kernel(VerdictArgs a) {
    constexpr uint32_t SW = SMALL ? 4 : kSetWordsMax, CW = SMALL ? 2 : kCcWordsMax, IW = SMALL ? 1 : kIntWordsMax, QW = SMALL ? 1 : kAcmpWordsMax;
    // LDS (one array): the rows of bit_col this instantiation can meet, in the order of the transposes below (slot -> source word:
    // SW ip-set words, CW country words, IW port-set words, IW asn-set words, QW asn-comparison words), then the staged comparison
    // atoms {col, c} and the staged short literals {col, len_exact, lit_lo, lit_hi}. 1.1 KiB + 2.5 KiB (SMALL), 4.5 KiB + 2.5 KiB.
    constexpr uint32_t kSlotCc = SW, kSlotPort = SW + CW, kSlotAsn = SW + CW + IW, kSlotAcmp = SW + CW + 2 * IW, kSlots = SW + CW + 2 * IW + QW;
    constexpr uint32_t kLdsCmp = kSlots * 32, kLdsShort = kLdsCmp + 2 * kAttrCmpStaged, kLdsWords = kLdsShort + 4 * kAttrShortStaged;
    __shared__ uint32_t tab[kLdsWords];
#ifdef PWAF_PROFILING
    if (a.debug_skip & 0x80000000u) __builtin_amdgcn_s_setprio(3);  // timing experiment
#endif
    const uint32_t lane = threadIdx.x & 63, wave = wave_index();
    const bool from_row = a.asn == nullptr;  // asn / country come from the engine's own GeoIP record (or its default)
#ifdef PWAF_PROFILING
    // timing experiments (wrong results): which part of the kernel costs what
    const bool skip_rows = (a.debug_skip >> 18) & 1u, skip_transpose = (a.debug_skip >> 19) & 1u, skip_cmp = (a.debug_skip >> 20) & 1u;
#else
    constexpr bool skip_rows = false, skip_transpose = false, skip_cmp = false;
#endif
    // group-invariant: the first 64 comparison atoms, one per lane (col | code << 24, constant)
    uint32_t h_col = 0, h_c = 0;
    if (lane < a.n_cmp) {
        h_col = a.cmp[lane].col;
        h_c = a.cmp[lane].c;
    }
    const uint32_t g_stride = gridDim.x * 4;
    // stage A: the fixed-width inputs of a group. Every load is UNCONDITIONAL: a column the rule set does not read (or the batch does not
    // carry) is replaced by element 0 of a column that always exists — one cached line for the whole wave, its value discarded. A load
    // under a wave-uniform condition becomes a branch around it, and the compiler waits for ALL outstanding loads where the branches
    // join: one exposed round trip per length column, in the middle of the prefetch.
    const uint32_t *const asn_col = from_row ? a.off[0] : a.asn;
    const uint16_t *const country_col = from_row ? a.port : a.country;
    const uint32_t *const short_col = a.n_short ? a.short_off : a.off[0];
    const uint8_t *const short_bytes = a.n_short ? a.short_data : reinterpret_cast<const uint8_t *>(a.off[0]);
    auto load_in = [&](const uint32_t g, AttrIn &in) {
        const uint32_t i0 = g * 64 + lane;
        const uint32_t i = (g < a.n_groups && i0 < a.n) ? i0 : 0u;
        if (PACKED) {
            const uint32_t w = a.ipres[i];
            in.cls = w & 0xFFFFu;
            in.set_id = w >> 16;
        } else {
            const uint2 w = reinterpret_cast<const uint2 *>(a.ipres)[i];
            in.cls = w.x;
            in.set_id = w.y;
        }
        in.port = a.port[i];
#pragma unroll
        for (int f = 0; f < 5; f++) {  // (wave-uniform: only the lengths some comparison atom reads)
            const bool used = (a.cmp_vars >> f) & 1u;
            const uint32_t j = used ? i : 0u;
            const uint32_t d = a.off[f][j + 1] - a.off[f][j];
            in.len[f] = used ? d : 0u;
        }
        const uint32_t ja = from_row ? 0u : i, js = a.n_short ? i : 0u;
        const uint32_t v_asn = asn_col[ja], v_country = country_col[ja], s0 = short_col[js], s1 = short_col[js + 1];
        in.asn = from_row ? 0u : v_asn;
        in.country = from_row ? 0u : v_country;
        in.sstart = a.n_short ? s0 : 0u;
        in.slen = a.n_short ? s1 - s0 : 0u;
    };
    // stage B: the short-literal field's first 8 bytes (arenas carry 16 readable slack bytes)
    auto load_short = [&](const AttrIn &in, uint32_t &s_lo, uint32_t &s_hi) {
        typedef uint2 __attribute__((aligned(1))) uint2_u;
        const uint2 sv = *reinterpret_cast<const uint2_u *>(short_bytes + in.sstart);  // (no short literals: the first 8 bytes of a column that exists, unused)
        s_lo = sv.x;
        s_hi = sv.y;
    };
    AttrIn cur, nxt;
    uint32_t c_slo, c_shi;
    const uint32_t g0 = blockIdx.x * 4 + wave;
    load_in(g0, cur);
    load_in(g0 + g_stride, nxt);
    load_short(cur, c_slo, c_shi);
    // group-invariant: the first 64 short-literal atoms, one per lane
    ShortAtom h_short{0, 0, 0, 0};
    if (lane < a.n_short) h_short = a.short_atoms[lane];
    // the LDS tables, once per workgroup (behind the first groups' input loads, so that all of them share one round trip)
    for (uint32_t t = threadIdx.x; t < kSlots * 32; t += 256) {
        const uint32_t s = t >> 5;
        const uint32_t src = s < kSlotCc ? kSrcSet + s : s < kSlotPort ? kSrcCc + (s - kSlotCc) : s < kSlotAsn ? kSrcPort + (s - kSlotPort) : s < kSlotAcmp ? kSrcAsn + (s - kSlotAsn) : kSrcAcmp + (s - kSlotAcmp);
        tab[t] = a.bit_col[src * 32 + (t & 31u)];
    }
    for (uint32_t t = threadIdx.x; t < kAttrCmpStaged && 64 + t < a.n_cmp; t += 256) {
        tab[kLdsCmp + 2 * t] = a.cmp[64 + t].col;
        tab[kLdsCmp + 2 * t + 1] = a.cmp[64 + t].c;
    }
    for (uint32_t t = threadIdx.x; t < kAttrShortStaged && 64 + t < a.n_short; t += 256) {
        const ShortAtom s = a.short_atoms[64 + t];
        tab[kLdsShort + 4 * t] = s.col;
        tab[kLdsShort + 4 * t + 1] = s.len_exact;
        tab[kLdsShort + 4 * t + 2] = s.lit_lo;
        tab[kLdsShort + 4 * t + 3] = s.lit_hi;
    }
    __syncthreads();

    for (uint32_t g = g0; g < a.n_groups; g += g_stride) {
        const uint32_t i = g * 64 + lane;
        const bool valid = i < a.n;
        const unsigned long long valid_mask = __ballot(valid);
        uint4 *pairs = a.gpairs + (size_t)g * a.pair_stride;
        uint32_t n_pairs = 0;  // wave-uniform
        // lane-private (column, mask) -> the group's pair list, in lane order
        auto emit_pairs = [&](const bool has, const uint32_t c, const uint32_t lo, const uint32_t hi) {
            const unsigned long long em = __ballot(has);
            if (has) pairs[n_pairs + __builtin_amdgcn_mbcnt_hi((uint32_t)(em >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)em, 0u))] = make_uint4(c, 0u, lo, hi);  // (emitting lanes below this one)
            n_pairs += (uint32_t)__builtin_popcountll(em);
        };
        const uint32_t port = cur.port;
        const uint32_t cls = cur.cls, set_id = cur.set_id;

        // ---- 1. membership rows: every row word of the request requested together, then ONE wait ----
        uint32_t asn = cur.asn, r_geo = 0;
        if (!from_row) {
            const uint32_t c0 = (cur.country & 0xFFu) - 'A', c1 = (cur.country >> 8) - 'A';
            r_geo = (c0 < 26u && c1 < 26u) ? c0 * 26u + c1 : 23u * 26u + 23u;  // invalid input is treated as "XX"
        }
        uint32_t r_int[2] = {0, 0};
#pragma unroll
        for (int var = 0; var < 2; var++) {
            // integer sets: ONE binary search per request over the union of every set tested against the variable
            if (!valid || a.iu_n[var] == 0 || (var == 1 && from_row)) continue;
            const long long v = var == VAR_PORT ? (long long)port : (long long)asn;
            uint32_t lo = 0, hi = a.iu_n[var];
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (a.iu_vals[var][mid] < v) lo = mid + 1;
                else hi = mid;
            }
            if (lo < a.iu_n[var] && a.iu_vals[var][lo] == v) r_int[var] = lo + 1;
        }
        // sources (kernels.h kSrc*): ip-set row, country words, port-set row, asn-set words, asn comparisons
        const uint32_t *srow = a.set_masks + (size_t)set_id * a.set_words;
        const uint32_t *crow = from_row ? a.class_rows + (size_t)cls * a.class_words : a.country_masks + (size_t)r_geo * a.cc_words;
        const uint32_t *prow = a.iu_masks[0] + (size_t)r_int[0] * a.iu_words[0];
        const uint32_t *arow = from_row ? crow + a.cc_words : a.iu_masks[1] + (size_t)r_int[1] * a.iu_words[1];
        const uint32_t *qrow = crow + a.cc_words + a.iu_words[1];
        const bool rows_on = valid && !skip_rows;
        const bool have_s = rows_on && a.n_ip_lists && set_id, have_c = rows_on && (from_row ? cls != 0 : true), have_p = rows_on && r_int[0],
                   have_a = rows_on && (from_row ? cls != 0 : r_int[1] != 0), have_q = rows_on && from_row && cls != 0;
        uint32_t rs[SW], rc[CW], rp[IW], ra[IW], rq[QW];
#pragma unroll
        for (uint32_t q = 0; q < SW; q++) rs[q] = (q < a.set_words && have_s) ? srow[q] : 0u;
#pragma unroll
        for (uint32_t q = 0; q < CW; q++) rc[q] = (q < a.cc_words && have_c) ? crow[q] : 0u;
#pragma unroll
        for (uint32_t q = 0; q < IW; q++) rp[q] = (q < a.iu_words[0] && have_p) ? prow[q] : 0u;
#pragma unroll
        for (uint32_t q = 0; q < IW; q++) ra[q] = (q < a.iu_words[1] && have_a) ? arow[q] : 0u;
#pragma unroll
        for (uint32_t q = 0; q < QW; q++) rq[q] = (q < a.acmp_words && have_q) ? qrow[q] : 0u;

        // ---- 2. prefetch: inputs of the group after next, the next group's short-literal bytes ----
        AttrIn nn;
        load_in(g + 2 * g_stride, nn);
        uint32_t n_slo, n_shi;
        load_short(nxt, n_slo, n_shi);
        // The rows are waited for HERE, once, with the prefetch behind them still in flight. Left to the first use inside each transpose,
        // the wait is placed where paths with and without a pair store join, and is counted for the path without: behind every
        // store it then also waits for one more load of the prefetch.
#pragma unroll
        for (uint32_t q = 0; q < SW; q++) asm volatile("" : "+v"(rs[q]));
#pragma unroll
        for (uint32_t q = 0; q < CW; q++) asm volatile("" : "+v"(rc[q]));
#pragma unroll
        for (uint32_t q = 0; q < IW; q++) asm volatile("" : "+v"(rp[q]), "+v"(ra[q]));
#pragma unroll
        for (uint32_t q = 0; q < QW; q++) asm volatile("" : "+v"(rq[q]));

        // ---- 3. transposes: one ballot per bit that ANY of the 64 requests has set (wave-wide OR first, so absent bits cost
        //         nothing); lane b keeps bit b's request mask and owns that atom's pair ----
        auto transpose = [&](const uint32_t w, const uint32_t slot) {
            const uint32_t orw0 = wave_or(w);
            if (orw0 == 0) return;
            // (the mask is PARKED in lane b with v_writelane: two vector instructions per bit — a compare of the lane id and two
            // selects, with the mask moved into vector registers first, were seven; the kernel is bound by vector-ALU issue)
            uint32_t mine_lo = 0, mine_hi = 0;
            for (uint32_t orw = orw0; orw; orw &= orw - 1) {
                const uint32_t b = (uint32_t)__builtin_ctz(orw);
                const unsigned long long m = __ballot((w & (1u << b)) != 0u);
                park64(mine_lo, mine_hi, m, b);
            }
            const bool owner = lane < 32 && ((orw0 >> lane) & 1u);
            const uint32_t c = owner ? tab[slot * 32 + (lane & 31u)] : 0u;  // (source word, bit) -> column, 0 = no such atom (LDS: no wait on the prefetch)
            emit_pairs(c != 0, c, mine_lo, mine_hi);
        };
        if (!skip_transpose) {
#pragma unroll
            for (uint32_t q = 0; q < SW; q++) if (q < a.set_words) transpose(rs[q], q);  // (uniform conditions)
#pragma unroll
            for (uint32_t q = 0; q < CW; q++) if (q < a.cc_words) transpose(rc[q], kSlotCc + q);
#pragma unroll
            for (uint32_t q = 0; q < IW; q++) if (q < a.iu_words[0]) transpose(rp[q], kSlotPort + q);
#pragma unroll
            for (uint32_t q = 0; q < IW; q++) if (q < a.iu_words[1]) transpose(ra[q], kSlotAsn + q);
#pragma unroll
            for (uint32_t q = 0; q < QW; q++) if (q < a.acmp_words) transpose(rq[q], kSlotAcmp + q);
        }

        // Comparison atoms (lengths, port, asn against constants): the engine has reduced them to `v == c` / `v <= c` on 32-bit
        // values and tagged each with code = 2 * variable + operator; an atom is a scalar broadcast of its constant, one
        // vector compare and a ballot parked in the atom's lane. (asn comparisons of engine-resolved records are class-row bits.)
        for (uint32_t base = 0; base < a.n_cmp && !skip_cmp; base += 64) {
            uint32_t m_col = h_col, m_c = h_c;
            if (base != 0) {  // more than 64 comparison atoms: the later chunks come from LDS (beyond the staged ones: re-read per group)
                m_col = m_c = 0;
                if (base + lane < a.n_cmp) {
                    if (base < 64 + kAttrCmpStaged) {  // (uniform)
                        m_col = tab[kLdsCmp + 2 * (base - 64 + lane)];
                        m_c = tab[kLdsCmp + 2 * (base - 64 + lane) + 1];
                    } else {
                        m_col = a.cmp[base + lane].col;
                        m_c = a.cmp[base + lane].c;
                        asm volatile("" : "+v"(m_col), "+v"(m_c));  // (the wait for this load belongs HERE, not where the branches join)
                    }
                }
            }
            const uint32_t my_code = base + lane < a.n_cmp ? (m_col >> 24) & 0x7Fu : 0xFFu;
            const unsigned long long flip_atoms = __ballot(base + lane < a.n_cmp && ((m_col >> 31) & 1u) != 0u);  // atoms evaluated complemented (engine.cpp, POLARITY)
            uint32_t acc_lo = 0, acc_hi = 0;
            auto cmp_var = [&](const uint32_t v, const int vi) {
#pragma unroll
                for (int op = 0; op < 2; op++) {
                    unsigned long long todo = __ballot(my_code == (uint32_t)(2 * vi + op));
                    while (todo) {
                        const uint32_t j = (uint32_t)__builtin_ctzll(todo);
                        todo &= todo - 1;
                        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)m_c, (int)j);
                        unsigned long long m = __ballot(op == 0 ? v == c : v <= c);
                        if ((flip_atoms >> j) & 1ull) m = ~m;
                        park64(acc_lo, acc_hi, m & valid_mask, j);
                    }
                }
            };
#pragma unroll
            for (int f = 0; f < 5; f++)
                if ((a.cmp_vars >> f) & 1u) cmp_var(cur.len[f], f);
            if ((a.cmp_vars >> 5) & 1u) cmp_var(port, 5);
            if (!from_row && ((a.cmp_vars >> 6) & 1u)) cmp_var(asn, 6);
            for (uint32_t f = 0; f < a.n_hlen; f++) {  // EXTENSION: lengths of header columns (rare: fetched here, not prefetched)
                const uint32_t ii = valid ? i : 0u;
                cmp_var(a.hoff[f][ii + 1] - a.hoff[f][ii], 7 + (int)f);
            }
            emit_pairs((acc_lo | acc_hi) != 0, m_col & 0xFFFFFFu, acc_lo, acc_hi);
        }
        // Short-literal atoms (kernels.h: ShortAtom): the field's first 8 bytes against each literal under its length mask — a
        // scalar broadcast of the atom, two vector compares and a ballot parked in the atom's lane.
        for (uint32_t base = 0; base < a.n_short; base += 64) {
            ShortAtom m = h_short;
            if (base != 0) {
                m = ShortAtom{0, 0, 0, 0};
                if (base + lane < a.n_short) {
                    const uint32_t *s = tab + kLdsShort + 4 * (base - 64 + lane);
                    if (base < 64 + kAttrShortStaged) {  // (uniform)
                        m = ShortAtom{s[0], s[1], s[2], s[3]};
                    } else {
                        m = a.short_atoms[base + lane];
                        asm volatile("" : "+v"(m.col), "+v"(m.len_exact), "+v"(m.lit_lo), "+v"(m.lit_hi));  // (as above)
                    }
                }
            }
            const uint32_t cnt = min(64u, a.n_short - base);
            uint32_t acc_lo = 0, acc_hi = 0;
            for (uint32_t j = 0; j < cnt; j++) {
                const uint32_t le = (uint32_t)__builtin_amdgcn_readlane((int)m.len_exact, (int)j), len = le & 0xFFu;
                const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)m.lit_lo, (int)j), hi = (uint32_t)__builtin_amdgcn_readlane((int)m.lit_hi, (int)j);
                const uint32_t mlo = len >= 4 ? 0xFFFFFFFFu : (1u << (8 * len)) - 1u, mhi = len >= 8 ? 0xFFFFFFFFu : len > 4 ? (1u << (8 * (len - 4))) - 1u : 0u;
                // (the length test is chosen by a SCALAR branch — `exact` is the atom's, not the request's — and the two masked compares
                // are one: xor, xor-and, and-or, compare)
                const unsigned long long len_ok = (le >> 8) ? __ballot(cur.slen == len) : __ballot(cur.slen >= len);
                const unsigned long long hit = __ballot((((c_slo ^ lo) & mlo) | ((c_shi ^ hi) & mhi)) == 0u) & len_ok & valid_mask;
                park64(acc_lo, acc_hi, hit, j);
            }
            emit_pairs((acc_lo | acc_hi) != 0, m.col, acc_lo, acc_hi);
        }
        if (lane == 0) a.ghdr[g] = n_pairs;
        cur = nxt;
        nxt = nn;
        c_slo = n_slo;
        c_shi = n_shi;
    }
}

// Flattens the first 24 bits of the GeoIP trie (leaves = class ids) and the ip-list trie (leaves = membership-set ids), IPv4 family,
// into one table of 4-byte entries: class | set << 16 when both walks end within 24 bits with ids that fit (class < 65536,
// set < 32768), otherwise DIR_ESCAPE | index of an 8-byte {geo entry, set entry} pair from which the attribute kernel continues.
// Two launches: `esc == nullptr` only counts the escapes.
__global__ __launch_bounds__(256) void dir24_kernel(VerdictArgs a, uint32_t *out, uint2 *esc, uint32_t *esc_count) {
    const uint32_t x = blockIdx.x * 256 + threadIdx.x;  // the top 24 address bits
    if (x >= (1u << 24)) return;
    uint32_t eg = a.geo_root4[x >> 8];
    if (!(eg & TRIE_LEAF)) eg = a.geo_nodes[(size_t)eg * 256 + (x & 0xFFu)];
    uint32_t ei = a.ip_root4[x >> 8];
    if (!(ei & TRIE_LEAF)) ei = a.ip_nodes[(size_t)ei * 256 + (x & 0xFFu)];
    const uint32_t vg = eg & ~TRIE_LEAF, vi = ei & ~TRIE_LEAF;
    if ((eg & ei & TRIE_LEAF) && vg < 65536u && vi < 32768u) {
        if (out) out[x] = vg | (vi << 16);
        return;
    }
    const uint32_t idx = atomicAdd(esc_count, 1u);
    if (esc) {
        esc[idx] = make_uint2(eg, ei);
        out[x] = DIR_ESCAPE | idx;
    }
}

int launch_dir24(const VerdictArgs &a, void *out, void *esc, void *esc_count, void *stream) {
    hipLaunchKernelGGL(dir24_kernel, dim3((1u << 24) / 256), dim3(256), 0, (hipStream_t)stream, a, (uint32_t *)out, (uint2 *)esc, (uint32_t *)esc_count);
    return (int)hipGetLastError();
}

// Launch shape of the COARSE instantiation. The bitmap is staged per workgroup and held for the whole (persistent) launch, so the shape
// trades how many lookups end in LDS against the waves and the LDS left on a CU for the kernels of the main stream (DESIGN.md §6.1:
// the three shapes measured in the step). 1: two 1024-thread workgroups per CU, 64 KiB each (/19 blocks); 2: four 512-thread
// workgroups, 32 KiB each (/18); 3: one 1024-thread workgroup, 64 KiB; 0: no coarse level.
#ifndef PWAF_IPRES_SHAPE
#define PWAF_IPRES_SHAPE 1
#endif
IpresShape ipres_shape() {
    static const IpresShape shapes[4] = {{256, 0, 8}, {1024, 64 * 1024, 2}, {512, 32 * 1024, 4}, {1024, 64 * 1024, 1}};
#ifdef PWAF_PROFILING
    static const uint32_t pick = getenv("PWAF_IPRES_SHAPE") ? (uint32_t)atoi(getenv("PWAF_IPRES_SHAPE")) & 3u : (uint32_t)PWAF_IPRES_SHAPE;
#else
    const uint32_t pick = PWAF_IPRES_SHAPE;
#endif
    return shapes[pick];
}

// address lookups: one lane per request at full occupancy (grid-stride; 8 workgroups of 256 per CU, or ipres_shape() with a coarse bitmap)
int launch_ipres(const VerdictArgs &a, void *stream) {
    if (a.n == 0) return 0;
#ifdef PWAF_PROFILING
    static const uint32_t forced = getenv("PWAF_IPRES_BLOCKS") ? (uint32_t)atoi(getenv("PWAF_IPRES_BLOCKS")) : 0u;
#else
    const uint32_t forced = 0;
#endif
    if (a.dir_coarse != nullptr) {
        const IpresShape sh = ipres_shape();
        // (the kernel indexes the bitmap by the address alone: its size must be the one the shift implies)
        if (a.dir_coarse_shift > 17u || a.dir_coarse_bytes != (1u << 21) >> a.dir_coarse_shift || a.dir_coarse_bytes > sh.coarse_bytes) return (int)hipErrorInvalidValue;
        const uint32_t blocks = std::min<uint32_t>((a.n + sh.threads - 1) / sh.threads, forced ? forced : sh.wg_per_cu * std::max(1u, a.attr_blocks));
        if (a.ipres_packed) hipLaunchKernelGGL((ipres_kernel<true, true>), dim3(blocks), dim3(sh.threads), a.dir_coarse_bytes, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((ipres_kernel<false, true>), dim3(blocks), dim3(sh.threads), a.dir_coarse_bytes, (hipStream_t)stream, a);
        return (int)hipGetLastError();
    }
    const uint32_t blocks = std::min<uint32_t>((a.n + 255) / 256, forced ? forced : 8 * std::max(1u, a.attr_blocks));
    if (a.ipres_packed) hipLaunchKernelGGL((ipres_kernel<true, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((ipres_kernel<false, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// GeoIP records: ipres_kernel's geometry (grid-stride; 8 workgroups of 256 per CU)
int launch_georec(const GeoRecArgs &a, void *stream) {
    if (a.n == 0) return 0;
    const uint32_t blocks = std::min<uint32_t>((a.n + 255) / 256, 8 * std::max(1u, a.n_cus));
    hipLaunchKernelGGL(georec_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_attr(const VerdictArgs &a, void *stream) {
    if (a.n == 0) return 0;
    // rows, transposes, comparisons (after launch_ipres on the same stream). A persistent grid of six workgroups per CU at the default wave priority 0, while the filter
    // waves raise theirs to 3: the attribute waves take the issue slots the filter leaves idle instead of competing for them
    // (measured on MI355X next to the stream filter: 512 / 768 / 1024 / 1536 / 2048 workgroups -> 2.00 / 2.00 / 1.98 / 1.94 / 1.94 ms per step).
#ifdef PWAF_PROFILING
    static const uint32_t forced = getenv("PWAF_ATTR_BLOCKS") ? (uint32_t)atoi(getenv("PWAF_ATTR_BLOCKS")) : 0u;
#else
    const uint32_t forced = 0;
#endif
    const uint32_t blocks = std::min<uint32_t>((a.n_groups + 3) / 4, forced ? forced : 6 * std::max(1u, a.attr_blocks));
    const bool small = a.set_words <= 4 && a.cc_words <= 2 && a.iu_words[0] <= 1 && a.iu_words[1] <= 1 && a.acmp_words <= 1;
    if (a.ipres_packed && small) hipLaunchKernelGGL((attr_kernel<true, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    else if (a.ipres_packed) hipLaunchKernelGGL((attr_kernel<true, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    else if (small) hipLaunchKernelGGL((attr_kernel<false, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((attr_kernel<false, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace pwaf
