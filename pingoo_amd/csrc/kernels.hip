// kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels of the WAF batch matcher: the overview of the pipeline, the three
// small kernels (copy_args_kernel, fcmp_kernel, residual_kernel) and the per-device configure_kernels. The filter stage is filter.hip, the
// DFA scans scan.hip, the confirm tier confirm.hip, the verdict stage verdict.hip, the attribute stage attr.hip; wave.h holds the
// wave-level helpers all of them share, hitrec.h the hit record that the scans, the confirm tier, fcmp_kernel and residual_kernel write.
//
// Data model: every predicate ("atom") of the compiled rule set is a COLUMN. The verdict kernel
// handles requests in GROUPS of 64 (one wavefront); for a group a column is one 64-bit word whose bit r says
// "atom holds for request 64*g + r", so rule evaluation is bit-parallel over 64 requests per ALU op with one
// lane per RULE — instead of one interpreter walk per rule per request (pingoo/rules.rs:37-51,
// http_listener.rs:251-264).
//
//   filter_kernel    (filter.hip, with resolve_kernel / bitcount_kernel / compact_kernel) the launch that streams the request bytes: every string pass whose patterns all have a literal factor sits behind
//                    a bucketed shift-or BIGRAM PREFILTER. A field's arena is one flat byte stream; per byte one independent lookup of
//                    a 16 KiB LDS table and two vector ops; the requests overlapping a completed window become CANDIDATES
//                    (resolve_kernel: flagged chunks -> bitmap; bitcount / compact_kernel: bitmap -> dense ascending list).
//   lscan_kernel     (scan.hip, with lscan_plan_kernel) every list-driven pass of a phase in one launch: the candidates of the filtered passes, then the gap passes
//                    (patterns with wide gaps, visited only by requests whose prefilter factor matched). One listed request per lane
//                    through the pass's DFA, hot rows in LDS. What a request matched is written as one 4-byte hit record (two atoms
//                    inline, more through an overflow chain): lanes never share state, no atomics on the common path.
//   scan_kernel<CH>  (scan.hip) a pass without a usable prefilter: the round-1 design, a DFA over EVERY request (one persistent workgroup per CU,
//                    lanes pull the next request of their wave's slab when done, hot rows in LDS, cold rows from the L2-resident table).
//   fcmp_kernel      (here, like residual_kernel and copy_args_kernel) predicates between two request fields (one lane per request compares the byte ranges).
//   attr_kernel      (attr.hip, with ipres_kernel / georec_kernel / dir24_kernel) on the engine's low-priority side stream, forked after the filter launches: everything that is not a string scan — GeoIP record and
//                    ip-list membership (DIR-24-8 table + radix tries), country / integer-set membership, length / port / asn
//                    comparisons — reduced per 64-request group to (column, 64-request mask) pairs with wave ballots.
//   verdict_kernel   (verdict.hip; verdict2_kernel is its entry-list form, the default) per group: turns hit records and pairs into LDS column words, finds the candidate rules through trigger lists,
//                    evaluates each candidate's DNF with one lane per rule, resolves first-match-wins, writes verdicts, action
//                    counters and the compacted index list of non-Allow requests.
//
// No MFMA: this is byte/integer work bounded by LDS lookups per input byte and HBM streaming (filter_kernel runs
// at 0.47 of the HBM roofline, bound by the bank conflicts of its table gather).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <set>

#include "hitrec.h"
#include "kernels.h"
#include "residual.h"
#include "wave.h"

namespace pwaf {

// The batch's launch descriptors, host to device in ONE launch: `src` is page-locked host memory (device-visible: the lanes read it
// over the link, 16 bytes each), `dst` device memory; both 16-byte aligned, bytes rounded up to 16 by the caller's 256-byte parts.
// The same launch clears the batch's zeroed block (control words, candidate / visited / walk bitmaps) when the caller hands it over: a memset
// of its own was one more launch (8 us) in front of every batch.
__global__ __launch_bounds__(256) void copy_args_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t n16, uint4 *__restrict__ zero, uint32_t z16) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n16; i += gridDim.x * 256u) dst[i] = src[i];
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < z16; i += gridDim.x * 256u) zero[i] = make_uint4(0u, 0u, 0u, 0u);
}
int upload_args_block(const void *host_pinned, void *dev, size_t bytes, void *zero, size_t zero_bytes, void *stream) {
    const uint32_t n16 = (uint32_t)((bytes + 15) / 16), z16 = (uint32_t)(zero_bytes / 16);  // (the zeroed block is a multiple of 256 bytes)
    if (n16 == 0 && z16 == 0) return 0;
    const uint32_t blocks = std::max(std::min<uint32_t>((n16 + 255) / 256, 64u), std::min<uint32_t>((z16 + 2047) / 2048, 1024u));
    hipLaunchKernelGGL(copy_args_kernel, dim3(std::max(1u, blocks)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)host_pinned, (uint4 *)dev, n16, (uint4 *)zero, z16);
    return (int)hipGetLastError();
}

// fcmp_kernel: field-against-field atoms (one string field of a request against another: ==, contains, starts_with, ends_with, or a
// comparison of their lengths). One lane per request; rare in rule sets, so plain byte loops (both fields were just streamed: cache hits).
__global__ __launch_bounds__(256) void fcmp_kernel(FcmpArgs a) {
    const SlowCtx ctx{nullptr, nullptr, a.pool, a.pool_count, a.status, a.pool_cap};
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < a.n; r += gridDim.x * 256u) {
        Hits h{0, 0, kNone};
        for (uint32_t k = 0; k < a.n_atoms; k++) {
            const uint32_t op = a.atoms[k] & 0xFFu, sa = (a.atoms[k] >> 8) & 0xFFu, sb = (a.atoms[k] >> 16) & 0xFFu;
            const uint32_t a0 = a.off[sa][r], la = a.off[sa][r + 1] - a0, b0 = a.off[sb][r], lb = a.off[sb][r + 1] - b0;
            const uint8_t *x = a.data[sa] + a0, *y = a.data[sb] + b0;
            bool holds = false;
            auto same = [&](const uint8_t *p, const uint8_t *q, uint32_t len) {
                for (uint32_t i = 0; i < len; i++)
                    if (p[i] != q[i]) return false;
                return true;
            };
            switch (op) {
                case FC_EQ: holds = la == lb && same(x, y, la); break;
                case FC_STARTS: holds = la >= lb && same(x, y, lb); break;
                case FC_ENDS: holds = la >= lb && same(x + (la - lb), y, lb); break;
                case FC_CONTAINS:
                    if (la >= lb)
                        for (uint32_t s = 0; s + lb <= la && !holds; s++) holds = same(x + s, y, lb);
                    break;
                case FC_LEN_EQ: holds = la == lb; break;
                case FC_LEN_LT: holds = la < lb; break;
                default: holds = la <= lb; break;
            }
            if (holds) h = record_atom(ctx, k, h);
        }
        a.rec[r] = record_of_hits(h);
    }
}

int launch_fcmp(const FcmpArgs &a, void *stream) {
    if (a.n == 0 || a.n_atoms == 0) return 0;
    hipLaunchKernelGGL(fcmp_kernel, dim3(std::min<uint32_t>((a.n + 255) / 256, 4096u)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// residual_kernel: the rules no column form exists for (residual.h), interpreted with one lane per request. The interpreter's value
// stack and heap live in the lane's private memory: this is the slow path by design (a rule set without such rules never launches it).
__global__ __launch_bounds__(128) void residual_kernel(ResidualArgs a) {
    const SlowCtx ctx{nullptr, nullptr, a.pool, a.pool_count, a.status, a.pool_cap};
    rvm::Machine m;
    m.blob = a.blob;
    m.h = reinterpret_cast<const rvm::Header *>(a.blob);
    m.q.data = a.data;
    m.q.off = a.off;
    for (uint32_t r = blockIdx.x * 128u + threadIdx.x; r < a.n; r += gridDim.x * 128u) {
        m.q.r = r;
        m.q.ip = a.ip + (size_t)r * 16;
        m.q.v6 = a.ip_is_v6[r];
        m.q.port = a.port[r];
        uint32_t asn = 0, country = (uint32_t)'X' | ((uint32_t)'X' << 8);  // the default record {0, "XX"} (http_listener.rs:148-156)
        if (a.asn != nullptr) {
            asn = a.asn[r];
            const uint32_t cc = a.country[r], c0 = (cc & 0xFFu) - 'A', c1 = (cc >> 8) - 'A';
            if (c0 < 26u && c1 < 26u) country = cc;  // (invalid input is treated as "XX", like the attribute kernel does)
        } else if (a.has_geo) {
            // GeoipDB::lookup (pingoo/geoip.rs:73-91): loopback / multicast are "not found"
            const uint8_t *ip = m.q.ip;
            bool walk;
            if (!m.q.v6) walk = !(ip[0] == 127u || (ip[0] & 0xF0u) == 0xE0u);
            else {
                bool loopback = ip[15] == 1;
                for (int k = 0; k < 15; k++) loopback = loopback && ip[k] == 0;
                walk = !(loopback || ip[0] == 0xFFu);
            }
            if (walk) {
                uint32_t e = (m.q.v6 ? a.geo_root6 : a.geo_root4)[((uint32_t)ip[0] << 8) | ip[1]];
                for (uint32_t k = 2; !(e & TRIE_LEAF); k++) e = a.geo_nodes[(size_t)e * 256 + ip[k]];
                const GeoRec g = a.geo_recs[e & ~TRIE_LEAF];
                asn = g.asn;
                country = g.country;
            }
        }
        m.q.asn = asn;
        m.q.country = country;
        Hits h{0, 0, kNone};
        for (uint32_t k = 0; k < a.n_rules; k++) {
            const uint32_t res = rvm::run_rule(m, k);
            if (res == 1u) h = record_atom(ctx, k, h);
            // execution errors are COUNTED per rule (the reference logs each one, pingoo/rules.rs:41-45; here: pwaf_engine_rule_errors):
            // one atomic per wave and rule that saw any
            const unsigned long long em = __ballot(res == 2u);
            if (em != 0 && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(em)) atomicAdd(&a.rule_errors[k], (unsigned long long)__builtin_popcountll(em));
        }
        a.rec[r] = h.ovf != kNone ? (REC_OVERFLOW | h.ovf) : (h.a0 | (h.a1 << 15));  // (record_of_hits written out: through the helper two registers of this kernel swap names, and the split changes no kernel)
    }
}

int launch_residual(const ResidualArgs &a, void *stream) {
    if (a.n == 0 || a.n_rules == 0) return 0;
    hipLaunchKernelGGL(residual_kernel, dim3(std::min<uint32_t>((a.n + 127) / 128, 8192u)), dim3(128), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// hipFuncSetAttribute applies to the CURRENT device: every device an engine is created on needs its own call (a per-thread
// or per-process "already configured" flag left the second device of a multi-GPU host at the 64 KiB default).
int configure_kernels(int device) {
    static std::mutex mu;
    static std::set<int> done;
    std::lock_guard<std::mutex> lock(mu);
    if (done.count(device)) return 0;
    if (int e = configure_scan_kernels()) return e;
    if (int e = configure_filter_kernels()) return e;
    if (int e = configure_verdict_kernels()) return e;
    done.insert(device);
    return 0;
}

}  // namespace pwaf
