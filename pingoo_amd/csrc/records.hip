// records.hip — unpack_records_kernel: request records (include/pwaf.h, csrc/records.h) -> the device batch's columns; and, further down,
// pack_records_kernel with its entry point pwaf_export_records: the inverse.
//
// pwaf_evaluate_records uploads the records' bytes as they are, with the column offsets the host computed from the lengths; this kernel
// moves every value byte into its column arena (zero-padded for PWAF_ARENA_PAD bytes, as the host paths pad them) and transposes the fixed
// fields, so that run_pipeline then reads an ordinary device batch. A separate translation unit: kernels.hip's code objects are unchanged.
//
// One wave per record (a one-wave workgroup, so that __syncthreads orders the wave's LDS prefix without a cross-wave barrier): the
// lanes scan the lengths into LDS, then each lane takes 16-byte chunks of the record's concatenated values — aligned loads, since the
// values begin at a 16-byte boundary of a 16-byte aligned record — finds the value its first byte belongs to and writes the chunk's bytes
// to their columns (byte stores: destinations are at any offset). Short values therefore share a lane instead of idling 60 of them.
#include <hip/hip_runtime.h>

#include <string>

#include "colscan.h"
#include "records.h"

namespace pwaf {
namespace records {
namespace {

__global__ __launch_bounds__(64) void unpack_records_kernel(UnpackArgs a) {
    __shared__ uint32_t start[kMaxValues + 1];  // start[k] = first byte of value k inside the record's values; start[nv] = their total
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x == 0)  // the PWAF_ARENA_PAD zero bytes behind every column
        for (uint32_t f = lane; f < a.n_cols; f += 64) {
            uint8_t *p = a.arena + a.col_at[f] + a.off[(size_t)f * a.off_stride + a.n];
            for (uint32_t b = 0; b < PWAF_ARENA_PAD; b++) p[b] = 0;
        }
    for (uint32_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const uint8_t *r = a.rec + a.rec_off[i];
        pwaf_record_head h;
        load_head(r, &h);
        const uint32_t nv = h.n_values;
        if (lane == 0) {
            uint4 ip;
            memcpy(&ip, h.ip, 16);
            reinterpret_cast<uint4 *>(a.ip)[i] = ip;
            a.ip_is_v6[i] = h.ip_is_v6;
            a.flags[i] = h.flags;
            a.port[i] = h.port;
            if (a.country) {
                a.asn[i] = h.asn;
                a.country[i] = (uint16_t)(h.country[0] | (h.country[1] << 8));
            }
            start[0] = 0;
        }
        // inclusive prefix of the lengths, 64 at a time
        uint32_t carry = 0;
        for (uint32_t k0 = 0; k0 < nv; k0 += 64) {
            const uint32_t k = k0 + lane;
            uint32_t x = k < nv ? load_len(r, k) : 0u;
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(x, d, 64);
                if (lane >= d) x += y;
            }
            if (k < nv) start[k + 1] = carry + x;
            carry += __shfl(x, 63, 64);
        }
        __syncthreads();
        const uint32_t total = start[nv];
        const uint8_t *vals = r + values_offset(nv);
        for (uint32_t c = lane; (size_t)c * 16u < total; c += 64) {
            const uint32_t p0 = c * 16u;
            const uint4 q = reinterpret_cast<const uint4 *>(vals)[c];
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
            // the value holding byte p0: the last k with start[k] <= p0 (empty values share their start with the next one)
            uint32_t lo = 0, hi = nv;  // start[lo] <= p0 < start[hi]
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (start[mid] <= p0) lo = mid;
                else hi = mid;
            }
            uint32_t k = lo, base = start[k], next = start[k + 1];
            uint8_t *dst = a.arena + a.col_at[k] + a.off[(size_t)k * a.off_stride + i];  // byte `base` of the values goes to dst[0]
#pragma unroll
            for (uint32_t b = 0; b < 16; b++) {
                const uint32_t p = p0 + b;
                if (p < total) {
                    while (p >= next) {
                        k++;
                        base = next;
                        next = start[k + 1];
                        dst = a.arena + a.col_at[k] + a.off[(size_t)k * a.off_stride + i];
                    }
                    dst[p - base] = (uint8_t)(w[b >> 2] >> ((b & 3u) * 8u));
                }
            }
        }
        __syncthreads();  // (start[] is rewritten by the next record)
    }
}

// pack_records_kernel — the inverse: the requests a list names (idx[0 .. min(*n_idx, idx_cap))) -> records in buf (pwaf_export_records).
//
// One-wave workgroups again, in a persistent grid-stride loop over blocks of 64 list entries; the list's length is read on the device, so
// the launch follows the kernel that wrote it without the host in between. Per block:
//   sizing       lane j takes entry j: its request's column lengths give the record's size (0: index out of range, or a record past 32 bits)
//   reservation  a wave prefix sum places the lane's record inside the wave's range, ONE 64-bit atomicAdd on stats->bytes_needed (zeroed by
//                the memset in front of the launch) places the range. Nobody waits for anybody: no spin, no look-back. A record is written
//                iff its whole range lies below buf_cap; every earlier range then does too, so the written records are a prefix of buf.
//   copy         the wave walks its fitting records one after another, 64 lanes on one record: the lengths go into an LDS prefix (64 at
//                a time) with each value's source address beside it, head + lengths + padding leave as aligned 16-byte stores from an LDS
//                image, and each lane then owns 16-byte chunks of the value area — it finds the value holding the chunk's first byte
//                (unpack_records_kernel's binary search, mirrored), gathers up to 16 bytes from the arenas (sources at any alignment:
//                one 16-byte load per value the chunk crosses, cut and shifted into place) and issues one aligned
//                16-byte store. Bytes past the last value are 0: the record's tail padding falls out of the last chunk.
// The column descriptors are read from the kernel argument block (PackArgs::col) by a wave-uniform index while sizing; the prefix loop
// indexes them per lane, from a copy in LDS made once per workgroup.
// The workgroup is ONE wave: its lanes' LDS writes and reads are ordered by wave_sync (colscan.h), not by __syncthreads, which would cost a
// round trip to global memory per record.
// Both kernels keep their own prefix loops, search and gather, which colscan.h also has (wave_scan, copy_wave_range): written on shared
// functions, pack_records_kernel measured 3.6 % to 7 % slower on the MI355X and unpack_records_kernel compiled to another schedule
// (DESIGN.md §0.6).
__global__ __launch_bounds__(64) void pack_records_kernel(PackArgs a) {
    __shared__ uint32_t start[kMaxValues + 1];          // as in unpack_records_kernel
    __shared__ const uint8_t *src[kMaxValues];          // src[k] = the first byte of value k in its arena
    __shared__ __attribute__((aligned(16))) uint32_t pre[(kHead + 4u * kMaxValues + 15u) / 16u * 4u];  // head, lengths, padding: [0, values_offset)
    __shared__ pwaf_strcol cols[kMaxValues];            // PackArgs::col, for the per-lane index of the prefix loop (one round trip to memory less per record)
    const uint32_t lane = threadIdx.x;
    const uint32_t m = selected(a);
    if (blockIdx.x == 0 && lane == 0) a.stats->n_selected = m;
    for (uint32_t k = lane; k < a.n_cols; k += 64) cols[k] = a.col[k];
    wave_sync();
    for (uint64_t e0 = blockIdx.x * 64u; e0 < m; e0 += gridDim.x * 64u) {
        const uint64_t e = e0 + lane;
        const bool live = e < m;
        const uint32_t i = live ? a.idx[e] : 0xFFFFFFFFu;
        uint32_t size = 0, nv = 0;
        if (i < a.n) {
            const ExportShape s = export_shape(a, i);
            size = s.size32();
            nv = s.n_values;
        }
        // inclusive prefix of the sizes (64 x 2^32 fits 64 bits)
        uint64_t x = size;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        const uint64_t total = __shfl(x, 63, 64);
        uint64_t base = 0;
        if (lane == 0 && total) base = atomicAdd((unsigned long long *)&a.stats->bytes_needed, (unsigned long long)total);
        base = __shfl(base, 0, 64);
        const uint64_t at = base + (x - size);
        const bool fits = size && at + size <= a.buf_cap;  // (buf_cap <= 0xFFFFFFF0: `at` of a fitting record is below 2^32)
        if (live) a.rec_off[e] = fits ? (uint32_t)at : PWAF_RECORD_NONE;
        uint64_t todo = __ballot(fits);
        if (lane == 0 && todo) atomicAdd(&a.stats->n_written, (uint32_t)__popcll(todo));
        while (todo) {
            const int r = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t ri = __builtin_amdgcn_readlane(i, r), rnv = __builtin_amdgcn_readlane(nv, r), rsize = __builtin_amdgcn_readlane(size, r);
            uint8_t *const dst = a.buf + (uint32_t)__builtin_amdgcn_readlane((uint32_t)at, r);
            // (the head's loads are issued here, wave-uniform, and waited for only where lane 0 stores the head below: they travel beside the
            // offsets' loads instead of in front of them)
            pwaf_record_head h;
            fill_head(a, ri, rnv, rsize, &h);
            const uint32_t vo = values_offset(rnv);
            for (uint32_t k = rnv + lane; kHead + 4u * k < vo; k += 64) pre[kHead / 4u + k] = 0;  // the padding behind the lengths
            uint32_t carry = 0;
            for (uint32_t k0 = 0; k0 < rnv; k0 += 64) {
                const uint32_t k = k0 + lane;
                uint32_t len = 0;
                if (k < rnv) {
                    const pwaf_strcol c = cols[k];
                    len = col_len(c, ri);
                    src[k] = len ? c.data + c.offsets[ri] : nullptr;
                    pre[kHead / 4u + k] = len;
                }
                uint32_t p = len;
                for (uint32_t d = 1; d < 64; d <<= 1) {
                    const uint32_t y = __shfl_up(p, d, 64);
                    if (lane >= d) p += y;
                }
                if (k < rnv) start[k + 1] = carry + p;
                carry += __shfl(p, 63, 64);
            }
            if (lane == 0) {
                memcpy(pre, &h, kHead);
                start[0] = 0;
            }
            wave_sync();
            for (uint32_t c = lane; c * 16u < vo; c += 64) reinterpret_cast<uint4 *>(dst)[c] = reinterpret_cast<const uint4 *>(pre)[c];
            const uint32_t bytes = start[rnv];
            uint4 *const out = reinterpret_cast<uint4 *>(dst + vo);
            for (uint32_t c = lane; (uint64_t)c * 16u < bytes; c += 64) {
                const uint32_t p0 = c * 16u;
                uint32_t lo = 0, hi = rnv;  // start[lo] <= p0 < start[hi]: value lo holds byte p0 (and is not empty)
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (start[mid] <= p0) lo = mid;
                    else hi = mid;
                }
                uint32_t k = lo, first = start[k], next = start[k + 1];
                const uint8_t *s = src[k];  // byte `first` of the values is s[0]
                // the chunk is a few runs, one per value it crosses: each is ONE 16-byte load at the run's own (any) alignment, cut to the run's
                // length and shifted to its place. A load may run past its value, by less than 16 bytes: inside the arena or its PWAF_ARENA_PAD.
                const uint32_t end = p0 + 16u < bytes ? p0 + 16u : bytes;
                unsigned __int128 acc = 0;
                for (uint32_t p = p0; p < end;) {
                    while (p >= next) {
                        k++;
                        first = next;
                        next = start[k + 1];
                        s = src[k];
                    }
                    const uint32_t run = (next < end ? next : end) - p;
                    unsigned __int128 v;
                    memcpy(&v, s + (p - first), 16);
                    if (run < 16u) v &= ((unsigned __int128)1 << (8u * run)) - 1u;
                    acc |= v << (8u * (p - p0));
                    p += run;
                }
                uint4 q;
                memcpy(&q, &acc, 16);
                out[c] = q;
            }
            wave_sync();  // (start[], src[] and pre[] are rewritten by the next record)
        }
    }
}

}  // namespace

int launch_unpack_records(const UnpackArgs &a, void *stream) {
    if (a.n == 0) return 0;
    const uint32_t blocks = a.n < 16384u ? a.n : 16384u;
    hipLaunchKernelGGL(unpack_records_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// *stats zeroed (bytes_needed is the kernel's byte cursor), then the launch. An empty list needs the memset alone: it writes n_selected = 0.
int launch_pack_records(const PackArgs &a, void *stream) {
    if (hipMemsetAsync(a.stats, 0, sizeof(pwaf_export_stats), (hipStream_t)stream) != hipSuccess) return -1;
    if (a.idx_cap == 0) return 0;
    const uint32_t groups = (uint32_t)(((uint64_t)a.idx_cap + 63u) / 64u);
    const uint32_t blocks = groups < 8192u ? groups : 8192u;
    hipLaunchKernelGGL(pack_records_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace records
}  // namespace pwaf

extern "C" int pwaf_export_records(const pwaf_batch *in, const uint32_t *idx, uint32_t idx_cap, const uint32_t *n_idx, uint8_t *buf, size_t buf_cap,
                                   uint32_t *rec_off, pwaf_export_stats *stats, void *stream) {
    namespace R = pwaf::records;
    using pwaf::fail;
    if (!in || !rec_off || !stats || (idx_cap && !idx)) return fail(PWAF_E_INVALID_ARG, "pwaf_export_records: NULL argument");
    if (int rc = pwaf::check_batch_header(in)) return rc;
    if (in->n_headers > R::kMaxValues - PWAF_N_FIELDS) return fail(PWAF_E_INVALID_ARG, "pwaf_export_records: more header columns than a record can carry");
    if (in->n_headers && !in->headers) return fail(PWAF_E_INVALID_ARG, "pwaf_batch.headers is NULL");
    if ((uintptr_t)stats & 7u) return fail(PWAF_E_INVALID_ARG, "pwaf_export_records: stats is not 8-byte aligned");
    if ((uintptr_t)buf & 15u) return fail(PWAF_E_INVALID_ARG, "pwaf_export_records: buf is not 16-byte aligned");
    if (!buf && buf_cap) return fail(PWAF_E_INVALID_ARG, "pwaf_export_records: buf is NULL");
    if (buf_cap > R::kMaxRecord) return fail(PWAF_E_INVALID_ARG, "pwaf_export_records: buf_cap exceeds 0xFFFFFFF0 (rec_off is 32 bits wide)");
    if (in->n) {
        for (int f = 0; f < PWAF_N_FIELDS; f++)
            if (!in->field[f].data || !in->field[f].offsets) return fail(PWAF_E_INVALID_ARG, "pwaf_batch.field column is NULL");
        if (!in->ip || !in->ip_is_v6 || !in->port || !in->flags) return fail(PWAF_E_INVALID_ARG, "pwaf_batch numeric column is NULL");
    }
    static_assert(sizeof(pwaf_export_stats) == 16, "pwaf_export_stats layout");
    static_assert(sizeof(R::PackArgs) <= 4096, "PackArgs travels in the kernel argument block");
    R::PackArgs a{};
    for (int f = 0; f < PWAF_N_FIELDS; f++) a.col[f] = in->field[f];
    for (uint32_t h = 0; h < in->n_headers; h++) a.col[PWAF_N_FIELDS + h] = in->headers[h];
    a.n = in->n;
    a.n_cols = PWAF_N_FIELDS + in->n_headers;
    a.ip = in->ip, a.ip_is_v6 = in->ip_is_v6, a.flags = in->flags, a.port = in->port, a.asn = in->asn, a.country = in->country;
    a.idx = idx, a.n_idx = n_idx, a.idx_cap = idx_cap;
    a.buf = buf, a.buf_cap = buf_cap, a.rec_off = rec_off, a.stats = stats;
    if (in->memory == PWAF_MEM_HOST) {
        uint32_t bad = 0;
        if (!R::export_host(a, &bad)) return fail(PWAF_E_BATCH, "pwaf_export_records: list entry " + std::to_string(bad) + " (request " + std::to_string(idx[bad]) + "): offsets decrease");
        return PWAF_OK;
    }
    if (R::launch_pack_records(a, stream)) return fail(PWAF_E_DEVICE, "pack_records_kernel launch failed");
    return PWAF_OK;
}
