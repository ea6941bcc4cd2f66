// records.hip — unpack_records_kernel: request records (include/pwaf.h, csrc/records.h) -> the device batch's columns.
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

}  // namespace

int launch_unpack_records(const UnpackArgs &a, void *stream) {
    if (a.n == 0) return 0;
    const uint32_t blocks = a.n < 16384u ? a.n : 16384u;
    hipLaunchKernelGGL(unpack_records_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace records
}  // namespace pwaf
