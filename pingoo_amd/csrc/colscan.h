// colscan.h — what the batch services' kernels share (records.hip, records_scan.hip, clientid.hip, derive.hip, powbody.hip): the wave and
// workgroup prefix sums of their reduce-then-scan launches, and the copy of a wave's values into ONE contiguous range of a column, 16
// aligned output bytes at a time. Device only, beside wave.h and hitrec.h; service.h holds the host/device arithmetic that goes with it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace pwaf {

__device__ __forceinline__ uint64_t wave_sum(uint64_t x) {
    for (uint32_t d = 32; d; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}
__device__ __forceinline__ uint64_t wave_min(uint64_t x) {
    for (uint32_t d = 32; d; d >>= 1) {
        const uint64_t y = __shfl_xor(x, d, 64);
        x = y < x ? y : x;
    }
    return x;
}
// inclusive prefix inside the wave. (Beside wave.h's DPP wave_scan_add, which is 32 bits wide: this one is templated, for 64-bit sums.)
template <class T>
__device__ __forceinline__ T wave_scan(T x, uint32_t lane) {
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}
// A wave's LDS instructions execute in program order: what orders its lanes' LDS writes against its other lanes' LDS reads is that the
// compiler keeps them in program order across the point where the lanes exchange roles, not a barrier. (__syncthreads would also wait for
// every store to global memory to be acknowledged: a round trip that nothing needs.)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// inclusive prefix over the workgroup (W waves; every thread calls it); *total = the workgroup's sum. wsum: W words of LDS.
template <uint32_t W>
__device__ __forceinline__ uint64_t block_scan(uint64_t x, uint64_t *wsum, uint64_t *total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t incl = wave_scan(x, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint64_t all = 0;
#pragma unroll
    for (uint32_t w = 0; w < W; w++) {
        const uint64_t s = wsum[w];
        if (w < wave) incl += s;
        all += s;
    }
    *total = all;
    __syncthreads();  // (wsum is rewritten by the next call)
    return incl;
}
// tile[0 .. nt): sums -> exclusive bases, in place, by one workgroup of W waves, 64 W tiles a step with the carry in a register; returns
// the total (every thread calls it and gets it).
template <uint32_t W>
__device__ __forceinline__ uint64_t scan_tile_bases(uint64_t *tile, uint32_t nt, uint64_t *wsum) {
    uint64_t carry = 0;
    for (uint32_t t0 = 0; t0 < nt; t0 += 64u * W) {
        const uint32_t t = t0 + threadIdx.x;  // (the callers' nt is at most 2^16: no wrap)
        const uint64_t x = t < nt ? tile[t] : 0u;
        uint64_t total;
        const uint64_t incl = block_scan<W>(x, wsum, &total);
        if (t < nt) tile[t] = carry + incl - x;
        carry += total;
    }
    return carry;
}

// A wave copies its 64 values, ONE contiguous range [base, base + range) of the column `data`: woff[j] = where value j begins inside the
// range, woff[64] = range (> 0), wsrc[j] = its first byte in memory. The lanes take the aligned 16-byte chunks of the output that hold a
// byte of the range: one aligned 16-byte store when the whole chunk is the wave's and lies below cap, else byte by byte (a neighbouring
// wave owns the rest of a boundary chunk). Nothing is stored at or beyond cap. The caller's wave_sync stands between its writes of woff
// and wsrc and this call.
__device__ __forceinline__ void copy_wave_range(uint8_t *data, uint64_t cap, uint64_t base, uint32_t range, const uint32_t *woff, const uint8_t *const *wsrc, uint32_t lane) {
    const uint64_t end = base + range;
    for (uint64_t ck = (base >> 4) + lane; ck * 16u < end; ck += 64) {
        const uint64_t p0 = ck * 16u, lo64 = p0 > base ? p0 : base, hi64 = p0 + 16u < end ? p0 + 16u : end;
        const uint32_t lo = (uint32_t)(lo64 - base), hi = (uint32_t)(hi64 - base), shift = (uint32_t)(lo64 - p0);  // inside the range; the chunk's first own byte
        uint32_t l = 0, h = 64;  // woff[l] <= lo < woff[h]: value l holds byte lo (and is not empty)
        while (h - l > 1) {
            const uint32_t mid = (l + h) >> 1;
            if (woff[mid] <= lo) l = mid;
            else h = mid;
        }
        // the chunk is a few runs, one per value it crosses: each is ONE 16-byte load at the run's own (any) alignment, cut to the run's length
        // and shifted to its place. A load may pass its value's end by fewer than 16 bytes: inside the arena or its PWAF_ARENA_PAD.
        uint32_t k = l, first = woff[k], next = woff[k + 1];
        const uint8_t *src = wsrc[k];  // byte `first` of the range is src[0]
        unsigned __int128 acc = 0;
        for (uint32_t p = lo; p < hi;) {
            while (p >= next) {  // (p < hi <= range == woff[64]: k stays below 64)
                k++;
                first = next;
                next = woff[k + 1];
                src = wsrc[k];
            }
            const uint32_t run = (next < hi ? next : hi) - p;
            unsigned __int128 v;
            memcpy(&v, src + (p - first), 16);
            if (run < 16u) v &= ((unsigned __int128)1 << (8u * run)) - 1u;
            acc |= v << (8u * (p - lo + shift));
            p += run;
        }
        if (hi - lo == 16u && p0 + 16u <= cap) {
            uint4 q;
            memcpy(&q, &acc, 16);
            *reinterpret_cast<uint4 *>(data + p0) = q;
        } else {
            for (uint32_t b = shift; b < shift + (hi - lo); b++)
                if (p0 + b < cap) data[p0 + b] = (uint8_t)(acc >> (8u * b));
        }
    }
}

// Host side: a kernel whose one argument is its Args struct. The launch's own status (hipLaunchKernel returns it): an earlier error that
// still sticks to the thread is neither read nor cleared here.
template <class Args>
inline int launch_args(void (*kernel)(Args), uint32_t grid, uint32_t block, const Args &a, hipStream_t s) {
    Args copy = a;
    void *args[] = {&copy};
    return hipLaunchKernel(reinterpret_cast<const void *>(kernel), dim3(grid), dim3(block), args, 0, s) == hipSuccess ? 0 : -1;
}

}  // namespace pwaf
