// wave.h — what the gfx950 kernel units (*.hip) share below the level of any pipeline stage: explicit address spaces, the 16-byte
// vector types, and the wave-level helpers (the uniform wave index, descriptor loads into scalar registers, the DPP reductions,
// v_writelane parking). Device code only: included by the .hip units, never by host C++.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pwaf {

static constexpr uint32_t kNone = 0xFFFFFFFFu;

// Explicit address spaces: a generic pointer that may be LDS or global makes the compiler emit FLAT loads for the table
// lookups (one flat_load per input byte through the texture path instead of ds_read_u16 — measured 5x slower).
#define PWAF_LDS __attribute__((address_space(3)))
#define PWAF_GLOBAL __attribute__((address_space(1)))
typedef const PWAF_LDS uint16_t *lds_u16_ptr;
typedef const PWAF_GLOBAL uint16_t *glb_u16_ptr;
typedef const PWAF_LDS uint32_t *lds_u32_ptr;
typedef const PWAF_LDS uint8_t *lds_u8_ptr;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));  // 16 bytes at any byte address (gfx950 global loads need no alignment)

// The wave's index in its workgroup, as a value the compiler KNOWS to be wave-uniform (threadIdx.x >> 6 is, but is not provably so:
// everything derived from it — slab and group numbers, loop bounds, base addresses — would be computed per lane in vector registers
// and every branch on it would be an exec-mask branch).
__device__ __forceinline__ uint32_t wave_index() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// A pass descriptor read from the device-resident table into SCALAR registers (the address is wave-uniform; through a plain
// reference every use inside the hot loops became a reload from memory — the compiler must assume the kernel's own stores alias it —
// and the filter launch went from 0.74 to 0.85 ms).
template <class T>
__device__ __forceinline__ T load_descriptor(const T *p) {
    static_assert(sizeof(T) % 4 == 0, "descriptor size");
    typedef uint32_t __attribute__((may_alias)) word_t;  // (the descriptor's members are read and written as plain words)
    uint32_t w[sizeof(T) / 4];
    const word_t *s = reinterpret_cast<const word_t *>(p);
#pragma unroll
    for (size_t i = 0; i < sizeof(T) / 4; i++) w[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)s[i]);
    T out;
    __builtin_memcpy(&out, w, sizeof(T));
    return out;
}

// Bitwise OR over the 64 lanes, in the vector ALU (DPP row shifts + the two cross-row broadcasts): no LDS, no memory.
__device__ __forceinline__ uint32_t wave_or(uint32_t x) {
#define PWAF_DPP_OR(ctrl, rows) x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, (ctrl), (rows), 0xF, true)
    PWAF_DPP_OR(0x111, 0xF);  // row_shr:1
    PWAF_DPP_OR(0x112, 0xF);  // row_shr:2
    PWAF_DPP_OR(0x114, 0xF);  // row_shr:4
    PWAF_DPP_OR(0x118, 0xF);  // row_shr:8   -> lane 15 of each row holds its row
    PWAF_DPP_OR(0x142, 0xA);  // row_bcast:15 into rows 1 and 3
    PWAF_DPP_OR(0x143, 0xC);  // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave
#undef PWAF_DPP_OR
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// A wave-uniform 64-bit mask into ONE lane of a register pair (v_writelane_b32): `x = lane == l ? m : x` without the compare of the
// lane id, the two selects and the moves of the scalar pair into vector registers — two vector instructions instead of seven where a
// kernel is bound by vector-ALU issue (attr_kernel: one such parking per present membership bit and per comparison atom). gfx9 lets
// a VALU instruction read ONE scalar register, M0 not counted: the lane select travels in M0. (No compiler builtin for v_writelane.)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"  // (M0 is a reserved register: naming it as clobbered is what is meant)
__device__ __forceinline__ void park64(uint32_t &lo, uint32_t &hi, const unsigned long long m, const uint32_t l) {
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tv_writelane_b32 %0, %2, m0\n\tv_writelane_b32 %1, %4, m0"
                 : "+v"(lo), "+v"(hi)
                 : "s"((uint32_t)m), "s"(l), "s"((uint32_t)(m >> 32))
                 : "m0");
}
#pragma clang diagnostic pop

// Inclusive prefix sum over the 64 lanes, same DPP network (no LDS round trips, unlike __shfl_up).
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t x) {
#define PWAF_DPP_ADD(ctrl, rows) x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, (ctrl), (rows), 0xF, true)
    PWAF_DPP_ADD(0x111, 0xF);  // row_shr:1
    PWAF_DPP_ADD(0x112, 0xF);  // row_shr:2
    PWAF_DPP_ADD(0x114, 0xF);  // row_shr:4
    PWAF_DPP_ADD(0x118, 0xF);  // row_shr:8   -> inclusive scan inside each row of 16
    PWAF_DPP_ADD(0x142, 0xA);  // row_bcast:15: rows 1 and 3 add the total of the row before
    PWAF_DPP_ADD(0x143, 0xC);  // row_bcast:31: rows 2 and 3 add the total of rows 0-1
#undef PWAF_DPP_ADD
    return x;
}

}  // namespace pwaf
