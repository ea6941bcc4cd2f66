// service.h — what the batch services' headers share (records.h, clientid.h, cookie.h, pow.h, derive.h, powbody.h): the host/device
// switch, the list a call may select its requests with, the arithmetic of a reduce-then-scan over tiles that fills a column with a cap, and
// for the units' entry points the error record and the argument checks they repeat. Plain C++: compiled by hipcc for both sides and by g++
// for the stand-alone host programs of the tests and tools. No HIP include. colscan.h holds the device code that goes with it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "pwaf.h"

// an inline function of a service header: host and device under hipcc, host under g++
#if defined(__HIPCC__) || defined(__HIP__)
#define PWAF_SVC_HD __host__ __device__ inline
#else
#define PWAF_SVC_HD inline
#endif

namespace pwaf {

// ---- the list (idx, n_idx, idx_cap) ----------------------------------------------------------------------------------------------------
// how many entries of a list are looked at: min(*n_idx, idx_cap); n_idx NULL: idx_cap
PWAF_SVC_HD uint32_t list_length(const uint32_t *n_idx, uint32_t idx_cap) {
    if (!n_idx) return idx_cap;
    const uint32_t k = *n_idx;
    return k < idx_cap ? k : idx_cap;
}
// the entries of a call over n requests: idx NULL means every request, entry e is request e
PWAF_SVC_HD uint32_t selected(const uint32_t *idx, const uint32_t *n_idx, uint32_t idx_cap, uint32_t n) { return idx ? list_length(n_idx, idx_cap) : n; }
PWAF_SVC_HD uint32_t request_of(const uint32_t *idx, uint32_t e) { return idx ? idx[e] : e; }

// ---- a scan over tiles that fills a column ---------------------------------------------------------------------------------------------
PWAF_SVC_HD uint32_t tiles(uint32_t n, uint32_t tile) { return (uint32_t)(((uint64_t)n + tile - 1u) / tile); }
// 64-bit words of a tile array: one per tile and one for the total, rounded up to even
PWAF_SVC_HD uint32_t tile_stride(uint32_t n_tiles) { return (n_tiles + 2u) & ~1u; }
// the column's bytes were all written and so is its pad
PWAF_SVC_HD bool fits(uint64_t bytes, uint64_t cap) { return bytes + PWAF_ARENA_PAD <= cap; }
// the pad: the 16 bytes behind the column's last byte, those that lie below cap
PWAF_SVC_HD void write_pad_byte(uint8_t *data, uint64_t total, uint64_t cap, uint32_t k) {
    if (total + k < cap) data[total + k] = 0;
}
// a value of len bytes at byte `at` of the column: its bytes below cap
PWAF_SVC_HD void append_clipped(uint8_t *data, uint64_t cap, uint64_t at, const uint8_t *src, uint32_t len) {
    if (len && at < cap) memcpy(data + at, src, (size_t)(at + len <= cap ? len : cap - at));
}

// ---- behind the C ABI --------------------------------------------------------------------------------------------------------------------
int fail(int code, const std::string &msg);  // program_api.cpp: records pwaf_last_error() and returns code

// The checks that several entry points make, each 0 or the refusal it has recorded. `fn` is the entry point's name.
inline int check_batch_header(const pwaf_batch *in) {
    if (in->struct_size != sizeof(pwaf_batch)) return fail(PWAF_E_INVALID_ARG, "pwaf_batch.struct_size mismatch");
    if (in->memory != PWAF_MEM_HOST && in->memory != PWAF_MEM_DEVICE) return fail(PWAF_E_INVALID_ARG, "pwaf_batch.memory is neither HOST nor DEVICE");
    return 0;
}
inline int check_list(const char *fn, const uint32_t *idx, uint32_t idx_cap, const uint32_t *n_idx) {
    if (!idx && (idx_cap || n_idx)) return fail(PWAF_E_INVALID_ARG, std::string(fn) + ": idx is NULL with idx_cap != 0 or a non-NULL n_idx");
    return 0;
}
// what a client id is made of: the address, the User-Agent and the host of every request
inline int check_client_columns(const pwaf_batch *in) {
    const pwaf_strcol &ua = in->field[PWAF_FIELD_USER_AGENT], &host = in->field[PWAF_FIELD_HOST];
    if (!in->n) return 0;
    if (!in->ip || !in->ip_is_v6) return fail(PWAF_E_INVALID_ARG, "pwaf_batch.ip or ip_is_v6 is NULL");
    if (!ua.data || !ua.offsets || !host.data || !host.offsets) return fail(PWAF_E_INVALID_ARG, "pwaf_batch User-Agent or host column is NULL");
    return 0;
}
// an output column of n values; `what`: the entry point and the column, "pwaf_x: nonce"
inline int check_derived_col(const std::string &what, uint32_t n, const pwaf_derived_col &c) {
    if (n && !c.offsets) return fail(PWAF_E_INVALID_ARG, what + " offsets is NULL");
    if (!c.data && c.cap) return fail(PWAF_E_INVALID_ARG, what + " data is NULL with cap != 0");
    if ((uintptr_t)c.data & 15u) return fail(PWAF_E_INVALID_ARG, what + " data is not 16-byte aligned");
    if ((uintptr_t)c.offsets & 3u) return fail(PWAF_E_INVALID_ARG, what + " offsets is not 4-byte aligned");
    return 0;
}
// `need`: the text that names the size, "pwaf_x_scratch_bytes(n)"
inline int check_scratch(const char *fn, const void *scratch, size_t have, size_t want, const char *need) {
    if (!scratch || ((uintptr_t)scratch & 15u) || have < want)
        return fail(PWAF_E_INVALID_ARG, std::string(fn) + ": scratch is NULL, not 16-byte aligned or smaller than " + need);
    return 0;
}

}  // namespace pwaf
