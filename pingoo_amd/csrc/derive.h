// derive.h — the reference's own derivation of host, path and User-Agent (include/pwaf.h: pwaf_derive_batch) for a whole batch: what
// pwaf_derive_host / _path / _user_agent (program_api.cpp) answer per request, as three contiguous columns in request order.
//   path        uri.path().trim_end_matches('/')                                                   http_utils.rs:114-116
//   user_agent  the header's to_str() (every byte TAB or 0x20..0x7E), trim(), at most 256 bytes     http_listener.rs:159-165
//   host        uri.host() trimmed (0x09..0x0D, 0x20) when there is one, else the Host header
//               taken like the User-Agent; at most 256 bytes either way                             http_listener.rs:284-296
//
// One header, compiled three ways, like records.h and clientid.h: by derive.hip for the device (derive_span_kernel, derive_base_kernel,
// derive_copy_kernel), by the same unit for the HOST mode (derive_host below) and by tests/derive_host.cpp (g++ under the sanitizers, which
// also runs the three phases as loops over tiles: span_tile / base_column / copy_tile). No HIP include.
//
// A derived value is a sub-slice [start, start + len) of its raw value, so all a request costs is finding that slice: the whitespace runs
// at both ends (the trailing slashes of a path), and for a header value the byte check of what is left. A header value is kept only when
// at most 256 bytes are left between its runs, and a byte that fails the check is never whitespace, so it is never inside a run: the check
// looks at the kept bytes alone and a 40 KiB value costs its two ends. Bytes are looked at 16 at a time (classes below); the only
// difference between the compilations is that load (load16): the device reads 16 bytes and masks, which may run past the value by fewer
// than 16 bytes (inside the arena or its PWAF_ARENA_PAD), the host reads exactly the bytes of the value. No load begins before its value.
//
// The batch is reduce-then-scan over tiles of kTile requests (the scheme of records.h): phase 1 stores every kept length one slot up in
// the output offsets and a 64-bit sum per tile and column, phase 2 turns the tile sums into exclusive bases (slot n_tiles: the column's
// total), phase 3 rescans each tile from its base in place and copies the kept bytes. No phase-3 tile needs another one's result.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "pwaf.h"
#include "service.h"

namespace pwaf {
namespace derive {

static constexpr uint32_t kTile = 256;       // requests per tile: one workgroup of the span launch and of the copy launch
static constexpr uint32_t kStep = 256;       // tiles per step of the base launch
static constexpr uint32_t kCopyGroup = kTile;  // requests per workgroup of the copy launch (it reads ONE base per column)
static constexpr uint32_t kMaxKept = 256;    // heapless::String<256>
static constexpr uint32_t kMaxRequests = 0xFFFFFFF0u / kMaxKept;  // a derived host / User-Agent column stays below 32 bits
enum Column : uint32_t { kHost = 0, kPath = 1, kUserAgent = 2, kColumns = 3 };
static_assert(sizeof(pwaf_derive_stats) == 32, "pwaf_derive_stats layout");

// ---- sixteen bytes at a time ---------------------------------------------------------------------------------------------------------
struct Chunk {
    uint64_t lo, hi;  // byte k of the chunk in bits [8k, 8k + 8) of lo (k < 8) / of hi
};
// The `run` (1..16) bytes at s; what the other bytes of the chunk hold is unspecified (every user masks with run_bits).
PWAF_SVC_HD Chunk load16(const uint8_t *s, uint32_t run) {
    Chunk v{0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
    (void)run;
    memcpy(&v, s, 16);  // one 16-byte load at the value's own alignment; it may pass the value's end by up to 15 bytes
#else
    memcpy(&v, s, run);  // not a byte outside the value: a host column has no pad
#endif
    return v;
}
PWAF_SVC_HD uint32_t run_bits(uint32_t run) { return run >= 16u ? 0xFFFFu : (1u << run) - 1u; }

// SWAR byte tests over 8 bytes: 0x80 in every byte of the result for which the test holds, exactly (no carry crosses a byte).
static constexpr uint64_t kOnes = 0x0101010101010101ull, kLow7 = 0x7F7F7F7F7F7F7F7Full, kHigh = 0x8080808080808080ull;
PWAF_SVC_HD uint64_t zero_bytes(uint64_t v) { return ~(((v & kLow7) + kLow7) | v | kLow7); }
PWAF_SVC_HD uint64_t eq_bytes(uint64_t v, uint8_t c) { return zero_bytes(v ^ (kOnes * c)); }
// the 0x80 bits of 8 bytes -> 8 bits, byte k -> bit k (the products' bits are all distinct: nothing carries)
PWAF_SVC_HD uint32_t gather_bits(uint64_t m) { return (uint32_t)(((m & kHigh) >> 7) * 0x0102040810204080ull >> 56); }

enum ByteClass : uint32_t {
    kSlash,     // '/'
    kBlank,     // str::trim on a value that passed to_str: ' ' and TAB are the only whitespace it can hold
    kSpace,     // str::trim on uri.host(): char::is_whitespace below 0x80 is 0x09..0x0D and 0x20
    kNotText,   // HeaderValue::to_str refuses it: neither TAB nor 0x20..0x7E
};
PWAF_SVC_HD uint64_t class_bytes(uint64_t v, uint32_t cls) {
    const uint64_t blank = eq_bytes(v, 0x20) | eq_bytes(v, 0x09);
    if (cls == kSlash) return eq_bytes(v, '/');
    if (cls == kBlank) return blank;
    if (cls == kSpace) return blank | eq_bytes(v, 0x0A) | eq_bytes(v, 0x0B) | eq_bytes(v, 0x0C) | eq_bytes(v, 0x0D);
    // below 0x20 (the top three bits clear) and not TAB; or 0x7F; or 0x80 and above
    return (zero_bytes(v & (kOnes * 0xE0u)) & ~eq_bytes(v, 0x09)) | eq_bytes(v, 0x7F) | (v & kHigh);
}
// bit k: byte k of the chunk is of the class
PWAF_SVC_HD uint32_t class_bits(const Chunk &v, uint32_t cls) { return gather_bits(class_bytes(v.lo, cls)) | gather_bits(class_bytes(v.hi, cls)) << 8; }

PWAF_SVC_HD uint32_t lowest_bit(uint32_t x) { return (uint32_t)__builtin_ctz(x); }   // x != 0
PWAF_SVC_HD uint32_t highest_bit(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }  // x != 0

// ---- the kept slice of one value -----------------------------------------------------------------------------------------------------
struct Span {
    uint32_t start, len;  // bytes [start, start + len) of the raw value; start is 0 when len is
};
// [b, e) of s without the bytes of class `cls` at its end / at its beginning
PWAF_SVC_HD uint32_t trim_end(const uint8_t *s, uint32_t b, uint32_t e, uint32_t cls) {
    while (e > b) {
        const uint32_t at = e - b >= 16u ? e - 16u : b, run = e - at;  // (never a byte in front of b)
        const uint32_t other = ~class_bits(load16(s + at, run), cls) & run_bits(run);
        if (other) return at + highest_bit(other) + 1u;
        e = at;
    }
    return e;
}
PWAF_SVC_HD uint32_t trim_begin(const uint8_t *s, uint32_t b, uint32_t e, uint32_t cls) {
    while (b < e) {
        const uint32_t run = e - b >= 16u ? 16u : e - b;
        const uint32_t other = ~class_bits(load16(s + b, run), cls) & run_bits(run);
        if (other) return b + lowest_bit(other);
        b += run;
    }
    return b;
}
PWAF_SVC_HD bool any_of(const uint8_t *s, uint32_t b, uint32_t e, uint32_t cls) {
    for (; b < e; b += 16u) {
        const uint32_t run = e - b >= 16u ? 16u : e - b;
        if (class_bits(load16(s + b, run), cls) & run_bits(run)) return true;
    }
    return false;
}
PWAF_SVC_HD Span path_span(const uint8_t *s, uint32_t len) { return Span{0, trim_end(s, 0, len, kSlash)}; }
// A header value (Host, User-Agent): "" when a byte is not text, else trimmed of ' ' and TAB, "" when more than 256 bytes remain. A byte
// that is not text ends both runs, so it is among the kept bytes, and a value with more than 256 of those is "" whatever they are.
PWAF_SVC_HD Span header_span(const uint8_t *s, uint32_t len) {
    const uint32_t b = trim_begin(s, 0, len, kBlank), e = trim_end(s, b, len, kBlank);
    if (e == b || e - b > kMaxKept || any_of(s, b, e, kNotText)) return Span{0, 0};
    return Span{b, e - b};
}
// uri.host(): trimmed of whitespace, "" when more than 256 bytes remain; no byte check (it is a &str already)
PWAF_SVC_HD Span uri_host_span(const uint8_t *s, uint32_t len) {
    const uint32_t b = trim_begin(s, 0, len, kSpace), e = trim_end(s, b, len, kSpace);
    if (e == b || e - b > kMaxKept) return Span{0, 0};
    return Span{b, e - b};
}

// ---- the batch -------------------------------------------------------------------------------------------------------------------------
// The kernels' arguments, the phases' below and derive_host's (pwaf_derive_batch after its argument checks).
struct Args {
    pwaf_strcol raw[kColumns];  // the Host header's value, uri.path(), the User-Agent header's value
    pwaf_strcol uri_host;       // offsets NULL: no request has one
    const uint8_t *present;     // n x PWAF_RAW_HAS_*; NULL: kDefaultPresent for every request
    uint32_t n;
    uint32_t tile_stride;       // DEVICE / phases: entries per column of `tile` (scratch_layout)
    uint8_t *data[kColumns];
    uint32_t *off[kColumns];
    uint64_t cap[kColumns];
    pwaf_derive_stats *stats;
    uint64_t *tile;             // scratch: [column][tile_stride] tile sums, then exclusive bases; slot n_tiles: the column's total
    uint32_t *from;             // scratch: [2][n] where the kept bytes of the host (row 0) and the User-Agent (row 1) begin in their source arena
};
static constexpr uint32_t kDefaultPresent = PWAF_RAW_HAS_HOST_HEADER | PWAF_RAW_HAS_USER_AGENT;

PWAF_SVC_HD uint32_t present_of(const Args &a, uint32_t i) {
    uint32_t p = a.present ? a.present[i] : kDefaultPresent;
    if (!a.uri_host.offsets) p &= ~PWAF_RAW_HAS_URI_HOST;
    return p;
}
// which column the host of a request with these present bits is cut from: the URI's host wins, even when it derives to ""
PWAF_SVC_HD const pwaf_strcol &host_source(const Args &a, uint32_t present) { return (present & PWAF_RAW_HAS_URI_HOST) ? a.uri_host : a.raw[kHost]; }

// Where the derived value of column c of request i lies: its first byte's position in the source arena, and its length. Lengths in
// uint32 arithmetic, as every reader of the offsets computes them. The bytes of a value whose present bit is clear are not read.
struct Kept {
    uint32_t at, len;
};
PWAF_SVC_HD Kept kept_of(const Args &a, uint32_t c, uint32_t i, uint32_t present) {
    if (c == kPath) {
        const uint32_t o = a.raw[kPath].offsets[i];
        return Kept{o, path_span(a.raw[kPath].data + o, a.raw[kPath].offsets[i + 1] - o).len};
    }
    const bool uri = c == kHost && (present & PWAF_RAW_HAS_URI_HOST);
    if (!uri && !(present & (c == kHost ? PWAF_RAW_HAS_HOST_HEADER : PWAF_RAW_HAS_USER_AGENT))) return Kept{0, 0};
    const pwaf_strcol &col = uri ? a.uri_host : a.raw[c];
    const uint32_t o = col.offsets[i], len = col.offsets[i + 1] - o;
    const Span s = uri ? uri_host_span(col.data + o, len) : header_span(col.data + o, len);
    return Kept{o + s.start, s.len};
}
// the arena the kept bytes of column c are copied from
PWAF_SVC_HD const uint8_t *source_of(const Args &a, uint32_t c, uint32_t present) { return c == kHost ? host_source(a, present).data : a.raw[c].data; }

// ---- the scan's arithmetic ---------------------------------------------------------------------------------------------------------------
PWAF_SVC_HD uint32_t tiles(uint32_t n) { return pwaf::tiles(n, kTile); }
// scratch: the tile array (kColumns x stride 64-bit words, stride = tiles + 1 rounded up to even), then `from` (2 x n words)
PWAF_SVC_HD uint32_t tile_stride(uint32_t n) { return pwaf::tile_stride(tiles(n)); }
PWAF_SVC_HD size_t scratch_bytes(uint32_t n) { return ((size_t)kColumns * tile_stride(n) * 8u + (size_t)2u * n * 4u + 15u) & ~(size_t)15u; }
inline void scratch_layout(Args &a, void *scratch) {
    a.tile_stride = tile_stride(a.n);
    a.tile = (uint64_t *)scratch;
    a.from = (uint32_t *)(a.tile + (size_t)kColumns * a.tile_stride);
}
PWAF_SVC_HD void fill_stats(pwaf_derive_stats *st, const uint64_t total[kColumns], const uint64_t cap[kColumns], uint32_t n) {
    uint32_t overflow = 0;
    for (uint32_t c = 0; c < kColumns; c++) {
        st->bytes[c] = total[c];
        if (!fits(total[c], cap[c])) overflow |= 1u << c;
    }
    st->n = n;
    st->overflow = overflow;
}

// ---- the three phases as plain loops (tests/derive_host.cpp): what the kernels compute, a tile at a time, in any order of tiles ----------
// Phase 1, tile t: every kept length one slot up in the offsets, `from`, and the tile's sums.
inline void span_tile(const Args &a, uint32_t t) {
    uint64_t sum[kColumns] = {0, 0, 0};
    const uint64_t end = (uint64_t)t * kTile + kTile < a.n ? (uint64_t)t * kTile + kTile : a.n;
    for (uint32_t i = t * kTile; i < end; i++) {
        const uint32_t p = present_of(a, i);
        for (uint32_t c = 0; c < kColumns; c++) {
            const Kept k = kept_of(a, c, i, p);
            a.off[c][i + 1] = k.len;
            sum[c] += k.len;
            if (c != kPath) a.from[(size_t)(c == kUserAgent) * a.n + i] = k.at;
        }
    }
    for (uint32_t c = 0; c < kColumns; c++) a.tile[(size_t)c * a.tile_stride + t] = sum[c];
}
// Phase 2, column c: sums -> exclusive bases; slot n_tiles: the total.
inline void base_column(const Args &a, uint32_t c) {
    uint64_t *const tile = a.tile + (size_t)c * a.tile_stride, run = 0;
    const uint32_t nt = tiles(a.n);
    for (uint32_t t = 0; t < nt; t++) {
        const uint64_t x = tile[t];
        tile[t] = run;
        run += x;
    }
    tile[nt] = run;
}
// Phase 3, tile t (tile 0 also when n == 0): offsets in place, the kept bytes, and by the tiles that own them offsets[0], the pad, stats.
inline void copy_tile(const Args &a, uint32_t t) {
    const uint32_t nt = tiles(a.n);
    const uint64_t end = (uint64_t)t * kTile + kTile < a.n ? (uint64_t)t * kTile + kTile : a.n;
    for (uint32_t c = 0; c < kColumns; c++) {
        const uint64_t total = a.tile[(size_t)c * a.tile_stride + nt];
        uint64_t at = a.tile[(size_t)c * a.tile_stride + t];
        if (t == 0 && a.off[c]) a.off[c][0] = 0;  // (n == 0: the offsets may be NULL)
        for (uint32_t i = t * kTile; i < end; i++) {
            const uint32_t len = a.off[c][i + 1], p = present_of(a, i);
            const uint32_t from = c == kPath ? a.raw[kPath].offsets[i] : a.from[(size_t)(c == kUserAgent) * a.n + i];
            append_clipped(a.data[c], a.cap[c], at, source_of(a, c, p) + from, len);
            at += len;
            a.off[c][i + 1] = (uint32_t)at;
        }
        if (t + 1 >= nt)
            for (uint32_t k = 0; k < PWAF_ARENA_PAD; k++) write_pad_byte(a.data[c], total, a.cap[c], k);
    }
    if (t == 0) {
        uint64_t total[kColumns];
        for (uint32_t c = 0; c < kColumns; c++) total[c] = a.tile[(size_t)c * a.tile_stride + nt];
        fill_stats(a.stats, total, a.cap, a.n);
    }
}

// ---- the HOST mode -----------------------------------------------------------------------------------------------------------------------
// First every request is checked (offsets that decrease in a column it reads: false with the request and the column — 0 host, 1 path,
// 2 User-Agent, 3 the URI's host — and nothing written), then the columns are written in request order. Needs no scratch.
inline bool derive_host(const Args &a, uint32_t *bad_request, uint32_t *bad_column) {
    for (uint32_t i = 0; i < a.n; i++) {
        const uint32_t p = present_of(a, i);
        const bool uri = p & PWAF_RAW_HAS_URI_HOST;
        const bool reads[4] = {!uri && (p & PWAF_RAW_HAS_HOST_HEADER), true, (p & PWAF_RAW_HAS_USER_AGENT) != 0, uri};
        for (uint32_t c = 0; c < 4; c++) {
            const pwaf_strcol &col = c == 3 ? a.uri_host : a.raw[c];
            if (reads[c] && col.offsets[i + 1] < col.offsets[i]) {
                *bad_request = i, *bad_column = c;
                return false;
            }
        }
    }
    uint64_t at[kColumns] = {0, 0, 0};
    for (uint32_t c = 0; c < kColumns; c++)
        if (a.off[c]) a.off[c][0] = 0;  // (n == 0: the offsets may be NULL)
    for (uint32_t i = 0; i < a.n; i++) {
        const uint32_t p = present_of(a, i);
        for (uint32_t c = 0; c < kColumns; c++) {
            const Kept k = kept_of(a, c, i, p);
            append_clipped(a.data[c], a.cap[c], at[c], source_of(a, c, p) + k.at, k.len);
            at[c] += k.len;
            a.off[c][i + 1] = (uint32_t)at[c];
        }
    }
    for (uint32_t c = 0; c < kColumns; c++)
        for (uint32_t k = 0; k < PWAF_ARENA_PAD; k++) write_pad_byte(a.data[c], at[c], a.cap[c], k);
    fill_stats(a.stats, at, a.cap, a.n);
    return true;
}

int launch_derive(int phase, const Args &a, void *stream);  // derive.hip: 1 span, 2 base, 3 copy

}  // namespace derive
}  // namespace pwaf
