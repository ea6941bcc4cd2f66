// powbody.h — the body of a captcha proof-of-work submission (include/pwaf.h: pwaf_parse_pow_bodies, pwaf_parse_pow_body_one): what
// serde_json::from_reader hands CaptchaManager::api_verify as CaptchaVerifyRequestBody {hash: [u8; 32] (hex), nonce: String}
// (pingoo/captcha.rs:50-57, :291), read in a strict subset. DESIGN.md §5.1.8 states the decisions D-B1 to D-B10 this file follows.
//
// One header, compiled three ways, like derive.h and pow.h: by powbody.hip for the device (powbody_parse_kernel, powbody_base_kernel,
// powbody_copy_kernel), by the same unit for the HOST mode and pwaf_parse_pow_body_one (parse_host and read_body below) and by
// tools/powbody_host.cpp (g++ under the sanitizers). No HIP include.
//
// The reader is ONE function, read_body, templated on where its bytes come from: Padded reads 16 bytes at a time at the body's own
// alignment and may pass the body's end by fewer than 16 bytes (the arena or its PWAF_ARENA_PAD), Exact reads the body's bytes and no
// other (a host column has no pad). It looks at every byte once, left to right, through a cursor that holds the sixteen bytes around the
// position in two registers: a genuine body of 90 bytes is six loads. Its whole state is scalars — position, the chunk, the flags of the
// string being read, eight hash words written with a static index — so nothing of it lives in scratch memory.
//
// The batch is reduce-then-scan over tiles of kTile requests, the scheme of derive.h for one column: phase 1 parses and stores every nonce
// length one slot up in nonce->offsets (and where the nonce begins in the body arena, scratch `from`), phase 2 makes exclusive bases of the
// tiles' sums, phase 3 rescans each tile in place and copies the nonces. With a list the lengths of unselected requests are zeroed by one
// memset in front of phase 1, and phase 2 sums the tiles' lengths itself (a list may name a request twice, so the entries' sums are not
// the requests').
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "pwaf.h"
#include "service.h"

namespace pwaf {
namespace powbody {

static constexpr uint32_t kTile = 256;         // entries per workgroup of the parse launch; requests per tile of the scan
static constexpr uint32_t kStep = 1024;        // lanes of the base launch: tiles per step
static constexpr uint32_t kCopyGroup = kTile;  // requests per workgroup of the copy launch (it reads ONE base)
static constexpr uint32_t kMinGroups = 64;     // with a list the parse launch has at most max(tiles(n), kMinGroups) workgroups
static constexpr uint32_t kMaxRequests = 0xFFFFFFF0u / PWAF_POW_BODY_MAX_BYTES;  // the nonce column stays below 32 bits
static_assert(sizeof(pwaf_body_stats) == 32, "pwaf_body_stats layout");

// ---- where the bytes come from -----------------------------------------------------------------------------------------------------------
struct Chunk {
    uint64_t lo, hi;  // byte k of the chunk in bits [8k, 8k + 8) of lo (k < 8) / of hi
};
struct Padded {  // DEVICE: one 16-byte load at the body's own alignment; it may pass the body's end by up to 15 bytes
    const uint8_t *s;
    PWAF_SVC_HD Chunk load(uint32_t at, uint32_t run) const {
        (void)run;
        Chunk v;
        memcpy(&v, s + at, 16);
        return v;
    }
};
struct Exact {  // HOST: not a byte outside the body
    const uint8_t *s;
    PWAF_SVC_HD Chunk load(uint32_t at, uint32_t run) const {
        Chunk v{0, 0};
        memcpy(&v, s + at, run);
        return v;
    }
};
// the sixteen bytes [at, at + 16) of the body that hold the position asked for last; at is a multiple of 16, so no load begins before the
// body and a body of L bytes costs ceil(L / 16) loads when it is read left to right
template <class Src>
struct Cursor {
    Src src;
    uint32_t len, at;
    uint64_t lo, hi;
    PWAF_SVC_HD uint32_t byte(uint32_t p) {  // p < len
        if ((p & ~15u) != at) {
            at = p & ~15u;
            const Chunk c = src.load(at, len - at >= 16u ? 16u : len - at);
            lo = c.lo, hi = c.hi;
        }
        return (uint32_t)(((p & 8u) ? hi : lo) >> (8u * (p & 7u))) & 0xFFu;
    }
};

// ---- the reader ----------------------------------------------------------------------------------------------------------------------------
struct Body {
    uint32_t status;    // PWAF_BODY_OK / _MALFORMED / _UNDECIDED
    uint32_t nonce_at;  // OK: the nonce is body[nonce_at, nonce_at + nonce_len); else 0, 0
    uint32_t nonce_len;
    uint32_t hash[8];   // OK: the 32 bytes, byte k in bits [8(k & 3), +8) of word k / 4 (memory order on a little-endian machine); else 0
};
PWAF_SVC_HD bool is_ws(uint32_t b) { return b == 0x20u || b == 0x09u || b == 0x0Au || b == 0x0Du; }
// 0..15, or 16 for a byte that is no hexadecimal digit
PWAF_SVC_HD uint32_t hex_value(uint32_t b) {
    const uint32_t d = b - '0', l = (b | 0x20u) - 'a';
    return d < 10u ? d : l < 6u ? l + 10u : 16u;
}
// A string, its opening '"' at p - 1 (D-B4): where its closing '"' is and what lies in front of it.
struct Text {
    uint32_t end;    // the closing '"'; len: there is none
    uint32_t flags;  // kCtl / kEscape / kHigh / kNotHex
    uint64_t head;   // its first 8 bytes, byte k in bits [8k, +8)
    uint32_t word[8];  // its first 64 bytes taken as hexadecimal digits, two a byte, high nibble first (Body::hash's layout)
};
enum : uint32_t { kCtl = 1u, kEscape = 2u, kHigh = 4u, kNotHex = 8u };
static constexpr uint64_t kKeyHash = 0x68736168ull;     // "hash"
static constexpr uint64_t kKeyNonce = 0x65636E6F6Eull;  // "nonce"
template <class Src>
PWAF_SVC_HD Text read_text(Cursor<Src> &c, uint32_t p) {
    Text t{c.len, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0}};
    uint32_t acc = 0;
    for (uint32_t k = 0; p < c.len; p++, k++) {
        const uint32_t b = c.byte(p);
        if (b == '"') {
            t.end = p;
            break;
        }
        t.flags |= (b < 0x20u ? kCtl : 0u) | (b == '\\' ? kEscape : 0u) | (b >= 0x80u ? kHigh : 0u);
        if (k < 8u) t.head |= (uint64_t)b << (8u * k);
        // the value of `hash`: two digits a byte, high nibble first; word k / 8 is complete behind digit k % 8 == 7
        const uint32_t h = hex_value(b);
        if (h > 15u) t.flags |= kNotHex;
        acc = (acc << 4) | (h & 15u);
        if ((k & 7u) == 7u && k < 64u) {
            const uint32_t w = __builtin_bswap32(acc);
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) t.word[j] = (k >> 3) == j ? w : t.word[j];  // (a static index: the words stay in registers)
        }
    }
    return t;
}
// D-B1 to D-B10. The FIRST deciding event wins.
template <class Src>
PWAF_SVC_HD Body read_body(const Src &src, uint32_t len) {
    Body r{PWAF_BODY_MALFORMED, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0}};
    const Body malformed = r;
    Body undecided = r;
    undecided.status = PWAF_BODY_UNDECIDED;
    if (len > PWAF_POW_BODY_MAX_BYTES) return undecided;  // D-B1: nothing of it is read
    Cursor<Src> c{src, len, ~0u, 0, 0};
    uint32_t p = 0;
#define PWAF_PB_SKIP_WS()                 \
    while (p < len && is_ws(c.byte(p))) p++; \
    if (p == len) return malformed
    PWAF_PB_SKIP_WS();  // D-B2
    {
        const uint32_t b = c.byte(p++);
        if (b == '[') return undecided;
        if (b != '{') return malformed;
    }
    uint32_t seen = 0;  // bit 0: hash, bit 1: nonce
    for (;;) {
        PWAF_PB_SKIP_WS();  // D-B3
        if (c.byte(p++) != '"') return malformed;
        const Text key = read_text(c, p);  // D-B4
        if (key.end == len || (key.flags & kCtl)) return malformed;
        if (key.flags & kEscape) return undecided;
        const uint32_t key_len = key.end - p;  // D-B5 (a byte >= 0x80 makes the key another one: UNDECIDED either way)
        const uint32_t which = key_len == 4u && key.head == kKeyHash ? 1u : key_len == 5u && key.head == kKeyNonce ? 2u : 0u;
        if (!which) return undecided;
        if (seen & which) return malformed;
        seen |= which;
        p = key.end + 1u;
        PWAF_PB_SKIP_WS();
        if (c.byte(p++) != ':') return malformed;
        PWAF_PB_SKIP_WS();
        if (c.byte(p++) != '"') return malformed;  // D-B6
        const Text val = read_text(c, p);  // D-B4
        if (val.end == len || (val.flags & kCtl)) return malformed;
        if (val.flags & kEscape) return undecided;
        if (which == 1u) {
            if (val.end - p != 64u || (val.flags & kNotHex)) return malformed;  // D-B7
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) r.hash[j] = val.word[j];
        } else {
            if (val.flags & kHigh) return undecided;  // D-B8
            r.nonce_at = p, r.nonce_len = val.end - p;
        }
        p = val.end + 1u;
        PWAF_PB_SKIP_WS();
        const uint32_t b = c.byte(p++);
        if (b == '}') break;
        if (b != ',') return malformed;
    }
    if (seen != 3u) return malformed;  // D-B9
    while (p < len && is_ws(c.byte(p))) p++;
    if (p != len) return malformed;
#undef PWAF_PB_SKIP_WS
    r.status = PWAF_BODY_OK;  // D-B10
    return r;
}

// ---- the batch ---------------------------------------------------------------------------------------------------------------------------
// The kernels' arguments and parse_host's (pwaf_parse_pow_bodies after its argument checks).
struct Args {
    pwaf_strcol bodies;
    uint32_t n;
    const uint32_t *idx;    // NULL: every request, status[i] belongs to request i
    const uint32_t *n_idx;  // nullable: min(*n_idx, idx_cap) entries are looked at
    uint32_t idx_cap;
    uint8_t *status;
    uint8_t *hash;  // n x 32, by request
    uint8_t *data;  // the nonce column
    uint32_t *off;
    uint64_t cap;
    pwaf_body_stats *stats;
    uint32_t groups;  // DEVICE: workgroups of the parse launch (0: it is not made), each with one slot of `count`
    uint64_t *tile;   // scratch: tile sums, then exclusive bases; slot tiles(n): the column's total
    uint32_t *count;  // scratch: [groups][4] OK / MALFORMED / UNDECIDED / entries of each parse workgroup
    uint32_t *from;   // scratch: [n] where the nonce of a request begins in the body arena
};
PWAF_SVC_HD uint32_t selected(const Args &a) { return pwaf::selected(a.idx, a.n_idx, a.idx_cap, a.n); }
PWAF_SVC_HD uint32_t request_of(const Args &a, uint32_t e) { return pwaf::request_of(a.idx, e); }
// Entry e, of request i < n: the status, and where selected by request the hash row, the nonce's length one slot up and its start.
template <class Src>
PWAF_SVC_HD Body parse_entry(const Args &a, uint32_t e, uint32_t i) {
    const uint32_t o = a.bodies.offsets[i];
    const Body b = read_body(Src{a.bodies.data + o}, a.bodies.offsets[i + 1] - o);
    a.status[e] = (uint8_t)b.status;
    memcpy(a.hash + (size_t)i * 32u, b.hash, 32);
    a.off[(size_t)i + 1] = b.nonce_len;
    return b;
}

// ---- the scan's arithmetic -----------------------------------------------------------------------------------------------------------------
PWAF_SVC_HD uint32_t tiles(uint32_t n) { return pwaf::tiles(n, kTile); }
// the parse launch: one workgroup per tile of entries; with a list a bounded number of them, each striding over the tiles
PWAF_SVC_HD uint32_t parse_groups(uint32_t n, bool list, uint32_t idx_cap) {
    if (!list) return tiles(n);
    const uint32_t most = tiles(n) > kMinGroups ? tiles(n) : kMinGroups;
    return tiles(idx_cap) < most ? tiles(idx_cap) : most;
}
// scratch: the tile array (tiles + 1 64-bit words, rounded up to even), the count slots (16 bytes each), `from` (n words)
PWAF_SVC_HD uint32_t tile_stride(uint32_t n) { return pwaf::tile_stride(tiles(n)); }
PWAF_SVC_HD uint32_t count_slots(uint32_t n) { return tiles(n) > kMinGroups ? tiles(n) : kMinGroups; }
PWAF_SVC_HD size_t scratch_bytes(uint32_t n) { return ((size_t)tile_stride(n) * 8u + (size_t)count_slots(n) * 16u + (size_t)n * 4u + 15u) & ~(size_t)15u; }
inline void scratch_layout(Args &a, void *scratch) {
    a.tile = (uint64_t *)scratch;
    a.count = (uint32_t *)(a.tile + tile_stride(a.n));
    a.from = a.count + (size_t)count_slots(a.n) * 4u;
}
PWAF_SVC_HD void fill_stats(pwaf_body_stats *st, uint64_t total, uint64_t cap, const uint32_t count[4]) {
    st->nonce_bytes = total;
    st->n = count[3], st->n_ok = count[0], st->n_malformed = count[1], st->n_undecided = count[2];
    st->overflow = fits(total, cap) ? 0u : 1u;
    st->reserved = 0;
}

// ---- the HOST mode -------------------------------------------------------------------------------------------------------------------------
// First every selected request is checked (body offsets that decrease: false with *bad = the entry, nothing written), then statuses, hash
// rows and lengths are written in entry order and the nonces copied in request order. `from` is the caller's: n words (NULL when n == 0).
inline bool parse_host(const Args &a, uint32_t *from, uint32_t *bad) {
    const uint32_t m = selected(a);
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t i = request_of(a, j);
        if (i < a.n && a.bodies.offsets[i + 1] < a.bodies.offsets[i]) {
            *bad = j;
            return false;
        }
    }
    for (uint32_t i = 0; i < a.n; i++) a.off[(size_t)i + 1] = 0;
    uint32_t count[4] = {0, 0, 0, m};
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t i = request_of(a, j);
        if (i >= a.n) {
            a.status[j] = PWAF_BODY_NONE;
            continue;
        }
        const Body b = parse_entry<Exact>(a, j, i);
        from[i] = a.bodies.offsets[i] + b.nonce_at;
        count[b.status - 1u]++;
    }
    uint64_t at = 0;
    if (a.off) a.off[0] = 0;  // (n == 0: the offsets may be NULL)
    for (uint32_t i = 0; i < a.n; i++) {
        const uint32_t len = a.off[(size_t)i + 1];
        if (len) append_clipped(a.data, a.cap, at, a.bodies.data + from[i], len);  // (from[i] is written only for a request the list names)
        at += len;
        a.off[(size_t)i + 1] = (uint32_t)at;
    }
    for (uint32_t k = 0; k < PWAF_ARENA_PAD; k++) write_pad_byte(a.data, at, a.cap, k);
    fill_stats(a.stats, at, a.cap, count);
    return true;
}

int launch_parse_pow(const Args &a, void *stream);  // powbody.hip: the memset (with a list) and the three launches

}  // namespace powbody
}  // namespace pwaf
