// clientid.h — the captcha client id of a request (include/pwaf.h: pwaf_client_ids, pwaf_client_id_one): the reference's
// generate_captcha_client_id (pingoo/captcha.rs:409-421), base64url_nopad(SHA-256(ip octets || user_agent || host)), 43 characters.
//
// One header, compiled three ways, like confirm.h and records.h: by clientid.hip for the device (client_id_kernel: one request per lane),
// by the same unit for the host (the HOST mode of pwaf_client_ids and pwaf_client_id_one: ids_host / client_id_words below) and by
// tests/client_id_host.cpp (g++ under the sanitizers). No HIP include: compiled as plain C++ it needs <stdint.h> and <string.h> only.
//
// The message is never assembled in memory. It is three runs of bytes (ip, User-Agent, host), each at any source address, and a SHA-256
// block is four 16-byte chunks: a chunk takes ONE load per run it crosses, cut to the run's length and shifted to its place (the way
// pack_records_kernel gathers a chunk). The only difference between the compilations is that load (load_run): the device reads 16 bytes
// and masks, which may run past the value by fewer than 16 bytes (inside the arena or its PWAF_ARENA_PAD); the host reads exactly the
// bytes of the value.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "pwaf.h"
#include "service.h"

namespace pwaf {
namespace clientid {

typedef unsigned __int128 chunk_t;  // 16 message bytes, byte k of the chunk in bits [8k, 8k + 8)

static constexpr uint32_t kIdWords = 11;  // sizeof(pwaf_client_id) / 4: 43 characters and the NUL
static_assert(sizeof(pwaf_client_id) == 4 * kIdWords, "pwaf_client_id layout");

// ---- SHA-256 (FIPS 180-4) ---------------------------------------------------------------------------------------------------------
PWAF_SVC_HD uint32_t rotr(uint32_t x, uint32_t n) {
#if defined(__has_builtin)
#if __has_builtin(__builtin_rotateright32)
    return __builtin_rotateright32(x, n);  // v_alignbit_b32
#else
    return (x >> n) | (x << (32u - n));
#endif
#else
    return (x >> n) | (x << (32u - n));
#endif
}
// both in the bit-select shape "z ^ (x & (y ^ z))", which the compiler turns into ONE instruction (v_bfi_b32; on gfx950 v_bitop3_b32):
// Ch = e ? f : g bitwise, Maj = (a ^ b) ? c : b bitwise
PWAF_SVC_HD uint32_t ch(uint32_t e, uint32_t f, uint32_t g) { return g ^ (e & (f ^ g)); }
PWAF_SVC_HD uint32_t maj(uint32_t a, uint32_t b, uint32_t c) { return b ^ ((a ^ b) & (c ^ b)); }
// a ^ b ^ c: one v_bitop3_b32 (truth table 0x96) on gfx950, which the compiler does not form from two xors by itself
PWAF_SVC_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}
PWAF_SVC_HD uint32_t big0(uint32_t x) { return xor3(rotr(x, 2), rotr(x, 13), rotr(x, 22)); }
PWAF_SVC_HD uint32_t big1(uint32_t x) { return xor3(rotr(x, 6), rotr(x, 11), rotr(x, 25)); }
PWAF_SVC_HD uint32_t small0(uint32_t x) { return xor3(rotr(x, 7), rotr(x, 18), x >> 3); }
PWAF_SVC_HD uint32_t small1(uint32_t x) { return xor3(rotr(x, 17), rotr(x, 19), x >> 10); }

// One round with the state's roles rotated by the caller and every index a literal: the schedule is a rolling window of 16 words that
// stays in registers (a w[] indexed at run time would live in scratch).
#define PWAF_SHA_ROUND(a, b, c, d, e, f, g, h, t, k)                                                                     \
    {                                                                                                                    \
        if ((t) >= 16) w[(t) & 15] += small1(w[((t) - 2) & 15]) + w[((t) - 7) & 15] + small0(w[((t) - 15) & 15]);         \
        const uint32_t t1 = h + big1(e) + ch(e, f, g) + (k) + w[(t) & 15];                                               \
        d += t1;                                                                                                         \
        h = t1 + big0(a) + maj(a, b, c);                                                                                 \
    }
#define PWAF_SHA_ROUNDS8(t, k0, k1, k2, k3, k4, k5, k6, k7)  \
    PWAF_SHA_ROUND(a, b, c, d, e, f, g, h, (t) + 0, k0)      \
    PWAF_SHA_ROUND(h, a, b, c, d, e, f, g, (t) + 1, k1)      \
    PWAF_SHA_ROUND(g, h, a, b, c, d, e, f, (t) + 2, k2)      \
    PWAF_SHA_ROUND(f, g, h, a, b, c, d, e, (t) + 3, k3)      \
    PWAF_SHA_ROUND(e, f, g, h, a, b, c, d, (t) + 4, k4)      \
    PWAF_SHA_ROUND(d, e, f, g, h, a, b, c, (t) + 5, k5)      \
    PWAF_SHA_ROUND(c, d, e, f, g, h, a, b, (t) + 6, k6)      \
    PWAF_SHA_ROUND(b, c, d, e, f, g, h, a, (t) + 7, k7)

// state += compress(state, w); w[] (the block's 16 big-endian words) is used up
PWAF_SVC_HD void compress(uint32_t state[8], uint32_t w[16]) {
    uint32_t a = state[0], b = state[1], c = state[2], d = state[3], e = state[4], f = state[5], g = state[6], h = state[7];
    PWAF_SHA_ROUNDS8(0, 0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u)
    PWAF_SHA_ROUNDS8(8, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u)
    PWAF_SHA_ROUNDS8(16, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau)
    PWAF_SHA_ROUNDS8(24, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u)
    PWAF_SHA_ROUNDS8(32, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u)
    PWAF_SHA_ROUNDS8(40, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u)
    PWAF_SHA_ROUNDS8(48, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u)
    PWAF_SHA_ROUNDS8(56, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u)
    state[0] += a, state[1] += b, state[2] += c, state[3] += d, state[4] += e, state[5] += f, state[6] += g, state[7] += h;
}
#undef PWAF_SHA_ROUNDS8
#undef PWAF_SHA_ROUND

// ---- the message: three runs -------------------------------------------------------------------------------------------------------
struct Message {
    const uint8_t *ip, *ua, *host;  // a run of length 0 is never dereferenced (its pointer may be NULL)
    uint32_t ip_len, ua_len, host_len;
    PWAF_SVC_HD uint64_t bytes() const { return (uint64_t)ip_len + ua_len + host_len; }
    PWAF_SVC_HD uint64_t blocks() const { return (bytes() + 9u + 63u) >> 6; }  // the 0x80 byte and the 8-byte length ride in the last one
};
PWAF_SVC_HD Message make_message(const uint8_t *ip16, uint8_t ip_is_v6, const uint8_t *ua, uint32_t ua_len, const uint8_t *host, uint32_t host_len) {
    return Message{ip16, ua, host, ip_is_v6 ? 16u : 4u, ua_len, host_len};
}

// The low `run` (1..16) bytes at s, the rest 0.
PWAF_SVC_HD chunk_t load_run(const uint8_t *s, uint32_t run) {
    chunk_t v = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    memcpy(&v, s, 16);  // one 16-byte load at the run's own alignment; it may pass the value's end by up to 15 bytes
    if (run < 16u) v &= ((chunk_t)1 << (8u * run)) - 1u;
#else
    memcpy(&v, s, run);  // not a byte outside the value: a host column has no pad
#endif
    return v;
}
// what the run [start, start + len) of the message puts into the chunk [p0, p0 + 16)
PWAF_SVC_HD chunk_t run_part(uint64_t p0, const uint8_t *s, uint64_t start, uint32_t len) {
    const uint64_t end = start + len, lo = p0 > start ? p0 : start, hi = p0 + 16u < end ? p0 + 16u : end;
    if (lo >= hi) return 0;
    return load_run(s + (lo - start), (uint32_t)(hi - lo)) << (8u * (uint32_t)(lo - p0));
}
// block b (< m.blocks()) of the padded message as 16 big-endian words
PWAF_SVC_HD void load_block(const Message &m, uint64_t b, uint32_t w[16]) {
    const uint64_t total = m.bytes();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t c = 0; c < 4; c++) {
        const uint64_t p0 = 64u * b + 16u * c;
        chunk_t acc = 0;
        if (p0 < total) {
            acc = run_part(p0, m.ip, 0, m.ip_len);
            acc |= run_part(p0, m.ua, m.ip_len, m.ua_len);
            acc |= run_part(p0, m.host, (uint64_t)m.ip_len + m.ua_len, m.host_len);
        }
        if (total >= p0 && total < p0 + 16u) acc |= (chunk_t)0x80u << (8u * (uint32_t)(total - p0));
        for (uint32_t k = 0; k < 4; k++) w[4 * c + k] = __builtin_bswap32((uint32_t)(acc >> (32u * k)));
    }
    if (b + 1 == m.blocks()) {
        const uint64_t bits = total * 8u;  // (three 32-bit lengths: below 2^37)
        w[14] = (uint32_t)(bits >> 32);
        w[15] = (uint32_t)bits;
    }
}

// ---- base64url without padding (captcha.rs:420) -------------------------------------------------------------------------------------
// 0..25 'A'.., 26..51 'a'.., 52..61 '0'.., 62 '-', 63 '_': branch-free
PWAF_SVC_HD uint32_t b64_char(uint32_t v) { return v + 65u + (v >= 26u ? 6u : 0u) - (v >= 52u ? 75u : 0u) - (v >= 62u ? 13u : 0u) + (v >= 63u ? 49u : 0u); }
// 24 bits -> four characters, the first in the low byte (memory order)
PWAF_SVC_HD uint32_t b64_quad(uint32_t v) { return b64_char(v >> 18) | b64_char((v >> 12) & 63u) << 8 | b64_char((v >> 6) & 63u) << 16 | b64_char(v & 63u) << 24; }
// the digest (8 big-endian words) -> the 44 bytes of a pwaf_client_id as 11 words in memory order: word j holds the 24 bits at bit 24 j of
// the digest; the last one has 16 bits left (three characters) and the NUL
PWAF_SVC_HD void encode(const uint32_t h[8], uint32_t out[kIdWords]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 10; j++) {
        const uint32_t q = (24u * j) >> 5, r = (24u * j) & 31u;
        const uint64_t x = (uint64_t)h[q] << 32 | (q + 1 < 8 ? h[q + 1] : 0u);
        out[j] = b64_quad((uint32_t)(x >> (40u - r)) & 0xFFFFFFu);
    }
    out[10] = b64_quad((h[7] & 0xFFFFu) << 8) & 0x00FFFFFFu;
}

// The id of one message: what every lane of client_id_kernel runs, and the host.
PWAF_SVC_HD void client_id_words(const Message &m, uint32_t out[kIdWords]) {
    uint32_t state[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    const uint64_t nb = m.blocks();
    for (uint64_t b = 0; b < nb; b++) {
        uint32_t w[16];
        load_block(m, b, w);
        compress(state, w);
    }
    encode(state, out);
}

// ---- the batch call ----------------------------------------------------------------------------------------------------------------
// client_id_kernel's arguments, and ids_host's (pwaf_client_ids after its argument checks).
struct Args {
    pwaf_strcol ua, host;  // field[PWAF_FIELD_USER_AGENT], field[PWAF_FIELD_HOST]
    const uint8_t *ip, *ip_is_v6;
    uint32_t n;
    const uint32_t *idx;    // NULL: every request, out[i] belongs to request i
    const uint32_t *n_idx;  // nullable: min(*n_idx, idx_cap) entries are looked at
    uint32_t idx_cap;
    pwaf_client_id *out;
};
PWAF_SVC_HD uint32_t selected(const Args &a) { return pwaf::selected(a.idx, a.n_idx, a.idx_cap, a.n); }
// request i (< a.n) of the batch; lengths in uint32 arithmetic, as every reader of the offsets computes them
PWAF_SVC_HD Message message_of(const Args &a, uint32_t i) {
    const uint32_t u0 = a.ua.offsets[i], h0 = a.host.offsets[i];
    return make_message(a.ip + (size_t)i * 16, a.ip_is_v6[i], a.ua.data + u0, a.ua.offsets[i + 1] - u0, a.host.data + h0, a.host.offsets[i + 1] - h0);
}

// The HOST mode: first every selected request is checked (offsets that decrease in either column: false with *bad = the entry, nothing
// written), then the ids are written in entry order. An entry that names no request of the batch gets 44 zero bytes.
inline bool ids_host(const Args &a, uint32_t *bad) {
    const uint32_t m = selected(a);
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t i = request_of(a.idx, j);
        if (i >= a.n) continue;
        if (a.ua.offsets[i + 1] < a.ua.offsets[i] || a.host.offsets[i + 1] < a.host.offsets[i]) {
            *bad = j;
            return false;
        }
    }
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t i = request_of(a.idx, j);
        uint32_t words[kIdWords] = {0};
        if (i < a.n) client_id_words(message_of(a, i), words);
        memcpy(a.out[j].text, words, sizeof words);
    }
    return true;
}
int launch_client_ids(const Args &a, void *stream);

}  // namespace clientid
}  // namespace pwaf
