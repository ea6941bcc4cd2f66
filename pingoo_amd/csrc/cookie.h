// cookie.h — gate C of the reference for a request (include/pwaf.h: pwaf_verify_cookies, pwaf_verify_cookie_one): is there a
// `__pingoo_captcha_verified` cookie, and is its JWT valid for this client (pingoo/listeners/http_listener.rs:169-181, :222-236;
// CaptchaManager::validate_captcha_verified_cookie, pingoo/captcha.rs:125-156; jwt::parse_header / parse_and_verify, jwt/jwt.rs:198-327).
// DESIGN.md §5.1.6 states the semantics; this header is their only implementation.
//
// One header, compiled three ways, like clientid.h: by cookie.hip for the device (cookie_locate_kernel, cookie_verify_kernel: one request /
// one candidate per lane), by the same unit for the host (the HOST mode, pwaf_verify_cookie_one and key-set creation) and by
// tests/cookie_host.cpp (g++ under the sanitizers). No HIP include: compiled as plain C++ it needs <stdint.h> and <string.h> only.
// csrc/pow.h (pwaf_verify_pow) is built on it: the scan takes the cookie's name (locate_named), the subset reader one
// escape as a template switch (parse_flat_as); gate C uses both as it always did (locate, parse_flat).
//
// What is in it, in order: the cookie scan and the token split; base64url; SHA-512 (FIPS 180-4); arithmetic mod 2^255 - 19 on ten
// 26/25-bit limbs with 64-bit products and mod L (the group order) on 32-bit words; the double-scalar multiplication [S]B + [k](-A) over
// two 16-entry tables (RFC 8032 §5.1); the flat-subset JSON reader, which walks the base64 text and never materialises the JSON; the
// decision; the batch loop of the HOST mode. Square roots, point decompression and the tables are host-only (key-set creation). All of
// the arithmetic is written from RFC 8032 and FIPS 180-4: the reference has none of it (it calls aws-lc).
//
// Nothing is indexed at run time in what a lane keeps: limbs, schedule words and scalars are arrays with literal indices after unrolling
// (a run-time index would put them in scratch), and a scalar's next digit is taken from the top of a register window that is shifted.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "clientid.h"
#include "pwaf.h"
#include "service.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define PWAF_CK_UNROLL _Pragma("unroll")
#define PWAF_CK_CONST __constant__ const
#else
#define PWAF_CK_UNROLL
#define PWAF_CK_CONST static const
#endif

namespace pwaf {
namespace cookie {

static constexpr uint32_t kMaxKeys = PWAF_KEYSET_MAX_KEYS, kMaxKid = PWAF_KEYSET_MAX_KID;
static constexpr uint32_t kMaxSigned = PWAF_COOKIE_MAX_SIGNED_BYTES;  // a longer signed message is not parsed: UNDECIDED behind a verified signature
static constexpr uint8_t kCandidate = 0xFF;                           // locate(): not decided yet
static constexpr uint32_t kSigChars = 86;                             // 64 bytes in base64url without padding

// ---- bytes of a value -----------------------------------------------------------------------------------------------------------------
typedef unsigned __int128 chunk_t;
// up to 16 bytes at s: the device reads 16 and may pass the value's end by up to 15 bytes (inside the arena or its PWAF_ARENA_PAD); the
// host reads exactly `run` bytes
PWAF_SVC_HD chunk_t load_chunk(const uint8_t *s, uint32_t run) {
    chunk_t v = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    memcpy(&v, s, 16);
    (void)run;
#else
    memcpy(&v, s, run);
#endif
    return v;
}

// ---- base64url without padding (jwt.rs:205, :228, :236, :244: URL_SAFE_NO_PAD) -----------------------------------------------------------
// the 6 bits of a character, 64 for a byte outside A-Z a-z 0-9 - _ ('=' included)
PWAF_SVC_HD uint32_t b64_val(uint32_t c) {
    if (c - 'A' < 26u) return c - 'A';
    if (c - 'a' < 26u) return c - 'a' + 26u;
    if (c - '0' < 10u) return c - '0' + 52u;
    return c == '-' ? 62u : c == '_' ? 63u : 64u;
}
// a part of a token as a byte source: byte j of what the text decodes to, without decoding the rest
struct B64 {
    const uint8_t *p;
    uint32_t chars, bytes;  // bytes = floor(6 chars / 8)
};
PWAF_SVC_HD uint32_t b64_byte(const B64 &s, uint32_t j) {  // j < s.bytes, s checked by b64_open
    const uint32_t bit = 8u * j, at = bit / 6u, r = bit % 6u;
    return ((b64_val(s.p[at]) << 6 | b64_val(s.p[at + 1])) >> (4u - r)) & 0xFFu;
}
// false: not base64url without padding (a foreign byte, a length of 1 mod 4, non-zero trailing bits)
PWAF_SVC_HD bool b64_open(const uint8_t *p, uint32_t chars, B64 *out) {
    if ((chars & 3u) == 1u) return false;
    uint32_t last = 0;
    for (uint32_t i = 0; i < chars; i++) {
        last = b64_val(p[i]);
        if (last > 63u) return false;
    }
    const uint32_t spare = (6u * chars) & 7u;  // 0, 4 (two characters left over) or 2 (three)
    if (spare && (last & ((1u << spare) - 1u))) return false;
    *out = B64{p, chars, (6u * chars) >> 3};
    return true;
}
// the signature part: exactly 64 bytes (86 characters, the last with four zero bits) -> R and S as 8 little-endian words each
PWAF_SVC_HD bool decode_signature(const uint8_t *p, uint32_t chars, uint32_t r[8], uint32_t s[8]) {
    if (chars != kSigChars) return false;
    uint32_t w[16] = {0}, bad = 0;
    PWAF_CK_UNROLL
    for (uint32_t g = 0; g < 21; g++) {  // 21 groups of four characters: bytes 3 g .. 3 g + 2
        const uint32_t a = b64_val(p[4 * g]), b = b64_val(p[4 * g + 1]), c = b64_val(p[4 * g + 2]), d = b64_val(p[4 * g + 3]);
        bad |= a | b | c | d;
        const uint32_t v = a << 18 | b << 12 | c << 6 | d;
        PWAF_CK_UNROLL
        for (uint32_t k = 0; k < 3; k++) {
            const uint32_t j = 3 * g + k;
            w[j >> 2] |= ((v >> (16u - 8u * k)) & 0xFFu) << (8u * (j & 3u));
        }
    }
    const uint32_t a = b64_val(p[84]), b = b64_val(p[85]);
    bad |= a | b;
    if ((bad & 64u) || (b & 15u)) return false;
    w[15] |= ((a << 2 | b >> 4) & 0xFFu) << 24;
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 8; i++) r[i] = w[i], s[i] = w[8 + i];
    return true;
}

// ---- the Cookie header (http_listener.rs:169-181; cookie 0.18 Cookie::split_parse behind HeaderValue::to_str) -----------------------------
struct Token {  // where the token's parts lie in the cookie value
    uint32_t at, hdr_len, claims_len;  // header at [at, at + hdr_len), '.', claims, '.', the 86 signature characters
    PWAF_SVC_HD uint32_t signed_len() const { return hdr_len + 1u + claims_len; }
};
PWAF_SVC_HD bool is_blank(uint32_t b) { return b == ' ' || b == '\t'; }
// PWAF_COOKIE_ABSENT, PWAF_COOKIE_INVALID or kCandidate with *t, for the first cookie named exactly kName[0 .. kNameLen)
PWAF_SVC_HD uint8_t locate_named(const uint8_t *v, uint32_t len, Token *t, const char *kName, const uint32_t kNameLen) {
    bool bad = false, found = false, in_value = false;
    uint32_t name0 = 0, name1 = 0, val0 = 0, val1 = 0, tok0 = 0, tok1 = 0;  // [first, last + 1) of the bytes that are not blank; 0, 0: none
    for (uint32_t q0 = 0; q0 <= len; q0 += 16) {  // (q == len closes the last segment)
        const uint32_t run = len - q0 < 16u ? len - q0 : 16u;
        chunk_t c = run ? load_chunk(v + q0, run) : 0;
        for (uint32_t k = 0; k <= run && k < 16u; k++, c >>= 8) {
            const uint32_t q = q0 + k, b = (uint32_t)c & 0xFFu;
            const bool end = q == len;
            if (!end && b != '\t' && b - 0x20u > 0x5Eu) bad = true;  // HeaderValue::to_str fails: no cookies at all
            if (end || b == ';') {
                if (!found && in_value && name1 - name0 == kNameLen) {
                    bool same = true;
                    for (uint32_t i = 0; i < kNameLen; i++) same &= v[name0 + i] == (uint8_t)kName[i];
                    if (same) found = true, tok0 = val0, tok1 = val1;
                }
                in_value = false, name0 = name1 = val0 = val1 = 0;
                if (end) break;
            } else if (!in_value && b == '=') {
                in_value = true;
            } else if (!is_blank(b)) {
                if (!in_value) {
                    if (name1 == 0) name0 = q;
                    name1 = q + 1;
                } else {
                    if (val1 == 0) val0 = q;
                    val1 = q + 1;
                }
            }
        }
        if (run < 16u) break;
    }
    if (bad || !found) return PWAF_COOKIE_ABSENT;
    if (tok1 - tok0 >= 2u && v[tok0] == '"' && v[tok1 - 1] == '"') tok0++, tok1--;
    // exactly three parts (jwt.rs:199-203), the third 64 bytes of base64url (jwt.rs:228-230, Algorithm::signature_size)
    uint32_t dots = 0, dot0 = 0, dot1 = 0;
    for (uint32_t q = tok0; q < tok1; q++)
        if (v[q] == '.') {
            if (dots == 0) dot0 = q;
            if (dots == 1) dot1 = q;
            dots++;
        }
    if (dots != 2u || tok1 - (dot1 + 1u) != kSigChars) return PWAF_COOKIE_INVALID;
    uint32_t r[8], s[8];
    if (!decode_signature(v + dot1 + 1, kSigChars, r, s)) return PWAF_COOKIE_INVALID;
    t->at = tok0, t->hdr_len = dot0 - tok0, t->claims_len = dot1 - dot0 - 1u;
    return kCandidate;
}
PWAF_SVC_HD uint8_t locate(const uint8_t *v, uint32_t len, Token *t) {
    const char kName[] = "__pingoo_captcha_verified";
    return locate_named(v, len, t, kName, sizeof kName - 1);
}

// ---- SHA-512 (FIPS 180-4 §4.1.3, §4.2.3, §5.1.2, §6.4) --------------------------------------------------------------------------------------
PWAF_CK_CONST uint64_t kSha512K[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull,
    0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull,
    0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
    0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
    0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull,
    0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull,
    0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull,
    0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
PWAF_SVC_HD uint64_t rotr64(uint64_t x, uint32_t n) { return (x >> n) | (x << (64u - n)); }
// state += compress(state, w); the rounds in five runs of 16 over a rolling window: w[] keeps literal indices, the round constant is
// read at a wave-uniform index
PWAF_SVC_HD void sha512_compress(uint64_t st[8], uint64_t w[16]) {
    uint64_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    for (uint32_t t0 = 0; t0 < 80; t0 += 16) {
        PWAF_CK_UNROLL
        for (uint32_t j = 0; j < 16; j++) {
            if (t0) {
                const uint64_t x = w[(j + 1) & 15], y = w[(j + 14) & 15];
                w[j] += (rotr64(y, 19) ^ rotr64(y, 61) ^ (y >> 6)) + w[(j + 9) & 15] + (rotr64(x, 1) ^ rotr64(x, 8) ^ (x >> 7));
            }
            const uint64_t t1 = h + (rotr64(e, 14) ^ rotr64(e, 18) ^ rotr64(e, 41)) + (g ^ (e & (f ^ g))) + kSha512K[t0 + j] + w[j];
            const uint64_t t2 = (rotr64(a, 28) ^ rotr64(a, 34) ^ rotr64(a, 39)) + (b ^ ((a ^ b) & (c ^ b)));
            h = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
        }
    }
    st[0] += a, st[1] += b, st[2] += c, st[3] += d, st[4] += e, st[5] += f, st[6] += g, st[7] += h;
}
// The 8 bytes of the padded message at message offset q (a multiple of 8), big-endian. The signed message of a token is FOLLOWED in its
// cookie value by '.' and the 86 signature characters, so the 8-byte load at q <= len stays inside the value, on the host too.
PWAF_SVC_HD uint64_t message_word(const uint8_t *m, uint32_t len, uint32_t q) {
    if (q > len) return 0;
    uint64_t x;
    memcpy(&x, m + q, 8);
    x = __builtin_bswap64(x);
    const uint32_t keep = len - q;
    if (keep >= 8u) return x;
    x = keep ? x & (~0ull << (8u * (8u - keep))) : 0;
    return x | 0x80ull << (8u * (7u - keep));
}
PWAF_SVC_HD uint64_t be_pair(uint32_t lo_word, uint32_t hi_word) { return (uint64_t)__builtin_bswap32(lo_word) << 32 | __builtin_bswap32(hi_word); }
// SHA-512(R || A || m) as the 16 little-endian words of the digest read as one integer (RFC 8032 §5.1.7 step 2)
PWAF_SVC_HD void hash_ram(const uint32_t r[8], const uint32_t a[8], const uint8_t *m, uint32_t len, uint32_t out[16]) {
    uint64_t st[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                      0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
    const uint32_t blocks = (64u + len + 17u + 127u) >> 7;  // the 0x80 byte and the 16-byte length ride in the last one
    for (uint32_t b = 0; b < blocks; b++) {
        uint64_t w[16];
        PWAF_CK_UNROLL
        for (uint32_t t = 0; t < 16; t++) {
            if (b == 0 && t < 4)
                w[t] = be_pair(r[2 * t], r[2 * t + 1]);
            else if (b == 0 && t < 8)
                w[t] = be_pair(a[2 * (t - 4)], a[2 * (t - 4) + 1]);
            else
                w[t] = message_word(m, len, 128u * b + 8u * t - 64u);
        }
        if (b + 1 == blocks) w[15] = (uint64_t)(64u + len) * 8u;  // (w[14], the length's high half, is already 0)
        sha512_compress(st, w);
    }
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 8; i++) out[2 * i] = __builtin_bswap32((uint32_t)(st[i] >> 32)), out[2 * i + 1] = __builtin_bswap32((uint32_t)st[i]);
}

// ---- arithmetic mod p = 2^255 - 19 ---------------------------------------------------------------------------------------------------------
// Ten limbs, limb i of weight 2^ceil(25.5 i): 26 bits at even i, 25 at odd i. Every function returns limbs below 2^26 (even) and
// 2^25 + 2^15 (odd; limb 1 takes the last carry) and accepts such limbs: they stay below the limbs of 2p, which the subtraction adds, and
// the 64-bit products (v_mad_u64_u32) of a column of ten, with the factors 2 and 19, stay below 2^61.
struct fe {
    uint32_t v[10];
};
static constexpr uint32_t kM26 = 0x3FFFFFFu, kM25 = 0x1FFFFFFu;
PWAF_SVC_HD void fe_carry(fe &h) {  // limbs below 2^31
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 9; i++) {
        const uint32_t bits = (i & 1u) ? 25u : 26u;
        h.v[i + 1] += h.v[i] >> bits;
        h.v[i] &= (1u << bits) - 1u;
    }
    h.v[0] += 19u * (h.v[9] >> 25);
    h.v[9] &= kM25;
    h.v[1] += h.v[0] >> 26;
    h.v[0] &= kM26;
}
PWAF_SVC_HD fe fe_small(uint32_t x) {
    fe h = {{x, 0, 0, 0, 0, 0, 0, 0, 0, 0}};
    return h;
}
PWAF_SVC_HD fe fe_add(const fe &f, const fe &g) {
    fe h;
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 10; i++) h.v[i] = f.v[i] + g.v[i];
    fe_carry(h);
    return h;
}
PWAF_SVC_HD fe fe_sub(const fe &f, const fe &g) {  // f + 2p - g
    fe h;
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 10; i++) h.v[i] = f.v[i] + (i == 0 ? 0x7FFFFDAu : (i & 1u) ? 0x3FFFFFEu : 0x7FFFFFEu) - g.v[i];
    fe_carry(h);
    return h;
}
// the term f_i g_j belongs to limb i + j: twice when both i and j are odd (their weights round up), 19 times when i + j >= 10 (2^255 = 19)
PWAF_SVC_HD fe fe_mul(const fe &f, const fe &g) {
    uint32_t g19[10], f2[10];
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 10; i++) g19[i] = 19u * g.v[i], f2[i] = (i & 1u) ? 2u * f.v[i] : f.v[i];
    uint64_t t[10] = {0};
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 10; i++) {
        PWAF_CK_UNROLL
        for (uint32_t j = 0; j < 10; j++) {
            const uint32_t a = (j & 1u) ? f2[i] : f.v[i], b = i + j >= 10u ? g19[j] : g.v[j];
            t[(i + j) % 10u] += (uint64_t)a * b;
        }
    }
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 9; i++) {
        const uint32_t bits = (i & 1u) ? 25u : 26u;
        t[i + 1] += t[i] >> bits;
        t[i] &= (1u << bits) - 1u;
    }
    t[0] += 19u * (t[9] >> 25);
    t[9] &= kM25;
    t[1] += t[0] >> 26;
    t[0] &= kM26;
    fe h;
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 10; i++) h.v[i] = (uint32_t)t[i];
    return h;
}
PWAF_SVC_HD fe fe_sq(const fe &f) { return fe_mul(f, f); }
PWAF_SVC_HD fe fe_sq_times(fe f, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) f = fe_sq(f);
    return f;
}
// z^(2^250 - 1) and z^11: the common part of the inversion (z^(p - 2)) and of the square root's z^((p - 5) / 8)
PWAF_SVC_HD fe fe_pow_250(const fe &z, fe *z11) {
    const fe z2 = fe_sq(z), z9 = fe_mul(fe_sq_times(z2, 2), z);
    *z11 = fe_mul(z9, z2);
    const fe z5_0 = fe_mul(fe_sq(*z11), z9);  // z^(2^5 - 1)
    const fe z10_0 = fe_mul(fe_sq_times(z5_0, 5), z5_0);
    const fe z20_0 = fe_mul(fe_sq_times(z10_0, 10), z10_0);
    const fe z40_0 = fe_mul(fe_sq_times(z20_0, 20), z20_0);
    const fe z50_0 = fe_mul(fe_sq_times(z40_0, 10), z10_0);
    const fe z100_0 = fe_mul(fe_sq_times(z50_0, 50), z50_0);
    const fe z200_0 = fe_mul(fe_sq_times(z100_0, 100), z100_0);
    return fe_mul(fe_sq_times(z200_0, 50), z50_0);
}
PWAF_SVC_HD fe fe_invert(const fe &z) {  // z^(2^255 - 21)
    fe z11;
    const fe z250_0 = fe_pow_250(z, &z11);
    return fe_mul(fe_sq_times(z250_0, 5), z11);
}
// the canonical value (below p) as 8 little-endian words, bit 255 clear
PWAF_SVC_HD void fe_words(fe h, uint32_t out[8]) {
    fe_carry(h);
    fe_carry(h);  // the value is now below 2^255 + 2^8
    uint32_t q = (h.v[0] + 19u) >> 26;
    PWAF_CK_UNROLL
    for (uint32_t i = 1; i < 10; i++) q = (h.v[i] + q) >> ((i & 1u) ? 25u : 26u);  // 1 iff the value is at least p
    h.v[0] += 19u * q;
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 9; i++) {
        const uint32_t bits = (i & 1u) ? 25u : 26u;
        h.v[i + 1] += h.v[i] >> bits;
        h.v[i] &= (1u << bits) - 1u;
    }
    h.v[9] &= kM25;  // minus 2^255 when q
    uint64_t acc[9] = {0};
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 10; i++) {
        const uint32_t at = (51u * i + 1u) / 2u;  // ceil(25.5 i)
        const uint64_t x = (uint64_t)h.v[i] << (at & 31u);
        acc[at >> 5] |= (uint32_t)x;
        acc[(at >> 5) + 1] |= x >> 32;
    }
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 8; i++) out[i] = (uint32_t)acc[i];
}
PWAF_SVC_HD fe fe_from_words(const uint32_t w[8]) {  // bit 255 is ignored
    fe h;
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 10; i++) {
        const uint32_t at = (51u * i + 1u) / 2u, k = at >> 5;
        const uint64_t x = (uint64_t)w[k] | (k + 1 < 8 ? (uint64_t)w[k + 1] << 32 : 0);
        h.v[i] = (uint32_t)(x >> (at & 31u)) & ((i & 1u) ? kM25 : kM26);
    }
    return h;
}

// ---- the group: -x^2 + y^2 = 1 + d x^2 y^2 (RFC 8032 §5.1), extended coordinates -------------------------------------------------------------
struct Point {
    fe x, y, z, t;  // x = X/Z, y = Y/Z, x y = T/Z
};
struct Precomp {  // an affine point as the addition wants it: 120 bytes
    uint32_t ypx[10], ymx[10], t2d[10];  // y + x, y - x, 2 d x y; {1, 1, 0} is the neutral element
};
PWAF_SVC_HD Point point_neutral() { return Point{fe_small(0), fe_small(1), fe_small(1), fe_small(0)}; }
// RFC 8032 §5.1.4, doubling; T of the result only where the next step is an addition
PWAF_SVC_HD Point point_double(const Point &p, bool want_t) {
    const fe a = fe_sq(p.x), b = fe_sq(p.y), zz = fe_sq(p.z), c = fe_add(zz, zz), h = fe_add(a, b);
    const fe e = fe_sub(h, fe_sq(fe_add(p.x, p.y))), g = fe_sub(a, b), f = fe_add(c, g);
    Point r;
    r.x = fe_mul(e, f), r.y = fe_mul(g, h), r.z = fe_mul(f, g);
    r.t = want_t ? fe_mul(e, h) : p.t;
    return r;
}
// RFC 8032 §5.1.4, addition, with Z2 = 1 and the second point's y - x, y + x and 2 d T2 ready; entry `digit` (0..15) of a 16-entry table
PWAF_SVC_HD Point point_add_table(const Point &p, const Precomp *table, uint32_t digit) {
    const uint32_t *w = table[digit].ypx;  // 30 words
    fe ypx, ymx, t2d;
    PWAF_CK_UNROLL
    for (uint32_t i = 0; i < 10; i++) ypx.v[i] = w[i], ymx.v[i] = w[10 + i], t2d.v[i] = w[20 + i];
    const fe a = fe_mul(fe_sub(p.y, p.x), ymx), b = fe_mul(fe_add(p.y, p.x), ypx), c = fe_mul(p.t, t2d), d = fe_add(p.z, p.z);
    const fe e = fe_sub(b, a), f = fe_sub(d, c), g = fe_add(d, c), h = fe_add(b, a);
    return Point{fe_mul(e, f), fe_mul(g, h), fe_mul(f, g), fe_mul(e, h)};
}
// the encoding of a point (RFC 8032 §5.1.2) as 8 little-endian words
PWAF_SVC_HD void point_encode(const Point &p, uint32_t out[8]) {
    const fe zi = fe_invert(p.z);
    uint32_t xw[8];
    fe_words(fe_mul(p.x, zi), xw);
    fe_words(fe_mul(p.y, zi), out);
    out[7] |= (xw[0] & 1u) << 31;
}

// ---- scalars: mod L = 2^252 + c (RFC 8032 §5.1) ------------------------------------------------------------------------------------------------
template <int NA, int NB>
PWAF_SVC_HD void words_mul(const uint32_t (&a)[NA], const uint32_t (&b)[NB], uint32_t (&out)[NA + NB]) {
    PWAF_CK_UNROLL
    for (int i = 0; i < NA + NB; i++) out[i] = 0;
    PWAF_CK_UNROLL
    for (int i = 0; i < NA; i++) {
        uint64_t carry = 0;
        PWAF_CK_UNROLL
        for (int j = 0; j < NB; j++) {
            const uint64_t t = (uint64_t)a[i] * b[j] + out[i + j] + carry;
            out[i + j] = (uint32_t)t;
            carry = t >> 32;
        }
        out[i + NB] = (uint32_t)carry;
    }
}
// the low 252 bits of x (8 words) and x >> 252 (NH words), x having NX words
template <int NX, int NH>
PWAF_SVC_HD void words_split252(const uint32_t (&x)[NX], uint32_t (&lo)[8], uint32_t (&hi)[NH]) {
    PWAF_CK_UNROLL
    for (int i = 0; i < 8; i++) lo[i] = i < NX ? x[i] : 0u;
    lo[7] &= 0x0FFFFFFFu;
    PWAF_CK_UNROLL
    for (int i = 0; i < NH; i++) hi[i] = (7 + i < NX ? x[7 + i] >> 28 : 0u) | (8 + i < NX ? x[8 + i] << 4 : 0u);
}
PWAF_SVC_HD bool words_less(const uint32_t a[8], const uint32_t b[8]) {  // a < b
    bool less = false, decided = false;
    PWAF_CK_UNROLL
    for (int i = 7; i >= 0; i--) {
        if (!decided && a[i] != b[i]) less = a[i] < b[i], decided = true;
    }
    return less;
}
PWAF_SVC_HD void order_words(uint32_t l[8]) {
    l[0] = 0x5CF5D3EDu, l[1] = 0x5812631Au, l[2] = 0xA2F79CD6u, l[3] = 0x14DEF9DEu, l[4] = l[5] = l[6] = 0, l[7] = 0x10000000u;
}
// x mod L for a 512-bit x. With x = lo + 2^252 hi and 2^252 = -c (mod L):  x = lo - c hi;  c hi = ylo + 2^252 yhi = ylo - c yhi;
// c yhi = zlo + 2^252 zhi = zlo - c zhi. So x = lo + zlo - ylo - c zhi, each term below 2^252 (c zhi below 2^131): plus 2 L it is
// positive and below 4 L, and at most three subtractions of L finish it. No negative number occurs.
PWAF_SVC_HD void scalar_reduce(const uint32_t x[16], uint32_t out[8]) {
    const uint32_t c[4] = {0x5CF5D3EDu, 0x5812631Au, 0xA2F79CD6u, 0x14DEF9DEu};
    uint32_t xx[16], lo[8], hi[9], y[13], ylo[8], yhi[5], z[9], zlo[8], zhi[1], w[5], l[8];
    PWAF_CK_UNROLL
    for (int i = 0; i < 16; i++) xx[i] = x[i];
    words_split252<16, 9>(xx, lo, hi);
    words_mul<9, 4>(hi, c, y);
    words_split252<13, 5>(y, ylo, yhi);
    words_mul<5, 4>(yhi, c, z);
    words_split252<9, 1>(z, zlo, zhi);
    words_mul<1, 4>(zhi, c, w);
    order_words(l);
    uint32_t t[8];
    uint64_t carry = 0;
    PWAF_CK_UNROLL
    for (int i = 0; i < 8; i++) {  // lo + zlo + 2 L: below 2^255
        carry += (uint64_t)lo[i] + zlo[i] + 2ull * l[i];
        t[i] = (uint32_t)carry;
        carry >>= 32;
    }
    uint64_t borrow = 0;
    PWAF_CK_UNROLL
    for (int i = 0; i < 8; i++) {  // - ylo - w
        const uint64_t sub = (uint64_t)ylo[i] + (i < 5 ? w[i] : 0u) + borrow;
        const uint64_t d = (uint64_t)t[i] - sub;
        t[i] = (uint32_t)d;
        borrow = (d >> 32) ? (0u - (uint32_t)(d >> 32)) : 0u;  // how many times 2^32 was borrowed: 0, 1 or 2
    }
    for (int k = 0; k < 4; k++) {
        if (words_less(t, l)) break;
        uint64_t b = 0;
        PWAF_CK_UNROLL
        for (int i = 0; i < 8; i++) {
            const uint64_t d = (uint64_t)t[i] - l[i] - b;
            t[i] = (uint32_t)d;
            b = (d >> 32) & 1u;
        }
    }
    PWAF_CK_UNROLL
    for (int i = 0; i < 8; i++) out[i] = t[i];
}

// ---- keys ----------------------------------------------------------------------------------------------------------------------------------
struct KeyEntry {
    uint32_t a[8];  // the public key's encoding, as the hash takes it
    uint32_t kid_len, pad[3];
    uint8_t kid[kMaxKid];
    Precomp neg_a[16];  // digit * (-A)
};
struct KeySetData {  // what the verifier reads: one block, in host memory and (device >= 0) in device memory
    uint32_t n_keys, pad[3];
    Precomp base[16];  // digit * B
    KeyEntry keys[kMaxKeys];
};

// RFC 8032 §5.1.7 as aws-lc's ED25519_verify does it: S below L; k = SHA-512(R || A || m) mod L; [S]B + [k](-A) encoded and compared byte for
// byte with R, which is never decompressed. `base`: the 16 multiples of B (the kernel's copy in LDS, or data.base).
PWAF_SVC_HD bool signature_ok(const Precomp *base, const KeyEntry &key, const uint32_t r[8], const uint32_t s_in[8], const uint8_t *m, uint32_t len) {
    uint32_t l[8], s[8], k[8], digest[16];
    order_words(l);
    if (!words_less(s_in, l)) return false;
    hash_ram(r, key.a, m, len, digest);
    scalar_reduce(digest, k);
    PWAF_CK_UNROLL
    for (int i = 0; i < 8; i++) s[i] = s_in[i];
    Point p = point_neutral();
    for (uint32_t i = 0; i < 64; i++) {  // 4 bits of each scalar from the top, shifted out of an 8-word window
        if (i) {
            p = point_double(p, false), p = point_double(p, false), p = point_double(p, false), p = point_double(p, true);
        }
        const uint32_t ds = s[7] >> 28, dk = k[7] >> 28;
        PWAF_CK_UNROLL
        for (int j = 7; j > 0; j--) s[j] = s[j] << 4 | s[j - 1] >> 28, k[j] = k[j] << 4 | k[j - 1] >> 28;
        s[0] <<= 4, k[0] <<= 4;
        p = point_add_table(p, base, ds);
        p = point_add_table(p, key.neg_a, dk);
    }
    uint32_t enc[8], diff = 0;
    point_encode(p, enc);
    PWAF_CK_UNROLL
    for (int i = 0; i < 8; i++) diff |= enc[i] ^ r[i];
    return diff == 0;
}

// ---- the flat subset of JSON -----------------------------------------------------------------------------------------------
// One object of "name": value pairs; names and strings of bytes 0x20..0x7E without '\'; integers that fit int64, without fraction or
// exponent ("-0" is not one: serde_json reads it as a float); true, false, null (= absent); no nesting. The reader walks the base64 text.
enum Kind : uint32_t { kAbsent = 0, kString = 1, kInt = 2, kTrue = 3, kFalse = 4 };
struct Value {
    uint32_t kind, at, len;  // a string's bytes [at, at + len) of the decoded part
    int64_t num;
};
static constexpr uint32_t kMaxNames = 9;
struct Names {
    const char *name[kMaxNames];
    uint32_t n;
};
PWAF_SVC_HD bool text_is(const B64 &s, uint32_t at, uint32_t len, const char *lit) {
    uint32_t i = 0;
    for (; i < len && lit[i]; i++)
        if (b64_byte(s, at + i) != (uint8_t)lit[i]) return false;
    return i == len && !lit[i];
}
PWAF_SVC_HD bool is_json_space(uint32_t b) { return b == ' ' || b == '\t' || b == '\n' || b == '\r'; }
// false: outside the subset (or a known name twice). out[k] is the value of names.name[k]; unknown names are skipped.
// kNulEscape (the claims of pwaf_verify_pow only): inside a string VALUE the six bytes \u0000 are read as one byte 0x00;
// the value's [at, at + len) stays the text as it stands, and whoever reads it skips six bytes at a backslash (escape_aware_byte). Every
// other backslash, and every backslash in a name, stays outside the subset.
template <bool kNulEscape>
PWAF_SVC_HD bool parse_flat_as(const B64 &s, const Names &names, Value out[kMaxNames]) {
    PWAF_CK_UNROLL
    for (uint32_t k = 0; k < kMaxNames; k++) out[k] = Value{kAbsent, 0, 0, 0};
    const uint32_t n = s.bytes;
    uint32_t q = 0, seen = 0;
#define PWAF_CK_SKIP_SPACE() \
    while (q < n && is_json_space(b64_byte(s, q))) q++
#define PWAF_CK_STRING(at_var, len_var, escapes)                                                                      \
    {                                                                                                                 \
        at_var = ++q;                                                                                                 \
        for (;; q++) {                                                                                                \
            if (q >= n) return false;                                                                                 \
            const uint32_t b = b64_byte(s, q);                                                                        \
            if (b == '"') break;                                                                                      \
            if (b - 0x20u > 0x5Eu) return false;                                                                      \
            if (b == '\\') {                                                                                          \
                if (!(escapes) || q + 5u >= n || b64_byte(s, q + 1) != 'u') return false;                             \
                for (uint32_t z = 2; z < 6; z++)                                                                      \
                    if (b64_byte(s, q + z) != '0') return false;                                                      \
                q += 5;                                                                                               \
            }                                                                                                         \
        }                                                                                                             \
        len_var = q - at_var;                                                                                         \
        q++;                                                                                                          \
    }
    PWAF_CK_SKIP_SPACE();
    if (q >= n || b64_byte(s, q) != '{') return false;
    q++;
    PWAF_CK_SKIP_SPACE();
    if (q < n && b64_byte(s, q) == '}') {
        q++;
    } else {
        for (;;) {
            PWAF_CK_SKIP_SPACE();
            if (q >= n || b64_byte(s, q) != '"') return false;
            uint32_t name_at, name_len;
            PWAF_CK_STRING(name_at, name_len, false)
            PWAF_CK_SKIP_SPACE();
            if (q >= n || b64_byte(s, q) != ':') return false;
            q++;
            PWAF_CK_SKIP_SPACE();
            if (q >= n) return false;
            Value v{kAbsent, 0, 0, 0};
            const uint32_t b = b64_byte(s, q);
            if (b == '"') {
                v.kind = kString;
                PWAF_CK_STRING(v.at, v.len, kNulEscape)
            } else if (b == 't' || b == 'f' || b == 'n') {
                const char *lit = b == 't' ? "true" : b == 'f' ? "false" : "null";
                const uint32_t len = b == 'f' ? 5u : 4u;
                if (q + len > n || !text_is(s, q, len, lit)) return false;
                v.kind = b == 't' ? kTrue : b == 'f' ? kFalse : kAbsent;
                q += len;
            } else if (b == '-' || b - '0' < 10u) {
                const bool neg = b == '-';
                if (neg) q++;
                if (q >= n) return false;
                const uint32_t first = b64_byte(s, q);
                if (first - '0' >= 10u) return false;
                uint64_t mag = 0;
                uint32_t digits = 0;
                for (; q < n; q++, digits++) {
                    const uint32_t d = b64_byte(s, q) - '0';
                    if (d >= 10u) break;
                    if (mag > (0x8000000000000000ull - d) / 10u) return false;  // beyond int64
                    mag = mag * 10u + d;
                }
                if (first == '0' && (digits > 1u || neg)) return false;  // a leading zero; "-0"
                if (mag > (neg ? 0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFull)) return false;
                if (q < n) {
                    const uint32_t next = b64_byte(s, q);
                    if (next == '.' || next == 'e' || next == 'E') return false;
                }
                v.kind = kInt;
                v.num = (int64_t)(neg ? 0ull - mag : mag);
            } else {
                return false;  // a nested value, or no value
            }
            PWAF_CK_UNROLL
            for (uint32_t k = 0; k < kMaxNames; k++)  // (unrolled: names.name[] keeps literal indices)
                if (k < names.n && text_is(s, name_at, name_len, names.name[k])) {
                    if (seen >> k & 1u) return false;
                    seen |= 1u << k;
                    PWAF_CK_UNROLL
                    for (uint32_t j = 0; j < kMaxNames; j++)
                        if (j == k) out[j] = v;
                }
            PWAF_CK_SKIP_SPACE();
            if (q >= n) return false;
            const uint32_t sep = b64_byte(s, q);
            q++;
            if (sep == '}') break;
            if (sep != ',') return false;
        }
    }
    PWAF_CK_SKIP_SPACE();
    return q == n;
#undef PWAF_CK_STRING
#undef PWAF_CK_SKIP_SPACE
}
PWAF_SVC_HD bool parse_flat(const B64 &s, const Names &names, Value out[kMaxNames]) { return parse_flat_as<false>(s, names, out); }
// the next byte of a string value that parse_flat_as<true> accepted, *q moving over it: a backslash there begins \u0000
PWAF_SVC_HD uint32_t escape_aware_byte(const B64 &s, uint32_t *q) {
    const uint32_t b = b64_byte(s, *q);
    *q += b == '\\' ? 6u : 1u;
    return b == '\\' ? 0u : b;
}
PWAF_SVC_HD bool string_or_absent(const Value &v) { return v.kind == kAbsent || v.kind == kString; }

// ---- the decision (captcha.rs:125-156; jwt.rs:213-327) ---------------------------------------------------------------------------------------
// The header (jwt.rs:36-85): false = the device does not parse it. *key = the key its kid names (kMaxKeys: none), *alg_typ_ok
PWAF_SVC_HD bool read_header(const KeySetData &ks, const uint8_t *p, uint32_t chars, uint32_t *key, bool *alg_typ_ok) {
    B64 s;
    if (!b64_open(p, chars, &s)) return false;
    const Names names = {{"typ", "alg", "kid", "cty", "jku", "x5u", "x5t", "x5t#S256", "x5c"}, 9};
    Value v[kMaxNames];
    if (!parse_flat(s, names, v)) return false;
    if (!string_or_absent(v[3]) || !string_or_absent(v[4]) || !string_or_absent(v[5]) || !string_or_absent(v[6]) || !string_or_absent(v[7]) || v[8].kind != kAbsent)
        return false;  // serde refuses these; the host says so
    *alg_typ_ok = v[0].kind == kString && text_is(s, v[0].at, v[0].len, "JWT") && v[1].kind == kString && text_is(s, v[1].at, v[1].len, "EdDSA");
    *key = kMaxKeys;
    if (v[2].kind == kString && v[2].len && v[2].len <= kMaxKid)
        for (uint32_t k = 0; k < ks.n_keys && k < kMaxKeys; k++) {
            const KeyEntry &e = ks.keys[k];
            if (e.kid_len != v[2].len) continue;
            bool same = true;
            for (uint32_t i = 0; i < e.kid_len; i++) same &= b64_byte(s, v[2].at + i) == e.kid[i];
            if (same) {
                *key = k;
                break;
            }
        }
    return true;
}
// The claims (captcha.rs:70-75, jwt.rs:89-124) behind a verified signature: VERIFIED, INVALID, or UNDECIDED where the device does not parse them
PWAF_SVC_HD uint8_t judge_claims(const uint8_t *p, uint32_t chars, int64_t now, const uint32_t id[clientid::kIdWords]) {
    B64 s;
    if (!b64_open(p, chars, &s)) return PWAF_COOKIE_UNDECIDED;
    const Names names = {{"challenge_passed", "iss", "sub", "aud", "exp", "nbf", "iat", "jti", ""}, 8};
    Value v[kMaxNames];
    if (!parse_flat(s, names, v)) return PWAF_COOKIE_UNDECIDED;
    if ((v[6].kind != kAbsent && v[6].kind != kInt) || !string_or_absent(v[7])) return PWAF_COOKIE_UNDECIDED;  // serde refuses these; the host says so
    const int64_t kMin = (int64_t)0x8000000000000000ull, kMax = 0x7FFFFFFFFFFFFFFFll;
    const int64_t earliest = now < kMin + 5 ? kMin : now - 5, latest = now > kMax - 5 ? kMax : now + 5;  // JWT_VALDIATION_OPTIONS: 5 s of drift
    bool ok = v[4].kind == kInt && v[4].num >= earliest;                                                   // jwt.rs:258-271
    ok &= v[5].kind == kInt && v[5].num <= latest;                                                         // jwt.rs:273-286
    ok &= v[3].kind == kString && text_is(s, v[3].at, v[3].len, "pingoo");                                 // jwt.rs:288-301
    ok &= v[1].kind == kString && text_is(s, v[1].at, v[1].len, "pingoo");                                 // jwt.rs:303-316
    ok &= v[0].kind == kTrue;                                                                              // captcha.rs:150
    ok &= v[2].kind == kString && v[2].len == 43u;                                                         // captcha.rs:147-149
    if (!ok) return PWAF_COOKIE_INVALID;
    uint32_t diff = 0;
    PWAF_CK_UNROLL
    for (uint32_t j = 0; j < clientid::kIdWords; j++) {
        uint32_t w = 0;
        PWAF_CK_UNROLL
        for (uint32_t k = 0; k < 4; k++)
            if (4 * j + k < 43u) w |= b64_byte(s, v[2].at + 4 * j + k) << (8u * k);
        diff |= w ^ id[j];
    }
    return diff ? PWAF_COOKIE_INVALID : PWAF_COOKIE_VERIFIED;
}
// A located token of a request whose client id is id[]: the answer to gate C. `v` is the cookie value.
PWAF_SVC_HD uint8_t judge(const KeySetData &ks, const Precomp *base, const uint8_t *v, const Token &t, int64_t now, const uint32_t id[clientid::kIdWords]) {
    const uint8_t *m = v + t.at;
    const uint32_t len = t.signed_len();
    uint32_t r[8], s[8], key = kMaxKeys;
    if (!decode_signature(m + len + 1, kSigChars, r, s)) return PWAF_COOKIE_INVALID;  // (locate() saw to it)
    bool alg_typ_ok = false;
    if (len <= kMaxSigned && read_header(ks, m, t.hdr_len, &key, &alg_typ_ok)) {
        if (key >= kMaxKeys || !alg_typ_ok) return PWAF_COOKIE_INVALID;  // captcha.rs:132-140; jwt.rs:208, :240
        if (!signature_ok(base, ks.keys[key], r, s, m, len)) return PWAF_COOKIE_INVALID;
        return judge_claims(m + t.hdr_len + 1, t.claims_len, now, id);
    }
    // a header this code does not parse: whoever signed it holds a key of the set, or it is invalid
    for (uint32_t k = 0; k < ks.n_keys && k < kMaxKeys; k++)
        if (signature_ok(base, ks.keys[k], r, s, m, len)) return PWAF_COOKIE_UNDECIDED;
    return PWAF_COOKIE_INVALID;
}

// ---- the batch call ---------------------------------------------------------------------------------------------------------------------------
struct Candidate {  // 16 bytes: what cookie_locate_kernel hands cookie_verify_kernel
    uint32_t entry, at, hdr_len, claims_len;
};
struct Args {
    const KeySetData *ks;  // where the batch lives
    pwaf_strcol cookies, ua, host;
    const uint8_t *ip, *ip_is_v6, *flags;  // flags: nullable
    uint32_t n;
    int64_t now;
    const uint32_t *idx;    // NULL: every request, status[i] belongs to request i
    const uint32_t *n_idx;  // nullable: min(*n_idx, idx_cap) entries are looked at
    uint32_t idx_cap;
    uint8_t *status, *flags_out;  // flags_out: nullable, written only when idx == NULL
    uint32_t *count;              // DEVICE mode: the candidates' number (zeroed in front of the launches) and the list
    Candidate *cand;
};
PWAF_SVC_HD uint32_t selected(const Args &a) { return pwaf::selected(a.idx, a.n_idx, a.idx_cap, a.n); }
PWAF_SVC_HD uint32_t request_of(const Args &a, uint32_t e) { return pwaf::request_of(a.idx, e); }
// entry e's first step: ABSENT / INVALID, or kCandidate with *c
PWAF_SVC_HD uint8_t locate_entry(const Args &a, uint32_t e, Candidate *c) {
    const uint32_t i = request_of(a, e);
    if (i >= a.n) return PWAF_COOKIE_ABSENT;
    const uint32_t c0 = a.cookies.offsets[i];
    Token t{0, 0, 0};
    const uint8_t st = locate(a.cookies.data + c0, a.cookies.offsets[i + 1] - c0, &t);
    *c = Candidate{e, t.at, t.hdr_len, t.claims_len};
    return st;
}
PWAF_SVC_HD uint8_t judge_candidate(const Args &a, const Precomp *base, const Candidate &c) {
    const uint32_t i = request_of(a, c.entry);
    const uint32_t u0 = a.ua.offsets[i], h0 = a.host.offsets[i];
    uint32_t id[clientid::kIdWords];
    clientid::client_id_words(clientid::make_message(a.ip + (size_t)i * 16, a.ip_is_v6[i], a.ua.data + u0, a.ua.offsets[i + 1] - u0, a.host.data + h0, a.host.offsets[i + 1] - h0), id);
    return judge(*a.ks, base, a.cookies.data + a.cookies.offsets[i], Token{c.at, c.hdr_len, c.claims_len}, a.now, id);
}
PWAF_SVC_HD uint8_t flag_of(const Args &a, uint32_t i, uint8_t status) {
    const uint8_t f = a.flags ? a.flags[i] : 0;
    return status == PWAF_COOKIE_VERIFIED ? f | PWAF_FLAG_CAPTCHA_VERIFIED : f & (uint8_t)~PWAF_FLAG_CAPTCHA_VERIFIED;
}

// The HOST mode: first every selected request is checked (offsets that decrease in a column: false with *bad = the entry, nothing
// written), then the answers are written in entry order.
inline bool verify_host(const Args &a, uint32_t *bad) {
    const uint32_t m = selected(a);
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t i = request_of(a, j);
        if (i >= a.n) continue;
        if (a.cookies.offsets[i + 1] < a.cookies.offsets[i] || a.ua.offsets[i + 1] < a.ua.offsets[i] || a.host.offsets[i + 1] < a.host.offsets[i]) {
            *bad = j;
            return false;
        }
    }
    for (uint32_t j = 0; j < m; j++) {
        Candidate c;
        uint8_t st = locate_entry(a, j, &c);
        if (st == kCandidate) st = judge_candidate(a, a.ks->base, c);
        if (!a.idx && a.flags_out) a.flags_out[j] = flag_of(a, j, st);
        a.status[j] = st;
    }
    return true;
}
int launch_verify_cookies(const Args &a, void *stream);

// ---- key-set creation: host only ----------------------------------------------------------------------------------------------------------------
inline fe fe_pow_bytes(const fe &z, const uint8_t e[32]) {  // square and multiply, the exponent little-endian
    fe r = fe_small(1);
    for (int bit = 255; bit >= 0; bit--) {
        r = fe_sq(r);
        if (e[bit >> 3] >> (bit & 7) & 1) r = fe_mul(r, z);
    }
    return r;
}
inline bool fe_equal(const fe &a, const fe &b) {
    uint32_t x[8], y[8];
    fe_words(a, x), fe_words(b, y);
    return memcmp(x, y, sizeof x) == 0;
}
inline fe curve_d() { return fe_mul(fe_sub(fe_small(0), fe_small(121665)), fe_invert(fe_small(121666))); }  // -121665 / 121666
// RFC 8032 §5.1.3: false for an encoding that is not canonical (y >= p, or x = 0 with the sign bit) or not on the curve
inline bool point_decompress(const uint8_t enc[32], fe *x, fe *y) {
    uint32_t w[8], back[8];
    memcpy(w, enc, 32);
    const uint32_t sign = w[7] >> 31;
    *y = fe_from_words(w);
    fe_words(*y, back);
    w[7] &= 0x7FFFFFFFu;
    if (memcmp(w, back, 32) != 0) return false;  // y >= p
    const fe one = fe_small(1), yy = fe_sq(*y), u = fe_sub(yy, one), v = fe_add(fe_mul(curve_d(), yy), one);
    uint8_t e[32];  // (p - 5) / 8 = 2^252 - 3
    memset(e, 0xFF, 32), e[0] = 0xFD, e[31] = 0x0F;
    const fe v3 = fe_mul(fe_sq(v), v), v7 = fe_mul(fe_sq(v3), v);
    fe r = fe_mul(fe_mul(u, v3), fe_pow_bytes(fe_mul(u, v7), e));
    const fe vrr = fe_mul(v, fe_sq(r));
    if (!fe_equal(vrr, u)) {
        if (!fe_equal(vrr, fe_sub(fe_small(0), u))) return false;
        memset(e, 0xFF, 32), e[0] = 0xFB, e[31] = 0x1F;  // sqrt(-1) = 2^((p - 1) / 4), (p - 1) / 4 = 2^253 - 5
        r = fe_mul(r, fe_pow_bytes(fe_small(2), e));
    }
    uint32_t rw[8];
    fe_words(r, rw);
    bool zero = true;
    for (int i = 0; i < 8; i++) zero &= rw[i] == 0;
    if (zero && sign) return false;
    *x = (rw[0] & 1u) != sign ? fe_sub(fe_small(0), r) : r;
    return true;
}
inline void precomp_of(const Point &p, const fe &d2, Precomp *out) {
    const fe zi = fe_invert(p.z), x = fe_mul(p.x, zi), y = fe_mul(p.y, zi);
    const fe ypx = fe_add(y, x), ymx = fe_sub(y, x), t2d = fe_mul(fe_mul(x, y), d2);
    memcpy(out->ypx, ypx.v, 40), memcpy(out->ymx, ymx.v, 40), memcpy(out->t2d, t2d.v, 40);
}
// table[digit] = digit * (x, y), digit 0..15
inline void build_table(const fe &x, const fe &y, Precomp table[16]) {
    const fe d = curve_d(), d2 = fe_add(d, d);
    precomp_of(point_neutral(), d2, &table[0]);
    Precomp one[1];
    precomp_of(Point{x, y, fe_small(1), fe_mul(x, y)}, d2, one);
    Point q = point_neutral();
    for (uint32_t digit = 1; digit < 16; digit++) {
        q = point_add_table(q, one, 0);
        precomp_of(q, d2, &table[digit]);
    }
}
inline bool build_base_table(Precomp table[16]) {
    uint8_t enc[32];  // B: y = 4 / 5, x positive (RFC 8032 §5.1)
    memset(enc, 0x66, 32), enc[0] = 0x58;
    fe x, y;
    if (!point_decompress(enc, &x, &y)) return false;
    build_table(x, y, table);
    return true;
}
// one key of the set: false for an x that is not a canonical point on the curve
inline bool build_key(const uint8_t enc[32], const char *kid, uint32_t kid_len, KeyEntry *out) {
    fe x, y;
    if (!point_decompress(enc, &x, &y)) return false;
    memset(out, 0, sizeof *out);
    memcpy(out->a, enc, 32);
    out->kid_len = kid_len;
    memcpy(out->kid, kid, kid_len);
    build_table(fe_sub(fe_small(0), x), y, out->neg_a);
    return true;
}

}  // namespace cookie
}  // namespace pwaf

struct pwaf_keyset {  // include/pwaf.h's opaque type: cookie.hip creates and destroys it, cookie.hip and pow.hip read it
    pwaf::cookie::KeySetData data;
    pwaf::cookie::KeySetData *dev;  // NULL: host only
    int device;
};
