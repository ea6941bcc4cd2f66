// pow.h — the check of a captcha proof-of-work submission (include/pwaf.h: pwaf_verify_pow, pwaf_verify_pow_one): what
// CaptchaManager::api_verify (pingoo/captcha.rs:241-333) does between finding the `__pingoo_captcha` cookie and issuing the verified
// cookie — jwt::parse_header, the key by `kid`, jwt::parse_and_verify into CaptchaCookieJwtClaims (captcha.rs:61-67; jwt/jwt.rs:89-124,
// :198-327), sub == client id, the leading zeroes of the hash, hash == SHA-256(challenge || nonce). DESIGN.md §5.1.7 states the semantics;
// this header is their only implementation.
//
// One header, compiled three ways, like cookie.h, on which it rests: by pow.hip for the device (pow_check_kernel: one entry per lane;
// pow_verify_kernel: one candidate per lane), by the same unit for the host (the HOST mode and pwaf_verify_pow_one) and by
// tests/pow_host.cpp (g++ under the sanitizers). The cookie scan, the token split, base64url, the flat JSON reader, Ed25519 and the key
// set are cookie.h's; SHA-256 and the client id are clientid.h's. What is here: the claims of the challenge token with the one escape they
// need, the proof-of-work message (a run that comes out of base64 text with the escape decoded, then the nonce in its arena) as SHA-256
// blocks, the cheap checks, and the split into "decided without the curve" and "a candidate for the signature stage".
//
// The order is the opposite of the reference's, which verifies first: every failure of api_verify is the same response, so an entry that
// fails a cheap check is FAILED whatever its signature says, and only entries that passed every cheap check (or that this code does not
// parse) reach signature_ok. Nothing a lane keeps is indexed at run time: the block's words have literal indices after unrolling.
#pragma once
#include "cookie.h"

namespace pwaf {
namespace pow {

using cookie::B64;
using cookie::KeySetData;
using cookie::Precomp;
using cookie::Token;
using cookie::Value;
using cookie::kMaxKeys;

static constexpr uint8_t kCandidate = cookie::kCandidate;
static_assert(PWAF_POW_ABSENT == PWAF_COOKIE_ABSENT && PWAF_POW_FAILED == PWAF_COOKIE_INVALID, "locate_named's answers are this call's");

// ---- the cookie (captcha.rs:247-253) ---------------------------------------------------------------------------------------------------
// PWAF_POW_ABSENT, PWAF_POW_FAILED or kCandidate with *t
PWAF_SVC_HD uint8_t locate_pow(const uint8_t *v, uint32_t len, Token *t) {
    const char kName[] = "__pingoo_captcha";
    return cookie::locate_named(v, len, t, kName, sizeof kName - 1);
}

// ---- the proof of work (captcha.rs:311-333) --------------------------------------------------------------------------------------------
// hash[32] as 8 big-endian words: word 0 holds the first two hex digits in its top byte
PWAF_SVC_HD void hash_words(const uint8_t *hash, uint32_t hw[8]) {
    uint32_t raw[8];
    memcpy(raw, hash, 32);
    PWAF_CK_UNROLL
    for (uint32_t k = 0; k < 8; k++) hw[k] = __builtin_bswap32(raw[k]);
}
// the leading '0' characters of the hash's hex form: zero nibbles, the high nibble of byte 0 first
PWAF_SVC_HD uint32_t leading_zero_nibbles(const uint32_t hw[8]) {
    uint32_t zeros = 0;
    bool run = true;
    PWAF_CK_UNROLL
    for (uint32_t k = 0; k < 8; k++)
        if (run) {
            if (hw[k] == 0) {
                zeros += 8u;
            } else {
                zeros += (uint32_t)__builtin_clz(hw[k]) >> 2;
                run = false;
            }
        }
    return zeros;
}
// The message challenge || nonce as a source of bytes: the challenge is a string value of the claims (read through the base64 text, a
// backslash standing for \u0000), the nonce a value in its arena, read byte by byte (no load passes its end, on the device either).
struct Work {
    B64 claims;
    uint32_t q, q_end;  // the challenge's text still to read
    const uint8_t *nonce;
    uint32_t nonce_at, nonce_len;
};
PWAF_SVC_HD uint32_t work_byte(Work &w) {  // called total_bytes times at most
    if (w.q < w.q_end) return cookie::escape_aware_byte(w.claims, &w.q);
    return w.nonce[w.nonce_at++];
}
// SHA-256(challenge || nonce) == hash?  `challenge`: a kString value that parse_flat_as<true> accepted
PWAF_SVC_HD bool work_matches(const B64 &claims, const Value &challenge, const uint8_t *nonce, uint32_t nonce_len, const uint32_t hw[8]) {
    uint32_t decoded = 0;
    for (uint32_t q = challenge.at; q < challenge.at + challenge.len; decoded++) (void)cookie::escape_aware_byte(claims, &q);
    Work w{claims, challenge.at, challenge.at + challenge.len, nonce, 0, nonce_len};
    const uint64_t total = (uint64_t)decoded + nonce_len;
    const uint64_t blocks = (total + 9u + 63u) >> 6;  // the 0x80 byte and the 8-byte length ride in the last one
    uint32_t state[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    uint64_t pos = 0;
    for (uint64_t b = 0; b < blocks; b++) {
        uint32_t blk[16];
        PWAF_CK_UNROLL
        for (uint32_t t = 0; t < 16; t++) {  // (unrolled: blk[] keeps literal indices; the four bytes of a word are a loop)
            uint32_t x = 0;
            for (uint32_t k = 0; k < 4; k++, pos++) {
                const uint32_t byte = pos < total ? work_byte(w) : pos == total ? 0x80u : 0u;
                x = x << 8 | byte;
            }
            blk[t] = x;
        }
        if (b + 1 == blocks) {
            const uint64_t bits = total * 8u;
            blk[14] = (uint32_t)(bits >> 32);
            blk[15] = (uint32_t)bits;
        }
        clientid::compress(state, blk);
    }
    uint32_t diff = 0;
    PWAF_CK_UNROLL
    for (uint32_t k = 0; k < 8; k++) diff |= state[k] ^ hw[k];
    return diff == 0;
}
// the decoded bytes of a string value are exactly the 44 bytes of the client id (43 characters and the NUL: the reference's string)
PWAF_SVC_HD bool is_client_id(const B64 &claims, const Value &sub, const uint32_t id[clientid::kIdWords]) {
    uint32_t q = sub.at, count = 0, diff = 0;
    const uint32_t end = sub.at + sub.len;
    PWAF_CK_UNROLL
    for (uint32_t j = 0; j < clientid::kIdWords; j++) {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; k++)
            if (q < end) w |= cookie::escape_aware_byte(claims, &q) << (8u * k), count++;
        diff |= w ^ id[j];
    }
    return diff == 0 && count == 4u * clientid::kIdWords && q == end;
}

// ---- the decision ------------------------------------------------------------------------------------------------------------------------
struct Request {  // what one submission is checked against
    const uint8_t *ip16;
    uint8_t ip_is_v6;
    const uint8_t *ua, *host, *hash, *nonce;
    uint32_t ua_len, host_len, nonce_len;
};
struct Stage {  // what the signature stage is asked: under key `key` (kMaxKeys: under every key of the set) a good signature yields `good`
    uint32_t key, good;
};
// Rules 3 to 5 for a located token (`v` is the cookie value): PWAF_POW_FAILED, or kCandidate with *stage
PWAF_SVC_HD uint8_t check(const KeySetData &ks, const uint8_t *v, const Token &t, int64_t now, const Request &r, Stage *stage) {
    const uint8_t *m = v + t.at;
    uint32_t key = kMaxKeys;
    bool alg_typ_ok = false;
    *stage = Stage{kMaxKeys, PWAF_POW_UNDECIDED};
    if (t.signed_len() > cookie::kMaxSigned || !cookie::read_header(ks, m, t.hdr_len, &key, &alg_typ_ok)) return kCandidate;  // a header this code does not parse
    if (key >= kMaxKeys || !alg_typ_ok) return PWAF_POW_FAILED;  // captcha.rs:256-272; jwt.rs:208, :240
    stage->key = key;
    B64 s;
    if (!cookie::b64_open(m + t.hdr_len + 1, t.claims_len, &s)) return kCandidate;
    const cookie::Names names = {{"challenge", "difficulty", "iss", "sub", "aud", "exp", "nbf", "iat", "jti"}, 9};
    Value c[cookie::kMaxNames];
    if (!cookie::parse_flat_as<true>(s, names, c)) return kCandidate;
    if ((c[7].kind != cookie::kAbsent && c[7].kind != cookie::kInt) || !cookie::string_or_absent(c[8])) return kCandidate;  // serde refuses these; the host says so
    const int64_t kMin = (int64_t)0x8000000000000000ull, kMax = 0x7FFFFFFFFFFFFFFFll;
    const int64_t earliest = now < kMin + 5 ? kMin : now - 5, latest = now > kMax - 5 ? kMax : now + 5;  // JWT_VALDIATION_OPTIONS: 5 s of drift
    bool ok = c[5].kind == cookie::kInt && c[5].num >= earliest;                                           // jwt.rs:258-271
    ok &= c[6].kind == cookie::kInt && c[6].num <= latest;                                                 // jwt.rs:273-286
    ok &= c[4].kind == cookie::kString && cookie::text_is(s, c[4].at, c[4].len, "pingoo");                 // jwt.rs:288-301
    ok &= c[2].kind == cookie::kString && cookie::text_is(s, c[2].at, c[2].len, "pingoo");                 // jwt.rs:303-316
    ok &= c[0].kind == cookie::kString && c[3].kind == cookie::kString;                                    // captcha.rs:62; :299-309
    ok &= c[1].kind == cookie::kInt && c[1].num >= 0 && c[1].num <= 255;                                   // captcha.rs:63: a u8
    if (!ok) return PWAF_POW_FAILED;
    uint32_t hw[8];
    hash_words(r.hash, hw);
    if (leading_zero_nibbles(hw) < (uint32_t)c[1].num) return PWAF_POW_FAILED;  // captcha.rs:311-321
    if (!work_matches(s, c[0], r.nonce, r.nonce_len, hw)) return PWAF_POW_FAILED;  // captcha.rs:323-333
    uint32_t id[clientid::kIdWords];
    clientid::client_id_words(clientid::make_message(r.ip16, r.ip_is_v6, r.ua, r.ua_len, r.host, r.host_len), id);
    if (!is_client_id(s, c[3], id)) return PWAF_POW_FAILED;  // captcha.rs:299-309
    stage->good = PWAF_POW_PASSED;
    return kCandidate;
}
// Rules 3, 4 and 6 where they need the curve: stage.good behind a good signature, PWAF_POW_FAILED behind a bad one
PWAF_SVC_HD uint8_t verify(const KeySetData &ks, const Precomp *base, const uint8_t *v, const Token &t, const Stage &stage) {
    const uint8_t *m = v + t.at;
    const uint32_t len = t.signed_len();
    uint32_t r[8], s[8];
    if (!cookie::decode_signature(m + len + 1, cookie::kSigChars, r, s)) return PWAF_POW_FAILED;  // (locate_pow() saw to it)
    if (stage.key < kMaxKeys) return cookie::signature_ok(base, ks.keys[stage.key], r, s, m, len) ? (uint8_t)stage.good : (uint8_t)PWAF_POW_FAILED;
    for (uint32_t k = 0; k < ks.n_keys && k < kMaxKeys; k++)
        if (cookie::signature_ok(base, ks.keys[k], r, s, m, len)) return (uint8_t)stage.good;
    return PWAF_POW_FAILED;
}
// one submission on the host; *handed (nullable) is incremented when the signature stage was asked
inline uint8_t decide(const KeySetData &ks, const uint8_t *cookie_value, uint32_t cookie_len, int64_t now, const Request &r, uint32_t *handed) {
    Token t{0, 0, 0};
    uint8_t st = cookie_len ? locate_pow(cookie_value, cookie_len, &t) : (uint8_t)PWAF_POW_ABSENT;
    if (st != kCandidate) return st;
    Stage stage;
    st = check(ks, cookie_value, t, now, r, &stage);
    if (st != kCandidate) return st;
    if (handed) ++*handed;
    return verify(ks, ks.base, cookie_value, t, stage);
}

// ---- the batch call ------------------------------------------------------------------------------------------------------------------------
struct Candidate {  // 24 bytes: what pow_check_kernel hands pow_verify_kernel
    uint32_t entry, at, hdr_len, claims_len, key, good;
};
struct Args {
    const KeySetData *ks;  // where the batch lives
    pwaf_strcol cookies, nonce, ua, host;
    const uint8_t *ip, *ip_is_v6, *hash;  // hash: 32 bytes per request
    uint32_t n;
    int64_t now;
    const uint32_t *idx;    // NULL: every request, status[i] belongs to request i
    const uint32_t *n_idx;  // nullable: min(*n_idx, idx_cap) entries are looked at
    uint32_t idx_cap;
    uint8_t *status;
    uint32_t *count;  // DEVICE mode: the candidates' number (zeroed in front of the launches; scratch word 0) and the list
    Candidate *cand;
};
PWAF_SVC_HD uint32_t selected(const Args &a) { return pwaf::selected(a.idx, a.n_idx, a.idx_cap, a.n); }
PWAF_SVC_HD uint32_t request_of(const Args &a, uint32_t e) { return pwaf::request_of(a.idx, e); }
PWAF_SVC_HD Request request_at(const Args &a, uint32_t i) {  // i < a.n
    const uint32_t u0 = a.ua.offsets[i], h0 = a.host.offsets[i], n0 = a.nonce.offsets[i];
    return Request{a.ip + (size_t)i * 16, a.ip_is_v6[i], a.ua.data + u0, a.host.data + h0, a.hash + (size_t)i * 32, a.nonce.data + n0,
                   a.ua.offsets[i + 1] - u0,    a.host.offsets[i + 1] - h0, a.nonce.offsets[i + 1] - n0};
}
// entry e's first step (rules 1 to 5): ABSENT / FAILED, or kCandidate with *c
PWAF_SVC_HD uint8_t check_entry(const Args &a, uint32_t e, Candidate *c) {
    const uint32_t i = request_of(a, e);
    if (i >= a.n) return PWAF_POW_ABSENT;
    const uint32_t c0 = a.cookies.offsets[i];
    const uint8_t *v = a.cookies.data + c0;
    Token t{0, 0, 0};
    uint8_t st = locate_pow(v, a.cookies.offsets[i + 1] - c0, &t);
    if (st != kCandidate) return st;
    Stage stage;
    st = check(*a.ks, v, t, a.now, request_at(a, i), &stage);
    *c = Candidate{e, t.at, t.hdr_len, t.claims_len, stage.key, stage.good};
    return st;
}
PWAF_SVC_HD uint8_t verify_candidate(const Args &a, const Precomp *base, const Candidate &c) {
    const uint32_t i = request_of(a, c.entry);
    return verify(*a.ks, base, a.cookies.data + a.cookies.offsets[i], Token{c.at, c.hdr_len, c.claims_len}, Stage{c.key, c.good});
}

// The HOST mode: first every selected request is checked (offsets that decrease in a column: false with *bad = the entry, nothing
// written), then the answers are written in entry order. *handed (nullable): how many entries reached the signature stage.
inline bool verify_host(const Args &a, uint32_t *bad, uint32_t *handed) {
    const uint32_t m = selected(a);
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t i = request_of(a, j);
        if (i >= a.n) continue;
        if (a.cookies.offsets[i + 1] < a.cookies.offsets[i] || a.nonce.offsets[i + 1] < a.nonce.offsets[i] || a.ua.offsets[i + 1] < a.ua.offsets[i] ||
            a.host.offsets[i + 1] < a.host.offsets[i]) {
            *bad = j;
            return false;
        }
    }
    for (uint32_t j = 0; j < m; j++) {
        Candidate c{0, 0, 0, 0, 0, 0};
        uint8_t st = check_entry(a, j, &c);
        if (st == kCandidate) {
            if (handed) ++*handed;
            st = verify_candidate(a, a.ks->base, c);
        }
        a.status[j] = st;
    }
    return true;
}
int launch_verify_pow(const Args &a, void *stream);

}  // namespace pow
}  // namespace pwaf
