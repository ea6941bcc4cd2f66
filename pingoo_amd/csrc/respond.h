// respond.h — which response a request gets (include/pwaf.h: pwaf_respond, pwaf_respond_one): the control flow of the reference's listener
// behind its derivations (http_listener.rs:196-272) and the dispatch of serve_captcha_request (pingoo/captcha.rs:158-174), from what the
// earlier services wrote: the verdict, the verified-cookie status, the route and the path. DESIGN.md §5.1.9 states the table.
//
// One header, compiled three ways, like powbody.h: by respond.hip for the device (respond_classify_kernel, respond_base_kernel,
// respond_scatter_kernel), by the same unit for the HOST mode and pwaf_respond_one (respond_host and decide below) and by
// tools/respond_host.cpp (g++ under the sanitizers). No HIP include.
//
// The decision table is ONE function, decide, templated on where the path's bytes come from: Padded issues 16-byte loads at the path's
// own alignment and may pass the path's end by fewer than 16 bytes (the arena or its PWAF_ARENA_PAD), Exact reads the path's bytes and
// no other. Only a request whose action is BYPASS has its path looked at.
//
// The lists are reduce-then-scan over tiles of kTile requests, the scheme of derive.h and powbody.h with a bit per request where those
// have a length: phase 1 decides, stores the response and counts each list's members per tile, phase 2 makes exclusive bases of the
// tiles' counts, phase 3 re-reads the kinds and stores each member's index at base + rank. Ranks follow the request order, so every
// list is ascending.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "pwaf.h"
#include "service.h"

namespace pwaf {
namespace respond {

static constexpr uint32_t kTile = 256;   // requests per tile of the scan; lanes of a workgroup of the classify and scatter launches
static constexpr uint32_t kStep = 1024;  // lanes of the base launch: tiles per step
static constexpr uint32_t kCountWords = 16;  // scratch words in front of the tile arrays: PWAF_RESP_KINDS counters, then zero
static_assert(sizeof(pwaf_response) == 8 && sizeof(pwaf_verdict) == 8, "one 8-byte load, one 8-byte store");
static_assert(PWAF_RESP_KINDS <= kCountWords && PWAF_RESP_KINDS <= 32, "a kind is a bit of a list's mask");

// ---- the path of a captcha endpoint (captcha.rs:165-173) -----------------------------------------------------------------------------------
// eight bytes of a literal as they lie in memory on a little-endian machine, byte k in bits [8k, 8k + 8)
constexpr uint64_t word_of(const char *s, uint32_t from, uint32_t len) {
    uint64_t w = 0;
    for (uint32_t k = 0; k < 8 && from + k < len; k++) w |= (uint64_t)(uint8_t)s[from + k] << (8u * k);
    return w;
}
static constexpr char kAssets[] = "/__pingoo/captcha/assets";      // starts with
static constexpr char kInit[] = "/__pingoo/captcha/api/init";      // equals
static constexpr char kVerify[] = "/__pingoo/captcha/api/verify";  // equals: the longest, 28 bytes
static constexpr uint32_t kAssetsLen = sizeof(kAssets) - 1, kInitLen = sizeof(kInit) - 1, kVerifyLen = sizeof(kVerify) - 1;
static_assert(kAssetsLen == 24 && kInitLen == 26 && kVerifyLen == 28, "two 16-byte loads hold every literal");
static constexpr uint64_t kHead0 = word_of(kVerify, 0, kVerifyLen), kHead1 = word_of(kVerify, 8, kVerifyLen);  // "/__pingoo/captch": shared by the three
static constexpr uint64_t kAssets2 = word_of(kAssets, 16, kAssetsLen);
static constexpr uint64_t kInit2 = word_of(kInit, 16, kInitLen), kInit3 = word_of(kInit, 24, kInitLen);
static constexpr uint64_t kVerify2 = word_of(kVerify, 16, kVerifyLen), kVerify3 = word_of(kVerify, 24, kVerifyLen);
static_assert(kHead0 == word_of(kAssets, 0, kAssetsLen) && kHead1 == word_of(kInit, 8, kInitLen), "one head for the three literals");

struct Head {  // the first 32 bytes of a path of at least kAssetsLen bytes; what lies at or behind its end is whatever the source gave
    uint64_t w[4];
};
struct Padded {  // DEVICE: two 16-byte loads at the path's own alignment; they pass the path's end by at most 32 - kAssetsLen = 8 bytes
    const uint8_t *s;
    PWAF_SVC_HD Head load(uint32_t len) const {
        (void)len;
        Head h;
        memcpy(&h, s, 32);
        return h;
    }
};
struct Exact {  // HOST: not a byte outside the path
    const uint8_t *s;
    PWAF_SVC_HD Head load(uint32_t len) const {
        Head h{{0, 0, 0, 0}};
        memcpy(&h, s, len < 32u ? len : 32u);
        return h;
    }
};
// serve_captcha_request's dispatch. A path shorter than the shortest literal is not read at all; the lengths decide "equals" against
// "starts with", so bytes behind the path's end never count
template <class Src>
PWAF_SVC_HD uint32_t endpoint_kind(const Src &src, uint32_t len) {
    if (len < kAssetsLen) return PWAF_RESP_CAPTCHA_NOT_FOUND;
    const Head h = src.load(len);
    // (no branch between the loads and the last comparison: the two loads are issued together, not one behind a comparison of the other)
    const bool head = (h.w[0] == kHead0) & (h.w[1] == kHead1);
    const bool assets = h.w[2] == kAssets2;
    const bool init = (len == kInitLen) & (h.w[2] == kInit2) & ((h.w[3] & 0xFFFFull) == kInit3);
    const bool verify = (len == kVerifyLen) & (h.w[2] == kVerify2) & ((h.w[3] & 0xFFFFFFFFull) == kVerify3);
    const uint32_t under = assets ? PWAF_RESP_CAPTCHA_ASSET : init ? PWAF_RESP_CAPTCHA_INIT : verify ? PWAF_RESP_CAPTCHA_VERIFY : PWAF_RESP_CAPTCHA_NOT_FOUND;
    return head ? under : PWAF_RESP_CAPTCHA_NOT_FOUND;
}

// ---- the decision ------------------------------------------------------------------------------------------------------------------------
struct Decision {
    uint32_t kind, arg;
};
// the first row that applies decides. has_route false: no route column was given.
template <class Src>
PWAF_SVC_HD Decision decide(uint32_t action, uint32_t rule_idx, uint32_t status, bool has_route, uint32_t route, const Src &path, uint32_t path_len) {
    if (rule_idx == PWAF_RULE_UA_GATE) return {PWAF_RESP_BLOCKED, PWAF_RULE_UA_GATE};                                     // 1  :196-198
    if (action == PWAF_ACTION_BYPASS) return {endpoint_kind(path, path_len), PWAF_RULE_CAPTCHA_ENDPOINT};                 // 2  :200-204
    if (status == PWAF_COOKIE_INVALID) return {PWAF_RESP_CAPTCHA_PAGE, PWAF_RULE_COOKIE};                                 // 3  :233-235
    if (status == PWAF_COOKIE_UNDECIDED) return {PWAF_RESP_HOST_DECIDES, rule_idx};                                       // 4
    if (action == PWAF_ACTION_BLOCK) return {PWAF_RESP_BLOCKED, rule_idx};                                                // 5  :255
    if (action == PWAF_ACTION_CAPTCHA) return {PWAF_RESP_CAPTCHA_PAGE, rule_idx};                                         //    :258
    if (!has_route) return {PWAF_RESP_FORWARD, PWAF_ROUTE_NONE};                                                          // 6
    return {route == PWAF_ROUTE_NONE ? PWAF_RESP_NOT_FOUND : PWAF_RESP_FORWARD, route};                                   //    :266-272
}

// ---- the batch ---------------------------------------------------------------------------------------------------------------------------
// The kernels' arguments and respond_host's (pwaf_respond after its argument checks).
struct Args {
    pwaf_strcol path;
    uint32_t n;
    uint32_t n_lists;
    const pwaf_verdict *verdicts;
    const uint8_t *status;  // nullable: every request ABSENT
    const uint32_t *route;  // nullable
    pwaf_response *out;
    uint64_t *counts;  // nullable
    uint32_t kinds[PWAF_RESP_MAX_LISTS];
    uint32_t cap[PWAF_RESP_MAX_LISTS];
    uint32_t *idx[PWAF_RESP_MAX_LISTS];
    uint32_t *cnt[PWAF_RESP_MAX_LISTS];
    uint32_t *kcount;  // scratch: kCountWords words, zeroed by the memset; [k] the requests of kind k
    uint64_t *tile;    // scratch: n_lists arrays of tile_stride(n) words: a list's members per tile, then exclusive bases
};
// a verdict or a response as ONE 8-byte access at the structures' own alignment (the action / the kind is the first word's low byte)
typedef uint32_t Word2 __attribute__((vector_size(8), aligned(4), may_alias));
PWAF_SVC_HD bool member(uint32_t kinds, uint32_t kind) { return ((kinds >> kind) & 1u) != 0; }  // kind < PWAF_RESP_KINDS
// request i < n: decided and stored
template <class Src>
PWAF_SVC_HD uint32_t respond_request(const Args &a, uint32_t i) {
    const Word2 v = *reinterpret_cast<const Word2 *>(a.verdicts + i);
    const uint32_t action = v[0] & 0xFFu, rule_idx = v[1];
    uint32_t o = 0, len = 0;
    if (action == PWAF_ACTION_BYPASS) o = a.path.offsets[i], len = a.path.offsets[(size_t)i + 1] - o;
    const Decision d = decide(action, rule_idx, a.status ? a.status[i] : PWAF_COOKIE_ABSENT, a.route != nullptr, a.route ? a.route[i] : PWAF_ROUTE_NONE, Src{a.path.data + o}, len);
    *reinterpret_cast<Word2 *>(a.out + i) = Word2{d.kind, d.arg};  // (kind < 256: the pad bytes are 0)
    return d.kind;
}

// ---- the scan's arithmetic -----------------------------------------------------------------------------------------------------------------
PWAF_SVC_HD uint32_t tiles(uint32_t n) { return pwaf::tiles(n, kTile); }
PWAF_SVC_HD uint32_t tile_stride(uint32_t n) { return pwaf::tile_stride(tiles(n)); }
// scratch: the kind counters, then PWAF_RESP_MAX_LISTS tile arrays
PWAF_SVC_HD size_t scratch_bytes(uint32_t n) { return (size_t)kCountWords * 4u + (size_t)PWAF_RESP_MAX_LISTS * tile_stride(n) * 8u; }
inline void scratch_layout(Args &a, void *scratch) {
    a.kcount = (uint32_t *)scratch;
    a.tile = (uint64_t *)(a.kcount + kCountWords);
}

// ---- the HOST mode -------------------------------------------------------------------------------------------------------------------------
// First every request is checked (false with *bad = the request and *why = 0 an action above 3, 1 a status above 3, 2 path offsets that
// decrease; nothing written), then responses, lists and counts are written in request order.
inline bool respond_host(const Args &a, uint32_t *bad, uint32_t *why) {
    for (uint32_t i = 0; i < a.n; i++) {
        const uint32_t w = a.verdicts[i].action > 3u ? 0u : a.status && a.status[i] > 3u ? 1u : a.path.offsets[(size_t)i + 1] < a.path.offsets[i] ? 2u : 3u;
        if (w != 3u) {
            *bad = i, *why = w;
            return false;
        }
    }
    uint64_t kcount[PWAF_RESP_KINDS] = {};
    uint32_t members[PWAF_RESP_MAX_LISTS] = {};
    for (uint32_t i = 0; i < a.n; i++) {
        const uint32_t kind = respond_request<Exact>(a, i);
        kcount[kind]++;
        for (uint32_t l = 0; l < a.n_lists; l++) {
            if (!member(a.kinds[l], kind)) continue;
            if (members[l] < a.cap[l]) a.idx[l][members[l]] = i;
            members[l]++;
        }
    }
    for (uint32_t l = 0; l < a.n_lists; l++) *a.cnt[l] = members[l];
    if (a.counts) memcpy(a.counts, kcount, sizeof kcount);
    return true;
}

int launch_respond(const Args &a, void *stream);  // respond.hip: the memset and the three launches

}  // namespace respond
}  // namespace pwaf
