// derive_host.cpp — csrc/derive.h (the kept slice of a value, the HOST mode of pwaf_derive_batch and the three scan phases as loops over
// tiles) as a stand-alone program for the sanitizers: tests/test_derive_batch_cpu.py builds it with g++ -fsanitize=address,undefined and
// runs it.
//
//   derive_host < requests
//
// Every input line is one request: `<present bits> <Host header hex or -> <path hex or -> <User-Agent hex or -> <URI host hex or ->`.
// The program derives each request three ways. Alone: every value from a heap block of EXACTLY its bytes (a zero-byte block for an empty
// one), so a load in front of a value or behind it is the sanitizer's to report. As one batch in HOST mode (derive_host): arenas without
// slack whose offsets begin above 0, first with no room at all (cap 0: sizes only), then into blocks of exactly offsets[n] + 16 bytes. And
// as the device computes it: span_tile, base_column and copy_tile over a scratch block of exactly pwaf_derive_scratch_bytes(n), the tiles
// of phase 1 and 3 in descending order (no tile needs another one's result). The program checks that the three agree, byte for byte with
// pads, offsets and stats, and prints `<host hex> <path hex> <user agent hex>` per request for the test to compare with the oracle.
// Exit status 0 = ok.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../pingoo_amd/csrc/derive.h"

namespace D = pwaf::derive;
typedef std::vector<uint8_t> Bytes;

static Bytes unhex(const std::string &s) {
    Bytes v;
    if (s == "-") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return v;
}
static std::string hex(const uint8_t *p, size_t n) {
    static const char digits[] = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) s += digits[p[i] >> 4], s += digits[p[i] & 15];
    return s.empty() ? "-" : s;
}
static std::unique_ptr<uint8_t[]> exact(const Bytes &v) {
    std::unique_ptr<uint8_t[]> b(new uint8_t[v.size()]);  // size 0: a block no byte of which may be read
    if (!v.empty()) memcpy(b.get(), v.data(), v.size());
    return b;
}

struct Req {
    uint32_t present;
    Bytes raw[3], uri;  // Host header, path, User-Agent; the URI's host
};

// one arena without slack; its offsets begin at `first`
struct Arena {
    std::unique_ptr<uint8_t[]> data;
    std::unique_ptr<uint32_t[]> off;
    template <class Get>
    Arena(const std::vector<Req> &reqs, uint32_t first, Get get) {
        size_t bytes = first;
        for (const Req &r : reqs) bytes += get(r).size();
        data.reset(new uint8_t[bytes]);
        off.reset(new uint32_t[reqs.size() + 1]);
        memset(data.get(), 0xEE, first);
        off[0] = first;
        for (size_t i = 0; i < reqs.size(); i++) {
            const Bytes &v = get(reqs[i]);
            if (!v.empty()) memcpy(data.get() + off[i], v.data(), v.size());
            off[i + 1] = off[i] + (uint32_t)v.size();
        }
    }
    pwaf_strcol col() const { return pwaf_strcol{data.get(), off.get()}; }
};

// what one way of deriving the batch wrote
struct Result {
    std::unique_ptr<uint8_t[]> data[3];
    std::unique_ptr<uint32_t[]> off[3];
    pwaf_derive_stats stats;
    void attach(D::Args &a, uint32_t n, const uint64_t cap[3]) {
        for (uint32_t c = 0; c < 3; c++) {
            data[c].reset(new uint8_t[cap[c]]);
            off[c].reset(new uint32_t[n + 1]);
            memset(data[c].get(), 0x5A, cap[c]);
            a.data[c] = cap[c] ? data[c].get() : nullptr, a.off[c] = off[c].get(), a.cap[c] = cap[c];
        }
        memset(&stats, 0x5A, sizeof stats);
        a.stats = &stats;
    }
};

int main() {
    std::vector<Req> reqs;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned present;
        std::string h, p, u, uri;
        if (!(in >> present >> h >> p >> u >> uri)) continue;
        reqs.push_back(Req{present, {unhex(h), unhex(p), unhex(u)}, unhex(uri)});
    }
    const uint32_t n = (uint32_t)reqs.size();
    // alone
    std::vector<Bytes> alone[3];
    for (const Req &r : reqs) {
        auto h = exact(r.raw[0]), p = exact(r.raw[1]), u = exact(r.raw[2]), uri = exact(r.uri);
        const D::Span sp = D::path_span(p.get(), (uint32_t)r.raw[1].size());
        D::Span su{0, 0}, sh{0, 0};
        const uint8_t *hsrc = h.get();
        if (r.present & PWAF_RAW_HAS_USER_AGENT) su = D::header_span(u.get(), (uint32_t)r.raw[2].size());
        if (r.present & PWAF_RAW_HAS_URI_HOST) sh = D::uri_host_span(uri.get(), (uint32_t)r.uri.size()), hsrc = uri.get();
        else if (r.present & PWAF_RAW_HAS_HOST_HEADER) sh = D::header_span(h.get(), (uint32_t)r.raw[0].size());
        if (sp.start != 0 || sh.len > D::kMaxKept || su.len > D::kMaxKept) return 3;
        alone[0].push_back(Bytes(hsrc + sh.start, hsrc + sh.start + sh.len));
        alone[1].push_back(Bytes(p.get(), p.get() + sp.len));
        alone[2].push_back(Bytes(u.get() + su.start, u.get() + su.start + su.len));
    }
    // as a batch in HOST mode: exact arenas whose offsets begin above 0
    const Arena host(reqs, 5, [](const Req &r) -> const Bytes & { return r.raw[0]; }), path(reqs, 9, [](const Req &r) -> const Bytes & { return r.raw[1]; }),
        ua(reqs, 33, [](const Req &r) -> const Bytes & { return r.raw[2]; }), uri(reqs, 18, [](const Req &r) -> const Bytes & { return r.uri; });
    std::unique_ptr<uint8_t[]> present(new uint8_t[n]);
    for (uint32_t i = 0; i < n; i++) present[i] = (uint8_t)reqs[i].present;
    D::Args a{};
    a.raw[0] = host.col(), a.raw[1] = path.col(), a.raw[2] = ua.col(), a.uri_host = uri.col(), a.present = present.get(), a.n = n;
    uint32_t bad = 0, col = 0;
    const uint64_t none[3] = {0, 0, 0};
    Result sizes;
    sizes.attach(a, n, none);
    if (!D::derive_host(a, &bad, &col)) return 4;
    if (sizes.stats.n != n || sizes.stats.overflow != 7u) return 5;  // (no room for a pad: every column overflows)
    uint64_t cap[3];
    for (uint32_t c = 0; c < 3; c++) {
        cap[c] = sizes.stats.bytes[c] + PWAF_ARENA_PAD;
        if (sizes.off[c][0] != 0 || sizes.off[c][n] != sizes.stats.bytes[c]) return 6;
    }
    Result whole;
    whole.attach(a, n, cap);
    if (!D::derive_host(a, &bad, &col)) return 7;
    if (whole.stats.overflow != 0 || memcmp(whole.stats.bytes, sizes.stats.bytes, sizeof whole.stats.bytes) != 0) return 8;
    for (uint32_t c = 0; c < 3; c++) {
        if (memcmp(whole.off[c].get(), sizes.off[c].get(), 4 * ((size_t)n + 1)) != 0) return 9;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t o = whole.off[c][i], len = whole.off[c][i + 1] - o;
            if (len != alone[c][i].size() || (len && memcmp(whole.data[c].get() + o, alone[c][i].data(), len) != 0)) return 10;
        }
        for (uint32_t k = 0; k < PWAF_ARENA_PAD; k++)
            if (whole.data[c][whole.stats.bytes[c] + k] != 0) return 11;
    }
    // one byte short: the overflow bit, the offsets complete, nothing behind the block (the sanitizer's to report)
    {
        const uint64_t tight[3] = {cap[0] - 1, cap[1] - 1, cap[2] - 1};
        Result t;
        t.attach(a, n, tight);
        if (!D::derive_host(a, &bad, &col) || t.stats.overflow != 7u) return 12;
        for (uint32_t c = 0; c < 3; c++)
            if (memcmp(t.off[c].get(), whole.off[c].get(), 4 * ((size_t)n + 1)) != 0) return 13;
    }
    // as the device computes it: three phases over exact scratch, tiles in descending order
    for (int pass = 0; pass < 2; pass++) {
        const uint64_t tight[3] = {cap[0] - 1, cap[1] - 1, cap[2] - 1};
        Result ph;
        ph.attach(a, n, pass ? tight : cap);
        std::unique_ptr<uint8_t[]> scratch(new uint8_t[D::scratch_bytes(n)]);
        memset(scratch.get(), 0x5A, D::scratch_bytes(n));
        D::scratch_layout(a, scratch.get());
        const uint32_t nt = D::tiles(n);
        if ((size_t)((uint8_t *)(a.from + 2 * (size_t)n) - scratch.get()) > D::scratch_bytes(n) || a.tile_stride <= nt) return 14;
        for (uint32_t t = nt; t-- > 0;) D::span_tile(a, t);
        for (uint32_t c = 0; c < 3; c++) D::base_column(a, c);
        for (uint32_t t = nt ? nt : 1; t-- > 0;) D::copy_tile(a, t);
        if (ph.stats.n != n || ph.stats.overflow != (pass ? 7u : 0u) || memcmp(ph.stats.bytes, whole.stats.bytes, sizeof ph.stats.bytes) != 0) return 15;
        for (uint32_t c = 0; c < 3; c++) {
            if (memcmp(ph.off[c].get(), whole.off[c].get(), 4 * ((size_t)n + 1)) != 0) return 16;
            if (!pass && memcmp(ph.data[c].get(), whole.data[c].get(), cap[c]) != 0) return 17;
        }
    }
    // offsets that decrease in a column a request reads refuse the call before anything is written
    if (n) {
        Result r;
        r.attach(a, n, cap);
        const uint32_t keep = path.off[1];
        path.off[1] = path.off[0] - 1u;
        const bool ok = D::derive_host(a, &bad, &col);
        path.off[1] = keep;
        if (ok || bad != 0 || col != D::kPath) return 18;
        for (uint32_t c = 0; c < 3; c++)
            for (uint64_t b = 0; b < cap[c]; b++)
                if (r.data[c][b] != 0x5A) return 19;
        if (((const uint8_t *)&r.stats)[0] != 0x5A) return 20;
    }
    for (uint32_t i = 0; i < n; i++)
        std::printf("%s %s %s\n", hex(alone[0][i].data(), alone[0][i].size()).c_str(), hex(alone[1][i].data(), alone[1][i].size()).c_str(),
                    hex(alone[2][i].data(), alone[2][i].size()).c_str());
    return 0;
}
