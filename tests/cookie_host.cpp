// cookie_host.cpp — csrc/cookie.h (the HOST mode of pwaf_verify_cookies: verify_host; locate and judge, which pwaf_verify_cookie_one calls;
// key-set creation: build_base_table, build_key) as a stand-alone program for the sanitizers: tests/test_verify_cookies_cpu.py builds it with
// g++ -fsanitize=address,undefined and runs it.
//
//   cookie_host < script
//
// Every input line is one command (hex fields; `-` is the empty string, `~` no Cookie header at all):
//   K <kid> <x>                              a key of the set (before the first Q); prints nothing
//   X <x>                                    prints `X 1` when x is the canonical encoding of a point on the curve, else `X 0`
//   R <64 bytes>                             prints `R <32 bytes>`: the 512-bit little-endian number mod L
//   N <now>                                  decimal Unix seconds for the requests that follow it
//   Q <0|1> <ip, 32 digits> <ua> <host> <cookie>   one request
// The requests are answered twice. Alone: from heap blocks of EXACTLY the bytes each value owns. And as one batch: arenas without slack
// whose offsets begin above 0, once for every request with flags_out aliasing flags, once for a list with every request backwards, a
// duplicate and two out-of-range entries, into an output block of exactly the entries the call may write. A read outside a value or a
// write outside the output is the sanitizer's to report; the program checks that all ways agree and prints `Q <status>` per request for the
// test to compare with its oracle. Exit status 0 = ok.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../pingoo_amd/csrc/cookie.h"

namespace K = pwaf::cookie;
namespace C = pwaf::clientid;

static std::vector<uint8_t> unhex(const std::string &s) {
    std::vector<uint8_t> v;
    if (s == "-" || s == "~") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return v;
}
static std::unique_ptr<uint8_t[]> exact(const uint8_t *p, size_t n) {
    std::unique_ptr<uint8_t[]> b(new uint8_t[n]);  // n == 0: a block no byte of which may be read
    if (n) memcpy(b.get(), p, n);
    return b;
}

struct Req {
    uint8_t v6;
    std::vector<uint8_t> ip, ua, host, cookie;
    int64_t now;
};

int main() {
    std::unique_ptr<K::KeySetData> ks(new K::KeySetData());
    memset(ks.get(), 0, sizeof(K::KeySetData));
    if (!K::build_base_table(ks->base)) return 2;
    std::vector<Req> reqs;
    std::vector<std::string> printed;
    int64_t now = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "K") {
            std::string kid, x;
            in >> kid >> x;
            const std::vector<uint8_t> k = unhex(kid), xb = unhex(x);
            if (xb.size() != 32 || k.empty() || k.size() > K::kMaxKid || ks->n_keys >= K::kMaxKeys) return 3;
            auto xe = exact(xb.data(), 32);
            auto ke = exact(k.data(), k.size());
            if (!K::build_key(xe.get(), (const char *)ke.get(), (uint32_t)k.size(), &ks->keys[ks->n_keys])) return 4;
            ks->n_keys++;
        } else if (cmd == "X") {
            std::string x;
            in >> x;
            const std::vector<uint8_t> xb = unhex(x);
            if (xb.size() != 32) return 3;
            auto xe = exact(xb.data(), 32);
            std::unique_ptr<K::KeyEntry> e(new K::KeyEntry());
            std::printf("X %d\n", K::build_key(xe.get(), "k", 1, e.get()) ? 1 : 0);
        } else if (cmd == "R") {
            std::string x;
            in >> x;
            const std::vector<uint8_t> xb = unhex(x);
            if (xb.size() != 64) return 3;
            uint32_t w[16], out[8];
            memcpy(w, xb.data(), 64);
            K::scalar_reduce(w, out);
            std::printf("R ");
            for (int i = 0; i < 32; i++) std::printf("%02x", ((const uint8_t *)out)[i]);
            std::printf("\n");
        } else if (cmd == "N") {
            long long v;
            in >> v;
            now = v;
        } else if (cmd == "Q") {
            int v6;
            std::string ip, ua, host, cookie;
            if (!(in >> v6 >> ip >> ua >> host >> cookie)) return 3;
            reqs.push_back(Req{(uint8_t)v6, unhex(ip), unhex(ua), unhex(host), unhex(cookie), now});
            if (reqs.back().ip.size() != 16) return 3;
        }
    }
    const uint32_t n = (uint32_t)reqs.size();
    // alone (pwaf_verify_cookie_one's path)
    std::vector<uint8_t> alone;
    for (const Req &r : reqs) {
        auto ip = exact(r.ip.data(), r.v6 ? 16 : 4), ua = exact(r.ua.data(), r.ua.size()), host = exact(r.host.data(), r.host.size());
        auto cookie = exact(r.cookie.data(), r.cookie.size());
        K::Token t{0, 0, 0};
        uint8_t st = r.cookie.empty() ? (uint8_t)PWAF_COOKIE_ABSENT : K::locate(cookie.get(), (uint32_t)r.cookie.size(), &t);
        if (st == K::kCandidate) {
            uint32_t id[C::kIdWords];
            C::client_id_words(C::make_message(ip.get(), r.v6, ua.get(), (uint32_t)r.ua.size(), host.get(), (uint32_t)r.host.size()), id);
            st = K::judge(*ks, ks->base, cookie.get(), t, r.now, id);
        }
        alone.push_back(st);
    }
    // as a batch: one `now` per call, so the requests are grouped by theirs; exact arenas, offsets that begin above 0
    for (uint32_t lo = 0; lo < n;) {
        uint32_t hi = lo;
        while (hi < n && reqs[hi].now == reqs[lo].now) hi++;
        const uint32_t m = hi - lo, ua0 = 7, host0 = 21, ck0 = 3;
        size_t ua_bytes = ua0, host_bytes = host0, ck_bytes = ck0;
        for (uint32_t i = lo; i < hi; i++) ua_bytes += reqs[i].ua.size(), host_bytes += reqs[i].host.size(), ck_bytes += reqs[i].cookie.size();
        std::unique_ptr<uint8_t[]> ua(new uint8_t[ua_bytes]), host(new uint8_t[host_bytes]), ck(new uint8_t[ck_bytes]), ip(new uint8_t[16 * (size_t)m]), v6(new uint8_t[m]);
        std::unique_ptr<uint8_t[]> flags(new uint8_t[m]);
        std::unique_ptr<uint32_t[]> uo(new uint32_t[m + 1]), ho(new uint32_t[m + 1]), co(new uint32_t[m + 1]);
        memset(ua.get(), 0xEE, ua0), memset(host.get(), 0xEE, host0), memset(ck.get(), 0xEE, ck0);
        uo[0] = ua0, ho[0] = host0, co[0] = ck0;
        for (uint32_t j = 0; j < m; j++) {
            const Req &r = reqs[lo + j];
            if (!r.ua.empty()) memcpy(ua.get() + uo[j], r.ua.data(), r.ua.size());
            if (!r.host.empty()) memcpy(host.get() + ho[j], r.host.data(), r.host.size());
            if (!r.cookie.empty()) memcpy(ck.get() + co[j], r.cookie.data(), r.cookie.size());
            uo[j + 1] = uo[j] + (uint32_t)r.ua.size(), ho[j + 1] = ho[j] + (uint32_t)r.host.size(), co[j + 1] = co[j] + (uint32_t)r.cookie.size();
            memcpy(ip.get() + 16 * (size_t)j, r.ip.data(), 16);
            v6[j] = r.v6;
            flags[j] = (uint8_t)(0xA0u | (j & 1u));
        }
        K::Args a{};
        a.ks = ks.get(), a.now = reqs[lo].now;
        a.cookies = pwaf_strcol{ck.get(), co.get()}, a.ua = pwaf_strcol{ua.get(), uo.get()}, a.host = pwaf_strcol{host.get(), ho.get()};
        a.ip = ip.get(), a.ip_is_v6 = v6.get(), a.flags = flags.get(), a.n = m;
        uint32_t bad = 0;
        {  // every request (idx NULL), flags_out aliasing flags
            std::unique_ptr<uint8_t[]> out(new uint8_t[m]);
            a.status = out.get(), a.flags_out = flags.get();
            if (!K::verify_host(a, &bad)) return 5;
            for (uint32_t j = 0; j < m; j++) {
                if (out[j] != alone[lo + j]) return 6;
                if (flags[j] != (uint8_t)(0xA0u | (out[j] == PWAF_COOKIE_VERIFIED ? 1u : 0u))) return 7;
            }
        }
        {  // a list: every request backwards, a duplicate, two entries that name no request; the length word cuts the last entry off
            std::vector<uint32_t> idx;
            for (uint32_t j = m; j-- > 0;) idx.push_back(j);
            idx.push_back(0), idx.push_back(m), idx.push_back(0xFFFFFFFFu), idx.push_back(0);
            const uint32_t k = (uint32_t)idx.size() - 1;
            std::unique_ptr<uint32_t[]> list(new uint32_t[idx.size()]);
            memcpy(list.get(), idx.data(), 4 * idx.size());
            std::unique_ptr<uint8_t[]> out(new uint8_t[k]);  // exactly the k entries the call may write
            const uint8_t before = flags[0];
            a.idx = list.get(), a.idx_cap = (uint32_t)idx.size(), a.n_idx = &k, a.status = out.get();
            if (!K::verify_host(a, &bad)) return 8;
            for (uint32_t j = 0; j < k; j++)
                if (out[j] != (idx[j] < m ? alone[lo + idx[j]] : (uint8_t)PWAF_COOKIE_ABSENT)) return 9;
            if (flags[0] != before) return 10;  // flags_out is written only when idx == NULL
            // offsets that decrease for a selected request refuse the call before anything is written
            const uint32_t keep = co[1];
            co[1] = co[0] - 1u;
            memset(out.get(), 0x5A, k);
            const bool ok = K::verify_host(a, &bad);
            co[1] = keep;
            if (ok || bad != m - 1) return 11;  // (request 0 is entry m - 1 of the backwards list)
            for (uint32_t j = 0; j < k; j++)
                if (out[j] != 0x5A) return 12;
        }
        lo = hi;
    }
    for (uint8_t st : alone) std::printf("Q %u\n", (unsigned)st);
    return 0;
}
