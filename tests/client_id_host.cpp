// client_id_host.cpp — csrc/clientid.h (the HOST mode of pwaf_client_ids: ids_host, and client_id_words, which pwaf_client_id_one calls) as a
// stand-alone program for the sanitizers: tests/test_client_ids_cpu.py builds it with g++ -fsanitize=address,undefined and runs it.
//
//   client_id_host < requests
//
// Every input line is one request: `<0|1> <ip hex, 32 digits> <user agent hex or -> <host hex or ->`. The program hashes each request
// twice. Alone: from heap blocks of EXACTLY the bytes the message owns (4 bytes of ip for IPv4, the value's length for the two strings, a
// zero-byte block for an empty one). And as one batch: arenas without slack whose offsets begin above 0, a list with every request, a
// duplicate and two out-of-range entries, into an output block of exactly the entries the call may write. A read outside a value or a write
// outside the output is the sanitizer's to report; the program checks that both ways agree and prints the ids, one per line, for the test
// to compare with hashlib. Exit status 0 = ok.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../pingoo_amd/csrc/clientid.h"

namespace K = pwaf::clientid;

static std::vector<uint8_t> unhex(const std::string &s) {
    std::vector<uint8_t> v;
    if (s == "-") return v;
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
    std::vector<uint8_t> ip, ua, host;
};

int main() {
    std::vector<Req> reqs;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int v6;
        std::string ip, ua, host;
        if (!(in >> v6 >> ip >> ua >> host)) continue;
        reqs.push_back(Req{(uint8_t)v6, unhex(ip), unhex(ua), unhex(host)});
        if (reqs.back().ip.size() != 16) return 2;
    }
    const uint32_t n = (uint32_t)reqs.size();
    // alone
    std::vector<std::string> alone;
    for (const Req &r : reqs) {
        const size_t ip_len = r.v6 ? 16 : 4;
        auto ip = exact(r.ip.data(), ip_len), ua = exact(r.ua.data(), r.ua.size()), host = exact(r.host.data(), r.host.size());
        uint32_t words[K::kIdWords];
        K::client_id_words(K::make_message(ip.get(), r.v6, ua.get(), (uint32_t)r.ua.size(), host.get(), (uint32_t)r.host.size()), words);
        char text[44];
        memcpy(text, words, 44);
        if (text[43] != 0 || strlen(text) != 43) return 3;
        alone.push_back(text);
    }
    // as a batch: exact arenas, offsets that begin above 0 (the bytes below them belong to no request)
    const uint32_t ua0 = 7, host0 = 21;
    size_t ua_bytes = ua0, host_bytes = host0;
    for (const Req &r : reqs) ua_bytes += r.ua.size(), host_bytes += r.host.size();
    std::unique_ptr<uint8_t[]> ua(new uint8_t[ua_bytes]), host(new uint8_t[host_bytes]), ip(new uint8_t[16 * (size_t)n]), v6(new uint8_t[n]);
    std::unique_ptr<uint32_t[]> uo(new uint32_t[n + 1]), ho(new uint32_t[n + 1]);
    memset(ua.get(), 0xEE, ua0), memset(host.get(), 0xEE, host0);
    uo[0] = ua0, ho[0] = host0;
    for (uint32_t i = 0; i < n; i++) {
        const Req &r = reqs[i];
        if (!r.ua.empty()) memcpy(ua.get() + uo[i], r.ua.data(), r.ua.size());
        if (!r.host.empty()) memcpy(host.get() + ho[i], r.host.data(), r.host.size());
        uo[i + 1] = uo[i] + (uint32_t)r.ua.size(), ho[i + 1] = ho[i] + (uint32_t)r.host.size();
        memcpy(ip.get() + 16 * (size_t)i, r.ip.data(), 16);
        v6[i] = r.v6;
    }
    K::Args a{};
    a.ua = pwaf_strcol{ua.get(), uo.get()}, a.host = pwaf_strcol{host.get(), ho.get()}, a.ip = ip.get(), a.ip_is_v6 = v6.get(), a.n = n;
    uint32_t bad = 0;
    {  // every request (idx NULL)
        std::unique_ptr<pwaf_client_id[]> out(new pwaf_client_id[n]);
        a.out = out.get();
        if (!K::ids_host(a, &bad)) return 4;
        for (uint32_t i = 0; i < n; i++)
            if (alone[i] != out[i].text) return 5;
    }
    if (n) {  // a list: every request backwards, a duplicate, two entries that name no request; the length word cuts the last entry off
        std::vector<uint32_t> idx;
        for (uint32_t i = n; i-- > 0;) idx.push_back(i);
        idx.push_back(0), idx.push_back(n), idx.push_back(0xFFFFFFFFu), idx.push_back(0);
        const uint32_t m = (uint32_t)idx.size() - 1;
        std::unique_ptr<uint32_t[]> list(new uint32_t[idx.size()]);
        memcpy(list.get(), idx.data(), 4 * idx.size());
        std::unique_ptr<pwaf_client_id[]> out(new pwaf_client_id[m]);  // exactly the m entries the call may write
        a.idx = list.get(), a.idx_cap = (uint32_t)idx.size(), a.n_idx = &m, a.out = out.get();
        if (!K::ids_host(a, &bad)) return 6;
        for (uint32_t j = 0; j < m; j++) {
            const char zeros[44] = {0};
            if (idx[j] < n ? alone[idx[j]] != out[j].text : memcmp(out[j].text, zeros, 44) != 0) return 7;
        }
        // offsets that decrease for a selected request refuse the call before anything is written
        const uint32_t keep = ho[1];
        ho[1] = ho[0] - 1u;
        memset(out.get(), 0x5A, 44 * (size_t)m);
        const bool ok = K::ids_host(a, &bad);
        ho[1] = keep;
        if (ok || bad != n - 1) return 8;  // (request 0 is entry n - 1 of the backwards list)
        for (size_t b = 0; b < 44 * (size_t)m; b++)
            if (((const uint8_t *)out.get())[b] != 0x5A) return 9;
    }
    for (const std::string &s : alone) std::printf("%s\n", s.c_str());
    return 0;
}
