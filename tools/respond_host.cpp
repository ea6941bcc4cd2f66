// respond_host.cpp — csrc/respond.h alone, as a stand-alone program for the sanitizers: the decision (decide over the Exact byte source, what
// pwaf_respond_one runs) and the HOST mode (respond_host, what pwaf_respond runs for PWAF_MEM_HOST) over paths that lie flush against the
// end of their allocation, so that one byte read outside a path is a report. No HIP, no library.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include tools/respond_host.cpp -o respond_host
// stdin: one request a line, "<action> <rule_idx> <status> <route or -> <path as hexadecimal digits or ->" ("-" for the route: no route
// column; every line of one run agrees on that). stdout: per request "R <kind> <arg>", what decide answers for the path in a heap block of
// exactly its size; then the HOST mode runs over all of them with the path arena, the outputs and every list in blocks of exactly their
// size — four lists (every kind, none, the captcha endpoints, BLOCKED) with caps of count, count - 1, 0 and count + 1 — and must agree with
// the decisions entry by entry; "H <n> <the nine counts>" reports the run. Exit status 0: everything agreed.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../pingoo_amd/csrc/respond.h"

namespace R = pwaf::respond;

static int fail(const char *what, size_t at) {
    fprintf(stderr, "respond_host: %s at %zu\n", what, at);
    return 1;
}

struct Line {
    uint32_t action, rule_idx, status, route;
    std::string path;
};

static int run_host(const std::vector<Line> &reqs, bool has_route, const std::vector<R::Decision> &want, uint64_t counts_out[PWAF_RESP_KINDS]) {
    const uint32_t n = (uint32_t)reqs.size();
    size_t bytes = 0;
    for (auto &r : reqs) bytes += r.path.size();
    uint8_t *arena = new uint8_t[bytes ? bytes : 1];  // no pad: the last path ends the block
    uint32_t *off = new uint32_t[n + 1];
    pwaf_verdict *verdicts = new pwaf_verdict[n ? n : 1];
    uint8_t *status = new uint8_t[n ? n : 1];
    uint32_t *route = new uint32_t[n ? n : 1];
    pwaf_response *out = new pwaf_response[n ? n : 1];
    off[0] = 0;
    for (uint32_t i = 0; i < n; i++) {
        memcpy(arena + off[i], reqs[i].path.data(), reqs[i].path.size());
        off[i + 1] = off[i] + (uint32_t)reqs[i].path.size();
        verdicts[i] = pwaf_verdict{(uint8_t)reqs[i].action, {0, 0, 0}, reqs[i].rule_idx};
        status[i] = (uint8_t)reqs[i].status, route[i] = reqs[i].route;
    }
    const uint32_t masks[4] = {(1u << PWAF_RESP_KINDS) - 1u, 0u,
                               1u << PWAF_RESP_CAPTCHA_ASSET | 1u << PWAF_RESP_CAPTCHA_INIT | 1u << PWAF_RESP_CAPTCHA_VERIFY | 1u << PWAF_RESP_CAPTCHA_NOT_FOUND,
                               1u << PWAF_RESP_BLOCKED};
    std::vector<uint32_t> members[4];
    for (uint32_t l = 0; l < 4; l++)
        for (uint32_t i = 0; i < n; i++)
            if ((masks[l] >> want[i].kind) & 1u) members[l].push_back(i);
    R::Args a{};
    a.path = pwaf_strcol{arena, off}, a.n = n, a.n_lists = 4, a.verdicts = verdicts, a.status = status, a.route = has_route ? route : nullptr, a.out = out;
    uint64_t *counts = new uint64_t[PWAF_RESP_KINDS];
    uint32_t cnt[4];
    a.counts = counts;
    for (uint32_t l = 0; l < 4; l++) {
        const uint32_t c = (uint32_t)members[l].size();
        a.kinds[l] = masks[l];
        a.cap[l] = l == 0 ? c : l == 1 ? (c ? c - 1u : 0u) : l == 2 ? 0u : c + 1u;
        a.idx[l] = a.cap[l] ? new uint32_t[a.cap[l]] : nullptr;  // exactly cap entries: a store at idx[cap] is a report
        a.cnt[l] = &cnt[l];
    }
    uint32_t bad = 0, why = 0;
    int rc = 0;
    if (!R::respond_host(a, &bad, &why)) rc = fail("respond_host refused request", bad);
    for (uint32_t i = 0; i < n && !rc; i++)
        if (out[i].kind != want[i].kind || out[i].arg != want[i].arg || out[i].pad[0] || out[i].pad[1] || out[i].pad[2]) rc = fail("HOST response differs", i);
    uint64_t by_kind[PWAF_RESP_KINDS] = {};
    for (uint32_t i = 0; i < n; i++) by_kind[want[i].kind]++;
    for (uint32_t k = 0; k < PWAF_RESP_KINDS && !rc; k++)
        if (counts[k] != by_kind[k]) rc = fail("HOST count differs", k);
    for (uint32_t l = 0; l < 4 && !rc; l++) {
        if (cnt[l] != members[l].size()) rc = fail("HOST list count differs", l);
        for (uint32_t j = 0; j < a.cap[l] && j < members[l].size() && !rc; j++)
            if (a.idx[l][j] != members[l][j]) rc = fail("HOST list entry differs", j);
    }
    if (counts_out) memcpy(counts_out, counts, sizeof(uint64_t) * PWAF_RESP_KINDS);
    for (uint32_t l = 0; l < 4; l++) delete[] a.idx[l];
    delete[] arena, delete[] off, delete[] verdicts, delete[] status, delete[] route, delete[] out, delete[] counts;
    return rc;
}

int main() {
    std::vector<Line> reqs;
    std::vector<R::Decision> want;
    bool has_route = true;
    char *line = nullptr;
    size_t room = 0;
    ssize_t got;
    while ((got = getline(&line, &room, stdin)) > 0) {
        Line r{};
        char route[32] = "";
        int at = 0;
        if (sscanf(line, "%u %u %u %31s %n", &r.action, &r.rule_idx, &r.status, route, &at) < 4) return fail("a line does not parse", reqs.size());
        has_route = route[0] != '-';
        r.route = has_route ? (uint32_t)strtoul(route, nullptr, 10) : PWAF_ROUTE_NONE;
        const char *hex = line + at;
        if (hex[0] != '-')
            for (size_t k = 0; hex[k] && hex[k + 1] && hex[k] != '\n'; k += 2) {
                unsigned v = 0;
                sscanf(hex + k, "%2x", &v);
                r.path += (char)v;
            }
        reqs.push_back(r);
    }
    free(line);
    for (size_t i = 0; i < reqs.size(); i++) {
        const size_t len = reqs[i].path.size();
        uint8_t *block = new uint8_t[len ? len : 1];  // exactly the path: a read at block[len] is a report
        memcpy(block, reqs[i].path.data(), len);
        const R::Decision d = R::decide(reqs[i].action, reqs[i].rule_idx, reqs[i].status, has_route, reqs[i].route, R::Exact{len ? block : block + 1}, (uint32_t)len);
        printf("R %u %u\n", d.kind, d.arg);
        want.push_back(d);
        delete[] block;
    }
    uint64_t counts[PWAF_RESP_KINDS];
    if (run_host(reqs, has_route, want, counts)) return 1;
    printf("H %zu", reqs.size());
    for (uint32_t k = 0; k < PWAF_RESP_KINDS; k++) printf(" %llu", (unsigned long long)counts[k]);
    printf("\n");
    if (run_host({}, has_route, {}, nullptr)) return 1;
    return 0;
}
