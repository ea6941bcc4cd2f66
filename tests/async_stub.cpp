// TEST-ONLY: the non-blocking queue (pingoo_amd/csrc/async.cpp, the product source, compiled here with g++) over a STUB engine, so that its
// threading — lock-free slot reservation, closing and reusing segments, completions, the eventfd, destroy — is exercised on the CPU, also
// under ThreadSanitizer. The stub's pwaf_evaluate_records decodes the records with csrc/records.h (validating them as the engine does),
// takes ~150 us (a small batch on the device) and answers every request with a function of ITS OWN bytes; a batch holding a request whose
// host is "poison" fails with PWAF_E_DEVICE (one request in 5000 of submitter 1). Built and run by tests/test_async_cpu.py:
//   async_stub <mode> <threads> <per thread> <in flight per thread> <max_batch> <deadline us> <max_in_flight>
// modes: run (every tag once, its own verdict), flush (10 s deadline, flush), destroy (destroy with requests in flight), refuse (bad requests),
// starve (one GeoIP class saturates the dispatchers for <per thread> ms while a lone request of the other class waits for its deadline).
#include <poll.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../include/pwaf.h"
#include "../pingoo_amd/csrc/records.h"

struct pwaf_engine { int unused; };
namespace pwaf {
int fail(int code, const std::string &) { return code; }
}
static std::atomic<uint64_t> g_batches{0}, g_requests{0}, g_failed_batches{0};
static uint32_t mix(const uint8_t *p, uint32_t n, uint32_t seed) {
    uint32_t h = 2166136261u ^ seed;
    for (uint32_t i = 0; i < n; i++) h = (h ^ p[i]) * 16777619u;
    return h;
}
static bool poison(const uint8_t *host, uint32_t len) { return len == 6 && memcmp(host, "poison", 6) == 0; }
extern "C" {
uint32_t pwaf_engine_header_count(const pwaf_engine *) { return 2; }
const char *pwaf_last_error(void) { return "stub"; }
int pwaf_host_alloc(size_t bytes, void **out) {
    *out = aligned_alloc(4096, (bytes + 4095) & ~(size_t)4095);
    return *out ? PWAF_OK : PWAF_E_NOMEM;
}
void pwaf_host_free(void *p) { free(p); }
int pwaf_evaluate_records(pwaf_engine *, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n, pwaf_verdict *out, pwaf_counts *) {
    namespace R = pwaf::records;
    const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(150);
    std::vector<uint64_t> totals(PWAF_N_FIELDS + 2);
    uint32_t bad = 0;
    int geo = 0;
    uint64_t lo, hi;
    if (R::validate(buf, buf_bytes, rec_off, n, PWAF_N_FIELDS + 2, totals.data(), &bad, &geo, &lo, &hi) != R::kOk) return PWAF_E_BATCH;
    bool fails = false;
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t *r = buf + rec_off[i];
        pwaf_record_head h;
        R::load_head(r, &h);
        uint32_t at = R::values_offset(h.n_values) + R::load_len(r, 0) + R::load_len(r, 1);  // the path: value 2
        uint32_t hh = mix(r + at, R::load_len(r, 2), h.port);
        if (h.n_values > PWAF_N_FIELDS + 1) {  // header 1 (value 6) joins the function when the record carries it
            for (uint32_t k = 2; k < PWAF_N_FIELDS + 1; k++) at += R::load_len(r, k);
            hh = mix(r + at, R::load_len(r, PWAF_N_FIELDS + 1), hh);
        }
        hh ^= h.has_geoip ? (uint32_t)h.country[0] << 8 : 0u;
        out[i].action = (uint8_t)(hh & 3u);
        out[i].rule_idx = hh >> 2;
        fails = fails || poison(r + R::values_offset(h.n_values), R::load_len(r, 0));
    }
    g_batches++;
    g_requests += n;
    while (std::chrono::steady_clock::now() < until) std::this_thread::yield();
    if (fails) {
        g_failed_batches++;
        return PWAF_E_DEVICE;
    }
    return PWAF_OK;
}
}

struct Req {  // one request of the run and what it must come back with
    char path[48], hdr[24];
    pwaf_span spans[2];
    pwaf_request r;
    uint32_t want;
    bool poisoned;
};

static void make(Req &q, int t, uint64_t j) {
    const int n = snprintf(q.path, sizeof q.path, "/t%d/call%llu", t, (unsigned long long)j);
    const int m = snprintf(q.hdr, sizeof q.hdr, "h%llu", (unsigned long long)(j % 7));
    memset(&q.r, 0, sizeof q.r);
    q.poisoned = t == 1 && j % 5000 == 11;
    q.r.host = q.poisoned ? "poison" : "h", q.r.host_len = q.poisoned ? 6 : 1;
    q.r.url = q.path, q.r.url_len = (uint32_t)n;
    q.r.path = q.path, q.r.path_len = (uint32_t)n;
    q.r.method = "GET", q.r.method_len = 3;
    q.r.user_agent = "ua", q.r.user_agent_len = 2;
    q.r.port = (uint16_t)(t * 131 + j * 7);
    q.r.has_geoip = (j & 1) ? 1 : 0;  // both GeoIP classes
    q.r.country[0] = 'F', q.r.country[1] = 'R';
    // header values: none, one, or both (records of 5, 6 or 7 values)
    q.spans[0] = pwaf_span{"x", 1, 0};
    q.spans[1] = pwaf_span{q.hdr, (uint32_t)m, 0};
    q.r.headers = q.spans;
    q.r.n_headers = (uint32_t)(j % 3);
    uint32_t hh = mix((const uint8_t *)q.path, (uint32_t)n, q.r.port);
    if (q.r.n_headers == 2) hh = mix((const uint8_t *)q.hdr, (uint32_t)m, hh);
    hh ^= q.r.has_geoip ? (uint32_t)'F' << 8 : 0u;
    q.want = hh;
}

static int64_t now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "run";
    const int threads = argc > 2 ? atoi(argv[2]) : 8;
    const uint64_t per = argc > 3 ? strtoull(argv[3], nullptr, 10) : 20000;
    const int64_t window = argc > 4 ? atoi(argv[4]) : 2048;
    const uint32_t max_batch = argc > 5 ? (uint32_t)atoi(argv[5]) : 4096, deadline = argc > 6 ? (uint32_t)atoi(argv[6]) : 200;
    const uint32_t max_in_flight = argc > 7 ? (uint32_t)atoi(argv[7]) : (uint32_t)(threads * window);
    pwaf_engine eng{};
    pwaf_async *q = nullptr;
    if (pwaf_async_create(&eng, max_batch, deadline, max_in_flight, &q) != PWAF_OK) return 2;
    if (mode == "refuse") {
        Req a;
        make(a, 0, 1);
        a.r.country[0] = 'f';
        const int bad_country = pwaf_async_submit(q, &a.r, 1);
        make(a, 0, 1);
        std::vector<char> big(64u << 20, 'a');
        a.r.url = big.data(), a.r.url_len = (uint32_t)big.size();
        const int too_big = pwaf_async_submit(q, &a.r, 2);
        make(a, 0, 1);
        a.r.path = nullptr;
        const int null_field = pwaf_async_submit(q, &a.r, 3);
        uint64_t nb, nr, fl;
        pwaf_async_stats(q, &nb, &nr, &fl);
        pwaf_async_destroy(q);
        printf("{\"bad_country\": %d, \"too_big\": %d, \"null_field\": %d, \"in_flight\": %llu}\n", bad_country, too_big, null_field, (unsigned long long)fl);
        return 0;
    }
    if (mode == "starve") {
        // `threads` submitters keep the dispatchers saturated with requests WITHOUT GeoIP for `per` milliseconds (segments close by count);
        // 100 ms in, one request WITH GeoIP is submitted: its batch must still close at its deadline, not when the other class goes quiet
        const uint64_t kLone = 1ull << 62;
        std::atomic<bool> flood{true};
        std::atomic<int64_t> lone_done_ns{0};
        std::atomic<int> lone_status{1};
        std::atomic<uint64_t> submitted{0}, completed{0};
        std::vector<std::atomic<int64_t>> outstanding(threads);
        for (auto &o : outstanding) o.store(0);
        std::thread poller([&] {
            std::vector<pwaf_completion> c(1000);
            while (flood.load() || completed.load() < submitted.load() + 1) {
                pollfd p{pwaf_async_fd(q), POLLIN, 0};
                ::poll(&p, 1, 10);
                uint64_t one;
                (void)!read(p.fd, &one, sizeof one);
                size_t k;
                while ((k = pwaf_async_poll(q, c.data(), c.size())) > 0) {
                    for (size_t i = 0; i < k; i++) {
                        if (c[i].tag == kLone) {
                            lone_done_ns.store(now_ns());
                            lone_status.store(c[i].status);
                        } else {
                            outstanding[c[i].tag >> 40].fetch_sub(1);
                        }
                    }
                    completed += k;
                }
            }
        });
        std::vector<std::thread> th;
        for (int t = 0; t < threads; t++)
            th.emplace_back([&, t] {
                Req rq;
                for (uint64_t j = 0; flood.load();) {
                    if (outstanding[t].load() >= window) { std::this_thread::yield(); continue; }
                    make(rq, t, j);
                    rq.r.has_geoip = 0;
                    outstanding[t].fetch_add(1);
                    const int st = pwaf_async_submit(q, &rq.r, ((uint64_t)t << 40) | j);
                    if (st != PWAF_OK) { outstanding[t].fetch_sub(1); std::this_thread::yield(); continue; }
                    submitted++;
                    j++;
                }
            });
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        Req lone;
        make(lone, 0, 1);  // (odd j: has_geoip = 1)
        const int64_t t0 = now_ns();
        const int rc = pwaf_async_submit(q, &lone.r, kLone);
        std::this_thread::sleep_for(std::chrono::milliseconds(per > 100 ? per - 100 : 0));
        uint64_t mid_batches = 0;
        pwaf_async_stats(q, &mid_batches, nullptr, nullptr);
        const int64_t flood_end = now_ns();
        flood.store(false);
        for (auto &x : th) x.join();
        poller.join();
        pwaf_async_destroy(q);
        const int64_t done = lone_done_ns.load();
        printf("{\"lone_rc\": %d, \"lone_status\": %d, \"lone_ms\": %.3f, \"lone_before_flood_end\": %s, \"flood_requests\": %llu, \"batches\": %llu}\n", rc,
               lone_status.load(), done ? (done - t0) / 1e6 : -1.0, done && done < flood_end ? "true" : "false", (unsigned long long)submitted.load(),
               (unsigned long long)mid_batches);
        return 0;
    }
    if (mode == "flush" || mode == "destroy") {
        // one thread submits `per` requests; flush: they must come back long before the deadline; destroy: destroyed with all of them in flight
        std::vector<Req> rs(per);
        for (uint64_t j = 0; j < per; j++) {
            make(rs[j], 0, j);
            if (pwaf_async_submit(q, &rs[j].r, j) != PWAF_OK) return 5;
        }
        const int64_t t0 = now_ns();
        if (mode == "destroy") {
            pwaf_async_destroy(q);
            printf("{\"evaluated\": %llu, \"submitted\": %llu, \"destroy_ms\": %.2f}\n", (unsigned long long)g_requests.load(), (unsigned long long)per, (now_ns() - t0) / 1e6);
            return g_requests.load() == per ? 0 : 1;
        }
        pwaf_async_flush(q);
        std::vector<pwaf_completion> c(4096);
        uint64_t got = 0;
        while (got < per && now_ns() - t0 < 5000000000ll) {
            pollfd p{pwaf_async_fd(q), POLLIN, 0};
            ::poll(&p, 1, 100);
            uint64_t one;
            (void)!read(p.fd, &one, sizeof one);
            size_t k;
            while ((k = pwaf_async_poll(q, c.data(), c.size())) > 0) got += k;
        }
        const double ms = (now_ns() - t0) / 1e6;
        pwaf_async_destroy(q);
        printf("{\"completed\": %llu, \"submitted\": %llu, \"ms\": %.2f}\n", (unsigned long long)got, (unsigned long long)per, ms);
        return got == per ? 0 : 1;
    }
    // run: `threads` submitters with up to `window` requests each in flight, one poller on the eventfd
    const uint64_t total = (uint64_t)threads * per;
    std::vector<std::vector<Req>> rs(threads, std::vector<Req>(per));
    std::vector<std::vector<uint8_t>> seen(threads, std::vector<uint8_t>(per, 0));
    std::vector<std::atomic<int64_t>> outstanding(threads);
    for (auto &o : outstanding) o.store(0);
    std::atomic<uint64_t> busy{0}, refused{0};
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++)
        th.emplace_back([&, t] {
            for (uint64_t j = 0; j < per;) {
                if (outstanding[t].load(std::memory_order_acquire) >= window) {
                    std::this_thread::yield();
                    continue;
                }
                make(rs[t][j], t, j);
                outstanding[t].fetch_add(1, std::memory_order_acq_rel);
                const int s = pwaf_async_submit(q, &rs[t][j].r, ((uint64_t)t << 40) | j);
                if (s == PWAF_E_BUSY) {
                    outstanding[t].fetch_sub(1, std::memory_order_acq_rel);
                    busy++;
                    std::this_thread::yield();
                    continue;
                }
                if (s != PWAF_OK) refused++;
                j++;
            }
        });
    uint64_t completed = 0, dup = 0, wrong = 0, failed = 0, failed_wrong = 0, poisoned = 0;
    std::vector<pwaf_completion> c(1000);
    int64_t last = now_ns();
    while (completed < total && now_ns() - last < 20000000000ll) {
        pollfd p{pwaf_async_fd(q), POLLIN, 0};
        ::poll(&p, 1, 100);
        uint64_t one;
        (void)!read(p.fd, &one, sizeof one);
        size_t k;
        while ((k = pwaf_async_poll(q, c.data(), c.size())) > 0) {
            for (size_t i = 0; i < k; i++) {
                const int t = (int)(c[i].tag >> 40);
                const uint64_t j = c[i].tag & ((1ull << 40) - 1);
                if (t >= threads || j >= per || seen[t][j]++) { dup++; continue; }
                const Req &r = rs[t][j];
                poisoned += r.poisoned;
                if (c[i].status != PWAF_OK) {
                    failed++;
                    failed_wrong += c[i].status != PWAF_E_DEVICE || c[i].verdict.action != PWAF_ACTION_ALLOW || c[i].verdict.rule_idx != PWAF_RULE_NONE;
                } else {
                    wrong += r.poisoned || c[i].verdict.action != (uint8_t)(r.want & 3u) || c[i].verdict.rule_idx != (r.want >> 2);
                }
                outstanding[t].fetch_sub(1, std::memory_order_acq_rel);
            }
            completed += k;
            last = now_ns();
        }
    }
    for (auto &x : th) x.join();
    uint64_t nb = 0, nr = 0, fl = 0;
    pwaf_async_stats(q, &nb, &nr, &fl);
    pwaf_async_destroy(q);
    printf("{\"requests\": %llu, \"completed\": %llu, \"duplicates\": %llu, \"wrong\": %llu, \"failed\": %llu, \"failed_wrong\": %llu, \"poisoned\": %llu, "
           "\"failed_batches\": %llu, \"busy\": %llu, \"refused\": %llu, \"batches\": %llu, \"in_flight_after\": %llu}\n",
           (unsigned long long)total, (unsigned long long)completed, (unsigned long long)dup, (unsigned long long)wrong, (unsigned long long)failed,
           (unsigned long long)failed_wrong, (unsigned long long)poisoned, (unsigned long long)g_failed_batches.load(), (unsigned long long)busy.load(),
           (unsigned long long)refused.load(), (unsigned long long)nb, (unsigned long long)fl);
    return (completed == total && dup == 0 && wrong == 0 && failed_wrong == 0 && refused.load() == 0) ? 0 : 1;
}
