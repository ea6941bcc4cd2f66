// tools/async_bench.cpp — what a NATIVE async host sees through the non-blocking queue (pwaf_async_*): `threads` submitter threads keep
// up to `in_flight` requests each in flight, one poller waits on the queue's eventfd and collects completions. Reports requests/s,
// latency from a request's first submit attempt (PWAF_E_BUSY retries included) to its completion, the mean batch size and every
// verdict that differs from pwaf_evaluate_batch on the same request.
// Measurement harness only: built on first use by pingoo_amd.engine.native_async_throughput into tools/libasync_bench.so; it calls the
// product through the C ABI entry points it is handed, nothing else.
#include <poll.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "pwaf.h"

namespace {
typedef int (*create_fn)(pwaf_engine *, uint32_t, uint32_t, uint32_t, pwaf_async **);
typedef int (*submit_fn)(pwaf_async *, const pwaf_request *, uint64_t);
typedef size_t (*poll_fn)(pwaf_async *, pwaf_completion *, size_t);
typedef int (*fd_fn)(pwaf_async *);
typedef int (*flush_fn)(pwaf_async *);
typedef int (*stats_fn)(pwaf_async *, uint64_t *, uint64_t *, uint64_t *);
typedef void (*destroy_fn)(pwaf_async *);
int64_t now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace

extern "C" {
// fns: pwaf_async_create, _submit, _poll, _fd, _flush (unused: the deadline closes the tail), _stats, _destroy. want[k]: pwaf_evaluate_batch's verdict of reqs[k]. Thread t's
// j-th request is reqs[(t * 7 + j) % n_reqs], tagged (t << 40) | j. Writes one JSON object into out; returns 0, or the failing status.
int ab_run(void *const *fns, pwaf_engine *engine, void *, const pwaf_request *reqs, size_t n_reqs, const pwaf_verdict *want, int threads, int in_flight,
           uint64_t per_thread, uint32_t max_batch, uint32_t max_delay_us, char *out, size_t out_len) {
    auto create = (create_fn)fns[0];
    auto submit = (submit_fn)fns[1];
    auto poll_c = (poll_fn)fns[2];
    auto get_fd = (fd_fn)fns[3];
    auto stats = (stats_fn)fns[5];
    auto destroy = (destroy_fn)fns[6];
    pwaf_async *q = nullptr;
    int rc = create(engine, max_batch, max_delay_us, (uint32_t)threads * (uint32_t)in_flight, &q);
    if (rc) return rc;
    const uint64_t total = (uint64_t)threads * per_thread;
    std::vector<std::vector<int64_t>> t0(threads, std::vector<int64_t>(per_thread));
    std::vector<double> lat;
    lat.reserve(total);
    std::vector<std::atomic<int64_t>> outstanding(threads);
    for (auto &o : outstanding) o.store(0);
    std::atomic<uint64_t> busy{0}, refused{0};
    std::atomic<bool> go{false};
    uint64_t mismatches = 0, failed = 0, completed = 0;
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++)
        th.emplace_back([&, t] {
            while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
            bool first_try = true;  // a request's latency starts at its FIRST submit attempt: the time it spent refused with BUSY counts
            for (uint64_t j = 0; j < per_thread;) {
                if (outstanding[t].load(std::memory_order_acquire) >= in_flight) {
                    std::this_thread::yield();
                    continue;
                }
                const pwaf_request &r = reqs[((uint64_t)t * 7 + j) % n_reqs];
                if (first_try) t0[t][j] = now_ns();
                first_try = false;
                const int s = submit(q, &r, ((uint64_t)t << 40) | j);
                if (s == PWAF_E_BUSY) {
                    busy++;
                    std::this_thread::yield();
                    continue;
                }
                if (s != PWAF_OK) refused++;
                else outstanding[t].fetch_add(1, std::memory_order_acq_rel);
                j++;
                first_try = true;
            }
        });
    const auto w0 = std::chrono::steady_clock::now();
    go.store(true, std::memory_order_release);
    std::vector<pwaf_completion> c(8192);
    const int fd = get_fd(q);
    int64_t last_progress = now_ns();
    while (completed + refused.load() < total) {
        pollfd p{fd, POLLIN, 0};
        (void)::poll(&p, 1, 1);
        uint64_t one;
        (void)!read(fd, &one, sizeof one);
        size_t k;
        while ((k = poll_c(q, c.data(), c.size())) > 0) {
            const int64_t now = now_ns();
            for (size_t i = 0; i < k; i++) {
                const int t = (int)(c[i].tag >> 40);
                const uint64_t j = c[i].tag & ((1ull << 40) - 1);
                lat.push_back((double)(now - t0[t][j]) / 1000.0);
                const pwaf_verdict &w = want[((uint64_t)t * 7 + j) % n_reqs];
                if (c[i].status != PWAF_OK) failed++;
                else if (c[i].verdict.action != w.action || c[i].verdict.rule_idx != w.rule_idx) mismatches++;
                outstanding[t].fetch_sub(1, std::memory_order_acq_rel);
            }
            completed += k;
            last_progress = now;
        }
        if (now_ns() - last_progress > 60000000000ll) break;  // nothing for a minute: a hang, reported as completed < requests
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    for (auto &x : th) x.join();
    uint64_t nb = 0, nr = 0, fl = 0;
    stats(q, &nb, &nr, &fl);
    destroy(q);
    std::sort(lat.begin(), lat.end());
    auto pct = [&](double p) { return lat.empty() ? 0.0 : lat[std::min(lat.size() - 1, (size_t)(p / 100.0 * (double)(lat.size() - 1) + 0.5))]; };
    snprintf(out, out_len,
             "{\"submitter_threads\": %d, \"in_flight_per_thread\": %d, \"max_batch\": %u, \"deadline_us\": %u, \"requests\": %llu, \"completed\": %llu, "
             "\"seconds\": %.4f, \"requests_per_s\": %.1f, \"latency_us\": {\"p50\": %.1f, \"p99\": %.1f, \"max\": %.1f}, \"batches\": %llu, "
             "\"mean_batch\": %.1f, \"busy_retries\": %llu, \"refused\": %llu, \"failed\": %llu, \"mismatches\": %llu}",
             threads, in_flight, max_batch, max_delay_us, (unsigned long long)total, (unsigned long long)completed, secs, (double)completed / secs, pct(50), pct(99),
             lat.empty() ? 0.0 : lat.back(), (unsigned long long)nb, nb ? (double)nr / (double)nb : 0.0, (unsigned long long)busy.load(),
             (unsigned long long)refused.load(), (unsigned long long)failed, (unsigned long long)mismatches);
    return 0;
}
}
