// async.cpp — the non-blocking request queue (pwaf_async_*): submit now, collect the verdict later.
//
// The reference runs its rule loop inside the async hyper closure of every request (pingoo/listeners/http_listener.rs:133-274). An async
// host cannot block a worker per request the way pwaf_batcher_evaluate does, so here a request is submitted with a tag and answered through
// a completion queue and an eventfd. Plain C++17 on top of the public C ABI (pwaf_evaluate_records, pwaf_host_alloc): no device code.
//
// Segments. A segment is one page-locked block: the records of one batch (written by pwaf_async_submit, each request copied ONCE, as a
// record — csrc/records.h), their offsets and tags, and the verdicts pwaf_evaluate_records writes back. Every segment belongs to one GeoIP
// class for its whole life (requests with and without caller-supplied GeoIP never share a batch: pwaf_evaluate_records needs all or none).
// The open segment of a class takes submissions; a submitter reserves its slot and bytes with ONE compare-and-swap on the segment's
// packed word (bit 63 closed, bits 32..62 requests, bits 0..31 bytes), writes its record outside any lock and counts itself in `written`.
// Closing sets bit 63 (under the class's mutex, together with installing the next free segment); the reservations made before it are
// exactly the batch, and the dispatcher waits for `written` to reach their count before it reads the segment. A closed segment cannot
// take a reservation, and a free one is kept closed, so a stale pointer to the open segment is harmless: a reservation only succeeds in
// the segment that is open for its class at that moment.
//
// Dispatch. Two dispatcher threads take closed segments in order, run pwaf_evaluate_records on them (one overlaps the other's device
// time) and publish the completions. Before taking the next closed segment, a dispatcher closes every open segment whose oldest request
// has waited max_delay_us — unless a batch of the same class is still waiting in the queue, in which case it keeps filling until that one
// is taken — so a class that keeps the dispatchers busy cannot hold back the other class's deadline. A segment returns to its class's
// free list only after pwaf_evaluate_records on it has returned.
//
// GeoIP answers. A queue made by pwaf_async_create_geo keeps a pwaf_geo per slot and per completion. The evaluator that fills them
// (pwaf_evaluate_records_geo) reaches the queue as a function pointer (pwaf::async_create_with, called from evaluate_records.cpp): this file refers
// to no engine symbol beyond pwaf_engine_header_count, pwaf_host_alloc / _free and pwaf_evaluate_records, so the CPU suite links it
// against a stub engine.
#include <sys/eventfd.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pwaf.h"
#include "records.h"

namespace pwaf {
using RecordsGeoFn = int (*)(pwaf_engine *, const uint8_t *, size_t, const uint32_t *, uint32_t, pwaf_verdict *, pwaf_counts *, pwaf_geo *);
int async_create_with(pwaf_engine *engine, uint32_t max_batch, uint32_t max_delay_us, uint32_t max_in_flight, RecordsGeoFn eval_geo, pwaf_async **out);
}
using pwaf::fail;

namespace {

#ifdef PWAF_BATCHER_SYSTEM_CLOCK
using Clock = std::chrono::system_clock;  // (the ThreadSanitizer build: see batcher.cpp — timed waits on the steady clock are not intercepted)
#else
using Clock = std::chrono::steady_clock;
#endif

constexpr uint64_t kClosed = 1ull << 63;
constexpr uint64_t kOne = 1ull << 32;  // one request in the packed word
constexpr uint32_t kSegments = 4;      // per GeoIP class: the open one, one waiting, one on each dispatcher

inline uint32_t word_count(uint64_t w) { return (uint32_t)((w & ~kClosed) >> 32); }
inline uint32_t word_bytes(uint64_t w) { return (uint32_t)w; }

struct Segment {
    int geo = 0;
    uint8_t *mem = nullptr;  // page-locked: [records: cap_bytes] [tags: cap_n] [verdicts: cap_n] [rec_off: cap_n] [GeoIP answers: cap_n, a geo queue's only]
    uint32_t cap_bytes = 0, cap_n = 0;
    uint32_t *rec_off = nullptr;
    uint64_t *tags = nullptr;
    pwaf_verdict *verdicts = nullptr;
    pwaf_geo *geos = nullptr;  // a geo queue's segments: the record of every slot
    std::atomic<uint64_t> word{kClosed};
    std::atomic<uint32_t> written{0};
    std::atomic<int64_t> first_ns{0};  // when the batch's first request reserved its slot (Clock, since epoch)
    uint32_t n = 0, bytes = 0;         // the closed batch (set when it closes)
};

int64_t now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now().time_since_epoch()).count(); }

}  // namespace

struct pwaf_async {
    pwaf_engine *engine = nullptr;
    pwaf::RecordsGeoFn eval_geo = nullptr;  // a geo queue (pwaf_async_create_geo): the evaluator that also answers the records
    uint32_t n_cols = PWAF_N_FIELDS;
    uint32_t max_batch = 0, max_in_flight = 0;
    int64_t max_delay_ns = 0;
    int efd = -1;
    std::vector<Segment *> all;
    // per GeoIP class: the open segment (read lock-free by submitters) and the free list; `mu[g]` guards closing / installing
    std::atomic<Segment *> open[2] = {{nullptr}, {nullptr}};
    std::vector<Segment *> free_list[2];
    std::mutex mu[2];
    // closed segments waiting for a dispatcher
    std::mutex dmu;
    std::condition_variable dcv;
    std::deque<Segment *> closed;
    uint32_t queued[2] = {0, 0};  // segments of each GeoIP class in `closed`
    bool stop = false;
    std::thread worker[2];
    // completions
    std::mutex cmu;
    std::deque<pwaf_completion> done;
    std::deque<pwaf_geo> done_geo;  // a geo queue's: parallel to `done`
    std::atomic<uint64_t> in_flight{0};  // submitted, not yet handed out by poll
    std::atomic<uint64_t> n_batches{0}, n_requests{0};
    std::atomic<bool> stopping{false};
    std::atomic<uint32_t> inside{0};  // threads inside submit / poll / flush / stats / fd: destroy waits for them

    // Closes the open segment of class g when it is still `expect` (nullptr: whichever is open) and holds requests; installs the next free
    // one. Returns false when the class has no open segment afterwards (every segment is busy).
    bool close_open(int g, Segment *expect) {
        std::lock_guard<std::mutex> lk(mu[g]);
        Segment *s = open[g].load(std::memory_order_acquire);
        if (s && (!expect || s == expect)) {
            const uint64_t w = s->word.fetch_or(kClosed, std::memory_order_acq_rel);
            if (word_count(w) == 0) {
                s->word.store(0, std::memory_order_release);  // nothing to send: open again
            } else {
                s->n = word_count(w);
                s->bytes = word_bytes(w);
                open[g].store(nullptr, std::memory_order_release);
                {
                    std::lock_guard<std::mutex> dl(dmu);
                    closed.push_back(s);
                    queued[g]++;
                }
                dcv.notify_one();
                s = nullptr;
            }
        }
        if (!open[g].load(std::memory_order_relaxed)) install_locked(g);
        return open[g].load(std::memory_order_relaxed) != nullptr;
    }
    void install_locked(int g) {
        if (free_list[g].empty()) return;
        Segment *s = free_list[g].back();
        free_list[g].pop_back();
        s->written.store(0, std::memory_order_relaxed);
        s->first_ns.store(0, std::memory_order_relaxed);
        s->word.store(0, std::memory_order_release);  // (open: reservations may start)
        open[g].store(s, std::memory_order_release);
    }
    void release(Segment *s) {
        std::lock_guard<std::mutex> lk(mu[s->geo]);
        free_list[s->geo].push_back(s);
        if (!open[s->geo].load(std::memory_order_relaxed)) install_locked(s->geo);
    }

    void publish(Segment *s, int rc) {
        {
            std::lock_guard<std::mutex> lk(cmu);
            for (uint32_t i = 0; i < s->n; i++) {
                pwaf_completion c{};
                c.tag = s->tags[i];
                c.status = rc;
                if (rc == PWAF_OK) {
                    c.verdict = s->verdicts[i];
                } else {
                    c.verdict.action = PWAF_ACTION_ALLOW;
                    c.verdict.rule_idx = PWAF_RULE_NONE;
                }
                done.push_back(c);
                if (eval_geo) done_geo.push_back(rc == PWAF_OK ? s->geos[i] : pwaf_geo{0u, {'X', 'X'}, 0u});
            }
        }
        n_batches.fetch_add(1, std::memory_order_relaxed);
        n_requests.fetch_add(s->n, std::memory_order_relaxed);
        const uint64_t one = 1;
        ssize_t wr;
        do wr = write(efd, &one, sizeof one);
        while (wr < 0 && errno == EINTR);  // (EAGAIN: the counter is saturated — the fd is readable anyway)
    }

    void run() {
        std::unique_lock<std::mutex> lk(dmu);
        for (;;) {
            // Deadlines FIRST, on every iteration: while one GeoIP class keeps both dispatchers busy (its segments close by count and keep
            // `closed` non-empty), the other class's open segment must still close when its oldest request has waited max_delay_us. A due
            // segment whose class already has a batch waiting for a dispatcher keeps filling instead: it could only queue behind that one,
            // and it is closed here as soon as that one is taken (so a class saturating the dispatchers still gets batches that grow with
            // the load). Closing takes the class's mutex, which is never taken under `dmu`'s: done with `dmu` released.
            int64_t wake = INT64_MAX;
            const int64_t now = now_ns();
            Segment *due = nullptr;
            for (int g = 0; g < 2 && !due; g++) {
                Segment *s = open[g].load(std::memory_order_acquire);
                if (!s || queued[g]) continue;
                const int64_t f = s->first_ns.load(std::memory_order_acquire);
                if (f == 0 || word_count(s->word.load(std::memory_order_acquire)) == 0) continue;
                if (f + max_delay_ns <= now) due = s;
                else wake = std::min(wake, f + max_delay_ns);
            }
            if (due) {
                lk.unlock();
                close_open(due->geo, due);  // (a no-op when a submitter closed it meanwhile)
                lk.lock();
                continue;
            }
            if (!closed.empty()) {
                Segment *s = closed.front();
                closed.pop_front();
                queued[s->geo]--;
                lk.unlock();
                // the submitters that reserved before the close finish copying their records (a few hundred nanoseconds)
                while (s->written.load(std::memory_order_acquire) < s->n) std::this_thread::yield();
                try {
                    publish(s, eval_geo ? eval_geo(engine, s->mem, s->bytes, s->rec_off, s->n, s->verdicts, nullptr, s->geos)
                                        : pwaf_evaluate_records(engine, s->mem, s->bytes, s->rec_off, s->n, s->verdicts, nullptr));
                } catch (const std::exception &) {  // (std::bad_alloc of the completion queue: nothing may escape a worker thread)
                }
                release(s);
                lk.lock();
                continue;
            }
            if (stop) return;
            // idle until the earliest deadline of an open segment that holds requests (on Clock: a timed wait goes through wait_until)
            if (wake == INT64_MAX) dcv.wait(lk);
            else dcv.wait_until(lk, Clock::time_point(std::chrono::duration_cast<Clock::duration>(std::chrono::nanoseconds(wake))));
        }
    }
};

int pwaf::async_create_with(pwaf_engine *engine, uint32_t max_batch, uint32_t max_delay_us, uint32_t max_in_flight, pwaf::RecordsGeoFn eval_geo, pwaf_async **out) {
    if (!engine || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (max_batch == 0 || max_in_flight == 0) return fail(PWAF_E_INVALID_ARG, "max_batch and max_in_flight must be at least 1");
    auto *q = new (std::nothrow) pwaf_async();
    if (!q) return fail(PWAF_E_NOMEM, "pwaf_async_create: out of memory");
    q->engine = engine;
    q->eval_geo = eval_geo;
    q->n_cols = PWAF_N_FIELDS + pwaf_engine_header_count(engine);
    if (q->n_cols > pwaf::records::kMaxValues) {  // (submit's per-request arrays hold kMaxValues values)
        delete q;
        return fail(PWAF_E_UNSUPPORTED, "the engine has more columns than a record can carry");
    }
    q->max_batch = std::min<uint32_t>(max_batch, 1u << 20);
    q->max_in_flight = max_in_flight;
    q->max_delay_ns = (int64_t)max_delay_us * 1000;
    // a segment holds a full batch of requests of up to 1 KiB each, 1 MiB at least, 256 MiB at most
    const uint64_t cap_bytes = std::min<uint64_t>(std::max<uint64_t>((uint64_t)q->max_batch * 1024u, 1u << 20), 256u << 20);
    q->efd = eventfd(0, EFD_NONBLOCK | EFD_CLOEXEC);
    if (q->efd < 0) {
        delete q;
        return fail(PWAF_E_INVALID_ARG, std::string("eventfd failed: ") + strerror(errno));
    }
    for (int g = 0; g < 2; g++)
        for (uint32_t k = 0; k < kSegments; k++) {
            auto *s = new Segment();
            s->geo = g;
            s->cap_bytes = (uint32_t)cap_bytes;
            s->cap_n = q->max_batch;
            const size_t total = cap_bytes + (size_t)s->cap_n * (4 + 8 + sizeof(pwaf_verdict) + (eval_geo ? sizeof(pwaf_geo) : 0));
            void *p = nullptr;
            const int rc = pwaf_host_alloc(total, &p);
            if (rc != PWAF_OK) {
                delete s;
                pwaf_async_destroy(q);
                return rc;
            }
            s->mem = (uint8_t *)p;
            s->tags = (uint64_t *)(s->mem + cap_bytes);
            s->verdicts = (pwaf_verdict *)(s->tags + s->cap_n);
            s->rec_off = (uint32_t *)(s->verdicts + s->cap_n);
            if (eval_geo) s->geos = (pwaf_geo *)(s->mem + cap_bytes + (size_t)s->cap_n * (4 + 8 + sizeof(pwaf_verdict)));
            q->all.push_back(s);
            q->free_list[g].push_back(s);
        }
    for (int g = 0; g < 2; g++) {
        std::lock_guard<std::mutex> lk(q->mu[g]);
        q->install_locked(g);
    }
    for (auto &w : q->worker) w = std::thread([q] { q->run(); });
    *out = q;
    return PWAF_OK;
}

extern "C" {

int pwaf_async_create(pwaf_engine *engine, uint32_t max_batch, uint32_t max_delay_us, uint32_t max_in_flight, pwaf_async **out) {
    return pwaf::async_create_with(engine, max_batch, max_delay_us, max_in_flight, nullptr, out);
}

namespace {
// Counted on every way into / out of the queue's entry points: pwaf_async_destroy waits for these. The handshake with destroy is a
// store-buffer pattern (an entry point: count itself, then read `stopping`; destroy: set `stopping`, then read the count), so all four
// accesses are sequentially consistent: with release / acquire alone both sides could read the other's old value, and a submitter would
// write into a segment that destroy is freeing.
struct Inside {
    std::atomic<uint32_t> &c;
    explicit Inside(std::atomic<uint32_t> &x) : c(x) { c.fetch_add(1, std::memory_order_seq_cst); }
    ~Inside() { c.fetch_sub(1, std::memory_order_release); }
};
}  // namespace

int pwaf_async_submit(pwaf_async *q, const pwaf_request *r, uint64_t tag) {
    if (!q || !r) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    Inside guard(q->inside);
    if (q->stopping.load(std::memory_order_seq_cst)) return fail(PWAF_E_INVALID_ARG, "queue is shutting down");
    if (r->n_headers && !r->headers) return fail(PWAF_E_INVALID_ARG, "n_headers without a headers array");
    // the record: the five fields, then the header values the engine reads (the rest reads as "")
    const uint32_t n_values = PWAF_N_FIELDS + std::min<uint32_t>(r->n_headers, q->n_cols - PWAF_N_FIELDS);
    const char *ptr[pwaf::records::kMaxValues];
    uint32_t len[pwaf::records::kMaxValues];
    ptr[0] = r->host, ptr[1] = r->url, ptr[2] = r->path, ptr[3] = r->method, ptr[4] = r->user_agent;
    len[0] = r->host_len, len[1] = r->url_len, len[2] = r->path_len, len[3] = r->method_len, len[4] = r->user_agent_len;
    uint64_t value_bytes = 0;
    for (uint32_t k = 0; k < n_values; k++) {
        if (k >= PWAF_N_FIELDS) {
            ptr[k] = r->headers[k - PWAF_N_FIELDS].data;
            len[k] = r->headers[k - PWAF_N_FIELDS].len;
        }
        if (len[k] && !ptr[k]) return fail(PWAF_E_INVALID_ARG, "NULL field with non-zero length");
        value_bytes += len[k];
    }
    // what would fail the SHARED batch is refused here, for this request only (pingoo/geoip.rs:128-142: two letters A-Z)
    if (r->has_geoip && (r->country[0] < 'A' || r->country[0] > 'Z' || r->country[1] < 'A' || r->country[1] > 'Z'))
        return fail(PWAF_E_BATCH, "country is not two letters A-Z (pingoo/geoip.rs:128-142)");
    const uint64_t size = pwaf::records::record_size(n_values, value_bytes);
    const Segment *any = q->all.front();
    if (size > any->cap_bytes)
        return fail(PWAF_E_BATCH, "request of " + std::to_string(size) + " record bytes does not fit a queue segment (" + std::to_string(any->cap_bytes) + " bytes)");
    if (q->in_flight.fetch_add(1, std::memory_order_acq_rel) >= q->max_in_flight) {
        q->in_flight.fetch_sub(1, std::memory_order_acq_rel);
        return PWAF_E_BUSY;
    }
    const int g = r->has_geoip ? 1 : 0;
    for (;;) {
        Segment *s = q->open[g].load(std::memory_order_acquire);
        if (s) {
            uint64_t w = s->word.load(std::memory_order_acquire);
            while (!(w & kClosed) && word_count(w) < s->cap_n && (uint64_t)word_bytes(w) + size <= s->cap_bytes &&
                   !s->word.compare_exchange_weak(w, w + kOne + size, std::memory_order_acq_rel, std::memory_order_acquire)) {
            }
            if (!(w & kClosed) && word_count(w) < s->cap_n && (uint64_t)word_bytes(w) + size <= s->cap_bytes) {
                // reserved: slot word_count(w) at byte word_bytes(w)
                const uint32_t slot = word_count(w), at = word_bytes(w);
                uint8_t *rec = s->mem + at;
                pwaf_record_head h{};
                h.size = (uint32_t)size;
                h.n_values = (uint16_t)n_values;
                h.port = r->port;
                memcpy(h.ip, r->ip, 16);
                h.flags = r->flags;
                h.ip_is_v6 = r->ip_is_v6;
                if (g) {
                    h.has_geoip = 1;
                    h.asn = r->asn;
                    h.country[0] = r->country[0];
                    h.country[1] = r->country[1];
                }
                memcpy(rec, &h, sizeof h);
                memcpy(rec + sizeof h, len, 4u * n_values);
                const uint32_t vo = pwaf::records::values_offset(n_values);
                memset(rec + sizeof h + 4u * n_values, 0, vo - sizeof h - 4u * n_values);
                uint8_t *p = rec + vo;
                for (uint32_t k = 0; k < n_values; k++) {
                    if (len[k]) memcpy(p, ptr[k], len[k]);
                    p += len[k];
                }
                memset(p, 0, (size_t)(rec + size - p));
                s->rec_off[slot] = at;
                s->tags[slot] = tag;
                if (slot == 0) {
                    s->first_ns.store(now_ns(), std::memory_order_release);
                    std::lock_guard<std::mutex> dl(q->dmu);  // (a dispatcher starts the batch's clock)
                    q->dcv.notify_one();
                }
                s->written.fetch_add(1, std::memory_order_release);
                if (slot + 1 == s->cap_n) q->close_open(g, s);  // full: send it now
                return PWAF_OK;
            }
        }
        // no open segment, or no room in it: close it and take the next free one (or report BUSY when every segment is busy)
        if (!q->close_open(g, s)) {
            q->in_flight.fetch_sub(1, std::memory_order_acq_rel);
            return PWAF_E_BUSY;
        }
    }
}

namespace {
size_t poll_into(pwaf_async *q, pwaf_completion *out, pwaf_geo *geo, size_t cap) {
    Inside guard(q->inside);
    size_t k = 0;
    {
        std::lock_guard<std::mutex> lk(q->cmu);
        k = std::min(cap, q->done.size());
        std::copy(q->done.begin(), q->done.begin() + (ptrdiff_t)k, out);
        q->done.erase(q->done.begin(), q->done.begin() + (ptrdiff_t)k);
        if (q->eval_geo) {  // (a plain poll of a geo queue drops the records)
            if (geo) std::copy(q->done_geo.begin(), q->done_geo.begin() + (ptrdiff_t)k, geo);
            q->done_geo.erase(q->done_geo.begin(), q->done_geo.begin() + (ptrdiff_t)k);
        }
    }
    q->in_flight.fetch_sub(k, std::memory_order_acq_rel);
    return k;
}
}  // namespace

size_t pwaf_async_poll(pwaf_async *q, pwaf_completion *out, size_t cap) {
    if (!q || !out || !cap) return 0;
    return poll_into(q, out, nullptr, cap);
}

size_t pwaf_async_poll_geo(pwaf_async *q, pwaf_completion *out, pwaf_geo *geo, size_t cap) {
    if (!q || !out || !cap) return 0;
    if (!q->eval_geo) {
        (void)fail(PWAF_E_UNSUPPORTED, "pwaf_async_poll_geo: the queue was not made by pwaf_async_create_geo (PWAF_OPT_GEO_ANSWERS)");
        return 0;
    }
    return poll_into(q, out, geo, cap);
}

int pwaf_async_fd(pwaf_async *q) {
    if (!q) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    return q->efd;
}

int pwaf_async_flush(pwaf_async *q) {
    if (!q) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    Inside guard(q->inside);
    for (int g = 0; g < 2; g++) q->close_open(g, nullptr);
    return PWAF_OK;
}

int pwaf_async_stats(pwaf_async *q, uint64_t *n_batches, uint64_t *n_requests, uint64_t *in_flight) {
    if (!q) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    Inside guard(q->inside);
    if (n_batches) *n_batches = q->n_batches.load(std::memory_order_acquire);
    if (n_requests) *n_requests = q->n_requests.load(std::memory_order_acquire);
    if (in_flight) *in_flight = q->in_flight.load(std::memory_order_acquire);
    return PWAF_OK;
}

void pwaf_async_destroy(pwaf_async *q) {
    if (!q) return;
    q->stopping.store(true, std::memory_order_seq_cst);
    // submitters that got past the check finish their records, pollers leave
    while (q->inside.load(std::memory_order_seq_cst) != 0) std::this_thread::sleep_for(std::chrono::microseconds(50));
    // every accepted request is evaluated: close the open segments, let the dispatchers drain the queue
    for (int g = 0; g < 2; g++) q->close_open(g, nullptr);
    {
        std::unique_lock<std::mutex> lk(q->dmu);
        q->stop = true;
        q->dcv.notify_all();
    }
    for (auto &w : q->worker)
        if (w.joinable()) w.join();
    for (Segment *s : q->all) {
        pwaf_host_free(s->mem);
        delete s;
    }
    if (q->efd >= 0) close(q->efd);
    delete q;
}

}  // extern "C"
