// engine_impl.h — what the HIP-compiled host units behind the C ABI share (engine.cpp: lifetime and tables; pipeline.cpp: one batch
// through the launches; evaluate.cpp, evaluate_records.cpp: the entry points and their staging): the owners of device memory, a batch's
// scratch context, the engine itself. Internal: includes HIP, is included by those four units only, and nothing in here is exported.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.h"
#include "program_handle.h"
#include "scanplan.h"
#include "staging.h"
#include "tableplan.h"

#define HIP_TRY(expr)                                                                                              \
    do {                                                                                                           \
        hipError_t _e = (expr);                                                                                    \
        if (_e != hipSuccess) return pwaf::fail(PWAF_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

#pragma GCC visibility push(hidden)
namespace pwaf {

// The measurement switches of the batch path, read from the environment ONCE, and only by a -DPWAF_PROFILING build (tools/*.sh,
// docs/experiments/): every other build runs with the defaults written here. Timing experiments and debugging aids — several give
// wrong results; none is a product setting.
struct Switches {
    bool sync_each = false;           // PWAF_SYNC_EACH, debugging aid: wait after every launch and print how it ended (which launch faults)
    uint32_t debug_skip = 0;          // PWAF_DEBUG_SKIP: VerdictArgs::debug_skip
    bool attr_prio = false;           // PWAF_ATTR_PRIO: bit 31 of the same
    int placement = 2;                // PWAF_PLACEMENT=0..3, PWAF_ATTR_INLINE (= 1), PWAF_ATTR_EARLY (= 3): where the attribute path runs (BatchRun::ipres_stage)
    bool skip_ipres = false;          // PWAF_SKIP_IPRES, PWAF_SKIP_ATTR
    bool skip_attr = false;           // PWAF_SKIP_ATTR
    long list_shape = -1;             // PWAF_LIST_SHAPE = phase 0 | phase 1 << 4: the list scans' workgroup shapes (same results); -1: not given
    uint32_t filter_debug_skip = 0;   // PWAF_FILTER_DEBUG_SKIP: FilterArgs::debug
    bool attr_after_compact = false;  // PWAF_ATTR_AFTER_COMPACT: the attribute path forks behind resolve / compact instead of the prefilter
    bool dump_counts = false;         // PWAF_DUMP_COUNTS, debugging aid: the device-side list lengths of every batch
    bool skip_identity = false;       // PWAF_SKIP_IDENTITY: the identity passes are not walked
    bool side_priority_high = false;  // PWAF_SIDE_PRIORITY_HIGH: the side stream at the highest priority instead of the lowest
    bool no_packed_staging = false;   // PWAF_NO_PACKED_STAGING, A/B: the column-by-column path for every host batch
};
const Switches &switches();  // engine.cpp

// Device memory and its owner: move-only, freed when the owner goes (release(): the one table that is dropped early).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    int reserve(size_t bytes) {
        if (bytes <= cap) return PWAF_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) return fail(PWAF_E_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
        cap = want;
        return PWAF_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Page-locked host memory the device reads / writes directly: staging of small host batches, status words on their way back.
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    PinBuf(PinBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinBuf &operator=(PinBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~PinBuf() { release(); }
    int reserve(size_t bytes) {
        if (bytes <= cap) return PWAF_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 4 + 4096;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocPortable);
        if (e != hipSuccess) return fail(PWAF_E_NOMEM, std::string("hipHostMalloc failed: ") + hipGetErrorString(e));
        cap = want;
        return PWAF_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

template <class T>
int upload(DevBuf &b, const std::vector<T> &v, size_t pad_bytes = 0) {
    size_t bytes = v.size() * sizeof(T);
    int rc = b.reserve(bytes + pad_bytes + 16);
    if (rc) return rc;
    if (bytes) HIP_TRY(hipMemcpy(b.p, v.data(), bytes, hipMemcpyHostToDevice));
    if (pad_bytes + 16) HIP_TRY(hipMemset((char *)b.p + bytes, 0, pad_bytes + 16));
    return PWAF_OK;
}

// flat form of a DFA for list-driven walks (lscan_kernel): scanplan.h's FlatImage on the device (n_states == 0: not built)
struct FlatDev : FlatShape {
    DevBuf flat, flat_classmap, emit_off, emit_list, end_off, end_list, delta;
};

// One scan pass on the device: its streaming table (scanplan.h: ScanImage), its role (PassRole) and what the role needs
struct DevGroup : ScanShape, PassRole {
    DevBuf tab, classmap, special, list_off, list;
    uint32_t chunks = 1;  // 16-byte chunks per scan iteration (2 for fields whose sampled mean length is >= 48 bytes)
    GroupFilter filter;     // the prefilter in use (Program's, or rebuilt from a traffic sample by pwaf_engine_tune)
    DevBuf ftable;
    // flat form of the DFA for list-driven walks (lscan_kernel): of the pass's every atom (fl), and — a pass with a confirm tier and
    // atoms of both kinds — of its non-literal atoms alone (rt: DfaGroup::rtier), which is what confirmed candidates walk
    FlatDev fl, rt;
    // confirm tier in use (assign_lists uploads it with the filter table): ConfirmTable::head / entries / bytes / classes
    DevBuf c_head, c_entries, c_bytes, c_classes;
};

}  // namespace pwaf

// Everything one in-flight batch needs besides the immutable tables: device scratch, host-batch staging buffers, its own stream for
// the synchronous entry points, the side stream of the attribute kernel and the events that order them. An engine owns a small
// ring of these, so that callers on several threads / streams overlap (one batch's copies under another's kernels) instead of
// queueing behind one set of buffers; a context's `done` event makes its next user wait (on the device) for the previous one.
struct Scratch {
    using DevBuf = pwaf::DevBuf;
    using PinBuf = pwaf::PinBuf;
    std::mutex mu;  // held while a call enqueues on this context (device calls) or for the whole call (host batches: staging is reused)
    hipStream_t stream = nullptr, side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, done = nullptr;
    bool used = false;
    hipStream_t last = nullptr;  // the stream of the context's latest batch
    bool last_own = false;       // ... which was the context's own stream (a host batch)
    DevBuf status;            // one sticky word: bit 0 = some batch on this context exhausted the overflow pool (cleared when reported)
    uint64_t pool_entries = 0;  // overflow pool size in use (grown when a batch exhausted it)
    struct View { void *p = nullptr; };  // a part of zero_block / args (not owned)
    View res_cols;  // residual_kernel: the batch's string columns as device arrays of pointers
    bool retry = false;   // this run repeats a batch that exhausted the overflow pool: its residual rules' execution errors were counted by the first run
    DevBuf err_sink;      // ... and land here
    DevBuf ipres;  // ipres_kernel -> attr_kernel: (GeoIP class, membership set) of every request
    DevBuf rec, pool, gate_lists, attr;
    DevBuf verdict_spill;     // the sparse column file's per-wave spill arrays (kernels.h: VerdictArgs::spill)
    DevBuf res_words;  // specialized residual program: [words][n] match bits per (request, rule)
    // What a batch needs ZEROED lives in one block (one memset per batch instead of four): the control words ([0] pool allocator, [1]
    // status word, then one length per list slot and one pair count per filtered pass), the candidate bitmaps of the filtered passes,
    // the visited bitmaps of the gap passes and the walk bitmaps of the confirm tier.
    DevBuf zero_block;
    View ctrl, cand_bits, visit_bits, walk_bits;
    DevBuf chunk_bits, cand_cnt;  // filter_kernel's chunk bitmaps and per-slab counts
    std::vector<pwaf::FilterArgs> last_filter;  // the filter descriptors of the context's latest batch, for pwaf_engine_filter_flags (TEST HOOK; run_pipeline swaps them in)
    DevBuf need;                           // per sharing owner: gap-pass mask of every entry of its candidate list
    DevBuf pairs;                          // per filtered pass with a confirm tier: resolve_kernel's (request, flagged chunk) pairs
    DevBuf zero_off;                       // n + 1 zero offsets: the column of a header the batch does not carry
    // Launch descriptors of a batch (kernels.h: FilterArgs / ConfirmArgs / ListScanArgs per pass, the residual kernel's column pointers):
    // built on the host before the first launch and uploaded ONCE — the host writes them into a page-locked slot and one copy launch
    // on the batch's stream moves them to `args` (stream-ordered like the by-value store launches it replaces: a 4096-rule set over 64
    // header fields took 22 of those per batch). A slot is rewritten only after the copy launch that read it has run (its event);
    // with kArgSlots slots a caller can be that many batches ahead of the device before it has to wait.
    static constexpr uint32_t kArgSlots = 8;
    DevBuf args;
    PinBuf arg_slot[kArgSlots];
    hipEvent_t arg_ev[kArgSlots] = {};
    bool arg_pending[kArgSlots] = {};
    uint32_t arg_next = 0;
    std::vector<DevBuf> stage_field_data, stage_field_off;  // n_fields each
    DevBuf stage_ip, stage_v6, stage_port, stage_flags, stage_asn, stage_country, stage_out, stage_counts;
    DevBuf stage_route;  // a large host batch's routes on their way back (pwaf_evaluate_batch_routes)
    DevBuf stage_hits, stage_hit_counts;  // a host batch's rule hits on their way back (PWAF_OPT_RULE_HITS): the list; {n_hits, pad, rule_hits[n_rules]}
    DevBuf stage_geo;  // the GeoIP answers of a large host batch / a host pwaf_geoip_lookup on their way back (PWAF_OPT_GEO_ANSWERS)
    // A SMALL host batch (the micro-batcher's, pwaf_evaluate_one's) travels as ONE block: every column packed into page-locked memory,
    // one asynchronous copy in, one out (pwaf_evaluate_batch). pin_status: the status words on their way back (never a pageable target:
    // a device-to-host copy into pageable memory is a blocking staged copy).
    PinBuf pin_in, pin_out, pin_status;
    DevBuf packed;
    // pwaf_evaluate_records: rec_meta = [record offsets | column offsets | column places | counters, verdicts | the records' bytes] on the
    // device (rec_pin: its page-locked image up to the verdicts, and the records when the caller's memory is pageable), rec_cols = the
    // unpacked batch (column arenas, fixed columns), rec_back = counters and verdicts on their way back
    DevBuf rec_meta, rec_cols;
    PinBuf rec_pin, rec_back;
    // Streams and events are created on first use: every HIP stream takes a share of the few hardware queues of its priority
    // class, and a context (or its own stream) a caller never uses must not cost the caller's streams their concurrency (measured:
    // three idle contexts' streams made two caller streams share one queue — no overlap between two batches in flight).
    // The side stream (attribute kernel) is created at the LOWEST stream priority: priority classes have hardware queues of their
    // own, so it can never share a queue with the caller's (normal-priority) stream — when it did, the attribute kernel ran in
    // front of the prefilter instead of beside it (measured: +0.45 ms per 10M-request batch).
    int ensure(bool own_stream) {
        if (!side) {
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            if (pwaf::switches().side_priority_high) least = greatest;  // timing experiment
            if (hipStreamCreateWithPriority(&side, hipStreamNonBlocking, least) != hipSuccess || hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&ev_join, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess)
                return pwaf::fail(PWAF_E_DEVICE, "hipStreamCreate / hipEventCreate failed");
            for (hipEvent_t &ev : arg_ev)
                if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return pwaf::fail(PWAF_E_DEVICE, "hipEventCreate failed");
        }
        if (own_stream && !stream && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return pwaf::fail(PWAF_E_DEVICE, "hipStreamCreate failed");
        return PWAF_OK;
    }
    ~Scratch() {  // (the buffers free themselves)
        for (hipEvent_t ev : arg_ev)
            if (ev) (void)hipEventDestroy(ev);
        if (stream) (void)hipStreamDestroy(stream);
        if (side) (void)hipStreamDestroy(side);
        for (hipEvent_t ev : {ev_fork, ev_join, done})
            if (ev) (void)hipEventDestroy(ev);
    }
};
static constexpr size_t kContexts = 3;

struct pwaf_engine : pwaf::PlanShape, pwaf::PassShape {  // (the widths and counts of the planned tables: tableplan.h, scanplan.h)
    using DevBuf = pwaf::DevBuf;
    pwaf_program prog;
    int device = 0;
    std::vector<std::unique_ptr<Scratch>> ctx;  // kContexts
    size_t next_ctx = 0;
    std::vector<pwaf::DevGroup> groups;
    DevBuf num_atoms, bit_atoms /* (source word, bit) -> column */, trig_off, trig_rules, always_rules, country_luts /* transposed: [676][cc_words] */, rules, lits, set_masks;
    DevBuf lazy_atoms;  // (VerdictArgs::lazy)
    DevBuf short_atoms;  // (PassShape::n_short of them)
    DevBuf class_rows, dir_esc, leaf_root, geo_leaf_root;
    DevBuf iu_vals[2], iu_masks[2];
    DevBuf ip_root4, ip_root6, ip_nodes, geo_root4, geo_root6, geo_nodes, geo_recs;
    std::mutex mu;  // guards the context ring and table rebuilds (pwaf_engine_tune)
    std::mutex prof_mu;  // while profiling is on, calls enqueue one at a time: the event / timing tables below are per engine
    DevBuf residual_errors;  // per residual rule: requests whose evaluation ended in an execution error (accumulated; pwaf_engine_rule_errors)
    std::string residual_note;  // why the residual rules are interpreted although specialization was asked for (pwaf_engine_residual_fallback)
    pwaf::JitKernel residual_jit;  // the specialized residual program (residual_jit.cpp + rtc.cpp); function == nullptr: the rules are interpreted
    DevBuf rules_unrouted;  // engines with routes and PWAF_OPT_RULE_HITS: `rules` with the routes' literal lists emptied (a hit report names rules only)
    DevBuf residual_blob, geo_rec_root4, geo_rec_root6, geo_rec_nodes;  // residual rules: the program image; the GeoIP trie with RECORD leaves (client.asn / country values)
    DevBuf pass_base, colmask, dir24 /* build-time only: released once compressed */, dir_chunks, dir_vals, dir_summary;
    uint32_t dir_sum_shift = 0, dir_common = 0;  // (VerdictArgs::dir_summary)
    DevBuf dir_coarse;                           // (VerdictArgs::dir_coarse)
    uint32_t dir_coarse_shift = 0, dir_coarse_bytes = 0, dir_coarse_set = 0, dir_summary_set = 0;  // (.._set: bits set, pwaf_engine_coarse_tables)
    uint32_t dir_n_esc = 0, dir_n_vals = 0;      // (pwaf_engine_address_tables)
    // PWAF_OPT_GEO_ANSWERS: the RECORD of every request (georec_kernel). The record-leaf trie and the records are geo_rec_* / geo_recs
    // above (shared with the residual rules); the IPv4 table of record ids is the engine's own (csrc/georec.h)
    bool geo_answers = false;
    DevBuf georec_chunks, georec_vals, georec_summary;
    uint32_t georec_shift = 0, georec_common = 0, georec_n_esc = 0, georec_n_vals = 0;
    std::vector<double> mean_len;  // per field, from the tuning sample (0 = unknown)
    pwaf::ListPlan list_plan;  // the list-scan descriptors of every batch and the launch shapes (scanplan.h; assign_lists)
    DevBuf pass_table;                  // PassInfo per pass
    uint32_t n_fields = PWAF_N_FIELDS;  // 5 + header columns
    // profiling
    int profiling = 0;  // 0 off, 1 every kernel, 2 only the launches that stream request bytes (pwaf_engine_set_profiling)
    std::vector<hipEvent_t> ev;
    std::vector<pwaf_kernel_time> times;
    std::vector<std::pair<size_t, size_t>> time_ev;  // (begin, end) event index of each entry of `times`
    size_t n_timed = 0;
    uint32_t n_cus = 256;
};

namespace pwaf {

// ---- engine.cpp: the tables' part of the kernel arguments; what an entry point asks of its engine ----

// the trie part of the kernel arguments (shared by the per-batch pipeline and the one-off DIR-24 table build)
void set_trie_args(const pwaf_engine *e, VerdictArgs &v);
// the table part of georec_kernel's arguments (PWAF_OPT_GEO_ANSWERS engines)
void set_georec_args(const pwaf_engine *e, GeoRecArgs &g);
int need_geo_answers(const pwaf_engine *e, const char *fn);
int need_routes(const pwaf_engine *e, const char *fn);

// The opt-in report of a call beside its verdicts, where `out` lives: the rule hits (PWAF_OPT_RULE_HITS; include/pwaf.h: pwaf_evaluate_*_hits)
// OR the routes (engines with routes: pwaf_evaluate_*_routes) — one call answers one of them. All null = nothing asked for.
struct ReportOut {
    pwaf_rule_hit *hits = nullptr;
    uint32_t cap = 0;
    uint32_t *n_hits = nullptr;
    uint64_t *rule_hits = nullptr;
    uint32_t *route = nullptr;  // (engines with routes: pwaf_evaluate_*_routes; never together with the three above)
    bool hit_any() const { return hits || n_hits || rule_hits; }
    bool any() const { return hit_any() || route; }
};
int check_hit_args(const pwaf_engine *e, const char *fn, const ReportOut &h);

// ---- pipeline.cpp: one batch through the launches ----

// The scratch context of a call, locked. The batch will run on `caller` (device batches; NULL is HIP's default stream) or, with
// `own`, on the context's own stream (host batches). Preference: the context whose latest batch ran on the SAME stream (stream
// order already protects the buffers: a single-stream caller keeps using one context, and one context's worth of memory), then
// a fresh one, then the next of the ring — only in that last case must the stream wait (on the device) for the previous user.
// (Deliberately no "whichever context is idle by hipEventQuery": the choice must not depend on timing.)
Scratch &acquire_context(pwaf_engine *e, bool own, hipStream_t caller, std::unique_lock<std::mutex> &held, bool &must_wait);
// What a context remembers of its latest batch (acquire_context), and the event its next user waits for.
hipError_t mark_context_used(Scratch &S, hipStream_t s, bool own);
int device_error(const char *call, hipError_t he);

// Kernel times (pwaf_engine_set_profiling): HIP events on the launch stream. On the main stream the event that ends one kernel also
// starts the next (half the events; the few microseconds of launch gap or memset in between are charged to the later kernel).
// (evaluate calls are re-entrant, the timing tables are not — a profiled call holds prof_mu while it enqueues)
struct KernelTimer {
    pwaf_engine *e;
    hipStream_t stream;
    std::unique_lock<std::mutex> lock;
    size_t ev_i = 0;
    long last_main = -1;  // index of the last event recorded on `stream` during this call
    long open_begin = -1;
    bool streaming = false;  // the marks of a launch that streams request bytes (level 2 records no others)
    const bool sync_each = switches().sync_each;
    KernelTimer(pwaf_engine *e_, hipStream_t stream_) : e(e_), stream(stream_) {
        if (!e->profiling) return;
        lock = std::unique_lock<std::mutex>(e->prof_mu);
        ev_i = e->n_timed;
    }
    bool off() const { return !e->profiling || (e->profiling == 2 && !streaming); }
    int record(hipStream_t on);
    // `side`: the launch goes to that stream instead of the batch's
    int begin(hipStream_t side = nullptr);
    int end(const char *name, uint64_t alg_bytes, hipStream_t side = nullptr);
    void commit() { e->n_timed = ev_i; }
};

// One batch of device columns through every launch.
int run_pipeline(pwaf_engine *e, Scratch &S, const pwaf_batch &db /* device pointers */, pwaf_verdict *d_out, pwaf_counts *d_counts, uint32_t *d_match_idx,
                 uint32_t *d_n_matches, hipStream_t stream, bool totals_known = false, const std::vector<uint32_t> *col_begin = nullptr, bool sync_status = false,
                 pwaf_geo *d_geo = nullptr, const ReportOut *d_rep = nullptr);

// The synchronous entry points' batch on the context's own stream: runs the pipeline and waits ONCE — the status words travel back
// (into page-locked memory) behind the batch, together with whatever `after` enqueues (the verdicts on their way to the host). A batch
// that exhausted the overflow pool is run again, at most twice, with a pool of the size it asked for (the staged columns stay where
// they are). `counts_zero`: the first attempt's counters arrive zeroed (they are part of a staged block). Whatever fails, the stream is
// drained before the call returns: what was enqueued may still read the caller's buffers.
// (A template over `after`: the callers' lambdas are called in place, nothing is allocated per call.)
template <class After>
int run_with_retry(pwaf_engine *e, Scratch &S, const pwaf_batch &db, pwaf_verdict *d_out, pwaf_counts *d_counts, bool known, const std::vector<uint32_t> *begins, bool counts_zero,
                   After &&after, pwaf_geo *d_geo = nullptr, const ReportOut *d_rep = nullptr) {
    const hipStream_t s = S.stream;
    int r = S.pin_status.reserve(16);
    volatile uint32_t *const st = (volatile uint32_t *)S.pin_status.p;
    for (int attempt = 0;; attempt++) {
        hipError_t he = hipSuccess;
        if (!r && d_counts && !(counts_zero && attempt == 0) && (he = hipMemsetAsync(d_counts, 0, sizeof *d_counts, s)) != hipSuccess) r = device_error("hipMemsetAsync", he);
        // the rule hits are overwritten like the counters: zeroed before EVERY attempt, so that a batch run again is not counted twice
        if (!r && d_rep && d_rep->n_hits && (he = hipMemsetAsync(d_rep->n_hits, 0, 4, s)) != hipSuccess) r = device_error("hipMemsetAsync", he);
        if (!r && d_rep && d_rep->rule_hits && e->prog.p->n_user_rules && (he = hipMemsetAsync(d_rep->rule_hits, 0, (size_t)e->prog.p->n_user_rules * 8, s)) != hipSuccess)
            r = device_error("hipMemsetAsync", he);
        if (!r) {
            S.retry = attempt > 0;
            r = run_pipeline(e, S, db, d_out, d_counts, nullptr, nullptr, s, known, begins, true, d_geo, d_rep);
            S.retry = false;
        }
        if (!r) {
            he = hipMemcpyAsync((void *)&st[0], (uint32_t *)S.status.p + 1, 4, hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipMemcpyAsync((void *)&st[1], S.ctrl.p, 4, hipMemcpyDeviceToHost, s);  // overflow entries the batch asked for
            r = he != hipSuccess ? device_error("hipMemcpyAsync", he) : after();
        }
        const hipError_t re = mark_context_used(S, s, true), se = hipStreamSynchronize(s);
        if (r) return r;
        if (re != hipSuccess) return device_error("hipEventRecord", re);
        if (se != hipSuccess) return device_error("hipStreamSynchronize", se);
        if (!st[0]) return PWAF_OK;
        HIP_TRY(hipMemsetAsync((uint32_t *)S.status.p + 1, 0, 4, s));
        if (attempt >= 2 || st[1] >= 0x7FFFFFF0u) return fail(PWAF_E_NOMEM, "scan overflow pool exhausted: verdicts of this batch are incomplete");
        S.pool_entries = (uint64_t)st[1] + st[1] / 4 + 1024;
    }
}

// The device-side view of a batch whose columns the engine placed itself (a staged host batch, unpacked records): an ordinary DEVICE
// batch with every column's size known on the host.
struct DeviceBatch {
    pwaf_batch db{};
    std::vector<pwaf_strcol> hdr_cols;
    std::vector<uint32_t> hdr_bytes;
    DeviceBatch(uint32_t n, uint32_t n_fields) : hdr_cols(n_fields - PWAF_N_FIELDS, pwaf_strcol{nullptr, nullptr}), hdr_bytes(n_fields - PWAF_N_FIELDS, 0) {
        db.struct_size = sizeof db;
        db.n = n;
        db.memory = PWAF_MEM_DEVICE;
        db.n_headers = (uint32_t)hdr_cols.size();
        db.headers = hdr_cols.empty() ? nullptr : hdr_cols.data();
        db.header_bytes = hdr_bytes.empty() ? nullptr : hdr_bytes.data();
    }
    DeviceBatch(const DeviceBatch &) = delete;  // (db points into the vectors)
    void set_col(uint32_t f, const void *data, const void *offsets, uint32_t bytes) {
        const pwaf_strcol c{(const uint8_t *)data, (const uint32_t *)offsets};
        if (f < PWAF_N_FIELDS) {
            db.field[f] = c;
            db.field_bytes[f] = bytes;
        } else {
            hdr_cols[f - PWAF_N_FIELDS] = c;
            hdr_bytes[f - PWAF_N_FIELDS] = bytes;
        }
    }
    void set_fixed(const void *ip, const void *ip_is_v6, const void *port, const void *flags, const void *asn, const void *country) {
        db.ip = (const uint8_t *)ip;
        db.ip_is_v6 = (const uint8_t *)ip_is_v6;
        db.port = (const uint16_t *)port;
        db.flags = (const uint8_t *)flags;
        db.asn = (const uint32_t *)asn;
        db.country = (const uint16_t *)country;
    }
};

}  // namespace pwaf
#pragma GCC visibility pop
