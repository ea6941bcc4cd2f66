// engine.cpp — the C ABI of libpwaf.so (include/pwaf.h): engine lifetime, device tables, batch
// marshalling and the launch sequence. Construction mirrors where the reference builds its
// read-only rule state once (pingoo/server.rs:40-47,76) and hands it to every listener
// (server.rs:111-134); evaluation replaces the inline loop at http_listener.rs:196-264.
//
// There is NO CPU evaluation path in this library: without a working HIP device every evaluate call
// returns PWAF_E_DEVICE (the host may then fail open, as the reference does on rule errors —
// pingoo/rules.rs:41-45).
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "dirtable.h"
#include "georec.h"
#include "frontend.h"
#include "kernels.h"
#include "lscan_split.h"
#include "program.h"
#include "records.h"
#include "scanplan.h"
#include "tableplan.h"

using namespace pwaf;

struct pwaf_program {
    std::unique_ptr<Program> p;
    std::vector<uint8_t> dump;  // lazily built
    // what the list-scan hooks answer from (pwaf_program_flat_image, pwaf_program_list_scans): the profile of the latest tuning sample
    // (null: never tuned), the mean field lengths the samples so far left, and the plan built from them on the first call
    std::unique_ptr<TuneOut> tuned;
    std::vector<double> mean_len;
    std::unique_ptr<ProgramScans> scans;
    void keep_tuning(const TuneOut &T) {
        tuned.reset(new TuneOut(T));
        mean_len.resize(std::max(mean_len.size(), T.mean_len.size()), 0.0);
        for (size_t f = 0; f < T.mean_len.size(); f++)
            if (T.mean_len[f] > 0) mean_len[f] = T.mean_len[f];
        scans.reset();
        dump.clear();
    }
};

namespace {
thread_local std::string g_last_error = "";
}
namespace pwaf {
int fail(int code, const std::string &msg) {  // also used by loaders.cpp
    g_last_error = msg;
    return code;
}
}  // namespace pwaf
using pwaf::fail;
namespace {
#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t _e = (expr);                                                                                \
        if (_e != hipSuccess) return fail(PWAF_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

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
Switches read_switches() {
    Switches s;
#ifdef PWAF_PROFILING
    const auto set = [](const char *name) { return getenv(name) != nullptr; };
    s.sync_each = set("PWAF_SYNC_EACH");
    if (set("PWAF_DEBUG_SKIP")) s.debug_skip = (uint32_t)strtoul(getenv("PWAF_DEBUG_SKIP"), nullptr, 0);
    s.attr_prio = set("PWAF_ATTR_PRIO");
    s.placement = set("PWAF_PLACEMENT") ? atoi(getenv("PWAF_PLACEMENT")) : set("PWAF_ATTR_INLINE") ? 1 : set("PWAF_ATTR_EARLY") ? 3 : 2;
    s.skip_attr = set("PWAF_SKIP_ATTR");
    s.skip_ipres = set("PWAF_SKIP_IPRES") || s.skip_attr;
    if (set("PWAF_LIST_SHAPE")) s.list_shape = (long)(uint32_t)atoi(getenv("PWAF_LIST_SHAPE"));
    if (set("PWAF_FILTER_DEBUG_SKIP")) s.filter_debug_skip = (uint32_t)atoi(getenv("PWAF_FILTER_DEBUG_SKIP"));
    s.attr_after_compact = set("PWAF_ATTR_AFTER_COMPACT");
    s.dump_counts = set("PWAF_DUMP_COUNTS");
    s.skip_identity = set("PWAF_SKIP_IDENTITY");
    s.side_priority_high = set("PWAF_SIDE_PRIORITY_HIGH");
    s.no_packed_staging = set("PWAF_NO_PACKED_STAGING");
#endif
    return s;
}
const Switches &switches() {
    static const Switches sw = read_switches();
    return sw;
}

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

}  // namespace

// Everything one in-flight batch needs besides the immutable tables: device scratch, host-batch staging buffers, its own stream for
// the synchronous entry points, the side stream of the attribute kernel and the events that order them. An engine owns a small
// ring of these, so that callers on several threads / streams overlap (one batch's copies under another's kernels) instead of
// queueing behind one set of buffers; a context's `done` event makes its next user wait (on the device) for the previous one.
struct Scratch {
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
            if (switches().side_priority_high) least = greatest;  // timing experiment
            if (hipStreamCreateWithPriority(&side, hipStreamNonBlocking, least) != hipSuccess || hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&ev_join, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess)
                return fail(PWAF_E_DEVICE, "hipStreamCreate / hipEventCreate failed");
            for (hipEvent_t &ev : arg_ev)
                if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return fail(PWAF_E_DEVICE, "hipEventCreate failed");
        }
        if (own_stream && !stream && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return fail(PWAF_E_DEVICE, "hipStreamCreate failed");
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

struct pwaf_engine : PlanShape, PassShape {  // (the widths and counts of the planned tables: tableplan.h, scanplan.h)
    pwaf_program prog;
    int device = 0;
    std::vector<std::unique_ptr<Scratch>> ctx;  // kContexts
    size_t next_ctx = 0;
    std::vector<DevGroup> groups;
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
    JitKernel residual_jit;  // the specialized residual program (residual_jit.cpp + rtc.cpp); function == nullptr: the rules are interpreted
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
    ListPlan list_plan;  // the list-scan descriptors of every batch and the launch shapes (scanplan.h; assign_lists)
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

namespace {

int check_opts(const pwaf_options *o, pwaf_options &out) {
    memset(&out, 0, sizeof out);
    out.struct_size = sizeof out;
    out.device = -1;
    if (!o) return PWAF_OK;
    if (o->struct_size != sizeof(pwaf_options)) return fail(PWAF_E_INVALID_ARG, "pwaf_options.struct_size mismatch");
    out = *o;
    return PWAF_OK;
}

void put_err(pwaf_compile_error *dst, const pwaf_compile_error &src) {
    if (dst) *dst = src;
    g_last_error = src.message;
}

int validate_batch_header(const pwaf_batch *b) {
    if (!b) return fail(PWAF_E_INVALID_ARG, "batch is NULL");
    if (b->struct_size != sizeof(pwaf_batch)) return fail(PWAF_E_INVALID_ARG, "pwaf_batch.struct_size mismatch");
    if (b->memory != PWAF_MEM_HOST && b->memory != PWAF_MEM_DEVICE) return fail(PWAF_E_INVALID_ARG, "pwaf_batch.memory is neither HOST nor DEVICE");
    if (b->n == 0) return PWAF_OK;
    for (int f = 0; f < PWAF_N_FIELDS; f++)
        if (!b->field[f].data || !b->field[f].offsets) return fail(PWAF_E_INVALID_ARG, "pwaf_batch.field column is NULL");
    if (!b->ip || !b->ip_is_v6 || !b->port || !b->flags) return fail(PWAF_E_INVALID_ARG, "pwaf_batch numeric column is NULL");
    if ((b->asn == nullptr) != (b->country == nullptr)) return fail(PWAF_E_INVALID_ARG, "pwaf_batch.asn and .country must be given together");
    return PWAF_OK;
}

// the trie part of the kernel arguments (shared by the per-batch pipeline and the one-off DIR-24 table build)
void set_trie_args(const pwaf_engine *e, VerdictArgs &v) {
    const Program &P = *e->prog.p;
    // a family without prefixes walks an all-leaf root: the kernels never test the pointers
    const uint32_t *leaf = (const uint32_t *)e->leaf_root.p;
    v.ip_root4 = P.ipset_trie.root4.empty() ? leaf : (const uint32_t *)e->ip_root4.p;
    v.ip_root6 = P.ipset_trie.root6.empty() ? leaf : (const uint32_t *)e->ip_root6.p;
    v.ip_nodes = (const uint32_t *)e->ip_nodes.p;
    v.set_masks = (const uint32_t *)e->set_masks.p;
    v.set_words = P.set_words;
    v.n_ip_lists = P.n_ip_lists;
    const uint32_t *geo_leaf = (const uint32_t *)e->geo_leaf_root.p;
    v.geo_root4 = P.geo_trie.root4.empty() ? geo_leaf : (const uint32_t *)e->geo_root4.p;
    v.geo_root6 = P.geo_trie.root6.empty() ? geo_leaf : (const uint32_t *)e->geo_root6.p;
    v.geo_nodes = (const uint32_t *)e->geo_nodes.p;
    v.has_geo = P.has_geo ? 1u : 0u;
    v.dir24 = (const uint32_t *)e->dir24.p;
    v.dir_chunks = (const uint32_t *)e->dir_chunks.p;
    v.dir_vals = (const uint32_t *)e->dir_vals.p;
    v.dir_esc = (const uint2 *)e->dir_esc.p;
    v.dir_summary = (const uint32_t *)e->dir_summary.p;
    v.dir_sum_shift = e->dir_sum_shift;
    v.dir_common = e->dir_common;
    v.dir_coarse = (const uint32_t *)e->dir_coarse.p;
    v.dir_coarse_shift = e->dir_coarse_shift;
    v.dir_coarse_bytes = e->dir_coarse_bytes;
    v.class_rows = (const uint32_t *)e->class_rows.p;
    v.class_words = e->class_words;
    v.acmp_words = e->acmp_words;
    v.geo_default = e->geo_default;
    const size_t n_sets = P.set_words ? P.set_masks.size() / P.set_words : 1;
    v.ipres_packed = (e->n_classes <= 65536u && n_sets <= 65536u) ? 1u : 0u;
}

// the table part of georec_kernel's arguments (PWAF_OPT_GEO_ANSWERS engines)
void set_georec_args(const pwaf_engine *e, GeoRecArgs &g) {
    g.has_geo = e->prog.p->has_geo ? 1u : 0u;
    g.root4 = (const uint32_t *)e->geo_rec_root4.p;
    g.root6 = (const uint32_t *)e->geo_rec_root6.p;
    g.nodes = (const uint32_t *)e->geo_rec_nodes.p;
    g.recs = (const GeoRec *)e->geo_recs.p;
    g.chunks = (const uint32_t *)e->georec_chunks.p;
    g.vals = (const uint32_t *)e->georec_vals.p;
    g.summary = (const uint32_t *)e->georec_summary.p;
    g.sum_shift = e->georec_shift;
    g.common = e->georec_common;
    g.n_cus = e->n_cus;
}
int need_geo_answers(const pwaf_engine *e, const char *fn) {
    if (e->geo_answers) return PWAF_OK;
    return fail(PWAF_E_UNSUPPORTED, std::string(fn) + ": the engine was not created with PWAF_OPT_GEO_ANSWERS");
}

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
int need_routes(const pwaf_engine *e, const char *fn) {
    if (e->prog.p->n_routes) return PWAF_OK;
    return fail(PWAF_E_UNSUPPORTED, std::string(fn) + ": the engine was created without routes (pwaf_engine_create_routed)");
}
int check_hit_args(const pwaf_engine *e, const char *fn, const ReportOut &h) {
    if (!h.any()) return PWAF_OK;
    if (!(e->prog.p->flags & PWAF_OPT_RULE_HITS)) return fail(PWAF_E_UNSUPPORTED, std::string(fn) + ": the engine was not created with PWAF_OPT_RULE_HITS");
    if ((h.hits == nullptr) != (h.n_hits == nullptr)) return fail(PWAF_E_INVALID_ARG, std::string(fn) + ": hits and n_hits must be given together");
    return PWAF_OK;
}

// The scratch context of a call, locked. The batch will run on `caller` (device batches; NULL is HIP's default stream) or, with
// `own`, on the context's own stream (host batches). Preference: the context whose latest batch ran on the SAME stream (stream
// order already protects the buffers: a single-stream caller keeps using one context, and one context's worth of memory), then
// a fresh one, then the next of the ring — only in that last case must the stream wait (on the device) for the previous user.
// (Deliberately no "whichever context is idle by hipEventQuery": the choice must not depend on timing.)
Scratch &acquire_context(pwaf_engine *e, bool own, hipStream_t caller, std::unique_lock<std::mutex> &held, bool &must_wait) {
    must_wait = false;
    for (int pass = 0; pass < 2; pass++)
        for (auto &c : e->ctx) {
            std::unique_lock<std::mutex> l(c->mu, std::try_to_lock);
            if (!l.owns_lock()) continue;
            const bool ok = pass == 0 ? (c->used && (own ? c->last_own : (!c->last_own && c->last == caller))) : !c->used;
            if (ok) { held = std::move(l); return *c; }
        }
    size_t k;
    {
        std::lock_guard<std::mutex> lock(e->mu);
        k = e->next_ctx;
        e->next_ctx = (e->next_ctx + 1) % e->ctx.size();
    }
    held = std::unique_lock<std::mutex>(e->ctx[k]->mu);
    must_wait = e->ctx[k]->used;
    return *e->ctx[k];
}

// ---- one batch through the pipeline: run_pipeline at the end of this section is the driver, BatchRun holds the
//      steps ----

// Parts of one block (the zeroed block, the descriptor block, the staging blocks of the host entry points), each on a 256-byte boundary.
struct Layout {
    size_t used = 0;
    size_t take(size_t bytes) { const size_t at = used; used = (used + bytes + 255) & ~(size_t)255; return at; }
    size_t size() const { return used; }
};

// Slabs a filter pass streams: its arena cut into kStreamSlab pieces, less the whole slabs in front of the batch's own bytes.
uint32_t slab_count(uint32_t total, uint32_t slab0) { return (uint32_t)(((uint64_t)total + kStreamSlab - 1) / kStreamSlab) - slab0; }
uint32_t slabs_of(const FilterArgs &f) { return slab_count(f.total, f.slab0); }
// (request, flagged chunk) pairs of a pass with a confirm tier: at most one per chunk of the arena plus one per request (a chunk that
// straddles two requests counts for both)
uint32_t pair_cap_of(uint32_t slabs, uint32_t n) { return (uint32_t)std::min<uint64_t>(0xFFFFFFF0u, (uint64_t)slabs * (kStreamSlab / 16) + n + 64); }

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
    int record(hipStream_t on) {
        if (e->ev.size() < ev_i + 1) {
            hipEvent_t x;
            HIP_TRY(hipEventCreate(&x));
            e->ev.push_back(x);
        }
        HIP_TRY(hipEventRecord(e->ev[ev_i], on));
        ev_i++;
        return PWAF_OK;
    }
    // `side`: the launch goes to that stream instead of the batch's
    int begin(hipStream_t side = nullptr) {
        if (off()) return PWAF_OK;
        if (!side && last_main >= 0) { open_begin = last_main; return PWAF_OK; }
        const int rc = record(side ? side : stream);
        if (rc) return rc;
        open_begin = (long)ev_i - 1;
        if (!side) last_main = open_begin;
        return PWAF_OK;
    }
    int end(const char *name, uint64_t alg_bytes, hipStream_t side = nullptr) {
        if (sync_each) {
            hipError_t se = hipStreamSynchronize(side ? side : stream);
            fprintf(stderr, "[pwaf] %s done: %s\n", name, hipGetErrorString(se));
        }
        if (off()) return PWAF_OK;
        const int rc = record(side ? side : stream);
        if (rc) return rc;
        if (!side) last_main = (long)ev_i - 1;
        pwaf_kernel_time t{};
        snprintf(t.name, sizeof t.name, "%s", name);
        t.alg_bytes = alg_bytes;
        e->times.push_back(t);
        e->time_ev.push_back({(size_t)open_begin, ev_i - 1});
        return PWAF_OK;
    }
    void commit() { e->n_timed = ev_i; }
};

// The page-locked descriptor slot a batch wrote (Scratch::arg_slot): it may be rewritten only after the copy launch that read it has
// run, so WHATEVER way the batch leaves the pipeline its event is recorded behind what was enqueued. A batch that enqueued everything
// records it itself (record(): after the verdict launch — a record between two kernels keeps the second from starting while the first
// drains); every other exit leaves it to the destructor.
struct ArgSlotMark {
    Scratch &S;
    hipStream_t stream;
    int slot = -1;
    int record() {
        if (slot < 0) return PWAF_OK;
        const int k = slot;
        slot = -1;
        S.arg_pending[k] = true;  // (an event whose record failed reads as complete: the next user of the slot does not wait)
        HIP_TRY(hipEventRecord(S.arg_ev[k], stream));  // (the copy launch that read the slot ran before everything recorded here)
        return PWAF_OK;
    }
    ~ArgSlotMark() { (void)record(); }
};

struct BatchRun {
    pwaf_engine *e;
    Scratch &S;
    const Program &P;
    const pwaf_batch &db;  // device pointers
    hipStream_t stream;
    const std::vector<uint32_t> *col_begin;  // per field, where the batch's own bytes begin in the arena (a slab view of a larger batch); null: at 0
    const Switches &sw;
    KernelTimer prof;
    ArgSlotMark arg_slot;
    uint32_t n, n_groups, residual_pass, n_passes, bit_words, pair_stride;
    size_t n_slots, ctrl_words;
    uint32_t pool_cap = 0;
    uint32_t *status_word = nullptr;
    bool zero_deferred = false;  // the zeroed block is cleared by the descriptor upload's launch
    size_t zero_bytes = 0;
    std::vector<pwaf_strcol> cols;
    std::vector<uint32_t> col_bytes;  // arena sizes (0 = not known yet: learn_arena_sizes)
    std::vector<uint8_t> col_known;
    VerdictArgs v{};
    bool ipres_launched = false, attr_launched = false;
    pwaf_geo *d_geo = nullptr;  // PWAF_OPT_GEO_ANSWERS: where the batch's GeoIP records go (null: none asked for, nothing launched)
    const ListShape *lshapes = nullptr;  // (the shape is per PHASE: the filtered passes' candidate lists are long, the gap passes' short — scanplan.h: pick_list_shapes)
    // the descriptors of every launch of the batch (prefilter, resolve, confirm tier, list scans, residual kernel): built on the host,
    // uploaded ONCE
    std::vector<uint32_t> filter_index;  // a filtered pass's index among the filtered passes (its candidate / valid bitmap)
    std::vector<FilterArgs> fall;        // every filtered pass, in pass order
    std::vector<FilterArgs> by_stride[2];
    std::vector<ConfirmArgs> call;
    std::vector<ListScanArgs> la[2];
    ColPtrChunk ptrs{};  // residual kernel: the batch's string columns as arrays of pointers
    uint64_t alg_bytes[3] = {0, 0, 0};  // per sampling stride
    // ... and where they live in Scratch::args, with the work-item plans the plan kernels write behind them
    const FilterArgs *d_all = nullptr, *d_s1 = nullptr, *d_s2 = nullptr;
    const ConfirmArgs *d_c = nullptr;
    const ListScanArgs *d_la[2] = {nullptr, nullptr};
    uint32_t *c_plan = nullptr, *l_plan = nullptr;

    BatchRun(pwaf_engine *e_, Scratch &S_, const pwaf_batch &db_, hipStream_t stream_, const std::vector<uint32_t> *col_begin_)
        : e(e_), S(S_), P(*e_->prog.p), db(db_), stream(stream_), col_begin(col_begin_), sw(switches()), prof(e_, stream_), arg_slot{S_, stream_} {
        lshapes = e->list_plan.shapes;
        n = db.n;
        n_groups = (n + 63) / 64;
        residual_pass = (uint32_t)e->groups.size() + (P.fcmp.empty() ? 0u : 1u);
        n_passes = residual_pass + (P.n_residual ? 1u : 0u);  // (+ the pseudo passes of the field-against-field atoms and of the residual rules)
        // visited bitmaps of the list-driven passes (one bit per request, whole 64-request groups): zeroed per batch — 1/32 of what
        // zeroing the hit records themselves would write. They share ONE zeroed block with the control words and the confirm tier's walk bitmaps.
        bit_words = 2 * n_groups;
        // the attribute kernel's output: per group a header and room for EVERY non-scan atom (worst case: no overflow path)
        pair_stride = std::max(1u, e->n_bit_atoms + e->n_cmp_atoms + e->n_short);
        n_slots = (size_t)std::max(kGapLists, e->n_gated);
        ctrl_words = 2 + n_slots + e->n_filtered;  // [0] pool allocator, [1] status word, one length per list slot, one pair count per filtered pass
    }

    // ---- scratch, columns, the verdict kernel's arguments ----

    int reserve_scratch(bool sync_status) {
        int rc;
        // scratch sized for the worst case the 288 GB part can afford: one 4-byte hit record per (pass, request) and an overflow
        // pool of 8 entries per request (exhaustion is reported through the status word, never silently)
        // (a batch that exhausts the pool sets the context's sticky status word; the synchronous entry points then grow the pool to
        // what the batch asked for — the allocator keeps counting past the cap — and run the batch again)
        const uint64_t pool_cap64 = std::max<uint64_t>(std::max<uint64_t>(1u << 20, (uint64_t)n * 8), S.pool_entries);
        pool_cap = (uint32_t)std::min<uint64_t>(pool_cap64, 0x7FFFFFF0u);
        S.pool_entries = pool_cap;
        // two sticky status words per context: [0] device-resident batches (reported and cleared by pwaf_engine_device_status),
        // [1] the synchronous entry points (read and cleared by their own retry loop) — a synchronous batch on the same context can no
        // longer swallow the overflow bit of an earlier asynchronous one
        if (!S.status.p) {
            if ((rc = S.status.reserve(8))) return rc;
            HIP_TRY(hipMemsetAsync(S.status.p, 0, 8, stream));
        }
        status_word = (uint32_t *)S.status.p + (sync_status ? 1 : 0);
        if ((rc = S.rec.reserve((size_t)std::max(1u, n_passes) * n * 4))) return rc;
        // (attr: plus 64 pairs of slack so the verdict kernel may read a full wave's worth unconditionally)
        if ((rc = S.attr.reserve(((size_t)n_groups * pair_stride + 64) * 16 + (size_t)n_groups * 4))) return rc;
        if ((rc = S.pool.reserve((size_t)pool_cap * sizeof(PoolEntry)))) return rc;
        uint32_t n_conf = 0;
        for (const DevGroup &d : e->groups) n_conf += (d.filtered && d.confirm) ? 1u : 0u;
        Layout z;
        const size_t z_ctrl = z.take(4 * ctrl_words), z_cand = z.take((size_t)e->n_filtered * bit_words * 4), z_visit = z.take((size_t)e->n_visit * bit_words * 4),
                     z_walk = z.take((size_t)n_conf * bit_words * 4);
        zero_bytes = z.size();
        if ((rc = S.zero_block.reserve(zero_bytes))) return rc;
        // (cleared by the descriptor upload's launch when nothing needs it before that: no pass that streams every request — those run first and
        // count into the control words)
        zero_deferred = e->n_filtered != 0;
        for (const DevGroup &d : e->groups) zero_deferred = zero_deferred && (d.gate >= 0 || d.identity || d.short_lit);
        if (!zero_deferred) HIP_TRY(hipMemsetAsync(S.zero_block.p, 0, zero_bytes, stream));
        char *const zbase = (char *)S.zero_block.p;
        S.ctrl.p = zbase + z_ctrl;
        S.cand_bits.p = zbase + z_cand;
        S.visit_bits.p = zbase + z_visit;
        S.walk_bits.p = zbase + z_walk;
        if (e->n_gated && (rc = S.gate_lists.reserve((size_t)e->n_gated * n * 4))) return rc;
        if (e->n_need && (rc = S.need.reserve((size_t)e->n_need * n * 4))) return rc;
        return PWAF_OK;
    }

    // string columns by field id: the five fixed fields, then one column per header name the rule set mentions (EXTENSION); a header
    // the batch does not carry reads as the empty string for every request
    int resolve_columns(bool totals_known) {
        int rc;
        cols.resize(e->n_fields);
        col_bytes.assign(e->n_fields, 0);
        for (int f = 0; f < PWAF_N_FIELDS; f++) {
            cols[(size_t)f] = db.field[f];
            col_bytes[(size_t)f] = db.field_bytes[f];
        }
        bool missing_header = false;
        for (uint32_t f = PWAF_N_FIELDS; f < e->n_fields; f++) {
            const uint32_t k = f - PWAF_N_FIELDS;
            if (k < db.n_headers && db.headers != nullptr && db.headers[k].data != nullptr && db.headers[k].offsets != nullptr) {
                cols[f] = db.headers[k];
                col_bytes[f] = db.header_bytes ? db.header_bytes[k] : 0u;
            } else {
                missing_header = true;
            }
        }
        if (missing_header) {
            if (S.zero_off.cap < (size_t)(n + 1) * 4 + PWAF_ARENA_PAD) {
                if ((rc = S.zero_off.reserve((size_t)(n + 1) * 4 + PWAF_ARENA_PAD))) return rc;
                HIP_TRY(hipMemsetAsync(S.zero_off.p, 0, S.zero_off.cap, stream));
            }
            for (uint32_t f = PWAF_N_FIELDS; f < e->n_fields; f++)
                if (cols[f].data == nullptr) {
                    cols[f].data = (const uint8_t *)S.zero_off.p;
                    cols[f].offsets = (const uint32_t *)S.zero_off.p;
                    col_bytes[f] = 0;
                }
        }
        col_known.assign(e->n_fields, totals_known ? 1 : 0);
        for (uint32_t f = 0; f < e->n_fields; f++)
            if (col_bytes[f] != 0 || cols[f].data == (const uint8_t *)S.zero_off.p) col_known[f] = 1;
        return PWAF_OK;
    }

    int fill_verdict_args(pwaf_verdict *d_out, pwaf_counts *d_counts, uint32_t *d_match_idx, uint32_t *d_n_matches) {
        int rc;
        v.n = n;
        v.n_groups = n_groups;
        v.force_global_tables = (P.flags & PWAF_OPT_GLOBAL_VERDICT_TABLES) ? 1u : 0u;
        v.sparse_mode = verdict_mode(P.flags);
        if (v.sparse_mode) {
            // >= 3, the entry list: entries per wave in LDS, and the per-wave spill array (by column) for a group that appends more;
            // else the sparse column file: value slots per wave, and the spill array for a group that dirties more columns than that
            const VerdictShape vs = verdict_shape(P.n_cols, (uint32_t)P.rules.size(), e->n_trig, (uint32_t)P.lits.size(), v.force_global_tables != 0, (int)v.sparse_mode, n_passes);
            v.v_cap = vs.v_cap;
            const bool entry_list = v.sparse_mode >= 3;
            const uint32_t spill_cols = entry_list ? P.n_cols : P.n_cols - std::min(vs.v_cap, P.n_cols);
            if (entry_list || spill_cols) {
                if ((rc = S.verdict_spill.reserve((size_t)verdict_blocks_sp(vs, e->n_cus) * vs.waves * spill_cols * 8))) return rc;
                v.spill = (unsigned long long *)S.verdict_spill.p;
            }
        }
        v.debug_skip = sw.debug_skip | (sw.attr_prio ? 0x80000000u : 0u);  // timing experiments only: results are wrong when non-zero
        for (int f = 0; f < PWAF_N_FIELDS; f++) v.off[f] = db.field[f].offsets;
        v.ip = db.ip;
        v.ip_is_v6 = db.ip_is_v6;
        v.port = db.port;
        v.flags = db.flags;
        v.asn = db.asn;
        v.country = db.country;
        v.n_cols = P.n_cols;
        v.n_passes = n_passes;
        v.rec = (const uint32_t *)S.rec.p;
        v.passes = (const PassInfo *)e->pass_table.p;
        if (P.n_residual && e->residual_jit.function) {
            v.res_words = (P.n_residual + 31u) / 32u;
            v.res_base = P.residual_base;
            if ((rc = S.res_words.reserve((size_t)v.res_words * n * 4))) return rc;
            v.res_match = (const uint32_t *)S.res_words.p;
        }
        v.cand_bits = (const uint32_t *)S.cand_bits.p;
        v.visit_bits = (const uint32_t *)S.visit_bits.p;
        v.bit_words = bit_words;
        v.n_hlen = (uint32_t)e->hlen_fields.size();
        for (size_t k = 0; k < e->hlen_fields.size(); k++) v.hoff[k] = cols[e->hlen_fields[k]].offsets;
        v.gpairs = (uint4 *)S.attr.p;
        v.ghdr = (uint32_t *)((char *)S.attr.p + ((size_t)n_groups * pair_stride + 64) * 16);
        v.pair_stride = pair_stride;
        v.attr_blocks = e->n_cus;
        v.pool = (const PoolEntry *)S.pool.p;
        v.cmp = (const CmpAtomDev *)e->num_atoms.p;
        v.n_cmp = e->n_cmp_atoms;
        v.cmp_vars = e->cmp_vars;
        v.lazy = (const CmpAtomDev *)e->lazy_atoms.p;
        v.n_lazy = e->n_lazy;
        v.n_lazy_var = (uint32_t)e->lazy_vars.size();
        for (size_t k = 0; k < e->lazy_vars.size(); k++) v.lazy_var[k] = e->lazy_vars[k];
        v.n_short = e->n_short;
        v.short_atoms = (const ShortAtom *)e->short_atoms.p;
        if (e->n_short) {
            v.short_data = cols[(size_t)e->short_field].data;
            v.short_off = cols[(size_t)e->short_field].offsets;
        }
        v.n_trig = e->n_trig;
        v.n_lits = (uint32_t)P.lits.size();
        v.bit_col = (const uint32_t *)e->bit_atoms.p;
        v.trig_off = (const uint32_t *)e->trig_off.p;
        v.trig_rules = (const uint16_t *)e->trig_rules.p;
        v.always_rules = (const uint32_t *)e->always_rules.p;
        for (int var = 0; var < 2; var++) {
            v.iu_vals[var] = (const int64_t *)e->iu_vals[var].p;
            v.iu_masks[var] = (const uint32_t *)e->iu_masks[var].p;
            v.iu_n[var] = e->iu_n[var];
            v.iu_words[var] = e->iu_words[var];
        }
        v.country_masks = (const uint32_t *)e->country_luts.p;
        v.cc_words = e->cc_words;
        v.rules = (const DevRule *)e->rules.p;
        v.n_rules = (uint32_t)P.rules.size();
        v.lits = (const uint32_t *)e->lits.p;
        set_trie_args(e, v);
        if ((rc = S.ipres.reserve((size_t)n * (v.ipres_packed ? 4 : 8) + 64))) return rc;
        v.ipres = (uint32_t *)S.ipres.p;
        v.out = d_out;
        v.counts = (unsigned long long *)d_counts;
        v.match_idx = d_match_idx;
        v.n_matches = d_n_matches;
        return PWAF_OK;
    }

    // A pass with heads has records outside its candidate list too, read densely: filter_kernel stores the record of EVERY request of such
    // a pass, zero included (it visits each request's start once anyway; until then a memset of n x 4 bytes per pass stood in front of
    // every batch's descriptor upload: 7.6 us for 10M requests). (A confirm tier MERGES hits into zeroed records: resolve_kernel zeroes
    // the records of the requests that have a flagged chunk — the only ones a hit can land in.) What is left for the host is the pass
    // the launch has no wave for — an arena without a slab of its own (every field of the batch empty) — and, in profiling builds, the
    // "no heads" timing switch, which stores no record at all. Called once the arena sizes are known.
    int zero_head_records() {
        for (size_t k = 0; k < e->groups.size(); k++) {
            const DevGroup &d = e->groups[k];
            if (!d.filtered || d.filter.heads.empty()) continue;
            if (slab_count(col_bytes[d.field], slab0_of(d.field)) != 0 && !(sw.filter_debug_skip & 4u)) continue;
            HIP_TRY(hipMemsetAsync((uint32_t *)S.rec.p + k * (size_t)n, 0, (size_t)n * 4, stream));
        }
        return PWAF_OK;
    }

    // ---- launching ----

    // One launch between its two marks. `what` names it in the error text; `side`: it goes to that stream instead of the batch's.
    template <class Launch>
    int timed(const char *name, uint64_t bytes, const char *what, Launch &&launch, hipStream_t side = nullptr) {
        const int rc = prof.begin(side);
        if (rc) return rc;
        const int he = launch();
        if (he) return fail(PWAF_E_DEVICE, std::string(what) + " launch failed: " + hipGetErrorString((hipError_t)he));
        return prof.end(name, bytes, side);
    }

    // The attribute path — ipres_kernel (address lookups: one scattered 16-byte gather per request, bound by the texture addresser) and
    // attr_kernel (rows, transposes, comparisons: bound by vector-ALU issue) — does not depend on the scans. Placement (measured on
    // MI355X, 10M requests; `PWAF_PLACEMENT` in profiling builds, every other build takes 2: Switches::placement):
    //   0  ipres on the side stream from the START of the batch, attr_kernel on the main stream after the prefilter    1.838 ms / step
    //   1  both on the main stream after the prefilter (every kernel alone)                                              1.861
    //   2  both on the side stream, forked after the prefilter                                        <- default          1.779
    //   3  both on the side stream from the start                                                                         1.762
    // 3 is 1 % faster than 2 but slows the prefilter launch itself from 0.73 to 0.95 ms (0 to 0.86): the streaming kernel is what the
    // roofline is quoted on, so it runs undisturbed.
    // Kernels that run beside each other take about as long as one after the other here (the step is the SUM of what its kernels
    // cost alone, give or take 2 %), so the placement only matters where the two really use different units.
    // One of the two kernels on `q`: the batch's stream, or the side stream, which then leaves ev_join behind for join_side.
    template <class Launch>
    int side_stage(hipStream_t q, const char *name, uint64_t code, const char *what, Launch &&launch) {
        const hipStream_t side = q != stream ? q : nullptr;
        const int rc = timed(name, code, what, launch, side);
        if (rc) return rc;
        if (side) HIP_TRY(hipEventRecord(S.ev_join, q));
        return PWAF_OK;
    }
    int ipres_stage(hipStream_t q) {
        if (ipres_launched) return PWAF_OK;
        ipres_launched = true;
        if (q != stream) {  // fork: the side stream starts behind what the batch has enqueued so far
            HIP_TRY(hipEventRecord(S.ev_fork, stream));
            HIP_TRY(hipStreamWaitEvent(q, S.ev_fork, 0));
        }
        // (PWAF_SKIP_IPRES, timing experiments only: every address resolves to class 0 / set 0)
        const int rc = side_stage(q, "ipres", 0xFAu, "ipres kernel", [&] { return sw.skip_ipres ? (int)hipMemsetAsync(v.ipres, 0, (size_t)n * (v.ipres_packed ? 4 : 8), q) : launch_ipres(v, q); });
        if (rc || !d_geo) return rc;
        // the GeoIP answers: beside the address lookups, on the same stream (the side stream's join covers both)
        GeoRecArgs ga{};
        set_georec_args(e, ga);
        ga.ip = db.ip;
        ga.ip_is_v6 = db.ip_is_v6;
        ga.asn = db.asn;
        ga.country = db.country;
        ga.n = n;
        ga.out = (uint2 *)d_geo;
        return side_stage(q, "georec", 25ull * n, "georec kernel", [&] { return launch_georec(ga, q); });
    }
    int attr_stage(hipStream_t q) {
        if (attr_launched) return PWAF_OK;
        attr_launched = true;
        if (q == stream && sw.placement == 0) HIP_TRY(hipStreamWaitEvent(stream, S.ev_join, 0));  // the side stream's ipres results
        // (PWAF_SKIP_ATTR, timing experiments only: every non-scan predicate reads false)
        return side_stage(q, "attr", 0xFEu, "attribute kernel", [&] { return sw.skip_attr ? (int)hipMemsetAsync(v.ghdr, 0, (size_t)n_groups * 4, q) : launch_attr(v, q); });
    }
    // batch start: what forks here
    int attr_at_start() {
        int rc;
        if (sw.placement == 0) return ipres_stage(S.side);
        if (sw.placement == 3) return (rc = ipres_stage(S.side)) ? rc : attr_stage(S.side);
        return PWAF_OK;
    }
    // after the prefilter (or, without one, before the list scans); what has been launched is not launched again
    int attr_after_filter() {
        int rc;
        switch (sw.placement) {
        case 0: return attr_stage(stream);
        case 1: return (rc = ipres_stage(stream)) ? rc : attr_stage(stream);
        case 2: return (rc = ipres_stage(S.side)) ? rc : attr_stage(S.side);
        default: return PWAF_OK;
        }
    }
    // before the verdict kernel
    int join_side() {
        if (sw.placement >= 2) HIP_TRY(hipStreamWaitEvent(stream, S.ev_join, 0));  // (the attribute kernel ran on the side stream)
        return PWAF_OK;
    }

    // ---- 1. plain passes: the DFA walks every request (short fields go through the list-scan kernel below) ----
    int launch_plain_scans() {
        static const char *fn[5] = {"host", "url", "path", "method", "user_agent"};
        for (size_t gi = 0; gi < e->groups.size(); gi++) {
            const DevGroup &d = e->groups[gi];
            if (d.gate >= 0 || d.identity || d.short_lit) continue;
            const ScanArgs a = scan_args(gi);
            char nm[48];
            if (d.field < PWAF_N_FIELDS) snprintf(nm, sizeof nm, "scan_%s_g%zu", fn[d.field], gi);
            else snprintf(nm, sizeof nm, "scan_hdr%u_g%zu", d.field - PWAF_N_FIELDS, gi);
            prof.streaming = true;
            // algorithmic bytes: the field's bytes + its offsets (0 bytes when the arena size is unknown)
            const int rc = timed(nm, (uint64_t)col_bytes[d.field] + 4ull * (n + 1), "scan kernel", [&] { return launch_scan(a, stream); });
            prof.streaming = false;
            if (rc) return rc;
        }
        return PWAF_OK;
    }

    // ---- 2a. bigram prefilters of every filtered pass in one launch (the arenas as flat byte streams), hit segments -> candidate
    //          bitmaps / pair lists ----
    int launch_filter_stage() {
        prof.streaming = true;
        // algorithmic bytes: every streamed arena once + its offsets. The mark's name tells the bench which strides the launch mixed.
        const int rc = timed(by_stride[1].empty() ? "filter_s1" : by_stride[0].empty() ? "filter_s2" : "filter_mix", alg_bytes[1] + alg_bytes[2], "filter kernel", [&] {
            return launch_filter(by_stride[0].data(), (uint32_t)by_stride[0].size(), d_s1, by_stride[1].data(), (uint32_t)by_stride[1].size(), d_s2, stream);
        });
        prof.streaming = false;
        return rc;
    }
    int launch_resolve_stage() {
        bool any_list = false;  // (a pass with a confirm tier has no candidate bitmap to turn into a list: its flagged chunks are the work list)
        for (const DevGroup &d : e->groups) any_list = any_list || (d.filtered && !d.confirm);
        return timed("resolve+compact", 0xFCu, "resolve / compact kernel", [&] {
            const int he = launch_resolve(fall.data(), (uint32_t)fall.size(), d_all, stream);
            return !he && any_list ? launch_compact(fall.data(), (uint32_t)fall.size(), d_all, stream) : he;
        });
    }
    // ---- 2b. confirm tier ----
    int launch_confirm_stage() {
        if (call.empty()) return PWAF_OK;
        return timed("confirm", 0xF8u, "confirm kernel", [&] { return launch_confirm(call.data(), (uint32_t)call.size(), d_c, c_plan, e->n_cus, stream); });
    }
    // ---- 3. list-driven DFA passes: the launches plan_passes planned ----
    int launch_list_scans() {
        uint32_t *plan_at = l_plan;  // work-item prefix sums, one set per launch
        for (int phase = 0; phase < 2; phase++) {
            uint32_t first = 0;  // (a phase of more than 256 descriptors runs as several launches, one after the other on the stream)
            for (const uint32_t cnt : e->lscan_launches[phase]) {
                char nm[48];
                snprintf(nm, sizeof nm, "lscan_x%u", cnt);
                const int rc = timed(nm, 0xFDu, "gated scan kernel", [&] { return launch_scan_gated(la[phase].data() + first, cnt, d_la[phase] + first, plan_at, lshapes[phase], stream); });
                if (rc) return rc;
                plan_at += 2 * cnt + 1;  // (prefix sums, then the entries per work item of every pass)
                first += cnt;
            }
        }
        return PWAF_OK;
    }
    // field-against-field atoms: the last (pseudo) pass; its hit records are written for every request
    int launch_fcmp_stage() {
        if (P.fcmp.empty()) return PWAF_OK;
        FcmpArgs fa{};
        std::vector<uint32_t> slots;  // field ids in use, by slot
        for (size_t k = 0; k < P.fcmp.size(); k++) {
            uint32_t sl[2];
            const uint32_t fld[2] = {P.fcmp[k].a, P.fcmp[k].b};
            for (int q = 0; q < 2; q++) {
                size_t at = std::find(slots.begin(), slots.end(), fld[q]) - slots.begin();
                if (at == slots.size()) slots.push_back(fld[q]);
                sl[q] = (uint32_t)at;
            }
            fa.atoms[k] = P.fcmp[k].op | (sl[0] << 8) | (sl[1] << 16);
        }
        for (size_t q = 0; q < slots.size() && q < kMaxFcmpFields; q++) {
            fa.data[q] = cols[slots[q]].data;
            fa.off[q] = cols[slots[q]].offsets;
        }
        fa.n = n;
        fa.n_atoms = (uint32_t)P.fcmp.size();
        fa.rec = (uint32_t *)S.rec.p + e->groups.size() * (size_t)n;
        set_pool(fa);
        return timed("fcmp", 0xFBu, "field comparison kernel", [&] { return launch_fcmp(fa, stream); });
    }
    // rules the column compiler could not take: interpreted per request (residual.h), results = the hit records of the last pseudo pass
    template <class Args>
    int residual_inputs(Args &a) {  // what both forms of the residual kernel read
        a.data = (const uint8_t *const *)S.res_cols.p;
        a.off = (const uint32_t *const *)((const char *)S.res_cols.p + (size_t)e->n_fields * 8);
        a.blob = (const uint8_t *)e->residual_blob.p;
        a.n = n;
        a.n_rules = P.n_residual;
        a.ip = db.ip;
        a.ip_is_v6 = db.ip_is_v6;
        a.port = db.port;
        a.asn = db.asn;
        a.country = db.country;
        a.has_geo = (P.has_geo && P.residual_needs_geo) ? 1u : 0u;
        a.geo_root4 = (const uint32_t *)e->geo_rec_root4.p;
        a.geo_root6 = (const uint32_t *)e->geo_rec_root6.p;
        a.geo_nodes = (const uint32_t *)e->geo_rec_nodes.p;
        a.geo_recs = (const GeoRec *)e->geo_recs.p;
        a.rule_errors = (unsigned long long *)e->residual_errors.p;
        if (S.retry) {  // (pwaf_engine_rule_errors counts REQUESTS: a batch run again for a larger pool must not count its errors twice)
            const int rc = S.err_sink.reserve((size_t)P.n_residual * 8);
            if (rc) return rc;
            a.rule_errors = (unsigned long long *)S.err_sink.p;
        }
        return PWAF_OK;
    }
    int launch_residual_stage() {
        if (!P.n_residual) return PWAF_OK;
        int rc;
        if (e->residual_jit.function) {
            // the SPECIALIZED form: the same programs as straight-line device code (compiled at creation); the verdict kernel reads the result words
            ResidualJitArgs ja{};
            if ((rc = residual_inputs(ja))) return rc;
            ja.match_words = (uint32_t *)S.res_words.p;
            return timed("residual_jit", 0xF9u, "specialized residual kernel", [&] { return launch_residual_jit(e->residual_jit, ja, e->n_cus, stream); });
        }
        ResidualArgs ra{};
        if ((rc = residual_inputs(ra))) return rc;
        ra.rec = (uint32_t *)S.rec.p + (size_t)residual_pass * n;
        set_pool(ra);
        return timed("residual", 0xF9u, "residual kernel", [&] { return launch_residual(ra, stream); });
    }
    int launch_verdict_stage() { return timed("verdict", 0xFFu, "verdict kernel", [&] { return launch_verdict(v, stream); }); }
    // PWAF_DUMP_COUNTS, debugging aid: the device-side list lengths of this batch
    int dump_counts() {
        std::vector<uint32_t> cw(ctrl_words);
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpy(cw.data(), S.ctrl.p, 4 * ctrl_words, hipMemcpyDeviceToHost));
        fprintf(stderr, "[pwaf] n %u pool %u status %u |", n, cw[0], cw[1]);
        for (size_t k = 0; k < e->groups.size(); k++) {
            const DevGroup &d = e->groups[k];
            if (d.gate >= 0) fprintf(stderr, " pass %zu field %u %s list %u", k, d.field, d.filtered ? (d.confirm ? "confirm" : "filtered") : "gap", cw[2 + (size_t)d.gate]);
        }
        for (uint32_t k = 0; k < e->n_filtered; k++) fprintf(stderr, " pairs[%u] %u", k, cw[2 + n_slots + k]);
        fprintf(stderr, "\n");
        return PWAF_OK;
    }

    // ---- the descriptors: host arithmetic over DevGroup, the scratch pointers and the columns ----

    // where a kernel appends hit records that do not fit the pass's own: the overflow pool
    template <class Args>
    void set_pool(Args &a) const {
        a.pool = (PoolEntry *)S.pool.p;
        a.pool_count = (uint32_t *)S.ctrl.p;
        a.pool_cap = pool_cap;
        a.status = status_word;
    }
    // A pass that owns prefilter factors feeds the gated gap passes' request lists as its requests finish. (enq_bits: a gap pass's visited
    // bitmap, indexed by its list slot — set when the request is enqueued; scan_kernel's requests are enqueued once by construction.)
    bool feeds_gates(size_t gi) const { return e->n_gap && e->owns_factors[gi]; }
    template <class Args>
    void set_gate_feed(Args &a, const DevGroup &d) const {
        a.colmask_local = (const uint32_t *)e->colmask.p + d.atom_base;
        a.n_local = d.n_local;
        a.gate_lists = (uint32_t *)S.gate_lists.p;
        a.gate_count = (uint32_t *)S.ctrl.p + 2;
        if constexpr (!std::is_same<Args, ScanArgs>::value) {
            a.enq_bits = (uint32_t *)S.visit_bits.p;
            a.enq_words = bit_words;
        }
    }

    ScanArgs scan_args(size_t gi) const {
        const DevGroup &d = e->groups[gi];
        ScanArgs a{};
        if (feeds_gates(gi)) set_gate_feed(a, d);
        a.data = cols[d.field].data;
        a.off = cols[d.field].offsets;
        a.n = n;
        a.tab = (const uint16_t *)d.tab.p;
        a.classmap = (const uint8_t *)d.classmap.p;
        a.umap = d.scalar_mode ? (const uint8_t *)d.classmap.p + kUmapAt : nullptr;
        a.ill_class = d.ill_class;
        a.special = (const SpecialCell *)d.special.p;
        a.list_off = (const uint32_t *)d.list_off.p;
        a.list = (const uint16_t *)d.list.p;
        a.start_emit = d.start_emit;
        a.emit_base = d.emit_base;
        a.n_cus = e->n_cus;
        a.chunks = d.chunks;
        a.special_base = d.special_base;
        a.n_states = d.n_states;
        a.stride = d.stride;
        a.n_classes = d.n_classes;
        a.n_hot = d.n_hot;
        a.rec = (uint32_t *)S.rec.p + gi * (size_t)n;
        set_pool(a);
        return a;
    }

    // arena sizes: a host batch's offsets were read while staging; a device batch says so itself or is asked (one small copy)
    int learn_arena_sizes() {
        bool ask = false;
        for (const DevGroup &d : e->groups)
            if (d.filtered && !col_known[d.field]) {
                HIP_TRY(hipMemcpyAsync(&col_bytes[d.field], cols[d.field].offsets + n, 4, hipMemcpyDeviceToHost, stream));
                ask = true;
            }
        if (ask) HIP_TRY(hipStreamSynchronize(stream));
        return PWAF_OK;
    }

    uint32_t slab0_of(uint32_t field) const { return col_begin ? (*col_begin)[field] / kStreamSlab : 0u; }

    // FilterArgs of every filtered pass (fall, in pass order; by_stride: the same split for the fused launch), sized scratch included
    int build_filter_args() {
        int rc;
        filter_index.assign(e->groups.size(), 0);
        if (!e->n_filtered) return PWAF_OK;
        const uint32_t words = (n + 31) / 32, n_cblocks = (words + kCompactWords - 1) / kCompactWords;
        uint64_t sub_entries = 0, n_slabs_all = 0, pair_bytes = 0;
        for (const DevGroup &d : e->groups)
            if (d.filtered) {
                const uint64_t slabs = slab_count(col_bytes[d.field], slab0_of(d.field));
                n_slabs_all += slabs;
                sub_entries += slabs * (kStreamSlab / 512);  // chunk bitmap words
                if (d.confirm) pair_bytes += (uint64_t)pair_cap_of((uint32_t)slabs, n) * sizeof(uint2);
            }
        if ((rc = S.chunk_bits.reserve((size_t)sub_entries * 4))) return rc;
        if ((rc = S.cand_cnt.reserve((size_t)(2 * n_slabs_all + (uint64_t)e->n_filtered * n_cblocks) * 4))) return rc;  // per pass: flag counts per slab, pair-list starts per slab, candidates per compact workgroup
        if (pair_bytes && (rc = S.pairs.reserve((size_t)pair_bytes))) return rc;
        const bool dense_switch = !(P.flags & PWAF_OPT_NO_DENSE_SWITCH);
        uint32_t fi = 0;
        uint64_t sub_at = 0, cnt_at = 0, pair_at = 0;
        for (size_t gi = 0; gi < e->groups.size(); gi++) {
            const DevGroup &d = e->groups[gi];
            if (!d.filtered) continue;
            fall.emplace_back();
            FilterArgs &f = fall.back();
            f.data = cols[d.field].data;
            f.off = cols[d.field].offsets;
            f.n = n;
            f.total = col_bytes[d.field];
            f.init = d.filter.init;
            f.mul = d.filter.mul;
            f.stride = d.filter.stride;
            f.debug = sw.filter_debug_skip;
            f.table = (const uint32_t *)d.ftable.p;
            f.n_heads = (uint32_t)std::min<size_t>(2, d.filter.heads.size());
            for (uint32_t h = 0; h < f.n_heads; h++) {
                const FilterHead &fh = d.filter.heads[h];
                uint8_t lit[16] = {0}, msk[16] = {0};
                memcpy(lit, fh.bytes, fh.len);
                memset(msk, 0xFF, fh.len);
                memcpy(f.head_w[h], lit, 16);
                memcpy(f.head_m[h], msk, 16);
                f.head_len[h] = fh.len | ((uint32_t)fh.exact << 8);
                f.head_code[h] = h == 0 ? (uint32_t)fh.local + 1u : ((uint32_t)fh.local + 1u) << 15;
            }
            f.slab0 = slab0_of(d.field);
            const uint32_t slabs = slabs_of(f);
            f.rec = (uint32_t *)S.rec.p + gi * (size_t)n;
            f.chunk_bits = (uint32_t *)S.chunk_bits.p + sub_at;
            f.sub_count = (uint32_t *)S.cand_cnt.p + cnt_at;
            f.pair_base = f.sub_count + slabs;
            f.block_count = f.pair_base + slabs;
            f.bitmap = (uint32_t *)S.cand_bits.p + (size_t)fi * bit_words;
            filter_index[gi] = fi;
            f.list = (uint32_t *)S.gate_lists.p + (size_t)d.gate * n;
            f.list_count = (uint32_t *)S.ctrl.p + 2 + d.gate;
            if (d.confirm) {
                f.pair_cap = pair_cap_of(slabs, n);
                f.pairs = (uint2 *)((char *)S.pairs.p + pair_at);
                f.pair_count = (uint32_t *)S.ctrl.p + 2 + n_slots + fi;
                pair_at += (uint64_t)f.pair_cap * sizeof(uint2);
                if (dense_switch) {
                    // more than half of the arena's 16-byte chunks flagged: confirming them one by one costs more than walking every request
                    // (measured, round 5: the saturated stream took 22 ms in the confirm tier against 9 ms for the plain DFA over the same bytes;
                    // the hostile stream of the 1k-rule set flags a quarter of its chunks and stays on the confirm tier: 1.3 ms against 3.9)
                    f.dense_flag = f.pair_count;  // (the count filter_kernel leaves there, against dense_thresh)
                    f.dense_thresh = (uint32_t)std::min<uint64_t>(0xFFFFFFFEu, (uint64_t)slabs * (kStreamSlab / 16) / 2);
                }
            }
            f.first_block = 0;
            sub_at += (uint64_t)slabs * (kStreamSlab / 512);
            cnt_at += 2 * slabs + n_cblocks;
            alg_bytes[f.stride == 2 ? 2 : 1] += (uint64_t)f.total + 4ull * (n + 1);
            fi++;
        }
        // the fused filter launch takes the stride-1 passes and the stride-2 passes as two tables, first_block numbered within each
        for (const FilterArgs &f : fall) {
            std::vector<FilterArgs> &sub = by_stride[f.stride == 2 ? 1 : 0];
            const uint32_t block = sub.empty() ? 0u : sub.back().first_block + (slabs_of(sub.back()) + kFilterWaves - 1) / kFilterWaves;
            sub.push_back(f);
            sub.back().first_block = block;
        }
        return PWAF_OK;
    }

    // confirm tier: what the flagged chunks of every candidate really hold (literal atoms decided; walk flags). `wi`: the pass's walk bitmap
    ConfirmArgs confirm_args(const FilterArgs &f, const DevGroup &d, size_t gi, uint32_t wi) const {
        ConfirmArgs c{};
        c.data = f.data;
        c.off = f.off;
        c.n = n;
        c.total = f.total;
        c.pairs = f.pairs;
        c.pair_count = f.pair_count;
        c.pair_cap = f.pair_cap;
        c.mul = f.mul;
        c.stride = f.stride;
        c.init = f.init;
        c.ftable = f.table;
        c.c_head = (const uint32_t *)d.c_head.p;
        c.c_entries = (const ConfirmEntry *)d.c_entries.p;
        c.c_bytes = (const uint8_t *)d.c_bytes.p;
        c.c_classes = (const uint32_t *)d.c_classes.p;
        c.n_entries = (uint32_t)d.filter.confirm.entries.size();
        c.n_bytes = confirm_table_bytes(d.filter.confirm.bytes.size());
        c.n_class_words = (uint32_t)d.filter.confirm.classes.size();
        c.rec = f.rec;
        c.valid_bits = f.bitmap;
        c.dense_flag = f.dense_flag;
        c.dense_thresh = f.dense_thresh;
        c.walk_bits = (uint32_t *)S.walk_bits.p + (size_t)wi * bit_words;
        if (d.confirm_walk) {
            c.walk_list = f.list;
            c.walk_count = f.list_count;
        }
        set_pool(c);
        if (feeds_gates(gi)) {
            set_gate_feed(c, d);
            c.shared_bits = d.shared_bits;
        }
        return c;
    }
    void build_confirm_args() {
        for (size_t gi = 0; gi < e->groups.size(); gi++) {
            const DevGroup &d = e->groups[gi];
            if (d.filtered && d.confirm) call.push_back(confirm_args(fall[filter_index[gi]], d, gi, (uint32_t)call.size()));
        }
    }

    // One descriptor of the plan (scanplan.h: plan_list_scans decided what it walks and what it stages) with this batch's pointers
    ListScanArgs list_args(const ListDesc &pl) const {
        const size_t gi = pl.pass;
        const DevGroup &d = e->groups[gi];
        ListScanArgs a{};
        const DevGroup &src = d.share_owner >= 0 ? e->groups[(size_t)d.share_owner] : d;  // whose list this pass walks
        if (!d.identity) {
            a.req_list = (const uint32_t *)S.gate_lists.p + (size_t)src.gate * n;
            a.n_list = (const uint32_t *)S.ctrl.p + 2 + src.gate;
        }
        if (d.visit_slot >= 0) a.visited = (uint32_t *)S.visit_bits.p + (size_t)d.visit_slot * bit_words;
        if (pl.share_owner >= 0) {
            a.need_in = (const uint32_t *)S.need.p + (size_t)src.need_slot * n;
            a.need_bit = pl.need_bit;
        }
        if (feeds_gates(gi)) {
            set_gate_feed(a, d);
            if (d.need_slot >= 0) {
                a.need_out = (uint32_t *)S.need.p + (size_t)d.need_slot * n;
                a.shared_bits = d.shared_bits;
            }
        }
        a.merge_rec = pl.merge_rec ? 1u : 0u;
        a.behind_filter = pl.behind_filter ? 1u : 0u;
        a.data = cols[d.field].data;
        a.off = cols[d.field].offsets;
        a.n = n;
        const FlatDev &F = pl.rtier ? d.rt : d.fl;
        a.flat = (const uint16_t *)F.flat.p;
        a.classmap = (const uint8_t *)F.flat_classmap.p;
        a.umap = F.scalar_mode ? (const uint8_t *)F.flat_classmap.p + kUmapAt : nullptr;
        a.ill_class = F.ill_class;
        a.n_classes = F.n_classes;
        a.n_hot = pl.n_hot;
        a.n_delta = pl.n_delta;
        if (pl.n_delta) a.delta = (const uint64_t *)F.delta.p;
        a.emit_off = (const uint32_t *)F.emit_off.p;
        a.emit_list = (const uint16_t *)F.emit_list.p;
        a.end_off = (const uint32_t *)F.end_off.p;
        a.end_list = (const uint16_t *)F.end_list.p;
        a.rec = (uint32_t *)S.rec.p + gi * (size_t)n;
        set_pool(a);
        a.n_cus = e->n_cus;
        return a;
    }
    // The flag-density switch (kernels.h: ListScanArgs::dense_flag): the FilterArgs of a pass whose confirm tier has it — they name the
    // device word that says "walked whole this batch" and its threshold — else null.
    const FilterArgs *dense_of(size_t gi) const {
        const FilterArgs *f = e->groups[gi].filtered ? &fall[filter_index[gi]] : nullptr;
        return f && f->dense_flag ? f : nullptr;
    }
    static void set_dense(ListScanArgs &a, const FilterArgs &f, uint32_t mode) {
        a.dense_flag = f.dense_flag;
        a.dense_thresh = f.dense_thresh;
        a.dense_mode = mode;
    }
    // list-driven DFA passes, as planned when the passes got their roles (assign_lists): first those behind a prefilter (they may feed
    // the gap passes' lists), then the gap passes
    void build_list_args() {
        for (int phase = 0; phase < 2; phase++)
            for (const ListDesc &pl : e->list_plan.descs[phase]) {
                ListScanArgs a = list_args(pl);
                const size_t of = pl.dense_mode == 3 ? (size_t)pl.share_owner : (size_t)pl.pass;  // (3: a gap pass riding the owner's list through need masks)
                if (pl.dense_mode == 1) {
                    // the pass's dense alternative: EVERY request through the full table, records and valid bits written for all
                    a.req_list = nullptr;
                    a.n_list = nullptr;
                    a.visited = (uint32_t *)S.cand_bits.p + (size_t)filter_index[pl.pass] * bit_words;
                }
                if (pl.dense_mode) set_dense(a, *dense_of(of), pl.dense_mode);
                la[phase].push_back(a);
            }
    }
    int check_list_plan() const {  // (the launches plan_passes planned must take exactly these descriptors)
        for (int phase = 0; phase < 2; phase++) {
            size_t planned = 0;
            for (const uint32_t c : e->lscan_launches[phase]) planned += c;
            if (planned != la[phase].size()) return fail(PWAF_E_DEVICE, "list-scan launch plan does not match the batch's descriptors");
        }
        return PWAF_OK;
    }
    void build_column_pointers() {
        if (!P.n_residual) return;
        const size_t nc = e->n_fields;
        ptrs.count = (uint32_t)(2 * nc);
        for (size_t f = 0; f < nc; f++) { ptrs.p[f] = cols[f].data; ptrs.p[nc + f] = cols[f].offsets; }
    }

    // ---- placement and upload ----
    // Device layout of Scratch::args: [all filtered passes] [stride-1 passes] [stride-2 passes] [confirm passes] [list passes of phase 0] [of
    // phase 1] [column pointers] — the uploaded part — then the work-item plans the plan kernels write (confirm: count + 2 words; list
    // scans: per launch 2 * count + 1). The host writes the uploaded part into a page-locked slot; ONE copy launch moves it (and clears
    // the zeroed block, when that was deferred).
    int upload_descriptors() {
        int rc;
        struct Part { size_t at; const void *src; size_t bytes; };
        const size_t b_all = fall.size() * sizeof(FilterArgs), b_s1 = by_stride[0].size() * sizeof(FilterArgs), b_s2 = by_stride[1].size() * sizeof(FilterArgs),
                     b_c = call.size() * sizeof(ConfirmArgs), b_l0 = la[0].size() * sizeof(ListScanArgs), b_l1 = la[1].size() * sizeof(ListScanArgs),
                     b_ptrs = (size_t)ptrs.count * sizeof(void *);
        Layout L;  // (a list table keeps room for one descriptor more than it holds)
        const Part up[7] = {{L.take(b_all), fall.data(), b_all}, {L.take(b_s1), by_stride[0].data(), b_s1}, {L.take(b_s2), by_stride[1].data(), b_s2}, {L.take(b_c), call.data(), b_c},
                            {L.take(b_l0 + sizeof(ListScanArgs)), la[0].data(), b_l0}, {L.take(b_l1 + sizeof(ListScanArgs)), la[1].data(), b_l1}, {L.take(b_ptrs), ptrs.p, b_ptrs}};
        const size_t up_bytes = L.size();
        const size_t a_cplan = L.take((call.size() + 2) * 4), a_lplan = L.take((lsplit::plan_words(e->lscan_launches[0]) + lsplit::plan_words(e->lscan_launches[1])) * 4);
        if ((rc = S.args.reserve(L.size()))) return rc;
        char *const abase = (char *)S.args.p;
        d_all = (const FilterArgs *)(abase + up[0].at);
        d_s1 = (const FilterArgs *)(abase + up[1].at);
        d_s2 = (const FilterArgs *)(abase + up[2].at);
        d_c = (const ConfirmArgs *)(abase + up[3].at);
        d_la[0] = (const ListScanArgs *)(abase + up[4].at);
        d_la[1] = (const ListScanArgs *)(abase + up[5].at);
        S.res_cols.p = abase + up[6].at;
        c_plan = (uint32_t *)(abase + a_cplan);
        l_plan = (uint32_t *)(abase + a_lplan);
        if (up_bytes) {
            const uint32_t slot = S.arg_next++ % Scratch::kArgSlots;
            if (S.arg_pending[slot]) HIP_TRY(hipEventSynchronize(S.arg_ev[slot]));  // (the copy launch that read this slot last has run: returns at once unless the caller is kArgSlots batches ahead)
            if ((rc = S.arg_slot[slot].reserve(up_bytes))) return rc;
            char *const hb = (char *)S.arg_slot[slot].p;
            for (const Part &p : up)
                if (p.bytes) memcpy(hb + p.at, p.src, p.bytes);
            arg_slot.slot = (int)slot;  // (from here on every way out of the pipeline records the slot's event)
            const int he = upload_args_block(hb, S.args.p, up_bytes, zero_deferred ? S.zero_block.p : nullptr, zero_deferred ? zero_bytes : 0, stream);
            if (he) return fail(PWAF_E_DEVICE, std::string("descriptor upload failed: ") + hipGetErrorString((hipError_t)he));
        } else if (zero_deferred) {  // (nothing to upload: the block is cleared the old way)
            HIP_TRY(hipMemsetAsync(S.zero_block.p, 0, zero_bytes, stream));
        }
        zero_deferred = false;
        return PWAF_OK;
    }
};

// One batch of device columns through every launch. Nothing between upload_descriptors and the end returns past
// BatchRun's destructor: the descriptor slot's event is recorded whichever way the batch leaves (ArgSlotMark).
int run_pipeline(pwaf_engine *e, Scratch &S, const pwaf_batch &db /* device pointers */, pwaf_verdict *d_out, pwaf_counts *d_counts, uint32_t *d_match_idx,
                 uint32_t *d_n_matches, hipStream_t stream, bool totals_known = false, const std::vector<uint32_t> *col_begin = nullptr, bool sync_status = false,
                 pwaf_geo *d_geo = nullptr, const ReportOut *d_rep = nullptr) {
    if (db.n == 0) return PWAF_OK;
    BatchRun b(e, S, db, stream, col_begin);
    b.d_geo = d_geo;
    int rc;
    if ((rc = b.reserve_scratch(sync_status)) || (rc = b.resolve_columns(totals_known))) return rc;
    if ((rc = b.fill_verdict_args(d_out, d_counts, d_match_idx, d_n_matches))) return rc;
    if (d_rep && d_rep->any()) {  // (the verdict kernel's rule-hit variant, or its route variant: launch_verdict)
        b.v.hits = d_rep->hits;
        b.v.hits_cap = d_rep->cap;
        b.v.n_hits = d_rep->n_hits;
        b.v.rule_hits = (unsigned long long *)d_rep->rule_hits;
        b.v.route = d_rep->route;
        b.v.route_base = e->prog.p->route_base;
        if (d_rep->hit_any() && e->rules_unrouted.p) b.v.rules = (const DevRule *)e->rules_unrouted.p;
    }
    if ((rc = b.attr_at_start()) || (rc = b.launch_plain_scans())) return rc;
    // every descriptor of the batch: built, checked against the launch plan, uploaded once
    if ((rc = b.learn_arena_sizes()) || (rc = b.zero_head_records()) || (rc = b.build_filter_args())) return rc;
    b.build_confirm_args();
    b.build_list_args();
    b.build_column_pointers();
    if ((rc = b.check_list_plan()) || (rc = b.upload_descriptors())) return rc;
    if (e->n_filtered) {
        if ((rc = b.launch_filter_stage())) return rc;
        if (!b.sw.attr_after_compact && (rc = b.attr_after_filter())) return rc;  // (PWAF_ATTR_AFTER_COMPACT: timing experiment)
        if ((rc = b.launch_resolve_stage()) || (rc = b.launch_confirm_stage())) return rc;
    }
    if ((rc = b.attr_after_filter())) return rc;  // (no filtered pass: beside the list scans / the verdict kernel's predecessors)
    if ((rc = b.launch_list_scans()) || (rc = b.launch_fcmp_stage()) || (rc = b.launch_residual_stage())) return rc;
    if ((rc = b.join_side()) || (rc = b.launch_verdict_stage())) return rc;
    if (b.sw.dump_counts && (rc = b.dump_counts())) return rc;
    if ((rc = b.arg_slot.record())) return rc;
    b.prof.commit();
    return PWAF_OK;
}

// What a context remembers of its latest batch (acquire_context), and the event its next user waits for.
hipError_t mark_context_used(Scratch &S, hipStream_t s, bool own) {
    S.used = true;
    S.last = s;
    S.last_own = own;
    return hipEventRecord(S.done, s);
}

int device_error(const char *call, hipError_t he) { return fail(PWAF_E_DEVICE, std::string(call) + ": " + hipGetErrorString(he)); }

// The synchronous entry points' batch on the context's own stream: runs the pipeline and waits ONCE — the status words travel back
// (into page-locked memory) behind the batch, together with whatever `after` enqueues (the verdicts on their way to the host). A batch
// that exhausted the overflow pool is run again, at most twice, with a pool of the size it asked for (the staged columns stay where
// they are). `counts_zero`: the first attempt's counters arrive zeroed (they are part of a staged block). Whatever fails, the stream is
// drained before the call returns: what was enqueued may still read the caller's buffers.
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

}  // namespace

extern "C" {

uint32_t pwaf_abi_version(void) { return PWAF_ABI_VERSION; }
const char *pwaf_last_error(void) { return g_last_error.c_str(); }

int pwaf_compile_expression(const char *expression, char *errbuf, size_t errbuf_len) {
    Syntax syn;
    std::string err;
    bool ok = expression && parse_expression(expression, syn, err);
    if (!ok) {
        std::string m = "Expression is not valid: " + (expression ? err : std::string("null expression"));
        if (errbuf && errbuf_len) snprintf(errbuf, errbuf_len, "%s", m.c_str());
        return fail(PWAF_E_SYNTAX, m);
    }
    return PWAF_OK;
}

int pwaf_validate_expression(const char *expression, char *errbuf, size_t errbuf_len) {
    auto bad = [&](const std::string &why) {
        std::string m = "Expression is not valid: " + why;
        if (errbuf && errbuf_len) snprintf(errbuf, errbuf_len, "%s", m.c_str());
        return fail(PWAF_E_SYNTAX, m);
    };
    if (!expression || !*expression) return bad("expression is empty");  // rules/rules.rs:56-58
    Syntax syn;
    std::string err;
    if (!parse_expression(expression, syn, err)) return bad(err);
    if (syn.uses_in) return bad("unknown operator: in");  // rules/rules.rs:69-71
    return PWAF_OK;
}

int pwaf_program_compile(const pwaf_rule_desc *rules, size_t n_rules, const pwaf_list_desc *lists, size_t n_lists, const pwaf_geoip_table *geoip,
                         const pwaf_options *opts, pwaf_program **out, pwaf_compile_error *err) {
    return pwaf_program_compile_routed(rules, n_rules, nullptr, 0, lists, n_lists, geoip, opts, out, err);
}
// With an ordered list of routes beside the rules (include/pwaf.h: routes). n_routes == 0: nothing differs.
int pwaf_program_compile_routed(const pwaf_rule_desc *rules, size_t n_rules, const pwaf_route_desc *routes, size_t n_routes, const pwaf_list_desc *lists, size_t n_lists,
                                const pwaf_geoip_table *geoip, const pwaf_options *opts, pwaf_program **out, pwaf_compile_error *err) {
    if (!out || (n_rules && !rules) || (n_routes && !routes) || (n_lists && !lists)) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    pwaf_options o;
    int rc = check_opts(opts, o);
    if (rc) return rc;
    CompileInput in{rules, n_rules, routes, n_routes, lists, n_lists, geoip, o};
    pwaf_compile_error ce{};
    ce.rule_index = 0xFFFFFFFFu;
    std::unique_ptr<Program> p;
    try {
        rc = compile_program(in, p, ce);
    } catch (const std::bad_alloc &) {
        ce.code = rc = PWAF_E_NOMEM;
        snprintf(ce.message, sizeof ce.message, "out of memory while compiling the rule set");
    } catch (const std::exception &ex) {
        ce.code = rc = PWAF_E_UNSUPPORTED;
        snprintf(ce.message, sizeof ce.message, "internal compiler error: %s", ex.what());
    }
    if (rc) {
        put_err(err, ce);
        return rc;
    }
    auto *pp = new pwaf_program();
    pp->p = std::move(p);
    *out = pp;
    for (auto &st : pp->p->rule_status)
        if (st.first != PWAF_OK) return PWAF_W_PARTIAL;  // (PWAF_OPT_LENIENT: created, but some rule is not evaluated)
    return PWAF_OK;
}

void pwaf_program_destroy(pwaf_program *p) { delete p; }

size_t pwaf_program_dump(const pwaf_program *p, uint8_t *buf, size_t cap) {
    if (!p) return 0;
    auto *mp = const_cast<pwaf_program *>(p);
    if (mp->dump.empty()) mp->dump = dump_program(*p->p);
    if (buf && cap) memcpy(buf, mp->dump.data(), std::min(cap, mp->dump.size()));
    return mp->dump.size();
}
int pwaf_program_rule_status(const pwaf_program *p, uint32_t i, char *msg, size_t msg_len) {
    if (msg && msg_len) msg[0] = 0;
    if (!p || i >= p->p->rule_status.size()) return PWAF_E_INVALID_ARG;
    if (msg && msg_len) snprintf(msg, msg_len, "%s", p->p->rule_status[i].second.c_str());
    return p->p->rule_status[i].first;
}
size_t pwaf_program_warning_count(const pwaf_program *p) { return p ? p->p->warnings.size() : 0; }
const char *pwaf_program_warning(const pwaf_program *p, size_t i) { return (p && i < p->p->warnings.size()) ? p->p->warnings[i].c_str() : ""; }
int pwaf_program_stats(const pwaf_program *p, pwaf_stats *out) {
    if (!p || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    *out = p->p->stats;
    return PWAF_OK;
}

uint32_t pwaf_program_route_count(const pwaf_program *p) { return p && p->p ? p->p->n_routes : 0u; }
uint32_t pwaf_engine_route_count(const pwaf_engine *e) { return e && e->prog.p ? e->prog.p->n_routes : 0u; }

namespace {

// The tables of a plan (tableplan.h) and of the program itself on their way to the device; the engine keeps the plan's shape.
int upload_tables(pwaf_engine *e, const TablePlan &t) {
    const Program &P = *e->prog.p;
    int rc = PWAF_OK;
    const auto up = [&](DevBuf &buf, const auto &vec) { if (!rc) rc = upload(buf, vec); };
    static_cast<PlanShape &>(*e) = t;
    for (int var = 0; var < 2; var++) {
        up(e->iu_vals[var], t.iu_vals[var]);
        up(e->iu_masks[var], t.iu_masks[var]);
    }
    up(e->bit_atoms, t.bit_col);
    up(e->num_atoms, t.cmp_atoms);
    up(e->lazy_atoms, t.lazy_atoms);
    up(e->lits, t.lits);
    up(e->trig_off, t.trig_off);
    up(e->trig_rules, t.trig_rules);
    up(e->always_rules, t.always);
    up(e->country_luts, t.cc_masks);
    up(e->rules, P.rules);
    if (!t.rules_unrouted.empty()) up(e->rules_unrouted, t.rules_unrouted);
    up(e->set_masks, P.set_masks);
    up(e->ip_root4, P.ipset_trie.root4);
    up(e->ip_root6, P.ipset_trie.root6);
    up(e->ip_nodes, P.ipset_trie.nodes);
    up(e->class_rows, t.class_rows);
    up(e->geo_root4, t.geo_root4);
    up(e->geo_root6, t.geo_root6);
    up(e->geo_nodes, t.geo_nodes);
    // the root of a family without prefixes: every address reads class 0 (ip lists) / the default record's class (GeoIP: tableplan.cpp)
    up(e->leaf_root, std::vector<uint32_t>(65536, TRIE_LEAF));
    up(e->geo_leaf_root, std::vector<uint32_t>(65536, TRIE_LEAF | t.geo_default));
    if (P.n_residual) {
        up(e->residual_blob, P.residual_blob);
        up(e->residual_errors, std::vector<unsigned long long>(P.n_residual, 0ull));
        if (P.has_geo && P.residual_needs_geo) {
            // client.asn / client.country VALUES (the class trie above only keeps which predicates hold): the trie with record leaves
            const std::vector<uint32_t> leaf0(65536, TRIE_LEAF);  // record 0 = the default {0, "XX"}
            up(e->geo_rec_root4, P.geo_trie.root4.empty() ? leaf0 : P.geo_trie.root4);
            up(e->geo_rec_root6, P.geo_trie.root6.empty() ? leaf0 : P.geo_trie.root6);
            up(e->geo_rec_nodes, P.geo_trie.nodes);
            up(e->geo_recs, P.geo_recs);
        }
    }
    return rc;
}

// The scan tables of pass k (scanplan.h) on their way to the device: the streaming table, the flat table of the list scans and — a pass
// with an R tier — the flat table of its non-literal atoms. T: the profile of a tuning sample (null at creation).
int upload_flat(FlatDev &d, const FlatImage &m) {
    int rc = PWAF_OK;
    const auto up = [&](DevBuf &buf, const auto &vec, size_t pad = 0) { if (!rc) rc = upload(buf, vec, pad); };
    static_cast<FlatShape &>(d) = m;
    up(d.flat, m.flat, 16);  // (the LDS staging copies whole 16-byte units)
    up(d.delta, m.delta, 16);
    up(d.flat_classmap, m.classmap);
    up(d.emit_off, m.emit_off);
    up(d.emit_list, m.emit_list);
    up(d.end_off, m.end_off);
    up(d.end_list, m.end_list);
    return rc;
}
int upload_group(pwaf_engine *e, size_t k, const TuneOut *T) {
    const Program &P = *e->prog.p;
    const DfaGroup &g = P.groups[k];
    DevGroup &d = e->groups[k];
    int rc;
    ScanImage m;
    if ((rc = build_device_group(g, P.lds_hot_budget, m, T ? &T->visits[k] : nullptr, T ? &T->class_freq[k] : nullptr))) return rc;
    static_cast<ScanShape &>(d) = m;
    if ((rc = upload(d.tab, m.tab, 16)) || (rc = upload(d.classmap, m.classmap)) || (rc = upload(d.special, m.special)) || (rc = upload(d.list_off, m.list_off)) ||
        (rc = upload(d.list, m.list)))
        return rc;
    FlatImage fm, rm;
    const uint32_t lds[2] = {flat_lds_bytes(false), flat_lds_bytes(true)};
    build_flat_images(g, d.filter, lds, T, k, fm, rm);
    if ((rc = upload_flat(d.fl, fm)) || !g.rtier) return rc;
    return upload_flat(d.rt, rm);
}

// Gives every pass its role (scanplan.h: plan_passes) and uploads what the roles need. Called at creation and again when
// pwaf_engine_tune has rebuilt the filters from a traffic sample.
int assign_lists(pwaf_engine *e) {
    const Program &P = *e->prog.p;
    std::vector<GroupFilter> filters;
    for (const DevGroup &d : e->groups) filters.push_back(d.filter);
    PassPlan plan;
    plan_passes(P, filters, e->mean_len, e->residual_jit.function != nullptr, switches().skip_identity, plan);
    static_cast<PassShape &>(*e) = plan;
    std::vector<FlatShape> full, rtier;
    for (const DevGroup &d : e->groups) {
        full.push_back(d.fl);
        rtier.push_back(d.rt);
    }
    plan_list_scans(plan.roles, full, rtier, !(P.flags & PWAF_OPT_NO_DENSE_SWITCH), switches().skip_identity, switches().list_shape, e->list_plan);
    int rc = PWAF_OK;
    const auto up = [&](DevBuf &buf, const auto &vec) { if (!rc) rc = upload(buf, vec); };
    for (size_t k = 0; k < e->groups.size(); k++) {
        DevGroup &d = e->groups[k];
        static_cast<PassRole &>(d) = plan.roles[k];
        if (!d.filtered) continue;
        up(d.ftable, d.filter.table);
        if (!d.confirm) continue;
        const ConfirmTable &ct = d.filter.confirm;
        up(d.c_head, ct.head);
        up(d.c_entries, ct.entries);
        up(d.c_bytes, ct.bytes);
        up(d.c_classes, ct.classes);
    }
    if (!plan.short_atoms.empty()) up(e->short_atoms, plan.short_atoms);
    up(e->pass_table, plan.pass_table);
    up(e->colmask, plan.colmask);
    return rc;
}

}  // namespace

int pwaf_engine_create(const pwaf_rule_desc *rules, size_t n_rules, const pwaf_list_desc *lists, size_t n_lists, const pwaf_geoip_table *geoip,
                       const pwaf_options *opts, pwaf_engine **out, pwaf_compile_error *err) {
    return pwaf_engine_create_routed(rules, n_rules, nullptr, 0, lists, n_lists, geoip, opts, out, err);
}
int pwaf_engine_create_routed(const pwaf_rule_desc *rules, size_t n_rules, const pwaf_route_desc *routes, size_t n_routes, const pwaf_list_desc *lists, size_t n_lists,
                              const pwaf_geoip_table *geoip, const pwaf_options *opts, pwaf_engine **out, pwaf_compile_error *err) {
    if (!out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    pwaf_program *pp = nullptr;
    int rc = pwaf_program_compile_routed(rules, n_rules, routes, n_routes, lists, n_lists, geoip, opts, &pp, err);
    if (rc < 0) return rc;
    const int partial = rc;  // PWAF_W_PARTIAL or PWAF_OK
    std::unique_ptr<pwaf_engine> e(new pwaf_engine());
    e->prog.p = std::move(pp->p);
    delete pp;
    const Program &P = *e->prog.p;
    auto dev_fail = [&](int code) {
        if (err) {
            err->code = code;
            err->rule_index = 0xFFFFFFFFu;
            snprintf(err->message, sizeof err->message, "%s", g_last_error.c_str());
        }
        pwaf_engine_destroy(e.release());
        return code;
    };
    int ndev = 0;
    hipError_t he = hipGetDeviceCount(&ndev);
    if (he != hipSuccess || ndev == 0) {
        fail(PWAF_E_DEVICE, std::string("no HIP device available: ") + (he != hipSuccess ? hipGetErrorString(he) : "device count is 0"));
        return dev_fail(PWAF_E_DEVICE);
    }
    int dev = opts && opts->device >= 0 ? opts->device : -1;
    if (dev >= 0) {
        if (hipSetDevice(dev) != hipSuccess) { fail(PWAF_E_DEVICE, "hipSetDevice failed"); return dev_fail(PWAF_E_DEVICE); }
    } else if (hipGetDevice(&dev) != hipSuccess) {
        fail(PWAF_E_DEVICE, "hipGetDevice failed");
        return dev_fail(PWAF_E_DEVICE);
    }
    e->device = dev;
    if (hipSetDevice(dev) != hipSuccess) { fail(PWAF_E_DEVICE, "hipSetDevice failed"); return dev_fail(PWAF_E_DEVICE); }
    if (int ke = configure_kernels(dev)) {
        fail(PWAF_E_DEVICE, std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed: ") + hipGetErrorString((hipError_t)ke));
        return dev_fail(PWAF_E_DEVICE);
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) e->n_cus = (uint32_t)cus;
    }
    for (size_t k = 0; k < kContexts; k++) e->ctx.emplace_back(new Scratch());
    e->n_fields = PWAF_N_FIELDS + (uint32_t)P.header_names.size();
    e->mean_len.assign(e->n_fields, 0.0);
    e->groups.resize(P.groups.size());
    std::vector<uint32_t> pass_base;
    for (size_t k = 0; k < P.groups.size(); k++) {
        e->groups[k].filter = P.groups[k].filter;
        if ((rc = upload_group(e.get(), k, nullptr))) return dev_fail(rc);
        pass_base.push_back(P.groups[k].atom_base);
    }
    if ((rc = upload(e->pass_base, pass_base))) return dev_fail(rc);
    if (P.n_residual && !(opts && (opts->flags & PWAF_OPT_NO_RESIDUAL_JIT))) {
        // The SPECIALIZED form of the residual rules (before the pass table is built: their pseudo pass then has no records): translate,
        // compile for this device, load. Any failure leaves the interpreter in charge (same verdicts) and says so: pwaf_engine_residual_fallback.
        std::string text, why;
        std::vector<char> code;
        hipDeviceProp_t prop;
        bool ok = P.n_residual <= kMaxJitRules;
        if (!ok) why = "more than " + std::to_string(kMaxJitRules) + " residual rules";
        ok = ok && rvm_jit_program(P.residual_blob.data(), P.residual_blob.size(), text, why);
        if (ok && hipGetDeviceProperties(&prop, e->device) != hipSuccess) { ok = false; why = "hipGetDeviceProperties failed"; }
        ok = ok && rtc_compile(text, prop.gcnArchName, code, why) && jit_load(code, e->residual_jit, why);
        if (!ok) e->residual_note = "residual rules are interpreted per request, not specialized: " + why;  // (the ENGINE's: this device, this hiprtc — not the program's)
    }
    if ((rc = assign_lists(e.get()))) return dev_fail(rc);
    TablePlan plan;
    if ((rc = plan_tables(P, n_rules, n_routes, plan))) return dev_fail(rc);
    if (verdict_shape(P.n_cols, (uint32_t)P.rules.size(), plan.n_trig, (uint32_t)P.lits.size(), (P.flags & PWAF_OPT_GLOBAL_VERDICT_TABLES) != 0,
                      (int)verdict_mode(P.flags), (uint32_t)P.groups.size() + 2u).waves == 0 || P.n_cols >= 65536u) {
        fail(PWAF_E_UNSUPPORTED, "too many distinct predicates for one LDS column file (160 KiB)");
        return dev_fail(PWAF_E_UNSUPPORTED);
    }
    if ((rc = upload_tables(e.get(), plan))) return dev_fail(rc);
    if (P.flags & PWAF_OPT_GEO_ANSWERS) {
        // GeoIP answers: the trie with RECORD leaves and the records (shared with the residual rules: uploaded once), and for IPv4 a table
        // of record ids over the trie's first 24 bits, compressed like the class table (csrc/georec.h, csrc/dirtable.h)
        e->geo_answers = true;
        const std::vector<uint32_t> leaf0(65536, TRIE_LEAF);  // record 0 = the default {0, "XX"}
        if (!e->geo_rec_root4.p) {
            if ((rc = upload(e->geo_rec_root4, P.geo_trie.root4.empty() ? leaf0 : P.geo_trie.root4)) || (rc = upload(e->geo_rec_root6, P.geo_trie.root6.empty() ? leaf0 : P.geo_trie.root6)) ||
                (rc = upload(e->geo_rec_nodes, P.geo_trie.nodes)))
                return dev_fail(rc);
            const std::vector<GeoRec> def{GeoRec{0u, (uint16_t)('X' | ('X' << 8)), 0u}};
            if ((rc = upload(e->geo_recs, P.geo_recs.empty() ? def : P.geo_recs))) return dev_fail(rc);
        }
        if (P.has_geo && !P.geo_trie.root4.empty()) {
            std::vector<uint32_t> d24;
            e->georec_n_esc = georec::flatten(P.geo_trie.root4.data(), P.geo_trie.nodes.data(), d24);
            dirtable::Compressed ct;
            dirtable::compress(d24.data(), (P.flags & PWAF_OPT_NO_DIR_SUMMARY) != 0, ct, 0);  // (georec_kernel has no coarse level)
            if ((rc = upload(e->georec_chunks, ct.chunks)) || (rc = upload(e->georec_vals, ct.vals))) return dev_fail(rc);
            if (!ct.summary.empty()) {
                if ((rc = upload(e->georec_summary, ct.summary))) return dev_fail(rc);
                e->georec_shift = ct.shift;
                e->georec_common = ct.common;
            }
            e->georec_n_vals = (uint32_t)ct.vals.size();
        }
    }
    if ((P.has_geo && !P.geo_trie.root4.empty()) || (P.n_ip_lists && !P.ipset_trie.root4.empty())) {
        // DIR-24-8: one 64 MiB table (2^24 x 4 B) so that an IPv4 address resolves its GeoIP class AND its ip-list membership set with
        // a single gather; built on the device from the two tries that were just uploaded (first launch counts the escapes)
        VerdictArgs tv{};
        set_trie_args(e.get(), tv);
        DevBuf cnt;
        if ((rc = cnt.reserve(4))) return dev_fail(rc);
        uint32_t n_esc = 0;
        bool ok = hipMemset(cnt.p, 0, 4) == hipSuccess && launch_dir24(tv, nullptr, nullptr, cnt.p, nullptr) == 0 &&
                  hipMemcpy(&n_esc, cnt.p, 4, hipMemcpyDeviceToHost) == hipSuccess;
        if (ok) ok = e->dir24.reserve((size_t)4 << 24) == PWAF_OK && e->dir_esc.reserve((size_t)std::max(1u, n_esc) * 8) == PWAF_OK;
        if (ok) ok = hipMemset(cnt.p, 0, 4) == hipSuccess && launch_dir24(tv, e->dir24.p, e->dir_esc.p, cnt.p, nullptr) == 0 && hipDeviceSynchronize() == hipSuccess;
        if (!ok) { fail(PWAF_E_DEVICE, "DIR-24 table build failed"); return dev_fail(PWAF_E_DEVICE); }
        // Compressed for the lookups: runs of equal entries, 32 /24s per 16-byte record, and a summary bitmap in front of them
        // (csrc/dirtable.h: the layouts, the reasons and the code, shared with the CPU suite)
        {
            std::vector<uint32_t> d24((size_t)1 << 24);
            if (hipMemcpy(d24.data(), e->dir24.p, d24.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { fail(PWAF_E_DEVICE, "DIR-24 download failed"); return dev_fail(PWAF_E_DEVICE); }
            static_assert(dirtable::kChunkWords == kDirChunkWords, "dirtable.h and kernels.h disagree on the record layout");
            dirtable::Compressed ct;
            dirtable::compress(d24.data(), (P.flags & PWAF_OPT_NO_DIR_SUMMARY) != 0, ct, ipres_shape().coarse_bytes);
            if ((rc = upload(e->dir_chunks, ct.chunks)) || (rc = upload(e->dir_vals, ct.vals))) return dev_fail(rc);
            if (!ct.summary.empty()) {
                if ((rc = upload(e->dir_summary, ct.summary))) return dev_fail(rc);
                e->dir_sum_shift = ct.shift;
                e->dir_common = ct.common;
                e->dir_summary_set = (uint32_t)dirtable::popcount_words(ct.summary);
            }
            if (!ct.coarse.empty()) {  // (only in front of a summary)
                if ((rc = upload(e->dir_coarse, ct.coarse))) return dev_fail(rc);
                e->dir_coarse_shift = ct.coarse_shift;
                e->dir_coarse_bytes = (uint32_t)(ct.coarse.size() * 4);
                e->dir_coarse_set = (uint32_t)dirtable::popcount_words(ct.coarse);
            }
            e->dir_n_esc = n_esc;
            e->dir_n_vals = (uint32_t)ct.vals.size();
            e->dir24.release();
        }
    }
    if (hipDeviceSynchronize() != hipSuccess) { fail(PWAF_E_DEVICE, "device synchronize failed after table upload"); return dev_fail(PWAF_E_DEVICE); }
    *out = e.release();
    return partial;
}

void pwaf_engine_destroy(pwaf_engine *e) {
    if (!e) return;
    if (e->residual_jit.module) {  // (a module belongs to the device it was loaded on)
        int cur = -1;
        const bool have = hipGetDevice(&cur) == hipSuccess;
        (void)hipSetDevice(e->device);
        jit_release(e->residual_jit);
        if (have) (void)hipSetDevice(cur);
    }
    for (auto ev : e->ev) (void)hipEventDestroy(ev);
    delete e;  // (device and pinned memory, streams and events: their owners')
}

int pwaf_engine_residual_mode(const pwaf_engine *e) {
    if (!e || e->prog.p->n_residual == 0) return 0;
    return e->residual_jit.function ? 2 : 1;
}
const char *pwaf_engine_residual_fallback(const pwaf_engine *e) { return e ? e->residual_note.c_str() : ""; }
int pwaf_engine_address_tables(const pwaf_engine *e, uint32_t out[8]) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "pwaf_engine_address_tables: NULL argument");
    const Program &P = *e->prog.p;
    VerdictArgs v{};
    set_trie_args(e, v);
    out[0] = e->dir_n_esc;
    out[1] = e->dir_chunks.p ? e->dir_n_vals : 0u;
    out[2] = e->dir_summary.p ? 1u : 0u;
    out[3] = e->dir_sum_shift;
    out[4] = e->dir_common;
    out[5] = v.ipres_packed;
    out[6] = e->n_classes;
    out[7] = P.set_words ? (uint32_t)(P.set_masks.size() / P.set_words) : 1u;
    return PWAF_OK;
}
int pwaf_engine_coarse_tables(const pwaf_engine *e, uint32_t out[16]) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "pwaf_engine_coarse_tables: NULL argument");
    const IpresShape sh = ipres_shape();
    for (int i = 0; i < 16; i++) out[i] = 0;
    out[0] = e->dir_coarse.p ? 1u : 0u;
    out[1] = e->dir_coarse_shift;
    out[2] = e->dir_coarse_bytes;
    out[3] = e->dir_coarse_set;
    out[4] = e->dir_summary_set;
    out[5] = e->dir_coarse.p ? sh.threads : 256u;
    out[6] = e->dir_coarse.p ? sh.wg_per_cu : 8u;
    // out[8..11]: the record table (georec_kernel) has no coarse level
    return PWAF_OK;
}
int pwaf_engine_geo_answer_tables(const pwaf_engine *e, uint32_t out[8]) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "pwaf_engine_geo_answer_tables: NULL argument");
    if (int rc = need_geo_answers(e, "pwaf_engine_geo_answer_tables")) return rc;
    out[0] = e->georec_chunks.p ? 1u : 0u;
    out[1] = e->georec_n_esc;
    out[2] = e->georec_chunks.p ? e->georec_n_vals : 0u;
    out[3] = e->georec_summary.p ? 1u : 0u;
    out[4] = e->georec_shift;
    out[5] = e->georec_common;
    out[6] = (uint32_t)std::max<size_t>(1, e->prog.p->geo_recs.size());
    out[7] = 0;
    return PWAF_OK;
}
size_t pwaf_program_residual_source(const pwaf_program *p, int kind, char *buf, size_t cap) {
    if (!p || p->p->n_residual == 0) return 0;
    std::string text, why;
    const std::vector<uint8_t> &blob = p->p->residual_blob;
    if (!(kind == 0 ? rvm_specialize(blob.data(), blob.size(), text, why) : rvm_jit_program(blob.data(), blob.size(), text, why))) {
        (void)fail(PWAF_E_UNSUPPORTED, why);
        return 0;
    }
    if (buf && cap) {
        const size_t k = std::min(cap - 1, text.size());
        memcpy(buf, text.data(), k);
        buf[k] = '\0';
    }
    return text.size();
}
long pwaf_program_residual_compile(const pwaf_program *p, const char *arch, char *err, size_t err_len) {
    if (err && err_len) err[0] = '\0';
    if (!p || !arch) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    if (p->p->n_residual == 0) return 0;
    std::string text, why;
    std::vector<char> code;
    const std::vector<uint8_t> &blob = p->p->residual_blob;
    if (!rvm_jit_program(blob.data(), blob.size(), text, why) || !rtc_compile(text, arch, code, why)) {
        if (err && err_len) snprintf(err, err_len, "%s", why.c_str());
        return fail(PWAF_E_UNSUPPORTED, why);
    }
    return (long)code.size();
}

const pwaf_program *pwaf_engine_program(const pwaf_engine *e) { return e ? &e->prog : nullptr; }
uint32_t pwaf_program_header_count(const pwaf_program *p) { return p ? (uint32_t)p->p->header_names.size() : 0u; }
const char *pwaf_program_header_name(const pwaf_program *p, uint32_t i) { return (p && i < p->p->header_names.size()) ? p->p->header_names[i].c_str() : ""; }
uint32_t pwaf_engine_header_count(const pwaf_engine *e) { return e ? pwaf_program_header_count(&e->prog) : 0u; }
const char *pwaf_engine_header_name(const pwaf_engine *e, uint32_t i) { return e ? pwaf_program_header_name(&e->prog, i) : ""; }
void *pwaf_engine_stream(const pwaf_engine *e) {
    if (!e || e->ctx.empty() || hipSetDevice(e->device) != hipSuccess) return nullptr;
    Scratch &S = *e->ctx[0];
    std::lock_guard<std::mutex> lock(S.mu);
    return S.ensure(true) == PWAF_OK ? (void *)S.stream : nullptr;
}

int pwaf_engine_stats(const pwaf_engine *e, pwaf_stats *out) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    *out = e->prog.p->stats;
    // (the prefilters in use are the engine's: pwaf_engine_tune rebuilds them from traffic)
    out->n_filtered_groups = out->n_confirm_literals = 0;
    for (size_t k = 0; k < e->groups.size(); k++) {
        if (e->groups[k].filtered) out->n_filtered_groups++;
        if (e->groups[k].confirm) out->n_confirm_literals += e->prog.p->groups[k].n_confirm_literals;
    }
    return PWAF_OK;
}

int pwaf_engine_rule_errors(pwaf_engine *e, uint64_t *counts, size_t n_rules) {
    if (!e || (!counts && n_rules)) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    const Program &P = *e->prog.p;
    for (size_t k = 0; k < n_rules; k++) counts[k] = 0;
    if (P.n_residual == 0) return PWAF_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());  // (the counters of every batch enqueued so far)
    std::vector<unsigned long long> dev(P.n_residual);
    HIP_TRY(hipMemcpy(dev.data(), e->residual_errors.p, dev.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < dev.size() && k < P.residual_rule.size(); k++)
        if (P.residual_rule[k] < n_rules) counts[P.residual_rule[k]] += dev[k];
    return PWAF_OK;
}

int pwaf_program_confirm_field(const pwaf_program *p, uint32_t group, const uint8_t *bytes, size_t len, uint32_t arena_offset, uint16_t *atoms, size_t cap, size_t *n_atoms,
                               int *flagged, int *walk) {
    if (!p || !p->p || group >= p->p->groups.size() || (!bytes && len) || !n_atoms || !flagged || !walk) return fail(PWAF_E_INVALID_ARG, "bad argument");
    const GroupFilter &f = p->p->groups[group].filter;
    if (!f.enabled) return fail(PWAF_E_INVALID_ARG, "the pass has no prefilter");
    if (len > 0x7FFFFFF0u - arena_offset) return fail(PWAF_E_INVALID_ARG, "field too long");
    std::vector<uint8_t> arena((size_t)arena_offset + len + 2 * PWAF_ARENA_PAD, (uint8_t)'~');  // (what lies around the field must not matter)
    if (len) memcpy(arena.data() + arena_offset, bytes, len);
    std::vector<uint16_t> lits;
    bool fl = false;
    const bool wk = confirm_field_host(f, arena.data(), arena_offset, arena_offset + (uint32_t)len, lits, &fl);
    *n_atoms = std::min(cap, lits.size());
    for (size_t k = 0; k < *n_atoms; k++) atoms[k] = lits[k];
    *flagged = fl ? 1 : 0;
    *walk = wk ? 1 : 0;
    return PWAF_OK;
}

int pwaf_program_confirm_shape(const pwaf_program *p, uint32_t group, uint32_t out[8]) {
    if (!p || !p->p || group >= p->p->groups.size() || !out) return fail(PWAF_E_INVALID_ARG, "pwaf_program_confirm_shape: bad argument");
    const GroupFilter &f = p->p->groups[group].filter;
    if (!f.enabled || !f.confirm.enabled) return fail(PWAF_E_INVALID_ARG, "the pass has no confirm tier");
    const ConfirmTable &t = f.confirm;
    // the sizes as the engine hands them to confirm_kernel (ConfirmArgs: n_entries, n_bytes, n_class_words) and the kernel's own test (kernels.h)
    const uint32_t n_entries = (uint32_t)t.entries.size(), n_bytes = confirm_table_bytes(t.bytes.size()), n_class_words = (uint32_t)t.classes.size();
    const bool in_lds = confirm_tables_fit(n_entries, n_bytes, n_class_words);
    uint32_t longest = 0, top_class = 0, widest = 0, walk = 0;
    for (const ConfirmEntry &e : t.entries) {
        longest = std::max<uint32_t>(longest, e.len);
        if (e.atom == kConfirmWalk) walk = 1;
        const size_t cls = (size_t)e.bytes_off + 2u * ((e.len + 3u) & ~3u);  // behind the value and the mask: n_cls x {position, class id}
        for (uint32_t k = 0; k < e.n_cls && cls + 2u * k < t.bytes.size(); k++) top_class = std::max<uint32_t>(top_class, t.bytes[cls + 2u * k]);
    }
    for (const uint32_t hd : t.head) widest = std::max(widest, hd >> 20);
    out[0] = n_entries;
    out[1] = n_bytes;
    out[2] = n_class_words;
    out[3] = in_lds ? 1u : 0u;
    out[4] = longest;
    out[5] = top_class;
    out[6] = widest;
    out[7] = walk;
    return PWAF_OK;
}

}  // extern "C"
namespace {
// the plan the list-scan hooks answer from: built on the first call, again after pwaf_program_tune / pwaf_engine_tune
const ProgramScans &scans_of(const pwaf_program *p) {
    auto *mp = const_cast<pwaf_program *>(p);
    if (!mp->scans) {
        mp->mean_len.resize(std::max<size_t>(mp->mean_len.size(), PWAF_N_FIELDS + p->p->header_names.size()), 0.0);
        mp->scans.reset(new ProgramScans());
        plan_program_scans(*p->p, mp->tuned.get(), mp->mean_len, *mp->scans);
    }
    return *mp->scans;
}
template <class T>
void put_section(std::vector<uint8_t> &buf, const char tag[4], uint32_t count, const std::vector<T> &v) {
    const uint64_t len = v.size() * sizeof(T);
    const auto raw = [&](const void *q, size_t n) { buf.insert(buf.end(), (const uint8_t *)q, (const uint8_t *)q + n); };
    raw(tag, 4);
    raw(&count, 4);
    raw(&len, 8);
    if (len) raw(v.data(), (size_t)len);
    while (buf.size() % 8) buf.push_back(0);
}
}  // namespace
extern "C" {

size_t pwaf_program_flat_image(const pwaf_program *p, uint32_t group, uint32_t tier, uint8_t *buf, size_t cap) {
    if (!p || !p->p || group >= p->p->groups.size() || tier > 1) { fail(PWAF_E_INVALID_ARG, "pwaf_program_flat_image: bad argument"); return 0; }
    const ProgramScans &sc = scans_of(p);
    const FlatImage &m = tier ? sc.rtier[group] : sc.full[group];
    if (!m.n_states) { fail(PWAF_E_INVALID_ARG, "the pass has no R tier"); return 0; }
    std::vector<uint8_t> out{'P', 'W', 'A', 'F', 'P', 'R', 'G', '1'};
    put_section(out, "FSHP", group, std::vector<uint32_t>{m.n_states, m.n_classes, m.scalar_mode, m.ill_class, m.n_full, m.n_delta, tier ? sc.rtier_lds[group] : sc.full_lds[group]});
    put_section(out, "FFLT", group, m.flat);
    put_section(out, "FDLT", group, m.delta);
    put_section(out, "FCLS", group, m.classmap);
    put_section(out, "FEMO", group, m.emit_off);
    put_section(out, "FEML", group, m.emit_list);
    put_section(out, "FENO", group, m.end_off);
    put_section(out, "FENL", group, m.end_list);
    if (buf && cap) memcpy(buf, out.data(), std::min(cap, out.size()));
    return out.size();
}

uint32_t pwaf_engine_compute_units(const pwaf_engine *e) { return e ? e->n_cus : 0u; }

int pwaf_program_list_scans(const pwaf_program *p, uint32_t *out, size_t cap, size_t *n_descs) {
    if (!p || !p->p || !n_descs || (!out && cap)) return fail(PWAF_E_INVALID_ARG, "pwaf_program_list_scans: bad argument");
    const ProgramScans &sc = scans_of(p);
    size_t at = 0;
    for (int phase = 0; phase < 2; phase++) {
        const std::vector<ListDesc> &descs = sc.lists.descs[phase];
        const std::vector<uint32_t> &launches = sc.passes.lscan_launches[phase];
        size_t planned = 0;
        for (const uint32_t c : launches) planned += c;
        if (planned != descs.size()) return fail(PWAF_E_UNSUPPORTED, "list-scan launch plan does not match the descriptors");  // (run_pipeline's own check)
        size_t launch = 0, first = 0;
        for (size_t k = 0; k < descs.size(); k++, at++) {
            while (k >= first + launches[launch]) first += launches[launch++];
            if (at >= cap) continue;
            const ListDesc &d = descs[k];
            const ListShape &sh = sc.lists.shapes[phase];
            const uint32_t w[PWAF_LIST_SCAN_WORDS] = {d.phase, d.pass, d.rtier ? 1u : 0u, sh.threads, list_hot_bytes(sh), d.n_hot, d.n_delta, d.behind_filter ? 1u : 0u,
                                                      d.merge_rec ? 1u : 0u, d.dense_mode, d.share_owner >= 0 ? (uint32_t)d.share_owner : 0xFFFFFFFFu, d.need_bit, (uint32_t)launch,
                                                      launches[launch], sh.wg_per_cu, 0u};
            memcpy(out + at * PWAF_LIST_SCAN_WORDS, w, sizeof w);
        }
    }
    *n_descs = at;
    return PWAF_OK;
}

}  // extern "C"
namespace {
int evaluate_device_impl(pwaf_engine *e, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, uint32_t *match_idx, uint32_t *n_matches, pwaf_geo *geo, void *stream,
                         const ReportOut *rep = nullptr) {
    int rc = validate_batch_header(in);
    if (rc) return rc;
    if (in->memory != PWAF_MEM_DEVICE) return fail(PWAF_E_INVALID_ARG, "pwaf_evaluate_device needs a DEVICE batch");
    if ((match_idx == nullptr) != (n_matches == nullptr)) return fail(PWAF_E_INVALID_ARG, "match_idx and n_matches must be given together");
    HIP_TRY(hipSetDevice(e->device));
    // Re-entrant: the call takes the next scratch context of the ring; the caller's stream first waits (on the device) for whoever
    // used that context before, and leaves its own completion event behind. Calls on different streams therefore overlap.
    std::unique_lock<std::mutex> lock;
    bool must_wait;
    Scratch &S = acquire_context(e, false, (hipStream_t)stream, lock, must_wait);
    if ((rc = S.ensure(false))) return rc;
    if (must_wait) HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, S.done, 0));
    rc = run_pipeline(e, S, *in, out, counts, match_idx, n_matches, (hipStream_t)stream, false, nullptr, false, geo, rep);
    const hipError_t he = mark_context_used(S, (hipStream_t)stream, false);
    return he != hipSuccess ? device_error("hipEventRecord", he) : rc;
}

// `geo` (nullable; PWAF_OPT_GEO_ANSWERS engines only): the GeoIP record of every request, where `out` lives
// `rep` (nullable): the call's report — rule hits (PWAF_OPT_RULE_HITS engines; overwritten) or routes (engines with routes) — where `out` lives
int evaluate_batch_impl(pwaf_engine *e, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, pwaf_geo *geo, const ReportOut *rep = nullptr) {
    int rc = validate_batch_header(in);
    if (rc) return rc;
    if (rep && !rep->any()) rep = nullptr;
    uint32_t *const route = rep ? rep->route : nullptr;  // (nullable; engines with routes only) every request's route, where `out` lives
    const bool want_hits = rep && rep->hit_any();
    const size_t rule_hit_bytes = (size_t)e->prog.p->n_user_rules * 8;
    if (in->n == 0) {
        if (counts && in->memory == PWAF_MEM_HOST) memset(counts, 0, sizeof *counts);
        if (!want_hits) return PWAF_OK;
        if (in->memory == PWAF_MEM_HOST) {
            if (rep->n_hits) *rep->n_hits = 0;
            if (rep->rule_hits) memset(rep->rule_hits, 0, rule_hit_bytes);
        } else {
            HIP_TRY(hipSetDevice(e->device));
            if (rep->n_hits) HIP_TRY(hipMemset(rep->n_hits, 0, 4));
            if (rep->rule_hits && rule_hit_bytes) HIP_TRY(hipMemset(rep->rule_hits, 0, rule_hit_bytes));
        }
        return PWAF_OK;
    }
    HIP_TRY(hipSetDevice(e->device));
    // the context is held for the whole call (its staging buffers and its stream are reused); other threads take other contexts
    std::unique_lock<std::mutex> lock;
    bool must_wait;
    Scratch &S = acquire_context(e, true, nullptr, lock, must_wait);
    if ((rc = S.ensure(true))) return rc;
    hipStream_t s = S.stream;
    if (must_wait) HIP_TRY(hipStreamWaitEvent(s, S.done, 0));
    if (in->memory == PWAF_MEM_DEVICE) return run_with_retry(e, S, *in, out, counts, false, nullptr, false, [] { return PWAF_OK; }, geo, rep);
    // a HOST batch's rule hits: produced into staging buffers of the context ({n_hits, pad, rule_hits[]}; the list), fetched once the batch is
    // done and the number of entries is known — only the entries the batch wrote travel, the rest of the caller's list is left alone
    ReportOut dh;
    if (want_hits) {
        if ((rc = S.stage_hit_counts.reserve(8 + rule_hit_bytes)) || (rc = S.stage_hits.reserve(std::max<size_t>(16, (size_t)rep->cap * sizeof(pwaf_rule_hit))))) return rc;
        if (rep->n_hits) {
            dh.hits = (pwaf_rule_hit *)S.stage_hits.p;
            dh.cap = rep->cap;
            dh.n_hits = (uint32_t *)S.stage_hit_counts.p;
        }
        if (rep->rule_hits) dh.rule_hits = (uint64_t *)((char *)S.stage_hit_counts.p + 8);
    }
    const ReportOut *const d_rep = rep ? &dh : nullptr;
    auto fetch_hits = [&](int code) -> int {
        if (code || !want_hits) return code;
        std::vector<uint64_t> back(1 + rule_hit_bytes / 8);
        HIP_TRY(hipMemcpyAsync(back.data(), S.stage_hit_counts.p, back.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (rep->rule_hits && rule_hit_bytes) memcpy(rep->rule_hits, back.data() + 1, rule_hit_bytes);
        if (rep->n_hits) {
            const uint32_t total = (uint32_t)back[0], got = std::min(total, rep->cap);
            *rep->n_hits = total;
            if (got) {
                HIP_TRY(hipMemcpyAsync(rep->hits, S.stage_hits.p, (size_t)got * sizeof(pwaf_rule_hit), hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
            }
        }
        return PWAF_OK;
    };
    // HOST batch: stage, validate what a device cannot report (while the copies are in flight, when the caller's memory is page-locked:
    // pwaf_host_alloc / pwaf_host_register), run, copy back
    const uint32_t n = in->n;
    // host view of every string column by field id (five fields + the header columns the batch carries; the others read as "")
    const uint32_t n_hdr_in = in->headers ? std::min<uint32_t>(in->n_headers, e->n_fields - PWAF_N_FIELDS) : 0u;
    auto host_col = [&](uint32_t f) -> const pwaf_strcol * {
        if (f < PWAF_N_FIELDS) return &in->field[f];
        const uint32_t k = f - PWAF_N_FIELDS;
        return (k < n_hdr_in && in->headers[k].data && in->headers[k].offsets) ? &in->headers[k] : nullptr;
    };
    auto validate = [&]() -> int {
        for (uint32_t f = 0; f < e->n_fields; f++) {
            const pwaf_strcol *c = host_col(f);
            if (!c) continue;
            const uint32_t *o = c->offsets;
            uint32_t bad = 0;
            for (uint32_t i = 0; i < n; i++) bad |= (uint32_t)(o[i + 1] < o[i]);  // (branch-free: the loop vectorizes)
            if (bad) return fail(PWAF_E_BATCH, "field offsets are not monotone");
        }
        if (in->country) {
            uint32_t bad = 0;
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t c0 = (in->country[i] & 0xFFu) - 'A', c1 = ((uint32_t)in->country[i] >> 8) - 'A';
                bad |= (uint32_t)(c0 > 25u) | (uint32_t)(c1 > 25u);
            }
            if (bad) return fail(PWAF_E_BATCH, "country is not two letters A-Z (pingoo/geoip.rs:128-142)");
        }
        return PWAF_OK;
    };
    // the ends must be ordered before any size is computed from them (the full check follows)
    for (uint32_t f = 0; f < e->n_fields; f++) {
        const pwaf_strcol *c = host_col(f);
        if (c && c->offsets[n] < c->offsets[0]) return fail(PWAF_E_BATCH, "field offsets are not monotone");
    }
    DeviceBatch dv(n, e->n_fields);
    std::vector<uint32_t> col_begin(e->n_fields, 0);

    // ---- small batches: ONE packed block ----
    // [offsets + arena of every column] [ip] [v6] [port] [flags] [asn] [country] [counters] | [verdicts], each 256-byte aligned. The
    // micro-batcher's batches and pwaf_evaluate_one's single requests paid ~25 small copies from pageable memory (each a blocking staged
    // copy) and two waits per batch; now: memcpy into page-locked memory, one copy in, one out, one wait.
    static constexpr size_t kPackMax = 1u << 20;
    Layout pk;
    bool packable = true;
    std::vector<size_t> at_off(e->n_fields, 0), at_data(e->n_fields, 0);
    for (uint32_t f = 0; f < e->n_fields && packable; f++) {
        const pwaf_strcol *c = host_col(f);
        if (!c) continue;
        if (c->offsets[0] != 0) { packable = false; break; }  // (a slab view of a larger arena keeps its positions: the column-by-column path)
        at_off[f] = pk.take((size_t)(n + 1) * 4);
        at_data[f] = pk.take((size_t)c->offsets[n] + PWAF_ARENA_PAD);
        if (pk.size() > kPackMax) packable = false;
    }
    const size_t at_ip = pk.take((size_t)n * 16), at_v6 = pk.take(n), at_port = pk.take((size_t)n * 2), at_flags = pk.take(n);
    const size_t at_asn = in->asn ? pk.take((size_t)n * 4) : 0, at_cc = in->asn ? pk.take((size_t)n * 2) : 0;
    const size_t at_counts = pk.take(sizeof(pwaf_counts));  // (arrive zeroed with the inputs, return with the verdicts)
    const size_t in_bytes = pk.size();
    const size_t at_out = pk.take((size_t)n * sizeof(pwaf_verdict));
    const size_t at_geo = geo ? pk.take((size_t)n * sizeof(pwaf_geo)) : 0;  // (returns with the verdicts)
    const size_t at_route = route ? pk.take((size_t)n * 4) : 0;             // (the same)
    const size_t need = pk.size();
    if (packable && need <= kPackMax && !switches().no_packed_staging) {
        if ((rc = validate())) return rc;
        if ((rc = S.pin_in.reserve(in_bytes)) || (rc = S.pin_out.reserve(need - at_counts)) || (rc = S.packed.reserve(need))) return rc;
        uint8_t *const h = (uint8_t *)S.pin_in.p;
        const uint8_t *const d = (const uint8_t *)S.packed.p;
        for (uint32_t f = 0; f < e->n_fields; f++) {
            const pwaf_strcol *c = host_col(f);
            if (!c) continue;
            const uint32_t hi = c->offsets[n];
            memcpy(h + at_off[f], c->offsets, (size_t)(n + 1) * 4);
            if (hi) memcpy(h + at_data[f], c->data, hi);
            memset(h + at_data[f] + hi, 0, PWAF_ARENA_PAD);
            dv.set_col(f, d + at_data[f], d + at_off[f], hi);
        }
        memcpy(h + at_ip, in->ip, (size_t)n * 16);
        memcpy(h + at_v6, in->ip_is_v6, n);
        memcpy(h + at_port, in->port, (size_t)n * 2);
        memcpy(h + at_flags, in->flags, n);
        if (in->asn) {
            memcpy(h + at_asn, in->asn, (size_t)n * 4);
            memcpy(h + at_cc, in->country, (size_t)n * 2);
        }
        dv.set_fixed(d + at_ip, d + at_v6, d + at_port, d + at_flags, in->asn ? d + at_asn : nullptr, in->asn ? d + at_cc : nullptr);
        memset(h + at_counts, 0, sizeof(pwaf_counts));
        HIP_TRY(hipMemcpyAsync(S.packed.p, h, in_bytes, hipMemcpyHostToDevice, s));
        pwaf_verdict *const d_out = (pwaf_verdict *)((char *)S.packed.p + at_out);
        pwaf_counts *const d_counts = (pwaf_counts *)((char *)S.packed.p + at_counts);
        const size_t back = need - at_counts;
        if (route) dh.route = (uint32_t *)((char *)S.packed.p + at_route);
        rc = run_with_retry(e, S, dv.db, d_out, d_counts, true, &col_begin, true, [&]() -> int {
            HIP_TRY(hipMemcpyAsync(S.pin_out.p, d_counts, back, hipMemcpyDeviceToHost, s));
            return PWAF_OK;
        }, geo ? (pwaf_geo *)((char *)S.packed.p + at_geo) : nullptr, d_rep);
        if ((rc = fetch_hits(rc))) return rc;
        if (geo) memcpy(geo, (const char *)S.pin_out.p + (at_geo - at_counts), (size_t)n * sizeof(pwaf_geo));
        if (route) memcpy(route, (const char *)S.pin_out.p + (at_route - at_counts), (size_t)n * 4);
        memcpy(out, (const char *)S.pin_out.p + (at_out - at_counts), (size_t)n * sizeof(pwaf_verdict));
        if (counts) memcpy(counts, S.pin_out.p, sizeof(pwaf_counts));
        return PWAF_OK;
    }

    // ---- large batches: column by column, straight from the caller's buffers (page-locked ones are read by the copy engine while this
    //      thread goes on: pwaf_host_alloc / pwaf_host_register) ----
    if (S.stage_field_data.size() < e->n_fields) { S.stage_field_data.resize(e->n_fields); S.stage_field_off.resize(e->n_fields); }
    auto bail = [&](int code) { (void)hipStreamSynchronize(s); return code; };  // (copies in flight read the caller's buffers)
    for (uint32_t f = 0; f < e->n_fields; f++) {
        const pwaf_strcol *c = host_col(f);
        if (!c) continue;
        const uint32_t *o = c->offsets;
        const size_t lo = o[0], hi = o[n];
        col_begin[f] = (uint32_t)lo;
        // offsets are used unchanged on the device: the arena keeps its positions, but only the batch's own bytes [off[0], off[n]) travel
        // (a slab view of a larger batch — pwaf_node_evaluate_batch — does not re-send what lies before it)
        if ((rc = S.stage_field_data[f].reserve(hi + PWAF_ARENA_PAD))) return bail(rc);
        if ((rc = S.stage_field_off[f].reserve((size_t)(n + 1) * 4))) return bail(rc);
        if (hi > lo) HIP_TRY(hipMemcpyAsync((char *)S.stage_field_data[f].p + lo, c->data + lo, hi - lo, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync((char *)S.stage_field_data[f].p + hi, 0, PWAF_ARENA_PAD, s));
        HIP_TRY(hipMemcpyAsync(S.stage_field_off[f].p, o, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, s));
        dv.set_col(f, S.stage_field_data[f].p, S.stage_field_off[f].p, (uint32_t)hi);
    }
    auto stage = [&](DevBuf &b, const void *src, size_t bytes) -> int {
        int r = b.reserve(bytes);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s));
        return PWAF_OK;
    };
    if ((rc = stage(S.stage_ip, in->ip, (size_t)n * 16)) || (rc = stage(S.stage_v6, in->ip_is_v6, n)) || (rc = stage(S.stage_port, in->port, (size_t)n * 2)) ||
        (rc = stage(S.stage_flags, in->flags, n)))
        return bail(rc);
    if (in->asn && ((rc = stage(S.stage_asn, in->asn, (size_t)n * 4)) || (rc = stage(S.stage_country, in->country, (size_t)n * 2)))) return bail(rc);
    dv.set_fixed(S.stage_ip.p, S.stage_v6.p, S.stage_port.p, S.stage_flags.p, in->asn ? S.stage_asn.p : nullptr, in->asn ? S.stage_country.p : nullptr);
    if ((rc = S.stage_out.reserve((size_t)n * sizeof(pwaf_verdict)))) return bail(rc);
    if ((rc = S.stage_counts.reserve(sizeof(pwaf_counts)))) return bail(rc);
    if (geo && (rc = S.stage_geo.reserve((size_t)n * sizeof(pwaf_geo)))) return bail(rc);
    if (route) {
        if ((rc = S.stage_route.reserve((size_t)n * 4))) return bail(rc);
        dh.route = (uint32_t *)S.stage_route.p;
    }
    if ((rc = validate())) return bail(rc);
    return fetch_hits(run_with_retry(e, S, dv.db, (pwaf_verdict *)S.stage_out.p, (pwaf_counts *)S.stage_counts.p, true, &col_begin, false, [&]() -> int {
        HIP_TRY(hipMemcpyAsync(out, S.stage_out.p, (size_t)n * sizeof(pwaf_verdict), hipMemcpyDeviceToHost, s));
        if (counts) HIP_TRY(hipMemcpyAsync(counts, S.stage_counts.p, sizeof(pwaf_counts), hipMemcpyDeviceToHost, s));
        if (geo) HIP_TRY(hipMemcpyAsync(geo, S.stage_geo.p, (size_t)n * sizeof(pwaf_geo), hipMemcpyDeviceToHost, s));
        if (route) HIP_TRY(hipMemcpyAsync(route, S.stage_route.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        return PWAF_OK;
    }, geo ? (pwaf_geo *)S.stage_geo.p : nullptr, d_rep));
}
}  // namespace

extern "C" {

int pwaf_evaluate_device(pwaf_engine *e, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, uint32_t *match_idx, uint32_t *n_matches, void *stream) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    return evaluate_device_impl(e, in, out, counts, match_idx, n_matches, nullptr, stream);
}
int pwaf_evaluate_device_geo(pwaf_engine *e, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, uint32_t *match_idx, uint32_t *n_matches, pwaf_geo *geo, void *stream) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    if (int rc = need_geo_answers(e, "pwaf_evaluate_device_geo")) return rc;
    return evaluate_device_impl(e, in, out, counts, match_idx, n_matches, geo, stream);
}

int pwaf_evaluate_batch(pwaf_engine *e, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    return evaluate_batch_impl(e, in, out, counts, nullptr);
}
// The plain entry points with the rule-hit outputs (PWAF_OPT_RULE_HITS; include/pwaf.h). All of them NULL: exactly the plain call.
int pwaf_evaluate_batch_hits(pwaf_engine *e, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, pwaf_rule_hit *hits, uint32_t hits_cap, uint32_t *n_hits,
                             uint64_t *rule_hits) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    ReportOut h;
    h.hits = hits; h.cap = hits ? hits_cap : 0u; h.n_hits = n_hits; h.rule_hits = rule_hits;
    if (int rc = check_hit_args(e, "pwaf_evaluate_batch_hits", h)) return rc;
    return evaluate_batch_impl(e, in, out, counts, nullptr, &h);
}
int pwaf_evaluate_device_hits(pwaf_engine *e, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, uint32_t *match_idx, uint32_t *n_matches, pwaf_rule_hit *hits,
                              uint32_t hits_cap, uint32_t *n_hits, uint64_t *rule_hits, void *stream) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    ReportOut h;
    h.hits = hits; h.cap = hits ? hits_cap : 0u; h.n_hits = n_hits; h.rule_hits = rule_hits;
    if (int rc = check_hit_args(e, "pwaf_evaluate_device_hits", h)) return rc;
    return evaluate_device_impl(e, in, out, counts, match_idx, n_matches, nullptr, stream, &h);
}
// The plain entry points with the route output (engines created with routes; include/pwaf.h). route == NULL: exactly the plain call.
int pwaf_evaluate_batch_routes(pwaf_engine *e, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, uint32_t *route) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    if (!route) return evaluate_batch_impl(e, in, out, counts, nullptr);
    if (int rc = need_routes(e, "pwaf_evaluate_batch_routes")) return rc;
    ReportOut h;
    h.route = route;
    return evaluate_batch_impl(e, in, out, counts, nullptr, &h);
}
int pwaf_evaluate_device_routes(pwaf_engine *e, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, uint32_t *match_idx, uint32_t *n_matches, uint32_t *route,
                                void *stream) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    if (!route) return evaluate_device_impl(e, in, out, counts, match_idx, n_matches, nullptr, stream);
    if (int rc = need_routes(e, "pwaf_evaluate_device_routes")) return rc;
    ReportOut h;
    h.route = route;
    return evaluate_device_impl(e, in, out, counts, match_idx, n_matches, nullptr, stream, &h);
}
int pwaf_evaluate_batch_geo(pwaf_engine *e, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, pwaf_geo *geo) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    if (int rc = need_geo_answers(e, "pwaf_evaluate_batch_geo")) return rc;
    return evaluate_batch_impl(e, in, out, counts, geo);
}

// The GeoIP records of n addresses, nothing else: georec_kernel alone. DEVICE memory: enqueued on `stream`; HOST memory: staged through a
// context of the engine, launched on its stream, copied back, waited for.
int pwaf_geoip_lookup(pwaf_engine *e, const uint8_t *ip, const uint8_t *ip_is_v6, uint32_t n, uint32_t memory, pwaf_geo *out, void *stream) {
    if (!e || (n && (!ip || !ip_is_v6 || !out))) return fail(PWAF_E_INVALID_ARG, "pwaf_geoip_lookup: NULL argument");
    if (memory != PWAF_MEM_HOST && memory != PWAF_MEM_DEVICE) return fail(PWAF_E_INVALID_ARG, "pwaf_geoip_lookup: memory is neither HOST nor DEVICE");
    int rc = need_geo_answers(e, "pwaf_geoip_lookup");
    if (rc) return rc;
    if (n == 0) return PWAF_OK;
    HIP_TRY(hipSetDevice(e->device));
    GeoRecArgs ga{};
    set_georec_args(e, ga);
    ga.n = n;
    if (memory == PWAF_MEM_DEVICE) {
        ga.ip = ip;
        ga.ip_is_v6 = ip_is_v6;
        ga.out = (uint2 *)out;
        KernelTimer prof(e, (hipStream_t)stream);
        if ((rc = prof.begin())) return rc;
        if (const int he = launch_georec(ga, stream)) return fail(PWAF_E_DEVICE, std::string("georec kernel launch failed: ") + hipGetErrorString((hipError_t)he));
        if ((rc = prof.end("georec", 25ull * n))) return rc;
        prof.commit();
        return PWAF_OK;
    }
    std::unique_lock<std::mutex> lock;
    bool must_wait;
    Scratch &S = acquire_context(e, true, nullptr, lock, must_wait);
    if ((rc = S.ensure(true))) return rc;
    const hipStream_t s = S.stream;
    if (must_wait) HIP_TRY(hipStreamWaitEvent(s, S.done, 0));
    if ((rc = S.stage_ip.reserve((size_t)n * 16)) || (rc = S.stage_v6.reserve(n)) || (rc = S.stage_geo.reserve((size_t)n * sizeof(pwaf_geo)))) return rc;
    ga.ip = (const uint8_t *)S.stage_ip.p;
    ga.ip_is_v6 = (const uint8_t *)S.stage_v6.p;
    ga.out = (uint2 *)S.stage_geo.p;
    hipError_t he = hipMemcpyAsync(S.stage_ip.p, ip, (size_t)n * 16, hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(S.stage_v6.p, ip_is_v6, n, hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = (hipError_t)launch_georec(ga, s);
    if (he == hipSuccess) he = hipMemcpyAsync(out, S.stage_geo.p, (size_t)n * sizeof(pwaf_geo), hipMemcpyDeviceToHost, s);
    const hipError_t re = mark_context_used(S, s, true), se = hipStreamSynchronize(s);  // (what was enqueued reads the caller's buffers)
    if (he != hipSuccess) return device_error("pwaf_geoip_lookup", he);
    if (re != hipSuccess) return device_error("hipEventRecord", re);
    if (se != hipSuccess) return device_error("hipStreamSynchronize", se);
    return PWAF_OK;
}

// Page-locked host memory for batch columns: the copy engine reads it directly (no staging copy inside the runtime, the calling thread
// goes on while the copy runs). A listener that parses requests into such arenas hands pwaf_evaluate_batch its bytes at PCIe speed.
int pwaf_host_alloc(size_t bytes, void **out) {
    if (!out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    *out = nullptr;
    hipError_t he = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocPortable);
    if (he != hipSuccess) { *out = nullptr; return fail(PWAF_E_NOMEM, std::string("hipHostMalloc failed: ") + hipGetErrorString(he)); }
    return PWAF_OK;
}
void pwaf_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}
int pwaf_host_register(void *p, size_t bytes) {
    if (!p || !bytes) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterPortable));
    return PWAF_OK;
}
int pwaf_host_unregister(void *p) {
    if (!p) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    HIP_TRY(hipHostUnregister(p));
    return PWAF_OK;
}

// ---- request records (ABI 4) ----
namespace {
// The caller's [p, p + bytes) lies in ONE page-locked allocation (pwaf_host_alloc / pwaf_host_register): the copy engine can read it
// directly. Anything else (pageable memory, a range across two registrations) is staged.
bool page_locked(const void *p, size_t bytes) {
    hipPointerAttribute_t a{}, b{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess || hipPointerGetAttributes(&b, (const char *)p + bytes - 1) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost && b.type == hipMemoryTypeHost && a.devicePointer && b.devicePointer &&
           (const char *)b.devicePointer - (const char *)a.devicePointer == (ptrdiff_t)(bytes - 1);
}
}  // namespace

static_assert(pwaf::records::kMaxValues == PWAF_N_FIELDS + kMaxHeaders, "records.h kMaxValues must follow program.h kMaxHeaders");

}  // extern "C"
namespace {
// `geo` (nullable; host memory, n entries; PWAF_OPT_GEO_ANSWERS engines only): the GeoIP record of every request
int evaluate_records_impl(pwaf_engine *e, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n, pwaf_verdict *out, pwaf_counts *counts, pwaf_geo *geo_out) {
    namespace R = pwaf::records;
    if (e->n_fields > R::kMaxValues) return fail(PWAF_E_UNSUPPORTED, "the engine has more columns than a record can carry");
    if (n == 0) {
        if (counts) memset(counts, 0, sizeof *counts);
        return PWAF_OK;
    }
    // the host reads the heads and lengths only: validation (nothing is launched for a malformed call) and the column offsets
    const uint32_t n_cols = e->n_fields;
    std::vector<uint64_t> totals(n_cols);
    uint32_t bad = 0;
    int geo = 0;
    uint64_t lo = 0, hi = 0;
    const int chk = R::validate(buf, buf_bytes, rec_off, n, n_cols, totals.data(), &bad, &geo, &lo, &hi);
    if (chk != R::kOk) return fail(PWAF_E_BATCH, "record " + std::to_string(bad) + " (offset " + std::to_string(rec_off[bad]) + "): " + R::check_message(chk));
    HIP_TRY(hipSetDevice(e->device));
    std::unique_lock<std::mutex> lock;
    bool must_wait;
    Scratch &S = acquire_context(e, true, nullptr, lock, must_wait);
    int rc;
    if ((rc = S.ensure(true))) return rc;
    hipStream_t s = S.stream;
    if (must_wait) HIP_TRY(hipStreamWaitEvent(s, S.done, 0));
    // rec_meta: [record offsets (relative to lo)] [column offsets, n + 1 per column] [column places] [counters | verdicts] [records]
    Layout meta;
    const size_t off_stride = ((size_t)n + 1 + 63) & ~(size_t)63;
    const size_t at_recoff = meta.take((size_t)n * 4), at_off = meta.take(off_stride * 4 * n_cols), at_colat = meta.take((size_t)n_cols * 8);
    const size_t at_counts = meta.take(sizeof(pwaf_counts)), up_bytes = meta.size(), at_out = meta.take((size_t)n * sizeof(pwaf_verdict));
    const size_t at_geo = geo_out ? meta.take((size_t)n * sizeof(pwaf_geo)) : 0;  // (comes back with the verdicts)
    const size_t span = (size_t)(hi - lo), at_rec = meta.take(span), need = meta.size();
    const bool direct = page_locked(buf + lo, span);
    if ((rc = S.rec_meta.reserve(need)) || (rc = S.rec_pin.reserve(direct ? up_bytes : need)) || (rc = S.rec_back.reserve(at_rec - at_counts))) return rc;
    uint8_t *const h = (uint8_t *)S.rec_pin.p;
    uint32_t *const h_recoff = (uint32_t *)(h + at_recoff);
    for (uint32_t i = 0; i < n; i++) h_recoff[i] = (uint32_t)(rec_off[i] - lo);
    R::column_offsets(buf, rec_off, n, n_cols, (uint32_t *)(h + at_off), off_stride);
    // rec_cols: [column arenas, each with its PWAF_ARENA_PAD] [ip] [v6] [port] [flags] [asn] [country]
    Layout cl;
    uint64_t *const colat = (uint64_t *)(h + at_colat);
    for (uint32_t f = 0; f < n_cols; f++) colat[f] = cl.take(totals[f] + PWAF_ARENA_PAD);
    const size_t c_ip = cl.take((size_t)n * 16), c_v6 = cl.take(n), c_port = cl.take((size_t)n * 2), c_flags = cl.take(n);
    const size_t c_asn = geo ? cl.take((size_t)n * 4) : 0, c_cc = geo ? cl.take((size_t)n * 2) : 0;
    if ((rc = S.rec_cols.reserve(cl.size()))) return rc;
    memset(h + at_counts, 0, sizeof(pwaf_counts));
    uint8_t *const d = (uint8_t *)S.rec_meta.p;
    uint8_t *const dc = (uint8_t *)S.rec_cols.p;
    HIP_TRY(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, s));
    if (direct) {
        HIP_TRY(hipMemcpyAsync(d + at_rec, buf + lo, span, hipMemcpyHostToDevice, s));
    } else {
        memcpy(h + at_rec, buf + lo, span);
        HIP_TRY(hipMemcpyAsync(d + at_rec, h + at_rec, span, hipMemcpyHostToDevice, s));
    }
    R::UnpackArgs ua{};
    ua.rec = d + at_rec;
    ua.rec_off = (const uint32_t *)(d + at_recoff);
    ua.n = n;
    ua.n_cols = n_cols;
    ua.arena = dc;
    ua.col_at = (const uint64_t *)(d + at_colat);
    ua.off = (const uint32_t *)(d + at_off);
    ua.off_stride = (uint32_t)off_stride;
    ua.ip = dc + c_ip;
    ua.ip_is_v6 = dc + c_v6;
    ua.port = (uint16_t *)(dc + c_port);
    ua.flags = dc + c_flags;
    ua.asn = geo ? (uint32_t *)(dc + c_asn) : nullptr;
    ua.country = geo ? (uint16_t *)(dc + c_cc) : nullptr;
    if (R::launch_unpack_records(ua, s)) {
        (void)hipStreamSynchronize(s);  // (the copies in flight read the caller's buffer)
        return fail(PWAF_E_DEVICE, "unpack_records_kernel launch failed");
    }
    // the device batch the kernel writes: an ordinary DEVICE batch with every column's size known on the host
    DeviceBatch dv(n, n_cols);
    for (uint32_t f = 0; f < n_cols; f++) dv.set_col(f, dc + colat[f], (const uint32_t *)(d + at_off) + (size_t)f * off_stride, (uint32_t)totals[f]);
    dv.set_fixed(ua.ip, ua.ip_is_v6, ua.port, ua.flags, ua.asn, ua.country);
    const std::vector<uint32_t> col_begin(n_cols, 0);
    pwaf_counts *const d_counts = (pwaf_counts *)(d + at_counts);
    // (the counters arrive zeroed with the staged block; counters + verdicts come back in one copy)
    rc = run_with_retry(e, S, dv.db, (pwaf_verdict *)(d + at_out), d_counts, true, &col_begin, true, [&]() -> int {
        HIP_TRY(hipMemcpyAsync(S.rec_back.p, d_counts, at_rec - at_counts, hipMemcpyDeviceToHost, s));
        return PWAF_OK;
    }, geo_out ? (pwaf_geo *)(d + at_geo) : nullptr);
    if (rc) return rc;
    memcpy(out, (const char *)S.rec_back.p + (at_out - at_counts), (size_t)n * sizeof(pwaf_verdict));
    if (geo_out) memcpy(geo_out, (const char *)S.rec_back.p + (at_geo - at_counts), (size_t)n * sizeof(pwaf_geo));
    if (counts) memcpy(counts, S.rec_back.p, sizeof(pwaf_counts));
    return PWAF_OK;
}

// Records that already lie in DEVICE memory. What the host does above — validate every record, turn the lengths into
// column offsets — runs on the device here (records_scan.hip), on the caller's stream; the host waits for that stream ONCE, for the
// summary block (failure key, m, has_geoip, the column totals), because the arenas it reserves next and the pipeline's launch plan are
// sized from the totals. Everything behind the wait is enqueued and the call returns, like pwaf_evaluate_device.
int evaluate_records_device_impl(pwaf_engine *e, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n, const uint32_t *n_rec, pwaf_verdict *out,
                                 pwaf_counts *counts, uint32_t *match_idx, uint32_t *n_matches, hipStream_t stream) {
    namespace R = pwaf::records;
    if (e->n_fields > R::kMaxValues) return fail(PWAF_E_UNSUPPORTED, "the engine has more columns than a record can carry");
    if ((match_idx == nullptr) != (n_matches == nullptr)) return fail(PWAF_E_INVALID_ARG, "match_idx and n_matches must be given together");
    if ((uintptr_t)buf & 15u) return fail(PWAF_E_INVALID_ARG, "pwaf_evaluate_records_device: buf is not 16-byte aligned");
    if (n == 0) return PWAF_OK;
    HIP_TRY(hipSetDevice(e->device));
    std::unique_lock<std::mutex> lock;
    bool must_wait;
    Scratch &S = acquire_context(e, false, stream, lock, must_wait);
    int rc;
    if ((rc = S.ensure(false))) return rc;
    if (must_wait) HIP_TRY(hipStreamWaitEvent(stream, S.done, 0));
    const uint32_t n_cols = e->n_fields;
    // rec_meta, from n and n_cols alone: [summary] [column places] [tile sums / bases, per column] [column offsets, n + 1 per column]
    Layout meta;
    const size_t off_stride = R::offsets_stride(n), tile_stride = ((size_t)R::scan_tiles(n) + 31) & ~(size_t)31;
    const size_t at_sum = meta.take(sizeof(R::ScanSummary)), at_colat = meta.take((size_t)n_cols * 8), at_tile = meta.take(tile_stride * 8 * n_cols),
                 at_off = meta.take(off_stride * 4 * n_cols);
    if (off_stride > 0xFFFFFFFFull) return fail(PWAF_E_UNSUPPORTED, "pwaf_evaluate_records_device: too many records for one call");
    if ((rc = S.rec_meta.reserve(meta.size())) || (rc = S.rec_pin.reserve(sizeof(R::ScanSummary)))) return rc;
    uint8_t *const d = (uint8_t *)S.rec_meta.p;
    R::ScanArgs sa{};
    sa.buf = buf, sa.buf_bytes = buf_bytes, sa.rec_off = rec_off, sa.n_rec = n_rec, sa.n = n, sa.n_cols = n_cols;
    sa.off = (uint32_t *)(d + at_off), sa.off_stride = (uint32_t)off_stride;
    sa.tile = (uint64_t *)(d + at_tile), sa.tile_stride = (uint32_t)tile_stride;
    sa.col_at = (uint64_t *)(d + at_colat), sa.sum = (R::ScanSummary *)(d + at_sum);
    const volatile R::ScanSummary *const sum = (const volatile R::ScanSummary *)S.rec_pin.p;
    // From the first launch on, whatever way the call leaves, the context remembers the stream (its next user waits for what was enqueued).
    auto body = [&]() -> int {
        R::UnpackArgs ua{};
        uint64_t colat[R::kMaxValues], totals[R::kMaxValues];
        uint32_t m = 0;
        {
            KernelTimer prof(e, stream);  // (released before run_pipeline takes its own)
            HIP_TRY(hipMemsetAsync(&sa.sum->key, 0xFF, 8, stream));  // records::kNoFailure
            const uint64_t alg[3] = {(uint64_t)n * (4 + R::kHead + 4ull * n_cols), (uint64_t)tile_stride * 16 * n_cols, (uint64_t)off_stride * 8 * n_cols};
            for (int phase = 1; phase <= 3; phase++) {
                if ((rc = prof.begin())) return rc;
                if (R::launch_scan_records(phase, sa, stream)) return fail(PWAF_E_DEVICE, std::string(R::kScanKernelNames[phase - 1]) + " launch failed");
                if ((rc = prof.end(R::kScanKernelNames[phase - 1], alg[phase - 1]))) return rc;
            }
            // the call's one wait: the summary block
            HIP_TRY(hipMemcpyAsync(S.rec_pin.p, sa.sum, R::summary_bytes(n_cols), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            prof.commit();
            const uint64_t key = sum->key;
            if (key != R::kNoFailure)
                return fail(PWAF_E_BATCH, "record " + std::to_string(R::key_index(key)) + " (offset " + std::to_string(sum->bad_off) + "): " + R::check_message(R::key_check(key)));
            m = sum->m;
            if (m == 0) return PWAF_OK;
            const bool geo = sum->has_geoip != 0;
            for (uint32_t f = 0; f < n_cols; f++) totals[f] = sum->totals[f];
            // rec_cols, from the totals: [column arenas, each with its PWAF_ARENA_PAD: records::place_columns] [ip] [v6] [port] [flags] [asn] [country]
            Layout cl;
            cl.used = (size_t)R::place_columns(totals, n_cols, colat);
            const size_t c_ip = cl.take((size_t)m * 16), c_v6 = cl.take(m), c_port = cl.take((size_t)m * 2), c_flags = cl.take(m);
            const size_t c_asn = geo ? cl.take((size_t)m * 4) : 0, c_cc = geo ? cl.take((size_t)m * 2) : 0;
            if ((rc = S.rec_cols.reserve(cl.size()))) return rc;
            uint8_t *const dc = (uint8_t *)S.rec_cols.p;
            ua.rec = buf;
            ua.rec_off = rec_off;
            ua.n = m;
            ua.n_cols = n_cols;
            ua.arena = dc;
            ua.col_at = sa.col_at;
            ua.off = sa.off;
            ua.off_stride = sa.off_stride;
            ua.ip = dc + c_ip;
            ua.ip_is_v6 = dc + c_v6;
            ua.port = (uint16_t *)(dc + c_port);
            ua.flags = dc + c_flags;
            ua.asn = geo ? (uint32_t *)(dc + c_asn) : nullptr;
            ua.country = geo ? (uint16_t *)(dc + c_cc) : nullptr;
            prof.last_main = -1;  // (the unpack's time begins at its own event, not in front of the wait)
            if ((rc = prof.begin())) return rc;
            if (R::launch_unpack_records(ua, stream)) return fail(PWAF_E_DEVICE, "unpack_records_kernel launch failed");
            uint64_t bytes = 0;
            for (uint32_t f = 0; f < n_cols; f++) bytes += totals[f];
            if ((rc = prof.end("unpack_records_kernel", 2 * bytes + (uint64_t)m * (R::kHead + 4ull * n_cols)))) return rc;
            prof.commit();
        }
        // an ordinary DEVICE batch with every column's size known on the host
        DeviceBatch dv(m, n_cols);
        for (uint32_t f = 0; f < n_cols; f++) dv.set_col(f, ua.arena + colat[f], sa.off + (size_t)f * off_stride, (uint32_t)totals[f]);
        dv.set_fixed(ua.ip, ua.ip_is_v6, ua.port, ua.flags, ua.asn, ua.country);
        return run_pipeline(e, S, dv.db, out, counts, match_idx, n_matches, stream, true);
    };
    rc = body();
    const hipError_t he = mark_context_used(S, stream, false);
    return rc ? rc : he != hipSuccess ? device_error("hipEventRecord", he) : PWAF_OK;
}
}  // namespace

extern "C" {

int pwaf_evaluate_records(pwaf_engine *e, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n, pwaf_verdict *out, pwaf_counts *counts) {
    if (!e || (n && (!buf || !rec_off || !out))) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    return evaluate_records_impl(e, buf, buf_bytes, rec_off, n, out, counts, nullptr);
}
int pwaf_evaluate_records_geo(pwaf_engine *e, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n, pwaf_verdict *out, pwaf_counts *counts, pwaf_geo *geo) {
    if (!e || (n && (!buf || !rec_off || !out))) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    if (int rc = need_geo_answers(e, "pwaf_evaluate_records_geo")) return rc;
    return evaluate_records_impl(e, buf, buf_bytes, rec_off, n, out, counts, geo);
}
int pwaf_evaluate_records_device(pwaf_engine *e, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n, const uint32_t *n_rec, pwaf_verdict *out,
                                 pwaf_counts *counts, uint32_t *match_idx, uint32_t *n_matches, void *stream) {
    if (!e || (n && (!buf || !rec_off || !out))) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    return evaluate_records_device_impl(e, buf, buf_bytes, rec_off, n, n_rec, out, counts, match_idx, n_matches, (hipStream_t)stream);
}

int pwaf_program_tune(pwaf_program *p, const pwaf_batch *sample) {
    if (!p || !p->p) return fail(PWAF_E_INVALID_ARG, "program is NULL");
    int rc = validate_batch_header(sample);
    if (rc) return rc;
    if (sample->memory != PWAF_MEM_HOST) return fail(PWAF_E_INVALID_ARG, "pwaf_program_tune needs a HOST-memory sample");
    if (sample->n == 0) return PWAF_OK;
    TuneOut T;
    for (const DfaGroup &g : p->p->groups) T.filters.push_back(g.filter);
    if ((rc = tune_host(*p->p, sample, T))) return rc;
    for (size_t k = 0; k < p->p->groups.size(); k++) p->p->groups[k].filter = T.filters[k];
    p->keep_tuning(T);
    return PWAF_OK;
}

int pwaf_engine_tune(pwaf_engine *e, const pwaf_batch *sample) {
    if (!e) return fail(PWAF_E_INVALID_ARG, "engine is NULL");
    int rc = validate_batch_header(sample);
    if (rc) return rc;
    if (sample->memory != PWAF_MEM_HOST) return fail(PWAF_E_INVALID_ARG, "pwaf_engine_tune needs a HOST-memory sample");
    // no evaluate call may enqueue while the tables are rebuilt (calls already enqueued are waited for below)
    std::vector<std::unique_lock<std::mutex>> ctx_locks;
    for (auto &c : e->ctx) ctx_locks.emplace_back(c->mu);
    std::lock_guard<std::mutex> lock(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    const Program &P = *e->prog.p;
    if (sample->n == 0) return PWAF_OK;
    TuneOut T;
    for (const DevGroup &d : e->groups) T.filters.push_back(d.filter);
    if ((rc = tune_host(P, sample, T))) return rc;
    bool rows_only = false;
#ifdef PWAF_PROFILING
    rows_only = getenv("PWAF_TUNE_ROWS_ONLY") != nullptr;  // timing experiment: keep the prefilters, take only the sample's state visits (which rows are LDS-resident)
#endif
    for (size_t k = 0; k < P.groups.size() && !rows_only; k++) {
        e->groups[k].filter = T.filters[k];
        if (T.chunks[k]) e->groups[k].chunks = T.chunks[k];
    }
    for (uint32_t f = 0; f < e->n_fields && f < T.mean_len.size(); f++)
        if (T.mean_len[f] > 0) e->mean_len[f] = T.mean_len[f];
    HIP_TRY(hipDeviceSynchronize());  // no launch may still be reading the tables that are about to be replaced
    for (size_t k = 0; k < P.groups.size(); k++)
        if ((rc = upload_group(e, k, &T))) return rc;
    if ((rc = assign_lists(e))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    for (size_t k = 0; k < P.groups.size(); k++) T.filters[k] = e->groups[k].filter;  // (the filters in use)
    e->prog.keep_tuning(T);  // (the list-scan hooks of pwaf_engine_program answer for the tuned tables)
    return PWAF_OK;
}

int pwaf_engine_device_status(pwaf_engine *e) {
    if (!e) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    uint32_t any = 0;
    for (auto &c : e->ctx) {
        std::lock_guard<std::mutex> lock(c->mu);
        if (!c->status.p) continue;
        uint32_t status = 0;
        HIP_TRY(hipMemcpy(&status, c->status.p, 4, hipMemcpyDeviceToHost));
        if (status) {
            HIP_TRY(hipMemset(c->status.p, 0, 4));  // sticky until reported
            uint32_t asked = 0;  // the allocator keeps counting past the cap: what the last batch on this context needed
            if (c->ctrl.p) HIP_TRY(hipMemcpy(&asked, c->ctrl.p, 4, hipMemcpyDeviceToHost));
            c->pool_entries = std::max<uint64_t>(c->pool_entries * 2, (uint64_t)asked + asked / 4 + 1024);
        }
        any |= status;
    }
    if (any) return fail(PWAF_E_NOMEM, "scan overflow pool exhausted: verdicts of a device-resident batch since the last status call are incomplete "
                                       "(evaluate it again: the pool has been grown; the synchronous entry points retry by themselves)");
    return PWAF_OK;
}

}  // extern "C"
namespace {
int evaluate_one_impl(pwaf_engine *e, const pwaf_request *r, pwaf_verdict *out, pwaf_geo *geo, uint32_t *route = nullptr) {
    if (r->n_headers && !r->headers) return fail(PWAF_E_INVALID_ARG, "n_headers without a headers array");
    const uint32_t n_hdr = e->n_fields - PWAF_N_FIELDS;  // header columns the rule set reads
    const uint32_t n_cols = PWAF_N_FIELDS + n_hdr;
    std::vector<const char *> ptr{r->host, r->url, r->path, r->method, r->user_agent};
    std::vector<uint32_t> len{r->host_len, r->url_len, r->path_len, r->method_len, r->user_agent_len};
    for (uint32_t k = 0; k < n_hdr; k++) {
        const bool have = k < r->n_headers;
        ptr.push_back(have ? r->headers[k].data : nullptr);
        len.push_back(have ? r->headers[k].len : 0u);
    }
    std::vector<std::vector<uint8_t>> arena(n_cols);
    std::vector<uint32_t> offs(2 * (size_t)n_cols);
    std::vector<pwaf_strcol> hcols(n_hdr);
    std::vector<uint32_t> hbytes(n_hdr);
    pwaf_batch b{};
    b.struct_size = sizeof b;
    b.n = 1;
    b.memory = PWAF_MEM_HOST;
    for (uint32_t f = 0; f < n_cols; f++) {
        arena[f].assign(len[f] + PWAF_ARENA_PAD, 0);
        if (len[f]) {
            if (!ptr[f]) return fail(PWAF_E_INVALID_ARG, "NULL field with non-zero length");
            memcpy(arena[f].data(), ptr[f], len[f]);
        }
        offs[2 * f] = 0;
        offs[2 * f + 1] = len[f];
        pwaf_strcol &c = f < PWAF_N_FIELDS ? b.field[f] : hcols[f - PWAF_N_FIELDS];
        c.data = arena[f].data();
        c.offsets = &offs[2 * f];
        if (f >= PWAF_N_FIELDS) hbytes[f - PWAF_N_FIELDS] = len[f];
    }
    if (n_hdr) {
        b.n_headers = n_hdr;
        b.headers = hcols.data();
        b.header_bytes = hbytes.data();
    }
    uint16_t port = r->port, country = (uint16_t)(r->country[0] | r->country[1] << 8);
    uint8_t v6 = r->ip_is_v6, flags = r->flags;
    uint32_t asn = r->asn;
    b.ip = r->ip;
    b.ip_is_v6 = &v6;
    b.port = &port;
    b.flags = &flags;
    if (r->has_geoip) {
        b.asn = &asn;
        b.country = &country;
    }
    if (!route) return evaluate_batch_impl(e, &b, out, nullptr, geo);
    ReportOut h;
    h.route = route;
    return evaluate_batch_impl(e, &b, out, nullptr, geo, &h);
}
}  // namespace

extern "C" {

int pwaf_evaluate_one(pwaf_engine *e, const pwaf_request *r, pwaf_verdict *out) {
    if (!e || !r || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    return evaluate_one_impl(e, r, out, nullptr);
}
int pwaf_evaluate_one_route(pwaf_engine *e, const pwaf_request *r, pwaf_verdict *out, uint32_t *route) {
    if (!e || !r || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    if (route)
        if (int rc = need_routes(e, "pwaf_evaluate_one_route")) return rc;
    return evaluate_one_impl(e, r, out, nullptr, route);
}
int pwaf_evaluate_one_geo(pwaf_engine *e, const pwaf_request *r, pwaf_verdict *out, pwaf_geo *geo) {
    if (!e || !r || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    if (int rc = need_geo_answers(e, "pwaf_evaluate_one_geo")) return rc;
    return evaluate_one_impl(e, r, out, geo);
}

}  // extern "C"
namespace pwaf {  // async.cpp: the queue takes its records-with-answers evaluator as a pointer (it links against a stub engine in the CPU suite)
using RecordsGeoFn = int (*)(pwaf_engine *, const uint8_t *, size_t, const uint32_t *, uint32_t, pwaf_verdict *, pwaf_counts *, pwaf_geo *);
int async_create_with(pwaf_engine *engine, uint32_t max_batch, uint32_t max_delay_us, uint32_t max_in_flight, RecordsGeoFn eval_geo, pwaf_async **out);
}  // namespace pwaf
extern "C" {

int pwaf_async_create_geo(pwaf_engine *e, uint32_t max_batch, uint32_t max_delay_us, uint32_t max_in_flight, pwaf_async **out) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (int rc = need_geo_answers(e, "pwaf_async_create_geo")) return rc;
    return pwaf::async_create_with(e, max_batch, max_delay_us, max_in_flight, &pwaf_evaluate_records_geo, out);
}

int pwaf_engine_set_profiling(pwaf_engine *e, int on) {
    if (!e) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    std::lock_guard<std::mutex> lock(e->mu);
    std::lock_guard<std::mutex> plk(e->prof_mu);
    e->profiling = on < 0 ? 0 : on > 2 ? 1 : on;
    e->times.clear();  // (re)starting a measurement window: kernel_times() reports every launch since this call
    e->time_ev.clear();
    e->n_timed = 0;
    return PWAF_OK;
}

int pwaf_engine_kernel_times(pwaf_engine *e, pwaf_kernel_time *out, int cap) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    std::lock_guard<std::mutex> lock(e->mu);
    if (e->n_timed < 2 || e->times.empty()) return 0;
    int n = 0;
    for (size_t k = 0; k < e->times.size() && k < e->time_ev.size() && n < cap; k++, n++) {
        float ms = 0;
        HIP_TRY(hipEventSynchronize(e->ev[e->time_ev[k].second]));
        HIP_TRY(hipEventElapsedTime(&ms, e->ev[e->time_ev[k].first], e->ev[e->time_ev[k].second]));
        out[n] = e->times[k];
        out[n].ms = ms;
    }
    return n;
}

// ---- host-side field derivation ---------------------------------------------------------------------
size_t pwaf_derive_path(const uint8_t *p, size_t len) {
    // get_path: uri.path().trim_end_matches('/')  (pingoo/services/http_utils.rs:114-116)
    while (len && p[len - 1] == '/') len--;
    return len;
}

static bool visible_ascii(const uint8_t *p, size_t n) {
    // HeaderValue::to_str succeeds only if every byte is '\t' or 0x20..=0x7E
    for (size_t i = 0; i < n; i++)
        if (p[i] != '\t' && (p[i] < 0x20 || p[i] > 0x7E)) return false;
    return true;
}
static void trim_span(const uint8_t *p, size_t n, bool unicode_ws, size_t *start, size_t *len) {
    auto ws = [&](uint8_t c) { return c == ' ' || c == '\t' || (unicode_ws && c >= 0x0A && c <= 0x0D); };
    size_t b = 0, e = n;
    while (b < e && ws(p[b])) b++;
    while (e > b && ws(p[e - 1])) e--;
    *start = b;
    *len = e - b;
}

void pwaf_derive_user_agent(const uint8_t *hdr, size_t len, int present, size_t *out_start, size_t *out_len) {
    // pingoo/listeners/http_listener.rs:159-165
    *out_start = 0;
    *out_len = 0;
    if (!present || !visible_ascii(hdr, len)) return;
    size_t s, l;
    trim_span(hdr, len, false, &s, &l);
    if (l > 256) return;  // heapless::String<256>::from_str fails -> unwrap_or_default() == ""
    *out_start = s;
    *out_len = l;
}

void pwaf_derive_host(const uint8_t *uri_host, size_t uri_host_len, int uri_host_present, const uint8_t *host_hdr, size_t host_hdr_len,
                      int host_hdr_present, int *out_from_header, size_t *out_start, size_t *out_len) {
    // pingoo/listeners/http_listener.rs:284-296
    *out_from_header = 0;
    *out_start = 0;
    *out_len = 0;
    size_t s, l;
    if (uri_host_present) {
        trim_span(uri_host, uri_host_len, true, &s, &l);
        if (l > 256) return;
        *out_start = s;
        *out_len = l;
        return;
    }
    if (!host_hdr_present) return;
    *out_from_header = 1;
    if (!visible_ascii(host_hdr, host_hdr_len)) return;
    trim_span(host_hdr, host_hdr_len, false, &s, &l);
    if (l > 256) return;
    *out_start = s;
    *out_len = l;
}

}  // extern "C"
