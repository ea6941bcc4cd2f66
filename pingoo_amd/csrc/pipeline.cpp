// pipeline.cpp — one batch of device columns through the launch sequence: run_pipeline at the end of this file is the
// driver, BatchRun holds the steps. Also the ring of scratch contexts the entry points take theirs from (acquire_context) and the kernel
// timer. What calls this: evaluate.cpp and evaluate_records.cpp, after staging; run_with_retry (engine_impl.h) for the synchronous ones.
#include <type_traits>

#include "engine_impl.h"
#include "georec.h"
#include "lscan_split.h"

using namespace pwaf;

namespace {

// Slabs a filter pass streams: its arena cut into kStreamSlab pieces, less the whole slabs in front of the batch's own bytes.
uint32_t slab_count(uint32_t total, uint32_t slab0) { return (uint32_t)(((uint64_t)total + kStreamSlab - 1) / kStreamSlab) - slab0; }
uint32_t slabs_of(const FilterArgs &f) { return slab_count(f.total, f.slab0); }
// (request, flagged chunk) pairs of a pass with a confirm tier: at most one per chunk of the arena plus one per request (a chunk that
// straddles two requests counts for both)
uint32_t pair_cap_of(uint32_t slabs, uint32_t n) { return (uint32_t)std::min<uint64_t>(0xFFFFFFF0u, (uint64_t)slabs * (kStreamSlab / 16) + n + 64); }

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
        n_passes = verdict_pass_count(P);  // (+ the pseudo passes of the field-against-field atoms and of the residual rules)
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

}  // namespace

namespace pwaf {

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

hipError_t mark_context_used(Scratch &S, hipStream_t s, bool own) {
    S.used = true;
    S.last = s;
    S.last_own = own;
    return hipEventRecord(S.done, s);
}

int device_error(const char *call, hipError_t he) { return fail(PWAF_E_DEVICE, std::string(call) + ": " + hipGetErrorString(he)); }

int KernelTimer::record(hipStream_t on) {
    if (e->ev.size() < ev_i + 1) {
        hipEvent_t x;
        HIP_TRY(hipEventCreate(&x));
        e->ev.push_back(x);
    }
    HIP_TRY(hipEventRecord(e->ev[ev_i], on));
    ev_i++;
    return PWAF_OK;
}
int KernelTimer::begin(hipStream_t side) {
    if (off()) return PWAF_OK;
    if (!side && last_main >= 0) { open_begin = last_main; return PWAF_OK; }
    const int rc = record(side ? side : stream);
    if (rc) return rc;
    open_begin = (long)ev_i - 1;
    if (!side) last_main = open_begin;
    return PWAF_OK;
}
int KernelTimer::end(const char *name, uint64_t alg_bytes, hipStream_t side) {
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

// Nothing between upload_descriptors and the end returns past BatchRun's destructor: the descriptor slot's event is recorded whichever
// way the batch leaves (ArgSlotMark).
int run_pipeline(pwaf_engine *e, Scratch &S, const pwaf_batch &db /* device pointers */, pwaf_verdict *d_out, pwaf_counts *d_counts, uint32_t *d_match_idx,
                 uint32_t *d_n_matches, hipStream_t stream, bool totals_known, const std::vector<uint32_t> *col_begin, bool sync_status, pwaf_geo *d_geo, const ReportOut *d_rep) {
    S.last_filter.clear();  // (pwaf_engine_filter_flags answers for this batch from here on: nothing until its descriptors are swapped in below)
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
    S.last_filter.swap(b.fall);  // (kept for pwaf_engine_filter_flags, a test hook: no copy, the batch's vector changes hands)
    return PWAF_OK;
}

}  // namespace pwaf
