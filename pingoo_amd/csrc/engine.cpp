// engine.cpp — an engine's lifetime and its device tables (include/pwaf.h: pwaf_engine_*). Construction mirrors where the reference
// builds its read-only rule state once (pingoo/server.rs:40-47,76) and hands it to every listener (server.rs:111-134); evaluation
// (evaluate.cpp, evaluate_records.cpp -> pipeline.cpp) replaces the inline loop at http_listener.rs:196-264.
//
// There is NO CPU evaluation path in this library: without a working HIP device every evaluate call
// returns PWAF_E_DEVICE (the host may then fail open, as the reference does on rule errors —
// pingoo/rules.rs:41-45).
#include "dirtable.h"
#include "engine_impl.h"
#include "georec.h"

using namespace pwaf;

namespace {

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

namespace pwaf {

const Switches &switches() {
    static const Switches sw = read_switches();
    return sw;
}

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

}  // namespace pwaf

extern "C" {

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
            snprintf(err->message, sizeof err->message, "%s", pwaf_last_error());
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
    if (!verdict_launchable(verdict_shape(P.n_cols, (uint32_t)P.rules.size(), plan.n_trig, (uint32_t)P.lits.size(), (P.flags & PWAF_OPT_GLOBAL_VERDICT_TABLES) != 0,
                                          (int)verdict_mode(P.flags), verdict_pass_count(P)), P.n_cols)) {
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

uint32_t pwaf_engine_route_count(const pwaf_engine *e) { return e && e->prog.p ? e->prog.p->n_routes : 0u; }
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
// TEST HOOK: what filter_kernel left in the context of the engine's latest batch (include/pwaf.h). Host code and device-to-host copies only.
int pwaf_engine_filter_flags(pwaf_engine *e, uint32_t group, uint32_t info[8], uint64_t *rows, size_t cap_rows, uint32_t *per_slab, uint32_t *pair_base, size_t cap_slabs) {
    if (!e || !info) return fail(PWAF_E_INVALID_ARG, "pwaf_engine_filter_flags: NULL argument");
    if (group >= e->groups.size() || !e->groups[group].filtered) return fail(PWAF_E_INVALID_ARG, "pwaf_engine_filter_flags: pass " + std::to_string(group) + " has no prefilter");
    HIP_TRY(hipSetDevice(e->device));
    // the context of the latest host batch (its own stream) or default-stream device batch: acquire_context keeps each kind on ONE context
    Scratch *S = nullptr;
    for (auto &c : e->ctx) {
        std::lock_guard<std::mutex> lock(c->mu);
        if (!c->used || !(c->last_own || c->last == nullptr)) continue;
        if (S) return fail(PWAF_E_INVALID_ARG, "pwaf_engine_filter_flags: host batches and default-stream device batches were mixed on this engine: which came last is not recorded");
        S = c.get();
    }
    if (!S) return fail(PWAF_E_INVALID_ARG, "pwaf_engine_filter_flags: the engine has evaluated nothing");
    std::lock_guard<std::mutex> lock(S->mu);
    HIP_TRY(hipEventSynchronize(S->done));
    uint32_t fi = 0;  // the pass's index among the filtered passes (pipeline.cpp: build_filter_args)
    for (uint32_t k = 0; k < group; k++) fi += e->groups[k].filtered ? 1u : 0u;
    for (int i = 0; i < 8; i++) info[i] = 0;
    info[2] = e->groups[group].filter.stride;
    info[3] = e->groups[group].confirm ? 1u : 0u;
    info[5] = PWAF_FILTER_SLAB_ROWS;
    static_assert(PWAF_FILTER_SLAB_ROWS == kStreamSlab / 1024, "one 64-bit word per KiB row of a slab");
    if (fi >= S->last_filter.size()) return PWAF_OK;  // (the batch never reached the prefilter: no slab)
    const FilterArgs &f = S->last_filter[fi];
    const size_t slabs = (size_t)(((uint64_t)f.total + kStreamSlab - 1) / kStreamSlab) - f.slab0;
    info[0] = f.slab0;
    info[1] = (uint32_t)slabs;
    info[2] = f.stride;
    info[3] = f.pairs ? 1u : 0u;
    if ((rows && cap_rows < slabs * PWAF_FILTER_SLAB_ROWS) || ((per_slab || pair_base) && cap_slabs < slabs))
        return fail(PWAF_E_INVALID_ARG, "pwaf_engine_filter_flags: the pass streamed " + std::to_string(slabs) + " slabs, the arrays are shorter");
    if (f.pairs) HIP_TRY(hipMemcpy(&info[4], f.pair_count, 4, hipMemcpyDeviceToHost));
    if (!slabs) return PWAF_OK;
    if (rows) HIP_TRY(hipMemcpy(rows, f.chunk_bits, slabs * PWAF_FILTER_SLAB_ROWS * 8, hipMemcpyDeviceToHost));
    if (per_slab) HIP_TRY(hipMemcpy(per_slab, f.sub_count, slabs * 4, hipMemcpyDeviceToHost));
    if (pair_base) {
        if (f.pairs) HIP_TRY(hipMemcpy(pair_base, f.pair_base, slabs * 4, hipMemcpyDeviceToHost));
        else memset(pair_base, 0, slabs * 4);
    }
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

const pwaf_program *pwaf_engine_program(const pwaf_engine *e) { return e ? &e->prog : nullptr; }
uint32_t pwaf_engine_header_count(const pwaf_engine *e) { return e ? pwaf_program_header_count(&e->prog) : 0u; }
const char *pwaf_engine_header_name(const pwaf_engine *e, uint32_t i) { return e ? pwaf_program_header_name(&e->prog, i) : ""; }
uint32_t pwaf_engine_compute_units(const pwaf_engine *e) { return e ? e->n_cus : 0u; }
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

}  // extern "C"
