// evaluate.cpp — the evaluate entry points over batches (include/pwaf.h: pwaf_evaluate_batch*, pwaf_evaluate_device*, pwaf_evaluate_one*),
// pwaf_geoip_lookup and page-locked host memory. A DEVICE batch goes straight to the pipeline (pipeline.cpp); a HOST batch is staged
// first — where its parts go is staging.h's arithmetic, the copies are here (HostBatchCall).
#include "engine_impl.h"

using namespace pwaf;

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

// A batch without requests: nothing runs; the counters and the rule hits read zero where they live.
int empty_batch(pwaf_engine *e, const pwaf_batch *in, pwaf_counts *counts, const ReportOut *rep) {
    const size_t rule_hit_bytes = (size_t)e->prog.p->n_user_rules * 8;
    if (counts && in->memory == PWAF_MEM_HOST) memset(counts, 0, sizeof *counts);
    if (!rep || !rep->hit_any()) return PWAF_OK;
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

// One HOST batch on its context (held for the whole call): stage, validate what a device cannot report (while the copies are in
// flight, when the caller's memory is page-locked: pwaf_host_alloc / pwaf_host_register), run, copy back. evaluate_batch_impl below is
// the driver.
struct HostBatchCall {
    pwaf_engine *e;
    Scratch &S;
    const pwaf_batch *in;
    pwaf_verdict *out;
    pwaf_counts *counts;    // nullable
    pwaf_geo *geo;          // nullable
    const ReportOut *rep;   // nullable: the caller's report, in host memory
    uint32_t *const route;  // (nullable; engines with routes only) every request's route, where `out` lives
    const bool want_hits;
    const size_t rule_hit_bytes;
    const uint32_t n;
    const hipStream_t s;
    ReportOut dh;  // the report's device side, staged
    // host view of every string column by field id (five fields + the header columns the batch carries; the others read as "")
    const uint32_t n_hdr_in;
    const uint32_t *offs[kMaxCols];  // the offsets of host_col(f); null: absent
    DeviceBatch dv;
    std::vector<uint32_t> col_begin;

    HostBatchCall(pwaf_engine *e_, Scratch &S_, const pwaf_batch *in_, pwaf_verdict *out_, pwaf_counts *counts_, pwaf_geo *geo_, const ReportOut *rep_)
        : e(e_), S(S_), in(in_), out(out_), counts(counts_), geo(geo_), rep(rep_), route(rep_ ? rep_->route : nullptr), want_hits(rep_ && rep_->hit_any()),
          rule_hit_bytes((size_t)e_->prog.p->n_user_rules * 8), n(in_->n), s(S_.stream),
          n_hdr_in(in_->headers ? std::min<uint32_t>(in_->n_headers, e_->n_fields - PWAF_N_FIELDS) : 0u), dv(in_->n, e_->n_fields), col_begin(e_->n_fields, 0) {
        for (uint32_t f = 0; f < e->n_fields; f++) {
            const pwaf_strcol *c = host_col(f);
            offs[f] = c ? c->offsets : nullptr;
        }
    }
    const pwaf_strcol *host_col(uint32_t f) const {
        if (f < PWAF_N_FIELDS) return &in->field[f];
        const uint32_t k = f - PWAF_N_FIELDS;
        return (k < n_hdr_in && in->headers[k].data && in->headers[k].offsets) ? &in->headers[k] : nullptr;
    }
    const ReportOut *d_rep() const { return rep ? &dh : nullptr; }
    int validate() const { return check_host_columns(n, e->n_fields, offs, in->country); }
    int bail(int code) const { (void)hipStreamSynchronize(s); return code; }  // (copies in flight read the caller's buffers)

    // a HOST batch's rule hits: produced into staging buffers of the context ({n_hits, pad, rule_hits[]}; the list), fetched once the batch is
    // done and the number of entries is known — only the entries the batch wrote travel, the rest of the caller's list is left alone
    int stage_hit_buffers() {
        int rc;
        if (!want_hits) return PWAF_OK;
        if ((rc = S.stage_hit_counts.reserve(8 + rule_hit_bytes)) || (rc = S.stage_hits.reserve(std::max<size_t>(16, (size_t)rep->cap * sizeof(pwaf_rule_hit))))) return rc;
        if (rep->n_hits) {
            dh.hits = (pwaf_rule_hit *)S.stage_hits.p;
            dh.cap = rep->cap;
            dh.n_hits = (uint32_t *)S.stage_hit_counts.p;
        }
        if (rep->rule_hits) dh.rule_hits = (uint64_t *)((char *)S.stage_hit_counts.p + 8);
        return PWAF_OK;
    }
    int fetch_hits(int code) {
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
    }

    // where the batch's parts would go in ONE packed block, and whether it is small enough for that (the columns' ends are ordered: the caller checked)
    PackedPlan plan() const {
        HostCol col[kMaxCols];
        for (uint32_t f = 0; f < e->n_fields; f++)
            if (offs[f]) col[f] = HostCol{true, offs[f][0], offs[f][n]};
        return plan_packed(n, e->n_fields, col, in->asn != nullptr, geo != nullptr, route != nullptr);
    }

    // ---- small batches: ONE packed block (staging.h: PackedPlan) ----
    int run_packed(const PackedPlan &pk) {
        int rc;
        if ((rc = validate())) return rc;
        if ((rc = S.pin_in.reserve(pk.in_bytes)) || (rc = S.pin_out.reserve(pk.need - pk.at_counts)) || (rc = S.packed.reserve(pk.need))) return rc;
        uint8_t *const h = (uint8_t *)S.pin_in.p;
        const uint8_t *const d = (const uint8_t *)S.packed.p;
        for (uint32_t f = 0; f < e->n_fields; f++) {
            const pwaf_strcol *c = host_col(f);
            if (!c) continue;
            const uint32_t hi = c->offsets[n];
            memcpy(h + pk.at_off[f], c->offsets, (size_t)(n + 1) * 4);
            if (hi) memcpy(h + pk.at_data[f], c->data, hi);
            memset(h + pk.at_data[f] + hi, 0, PWAF_ARENA_PAD);
            dv.set_col(f, d + pk.at_data[f], d + pk.at_off[f], hi);
        }
        memcpy(h + pk.at_ip, in->ip, (size_t)n * 16);
        memcpy(h + pk.at_v6, in->ip_is_v6, n);
        memcpy(h + pk.at_port, in->port, (size_t)n * 2);
        memcpy(h + pk.at_flags, in->flags, n);
        if (in->asn) {
            memcpy(h + pk.at_asn, in->asn, (size_t)n * 4);
            memcpy(h + pk.at_cc, in->country, (size_t)n * 2);
        }
        dv.set_fixed(d + pk.at_ip, d + pk.at_v6, d + pk.at_port, d + pk.at_flags, in->asn ? d + pk.at_asn : nullptr, in->asn ? d + pk.at_cc : nullptr);
        memset(h + pk.at_counts, 0, sizeof(pwaf_counts));
        HIP_TRY(hipMemcpyAsync(S.packed.p, h, pk.in_bytes, hipMemcpyHostToDevice, s));
        pwaf_verdict *const d_out = (pwaf_verdict *)((char *)S.packed.p + pk.at_out);
        pwaf_counts *const d_counts = (pwaf_counts *)((char *)S.packed.p + pk.at_counts);
        const size_t back = pk.need - pk.at_counts;
        if (route) dh.route = (uint32_t *)((char *)S.packed.p + pk.at_route);
        rc = run_with_retry(e, S, dv.db, d_out, d_counts, true, &col_begin, true, [&]() -> int {
            HIP_TRY(hipMemcpyAsync(S.pin_out.p, d_counts, back, hipMemcpyDeviceToHost, s));
            return PWAF_OK;
        }, geo ? (pwaf_geo *)((char *)S.packed.p + pk.at_geo) : nullptr, d_rep());
        if ((rc = fetch_hits(rc))) return rc;
        if (geo) memcpy(geo, (const char *)S.pin_out.p + (pk.at_geo - pk.at_counts), (size_t)n * sizeof(pwaf_geo));
        if (route) memcpy(route, (const char *)S.pin_out.p + (pk.at_route - pk.at_counts), (size_t)n * 4);
        memcpy(out, (const char *)S.pin_out.p + (pk.at_out - pk.at_counts), (size_t)n * sizeof(pwaf_verdict));
        if (counts) memcpy(counts, S.pin_out.p, sizeof(pwaf_counts));
        return PWAF_OK;
    }

    // ---- large batches: column by column, straight from the caller's buffers (page-locked ones are read by the copy engine while this
    //      thread goes on: pwaf_host_alloc / pwaf_host_register) ----
    int stage(DevBuf &b, const void *src, size_t bytes) {
        int r = b.reserve(bytes);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s));
        return PWAF_OK;
    }
    int run_by_column() {
        int rc;
        if (S.stage_field_data.size() < e->n_fields) { S.stage_field_data.resize(e->n_fields); S.stage_field_off.resize(e->n_fields); }
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
        }, geo ? (pwaf_geo *)S.stage_geo.p : nullptr, d_rep()));
    }
};

// `geo` (nullable; PWAF_OPT_GEO_ANSWERS engines only): the GeoIP record of every request, where `out` lives
// `rep` (nullable): the call's report — rule hits (PWAF_OPT_RULE_HITS engines; overwritten) or routes (engines with routes) — where `out` lives
int evaluate_batch_impl(pwaf_engine *e, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, pwaf_geo *geo, const ReportOut *rep = nullptr) {
    int rc = validate_batch_header(in);
    if (rc) return rc;
    if (rep && !rep->any()) rep = nullptr;
    if (in->n == 0) return empty_batch(e, in, counts, rep);
    HIP_TRY(hipSetDevice(e->device));
    // the context is held for the whole call (its staging buffers and its stream are reused); other threads take other contexts
    std::unique_lock<std::mutex> lock;
    bool must_wait;
    Scratch &S = acquire_context(e, true, nullptr, lock, must_wait);
    if ((rc = S.ensure(true))) return rc;
    if (must_wait) HIP_TRY(hipStreamWaitEvent(S.stream, S.done, 0));
    if (in->memory == PWAF_MEM_DEVICE) return run_with_retry(e, S, *in, out, counts, false, nullptr, false, [] { return PWAF_OK; }, geo, rep);
    HostBatchCall call(e, S, in, out, counts, geo, rep);
    if ((rc = call.stage_hit_buffers())) return rc;
    // the ends must be ordered before any size is computed from them (the full check follows, on either path)
    if ((rc = check_column_ends(call.n, e->n_fields, call.offs))) return rc;
    const PackedPlan pk = call.plan();
    if (pk.packable && !switches().no_packed_staging) return call.run_packed(pk);
    return call.run_by_column();
}

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

}  // extern "C"
