// program_api.cpp — the part of the C ABI (include/pwaf.h) that needs no device: the thread's last-error text, expressions and rule sets
// through the compiler (pwaf_program_*), the hooks the CPU suite reads a program through, tuning a program on a traffic sample, and the
// host-side field derivation. Plain C++, no HIP header: the `asan` build variant (build.py) instruments this unit with the compiler behind it.
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "frontend.h"
#include "program_handle.h"
#include "tableplan.h"
// kernels.h names HIP's vector types, through pointers only, in argument blocks this unit never touches; it is included for the sizes
// confirm_kernel tests (confirm_tables_fit) and the residual translators' declarations.
struct uint2;
struct uint4;
#include "kernels.h"

using namespace pwaf;

namespace {

thread_local std::string g_last_error = "";

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

bool visible_ascii(const uint8_t *p, size_t n) {
    // HeaderValue::to_str succeeds only if every byte is '\t' or 0x20..=0x7E
    for (size_t i = 0; i < n; i++)
        if (p[i] != '\t' && (p[i] < 0x20 || p[i] > 0x7E)) return false;
    return true;
}
void trim_span(const uint8_t *p, size_t n, bool unicode_ws, size_t *start, size_t *len) {
    auto ws = [&](uint8_t c) { return c == ' ' || c == '\t' || (unicode_ws && c >= 0x0A && c <= 0x0D); };
    size_t b = 0, e = n;
    while (b < e && ws(p[b])) b++;
    while (e > b && ws(p[e - 1])) e--;
    *start = b;
    *len = e - b;
}

}  // namespace

namespace pwaf {

int fail(int code, const std::string &msg) {  // (every unit of the library reports through this)
    g_last_error = msg;
    return code;
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

}  // namespace pwaf

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
uint32_t pwaf_program_header_count(const pwaf_program *p) { return p ? (uint32_t)p->p->header_names.size() : 0u; }
const char *pwaf_program_header_name(const pwaf_program *p, uint32_t i) { return (p && i < p->p->header_names.size()) ? p->p->header_names[i].c_str() : ""; }

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

int pwaf_program_verdict_shape(const pwaf_program *p, uint32_t out[8]) {
    if (!p || !p->p || !out) return fail(PWAF_E_INVALID_ARG, "pwaf_program_verdict_shape: bad argument");
    const Program &P = *p->p;
    // as pwaf_engine_create plans the tables and BatchRun::fill_verdict_args asks for the shape
    TablePlan plan;
    const size_t n_given = P.rule_status.size();  // (the caller's rules, then its routes)
    if (int rc = plan_tables(P, n_given - std::min<size_t>(n_given, P.n_routes), P.n_routes, plan)) return rc;
    const uint32_t mode = verdict_mode(P.flags), n_passes = verdict_pass_count(P);
    const VerdictShape sh = verdict_shape(P.n_cols, (uint32_t)P.rules.size(), plan.n_trig, (uint32_t)P.lits.size(), (P.flags & PWAF_OPT_GLOBAL_VERDICT_TABLES) != 0, (int)mode, n_passes);
    out[0] = mode;
    out[1] = sh.v_cap;
    out[2] = verdict_launchable(sh, P.n_cols) ? sh.waves : 0u;
    out[3] = sh.per_cu;
    out[4] = sh.lds_tables;
    out[5] = sh.lds_bytes;
    out[6] = n_passes;
    out[7] = verdict_variant(n_passes) ? 1u : (uint32_t)((kMaxPasses + 1 + 63) / 64);
    return PWAF_OK;
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

// ---- host-side field derivation ---------------------------------------------------------------------
size_t pwaf_derive_path(const uint8_t *p, size_t len) {
    // get_path: uri.path().trim_end_matches('/')  (pingoo/services/http_utils.rs:114-116)
    while (len && p[len - 1] == '/') len--;
    return len;
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
