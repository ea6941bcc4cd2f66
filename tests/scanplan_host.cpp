// TEST-ONLY host build of the scan-side planner (tests/test_scanplan_cpu.py): compiles a rule set with the product's compiler units and
// runs csrc/scanplan.cpp on the result — tune_host (when the case carries a sample), build_device_group and build_flat_group for every
// pass, plan_passes — as pwaf_engine_create / pwaf_engine_tune call them, without engine.cpp and without a device. Links no HIP. Not part
// of the product.
//
// usage: scanplan_host CASE OUT [CASE OUT ...]   one JSON line per case on stdout: {"stage": "ok" | "compile" | "plan", "rc", "rule_index", "message"}
//        scanplan_host --synthetic GROUP OUT     the two table builders over ONE hand-made DfaGroup (shapes no rule set reaches)
//        scanplan_host --passes SPEC OUT         plan_passes over a hand-made Program: passes that are nothing but their columns, their factor
//                                                columns and the shape of their filter (owners no rule set gives a gap pass)
// CASE: tests/plan_case.h, then: "SCANPLAN", u32 lds_narrow, lds_wide (the list scan's LDS bytes per workgroup shape), residual_specialized,
//   skip_identity, n_mean, f64 mean_len[n_mean], u32 has_sample; a sample is u32 n, n_cols, then per string column (the five fields, then
//   the header columns) u32 present and, if so, (n + 1) u32 offsets, u32 n_bytes, the bytes.
// GROUP: "PWAFDFA1", u32 n_states, n_classes, hot_budget, lds_bytes, has_visits, has_class_freq, n_stays; u8 classmap[256]; u8 stays[n_stays];
//   u16 trans[n_states * n_classes]; u32 emit_off[n_states + 1]; u32 n; u16 emit_list[n]; u32 end_off[n_states + 1]; u32 n; u16 end_list[n];
//   u64 visits[n_states] if has_visits; u64 class_freq[256] if has_class_freq.
// SPEC: "PWAFPAS1", u32 flags, n_cols, n_groups; per group u32 field, atom_base, n_local, filter enabled, confirm tier, ... that walks, heads,
//   n_filter_cols, the filter columns.
// OUT: the program dump (pwaf_program_dump's format; --synthetic: its magic alone) followed by more sections of the same format, `count`
//   = the pass: "S..." the streaming table, "F..." the flat table, "T..." the flat table of the R tier, "U..." what tuning found, then "L..." the pass plan ("LDSC": the list-scan descriptors, 12 words each: phase, pass, tier,
//   threads, hot bytes, n_hot, n_delta, behind_filter, merge_rec, dense_mode, share owner, need bit).
#include "plan_case.h"

#include "../pingoo_amd/csrc/scanplan.h"

static uint32_t g_count = 0;  // the `count` word of the sections being written: the pass
template <class T>
static void gsection(std::vector<uint8_t> &buf, const char tag[4], const std::vector<T> &v) {
    const size_t at = buf.size();
    section(buf, tag, v);
    memcpy(&buf[at + 4], &g_count, 4);
}

static void write_scan(std::vector<uint8_t> &buf, const ScanImage &m) {
    gsection(buf, "SSHP", std::vector<uint32_t>{m.n_states, m.stride, m.n_classes, m.n_hot, m.start_emit, m.emit_base, m.special_base, m.atom_base, m.n_local, m.field,
                                                m.scalar_mode, m.ill_class});
    gsection(buf, "STAB", m.tab);
    gsection(buf, "SCLS", m.classmap);
    gsection(buf, "SSPC", m.special);
    gsection(buf, "SLOF", m.list_off);
    gsection(buf, "SLST", m.list);
}

static void write_flat(std::vector<uint8_t> &buf, char t, const FlatImage &m, uint32_t lds_bytes) {
    const auto tag = [&](const char *rest) { static char x[5]; x[0] = t; memcpy(x + 1, rest, 4); return (const char *)x; };
    gsection(buf, tag("SHP"), std::vector<uint32_t>{m.n_states, m.n_classes, m.scalar_mode, m.ill_class, m.n_full, m.n_delta, lds_bytes});
    gsection(buf, tag("FLT"), m.flat);
    gsection(buf, tag("DLT"), m.delta);
    gsection(buf, tag("CLS"), m.classmap);
    gsection(buf, tag("EMO"), m.emit_off);
    gsection(buf, tag("EML"), m.emit_list);
    gsection(buf, tag("ENO"), m.end_off);
    gsection(buf, tag("ENL"), m.end_list);
}

static void write_passes(std::vector<uint8_t> &buf, const PassPlan &p) {
    g_count = 0;
    std::vector<int32_t> roles;
    for (const PassRole &r : p.roles)
        for (int32_t x : {r.gate, (int)r.filtered, (int)r.confirm, (int)r.confirm_walk, r.share_owner, (int)r.shared_bits, r.need_slot, r.visit_slot, (int)r.identity, (int)r.short_lit})
            roles.push_back(x);
    gsection(buf, "LROL", roles);
    gsection(buf, "LCNT", std::vector<int32_t>{(int)p.n_gap, (int)p.n_filtered, (int)p.n_gated, (int)p.n_need, (int)p.n_visit, (int)p.n_short, p.short_field});
    gsection(buf, "LOWN", p.owns_factors);
    gsection(buf, "LCOL", p.colmask);
    gsection(buf, "LSHA", p.short_atoms);
    gsection(buf, "LPTB", p.pass_table);
    gsection(buf, "LLS0", p.lscan_launches[0]);
    gsection(buf, "LLS1", p.lscan_launches[1]);
}

static int run_case(const char *case_path, const char *out_path) {
    Case c;
    if (int rc = load_case(case_path, c)) return rc;
    if (!c.p) {
        puts(c.status.c_str());
        return 0;
    }
    Program &P = *c.p;
    Reader &r = c.r;
    const uint32_t n_fields = PWAF_N_FIELDS + (uint32_t)P.header_names.size();
    uint32_t lds[2] = {48u * 1024u, 144u * 1024u};
    bool specialized = false, skip_identity = false, has_sample = false;
    std::vector<double> mean_len(n_fields, 0.0);
    if (r.pos + 8 <= c.file.size() && memcmp(&c.file[r.pos], "SCANPLAN", 8) == 0) {
        r.pos += 8;
        lds[0] = r.u32();
        lds[1] = r.u32();
        specialized = r.u32() != 0;
        skip_identity = r.u32() != 0;
        const uint32_t n_mean = r.u32();
        for (uint32_t k = 0; k < n_mean; k++) {
            r.need(8);
            double v;
            memcpy(&v, &c.file[r.pos], 8);
            r.pos += 8;
            if (k < n_fields) mean_len[k] = v;
        }
        has_sample = r.u32() != 0;
    }
    // the sample, as a host batch
    std::vector<std::vector<uint32_t>> offs;
    std::vector<std::vector<uint8_t>> data;
    std::vector<pwaf_strcol> cols;
    pwaf_batch sample{};
    TuneOut T;
    if (has_sample) {
        const uint32_t n = r.u32(), n_cols = r.u32();
        offs.resize(n_cols);
        data.resize(n_cols);
        cols.assign(n_cols, pwaf_strcol{nullptr, nullptr});
        for (uint32_t k = 0; k < n_cols; k++) {
            if (!r.u32()) continue;
            offs[k].resize((size_t)n + 1);
            for (uint32_t &o : offs[k]) o = r.u32();
            const uint32_t nb = r.u32();
            r.need(nb);
            data[k].assign(c.file.begin() + r.pos, c.file.begin() + r.pos + nb);
            data[k].push_back(0);  // (never empty: a column's data pointer says whether the sample carries it)
            r.pos += nb;
            cols[k] = pwaf_strcol{data[k].data(), offs[k].data()};
        }
        if (n_cols < PWAF_N_FIELDS) { fprintf(stderr, "a sample carries the five fields\n"); return 2; }
        sample.struct_size = sizeof sample;
        sample.memory = PWAF_MEM_HOST;
        sample.n = n;
        for (int f = 0; f < PWAF_N_FIELDS; f++) sample.field[f] = cols[(size_t)f];
        sample.headers = n_cols > PWAF_N_FIELDS ? &cols[PWAF_N_FIELDS] : nullptr;
        sample.n_headers = n_cols - PWAF_N_FIELDS;
        for (const DfaGroup &g : P.groups) T.filters.push_back(g.filter);
        g_message.clear();
        if (const int rc = tune_host(P, &sample, T)) {
            puts(json_line("plan", rc, 0xFFFFFFFFu, g_message).c_str());
            return 0;
        }
        // (as pwaf_program_tune / pwaf_engine_tune take the result)
        for (size_t k = 0; k < P.groups.size(); k++) P.groups[k].filter = T.filters[k];
        for (uint32_t f = 0; f < n_fields; f++)
            if (T.mean_len[f] > 0) mean_len[f] = T.mean_len[f];
    }
    std::vector<uint8_t> buf = dump_program(P);
    std::vector<GroupFilter> filters;
    std::vector<FlatShape> flat_shapes[2];  // full, R tier
    for (size_t k = 0; k < P.groups.size(); k++) {
        const DfaGroup &g = P.groups[k];
        filters.push_back(g.filter);
        g_count = (uint32_t)k;
        ScanImage m;
        g_message.clear();
        if (const int rc = build_device_group(g, P.lds_hot_budget, m, has_sample ? &T.visits[k] : nullptr, has_sample ? &T.class_freq[k] : nullptr)) {
            puts(json_line("plan", rc, 0xFFFFFFFFu, g_message).c_str());
            return 0;
        }
        write_scan(buf, m);
        FlatImage fm, rm;
        build_flat_images(g, g.filter, lds, has_sample ? &T : nullptr, k, fm, rm);
        write_flat(buf, 'F', fm, lds[flat_wide(g, g.filter) ? 1 : 0]);
        if (g.rtier) write_flat(buf, 'T', rm, lds[1]);
        flat_shapes[0].push_back(fm);
        flat_shapes[1].push_back(rm);
        if (has_sample) {
            gsection(buf, "UVIS", T.visits[k]);
            gsection(buf, "UCFQ", T.class_freq[k]);
            gsection(buf, "URVS", T.rvisits[k]);
            gsection(buf, "UFLT", std::vector<uint32_t>{g.filter.enabled, g.filter.stride, (uint32_t)g.filter.heads.size(), T.chunks[k]});
            gsection(buf, "UNOT", std::vector<char>(g.filter.note.begin(), g.filter.note.end()));
        }
    }
    g_count = 0;
    gsection(buf, "UMLN", mean_len);
    PassPlan plan;
    plan_passes(P, filters, mean_len, specialized, skip_identity, plan);
    write_passes(buf, plan);
    // the list-scan descriptors of a batch (for the default budgets: what the engine launches with)
    ListPlan lp;
    plan_list_scans(plan.roles, flat_shapes[0], flat_shapes[1], !(P.flags & PWAF_OPT_NO_DENSE_SWITCH), skip_identity, -1, lp);
    std::vector<uint32_t> descs;
    for (int phase = 0; phase < 2; phase++)
        for (const ListDesc &d : lp.descs[phase])
            for (uint32_t x : {d.phase, d.pass, (uint32_t)d.rtier, lp.shapes[phase].threads, list_hot_bytes(lp.shapes[phase]), d.n_hot, d.n_delta, (uint32_t)d.behind_filter,
                               (uint32_t)d.merge_rec, d.dense_mode, (uint32_t)d.share_owner, d.need_bit})
                descs.push_back(x);
    gsection(buf, "LDSC", descs);
    if (int wrc = write_file(out_path, buf)) return wrc;
    puts(json_line("ok", 0, 0xFFFFFFFFu, "").c_str());
    return 0;
}

static int run_synthetic(const char *group_path, const char *out_path) {
    const std::vector<uint8_t> file = slurp(group_path);
    if (file.size() < 8 || memcmp(file.data(), "PWAFDFA1", 8) != 0) { fprintf(stderr, "bad group magic\n"); return 2; }
    Reader r{file, 8};
    DfaGroup g;
    g.n_states = r.u32();
    g.n_classes = r.u32();
    const uint32_t hot_budget = r.u32(), lds_bytes = r.u32(), has_visits = r.u32(), has_freq = r.u32(), n_stays = r.u32();
    const auto bytes = [&](void *dst, size_t n) { r.need(n); if (n) memcpy(dst, &file[r.pos], n); r.pos += n; };
    bytes(g.classmap, 256);
    g.class_stays.resize(n_stays);
    bytes(g.class_stays.data(), n_stays);
    g.trans.resize((size_t)g.n_states * g.n_classes);
    bytes(g.trans.data(), g.trans.size() * 2);
    g.emit_off.resize((size_t)g.n_states + 1);
    bytes(g.emit_off.data(), g.emit_off.size() * 4);
    g.emit_list.resize(r.u32());
    bytes(g.emit_list.data(), g.emit_list.size() * 2);
    g.end_off.resize((size_t)g.n_states + 1);
    bytes(g.end_off.data(), g.end_off.size() * 4);
    g.end_list.resize(r.u32());
    bytes(g.end_list.data(), g.end_list.size() * 2);
    std::vector<uint64_t> visits(has_visits ? g.n_states : 0), freq(has_freq ? 256 : 0);
    bytes(visits.data(), visits.size() * 8);
    bytes(freq.data(), freq.size() * 8);
    g.n_local = 0x7FFF;
    std::vector<uint8_t> buf{'P', 'W', 'A', 'F', 'P', 'R', 'G', '1'};
    ScanImage m;
    g_message.clear();
    if (const int rc = build_device_group(g, hot_budget, m, has_visits ? &visits : nullptr, has_freq ? &freq : nullptr)) {
        puts(json_line("plan", rc, 0xFFFFFFFFu, g_message).c_str());
        return 0;
    }
    write_scan(buf, m);
    FlatImage fm;
    build_flat_group(g, lds_bytes, fm, has_visits ? &visits : nullptr);
    write_flat(buf, 'F', fm, lds_bytes);
    if (int wrc = write_file(out_path, buf)) return wrc;
    puts(json_line("ok", 0, 0xFFFFFFFFu, "").c_str());
    return 0;
}

static int run_passes(const char *spec_path, const char *out_path) {
    const std::vector<uint8_t> file = slurp(spec_path);
    if (file.size() < 8 || memcmp(file.data(), "PWAFPAS1", 8) != 0) { fprintf(stderr, "bad spec magic\n"); return 2; }
    Reader r{file, 8};
    Program P;
    P.flags = r.u32();
    P.n_cols = r.u32();
    P.groups.resize(r.u32());
    std::vector<GroupFilter> filters;
    for (DfaGroup &g : P.groups) {
        g.field = (uint8_t)r.u32();
        g.atom_base = r.u32();
        g.n_local = r.u32();
        g.filter.enabled = r.u32() != 0;
        g.filter.confirm.enabled = r.u32() != 0;
        g.filter.confirm.has_walk = r.u32() != 0;
        g.filter.heads.resize(r.u32(), FilterHead{});
        g.filter_cols.resize(r.u32());
        for (uint32_t &c : g.filter_cols) c = r.u32();
        g.emit_off.assign(1, 0);
        g.end_off.assign(1, 0);
        filters.push_back(g.filter);
    }
    std::vector<uint8_t> buf = dump_program(P);
    const std::vector<double> mean_len(PWAF_N_FIELDS, 0.0);
    gsection(buf, "UMLN", mean_len);
    PassPlan plan;
    plan_passes(P, filters, mean_len, false, false, plan);
    write_passes(buf, plan);
    if (int wrc = write_file(out_path, buf)) return wrc;
    puts(json_line("ok", 0, 0xFFFFFFFFu, "").c_str());
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "--passes")) return run_passes(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "--synthetic")) return run_synthetic(argv[2], argv[3]);
    if (argc < 3 || argc % 2 != 1) { fprintf(stderr, "usage: scanplan_host CASE OUT [CASE OUT ...] | --synthetic GROUP OUT | --passes SPEC OUT\n"); return 2; }
    for (int k = 1; k + 1 < argc; k += 2)
        if (int rc = run_case(argv[k], argv[k + 1])) return rc;
    return 0;
}
