// TEST-ONLY host build of the table planner (tests/test_tableplan_cpu.py): compiles a rule set with the product's compiler units and
// runs csrc/tableplan.cpp's plan_tables on the result — the call pwaf_engine_create makes between plan_passes (csrc/scanplan.cpp) and upload_tables — without
// engine.cpp and without a device. Not part of the product.
//
// usage: tableplan_host CASE OUT [CASE OUT ...]   one JSON line per case on stdout: {"stage": "ok" | "compile" | "plan", "rc", "rule_index", "message"}
//        tableplan_host --synthetic KIND N        plan_tables over a hand-made Program with N items of one kind (the planner's own limits:
//                                                 the compiler lowers a rule that would exceed one to a residual program, so no rule set reaches them)
// CASE: tests/plan_case.h.
// OUT: the program dump (pwaf_program_dump's format) followed by the plan as more sections of the same format, tags "P...".
#include "plan_case.h"

#include "../pingoo_amd/csrc/tableplan.h"

static void write_plan(std::vector<uint8_t> &buf, const TablePlan &t) {
    section(buf, "PSHP", std::vector<uint32_t>{t.iu_n[0], t.iu_n[1], t.iu_words[0], t.iu_words[1], t.n_bit_atoms, t.n_cmp_atoms, t.cmp_vars, t.n_lazy, t.n_trig, t.cc_words,
                                               t.acmp_words, t.class_words, t.n_classes, t.geo_default});
    section(buf, "PLZV", t.lazy_vars);
    section(buf, "PHLN", t.hlen_fields);
    section(buf, "PIV0", t.iu_vals[0]);
    section(buf, "PIV1", t.iu_vals[1]);
    section(buf, "PIM0", t.iu_masks[0]);
    section(buf, "PIM1", t.iu_masks[1]);
    section(buf, "PBIT", t.bit_col);
    section(buf, "PCMP", t.cmp_atoms);
    section(buf, "PLZY", t.lazy_atoms);
    section(buf, "PLIT", t.lits);
    section(buf, "PTOF", t.trig_off);
    section(buf, "PTRL", t.trig_rules);
    section(buf, "PALW", t.always);
    section(buf, "PCCM", t.cc_masks);
    std::vector<uint32_t> acmp;
    for (auto &a : t.acmp) { acmp.push_back(a.first); acmp.push_back(a.second); }
    section(buf, "PACM", acmp);
    section(buf, "PCLS", t.class_rows);
    section(buf, "PGR4", t.geo_root4);
    section(buf, "PGR6", t.geo_root6);
    section(buf, "PGND", t.geo_nodes);
    section(buf, "PUNR", t.rules_unrouted);
}

static int run_case(const char *case_path, const char *out_path) {
    Case c;
    if (int rc = load_case(case_path, c)) return rc;
    if (!c.p) {
        puts(c.status.c_str());
        return 0;
    }
    const std::unique_ptr<Program> &p = c.p;
    const uint32_t n_rules = c.n_rules, n_routes = c.n_routes;
    std::vector<uint8_t> buf = dump_program(*p);
    TablePlan plan;
    g_message.clear();
    const int rc = plan_tables(*p, n_rules, n_routes, plan);
    if (rc) {
        puts(json_line("plan", rc, 0xFFFFFFFFu, g_message).c_str());
        return 0;
    }
    write_plan(buf, plan);
    if (int wrc = write_file(out_path, buf)) return wrc;
    puts(json_line("ok", rc, 0xFFFFFFFFu, "").c_str());
    return 0;
}

// A Program no rule set compiles to: N items of one kind, nothing else. Columns 1 .. N, one rule-less literal table.
static int run_synthetic(const std::string &kind, uint32_t n) {
    Program P;
    P.atoms.resize(1);
    P.geo_recs.push_back({0, (uint16_t)('X' | 'X' << 8), 0});
    P.n_cols = 1;
    size_t n_rules = 0, n_routes = 0;
    auto num = [&](uint8_t k, uint8_t var, uint8_t op, uint32_t ref, uint32_t ref2, int64_t c) { P.num_atoms.push_back(NumAtomDev{P.n_cols++, k, var, op, 0, ref, ref2, c}); };
    if (kind == "intset0" || kind == "intset1") {
        for (uint32_t k = 0; k < n; k++) { P.int_pool.push_back(k); num(ATOM_INTSET, kind == "intset1", 0, k, k + 1, 0); }
    } else if (kind == "hlen") {
        for (uint32_t k = 0; k < n; k++) num(ATOM_LEN, (uint8_t)(PWAF_N_FIELDS + k), OP_LE, 0, 0, 7);
    } else if (kind == "asncmp") {
        for (uint32_t k = 0; k < n; k++) num(ATOM_INT, VAR_ASN, OP_EQ, 0, 0, k);
    } else if (kind == "cmp") {
        for (uint32_t k = 0; k < n; k++) num(ATOM_INT, VAR_PORT, OP_EQ, 0, 0, k);
    } else if (kind == "unknown_var") {
        num(ATOM_INT, (uint8_t)n, OP_EQ, 0, 0, 1);
    } else if (kind == "country") {
        P.country_luts.resize(n);
    } else if (kind == "set_words") {
        P.set_words = n;
    } else if (kind == "cols") {
        P.n_cols = n;
    } else if (kind == "rules") {
        P.rules.resize(n, DevRule{0, 0, 0, PWAF_ACTION_BLOCK, PWAF_ACTION_BLOCK, {0, 0}});
    } else if (kind == "caller_rules") {
        n_rules = n;
    } else if (kind == "caller_routes") {
        n_rules = n - 1;
        n_routes = 1;
    } else {
        fprintf(stderr, "unknown kind %s\n", kind.c_str());
        return 2;
    }
    TablePlan plan;
    g_message.clear();
    const int rc = plan_tables(P, n_rules, n_routes, plan);
    puts(json_line(rc ? "plan" : "ok", rc, 0xFFFFFFFFu, rc ? g_message : "").c_str());
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "--synthetic")) return run_synthetic(argv[2], (uint32_t)strtoul(argv[3], nullptr, 0));
    if (argc < 3 || argc % 2 != 1) { fprintf(stderr, "usage: tableplan_host CASE OUT [CASE OUT ...] | --synthetic KIND N\n"); return 2; }
    for (int k = 1; k + 1 < argc; k += 2)
        if (int rc = run_case(argv[k], argv[k + 1])) return rc;
    return 0;
}
