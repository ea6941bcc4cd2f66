// TEST-ONLY pieces shared by the host harnesses of the planners (tests/tableplan_host.cpp, tests/scanplan_host.cpp): the case file,
// its reader, the product's compiler over it, the section writer and the status line. Not part of the product.
//
// CASE (little-endian): "PWAFCAS1", u32 flags, n_rules, n_routes, n_lists, n_geo; strings are u32 length (0xFFFFFFFF: NULL) + bytes.
//   rule: name, expression, u32 n_actions, the action bytes; route: name, expression; list: name, u32 type, u32 n_items, the items;
//   then n_geo pwaf_geoip_entry records; then, optional, "CASEOPTS", u32 lds_table_budget, max_dfa_states, max_table_bytes (pwaf_options).
//   (A harness may read more behind them: Case::r stands there.)
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../pingoo_amd/csrc/program.h"

using namespace pwaf;

static std::string g_message;
namespace pwaf {
int fail(int code, const std::string &msg) {  // (the product's is program_api.cpp's)
    g_message = msg;
    return code;
}
}  // namespace pwaf

static std::vector<uint8_t> slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    std::vector<uint8_t> b;
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + k);
    fclose(f);
    return b;
}

struct Reader {
    const std::vector<uint8_t> &b;
    size_t pos = 0;
    void need(size_t n) const { if (pos + n > b.size()) { fprintf(stderr, "truncated case file\n"); exit(2); } }
    uint32_t u32() { need(4); uint32_t v; memcpy(&v, &b[pos], 4); pos += 4; return v; }
    bool str(std::string &out) {  // false: NULL
        const uint32_t n = u32();
        if (n == 0xFFFFFFFFu) return false;
        need(n);
        out.assign((const char *)b.data() + pos, n);
        pos += n;
        return true;
    }
};

static std::string json_line(const char *stage, int rc, uint32_t rule_index, const std::string &msg) {
    std::string s = std::string("{\"stage\": \"") + stage + "\", \"rc\": " + std::to_string(rc) + ", \"rule_index\": " + std::to_string(rule_index) + ", \"message\": \"";
    for (char c : msg) {
        if (c == '"' || c == '\\') { s += '\\'; s += c; }
        else if ((unsigned char)c < 0x20) { char u[8]; snprintf(u, sizeof u, "\\u%04x", c); s += u; }
        else s += c;
    }
    return s + "\"}";
}

template <class T>
static void section(std::vector<uint8_t> &buf, const char tag[4], const std::vector<T> &v) {
    const uint32_t count = (uint32_t)v.size();
    const uint64_t len = v.size() * sizeof(T);
    const uint8_t *p = (const uint8_t *)v.data();
    buf.insert(buf.end(), tag, tag + 4);
    buf.insert(buf.end(), (const uint8_t *)&count, (const uint8_t *)&count + 4);
    buf.insert(buf.end(), (const uint8_t *)&len, (const uint8_t *)&len + 8);
    if (len) buf.insert(buf.end(), p, p + len);
    while (buf.size() % 8) buf.push_back(0);
}


// A case file, compiled: `p` on success, else `status` holds the "compile" line. n_rules / n_routes: what the case hands to the compiler.
struct Case {
    std::vector<uint8_t> file;
    Reader r{file, 8};
    uint32_t n_rules = 0, n_routes = 0;
    std::unique_ptr<Program> p;
    std::string status;
};
static int load_case(const char *case_path, Case &c) {
    c.file = slurp(case_path);
    const std::vector<uint8_t> &file = c.file;
    Reader &r = c.r;
    if (file.size() < 28 || memcmp(file.data(), "PWAFCAS1", 8) != 0) { fprintf(stderr, "bad case magic\n"); return 2; }
    const uint32_t flags = r.u32(), n_rules = c.n_rules = r.u32(), n_routes = c.n_routes = r.u32(), n_lists = r.u32(), n_geo = r.u32();
    struct Text { std::string s; bool set = false; const char *c() const { return set ? s.c_str() : nullptr; } };
    std::vector<Text> rule_name(n_rules), rule_expr(n_rules), route_name(n_routes), route_expr(n_routes), list_name(n_lists);
    std::vector<std::vector<uint8_t>> actions(n_rules);
    std::vector<pwaf_rule_desc> rules(n_rules);
    for (uint32_t k = 0; k < n_rules; k++) {
        rule_name[k].set = r.str(rule_name[k].s);
        rule_expr[k].set = r.str(rule_expr[k].s);
        const uint32_t na = r.u32();
        r.need(na);
        actions[k].assign(file.begin() + r.pos, file.begin() + r.pos + na);
        r.pos += na;
        rules[k] = pwaf_rule_desc{rule_name[k].c(), rule_expr[k].c(), actions[k].data(), na, 0};
    }
    std::vector<pwaf_route_desc> routes(n_routes);
    for (uint32_t k = 0; k < n_routes; k++) {
        route_name[k].set = r.str(route_name[k].s);
        route_expr[k].set = r.str(route_expr[k].s);
        routes[k] = pwaf_route_desc{route_name[k].c(), route_expr[k].c(), 0};
    }
    std::vector<std::vector<std::string>> items(n_lists);
    std::vector<std::vector<const char *>> item_ptrs(n_lists);
    std::vector<pwaf_list_desc> lists(n_lists);
    for (uint32_t k = 0; k < n_lists; k++) {
        list_name[k].set = r.str(list_name[k].s);
        const uint32_t type = r.u32(), n_items = r.u32();
        items[k].resize(n_items);
        for (auto &it : items[k]) r.str(it);
        for (auto &it : items[k]) item_ptrs[k].push_back(it.c_str());
        lists[k] = pwaf_list_desc{list_name[k].c(), type, n_items, item_ptrs[k].data()};
    }
    r.need((size_t)n_geo * sizeof(pwaf_geoip_entry));
    std::vector<pwaf_geoip_entry> geo(n_geo);
    if (n_geo) memcpy(geo.data(), &file[r.pos], (size_t)n_geo * sizeof(pwaf_geoip_entry));
    r.pos += (size_t)n_geo * sizeof(pwaf_geoip_entry);
    const pwaf_geoip_table table{geo.data(), n_geo};

    pwaf_options o{};
    o.struct_size = sizeof o;
    o.flags = flags;
    o.device = -1;
    if (r.pos + 8 <= file.size() && memcmp(&file[r.pos], "CASEOPTS", 8) == 0) {  // (optional)
        r.pos += 8;
        o.lds_table_budget = r.u32();
        o.max_dfa_states = r.u32();
        o.max_table_bytes = r.u32();
    }
    const CompileInput in{rules.data(), n_rules, routes.data(), n_routes, lists.data(), n_lists, n_geo ? &table : nullptr, o};
    pwaf_compile_error ce{};
    ce.rule_index = 0xFFFFFFFFu;
    const int rc = compile_program(in, c.p, ce);
    if (rc < 0) {
        c.p.reset();
        c.status = json_line("compile", rc, ce.rule_index, ce.message);
    }
    return 0;
}

static int write_file(const char *path, const std::vector<uint8_t> &buf) {
    FILE *f = fopen(path, "wb");
    if (!f) { perror(path); return 2; }
    fwrite(buf.data(), 1, buf.size(), f);
    fclose(f);
    return 0;
}
