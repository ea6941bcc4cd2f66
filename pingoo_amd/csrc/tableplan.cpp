// tableplan.cpp — the host-side planning of the attribute / verdict tables (tableplan.h): a sequence of small steps over plain data,
// run by plan_tables in the order the refusals have always had. Nothing here touches a device.
#include "tableplan.h"

#include <algorithm>
#include <map>
#include <string>

namespace pwaf {

int fail(int code, const std::string &msg);  // program_api.cpp: records pwaf_last_error()

namespace {

// A comparison in the canonical form the kernels evaluate: variable (cmp_code's) against a 32-bit constant with == (op 0) or <= (op 1)
struct Canon { uint32_t vi, op, col, c; };

// integer-set atoms: merge all sets tested against one variable into a sorted union with membership rows, so the
// device does one binary search per request and variable instead of one per predicate.
// `atoms`: an INTSET atom's ref becomes its bit index in the variable's membership row.
int merge_int_sets(const Program &P, std::vector<NumAtomDev> &atoms, TablePlan &out) {
    for (int var = 0; var < 2; var++) {
        std::map<int64_t, std::vector<uint32_t>> member;
        uint32_t n_sets = 0;
        for (auto &d : atoms) {
            if (d.kind != ATOM_INTSET || d.var != var) continue;
            for (uint32_t k = d.ref; k < d.ref2; k++) member[P.int_pool[k]].push_back(n_sets);
            d.ref = n_sets++;
        }
        if (n_sets > 32 * kIntWordsMax) return fail(PWAF_E_UNSUPPORTED, "more than 128 integer-set predicates on one client variable");
        const uint32_t words = out.iu_words[var] = std::max(1u, (n_sets + 31) / 32);
        out.iu_n[var] = (uint32_t)member.size();
        out.iu_vals[var].clear();
        out.iu_masks[var].assign(words, 0);  // row 0: the value is in no set
        for (auto &kv : member) {
            out.iu_vals[var].push_back(kv.first);
            std::vector<uint32_t> row(words, 0);
            for (uint32_t b : kv.second) row[b >> 5] |= 1u << (b & 31);
            out.iu_masks[var].insert(out.iu_masks[var].end(), row.begin(), row.end());
        }
    }
    return PWAF_OK;
}

// split: membership atoms become register bit tests — column | bit << 20 | source word << 25 —, the rest are comparisons
void split_atoms(const std::vector<NumAtomDev> &atoms, std::vector<uint32_t> &bit_atoms, std::vector<NumAtomDev> &cmp_src) {
    for (const NumAtomDev &d : atoms) {
        uint32_t src;
        if (d.kind == ATOM_IPSET) src = d.ref >> 5;
        else if (d.kind == ATOM_COUNTRY) src = kSrcCc + (d.ref >> 5);
        else if (d.kind == ATOM_INTSET) src = (d.var == 0 ? kSrcPort : kSrcAsn) + (d.ref >> 5);
        else {
            cmp_src.push_back(d);
            continue;
        }
        bit_atoms.push_back(d.col | ((d.ref & 31u) << 20) | (src << 25));
    }
}

// Comparison atoms in the canonical form the kernel evaluates: variable (0-4 field lengths, 5 remote_port, 6 asn) against
// a 32-bit constant with == or <=. Lengths, ports and ASNs are unsigned 32-bit, so constants outside [0, 2^32) fold to
// "never" (the atom is dropped: its column stays zero) or "always" (<= 0xFFFFFFFF); `v < c` becomes `v <= c - 1`.
// Sorted by (variable, operator); hlen_fields grows by every header column met.
int canonical_comparisons(const std::vector<NumAtomDev> &cmp_src, std::vector<uint32_t> &hlen_fields, std::vector<Canon> &canon) {
    for (const NumAtomDev &d : cmp_src) {
        uint32_t vi;
        if (d.kind == ATOM_LEN && d.var >= PWAF_N_FIELDS) {
            // length of a header column: comparison variable 7 + k for the k-th such column
            size_t slot = std::find(hlen_fields.begin(), hlen_fields.end(), (uint32_t)d.var) - hlen_fields.begin();
            if (slot == hlen_fields.size()) hlen_fields.push_back(d.var);
            if (slot >= kMaxHeaderLens) return fail(PWAF_E_UNSUPPORTED, "length() of more than 8 distinct headers is compared");
            vi = kCmpVarHeader + (uint32_t)slot;
        } else {
            vi = d.kind == ATOM_LEN ? d.var : 5u + d.var;
            if (vi > kCmpVarAsn) return fail(PWAF_E_UNSUPPORTED, "comparison atom on an unknown variable");
        }
        int64_t c = d.c;
        uint32_t op;  // 0: ==, 1: <=
        if (d.op == OP_EQ) {
            if (c < 0 || c > 0xFFFFFFFFll) continue;
            op = 0;
        } else {
            if (d.op == OP_LT) {
                if (c <= 0) continue;  // v < c with c <= 0: never
                c -= 1;
            }
            if (c < 0) continue;
            if (c > 0xFFFFFFFFll) c = 0xFFFFFFFFll;
            op = 1;
        }
        canon.push_back({vi, op, d.col, (uint32_t)c});
    }
    std::stable_sort(canon.begin(), canon.end(), [](const Canon &x, const Canon &y) { return x.vi != y.vi ? x.vi < y.vi : x.op < y.op; });
    if (canon.size() > 65535) return fail(PWAF_E_UNSUPPORTED, "more than 65535 comparison predicates");
    return PWAF_OK;
}

// lazy atoms and flipped polarity belong to the entry-list verdict kernel, and PWAF_OPT_EAGER_CMP switches both off
bool lazy_cmp_enabled(const Program &P) { return verdict_mode(P.flags) >= 3u && !(P.flags & PWAF_OPT_EAGER_CMP); }

// POLARITY (round 6). `user_agent.length() >= 256` reaches here as NOT(length <= 255), `path.length() > 20` as NOT(length <= 20): atoms that
// hold for nearly every request and only ever appear negated — a (column, mask) pair per group for nothing, and gate A's term
// [NOT(length <= 255)] has no positive literal at all: the gate was a candidate rule in EVERY group. An atom whose literals are mostly
// negations is evaluated COMPLEMENTED on the device (kCmpComplement of its code: `v > c`, `v != c`) and every literal of it toggles its
// negation in the device copy of the literals: same truth table, rare columns, and gate A becomes a triggered rule. (client.asn
// comparisons keep their polarity: an engine-resolved record answers them through class-row bits: record_classes.)
// -> per column: the atom is flipped
std::vector<uint8_t> choose_polarity(const Program &P, const std::vector<Canon> &canon) {
    std::vector<uint8_t> flipped(P.n_cols, 0);
    if (!lazy_cmp_enabled(P)) return flipped;
    std::vector<uint32_t> n_pos(P.n_cols, 0), n_neg(P.n_cols, 0);
    for (const uint32_t lit : P.lits) ((lit & LIT_NEG) ? n_neg : n_pos)[lit & LIT_ATOM_MASK]++;
    for (const Canon &cn : canon)
        if (cn.vi != kCmpVarAsn && n_neg[cn.col] > n_pos[cn.col]) flipped[cn.col] = 1;
    return flipped;
}

// the literals with every flipped atom's negation toggled
std::vector<uint32_t> flip_literals(const std::vector<uint32_t> &lits, const std::vector<uint8_t> &flipped) {
    std::vector<uint32_t> L = lits;
    for (uint32_t &lit : L)
        if (flipped[lit & LIT_ATOM_MASK]) lit ^= LIT_NEG;
    return L;
}

// The device form of the canonical comparisons (all eager so far: select_lazy moves some out), and the client.asn ones a second time:
// client.asn against a constant is a function of the GeoIP record — bit j of the class row's comparison words (source words
// kSrcAcmp ..) when the engine resolves the record itself; out.acmp[j] says which comparison, out.bit_col which column the bit sets.
int encode_comparisons(const std::vector<Canon> &canon, const std::vector<uint8_t> &flipped, TablePlan &out) {
    for (const Canon &cn : canon) {
        out.cmp_atoms.push_back({cn.col | (cmp_code(cn.vi, cn.op, flipped[cn.col] != 0) << 24), cn.c});
        if (cn.vi != kCmpVarAsn) continue;
        const uint32_t j = (uint32_t)out.acmp.size();
        if (j >= 32 * kAcmpWordsMax) return fail(PWAF_E_UNSUPPORTED, "more than 128 distinct client.asn comparisons");
        out.bit_col[(kSrcAcmp + j / 32) * 32 + (j & 31)] = cn.col;
        out.acmp.push_back({cn.op, cn.c});
    }
    out.acmp_words = ((uint32_t)out.acmp.size() + 31) / 32;
    return PWAF_OK;
}

// How likely a column is to be set, for choosing triggers. lower = rarer: scan atoms by how specific their pattern is (shortest
// possible match), then memberships, then comparisons (often true for most requests), then the constant TRUE column
std::vector<uint32_t> rarity_ranks(const Program &P, const std::vector<NumAtomDev> &cmp_src, const std::vector<uint32_t> &bit_atoms) {
    std::vector<uint32_t> rank(P.n_cols, 100);
    for (auto &at : P.atoms)
        if (at.kind == ATOM_SCAN && at.id < P.n_cols) rank[at.id] = 64 - std::min<uint32_t>(at.min_len, 64);
    rank[0] = 300;
    for (auto &d : cmp_src) rank[d.col] = 200;
    for (uint32_t d : bit_atoms) rank[d & 0xFFFFFu] = 60;
    return rank;
}

// What select_lazy needs to know about the triggers besides the lists themselves
struct TriggerUse {
    std::vector<uint8_t> is_trigger;           // per column: some rule is filed under it
    std::vector<uint8_t> in_untriggered_term;  // per column: it stands in a term made of negations only (its rule is a candidate in EVERY group)
};

// Trigger lists: a rule can match only if one of its DNF terms is true; a term with a positive literal needs that
// column to be non-zero. Per term pick the positive literal least likely to be set (scan < membership < comparison <
// TRUE) and file the rule under that column; terms made of negations only make the rule an unconditional candidate.
// L: the literals after flip_literals.
TriggerUse trigger_lists(const Program &P, const std::vector<uint32_t> &L, const std::vector<uint32_t> &rank, TablePlan &out) {
    std::vector<std::vector<uint16_t>> by_col(P.n_cols);
    TriggerUse use{std::vector<uint8_t>(P.n_cols, 0), std::vector<uint8_t>(P.n_cols, 0)};
    out.always.assign((P.rules.size() + 31) / 32 + 1, 0);
    for (size_t r = 0; r < P.rules.size(); r++) {
        const DevRule &dr = P.rules[r];
        int best = -1;
        bool term_open = false;
        uint32_t term_first = dr.lit_off;
        for (uint32_t k = dr.lit_off; k < dr.lit_off + dr.lit_cnt; k++) {
            const uint32_t lit = L[k];
            if (!term_open) { best = -1; term_open = true; term_first = k; }
            if (!(lit & LIT_NEG)) {
                const int c = (int)(lit & LIT_ATOM_MASK);
                if (best < 0 || rank[c] < rank[best]) best = c;
            }
            if (lit & LIT_TERM_END) {
                if (best < 0) {
                    out.always[r >> 5] |= 1u << (r & 31);
                    for (uint32_t q = term_first; q <= k; q++) use.in_untriggered_term[L[q] & LIT_ATOM_MASK] = 1;
                } else if (by_col[best].empty() || by_col[best].back() != (uint16_t)r) by_col[best].push_back((uint16_t)r);
                term_open = false;
            }
        }
    }
    out.trig_off.assign(1, 0);
    for (uint32_t c = 0; c < P.n_cols; c++) {
        out.trig_rules.insert(out.trig_rules.end(), by_col[c].begin(), by_col[c].end());
        out.trig_off.push_back((uint32_t)out.trig_rules.size());
        use.is_trigger[c] = !by_col[c].empty();
    }
    out.n_trig = (uint32_t)out.trig_rules.size();
    return use;
}

// LAZY comparison atoms (round 6; program.h: LIT_LAZY). `path.length() > 20`, `remote_port >= 1024` hold for somebody in nearly every
// group of 64 requests, yet almost all of them only ever stand beside a rarer literal (`lit && path.length() > K`): the attribute kernel
// spent a third of its time evaluating them for every group, and the verdict kernel filed a pair for each. An atom that is NO rule's
// trigger (and stands in no term of negations only) is only needed once such a rule is a candidate whose other literals hold for somebody: the verdict kernel then compares the
// 64 requests' values itself. (client.asn comparisons stay eager: engine-resolved records answer them through class-row bits.)
// Moves the chosen atoms from out.cmp_atoms to out.lazy_atoms. -> per column: the low bits of its LIT_LAZY literal word, or kNotLazy
static constexpr uint32_t kNotLazy = 0xFFFFFFFFu;
std::vector<uint32_t> select_lazy(const Program &P, const TriggerUse &use, TablePlan &out) {
    std::vector<uint32_t> lazy_of(P.n_cols, kNotLazy);
    if (!lazy_cmp_enabled(P)) return lazy_of;
    // (up to two variables: the verdict kernel keeps a group's raw values of the lazy variables in two registers)
    std::vector<CmpAtomDev> eager;
    for (const CmpAtomDev &ca : out.cmp_atoms) {
        const uint32_t col = ca.col & 0xFFFFFFu, code = ca.col >> 24, vi = cmp_code_var(code), op = code & 1u;
        const bool complement = (code & kCmpComplement) != 0;
        // (an atom of a term without a trigger — `user_agent.length() >= 256` is NOT(length <= 255): gate A — would be evaluated lazily in every group)
        bool lazy = vi != kCmpVarAsn && !use.is_trigger[col] && !use.in_untriggered_term[col] && ca.c <= LIT_LAZY_CONST_MASK;  // (the constant travels inside the literal word)
        uint32_t slot = 0;
        if (lazy) {
            slot = (uint32_t)(std::find(out.lazy_vars.begin(), out.lazy_vars.end(), vi) - out.lazy_vars.begin());
            if (slot == out.lazy_vars.size()) {
                if (slot < 2) out.lazy_vars.push_back(vi);
                else lazy = false;
            }
        }
        if (lazy) {
            lazy_of[col] = ca.c | (op ? LIT_LAZY_OP : 0u) | (slot ? LIT_LAZY_SLOT : 0u) | (complement ? LIT_LAZY_COMPLEMENT : 0u);
            out.lazy_atoms.push_back({cmp_code(slot, op, complement) << 24, ca.c});  // (kept for pwaf_engine_stats-style introspection: the kernel reads the literal word)
        } else {
            eager.push_back(ca);
        }
    }
    out.cmp_atoms.swap(eager);
    return lazy_of;
}

// the literals as the device reads them: a lazy atom's carry LIT_LAZY and the atom itself in place of a column
std::vector<uint32_t> device_literals(std::vector<uint32_t> L, const std::vector<uint32_t> &lazy_of) {
    for (uint32_t &lit : L) {
        const uint32_t j = lazy_of[lit & LIT_ATOM_MASK];
        if (j != kNotLazy) lit = (lit & (LIT_NEG | LIT_TERM_END)) | LIT_LAZY | j;
    }
    return L;
}

// transpose the per-predicate 676-bit country tables into per-country membership words (one gather per request)
void transpose_countries(const Program &P, TablePlan &out) {
    const uint32_t n_luts = (uint32_t)P.country_luts.size();
    out.cc_words = std::max(1u, (n_luts + 31) / 32);
    out.cc_masks.assign((size_t)676 * out.cc_words, 0);
    for (uint32_t t = 0; t < n_luts; t++)
        for (uint32_t c = 0; c < 676; c++)
            if (P.country_luts[t][c]) out.cc_masks[(size_t)c * out.cc_words + (t >> 5)] |= 1u << (t & 31);
}

// The HITS variant of the verdict kernel reports every candidate's match word under its public index; a route's is its ROUTE index.
// A hit call therefore runs over a copy of the rule table in which the routes have no literal: their word is 0, nothing is reported.
std::vector<DevRule> unrouted_rules(const Program &P) {
    if (!(P.n_dev_routes && (P.flags & PWAF_OPT_RULE_HITS))) return {};
    std::vector<DevRule> unrouted = P.rules;
    for (size_t k = P.route_base; k < unrouted.size(); k++) unrouted[k].lit_cnt = 0;
    return unrouted;
}

// everything of one GeoIP record the rules ask about: country-table bits | asn-set bits | asn comparisons
std::vector<uint32_t> record_row(const GeoRec &rec, const TablePlan &out) {
    std::vector<uint32_t> row(out.class_words, 0);
    const uint32_t c0 = (rec.country & 0xFFu) - 'A', c1 = (rec.country >> 8) - 'A';
    const uint32_t cidx = (c0 < 26u && c1 < 26u) ? c0 * 26u + c1 : 23u * 26u + 23u;
    for (uint32_t w = 0; w < out.cc_words; w++) row[w] = out.cc_masks[(size_t)cidx * out.cc_words + w];
    const uint32_t asn = rec.asn, iw = out.iu_words[1];
    auto it = std::lower_bound(out.iu_vals[1].begin(), out.iu_vals[1].end(), (int64_t)asn);
    const size_t mrow = (it != out.iu_vals[1].end() && *it == (int64_t)asn) ? (size_t)(it - out.iu_vals[1].begin()) + 1 : 0;
    for (uint32_t w = 0; w < iw; w++) row[out.cc_words + w] = out.iu_masks[1][mrow * iw + w];
    for (size_t j = 0; j < out.acmp.size(); j++)
        if (out.acmp[j].first == 0 ? asn == out.acmp[j].second : asn <= out.acmp[j].second) row[out.cc_words + iw + j / 32] |= 1u << (j & 31);
    return row;
}

// GeoIP classes: everything that depends on the record — country-table bits, asn-set bits, asn comparisons — as one row per
// record; records with equal rows share a CLASS (a few hundred for a real rule set), class 0 is the all-zero row. The
// device trie's leaves carry class ids, so a request gathers one small cache-resident row instead of a per-record one.
// (geo_default: a GeoIP family without prefixes makes every address read the DEFAULT record's class — not class 0:
// `["XX"].contains(client.country)` or `client.asn < N` hold for the default record. Round 6: an IPv6 client against a table of IPv4
// prefixes read class 0 and such a rule failed open; found by tests/test_gpu_paths.py: test_lazy_comparison_atoms_agree_with_eager_ones_and_the_oracle)
void record_classes(const Program &P, TablePlan &out) {
    out.class_words = std::max(1u, out.cc_words + out.iu_words[1] + out.acmp_words);
    std::map<std::vector<uint32_t>, uint32_t> class_of;
    out.class_rows.assign(out.class_words, 0);  // class 0
    class_of.emplace(out.class_rows, 0u);
    std::vector<uint32_t> rec_class(P.geo_recs.size(), 0);
    for (size_t r = 0; r < P.geo_recs.size(); r++) {
        const std::vector<uint32_t> row = record_row(P.geo_recs[r], out);
        auto ins = class_of.emplace(row, (uint32_t)class_of.size());
        if (ins.second) out.class_rows.insert(out.class_rows.end(), row.begin(), row.end());
        rec_class[r] = ins.first->second;
    }
    out.n_classes = (uint32_t)class_of.size();
    out.geo_default = rec_class[0];
    auto remap = [&](const std::vector<uint32_t> &src) {
        std::vector<uint32_t> leaves(src);
        for (auto &x : leaves)
            if (x & TRIE_LEAF) x = TRIE_LEAF | rec_class[x & ~TRIE_LEAF];
        return leaves;
    };
    out.geo_root4 = remap(P.geo_trie.root4);
    out.geo_root6 = remap(P.geo_trie.root6);
    out.geo_nodes = remap(P.geo_trie.nodes);
}

}  // namespace

int plan_tables(const Program &P, size_t n_rules, size_t n_routes, TablePlan &out) {
    out = TablePlan();
    std::vector<NumAtomDev> atoms = P.num_atoms;
    if (int rc = merge_int_sets(P, atoms, out)) return rc;
    if (P.n_cols >= (1u << 20)) return fail(PWAF_E_UNSUPPORTED, "more than 2^20 predicate columns");
    if (P.set_words > kSetWordsMax) return fail(PWAF_E_UNSUPPORTED, "more than 512 ip lists");
    if (P.country_luts.size() > 32 * kCcWordsMax) return fail(PWAF_E_UNSUPPORTED, "more than 256 distinct client.country predicates");
    std::vector<uint32_t> bit_atoms;
    std::vector<NumAtomDev> cmp_src;
    split_atoms(atoms, bit_atoms, cmp_src);
    out.n_bit_atoms = (uint32_t)bit_atoms.size();
    out.bit_col.assign(kSrcWords * 32, 0);
    for (uint32_t d : bit_atoms) out.bit_col[(d >> 25) * 32 + ((d >> 20) & 31u)] = d & 0xFFFFFu;
    std::vector<Canon> canon;
    if (int rc = canonical_comparisons(cmp_src, out.hlen_fields, canon)) return rc;
    const std::vector<uint8_t> flipped = choose_polarity(P, canon);
    const std::vector<uint32_t> L = flip_literals(P.lits, flipped);
    if (int rc = encode_comparisons(canon, flipped, out)) return rc;
    // (rule indices travel as 16-bit values inside the verdict kernel; 0xFFF0.. is kept for the pseudo rules of the two gates)
    // (the caller's routes are device rules too: rules and routes share the limit)
    if (P.rules.size() > 65519 || n_rules + n_routes > 65519) return fail(PWAF_E_UNSUPPORTED, n_routes ? "more than 65519 rules and routes" : "more than 65519 rules");
    const TriggerUse use = trigger_lists(P, L, rarity_ranks(P, cmp_src, bit_atoms), out);
    const std::vector<uint32_t> lazy_of = select_lazy(P, use, out);
    out.n_cmp_atoms = (uint32_t)out.cmp_atoms.size();
    for (const CmpAtomDev &ca : out.cmp_atoms) out.cmp_vars |= 1u << std::min(31u, cmp_code_var(ca.col >> 24));
    out.n_lazy = (uint32_t)out.lazy_atoms.size();
    if (out.lazy_atoms.empty()) out.lazy_atoms.push_back({0, 0});
    out.lits = device_literals(L, lazy_of);
    transpose_countries(P, out);
    out.rules_unrouted = unrouted_rules(P);
    record_classes(P, out);
    return PWAF_OK;
}

}  // namespace pwaf
