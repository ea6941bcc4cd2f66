// tableplan.h — what the attribute and verdict kernels READ, decided on the host alone: from a compiled Program to every vector
// pwaf_engine_create uploads and every scalar it keeps beside them (tableplan.cpp). No HIP in here: the planner runs, and is tested,
// without a device (tests/tableplan_host.cpp, tests/test_tableplan_cpu.py).
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "program.h"

namespace pwaf {

// which verdict kernel (kernels.h: verdict_shape's mode): the entry list unless an A/B flag asks for an earlier column file
inline uint32_t verdict_mode(uint32_t flags) {
    const bool tiny = (flags & PWAF_OPT_TINY_VERDICT_SLOTS) != 0;
    if (flags & PWAF_OPT_DENSE_VERDICT) return 0u;
    if (flags & PWAF_OPT_SPARSE_VERDICT) return tiny ? 2u : 1u;
    return tiny ? 4u : 3u;
}

// the passes whose hit records the verdict kernel reads (VerdictArgs::n_passes): the scan passes, then the pseudo passes of the
// field-against-field atoms and of the residual rules — what verdict_shape is computed for
inline uint32_t verdict_pass_count(const Program &P) { return (uint32_t)P.groups.size() + (P.fcmp.empty() ? 0u : 1u) + (P.n_residual ? 1u : 0u); }

// Code of a comparison atom, bits [31:24] of CmpAtomDev::col: 2 * variable + operator (0: ==, 1: <=), | kCmpComplement when the device
// evaluates the atom complemented (!=, >). Variables: 0-4 field lengths, 5 remote_port, 6 asn, 7 + k the k-th compared header length;
// a LAZY atom's variable is its slot in TablePlan::lazy_vars.
static constexpr uint32_t kCmpComplement = 0x80u, kCmpVarAsn = 6u, kCmpVarHeader = 7u;
inline uint32_t cmp_code(uint32_t var, uint32_t op, bool complement) { return (2u * var + op) | (complement ? kCmpComplement : 0u); }
inline uint32_t cmp_code_var(uint32_t code) { return (code & 0x7Fu) / 2u; }

// What the per-batch code reads of a plan besides the uploaded tables: their widths and counts. The engine keeps a copy for life.
struct PlanShape {
    uint32_t iu_n[2] = {0, 0}, iu_words[2] = {1, 1};  // integer sets per variable: distinct values, words per membership row
    uint32_t n_bit_atoms = 0;
    uint32_t n_cmp_atoms = 0, cmp_vars = 0;  // the eager comparison atoms (VerdictArgs::cmp_vars: bit per variable some of them reads)
    uint32_t n_lazy = 0;
    std::vector<uint32_t> lazy_vars;    // (VerdictArgs::lazy_var) at most two
    std::vector<uint32_t> hlen_fields;  // header columns whose length some rule compares (comparison variable 7 + k)
    uint32_t n_trig = 0;
    uint32_t cc_words = 1, acmp_words = 0;
    uint32_t class_words = 1, n_classes = 1, geo_default = 0;  // (geo_default: the class of GeoIP record 0)
};

struct TablePlan : PlanShape {
    // integer sets, merged per variable (0 = remote_port, 1 = asn): sorted distinct values + membership rows (row 0 = miss)
    std::vector<int64_t> iu_vals[2];
    std::vector<uint32_t> iu_masks[2];
    std::vector<uint32_t> bit_col;       // [kSrcWords source words][32 bits] -> column of the membership atom, 0 = none
    std::vector<CmpAtomDev> cmp_atoms;   // the EAGER comparison atoms (attr_kernel)
    std::vector<CmpAtomDev> lazy_atoms;  // one {0, 0} when there is none (n_lazy says how many are real)
    std::vector<uint32_t> lits;          // Program::lits as the device evaluates them: polarity applied, lazy atoms as LIT_LAZY words
    std::vector<uint32_t> trig_off;      // n_cols + 1 offsets into trig_rules
    std::vector<uint16_t> trig_rules;
    std::vector<uint32_t> always;        // bitmap of the rules that are candidates in every group
    std::vector<uint32_t> cc_masks;      // transposed country tables: [676][cc_words]
    std::vector<std::pair<uint32_t, uint32_t>> acmp;  // (operator 0: ==, 1: <=; constant) of the client.asn comparisons, in class-row bit order
    std::vector<uint32_t> class_rows;    // [n_classes][class_words]: country-table bits | asn-set bits | asn comparisons
    std::vector<uint32_t> geo_root4, geo_root6, geo_nodes;  // Program::geo_trie with CLASS leaves
    std::vector<DevRule> rules_unrouted;  // device routes and PWAF_OPT_RULE_HITS: Program::rules with the routes' literal lists emptied; else empty
};

// Fills `out` from P. n_rules / n_routes: what the caller handed to the compiler (they share the device's rule limit).
// PWAF_OK, or PWAF_E_UNSUPPORTED with the reason in pwaf::fail (`out` is then half filled: discard it). Deterministic; reads no environment.
int plan_tables(const Program &P, size_t n_rules, size_t n_routes, TablePlan &out);

}  // namespace pwaf
