"""The table planner on the CPU (no device): csrc/tableplan.cpp's plan_tables — what pwaf_engine_create runs between the rule compiler and
the uploads — through the host harness tests/tableplan_host.cpp, checked against brute force written here from the program DUMP alone
(NUMA with the original operators and 64-bit constants, INTP, CLUT, RULE, LITS, GREC and the record-leaf tries): truth tables of every
rule over the plan's device literals, trigger lists, integer-set unions, the (source word, bit) table, GeoIP classes, the flags that
switch lazy atoms off, the route-less rule table, and the planner's refusals with their exact text.

The four widths of the attribute rows (128 integer sets per variable, 8 header lengths, 128 asn comparisons, 256 country tables) are
counted by the rule compiler too, which lowers the rule that would cross one to a residual program (test_compiler.py:
test_rule_sets_beyond_a_device_table_width_fall_to_residual_programs): no rule set reaches the planner's refusal of them. Their
largest accepted / smallest refused case is therefore tested twice: with rule sets (the compiler's answer, and the plan of what it
hands on), and with hand-made programs (harness --synthetic) for the planner's own code and message."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import helpers as H
from pingoo_amd import _abi, geoip_entries
from plan_harness import COMPILER_UNITS, U32, tool as plan_tool, write_case
from table_walker import (ATOM_COUNTRY, ATOM_INT, ATOM_INTSET, ATOM_IPSET, ATOM_LEN, GREC_DTYPE, LIT_ATOM_MASK, LIT_NEG, LIT_TERM_END, NUMA_DTYPE, OP_EQ, OP_GE, OP_GT, OP_LE, OP_LT,
                          OP_NE, RULE_DTYPE, TRIE_LEAF, parse_dump)

HERE = os.path.dirname(os.path.abspath(__file__))
UNITS = COMPILER_UNITS + ["tableplan.cpp"]
SRC = os.path.join(HERE, "tableplan_host.cpp")

LIT_LAZY, LAZY_CONST, LAZY_OP, LAZY_SLOT, LAZY_COMPLEMENT = 1 << 29, 0xFFFF, 1 << 16, 1 << 17, 1 << 18  # (program.h)
SRC_CC, SRC_PORT, SRC_ASN, SRC_ACMP, SRC_WORDS = 16, 24, 28, 32, 36  # (program.h: source words of the membership atoms)
N_FIELDS = 5
B = _abi.RULE_ACTION_BLOCK
NO_LAZY_FLAGS = [_abi.OPT_EAGER_CMP, _abi.OPT_SPARSE_VERDICT, _abi.OPT_DENSE_VERDICT, _abi.OPT_SPARSE_VERDICT | _abi.OPT_TINY_VERDICT_SLOTS]


# ---------------------------------------------------------------------------------------------------------
# the harness
# ---------------------------------------------------------------------------------------------------------
def tool(name="tableplan_host", *extra):
    return plan_tool(name, SRC, UNITS, *extra)


def run_cases(tmp_path, cases, exe=None):
    """cases: [dict(rules=, routes=, lists=, geo=, flags=)] -> [(status, Plan | None)], one process for all of them"""
    args = []
    for k, c in enumerate(cases):
        fc, fo = str(tmp_path / f"case{k}.bin"), str(tmp_path / f"case{k}.out")
        write_case(fc, **c)
        args += [fc, fo]
    r = subprocess.run([exe or tool(), *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(cases), r.stdout[-2000:]
    res = []
    for k, line in enumerate(lines):
        st = json.loads(line)
        res.append((st, Plan(open(args[2 * k + 1], "rb").read()) if st["stage"] == "ok" else None))
    for f in args:
        if os.path.exists(f):
            os.remove(f)
    return res


def run_one(tmp_path, rules, **kw):
    (st, plan), = run_cases(tmp_path, [dict(rules=rules, **kw)])
    return st, plan


def synthetic(kind, n):
    r = subprocess.run([tool(), "--synthetic", kind, str(n)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


class Plan:
    """the harness's output: the program dump's sections, then the plan's ("P...")"""

    def __init__(self, blob):
        sec = {}
        for tag, count, payload in parse_dump(blob):
            sec.setdefault(tag, payload)  # (per-group sections repeat: not read here)
        u4 = lambda tag: np.frombuffer(sec[tag], dtype="<u4")  # noqa: E731
        head = u4("HEAD")
        self.n_cols, self.n_rules, self.set_words, self.flags = int(head[0]), int(head[3]), int(head[5]), int(head[7])
        self.numa = np.frombuffer(sec["NUMA"], dtype=NUMA_DTYPE)
        self.intp = np.frombuffer(sec["INTP"], dtype="<i8")
        self.clut = u4("CLUT").reshape(-1, 22)
        self.rules = np.frombuffer(sec["RULE"], dtype=RULE_DTYPE)
        self.lits = u4("LITS")
        self.grec = np.frombuffer(sec["GREC"], dtype=GREC_DTYPE)
        self.gr4, self.gr6, self.gnod = u4("GR4 "), u4("GR6 "), u4("GNOD")
        self.n_residual = int(u4("RSDL")[0]) if "RSDL" in sec else 0
        self.rout = [int(x) for x in u4("ROUT")] if "ROUT" in sec else None  # route_base, n_dev_routes, n_routes, n_user_rules
        shp = [int(x) for x in u4("PSHP")]
        (self.iu_n, self.iu_words) = (shp[0:2], shp[2:4])
        (self.n_bit_atoms, self.n_cmp_atoms, self.cmp_vars, self.n_lazy, self.n_trig, self.cc_words, self.acmp_words, self.class_words, self.n_classes,
         self.geo_default) = shp[4:14]
        self.lazy_vars, self.hlen_fields = [int(x) for x in u4("PLZV")], [int(x) for x in u4("PHLN")]
        self.iu_vals = [np.frombuffer(sec["PIV0"], dtype="<i8"), np.frombuffer(sec["PIV1"], dtype="<i8")]
        self.iu_masks = [u4("PIM0"), u4("PIM1")]
        self.bit_col, self.dev_lits, self.trig_off, self.always, self.cc_masks = u4("PBIT"), u4("PLIT"), u4("PTOF"), u4("PALW"), u4("PCCM")
        self.cmp_atoms, self.lazy_atoms, self.acmp = u4("PCMP").reshape(-1, 2), u4("PLZY").reshape(-1, 2), u4("PACM").reshape(-1, 2)
        self.trig_rules = np.frombuffer(sec["PTRL"], dtype="<u2")
        self.class_rows = u4("PCLS")
        self.pgr4, self.pgr6, self.pgnd = u4("PGR4"), u4("PGR6"), u4("PGND")
        self.unrouted = np.frombuffer(sec["PUNR"], dtype=RULE_DTYPE)


# ---------------------------------------------------------------------------------------------------------
# brute force
# ---------------------------------------------------------------------------------------------------------
def compare(op, v, c):
    """the ORIGINAL comparison of a NUMA entry: values are non-negative Python ints / int64 arrays, c a 64-bit constant"""
    return {OP_EQ: v == c, OP_NE: v != c, OP_LT: v < c, OP_LE: v <= c, OP_GT: v > c, OP_GE: v >= c}[op]


def terms_of(lits, rule):
    """[[literal word, ...], ...] of one rule"""
    out, cur = [], []
    for k in range(int(rule["lit_off"]), int(rule["lit_off"]) + int(rule["lit_cnt"])):
        cur.append(int(lits[k]))
        if lits[k] & LIT_TERM_END:
            out.append(cur)
            cur = []
    assert not cur, "a rule's last literal ends a term"
    return out


def is_cmp(a):
    return a["kind"] in (ATOM_LEN, ATOM_INT)


def source_var(a):
    """the request value a comparison entry of NUMA reads: ("len", field) | ("port",) | ("asn",)"""
    return ("len", int(a["var"])) if a["kind"] == ATOM_LEN else ("port",) if a["var"] == 0 else ("asn",)


def plan_var(p, vi):
    """the request value behind a variable index of the plan"""
    return ("len", vi) if vi < 5 else ("port",) if vi == 5 else ("asn",) if vi == 6 else ("len", p.hlen_fields[vi - 7])


def draw_values(p, rng, n):
    """n requests' worth of every compared value: the constants of the atoms and their neighbours, the edges of the 16- and 32-bit ranges, random"""
    pool = {}
    for a in p.numa:
        if is_cmp(a):
            c = int(a["c"])
            pool.setdefault(source_var(a), set()).update(min(max(v, 0), U32) for v in (c - 1, c, c + 1))
    vals = {}
    for var, s in pool.items():
        cand = sorted(s | {0, 1, 0xFFFE, 0xFFFF, 0x10000, 0x10001, U32 - 1, U32})
        vals[var] = np.array([rng.choice(cand) if rng.random() < 0.8 else rng.randrange(1 << rng.choice([4, 16, 32])) for _ in range(n)], dtype=np.int64)
    return vals


def check_truth_table(p, rng, n=300):
    """every rule's DNF over the dump's literals (columns from NUMA's original comparisons) == its DNF over the plan's device literals
    (eager columns from the plan's canonical atoms, lazy literals decoded from the literal word)"""
    vals = draw_values(p, rng, n)
    nrng = np.random.default_rng(rng.getrandbits(32))
    src_cols = nrng.integers(0, 2, size=(p.n_cols, n)).astype(bool)  # arbitrary bits for everything that is no comparison
    src_cols[0] = True
    dev_cols = src_cols.copy()
    for a in p.numa:
        if is_cmp(a):
            src_cols[a["col"]] = compare(int(a["op"]), vals[source_var(a)], int(a["c"]))
            dev_cols[a["col"]] = False  # (a comparison the plan drops — it can never hold — leaves its column zero)
    for word, c in p.cmp_atoms:
        col, code = int(word) & 0xFFFFFF, int(word) >> 24
        v = vals[plan_var(p, (code & 0x7F) // 2)]
        dev_cols[col] = ((v <= int(c)) if code & 1 else (v == int(c))) ^ bool(code & 0x80)

    def lazy_value(w):
        v = vals[plan_var(p, p.lazy_vars[1 if w & LAZY_SLOT else 0])]
        return ((v <= (w & LAZY_CONST)) if w & LAZY_OP else (v == (w & LAZY_CONST))) ^ bool(w & LAZY_COMPLEMENT)

    def dnf(lits, rule, cols, device):
        acc = np.zeros(n, dtype=bool)
        for term in terms_of(lits, rule):
            t = np.ones(n, dtype=bool)
            for w in term:
                x = lazy_value(w) if device and w & LIT_LAZY else cols[w & LIT_ATOM_MASK]
                t &= ~x if w & LIT_NEG else x
            acc |= t
        return acc

    assert len(p.dev_lits) == len(p.lits)
    assert not (p.lits & LIT_LAZY).any()
    for r, rule in enumerate(p.rules):
        want, got = dnf(p.lits, rule, src_cols, False), dnf(p.dev_lits, rule, dev_cols, True)
        assert (want == got).all(), f"rule {r}: request {int(np.nonzero(want != got)[0][0])} differs"


def check_triggers(p):
    lazy_cols = {int(p.lits[k] & LIT_ATOM_MASK) for k in np.nonzero(p.dev_lits & LIT_LAZY)[0]}
    assert len(p.trig_off) == p.n_cols + 1 and p.trig_off[0] == 0 and (np.diff(p.trig_off.astype(np.int64)) >= 0).all()
    assert p.n_trig == len(p.trig_rules) == p.trig_off[-1]
    filed = {c: set(p.trig_rules[p.trig_off[c]:p.trig_off[c + 1]].tolist()) for c in range(p.n_cols) if p.trig_off[c + 1] > p.trig_off[c]}
    allowed = set()
    for r, rule in enumerate(p.rules):
        bare = False
        for term in terms_of(p.dev_lits, rule):
            positive = [w for w in term if not w & LIT_NEG]
            usable = [w & LIT_ATOM_MASK for w in positive if not w & LIT_LAZY]
            if not positive:
                bare = True
                assert not any(w & LIT_LAZY for w in term), f"rule {r}: a lazy atom stands in a term of negations only"
            else:
                assert any(r in filed.get(c, ()) for c in usable), f"rule {r}: a term with a positive literal is filed under none of its columns"
            allowed |= {(c, r) for c in usable}
        assert bool(p.always[r >> 5] >> (r & 31) & 1) == bare, f"rule {r}: always-candidate bit"
    assert {(c, r) for c, rs in filed.items() for r in rs} <= allowed, "a rule is filed under a column that is no positive literal of it"
    assert not lazy_cols & set(filed), "a lazy column has a trigger entry"
    # a lazy atom is lazy in every literal of it, with one word; n_lazy and the variables
    word_of = {}
    for k in range(len(p.lits)):
        col = int(p.lits[k] & LIT_ATOM_MASK)
        if col in lazy_cols:
            assert p.dev_lits[k] & LIT_LAZY and word_of.setdefault(col, int(p.dev_lits[k]) & 0x7FFFF) == int(p.dev_lits[k]) & 0x7FFFF
            assert int(p.dev_lits[k]) & ~(LIT_NEG | LIT_TERM_END | LIT_LAZY | 0x7FFFF) == 0
        else:
            assert int(p.dev_lits[k]) & ~LIT_NEG == int(p.lits[k]) & ~LIT_NEG
    assert len(p.lazy_vars) <= 2 and all(not (w & LAZY_SLOT) or len(p.lazy_vars) == 2 for w in word_of.values())
    assert p.n_lazy >= len(word_of) and len(p.lazy_atoms) == max(1, p.n_lazy)
    if p.n_lazy == 0:
        assert p.lazy_atoms.tolist() == [[0, 0]] and not p.lazy_vars
    eager_cols = {int(w) & 0xFFFFFF for w, _ in p.cmp_atoms}
    assert p.n_cmp_atoms == len(p.cmp_atoms) and not eager_cols & lazy_cols
    want_vars = 0
    for w, _ in p.cmp_atoms:
        want_vars |= 1 << min(31, ((int(w) >> 24) & 0x7F) // 2)
    assert p.cmp_vars == want_vars
    # client.asn comparisons: never lazy, never flipped
    flipped = {int(p.lits[k] & LIT_ATOM_MASK) for k in range(len(p.lits)) if (int(p.lits[k]) ^ int(p.dev_lits[k])) & LIT_NEG}
    for a in p.numa:
        if a["kind"] == ATOM_INT and a["var"] == 1:
            assert int(a["col"]) not in lazy_cols and int(a["col"]) not in flipped
    for w, _ in p.cmp_atoms:
        if ((int(w) >> 24) & 0x7F) // 2 == 6:
            assert not (int(w) >> 24) & 0x80
    return lazy_cols, flipped


def check_int_sets(p):
    bit_of = {}
    for var in (0, 1):
        sets = [a for a in p.numa if a["kind"] == ATOM_INTSET and a["var"] == var]
        members = [set(p.intp[a["ref"]:a["ref2"]].tolist()) for a in sets]
        vals, words = p.iu_vals[var], p.iu_words[var]
        assert words == max(1, (len(sets) + 31) // 32) and p.iu_n[var] == len(vals)
        assert vals.tolist() == sorted(set().union(*members)) and (np.diff(vals) > 0).all()
        rows = p.iu_masks[var].reshape(len(vals) + 1, words)
        assert not rows[0].any()
        for i, v in enumerate(vals.tolist()):
            assert [int(rows[i + 1][k >> 5] >> (k & 31) & 1) for k in range(32 * words)] == [int(k < len(sets) and v in members[k]) for k in range(32 * words)]
        for k, a in enumerate(sets):
            bit_of[int(a["col"])] = ((SRC_PORT, SRC_ASN)[var] + (k >> 5), k & 31)
    return bit_of


def canonical(a):
    """(op 0 ==, 1 <=; constant) of a comparison over unsigned 32-bit values, None when it can never hold"""
    c, op = int(a["c"]), int(a["op"])
    if op == OP_EQ:
        return (0, c) if 0 <= c <= U32 else None
    assert op in (OP_LT, OP_LE)  # (the compiler writes the other three as negations of these)
    c -= op == OP_LT
    return (1, min(c, U32)) if c >= 0 else None


def check_bit_table(p, intset_bits):
    want = np.zeros(SRC_WORDS * 32, dtype=np.int64)
    n_members = 0
    for a in p.numa:
        if a["kind"] == ATOM_IPSET:
            src, bit = int(a["ref"]) >> 5, int(a["ref"]) & 31
        elif a["kind"] == ATOM_COUNTRY:
            src, bit = SRC_CC + (int(a["ref"]) >> 5), int(a["ref"]) & 31
        elif a["kind"] == ATOM_INTSET:
            src, bit = intset_bits[int(a["col"])]
        else:
            continue
        n_members += 1
        want[src * 32 + bit] = a["col"]
    # the client.asn comparisons: bit j of the class row's comparison words, in the plan's order
    asn_cmp = {int(a["col"]): canonical(a) for a in p.numa if a["kind"] == ATOM_INT and a["var"] == 1 and canonical(a) is not None}
    assert len(p.acmp) == len(asn_cmp) and p.acmp_words == (len(asn_cmp) + 31) // 32
    for j, (op, c) in enumerate(p.acmp.tolist()):
        col = int(p.bit_col[(SRC_ACMP + j // 32) * 32 + (j & 31)])
        assert asn_cmp.get(col) == (op, c), (j, col)
        want[(SRC_ACMP + j // 32) * 32 + (j & 31)] = col
    assert len({int(p.bit_col[(SRC_ACMP + j // 32) * 32 + (j & 31)]) for j in range(len(p.acmp))}) == len(p.acmp)
    assert p.bit_col.tolist() == want.tolist() and p.n_bit_atoms == n_members


def check_classes(p):
    cw, iw = p.cc_words, p.iu_words[1]
    assert cw == max(1, (len(p.clut) + 31) // 32) and p.class_words == max(1, cw + iw + p.acmp_words)
    masks = p.cc_masks.reshape(676, cw)
    for c in range(676):
        assert [int(masks[c][t >> 5] >> (t & 31) & 1) for t in range(len(p.clut))] == [int(p.clut[t][c >> 5] >> (c & 31) & 1) for t in range(len(p.clut))]
    rows = p.class_rows.reshape(p.n_classes, p.class_words)
    assert not rows[0].any() and len({tuple(r) for r in rows.tolist()}) == p.n_classes
    asn_sets = [set(p.intp[a["ref"]:a["ref2"]].tolist()) for a in p.numa if a["kind"] == ATOM_INTSET and a["var"] == 1]
    by_col = {int(a["col"]): a for a in p.numa}
    asn_cmps = [by_col[int(p.bit_col[(SRC_ACMP + j // 32) * 32 + (j & 31)])] for j in range(len(p.acmp))]

    def brute_row(rec):
        row = [0] * p.class_words
        c0, c1 = (int(rec["country"]) & 0xFF) - 65, (int(rec["country"]) >> 8) - 65
        cidx = c0 * 26 + c1 if 0 <= c0 < 26 and 0 <= c1 < 26 else 23 * 26 + 23  # (anything else reads as "XX")
        for t in range(len(p.clut)):
            row[t >> 5] |= int(p.clut[t][cidx >> 5] >> (cidx & 31) & 1) << (t & 31)
        for k, s in enumerate(asn_sets):
            row[cw + (k >> 5)] |= int(int(rec["asn"]) in s) << (k & 31)
        for j, a in enumerate(asn_cmps):
            row[cw + iw + (j >> 5)] |= int(bool(compare(int(a["op"]), int(rec["asn"]), int(a["c"])))) << (j & 31)
        return row

    # record -> class, read off the leaves of the remapped tries (and record 0 from geo_default)
    cls = {0: p.geo_default}
    for src, dst in ((p.gr4, p.pgr4), (p.gr6, p.pgr6), (p.gnod, p.pgnd)):
        assert len(src) == len(dst)
        leaf = (src & TRIE_LEAF) != 0
        assert (dst[~leaf] == src[~leaf]).all() and ((dst & TRIE_LEAF) != 0).tolist() == leaf.tolist()
        for rec, c in set(zip((src[leaf] & ~np.uint32(TRIE_LEAF)).tolist(), (dst[leaf] & ~np.uint32(TRIE_LEAF)).tolist())):
            assert cls.setdefault(rec, c) == c, f"record {rec} has two classes"
    for rec, c in cls.items():
        assert c < p.n_classes and rows[c].tolist() == brute_row(p.grec[rec]), f"record {rec}, class {c}"
    return cls


def check_unrouted(p):
    if p.rout and p.rout[1] and p.flags & _abi.OPT_RULE_HITS:
        want = p.rules.copy()
        want["lit_cnt"][p.rout[0]:] = 0
        assert p.unrouted.tobytes() == want.tobytes() and p.rout[0] + p.rout[1] == len(p.rules)
    else:
        assert len(p.unrouted) == 0


def check_plan(p, seed=1):
    check_truth_table(p, random.Random(seed))
    lazy_cols, flipped = check_triggers(p)
    check_bit_table(p, check_int_sets(p))
    check_classes(p)
    check_unrouted(p)
    if p.flags & (_abi.OPT_EAGER_CMP | _abi.OPT_SPARSE_VERDICT | _abi.OPT_DENSE_VERDICT):
        assert not lazy_cols and not flipped and p.n_lazy == 0 and p.dev_lits.tolist() == p.lits.tolist()
        assert not any((int(w) >> 24) & 0x80 for w, _ in p.cmp_atoms)
    return lazy_cols, flipped


# ---------------------------------------------------------------------------------------------------------
# rule sets
# ---------------------------------------------------------------------------------------------------------
CONSTS = [0xFFFF, -1, 1, 0, 0x10000, 1 << 32, U32, (1 << 32) + 5]
OPS = ["==", "!=", "<", "<=", ">", ">="]
GEO_ROWS = [("10.0.0.0/8", 64512, "FR"), ("10.1.0.0/16", 0, "US"), ("10.1.2.0/25", 65535, "XX"), ("11.0.0.0/8", 65536, "DE"), ("12.0.0.0/8", U32, "FR"),
            ("2001:db8::/32", 1, "CN"), ("2001:db8:1::/48", 64512, "zz"), ("::/0", 2, "DE"), ("0.0.0.0/0", 65534, "AA")]
LISTS = {"nets": (_abi.LIST_IP, ["10.0.0.0/8", "2001:db8::/32"]), "more": (_abi.LIST_IP, ["1.2.3.4"]), "asns": (_abi.LIST_INT, ["64512", " 7 "])}


def comparison_rules():
    """every operator x every constant on a field length, a header length, remote_port and client.asn — beside a rarer literal (the
    shape that becomes lazy), alone, negated beside a literal, in a disjunction and negated alone (a term without a trigger) — plus
    memberships of every kind. `==`/`!=`, `<`/`>=` and `<=`/`>` share an atom: the constants at even places give all six operators
    one shape (atoms that can be lazy), the others a shape per operator (atoms some other rule keeps eager)."""
    words = H.pass_words(5, 4 * len(CONSTS) * len(OPS))
    rules = []
    for vi, var in enumerate(("http_request.url.length()", 'http_request.headers["x-len"].length()', "client.remote_port", "client.asn")):
        for ci, c in enumerate(CONSTS):
            for oi, op in enumerate(OPS):
                k, w = len(rules), words[len(rules)]
                cmp_ = f"{var} {op} {c}"
                expr = [f'http_request.path.contains("{w}") && {cmp_}', cmp_, f'!({cmp_}) && http_request.host.contains("{w}")',
                        f'{cmp_} || http_request.path.length() > {k % 7}', f'!({cmp_})'][(ci + vi + (oi if ci % 2 else 0)) % 5]
                rules.append((f"r{k}", expr, [B]))
    # atoms that only ever stand negated, beside a rarer literal: flipped AND lazy (the complement bit of the literal word)
    rules += [("c0", 'http_request.path.contains("zzq") && http_request.url.length() > 37', [B]), ("c1", 'http_request.host.contains("qzz") && http_request.url.length() != 17', [B]),
              ("c2", 'http_request.path.contains("zqz") && http_request.method.length() >= 9', [B])]
    rules += [("m0", "[80, 443, 65535].contains(client.remote_port)", [B]), ("m1", "[64512, 1, 0].contains(client.asn) && client.remote_port > 1024", [B]),
              ("m2", '["FR", "XX"].contains(client.country)', [B]), ("m3", 'client.country == "DE" && http_request.method.length() < 4', [B]),
              ("m4", 'lists["nets"].contains(client.ip) || lists["asns"].contains(client.asn)', [B]), ("m5", 'client.ip in lists.more && !(client.asn in [2, 3])', [B]),
              ("m6", None, [_abi.RULE_ACTION_CAPTCHA])]
    return rules


def fuzz_case(seed, flags=0, routes=False):
    rng = random.Random(seed)
    lists = H.fuzz_lists(rng, seed % 3 == 0)
    geo = H.fuzz_geoip(rng, seed % 3 == 0) if rng.random() < 0.7 else None
    rules = [(f"r{k}", H.rexpr(rng, lists) if rng.random() < 0.95 else None, H.fuzz_actions(rng)) for k in range(rng.randint(1, 12))]
    rt = [(f"s{k}", H.rexpr(rng, lists) if rng.random() < 0.9 else None) for k in range(rng.randint(1, 4))] if routes else None
    return dict(rules=rules, routes=rt, lists=lists, geo=geo, flags=flags | _abi.OPT_LENIENT)


# ---------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, _abi.OPT_TINY_VERDICT_SLOTS] + NO_LAZY_FLAGS)
def test_every_comparison_shape_against_brute_force(tmp_path, flags):
    st, p = run_one(tmp_path, comparison_rules(), lists=LISTS, geo=geoip_entries(GEO_ROWS), flags=flags)
    assert st["stage"] == "ok" and p.n_residual == 0, st
    lazy_cols, flipped = check_plan(p)
    assert p.hlen_fields == [5] and len(p.grec) == len(GEO_ROWS)  # (the row with country "zz" reads the default record)
    if flags in (0, _abi.OPT_TINY_VERDICT_SLOTS):
        # both mechanisms are exercised, on both sides of the 16-bit constant a literal word holds
        # (lazy at least: the three atoms of url.length() against 0xFFFF and against 1, those of c0, c1, c2 and m3's method.length() — variables 1 and 3, which
        # take both slots: remote_port against 0xFFFF stands in the same shape as url.length() against 1 and stays eager)
        assert len(lazy_cols) >= 10 and len(flipped) >= 3 and p.lazy_vars == [1, 3] and p.n_lazy == len(lazy_cols)
        words = {int(w) for w in p.dev_lits if w & LIT_LAZY}  # every field of the literal word takes both values
        for bit in (LAZY_OP, LAZY_SLOT, LAZY_COMPLEMENT, LIT_NEG):
            assert any(w & bit for w in words) and any(not w & bit for w in words), hex(bit)
        port_cols = {int(a["col"]) for a in p.numa if a["kind"] == ATOM_INT and a["var"] == 0 and a["c"] == 0xFFFF}
        assert len(port_cols) == 3 and not port_cols & lazy_cols
        consts = {int(c) for _, c in p.lazy_atoms}
        assert 0xFFFF in consts and max(consts) == 0xFFFF and any(int(c) > 0xFFFF for _, c in p.cmp_atoms)
    else:
        assert p.n_lazy == 0


def test_fuzzed_rule_sets_against_brute_force(tmp_path):
    cases = [fuzz_case(7000 + s, flags=(0, 0, _abi.OPT_EAGER_CMP, _abi.OPT_SPARSE_VERDICT)[s % 4]) for s in range(24)]
    cases += [fuzz_case(7100 + s, flags=_abi.OPT_RULE_HITS, routes=True) for s in range(8)]
    n_lazy = n_flipped = 0
    for k, (st, p) in enumerate(run_cases(tmp_path, cases)):
        assert st["stage"] == "ok", (k, st)
        lazy_cols, flipped = check_plan(p, seed=k)
        n_lazy, n_flipped = n_lazy + len(lazy_cols), n_flipped + len(flipped)
    assert n_lazy > 0 and n_flipped > 0


@pytest.mark.parametrize("family", ["v4", "v6", "both", "none"])
def test_classes_of_a_table_with_one_family(tmp_path, family):
    rows = [r for r in GEO_ROWS if family == "both" or (":" in r[0]) == (family == "v6")] if family != "none" else None
    rules = [("a", '["XX", "FR"].contains(client.country)', [B]), ("b", "client.asn < 65535", [B]), ("c", "client.asn == 0 || client.asn >= 64512", [B]),
             ("d", "[0, 2, 64512].contains(client.asn)", [B]), ("e", 'client.country != "DE"', [B])]
    st, p = run_one(tmp_path, rules, geo=geoip_entries(rows) if rows else None)
    assert st["stage"] == "ok", st
    check_plan(p)
    cls = check_classes(p)
    # the default record {0, "XX"} satisfies a, b, c, d, e: its class is not class 0, and a family without prefixes reads it
    assert p.geo_default != 0 and cls[0] == p.geo_default
    assert (len(p.pgr4) == 65536) == (family in ("v4", "both")) and (len(p.pgr6) == 65536) == (family in ("v6", "both"))
    if rows:
        assert len(cls) >= 3 and p.n_classes >= 3


def test_route_less_rule_table_only_with_routes_and_rule_hits(tmp_path):
    rules = [("r0", 'http_request.path.contains("ab")', [B]), ("r1", "client.remote_port > 80", []), ("r2", 'http_request.host == "h"', [B])]
    routes = [("s0", 'http_request.host.starts_with("api.")'), ("s1", "false"), ("s2", None)]
    res = run_cases(tmp_path, [dict(rules=rules, routes=routes, flags=_abi.OPT_RULE_HITS), dict(rules=rules, routes=routes), dict(rules=rules, flags=_abi.OPT_RULE_HITS),
                               dict(rules=rules, routes=[("s1", "false")], flags=_abi.OPT_RULE_HITS)])
    for st, p in res:
        assert st["stage"] == "ok", st
        check_plan(p)
    hits, plain, unrouted, dropped = (p for _, p in res)
    assert hits.rout[1] == 2 and len(hits.unrouted) == len(hits.rules) and (hits.unrouted["lit_cnt"][hits.rout[0]:] == 0).all()
    assert (hits.unrouted["lit_cnt"][:hits.rout[0]] == hits.rules["lit_cnt"][:hits.rout[0]]).all() and hits.rules["lit_cnt"][hits.rout[0]:].all()
    assert len(plain.unrouted) == 0 and len(unrouted.unrouted) == 0 and unrouted.rout is None
    assert dropped.rout[1] == 0 and len(dropped.unrouted) == 0  # (the only route can never match: no device route)


WIDTHS = {
    "intset0": (128, lambda k: f"[{k + 2}, {70000 + k}].contains(client.remote_port)", "more than 128 integer-set predicates on one client variable"),
    "intset1": (128, lambda k: f"[{k + 2}, {70000 + k}].contains(client.asn)", "more than 128 integer-set predicates on one client variable"),
    "hlen": (8, lambda k: f'http_request.headers["x-h{k}"].length() > 3', "length() of more than 8 distinct headers is compared"),
    "asncmp": (128, lambda k: f"client.asn == {1000 + k}", "more than 128 distinct client.asn comparisons"),
    "country": (256, lambda k: f'client.country == "{chr(65 + k // 26)}{chr(65 + k % 26)}"', "more than 256 distinct client.country predicates"),
}


@pytest.mark.parametrize("what", sorted(WIDTHS))
def test_attribute_row_widths_at_and_past_the_limit(tmp_path, what):
    limit, expr, message = WIDTHS[what]
    at = [(f"r{k}", expr(k), [B]) for k in range(limit)]
    past = at + [(f"r{limit}", expr(limit), [B])]
    (st_at, p_at), (st_past, p_past), (st_col, _) = run_cases(tmp_path, [dict(rules=at), dict(rules=past), dict(rules=past, flags=_abi.OPT_NO_RESIDUAL)])
    # the largest accepted rule set: planned whole, on the columns
    assert st_at["stage"] == "ok" and p_at.n_residual == 0
    check_plan(p_at)
    # one more: the compiler hands the planner a program within the width (the last rule runs as a residual program) ...
    assert st_past["stage"] == "ok" and p_past.n_residual == 1
    check_plan(p_past)
    # ... and without the residual interpreter it refuses the RULE, with the text the planner keeps for a program that got past it
    assert st_col == {"stage": "compile", "rc": _abi.E_UNSUPPORTED, "rule_index": limit, "message": f"rule r{limit}: {message}"}
    # the planner's own limit (hand-made programs)
    assert synthetic(what, limit) == {"stage": "ok", "rc": 0, "rule_index": U32, "message": ""}
    assert synthetic(what, limit + 1) == {"stage": "plan", "rc": _abi.E_UNSUPPORTED, "rule_index": U32, "message": message}


def test_ip_list_limit(tmp_path):
    """set_words <= 16: 512 ip lists, referenced or not (the one refusal of the attribute rows a rule set does reach)"""
    lists = lambda n: {f"l{k}": (_abi.LIST_IP, [f"10.{k >> 8}.{k & 255}.0/24"]) for k in range(n)}  # noqa: E731
    rules = [("r", 'lists["l0"].contains(client.ip) || client.ip in lists.l511', [B])]
    (st_at, p), (st_past, _) = run_cases(tmp_path, [dict(rules=rules, lists=lists(512)), dict(rules=rules, lists=lists(513))])
    assert st_at["stage"] == "ok" and p.set_words == 16
    check_plan(p)
    assert st_past == {"stage": "plan", "rc": _abi.E_UNSUPPORTED, "rule_index": U32, "message": "more than 512 ip lists"}
    assert synthetic("set_words", 16)["stage"] == "ok" and synthetic("set_words", 17)["message"] == "more than 512 ip lists"


def test_rule_and_route_count_limit(tmp_path):
    """65519 DEVICE rules — the caller's, the two gates' pseudo rules, the routes — and 65519 rules and routes as the caller counts them"""
    rules = lambda n: [("r", "client.remote_port == 1", [B])] * n  # noqa: E731
    no_gates = _abi.OPT_NO_UA_GATE | _abi.OPT_NO_CAPTCHA_BYPASS
    res = run_cases(tmp_path, [dict(rules=rules(65517)), dict(rules=rules(65518)), dict(rules=rules(65519), flags=no_gates), dict(rules=rules(65520), flags=no_gates),
                               dict(rules=rules(65518), routes=[("s", None)], flags=no_gates), dict(rules=rules(65518), routes=[("s", None), ("t", "false")], flags=no_gates)])
    assert [st["stage"] for st, _ in res] == ["ok", "plan", "ok", "plan", "ok", "plan"]
    assert [len(p.rules) for _, p in res[::2]] == [65519, 65519, 65519]
    refused = lambda text: {"stage": "plan", "rc": _abi.E_UNSUPPORTED, "rule_index": U32, "message": text}  # noqa: E731
    assert res[1][0] == res[3][0] == refused("more than 65519 rules")
    assert res[5][0] == refused("more than 65519 rules and routes")  # (the second route never matches and is no device rule: the caller's count decides)
    for _, p in res[::2]:
        assert len(p.always) == (len(p.rules) + 31) // 32 + 1 and len(p.trig_rules) >= 65517


@pytest.mark.parametrize("kind,limit,message", [("cols", (1 << 20) - 1, "more than 2^20 predicate columns"), ("cmp", 65535, "more than 65535 comparison predicates"),
                                                ("rules", 65519, "more than 65519 rules"), ("caller_rules", 65519, "more than 65519 rules"),
                                                ("caller_routes", 65519, "more than 65519 rules and routes")])
def test_limits_only_a_hand_made_program_reaches_quickly(kind, limit, message):
    assert synthetic(kind, limit)["stage"] == "ok"
    assert synthetic(kind, limit + 1) == {"stage": "plan", "rc": _abi.E_UNSUPPORTED, "rule_index": U32, "message": message}


def test_refusals_keep_their_order_and_an_unknown_variable_is_refused():
    assert synthetic("unknown_var", 2) == {"stage": "plan", "rc": _abi.E_UNSUPPORTED, "rule_index": U32, "message": "comparison atom on an unknown variable"}
    assert synthetic("unknown_var", 1)["stage"] == "ok"


def test_the_case_list_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same harness built with -fsanitize=address,undefined (a stand-alone program: nothing is preloaded), run once over the cases above"""
    exe = tool("tableplan_host_asan", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g")
    cases = [dict(rules=comparison_rules(), lists=LISTS, geo=geoip_entries(GEO_ROWS), flags=f) for f in (0, _abi.OPT_EAGER_CMP)]
    cases += [fuzz_case(7000 + s) for s in range(8)] + [fuzz_case(7100 + s, flags=_abi.OPT_RULE_HITS, routes=True) for s in range(4)]
    cases += [dict(rules=[(f"r{k}", WIDTHS[w][1](k), [B]) for k in range(WIDTHS[w][0] + 1)]) for w in sorted(WIDTHS)]
    cases.append(dict(rules=[("r", "client.remote_port == 1", [B])], lists={f"l{k}": (_abi.LIST_IP, ["10.0.0.0/8"]) for k in range(513)}))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    args = []
    for k, c in enumerate(cases):
        fc, fo = str(tmp_path / f"san{k}.bin"), str(tmp_path / f"san{k}.out")
        write_case(fc, **c)
        args += [fc, fo]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=900, env=env)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and len(r.stdout.strip().splitlines()) == len(cases), (r.returncode, r.stderr[-2000:])
    for kind, n in (("intset0", 129), ("hlen", 9), ("asncmp", 129), ("country", 257), ("cmp", 65536), ("rules", 65520), ("cols", (1 << 20) - 1)):
        r = subprocess.run([exe, "--synthetic", kind, str(n)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
