"""attr_kernel's edge cases without a device (docs/attr_edges.md): every builder assertion of tests/attr_cases.py, the model against the
oracle on every bit of every base batch, and each rule set landing where the cases aim it — read from the two plan dumps
(tests/tableplan_host.cpp: PCMP, PLZY, PLZV, PHLN, cmp_vars, acmp, the class rows; tests/scanplan_host.cpp: n_short, short_field and the
short atoms). A case that does not land where it was aimed fails here."""
import numpy as np
import pytest

import attr_cases as AC
import helpers as H
import test_scanplan_cpu as SP
import test_tableplan_cpu as TP
from oracle import pyoracle
from table_walker import LIT_ATOM_MASK, LIT_NEG

COMPLEMENT = 0x80  # (program.h: kCmpComplement of a comparison atom's code)


# ---------------------------------------------------------------------------------------------------------
# the two plans of a case
# ---------------------------------------------------------------------------------------------------------
def plans(tmp_path, c, flags=AC.OBSERVE, rules=None):
    d = dict(rules=rules or c.observe(), geo=c.geoip(), flags=flags | c.flags)
    (st, p), = TP.run_cases(tmp_path, [d])
    (st2, sc), = SP.run_cases(tmp_path, [d])
    assert st["stage"] == "ok" and st2["stage"] == "ok", (st, st2)
    return p, sc


def rule_literal(p, k):
    """-> (device rule index, column, negated in the source literals, negated in the device literals) of caller rule k, one atom alone"""
    at = np.nonzero(p.rules["public_idx"] == k)[0]
    if len(at) == 0:
        return None  # (a rule the compiler has decided can never match is no device rule)
    r = int(at[0])
    rule = p.rules[r]
    assert rule["lit_cnt"] == 1, (k, int(rule["lit_cnt"]))
    src, dev = int(p.lits[rule["lit_off"]]), int(p.dev_lits[rule["lit_off"]])
    return r, src & LIT_ATOM_MASK, bool(src & LIT_NEG), bool(dev & LIT_NEG)


def entry_of(p, col):
    at = [j for j, (w, _) in enumerate(p.cmp_atoms) if int(w) & 0xFFFFFF == col]
    assert len(at) <= 1
    return at[0] if at else None


def var_index(p, var):
    return 7 + p.hlen_fields.index(5 + AC.H8.index(var)) if isinstance(var, str) else var


def is_small(p):
    return p.set_words <= 4 and p.cc_words <= 2 and p.iu_words[0] <= 1 and p.iu_words[1] <= 1 and p.acmp_words <= 1


def check_comparisons(p, c):
    """every comparison rule against the plan: the constant and operator the device compares with are the model's canonical form (`<` is
    `<= c - 1`, a constant of more than 32 bits folds), the literal's negation and the atom's complement bit together give the source
    operator's, a comparison nothing satisfies has no atom at all"""
    for k, a in enumerate(c.atoms):
        if a[0] != "cmp" or (isinstance(a[1], str) and 5 + AC.H8.index(a[1]) not in p.hlen_fields):  # (the ninth header: a residual rule)
            continue
        if rule_literal(p, k) is None:
            assert c.constant[k] is False, (k, c.exprs[k])
            continue
        r, col, neg, dev_neg = rule_literal(p, k)
        cn = AC.canon(a[2], a[3])
        j = entry_of(p, col)
        if col == 0:  # the compiler's constant TRUE column: the rule is decided at compile time
            assert c.constant[k] == (not neg), (k, c.exprs[k])
        elif cn is None:
            assert j is None and c.constant[k] == neg, (k, c.exprs[k])
        else:
            assert j is not None, (k, c.exprs[k], "no comparison atom")
            code, const = int(p.cmp_atoms[j][0]) >> 24, int(p.cmp_atoms[j][1])
            assert (code & 1, const) == cn[:2], (k, c.exprs[k], code, const, cn)
            assert (code & 0x7F) // 2 == var_index(p, a[1]), (k, c.exprs[k], code)
            assert (dev_neg != bool(code & COMPLEMENT)) == neg == cn[2], (k, c.exprs[k])
    assert p.n_lazy == 0 and p.n_cmp_atoms == len(p.cmp_atoms)


# ---------------------------------------------------------------------------------------------------------
# targets by family
# ---------------------------------------------------------------------------------------------------------
CMP_VARS = {"LEN0": 1, "LEN1": 2, "LEN2": 4, "LEN3": 8, "LEN4": 16, "LENALL": 31, "PORT": 1 << 5, "ASNCOL": 1 << 6, "ASNGEO": 1 << 6, "H1": 1 << 7, "H8": 0xFF << 7}


def default_class_bits(p, c):
    """the default record {0, "XX"} answers `asn < 5`, `<= 0` and `== 0` and not `!= 0`: its class is not class 0, and the bits are set"""
    assert p.geo_default != 0
    row = p.class_rows.reshape(p.n_classes, p.class_words)[p.geo_default]
    base = p.cc_words + p.iu_words[1]
    acmp = p.acmp.tolist()
    for op, const in ((1, 4), (1, 0), (0, 0)):
        j = acmp.index([op, const])
        assert row[base + j // 32] >> (j & 31) & 1, (op, const)
    assert sum(int(x).bit_count() for x in row[base:]) == sum(1 for op, const in acmp if op == 1 or const == 0)  # (asn 0: every `<=` and `== 0`)


def cmp_targets(tmp_path, c):
    p, sc = plans(tmp_path, c)
    check_comparisons(p, c)
    assert p.cmp_vars == CMP_VARS[c.name], bin(p.cmp_vars)
    # (the asn sets hold 33 distinct comparisons: a second comparison word of the class row, the wide instantiation)
    assert sc.n_short == 0 and is_small(p) == (c.name not in ("ASNCOL", "ASNGEO")) and p.acmp_words == (2 if c.name in ("ASNCOL", "ASNGEO") else 0)
    folded = {c.exprs[k]: v for k, v in c.constant.items() if AC.constant_over(c.atoms[k], AC.var_range(c.atoms[k][1])) is not None}
    if c.name == "PORT":
        assert folded["client.remote_port <= 65536"] is True and folded["client.remote_port > 65535"] is False and folded["client.remote_port >= 0"] is True
    if c.name in ("ASNCOL", "ASNGEO"):
        assert folded["client.asn < 4294967296"] is True and folded["client.asn == 4294967296"] is False and folded["client.asn <= -1"] is False
        assert "client.asn <= 4294967294" not in folded and "client.asn >= 2147483648" not in folded
    if c.name.startswith("LEN"):
        assert folded[AC.var_expr(c.atoms[0][1]) + " >= 0"] is True
    if c.name == "ASNGEO":
        # every client.asn comparison is a class-row bit, in the plan's order, and the rows are the records' own answers
        asn = [(int(w) >> 24 & 1, int(k)) for w, k in p.cmp_atoms]
        assert [tuple(x) for x in p.acmp.tolist()] == asn and p.acmp_words == (len(asn) + 31) // 32 == 2 and len(asn) == 34  # (`asn < 5` beside the 33)
        TP.check_classes(p)
        default_class_bits(p, c)
    if c.name == "H1":
        assert p.hlen_fields == [5] and p.n_residual == 0
    if c.name == "H8":
        assert len(p.hlen_fields) == 8 and p.n_residual == 1 and entry_of(p, rule_literal(p, len(c.atoms) - 1)[1]) is None


def polarity_targets(tmp_path, c):
    p, _ = plans(tmp_path, c)
    check_comparisons(p, c)
    for k in range(len(c.atoms)):
        r, col, neg, dev_neg = rule_literal(p, k)
        code = int(p.cmp_atoms[entry_of(p, col)][0]) >> 24
        assert bool(code & COMPLEMENT) == (k in c.complemented) and not dev_neg, (k, c.exprs[k])
        assert not p.always[r >> 5] >> (r & 31) & 1
    e, _ = plans(tmp_path, c, flags=AC.OBSERVE | AC.EAGER)
    check_comparisons(e, c)
    assert not any(int(w) >> 24 & COMPLEMENT for w, _ in e.cmp_atoms) and len(e.cmp_atoms) == len(p.cmp_atoms)
    for k in range(len(c.atoms)):
        r, col, neg, dev_neg = rule_literal(e, k)
        assert dev_neg == neg == (k in c.complemented) == bool(e.always[r >> 5] >> (r & 31) & 1), (k, c.exprs[k])


def chunk_targets(tmp_path, c):
    p, sc = plans(tmp_path, c)
    n = c.n_cmp
    assert len(p.cmp_atoms) == n == p.n_cmp_atoms and p.n_lazy == 0 and sc.n_short == 0
    for k in range(n):  # rule k is PCMP entry k: the probes sit at entries 0, 63, 64, 255, 256 and the last
        assert entry_of(p, rule_literal(p, k)[1]) == k, k
    assert set(c.probes) == {0, 63, 64, 255, 256, n - 1} & set(range(n)) and all(c.M[k].any() and not c.M[k].all() for k in c.probes)
    var_of = lambda j: (int(p.cmp_atoms[j][0]) >> 24 & 0x7F) // 2  # noqa: E731
    op_of = lambda j: int(p.cmp_atoms[j][0]) >> 24 & 1  # noqa: E731
    if n >= 65:
        assert var_of(63) == var_of(64), "no variable straddles the registers and the staged atoms"
    if n >= 257:
        assert var_of(255) == var_of(256), "no variable straddles the staged atoms and the re-read ones"
    if n == 300:  # one (variable, operator) ballot loop on both sides of both edges
        assert (var_of(63), op_of(63)) == (var_of(64), op_of(64)) == (var_of(255), op_of(255)) == (var_of(256), op_of(256)) == (AC.V_PORT, 0)
        assert n > AC.CMP_REGS + AC.CMP_STAGED
    assert p.cmp_vars == (1 << 5 if n == 1 else 1 << 2 | 1 << 5 | 1 << 6)
    assert is_small(p) == (not c.wide) and p.n_bit_atoms == (33 if c.wide else 0) and p.iu_words[0] == (2 if c.wide else 1)
    check_comparisons(p, c)


def geo_targets(tmp_path, c):
    p, _ = plans(tmp_path, c)
    n = c.n_acmp
    assert len(p.acmp) == n and p.acmp_words == (n + 31) // 32 and is_small(p) == (n <= 32)
    for k in range(n):  # rule k is class-row bit k: words 0, 1 and 3, bits 0, 31, 32 and 127
        assert int(p.bit_col[(TP.SRC_ACMP + k // 32) * 32 + (k & 31)]) == rule_literal(p, k)[1], k
    assert rule_literal(p, n)[1:3] == (rule_literal(p, 0)[1], True)  # `!= 0` is the negation of bit 0
    for k in {0, 31, 32, 127} & set(range(n)):
        assert c.M[k].any() and not c.M[k].all()
    TP.check_classes(p)
    default_class_bits(p, c)
    default = [i for i, r in enumerate(c.rows) if r.get("default")]
    assert len(default) >= len(AC.DEFAULT_IPS) and all(c.rows[i]["asn"] == 0 for i in default)
    check_comparisons(p, c)


def lazy_targets(tmp_path, c):
    p, _ = plans(tmp_path, c)
    assert p.lazy_vars == [2, 4] and p.n_lazy == 6 and len(p.lazy_atoms) == 6
    assert [(int(w) >> 24 & 0x7F) // 2 for w, _ in p.cmp_atoms] == [AC.V_PORT] * 3 and p.cmp_vars == 1 << 5
    for w, _ in p.cmp_atoms:  # eager, and no rule's trigger: the token is
        col = int(w) & 0xFFFFFF
        assert p.trig_off[col + 1] == p.trig_off[col]
    e, _ = plans(tmp_path, c, flags=AC.OBSERVE | AC.EAGER)
    assert e.n_lazy == 0 and len(e.cmp_atoms) == 9


def short_atom_of(p, sc, k):
    col = rule_literal(p, k)[1]
    at = [j for j, a in enumerate(sc.short_atoms) if int(a["col"]) == col]
    return (at[0], sc.short_atoms[at[0]]) if at else (None, None)


def short_targets(tmp_path, c):
    p, sc = plans(tmp_path, c)
    mine = [k for k, a in enumerate(c.atoms) if a[1] == c.field]
    other = [k for k, a in enumerate(c.atoms) if a[1] != c.field]
    assert p.n_cmp_atoms == 0 and p.n_bit_atoms == 0
    if c.flags & AC.NO_PREFILTER:
        assert sc.n_short == 0 and sc.short_field == -1 and not any(r["short_lit"] for r in sc.roles)
        return
    # (with two fields that qualify, only the first pass's: the other field is answered by its identity or DFA pass)
    first = min(range(len(sc.groups)), key=lambda g: sc.groups[g]["atom_base"])
    assert sc.short_field == c.field == sc.groups[first]["field"] and sc.n_short == len(mine) == len(sc.short_atoms)
    assert [r["short_lit"] for r in sc.roles].count(1) == 1 and len(sc.groups) == (2 if c.both else 1)
    for j, k in enumerate(mine):
        at, a = short_atom_of(p, sc, k)
        _, _, form, lit = c.atoms[k]
        assert at == j and int(a["len_exact"]) == len(lit) | (0x100 if form in ("eq", "re_eq") else 0) and a["lit"] == lit, (k, c.exprs[k])
    assert sorted({len(c.atoms[k][3]) for k in mine}) == list(range(9))
    for k in other:
        assert short_atom_of(p, sc, k)[0] is None


def short_chunk_targets(tmp_path, c):
    p, sc = plans(tmp_path, c)
    n = c.n_short
    assert sc.n_short == n and sc.short_field == 3 and p.n_cmp_atoms == 0
    for k in range(n):
        at, a = short_atom_of(p, sc, k)
        assert at == k and a["lit"] == c.atoms[k][3], k
    assert c.edges == sorted({0, 63, 64, 127, 128, n - 1} & set(range(n))) and all(int(sc.short_atoms[k]["len_exact"]) & 0xFF == 8 for k in c.edges)
    assert is_small(p) == (not c.wide) and p.n_bit_atoms == (33 if c.wide else 0)
    assert (n > AC.SHORT_REGS + AC.SHORT_STAGED) == (n == 129)


def mixed_targets(tmp_path, c):
    p, sc = plans(tmp_path, c)
    g = c.per_kind
    # pair_stride = n_bit_atoms + n_cmp_atoms + n_short: all three addends, and in a full group every atom files a pair
    assert (p.n_bit_atoms, p.n_cmp_atoms, sc.n_short) == (g, 2 * g, g) and p.n_bit_atoms + p.n_cmp_atoms + sc.n_short == len(c.atoms)
    assert is_small(p) == (not c.wide) and p.iu_words[0] == (2 if c.wide else 1) and sc.short_field == 3
    order = [k for k, _ in c.groups]
    assert order[:3] == ["full A", "full B", "empty"] and order[-2] == "full C"


def turn_targets(tmp_path, c):
    p, sc = plans(tmp_path, c)
    assert (p.n_cmp_atoms, sc.n_short, sc.short_field, p.n_lazy) == (42, 6, 3, 0) and p.cmp_vars == 0x7F and len(c.atoms) <= 48
    # the neighbour property: whatever the stride, the groups a wave meets in consecutive turns are different base groups (and any two
    # different base groups differ, lane by lane, in every prefetched input: asserted by the builder); a rotation that is one group
    # off (the group after next) is a different base group as well
    for cus in range(8, 305):
        stride = cus * AC.ATTR_GROUPS_PER_CU
        kinds = AC.turn_kinds(stride)
        assert len(kinds) == 2 * stride + 96
        assert (kinds[:-stride] != kinds[stride:]).all() and (kinds[:-2 * stride] != kinds[2 * stride:]).all()
        assert set(kinds[:stride].tolist()) == set(range(AC.TURN_K))


FAMILIES = [(AC.CMP_SETS, cmp_targets), (["POL"], polarity_targets), (AC.CHUNK_SETS, chunk_targets), (AC.GEO_SETS, geo_targets), (["Z"], lazy_targets),
            (AC.SHORT_SETS, short_targets), (AC.SHORT_CHUNK_SETS, short_chunk_targets), (["X", "Xw"], mixed_targets), (["T"], turn_targets)]
TARGETS = {name: fn for names, fn in FAMILIES for name in names}
assert sorted(TARGETS) == sorted(AC.ALL_SETS)


# ---------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AC.ALL_SETS)
def test_model_is_the_oracle_on_every_bit(name):
    c = AC.case(name)
    got, _ = H.oracle_matrix(pyoracle.Oracle(c.observe(), None, c.geoip(), flags=AC.NO_GATES), c.batch)
    bad = np.argwhere(got != c.M)
    assert len(bad) == 0, f"{name}: the model and the oracle differ in {len(bad)} of {c.M.size} bits; first: rule {bad[0][0]} ({c.exprs[bad[0][0]]}), request {bad[0][1]}"
    want = pyoracle.Oracle(c.deciding(), None, c.geoip(), flags=AC.NO_GATES).evaluate(c.batch)
    exp = c.expect()
    assert (want["action"] == exp["action"]).all() and (want["rule_idx"] == exp["rule_idx"]).all(), name
    assert 0.25 < c.verified.mean() < 0.4 and not c.verified[-1]
    print(f"set {name}: {len(c.atoms)} atoms, {c.n} requests, {c.M.size} bits, {int(c.M.sum())} set, {len(c.constant)} atoms the model calls constant")


@pytest.mark.parametrize("name", AC.ALL_SETS)
def test_set_lands_where_it_is_aimed(tmp_path, name):
    TARGETS[name](tmp_path, AC.case(name))


def test_values_and_constants_of_the_comparison_sets():
    """the values the issue names are carried by some request, on both sources of the asn"""
    lens = {AC.value(r, 1) for r in AC.case("LEN1").rows}
    assert {0, 1, 2, 3, 255, 256, 4097, 65535, 65536, 65537} <= lens
    assert any(r["f"][1] == "é".encode() for r in AC.case("LEN1").rows)  # two bytes, one character
    for f in range(5):
        assert {0, 1, 255, 256, 4097} <= {AC.value(r, f) for r in AC.case(f"LEN{f}").rows}
    assert {0, 1, 65534, 65535} <= {r["port"] for r in AC.case("PORT").rows}
    for name in ("ASNCOL", "ASNGEO"):
        assert {0, 1, (1 << 31) - 1, 1 << 31, AC.U32 - 1, AC.U32} <= {r["asn"] for r in AC.case(name).rows}
    assert AC.case("ASNCOL").batch.asn is not None and AC.case("ASNGEO").batch.asn is None
    geo = AC.case("ASNGEO")
    assert {(1 << 31) - 1, 1 << 31, AC.U32 - 1, AC.U32} <= {asn for _, asn, _ in geo.geo}
    for k, e in enumerate(geo.exprs):  # the default record answers
        if e in ("client.asn < 5", "client.asn <= 0", "client.asn == 0", "client.asn != 0"):
            assert [bool(geo.M[k, i]) for i, r in enumerate(geo.rows) if r.get("default")] == [e != "client.asn != 0"] * sum(1 for r in geo.rows if r.get("default"))
    h8 = AC.case("H8")
    assert any(not r["hdr"] for r in h8.rows) and any(r["hdr"].get("x-h7") == b"" for r in h8.rows)


def test_canonical_form_of_the_model():
    assert AC.canon("<", 5) == (1, 4, False) and AC.canon(">=", 5) == (1, 4, True) and AC.canon("<", 0) is None and AC.canon("<=", -1) is None
    assert AC.canon("<", AC.U32 + 1) == (1, AC.U32, False) and AC.canon("<=", AC.I64_MAX) == (1, AC.U32, False) and AC.canon("==", AC.U32 + 1) is None
    assert AC.canon(">", AC.U32) == (1, AC.U32, True) and AC.canon("<", 1) == (1, 0, False) and AC.canon("!=", 0) == (0, 0, True)
