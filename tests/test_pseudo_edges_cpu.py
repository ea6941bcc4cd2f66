"""The pseudo passes' edge cases without a device (docs/pseudo_edges.md): every builder assertion of tests/pseudo_cases.py, the model
against the oracle on every bit of every base batch, and each rule set landing where the cases need it — read from the compiled
program's dump (table_walker.Tables: the FCMP and RSDL sections) and its warnings."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import pseudo_cases as PC
from oracle import pyoracle
from pingoo_amd import _abi
from pingoo_amd.engine import CompiledProgram
from table_walker import Tables

SETS = ("F32", "F33", "F9", "R74", "RE", "M")
# set -> (field atoms, distinct fields, residual rules)
LANDS = {"F32": (32, 8, 0), "F33": (32, 8, 1), "F9": (31, 8, 1), "R74": (0, 0, 74), "RE": (0, 0, 78), "M": (32, 8, 20)}
# in reversed rule order F9's ninth field is met first: the user agent and the method, met last and together, would be the 8th and 9th, and
# their four remaining predicates are lowered beside `<` (F33 reversed refuses its last predicate instead: still 32 + 1)
LANDS_REVERSED = dict(LANDS, F9=(27, 7, 5))


def assert_model_is_the_oracle(what, rules, batch, m):
    got, _ = H.oracle_matrix(pyoracle.Oracle(rules, flags=PC.NO_GATES), batch)
    bad = np.argwhere(got != m)
    assert len(bad) == 0, f"{what}: the model and the oracle differ in {len(bad)} of {m.size} bits; first: rule {bad[0][0]} ({rules[bad[0][0]][1]}), request {bad[0][1]}"


def oracle_errors(rules, batch):
    """per rule: the requests for which the oracle's evaluation ends in an execution error"""
    o = pyoracle.Oracle(rules, flags=PC.NO_GATES)
    st = batch.as_struct(o.header_names)
    fn, ref = pyoracle.lib().pwaf_oracle_execute_rule, C.byref(st)
    return [sum(fn(o._h, k, ref, i) == 3 for i in range(batch.n)) for k in range(len(rules))]


@pytest.mark.parametrize("name", SETS)
def test_targets_and_the_model_against_the_oracle(name):
    c = PC.case(name)
    PC.assert_targets(c)
    assert_model_is_the_oracle(name, c.observe(), c.batch, c.M)
    assert oracle_errors(c.observe(), c.batch) == c.errors
    # the deciding form, both rule orders: the oracle's verdicts are the first rule of the model's matrix that takes effect
    for reverse in (False, True):
        want = pyoracle.Oracle(c.deciding(reverse), flags=PC.NO_GATES).evaluate(c.batch)
        exp = c.expect(reverse)
        assert (want["action"] == exp["action"]).all() and (want["rule_idx"] == exp["rule_idx"]).all(), (name, reverse)
    print(f"set {name}: {c.n} requests, {c.M.size} bits, {int(c.M.sum())} set; true atoms per request 0 ... {int(c.M.sum(axis=0).max())}")


@pytest.mark.parametrize("name", SETS)
def test_set_lands_where_the_cases_need_it(name):
    c = PC.case(name)
    for rules, lands in ((c.observe(), LANDS), (c.deciding(), LANDS), (c.deciding(reverse=True), LANDS_REVERSED)):
        n_fcmp, n_fields, n_res = lands[name]
        flags = PC.OBSERVE if rules[0][2] == [] else PC.NO_GATES
        p = CompiledProgram(rules, flags=flags)
        t = Tables(p.dump())
        fcmp = getattr(t, "fcmp", [])
        assert len(fcmp) == n_fcmp and len({int(d[k]) for d in fcmp for k in ("a", "b")}) == n_fields, (name, len(fcmp))
        assert getattr(t, "n_residual", 0) == n_res and sum("residual interpreter" in w for w in p.warnings()) == n_res, (name, p.warnings()[:3])
        assert p.unsupported_rules(len(rules)) == [] and p.stats()["n_rules"] >= len(rules)
        if name == "M":
            assert p.stats()["n_dfa_groups"] >= 1
        if name in ("F33", "F9") and rules is c.observe():
            # the rule the field pass refuses is the last one, and it alone
            lowered = [w for w in p.warnings() if "residual interpreter" in w]
            assert len(lowered) == 1 and f"r{len(rules) - 1}" in lowered[0], lowered


def test_error_batches():
    for n in PC.ERR_SIZES:
        batch, m, errors = PC.error_batch(n)
        rules = PC.case("RE").observe()
        assert batch.n == n and (n not in PC.ERR_ONLY_LAST or [int(e) for k, e in enumerate(errors) if k in PC.RE_AT] == [1] * 5)
        if n in PC.ERR_ONLY_LAST:
            assert int(batch.asn[-1]) % 3 == 1 and not (batch.asn[:-1] % 3 == 1).any()
        assert_model_is_the_oracle(f"error batch of {n}", rules, batch, m)
        assert oracle_errors(rules, batch) == errors
    assert {n % 64 for n in PC.ERR_ONLY_LAST} == {n % 64 for n in PC.ERR_SIZES} == {0, 1, 63}


@pytest.mark.parametrize("name", ["F32", "R8"])
def test_second_round_base(name):
    exprs, batch, m, idx = PC.second_round(name)
    assert len(idx) == PC.ROUND + 257 and batch.n == PC.BIG_BASE
    assert_model_is_the_oracle(f"second round, {name}", [(f"r{k}", e, []) for k, e in enumerate(exprs)], batch, m)
    p = CompiledProgram([(f"r{k}", e, []) for k, e in enumerate(exprs)], flags=PC.OBSERVE)
    t = Tables(p.dump())
    assert (len(getattr(t, "fcmp", [])), getattr(t, "n_residual", 0)) == ((32, 0) if name == "F32" else (0, 8))


@pytest.mark.parametrize("name", ["F32", "RE"])
def test_pool_cases(name):
    exprs, req, col, n, errors = PC.pool_case(name)
    from pingoo_amd import RequestBatch

    one = RequestBatch.from_requests([req])
    rules = [(f"r{k}", e, []) for k, e in enumerate(exprs)]
    assert_model_is_the_oracle(f"pool, {name}", rules, one, col[:, None])
    assert [e * n for e in oracle_errors(rules, one)] == errors
    assert n * int(col.sum()) > max(PC.POOL_MIN, 8 * n)  # a chained request takes one pool entry per true atom


def test_packed_masks():
    """the large batches' comparison states what helpers.assert_hits states"""
    rng = np.random.default_rng(5)
    m = rng.random((5, 131)) < 0.3
    masks = PC.packed(m)
    hits = np.array([(k, g, masks[k, g]) for k in range(5) for g in range(3) if masks[k, g]], dtype=[("rule_idx", "<u4"), ("group", "<u4"), ("mask", "<u8")])
    PC.assert_hits_packed("ok", hits, m.sum(axis=1), masks, m.sum(axis=1))
    H.assert_hits("ok", hits, m.sum(axis=1), m)
    flipped = hits.copy()
    flipped["mask"][3] ^= np.uint64(1 << 17)
    with pytest.raises(AssertionError, match="1 .rule, request. bits differ"):
        PC.assert_hits_packed("flipped", flipped, m.sum(axis=1), masks, m.sum(axis=1))
    with pytest.raises(AssertionError, match="twice"):
        PC.assert_hits_packed("twice", np.concatenate([hits, hits[:1]]), m.sum(axis=1), masks, m.sum(axis=1))
