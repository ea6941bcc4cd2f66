"""resolve_kernel and confirm_kernel at their edges on the device (the chain filter_kernel -> resolve_kernel ->
confirm_plan_kernel -> confirm_kernel -> walk lists decides every literal predicate of a filtered pass). The cases are built by
tests/confirm_cases.py, which proves each one's shape with a numpy model of the filter and pwaf_program_confirm_shape before anything is
sent (tests/test_confirm_edges_cpu.py makes the same assertions without a device):

  A  comparison tables read from global memory (4 000 literals: confirm_entry<1>)     F  the record reset's bound of 48 requests
  B  more than four windows completing in one chunk; the arena's first / last chunk  G  stale records: two batches in turn, four turns
  C  2 - 16 requests in one chunk, hits in the first / a middle / the last; C2: at     H  confirm_entry: lengths 2 - 64 (65: a walk factor),
     stride 2                                                                            anchors, classes at bytes 3 and 19, (?i), near misses
  D  slabs with 0, 1, 64, 65, 127, 128, 129, 200 flagged chunks (the sparse switch)   I  forty entries in one bin
  E  the chunk's owner 4 095 / 4 096 / 4 097 requests into the slab                   J  the walk queue of a workgroup running full

Every case: (action, rule_idx) and the four action counters against pyoracle.Oracle for the engine as built, with stride 2 forced,
without the dense switch and with PWAF_RESOLVE_PARTS = 1 and 4; the whole hit matrix of a PWAF_OPT_RULE_HITS engine over the bare
predicates against the oracle's (the leg that sees every atom of every request: a stale or misplaced atom shows there). The engines
without the confirm tier and without prefilters are cross-checks that tell a confirm bug from a filter or DFA bug.

Set A is the slow one: an engine of its 4 000 rules takes two to three seconds to create, whatever its flags. Its module-scoped fixture is
the engine as built (with resolve parts 1 and 4); every other leg of A creates its engine in a test of its own: the hit matrix of a
PWAF_OPT_RULE_HITS engine (a wrong atom behind the deciding rule shows only there), stride 2 (162 710 entries, in global memory too), no
dense switch, and the two cross-checks (a case that fails as built and passes without prefilters is a bug of the global-table
comparison, not of the 4 000-literal DFA)."""
import numpy as np
import pytest

import confirm_cases as CC
import helpers as H
from oracle import pyoracle
from pingoo_amd import _abi
from pingoo_amd.engine import PwafError, RuleEngine

pytestmark = pytest.mark.gpu
HITS = _abi.OPT_RULE_HITS
SETS = {"S": (CC.set_s, ["B", "C", "D", "E", "F", "G"]), "S2": (CC.set_s2, ["C2"]), "H": (CC.set_h, ["H", "I"]), "A": (CC.set_a, ["A"])}
SET_OF = {case: s for s, (_, cases) in SETS.items() for case in cases}


class Engines:
    """One rule set: the module-scoped legs and the oracles; references are computed once per batch and shared."""

    def __init__(self, name):
        self.name = name
        self.rs = SETS[name][0]()
        self.oracle = pyoracle.Oracle(self.rs.verdict_rules, {})
        self.legs, self.hit_legs, self.refs = [], [], {}
        if name == "A":
            plan = [("as built", 0)]
        else:
            plan = [("as built", 0), ("stride 2", _abi.OPT_FILTER_STRIDE2), ("no dense switch", _abi.OPT_NO_DENSE_SWITCH), ("rule hits", HITS)]
            if name == "S2":
                plan.append(("rule hits, stride 2", HITS | _abi.OPT_FILTER_STRIDE2))
            self.hit_oracle = pyoracle.Oracle(self.rs.bare_rules, {})
        for label, flags in plan:
            eng = RuleEngine(self.rs.rules(flags), {}, flags=flags)
            # the engine's own program has the pass under test, in the shape the case was proved for
            gi, g = self.rs.pass_of(flags)
            assert eng.program.confirm_shape(gi) == self.rs.confirm_shape(flags), (name, label)
            (self.hit_legs if flags & HITS else self.legs).append((label, eng))

    def reference(self, batch):
        key = id(batch)
        if key not in self.refs:
            want = self.oracle.evaluate(batch)
            self.refs[key] = (batch, want, H.oracle_matrix(self.hit_oracle, batch) if self.hit_legs else None)
        return self.refs[key][1:]

    def check_verdicts(self, what, eng, batch, want):
        got, counts = eng.evaluate_batch(batch, with_counts=True)
        H.assert_verdicts_equal(got, want, batch, what)
        assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist(), what

    def check(self, case, only=None):
        for turn in range(case.turns):
            for label, batch in case.batches:
                want, hit_ref = self.reference(batch)
                for leg, eng in self.legs:
                    if only is None or leg in only:
                        self.check_verdicts(f"case {case.name}: {label}, turn {turn}, {leg}", eng, batch, want)
                for leg, eng in self.hit_legs:
                    if only is None or leg in only:
                        m, hit_want = hit_ref
                        what = f"case {case.name}: {label}, turn {turn}, {leg}"
                        got, hits, rule_hits, counts = eng.evaluate_batch_hits(batch, with_counts=True)
                        H.assert_verdicts_equal(got, hit_want, batch, what)
                        assert counts.tolist() == np.bincount(hit_want["action"], minlength=4).tolist(), what
                        H.assert_hits(what, hits, rule_hits, m)

    def close(self):
        for _, eng in self.legs + self.hit_legs:
            eng.close()


_engines = {}


@pytest.fixture(scope="module")
def engines():
    """the sets' engines, each built when its first case asks for it and kept for the module"""
    def get(name):
        if name not in _engines:
            _engines[name] = Engines(name)
        return _engines[name]

    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_case_on_every_leg(engines, name):
    case = CC.CASES[name]()
    e = engines(SET_OF[name])
    e.check(case)
    want, _ = e.reference(case.batches[0][1])
    assert len(set(want["action"].tolist())) >= 2, f"case {name}: the oracle's verdicts are all alike"


@pytest.mark.parametrize("parts", ["1", "4"])
@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_case_with_one_wave_and_four_waves_per_slab(engines, name, parts, monkeypatch):
    """resolve_kernel<1> and <4> forced (PWAF_RESOLVE_PARTS is read per launch): the chunk-driven path is taken by part 0 alone, its
    fall-backs walk the whole slab whatever the parts"""
    monkeypatch.setenv("PWAF_RESOLVE_PARTS", parts)
    case = CC.CASES[name]()
    e = engines(SET_OF[name])
    one_turn = CC.Case(f"{name} (resolve parts {parts})", case.rs, case.batches, case.measured, turns=min(case.turns, 2))
    e.check(one_turn, only=("as built", "rule hits"))


@pytest.mark.parametrize("set_name", ["S", "S2", "H"])
def test_cross_checks_without_the_confirm_tier_and_without_prefilters(engines, set_name):
    """the same cases through an engine that walks every flagged request through the pass's full DFA (PWAF_OPT_NO_CONFIRM: resolve_kernel
    marks candidates, nothing is confirmed) and through one that walks every request (PWAF_OPT_NO_PREFILTER): a case that fails above and
    passes here is a bug of the confirm tier, one that fails with NO_CONFIRM too is the filter's or the resolve step's"""
    e = engines(set_name)
    for label, flags in (("no confirm tier", _abi.OPT_NO_CONFIRM), ("no prefilter", _abi.OPT_NO_PREFILTER)):
        eng = RuleEngine(e.rs.verdict_rules, {}, flags=flags)
        try:
            for name in SETS[set_name][1]:
                case = CC.CASES[name]()
                for blabel, batch in case.batches:
                    e.check_verdicts(f"case {name}: {blabel}, {label}", eng, batch, e.reference(batch)[0])
        finally:
            eng.close()


def confirm_shape_of(eng):
    """the shape of the engine's largest confirm tier, the url pass (set A: finding it through CC.RuleSet would compile the 4 000 rules again)"""
    shapes = []
    for gi in range(eng.program.stats()["n_dfa_groups"]):
        try:
            shapes.append(eng.program.confirm_shape(gi))
        except PwafError:
            pass
    top = max(shapes, key=lambda cs: cs["entries"])
    assert top["entries"] >= CC.A_RULES, top
    return top


def test_case_a_as_a_hit_matrix(engines):
    """A through a PWAF_OPT_RULE_HITS engine: every (rule, request) bit. The reference for the 16 M bits is the predicate's meaning, a
    substring search (4 000 x 4 080 oracle calls would take a minute); every 47th request's column of it -- hits, last-byte misses
    and cut literals, at all offsets -- is checked against the oracle's own."""
    e = engines("A")
    rs, (label, batch) = e.rs, CC.CASES["A"]().batches[0]
    want, _ = e.reference(batch)
    urls = [bytes(batch.field_bytes(rs.field_id, i)) for i in range(batch.n)]
    m = np.array([[lit.encode() in u for u in urls] for lit in rs.lits], dtype=bool)
    sample = range(0, batch.n, 47)
    by_oracle, _ = H.oracle_matrix(e.oracle, batch, only=sample)
    assert (by_oracle[:, sample] == m[:, sample]).all(), "case A: the substring reference is not the oracle's"
    assert 0 < m[:, sample].any(axis=0).sum() < len(sample), "case A: the sample holds no hit, or nothing else"
    eng = RuleEngine(rs.rules(HITS), {}, flags=HITS)
    try:
        assert confirm_shape_of(eng)["in_lds"] == 0
        what = "case A: rule hits"
        got, hits, rule_hits, counts = eng.evaluate_batch_hits(batch, with_counts=True)
        H.assert_verdicts_equal(got, want, batch, what)
        assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist(), what
        H.assert_hits(what, hits, rule_hits, m)
    finally:
        eng.close()


A_LEGS = {"stride 2": _abi.OPT_FILTER_STRIDE2, "no dense switch": _abi.OPT_NO_DENSE_SWITCH, "no confirm tier": _abi.OPT_NO_CONFIRM, "no prefilter": _abi.OPT_NO_PREFILTER}


@pytest.mark.parametrize("leg", sorted(A_LEGS))
def test_case_a_on_its_other_legs(engines, leg):
    """A with stride 2 forced and without the dense switch (the comparison tables still in global memory), and through the engines that
    walk every flagged request / every request through the pass's DFA: what tells a bug of the global-table comparison from one of
    the filter or of the 4 000-literal DFA"""
    e = engines("A")
    label, batch = CC.CASES["A"]().batches[0]
    eng = RuleEngine(e.rs.verdict_rules, {}, flags=A_LEGS[leg])
    try:
        if leg in ("stride 2", "no dense switch"):
            assert confirm_shape_of(eng)["in_lds"] == 0
        e.check_verdicts(f"case A: {leg}", eng, batch, e.reference(batch)[0])
    finally:
        eng.close()


def test_the_walk_queue_of_a_workgroup_runs_full():
    """J: more than 2 * 1 024 * blocks pairs of one pass, every one a walk request of its own: each workgroup of confirm_kernel's grid
    (2 per compute unit) parks more than kConfirmQueue requests in one run of the pass, the rest is appended directly. The expected
    verdicts are the oracle's on the four base requests, tiled; the engine without prefilters is the cross-check."""
    import torch

    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    case, times = CC.case_j(n_cus)
    rs, base = case.rs, case.batches[0][1]
    base_want = pyoracle.Oracle(rs.verdict_rules, {}).evaluate(base)
    assert base_want["action"].tolist() == [1, 0, 1, 0]
    batch, want = base.tile(times), np.tile(base_want, times)
    assert batch.n * 1 > 2 * CC.QUEUE * 2 * n_cus  # (one pair per request: the model, case_j)
    hist = np.bincount(want["action"], minlength=4).tolist()
    for label, flags in (("as built", 0), ("no prefilter", _abi.OPT_NO_PREFILTER)):
        eng = RuleEngine(rs.verdict_rules, {}, flags=flags)
        try:
            if not flags:
                assert eng.program.confirm_shape(rs.pass_of()[0])["has_walk"] == 1
            for n in (base, batch):
                got, counts = eng.evaluate_batch(n, with_counts=True)
                w = want[:n.n]
                H.assert_verdicts_equal(got, w, None, f"case J: {n.n} requests, {label}")
                assert counts.tolist() == np.bincount(w["action"], minlength=4).tolist(), f"case J: {n.n} requests, {label}"
        finally:
            eng.close()
    assert hist[1] == 2 * times
