"""lscan_kernel at its edges on the device: every list-driven DFA walk -- the R-tier walks behind the confirm tier, the
dense alternative, the candidate lists of a PWAF_OPT_NO_CONFIRM engine, the gap passes that share an owner's list, the identity pass --
through rows staged in LDS, delta records and the L2-resident flat table, in the lockstep loop and in lscan_async. The cases are built
by tests/lscan_cases.py, which proves each one's shape on the host from the two hooks (pwaf_program_flat_image, pwaf_program_list_scans)
before anything is sent; tests/test_lscan_edges_cpu.py makes the same assertions without a device:

  T   tier boundaries: n_hot - 1, n_hot, n_hot + n_delta - 1, n_hot + n_delta, n_states - 1 and more, each left from at byte 0 - 3 of a
      group; record states by exception 1, exception 2, the base row and the field's end; cold steps in last groups of 1 - 3 bytes
  E   (in T) emits from a hot row's, a record state's and a cold row's EMIT cell, an emit list, an atom twice, 3 and 4 atoms, end atoms,
      an atom emitted at the start state (the method's identity pass), the scalar-mode rule
  TL  T over set L: literals alone, whose records hold exception classes a printable byte has
  W   fields of 0 - 49 bytes at every arena offset mod 16, the deciding byte last; the arena's last request
  P   candidate lists of 0 - 513 of 4 096 requests (both sides of 8 * n_l >= n: the lockstep loop and lscan_async); FULL waves of
      lscan_async (a batch tiled past 32 entries per wave of the launch: lscan_cases.entries_per_item) with 1, 31, 32, 33 and 64 lanes
      blocked in the same iteration; a launch of several passes with an empty list between two that are not and a single entry
  S   need bits set and clear on the owner's list; two batches in turn, four turns; SG: six gap passes on one owner, records of the
      first batch where the passes do not walk in the second; SH: two gap passes with factors of their own on one owner, the need bit
      of exactly one, of both, of none; SO: the same passes with lists of their own (enqueues, visited bitmaps)
  TQ  T's targets over the passes of three fields in one launch; D, DL, DG, DH, DO: every set's dense alternative
  D   more than half of the chunks flagged: dense_mode 1 and 3 under the clamped n_hot

Every case: (action, rule_idx) and the four action counters against pyoracle.Oracle for the engine as built, without the confirm tier,
without the dense switch and tuned; the whole hit matrix of a PWAF_OPT_RULE_HITS engine over the bare predicates against the
oracle's. The engine without prefilters (scan_kernel) is the cross-check: a case that fails as built and passes there is a list-scan
bug, not a DFA bug. Each test asserts from the kernel times that the lscan_x<k> launches the hook predicted ran."""
import numpy as np
import pytest

import helpers as H
import lscan_cases as LC
from oracle import pyoracle
from pingoo_amd import _abi
from pingoo_amd.engine import RuleEngine

pytestmark = pytest.mark.gpu
NC, ND, HITS, NP = _abi.OPT_NO_CONFIRM, _abi.OPT_NO_DENSE_SWITCH, _abi.OPT_RULE_HITS, _abi.OPT_NO_PREFILTER
SETS = {"M": LC.set_m, "L": LC.set_l, "G": LC.set_g, "H": lambda: LC.set_h(True), "O": lambda: LC.set_h(False), "Q": LC.set_q}
SET_OF = {"T": "M", "TL": "L", "W": "M", "S": "M", "SG": "G", "SH": "H", "SO": "O", "lists": "Q", "TQ": "Q", "D": "M", "DL": "L", "DG": "G", "DH": "H", "DO": "O"}


def expected_launches(prog):
    """the lscan_x<k> entries of one batch, in order, from the hook's descriptors"""
    out, seen = [], set()
    for d in prog.list_scans():
        if (d["phase"], d["launch"]) not in seen:
            seen.add((d["phase"], d["launch"]))
            out.append(f"lscan_x{d['launch_count']}")
    return out


class Engines:
    """One rule set: the module-scoped legs and the oracles; references are computed once per batch and shared."""

    def __init__(self, name):
        self.name, self.rs = name, SETS[name]()
        rs = self.rs
        self.oracle = pyoracle.Oracle(rs.verdict_rules, {})
        self.hit_oracle = pyoracle.Oracle(rs.bare_rules, {})
        self.legs, self.refs = [], {}
        for label, flags in (("as built", 0), ("no confirm tier", NC), ("no dense switch", ND), ("rule hits", HITS), ("no prefilter", NP)):
            eng = RuleEngine(rs.rules(flags), {}, flags=flags, **rs.opts)
            # the engine's own program answers the descriptors the case was proved for (the same planner over the same tables; what the
            # engine really launched shows in the lscan_x<k> entries checked below)
            assert eng.program.list_scans() == rs.program(flags).list_scans(), (name, label)
            self.legs.append((label, flags, eng, expected_launches(rs.program(flags))))

    def reference(self, batch, hits=False):
        key = (id(batch), hits)
        if key not in self.refs:
            self.refs[key] = (batch,) + (H.oracle_matrix(self.hit_oracle, batch) if hits else (self.oracle.evaluate(batch),))
        return self.refs[key][1:]

    def check_one(self, what, flags, eng, launches, batch):
        eng.set_profiling(1)
        if flags & HITS:
            m, hit_want = self.reference(batch, hits=True)
            got, hits, rule_hits, counts = eng.evaluate_batch_hits(batch, with_counts=True)
            names = [k[0] for k in eng.kernel_times()]
            eng.set_profiling(0)
            H.assert_verdicts_equal(got, hit_want, batch, what)
            assert counts.tolist() == np.bincount(hit_want["action"], minlength=4).tolist(), what
            H.assert_hits(what, hits, rule_hits, m)
        else:
            (want,) = self.reference(batch)
            got, counts = eng.evaluate_batch(batch, with_counts=True)
            names = [k[0] for k in eng.kernel_times()]
            eng.set_profiling(0)
            H.assert_verdicts_equal(got, want, batch, what)
            assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist(), what
        ran = [x for x in names if x.startswith("lscan_x")]
        # (evaluate_batch_hits fetches a hit list that outgrew its first capacity again, once: the batch then ran twice)
        assert ran == launches or (flags & HITS and ran == launches * 2), (what, names)

    def check(self, case, only=None):
        for turn in range(case.turns):
            for label, batch in case.batches:
                for leg, flags, eng, launches in self.legs:
                    if only is None or leg in only:
                        self.check_one(f"case {case.name}: {label}, turn {turn}, {leg}", flags, eng, launches, batch)

    def close(self):
        for _, _, eng, _ in self.legs:
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


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_case_on_every_leg(engines, name):
    case = LC.CASES[name]()
    e = engines(SET_OF[name])
    e.check(case)
    want = e.reference(case.batches[0][1])[0]
    assert len(set(want["action"].tolist())) >= 2, f"case {name}: the oracle's verdicts are all alike"


@pytest.mark.parametrize("n_list", LC.P_LENGTHS)
def test_candidate_lists_on_both_sides_of_an_eighth_of_the_batch(engines, n_list):
    """the same pass in the lockstep loop (n_list < 512 of 4 096) and in lscan_async (from 512 on): without the confirm tier the list is
    the prefilter's candidate list (its length proved by the numpy model of the filter), as built it is the confirm tier's walk list"""
    case = LC.case_p(n_list)
    assert case.measured["n_list"] == n_list and case.measured["long_list"] == (8 * n_list >= LC.N_P)
    engines("M").check(case, only=("as built", "no confirm tier", "rule hits"))


@pytest.mark.parametrize("blocked", LC.WAVE_COUNTS)
def test_full_waves_of_the_asynchronous_loop_with_blocked_lanes(engines, blocked):
    """every request a candidate of the engine without confirm tier, the base batch of 64 tiled until lscan_plan_kernel packs 64 list
    entries into a wave ON THIS DEVICE (the builder proves it from the launch shape and the compute units); wave w then holds requests
    64 w .. 64 w + 63, of which `blocked` stand in a cold state in the same iteration: below, at and above the 32 lanes from which the
    slow iteration is taken at once, and all 64 (nobody else can move). Expected verdicts: the oracle's on the base batch, tiled."""
    e = engines("M")
    (nc,) = [eng for leg, _, eng, _ in e.legs if leg == "no confirm tier"]
    case, times = LC.case_p_waves(blocked, nc.compute_units())  # (the count the engine itself sizes the launch's grid with)
    base = case.batches[0][1]
    (base_want,) = e.reference(base)
    batch, want = base.tile(times), np.tile(base_want, times)
    assert batch.n == case.measured["n"] and case.measured["epi"] == 64 and len(set(base_want["action"].tolist())) >= 2
    for leg, flags, eng, launches in e.legs:
        if leg in ("no confirm tier", "no prefilter"):
            eng.set_profiling(1)
            got, counts = eng.evaluate_batch(batch, with_counts=True)
            names = [k[0] for k in eng.kernel_times()]
            eng.set_profiling(0)
            what = f"case {case.name}: {batch.n} requests, {leg}"
            H.assert_verdicts_equal(got, want, None, what)
            assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist(), what
            assert [x for x in names if x.startswith("lscan_x")] == launches, (what, names)


def test_a_tuned_engine_with_other_states_hot(engines):
    """tuned on requests of case T (walks deep into states that are cold as built) among benign ones: the tables are rebuilt with the
    sample's most visited states first. The shapes are re-proved from a host program tuned on the same sample -- the engine's own program answers
    the same descriptors and images -- before the cases are sent."""
    e = engines("M")
    rs = e.rs
    sample, host, d, m = LC.tuned_m()
    eng = RuleEngine(rs.verdict_rules, {}, **rs.opts)
    try:
        eng.tune(sample)
        assert eng.program.list_scans() == host.list_scans()
        assert eng.program.flat_image(d["pass"], 1) == host.flat_image(d["pass"], 1)
        t = LC.case_t("M").batches[0][1]
        row = LC.Coverage(rs, 0, t, prog=host).row(phase=0, tier=1)
        LC.assert_tiers_at_every_position(row, "tuned, R tier")
        launches = expected_launches(host)
        for name in ("T", "W", "S", "D"):
            c = LC.CASES[name]()
            for label, batch in c.batches:
                # re-proved from the tuned program before sending: the R tier (the dense alternative, for D) walks requests of the batch through
                # hot AND cold rows of the tuned table
                cov = LC.Coverage(rs, 0, batch, dense=name == "D", prog=host, only=None if name in ("T", "W") else range(0, batch.n, 4))
                r = cov.row(phase=0, tier=0, dense_mode=1) if name == "D" else cov.row(phase=0, tier=1)
                assert r[2] > 0 and any(r[3].get((LC.HOT, p), 0) for p in range(4)), (name, label)
                assert name in ("W", "S") or any(r[3].get((LC.COLD, p), 0) for p in range(4)), (name, label)
                e.check_one(f"case {name}: {label}, tuned", 0, eng, launches, batch)
    finally:
        eng.close()
