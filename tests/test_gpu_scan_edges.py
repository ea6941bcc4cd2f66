"""scan_kernel<CH, WIDE> at its edges on the device (csrc/scan.hip: scan_body): the DFA walk over EVERY request of a pass -- every pass
of a PWAF_OPT_NO_PREFILTER engine, every pass without a usable prefilter -- which three other edge suites use as their cross-check. The
cases are built by tests/scan_cases.py, which proves each one's shape on the host from the scan-plan harness before anything is sent;
tests/test_scan_edges_cpu.py makes the same assertions without a device and walks every request through the streaming table:

  W1 W2 W4  fields of 0 .. 2 * 16 * CH + 17 bytes at every arena offset mod 16, the deciding byte last; the same fields ending in X in front
            of a Q (the next field's first byte, the arena's slack) under contains("XQ"); CH = 1, 2, 4 by the tuning sample
  B         1, 15, 16, 17, 1 024, 1 040, 4 096, 4 097 requests, matches on both sides of every share boundary; runs of 63 - 200 empty and
            one-byte fields (block switches in consecutive iterations); a 40 KiB field at lane 0 and lane 63 of a share's first take;
            4 096 * CUs + 777 requests, beyond the cap of one workgroup per CU
  T         plain hot, emitting hot and cold rows entered at byte 0 - 3 of a group; cold to hot, cold to cold; fields ending 1 - 3 bytes into
            a group on every tier; the END cell of a cold row; two lanes of one take in different tiers in the same group
  E         an emit list, an atom twice, records of 1 - 10 atoms, single END atoms and END lists with the record full, start_emit
  U         scalar mode: lead bytes at chunk bytes 13 - 15, truncated sequences, stray continuation bytes, overlong forms, a lone lane
  X         more than 127 byte classes (the 32-bit class table) over W1's lengths
  G         the url's plain pass feeds six gap passes from records of one atom, of two, from overflowed ones; hits that gate nothing
  V         several passes in one batch, two batches in turn, a view whose offsets begin above zero, the device-resident entry point

Every case runs on five legs -- PWAF_OPT_NO_PREFILTER as created, with the case's small lds_table_budget, tuned on the case's sample,
PWAF_OPT_RULE_HITS over the bare predicates, and the naturally unfilterable rule with flags 0 -- against pyoracle.Oracle: (action,
rule_idx) and the four action counters exactly, on the hits leg the whole hit matrix. Each check asserts from the kernel times that the
scan_<field>_g<k> launches the plan predicts ran (set G: and the gap passes' lscan_x6): a planner change that routes a pass elsewhere
fails here instead of testing another kernel. A tuned engine is cached under its sample's digest and must show, through
pwaf_program_flat_image, the tables the harness builds from that very sample (scan_cases.assert_tuned_as_planned)."""
import numpy as np
import pytest

import helpers as H
import scan_cases as SC
from oracle import pyoracle
from pingoo_amd.engine import DeviceBatch, RuleEngine

pytestmark = pytest.mark.gpu
LEGS = ("as built", "small budget", "tuned", "rule hits", "natural")


class Engines:
    """One rule set: the module-scoped legs and the oracles; references are computed once per batch and shared."""

    def __init__(self, name):
        self.name, self.rs = name, SC.SETS[name]()
        rs = self.rs
        self.oracles = {"verdict": pyoracle.Oracle(rs.verdict_rules, {}), "hits": pyoracle.Oracle(rs.bare_rules, {}), "natural": pyoracle.Oracle(rs.natural_rules, {})}
        self.engines, self.refs = {}, {}

    def engine(self, leg, sample=None):
        """-> (engine, the harness's plan for it); a tuned leg is one engine per sample, by the sample's key (scan_cases.sample_of: a digest
        of its values, so that no two different samples meet in one engine)"""
        rs = self.rs
        key = (leg, sample[0] if sample else None)
        if key not in self.engines:
            rules, flags, budget = rs.leg(leg)
            eng = RuleEngine(rules, {}, flags=flags, lds_table_budget=budget, max_table_bytes=rs.table_bytes)
            # the engine compiled the program the case was proved for (the streaming tables follow from it by the same build_device_group)
            assert rs.scan(leg).blob.startswith(eng.program.dump()), (self.name, leg)
            sc = rs.scan(leg, sample)
            if sample is not None:
                eng.tune(sample[1])
                SC.assert_tuned_as_planned(eng.program, sc, rs.scan(leg), (self.name, leg, sample[0]))
            self.engines[key] = (eng, sc, sample[1] if sample else None)
        eng, sc, tuned_on = self.engines[key]
        assert (tuned_on is None) == (sample is None) and (sample is None or SC.same_sample((None, tuned_on), sample)), (self.name, leg, "the engine was tuned on another sample")
        return eng, sc

    def reference(self, batch, kind):
        key = (id(batch), kind)
        if key not in self.refs:
            self.refs[key] = (batch,) + (H.oracle_matrix(self.oracles[kind], batch) if kind == "hits" else (self.oracles[kind].evaluate(batch),))
        return self.refs[key][1:]

    def check_one(self, what, leg, batch, sample=None, rows=None):
        """rows: (lo, hi) when `batch` is a view of the requests [lo, hi) of the batch the reference is computed for"""
        eng, sc = self.engine(leg, sample if leg in ("tuned", "natural tuned") else None)
        full = batch if rows is None else rows[2]
        cut = (lambda a: a) if rows is None else (lambda a: a[rows[0]:rows[1]])
        eng.set_profiling(1)
        if leg == "rule hits":
            m, want = self.reference(full, "hits")
            got, hits, rule_hits, counts = eng.evaluate_batch_hits(batch, with_counts=True)
            names = [k[0] for k in eng.kernel_times()]
            eng.set_profiling(0)
            H.assert_verdicts_equal(got, cut(want), batch, what)
            assert counts.tolist() == np.bincount(cut(want)["action"], minlength=4).tolist(), what
            H.assert_hits(what, hits, rule_hits, m if rows is None else m[:, rows[0]:rows[1]])
        else:
            (want,) = self.reference(full, "natural" if leg.startswith("natural") else "verdict")
            got, counts = eng.evaluate_batch(batch, with_counts=True)
            names = [k[0] for k in eng.kernel_times()]
            eng.set_profiling(0)
            H.assert_verdicts_equal(got, cut(want), batch, what)
            assert counts.tolist() == np.bincount(cut(want)["action"], minlength=4).tolist(), what
        self.assert_launches(what, leg, sc, names)

    def assert_launches(self, what, leg, sc, names):
        want = SC.scan_names(sc)
        assert f"scan_url_g{self.rs.pass_of(sc)}" in want
        ran = [x for x in names if x.startswith("scan_")]
        # (evaluate_batch_hits fetches a hit list that outgrew its first capacity again, once: the batch then ran twice)
        assert ran == want or (leg == "rule hits" and ran == want * 2), (what, names)
        if self.name == "G" and not leg.startswith("natural"):
            assert sc.launches[1] == [6] and "lscan_x6" in names, (what, names)

    def check(self, case, legs=LEGS):
        for turn in range(case.turns):
            for label, batch in case.batches:
                for leg in legs:
                    self.check_one(f"case {case.name}: {label}, turn {turn}, {leg}", leg, batch, case.sample)

    def close(self):
        for eng, _, _ in self.engines.values():
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


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_case_on_every_leg(engines, name):
    case = SC.CASES[name]()
    e = engines(case.rs.name)
    rs, first = case.rs, case.batches[0][1]
    # the shapes the case was built for, re-proved for the tables of the legs that are sent (the CPU suite proves more of them)
    if name == "T":
        SC.assert_t_coverage(rs.model("small budget"), first)
    elif name == "E":
        SC.assert_e_coverage(rs.model("as built"), first, cold=False)
        SC.assert_e_coverage(rs.model("small budget"), first, cold=True)
    elif name == "U":
        SC.assert_u_coverage(rs.model("small budget"), first)
    elif name == "G":
        SC.assert_g_coverage(rs, "small budget", first)
        SC.assert_g_coverage(rs, "tuned", first, case.sample)
    elif name.startswith("W"):
        assert SC.chunks_of(rs, case.sample) == int(name[1:])
    e.check(case)
    want = e.reference(first, "verdict")[0]
    assert first.n == 1 or len(set(want["action"].tolist())) >= 2, f"case {name}: the oracle's verdicts are all alike"


def test_a_batch_beyond_one_workgroup_per_compute_unit(engines):
    """n = 4 096 * CUs + 777, the 4 097 case tiled (the last tile cut): every workgroup's waves hold shares of more than 256 requests in
    five blocks and more. A request's verdict depends on nothing but the request: the expected result is the oracle's on the base batch,
    tiled -- the oracle is never run at that size."""
    e = engines("M")
    eng, _ = e.engine("as built")
    base, times, n = SC.tiled_shape(eng.compute_units())
    (base_want,) = e.reference(base, "verdict")
    batch, want = base.tile(times).slice(0, n), np.tile(base_want, times)[:n]
    assert batch.n == n and len(set(base_want["action"].tolist())) >= 2
    sample = SC.case_b().sample
    for leg in ("as built", "small budget", "tuned"):
        eng, sc = e.engine(leg, sample if leg == "tuned" else None)
        eng.set_profiling(1)
        got, counts = eng.evaluate_batch(batch, with_counts=True)
        names = [k[0] for k in eng.kernel_times()]
        eng.set_profiling(0)
        what = f"{n} requests, {leg}"
        H.assert_verdicts_equal(got, want, None, what)
        assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist(), what
        e.assert_launches(what, leg, sc, names)


def test_views_and_the_device_resident_entry_point(engines):
    """case V's first batch as a view whose offsets begin above zero (requests 100 .. 300 of the same arenas), as its re-based slice, and
    through pwaf_evaluate_device; the natural leg tuned on the case's sample, where the method pass is a scan_kernel pass too"""
    import torch

    case = SC.case_v()
    e = engines("M")
    full = case.batches[0][1]
    lo, hi = 100, full.n
    view, cut = full.view(lo, hi), full.slice(lo, hi)
    assert all(int(view.offsets[f][0]) > 0 for f in (0, 1, 2, 4)) and all(int(cut.offsets[f][0]) == 0 for f in range(5))
    for leg in LEGS:
        e.check_one(f"case V: a view of requests {lo} .. {hi}, {leg}", leg, view, case.sample, rows=(lo, hi, full))
        e.check_one(f"case V: a slice of requests {lo} .. {hi}, {leg}", leg, cut, case.sample, rows=(lo, hi, full))
    for label, batch in case.batches:
        e.check_one(f"case V: {label}, natural tuned", "natural tuned", batch, case.sample)
    eng, sc = e.engine("natural tuned", case.sample)
    assert any(n.startswith("scan_method_g") for n in SC.scan_names(sc))
    (want,) = e.reference(full, "verdict")
    for leg in ("as built", "small budget", "tuned"):
        eng, sc = e.engine(leg, case.sample if leg == "tuned" else None)
        db = DeviceBatch(full)
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        eng.set_profiling(1)
        out = eng.evaluate_device(db, counts=counts)
        torch.cuda.synchronize()
        eng.device_status()
        names = [k[0] for k in eng.kernel_times()]
        eng.set_profiling(0)
        got = out.cpu().numpy().view(np.uint32)
        what = f"case V: device-resident, {leg}"
        assert (got[:, 0] == want["action"]).all() and (got[:, 1] == want["rule_idx"]).all(), what
        assert counts.cpu().tolist() == np.bincount(want["action"], minlength=4).tolist(), what
        e.assert_launches(what, leg, sc, names)
