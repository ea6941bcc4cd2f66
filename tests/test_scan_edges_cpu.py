"""The streaming-scan edge cases (tests/scan_cases.py) on the host: every case is BUILT here -- its shape assertions made by the same
functions the device suite calls, from the tables and the plan the scan-plan harness (tests/scanplan_host.cpp) dumps -- and every request
of every batch is walked through the streaming table (scan_walkers.ScanWalker) next to the raw DFA (scan_walkers.RawWalker); the two atom
sets must agree, and the bare predicates they stand for must be the ones pyoracle.Oracle finds true -- for the table of every leg the
device suite runs, under its own name (device_legs). A device failure then points at scan_kernel, not at the tables. The last two tests
show that the cases bite: scan_body's walk of one request restated with two of its lines switchable, and the block switches that must
not take a stale prefetch. No device."""
import numpy as np
import pytest

import helpers as H
import scan_cases as SC
from oracle import pyoracle
from pingoo_amd import _abi
from pingoo_amd.engine import CompiledProgram

URL = SC.URL


def device_legs(case, natural_tuned=False):
    """the tables the device suite walks for a case, under the names RuleSet.leg knows them by: -> [(leg, tuning sample or None)]. The four
    legs an engine is created for, untuned, and the small-budget engine tuned on the case's OWN sample (case V: the natural leg tuned as
    well). Nothing stands in for anything: "small budget" is the table of the verdict rules under the small budget, "rule hits" that of
    the bare predicates."""
    legs = [(leg, None) for leg in SC.LEGS] + [("tuned", case.sample)]
    return legs + ([("natural tuned", case.sample)] if natural_tuned else [])


def check_walks_against_the_oracle(case, legs):
    """legs: [(leg, sample)] as device_legs gives them. Per request of every batch and for the table of every leg: ScanWalker over the
    streaming table == RawWalker over the raw DFA, as atom sets; the url predicates of the bare rule set that hold by those atoms == the
    oracle's hit matrix rows. The atom -> predicate map is read off the oracle itself: an atom stands for the predicates that are true
    exactly where it is reported (single-atom predicates), so it is checked, not assumed. The verdict rules' url pass holds the same
    predicates as the bare rules'; the natural leg's holds the unfilterable ones alone."""
    rs = case.rs
    oracle = pyoracle.Oracle(rs.bare_rules, {})
    for label, batch in case.batches:
        hit, want = H.oracle_matrix(oracle, batch)
        assert len(want) == batch.n
        values = [batch.field_bytes(URL, i) for i in range(batch.n)]
        for leg, sample in legs:
            m = rs.model(leg, sample)
            what = (case.name, label, leg, sample[0] if sample else "untuned")
            seen = {}  # (a batch of the block cases holds a handful of distinct values)
            for v in values:
                if v not in seen:
                    w = m.walk(v)
                    assert set(w["atoms"]) == set(w["raw_atoms"]), (what, v, w["atoms"], w["raw_atoms"])
                    seen[v] = frozenset(w["atoms"])
            # a predicate that is one atom: its oracle row is that atom's report row, for SOME atom of the pass; conjunctions: of all theirs
            n_atoms = m.g["n_local"]
            rows = np.zeros((n_atoms, batch.n), dtype=bool)
            for i, v in enumerate(values):
                for x in seen[v]:
                    rows[x, i] = True
            for k, pred in enumerate(rs.preds):
                if " && " in pred or k in getattr(rs, "elsewhere", ()) or (leg.startswith("natural") and k not in rs.natural):
                    continue  # (a conjunction of predicates that are rules of their own; a predicate another pass or the attribute kernel decides)
                assert any((rows[a] == hit[k]).all() for a in range(n_atoms)), f"{what}: no atom of the url pass is reported exactly where predicate {k} ({pred}) holds"
    assert len({id(rs.model(leg, sample)) for leg, sample in legs}) == len(legs), f"case {case.name}: two legs share one table object"


def test_the_constants_the_cases_rest_on():
    """launch_scan: 256 requests per wave at least, 16 waves per workgroup, at most one workgroup per CU; scan_body: shares of
    ceil(n / waves); tune_host: 48 and 80 bytes"""
    assert SC.shares(1) == (1, 1, [(0, 1)]) and SC.shares(4096)[:2] == (1, 256) and SC.shares(4097)[:2] == (2, 129)
    assert SC.shares(4096 * 256 + 777, 256)[:2] == (256, 257) and SC.shares(10 ** 7, 256)[0] == 256
    src = open(SC.SP.HERE + "/../pingoo_amd/csrc/scan.hip").read() + open(SC.SP.HERE + "/../pingoo_amd/csrc/scanplan.cpp").read()
    for text in ("uint32_t waves = (a.n + 255) / 256;", "static constexpr int kScanThreads = 1024;", "const uint32_t f_base = blk + 64;", "const uint32_t t4 = 80u, t2 = 48u;"):
        assert text in src, text


@pytest.mark.parametrize("name", sorted(SC.SETS))
def test_the_sets_have_the_shapes_they_were_written_for(name):
    """every leg's url pass is a plain scan pass (RuleSet.pass_of); the harness compiles what an engine compiles (the same program dump);
    the natural leg's pass has no prefilter without being told so"""
    rs = SC.SETS[name]()
    for leg in SC.LEGS:
        sc = rs.scan(leg)
        k = rs.pass_of(sc)
        rules, flags, budget = rs.leg(leg)
        prog = CompiledProgram(rules, {}, flags=flags, lds_table_budget=budget, max_table_bytes=rs.table_bytes)
        assert sc.blob.startswith(prog.dump()), f"set {name}, {leg}: the harness and pwaf_program_create compile different programs"
        assert f"scan_url_g{k}" in SC.scan_names(sc)
        if leg == "natural":
            assert flags == 0 and sc.roles[k]["filtered"] == 0 and "f_table" not in sc.groups[k], "the unfilterable regex got a prefilter"
    small = rs.model("small budget")
    assert small.n_hot < small.n_states, f"set {name}: nothing is cold under the small budget"
    if name == "M":
        assert 1 < small.n_hot < small.n_states and 0 < small.m["emit_base"] < small.m["special_base"]
    if name == "U":
        assert small.m["scalar_mode"] == 1 and rs.model("as built").m["scalar_mode"] == 1
    if name == "X":
        assert small.n_classes > 127 and rs.model("as built").n_classes > 127
    if name == "E":
        assert small.m["start_emit"] and len(small.m["list"]) >= 4, "emit lists and a start emit"


def test_every_tuning_sample_is_cached_under_a_key_of_its_own():
    """RuleSet.scan, RuleSet.model and the device suite's engines are cached by the sample's key: two cases share a key exactly when their
    samples hold the same values, in whatever order the cases are built -- and the table a case gets for its sample is the one a fresh
    run of the harness over that sample gives, after every other case of the set has been built"""
    cases = {name: SC.CASES[name]() for name in sorted(SC.CASES, reverse=True)}
    names = sorted(cases)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            ca, cb = cases[a], cases[b]
            assert (ca.sample[0] == cb.sample[0]) == SC.same_sample(ca.sample, cb.sample), (a, b)
    assert len({cases[n].sample[0] for n in ("W1", "W2", "W4", "B", "T", "V")}) == 6, "six different samples over set M"
    assert cases["B"].sample[0] == cases["B runs"].sample[0] == cases["B long"].sample[0], "the block cases are tuned on one sample"
    for name in names:
        case = cases[name]
        rs = case.rs
        leg = "tuned"
        rules, flags, budget = rs.leg(leg)
        got = rs.scan(leg, case.sample)
        cols = SC.sample_columns(case.sample[1], got.tables.header_names)
        fresh = SC.harness(rules, flags, budget, cols, rs.table_bytes)
        assert got.blob == fresh.blob, f"case {name}: the cached plan of its tuned leg is not the harness's over its own sample"
        k = rs.pass_of(got)
        assert (rs.model(leg, case.sample).m["tab"] == fresh.scan_image(k)["tab"]).all(), name
        # what the device suite asserts of every engine it tunes, here of the program tuned on the host (the same tune_host, no device)
        for tleg in ("tuned", "natural tuned") if name == "V" else ("tuned",):
            rules, flags, budget = rs.leg(tleg)
            prog = CompiledProgram(rules, {}, flags=flags, lds_table_budget=budget, max_table_bytes=rs.table_bytes)
            prog.tune(case.sample[1])
            SC.assert_tuned_as_planned(prog, rs.scan(tleg, case.sample), rs.scan(tleg), (name, tleg))
    # the samples of B and T differ, and so do the tables they tune
    assert (cases["B"].rs.model("tuned", cases["B"].sample).m["tab"] != cases["T"].rs.model("tuned", cases["T"].sample).m["tab"]).any()


@pytest.mark.parametrize("ch", [1, 2, 4])
def test_case_w_every_length_at_every_offset_for_each_chunk_count(ch):
    """the builder asserts the lengths, the offsets and the Q behind every X; here: CH from the tuning sample on both sides of each threshold,
    fields without any atom (a record of zero atoms), and the walks"""
    case = SC.case_w(ch)
    rs = case.rs
    print(case.name, case.measured)
    n = 64
    for total, want in ((SC.CH2_MEAN * n - 1, 1), (SC.CH2_MEAN * n, 2), (SC.CH4_MEAN * n - 1, 2), (SC.CH4_MEAN * n, 4)):
        assert SC.chunks_of(rs, SC.fixed_sample(rs, f"edge {total}", total, n)) == want, total
    m = rs.model("tuned", case.sample)
    cov = SC.coverage(m, case.batches[0][1], only=range(0, case.batches[0][1].n, 3))
    assert cov.get(("atoms", 0)) and cov.get(("atoms", 1))
    check_walks_against_the_oracle(case, device_legs(case))


def test_case_b_shares_blocks_and_runs():
    for case in (SC.case_b(), SC.case_b_runs(), SC.case_b_long()):
        print(case.name, case.measured)
        check_walks_against_the_oracle(case, device_legs(case))
    base, times, n = SC.tiled_shape()
    assert base.n == 4097 and times * base.n >= n > (times - 1) * base.n and n == 4096 * SC.MI355X_CUS + 777


def test_case_t_reaches_every_tier_at_every_group_position():
    case = SC.case_t()
    rs = case.rs
    print(case.name, case.measured)
    batch = case.batches[0][1]
    cov = SC.assert_t_coverage(rs.model("small budget"), batch)
    print({k: v for k, v in sorted(cov.items(), key=str) if k[0] in ("enter", "cold to", "end")})
    SC.assert_t_coverage(rs.model("rule hits"), batch)
    # as built every row is hot: plain and emitting rows at every position, nothing cold
    hot = SC.coverage(rs.model("as built"), batch)
    assert all(hot.get(("enter", kind, p)) for kind in (SC.PLAIN, SC.EMIT) for p in range(4)) and not any(k[0] == "enter" and k[1] == SC.COLD for k in hot)
    # tuned: the sample re-ranks the rows; the case still reaches the three tiers
    tuned = rs.model("tuned", case.sample)
    tc = SC.coverage(tuned, batch)
    print("tuned on T's own sample: cold rows entered per group byte", [tc.get(("enter", SC.COLD, p), 0) for p in range(4)])
    assert (tuned.m["tab"] != rs.model("small budget").m["tab"]).any(), "the sample's visits reorder no row"
    assert all(any(tc.get(("enter", kind, p)) for p in range(4)) for kind in SC.KINDS)
    check_walks_against_the_oracle(case, device_legs(case))


def test_case_e_every_emit_shape_on_hot_and_on_cold_rows():
    case = SC.case_e()
    rs = case.rs
    batch = case.batches[0][1]
    print(SC.assert_e_coverage(rs.model("as built"), batch, cold=False))
    print(SC.assert_e_coverage(rs.model("small budget"), batch, cold=True))
    SC.assert_e_coverage(rs.model("rule hits"), batch, cold=True)
    check_walks_against_the_oracle(case, device_legs(case))


def test_case_u_scalar_mode():
    case = SC.case_u()
    rs = case.rs
    SC.assert_u_coverage(rs.model("as built"), case.batches[0][1])
    SC.assert_u_coverage(rs.model("small budget"), case.batches[0][1])
    assert SC.chunks_of(rs, case.sample) == 2
    check_walks_against_the_oracle(case, device_legs(case))


def test_case_x_more_than_127_classes():
    case = SC.case_x()
    print(case.name, case.measured)
    check_walks_against_the_oracle(case, device_legs(case))


def test_case_g_the_owner_feeds_the_gap_passes():
    case = SC.case_g()
    rs = case.rs
    for leg in ("as built", "small budget", "rule hits"):
        print(leg, SC.assert_g_coverage(rs, leg, case.batches[0][1]))
    SC.assert_g_coverage(rs, "tuned", case.batches[0][1], case.sample)
    check_walks_against_the_oracle(case, device_legs(case))


def test_case_v_five_plain_passes_and_the_method_pass_once_tuned():
    case = SC.case_v()
    rs = case.rs
    want = {0, 1, 2, 4, 5}  # (the method pass walks the identity list: see the case)
    for leg, sample in (("as built", None), ("small budget", None), ("rule hits", None), ("tuned", case.sample)):
        sc = rs.scan(leg, sample)
        assert {sc.groups[int(n.rsplit("_g", 1)[1])]["field"] for n in SC.scan_names(sc)} == want, leg
    sc = rs.scan("natural tuned", case.sample)
    assert {sc.groups[int(n.rsplit("_g", 1)[1])]["field"] for n in SC.scan_names(sc)} == {1, 3}, "flags 0, tuned on long methods: the url and the method pass"
    # each pass has requests of its own that match: the oracle decides by every extra rule and by url rules
    oracle = pyoracle.Oracle(rs.verdict_rules, {})
    for label, batch in case.batches:
        got = set(oracle.evaluate(batch)["rule_idx"].tolist())
        assert got >= set(range(len(rs.preds), len(rs.verdict_rules))) | {_abi.RULE_NONE}, (label, sorted(got))
    check_walks_against_the_oracle(case, device_legs(case, natural_tuned=True))


# ---------------------------------------------------------------------------------------------------------
# that the cases bite: scan_body's walk of ONE request restated over the harness's tables, with two of its lines switchable
# ---------------------------------------------------------------------------------------------------------
def kernel_walk(m, arena, p, end, ch, mutation=None):
    """csrc/scan.hip, scan_body, sections 2 and 3 for one lane and one request [p, end) of `arena` (tables without scalar mode): the
    chunks as the prefetch addresses them (a chunk the field does not reach, and an empty field's, is the arena's first 16 bytes), the
    classes with bytes past the field's end as the STAY cell, the speculative groups of four over the LDS copy (hot rows, then a
    sentinel row of 0xFFFF), redo / chain / careful_step, the END cell from the global table for a parked lane. -> the set of atoms.
    mutation "no mask": c2[k] = c whatever k < cnt says; "end from lds": the END cell always from LDS."""
    T, img = m.m, m.img
    tab, st, C, cls = T["tab"], T["stride"], T["n_classes"], T["cls"]
    hot, eb, sb = T["n_hot"] * st, T["emit_base"], T["special_base"]
    assert m.um is None
    lds = lambda i: int(tab[i]) if i < hot else 0xFFFF  # noqa: E731  (whatever lies behind the sentinel row is never used: see chain)
    atoms = set(img.start()[1])
    row, crow, pos = 0, 0, p

    def careful(prev, col, t):
        nonlocal crow
        cell = int(tab[crow * st + col]) if prev == hot else t
        if cell >= sb:
            sp = T["special"][cell - sb]
            crow = int(sp["next_off"]) // (2 * st)
            if sp["emit"]:
                atoms.update(img.lst(int(sp["emit"])))
            return hot
        if cell >= eb:
            atoms.update(img.cell(lds(cell + C + 2)))
        return cell

    while True:
        have = pos < end
        cnt_all = min(16 * ch, end - pos) if have else 0
        for q in range(ch):
            cnt = min(16, cnt_all - 16 * q) if cnt_all > 16 * q else 0
            at = pos + 16 * q if have and (q == 0 or pos + 16 * q < end) else 0
            cols = [int(cls[b]) if k < cnt or mutation == "no mask" else C for k, b in enumerate(arena[at:at + 16].tolist())]
            for k0 in range(0, 16, 4):
                ts, t = [], row
                for k in range(4):
                    t = lds(t + cols[k0 + k])
                    ts.append(t)
                if max(ts) < eb:
                    row = ts[3]
                    continue
                cur, chain = row, True
                for k in range(4):
                    t = ts[k] if chain else lds(cur + cols[k0 + k])
                    if k0 + k >= cnt:
                        chain = chain and t < sb
                    elif t >= sb:
                        new = careful(cur, cols[k0 + k], t)
                        chain, cur = chain and new == t, new
                    else:
                        if t >= eb:
                            atoms.update(img.cell(lds(t + C + 2)))
                        cur = t
                row = cur
        pos += cnt_all
        if pos >= end:
            e = int(tab[crow * st + C + 1]) if row == hot and mutation != "end from lds" else lds(row + C + 1)
            atoms.update(img.cell(e) if e != 0xFFFF else {0x7FFF})
            return atoms


def changed_by(case, leg, sample, ch, mutation):
    """-> per batch of the case, the requests whose set of real atoms the mutation changes; unmutated, kernel_walk gives the table walker's atoms for
    every request (asserted)"""
    m = case.rs.model(leg, sample)
    out = []
    for label, batch in case.batches:
        arena, off = batch.data[URL], batch.offsets[URL].astype(np.int64)
        memo, changed = {}, 0
        for i in range(batch.n):
            p, end = int(off[i]), int(off[i + 1])
            key = (end - p, arena[p:end + 16 * ch].tobytes())
            if key not in memo:
                plain = kernel_walk(m, arena, p, end, ch)
                assert plain == set(m.walk(arena[p:end].tobytes())["atoms"]), (case.name, label, i)
                memo[key] = kernel_walk(m, arena, p, end, ch, mutation) - {0x7FFF} != plain  # (the sentinel's END cell reads as atom 0x7FFF: no atom of any pass)
            changed += bool(memo[key])
        out.append(changed)
    return out


NO_MASK, END_LDS = "no mask", "end from lds"
# (case, leg, chunks per iteration on that leg, the mutations that must change a request there). As built every row is hot: no lane parks,
# and a byte read past the end moves a lane along plain rows unseen -- the leg where the dropped mask shows most; under the small
# budget a lane parked on a cold row, or a step onto an emitting row, sends the group through redo, which tests k < cnt itself.
BITES = [("W1", "as built", 1, {NO_MASK}), ("W1", "tuned", 1, {NO_MASK, END_LDS}), ("W2", "tuned", 2, {NO_MASK, END_LDS}), ("W4", "tuned", 4, {NO_MASK, END_LDS}),
         ("B runs", "as built", 1, {NO_MASK}), ("B runs", "small budget", 1, {NO_MASK}), ("T", "as built", 1, {NO_MASK}), ("T", "small budget", 1, {NO_MASK, END_LDS}),
         ("E", "as built", 1, {NO_MASK}), ("E", "small budget", 1, {END_LDS}), ("X", "small budget", 1, {NO_MASK, END_LDS}), ("G", "small budget", 1, {NO_MASK})]


@pytest.mark.parametrize("name,leg,ch,expects", BITES, ids=[f"{b[0]}, {b[1]}" for b in BITES])
def test_the_walk_restated_and_two_of_its_lines_broken(name, leg, ch, expects):
    """scan_body's per-request walk restated (kernel_walk) reproduces the table walker on every request of the case; with the k < cnt mask
    dropped, and with the END cell of a parked lane read from LDS, requests of the case change their atoms -- each an entry of the hit
    matrix the device suite compares. docs/scan_edges.md records the counts this prints. (Which lanes and offsets a request gets is not
    part of this restatement: see test_a_block_switch_that_must_load_on_the_spot.)"""
    case = SC.CASES[name]()
    sample = case.sample if leg == "tuned" else None
    assert SC.chunks_of(case.rs, sample) == ch if leg == "tuned" else ch == 1, "an engine walks with CH = 1 until it is tuned"
    changed = {mut: changed_by(case, leg, sample, ch, mut) for mut in (NO_MASK, END_LDS)}
    print(name, leg, "requests", [b.n for _, b in case.batches], changed)
    for mut in expects:
        assert sum(changed[mut]), f"case {name}, {leg}: '{mut}' changes no request's atoms"


def test_a_block_switch_that_must_load_on_the_spot():
    """"always take the prefetched offsets": at a switch that follows another at once the prefetch still holds the offsets of the block
    just consumed, at a wave's first switch nothing (0, 0). The requests of the new block would then be walked over the bytes of the
    requests 64 before them, or as empty fields at the arena's start. simulate_pulls names every such switch of case B runs; the switch
    SHOWS in the hit matrix the device suite compares when the oracle's hit columns of the new block differ from what those bytes give.
    A block inside a run does not show it (its fields equal those 64 before them); the block that holds the run's end and the matching
    request behind it does: every share with a switch that follows another has one that shows, in both batches."""
    case = SC.case_b_runs()
    rs = case.rs
    oracle = pyoracle.Oracle(rs.bare_rules, {})
    url = slice(0, len(rs.preds))
    empty = H.oracle_matrix(oracle, SC.RequestBatch.from_requests([rs.request(b"")]))[0][url, 0]
    for label, batch in case.batches:
        hit, _ = H.oracle_matrix(oracle, batch)
        lens = np.diff(batch.offsets[URL].astype(np.int64))
        first, after, shares_with = [0, 0], [0, 0], 0
        for w0, w1 in SC.shares(batch.n)[2]:
            shown = []
            for blk, stale in SC.simulate_pulls(lens, w0, w1, 16)["spot_blocks"]:
                hi = min(blk + 64, w1)
                if stale is None:
                    first[0] += 1
                    first[1] += bool((hit[url, blk:hi] != empty[:, None]).any())
                else:
                    assert stale == blk - 64
                    shown.append(bool((hit[url, blk:hi] != hit[url, stale:stale + hi - blk]).any()))
            if shown:
                shares_with += 1
                assert any(shown), (label, w0, "no switch that follows another shows in the hit matrix")
            after[0] += len(shown)
            after[1] += sum(shown)
        print(label, "switches loaded on the spot (all, those that show): a wave's first", first, "after another switch", after, "in", shares_with, "shares")
        assert shares_with == 8 and first[1] >= 8, "five runs of 64 and more from share offset 0, three of 128 and more from offset 37"
