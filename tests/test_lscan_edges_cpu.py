"""The list-scan edge cases (tests/lscan_cases.py) on the host: the two hooks they are built from -- pwaf_program_flat_image, the flat
table exactly as an engine uploads it, and pwaf_program_list_scans, the descriptors of a batch from the plan the engine launches -- are
checked against the scan-plan harness (tests/scanplan_host.cpp) and against a restatement of the descriptor rules; every case is BUILT
here, its shape assertions made by the same functions the device suite calls, and walked request by request through the CPU table
walker against the oracle. No device."""
import random

import numpy as np
import pytest

import lscan_cases as LC
import table_walker
import test_scanplan_cpu as SP
from oracle import pyoracle
from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.engine import CompiledProgram, PwafError

NC, ND, HITS = _abi.OPT_NO_CONFIRM, _abi.OPT_NO_DENSE_SWITCH, _abi.OPT_RULE_HITS
LIST_SHAPES = {0: (512, 48 * 1024), 2: (1024, 144 * 1024)}  # (scanplan.cpp: list_shape(0), list_shape(2))


# ---------------------------------------------------------------------------------------------------------
# the hooks against the harness, and the descriptors restated
# ---------------------------------------------------------------------------------------------------------
def restated(roles, flat, rt, dense_switch):
    """the descriptors of a batch from the roles and the table shapes: what run_pipeline built inline before the planner had them. A second
    copy of the code under test, kept to PIN the refactor (same constants, same 48-byte reserve): not a specification of the planner"""
    filtered = [r for r in roles if r["filtered"]]
    wide0 = not (filtered and all(r["confirm"] for r in filtered))
    shapes = [LIST_SHAPES[2 if wide0 else 0], LIST_SHAPES[0]]

    def resident(f, hb):
        row = 2 * (f["n_classes"] + 3)
        if f["n_delta"] and f["n_full"] * row + 48 + 8 * f["n_delta"] <= hb:
            return f["n_full"], f["n_delta"]
        return min(f["n_full"] if f["n_delta"] else f["n_states"], (hb - 48) // row), 0

    out = []
    for phase in (0, 1):
        threads, hb = shapes[phase]
        for k, r in enumerate(roles):
            if (phase != 0) if r["identity"] else (r["gate"] < 0 or bool(r["filtered"]) != (phase == 0)):
                continue
            has_dense = lambda q: bool(dense_switch and roles[q]["filtered"] and roles[q]["confirm"])  # noqa: E731
            dense = phase == 0 and r["confirm"] and has_dense(k)
            base = dict(phase=phase, threads=threads, hot_bytes=hb, behind_filter=r["filtered"], share_owner=r["share_owner"], need_bit=r["gate"] if r["share_owner"] >= 0 else 0)
            base["pass"] = k
            if dense:
                n_hot, n_delta = resident(flat[k], hb)
                out.append(dict(base, tier=0, n_hot=n_hot, n_delta=n_delta, merge_rec=0, dense_mode=1))
            if r["confirm"] and not r["confirm_walk"]:
                continue
            tier = int(bool(r["confirm"] and rt[k] is not None))
            n_hot, n_delta = resident(rt[k] if tier else flat[k], hb)
            out.append(dict(base, tier=tier, n_hot=n_hot, n_delta=n_delta, merge_rec=r["confirm"],
                            dense_mode=2 if dense else 3 if r["share_owner"] >= 0 and has_dense(r["share_owner"]) else 0))
    return out


PIN_SETS = {"M": lambda: (LC.set_m().verdict_rules, {}), "L": lambda: (LC.set_l().verdict_rules, {}),
            "gap": lambda: (SP.H.kind_rules("gap", 6, seed=1)[0] + SP.H.kind_rules("confirm_walk", 3, seed=2)[0], dict(max_table_bytes=65536)),
            "tune": lambda: (SP.TUNE_RULES, {}), "method": lambda: (SP.METHOD_RULES, {})}


@pytest.mark.parametrize("flags", [0, NC, ND], ids=["as built", "no confirm tier", "no dense switch"])
@pytest.mark.parametrize("name", sorted(PIN_SETS))
def test_the_hooks_answer_what_the_scan_plan_harness_reports(tmp_path, name, flags):
    """pins the refactor: for a handful of rule sets the hook's descriptors are the harness's (the same planner, called as the engine
    calls it), fall into the LLS0 / LLS1 launch split, follow from the roles by the rules restated above, and the hook's flat images
    are the harness's byte for byte"""
    rules, opts = PIN_SETS[name]()
    sc = SP.run_one(tmp_path, rules, flags=flags, opts=(0, 0, opts.get("max_table_bytes", 0)))
    prog = CompiledProgram(rules, {}, flags=flags, **opts)
    got = prog.list_scans()
    keys = ("phase", "pass", "tier", "threads", "hot_bytes", "n_hot", "n_delta", "behind_filter", "merge_rec", "dense_mode", "share_owner", "need_bit")
    ldsc = np.frombuffer(sc.plan["LDSC"], dtype="<u4").reshape(-1, len(keys)).astype(np.int64)
    ldsc[ldsc == 0xFFFFFFFF] = -1
    assert [[d[k] for k in keys] for d in got] == ldsc.tolist()
    # the launch split
    for phase in (0, 1):
        mine = [d for d in got if d["phase"] == phase]
        launches = sc.launches[phase]
        assert sum(launches) == len(mine)
        at = 0
        for li, cnt in enumerate(launches):
            assert all((d["launch"], d["launch_count"]) == (li, cnt) for d in mine[at:at + cnt])
            at += cnt
    # the roles, by brute force from the dump; the descriptors from them
    SP.check_pass_plan(sc, short=(next(k for k, g in enumerate(sc.groups) if g["field"] == SP.FIELD_METHOD), [(b"POST", True), (b"PU", False)]) if name == "method" else None)
    flat = [sc.flat_image(k) for k in range(len(sc.groups))]
    rt = [sc.flat_image(k, "T") if "TSHP" in sc.img[k] else None for k in range(len(sc.groups))]
    want = restated(sc.roles, flat, rt, not flags & ND)
    assert [{k: d[k] for k in keys} for d in got] == [{k: int(w[k]) for k in keys} for w in want]
    # the images
    for k in range(len(sc.groups)):
        for tier, tag in ((0, "F"), (1, "T")):
            if tier and rt[k] is None:
                with pytest.raises(PwafError):
                    prog.flat_image(k, 1)
                continue
            mine = {t: pl for t, _, pl in table_walker.parse_dump(prog.flat_image(k, tier))}
            for sfx in ("SHP", "FLT", "DLT", "CLS", "EMO", "EML", "ENO", "ENL"):
                assert mine["F" + sfx] == sc.img[k][tag + sfx], (k, tier, sfx)
    with pytest.raises(PwafError):
        prog.flat_image(len(sc.groups), 0)


def test_a_tuned_program_answers_for_the_tuned_tables(tmp_path):
    """after pwaf_program_tune the hooks give the tables rebuilt for the sample (states renumbered by visits): the harness's, run over
    the same sample"""
    sample = SP.tune_sample(random.Random(21), header=False)[:5]
    rules = [r for r in SP.TUNE_RULES if r[0] != "h"]  # (the five fields alone)
    sc = SP.run_one(tmp_path, rules, sample=sample)
    prog = CompiledProgram(rules, {})
    before = [prog.flat_image(k, 0) for k in range(len(sc.groups))]
    n = len(sample[0])
    reqs = [Request(host=sample[0][i].decode(), url=sample[1][i].decode(), path=sample[2][i].decode(), method=sample[3][i].decode(), user_agent=sample[4][i].decode()) for i in range(n)]
    prog.tune(RequestBatch.from_requests(reqs))
    moved = 0
    for k in range(len(sc.groups)):
        mine = {t: pl for t, _, pl in table_walker.parse_dump(prog.flat_image(k, 0))}
        for sfx in ("SHP", "FLT", "DLT", "EMO", "EML", "ENO", "ENL"):
            assert mine["F" + sfx] == sc.img[k]["F" + sfx], (k, sfx)
        moved += prog.flat_image(k, 0) != before[k]
    assert moved, "the sample's visits reorder no table"
    keys = ("phase", "pass", "tier", "n_hot", "n_delta", "dense_mode")
    ldsc = np.frombuffer(sc.plan["LDSC"], dtype="<u4").reshape(-1, 12)
    assert [[d[k] for k in keys] for d in prog.list_scans()] == ldsc[:, [0, 1, 2, 5, 6, 9]].tolist()


# ---------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------
def check_against_the_oracle(case, covs, alike_ok=False):
    """every request through the CPU table walker (Coverage kept its verdicts) against the oracle, for each program walked"""
    oracle = pyoracle.Oracle(case.rs.verdict_rules, {})
    for label, batch in case.batches:
        want = oracle.evaluate(batch)
        for what, cov in covs[label].items():
            got = cov.verdicts
            bad = [i for i in cov.only if got[i] != (int(want[i]["action"]), int(want[i]["rule_idx"]))]
            assert not bad, (case.name, label, what, len(bad), bad[:3], batch.field_bytes(case.rs.field_id, bad[0]), got[bad[0]], want[bad[0]])
        assert alike_ok or len(set(want["action"].tolist())) >= 2, f"{case.name}: the oracle's verdicts are all alike"


def coverage(case, flag_list, dense=False, only=None):
    return {label: {f: LC.Coverage(case.rs, f, batch, dense=dense, only=only) for f in flag_list} for label, batch in case.batches}


def assert_emits_of_every_tier(row, what):
    """an EMIT cell read for a state of every tier that has an emitting state, an end-of-field atom from every tier that has one; a tier
    without such a state shows none"""
    d, m, _, count = row
    for key, has in LC.emitting_tiers(d, m).items():
        assert bool(count.get(key, 0)) == has, f"{what}: {key}: the table {'has' if has else 'has no'} such state, the case shows {count.get(key, 0)}"


@pytest.mark.parametrize("set_name", ["M", "L"])
def test_case_t_reaches_every_tier_at_every_group_position(set_name):
    """T and E: the shapes asserted by the builders (lscan_cases.m_descriptors / l_descriptors), then per descriptor: every boundary
    state is left from, every tier that exists at each of the four positions, a tier that does not exist nowhere; the record, tail,
    consecutive-cold and emit features the issue names"""
    case = LC.case_t(set_name)
    rs, descs = LC.DESCRIPTORS[set_name]()
    assert all(v == [] for v in case.measured["unreached"].values()), case.measured
    covs = coverage(case, (0, NC))
    cov = covs[case.batches[0][0]]
    for name, (flags, d, m) in descs.items():
        if d["dense_mode"] == 1:
            continue  # (walks in case D)
        row = cov[flags].row(**{"pass": d["pass"], "tier": d["tier"], "phase": d["phase"]})
        print(set_name, name, LC.Coverage.summary(row))
        LC.assert_tiers_at_every_position(row, f"{set_name}, {name}")
        count = row[3]
        for s in LC.boundary_states(d, m):
            assert count.get(("state", s), 0), f"{set_name}, {name}: boundary state {s} is never left from"
        if d["n_hot"] + d["n_delta"] < m.n_states:
            assert all(count.get(("cold-tail", k), 0) for k in (1, 2, 3)), "a cold step in a last group of 1, 2 and 3 valid bytes"
            assert count.get("cold-cold", 0) and count.get("cold-to-hot", 0) and count.get(("stay", LC.COLD), 0)
        assert_emits_of_every_tier(row, f"{set_name}, {name}")
        if m.scalar_mode and d["n_hot"] + d["n_delta"] < m.n_states and d["behind_filter"]:
            # scalar mode: a lead byte at each group position and a sequence cut off by the field's end, read while the walk stands in a cold state
            assert all(count.get(("lead", LC.COLD, p), 0) for p in range(4)) and count.get(("truncated", LC.COLD), 0), (name, {k: v for k, v in count.items() if k[0] in ("lead", "truncated")})
    if set_name == "M":
        full = cov[NC].row(phase=0, tier=0, behind_filter=1, **{"pass": descs["R as built"][1]["pass"]})[3]
        r = cov[0].row(phase=0, tier=1)[3]
        assert full.get(("emit", LC.HOT, "single"), 0)
        assert full.get(("emit", "flat", "list"), 0), "two literals that end at the same byte: an emit LIST"
        assert full.get("atom-twice", 0) and r.get("atom-twice", 0) and full.get(("atoms", 3), 0) and full.get(("atoms", 4), 0) and r.get(("atoms", 3), 0)
        assert full.get(("emit-state", "rec"), 0), "a record state's EMIT cell (read from the flat table)"
        # the atom emitted at the start state: the method's identity pass
        prog = rs.program(0)
        (ident,) = [d for d in LC.descriptors_of(prog) if d["field"] == 3]
        m = LC.FlatModel(prog, ident["pass"], 0)
        assert ident["behind_filter"] == 0 and m.emits(0), "the method pass does not emit at its start state"
    else:
        full = cov[NC].rows[0][3]
        assert full.get(("rec<2", LC.EX1), 0) and full.get(("rec<2", LC.BASE), 0), "a record with fewer than two exceptions"
        assert full.get(("emit-state", "rec"), 0)
    check_against_the_oracle(case, covs)


def test_case_w_every_length_at_every_offset():
    case = LC.case_w()
    rs, (label, batch) = case.rs, case.batches[0]
    off = batch.offsets[rs.field_id]
    lens = np.diff(off)
    seen = {(int(off[i]) % 16, int(lens[i])) for i in range(1, batch.n, 2)}
    assert seen >= {(o, n) for o in range(16) for n in (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49)}
    covs = coverage(case, (0, NC))
    for flags, tier in ((0, 1), (NC, 0)):
        d, m, n_walked, count = covs[label][flags].row(phase=0, tier=tier, behind_filter=1, **{"pass": LC.m_descriptors()[1]["R as built"][1]["pass"]})
        walked = covs[label][flags].walked
        got = {int(lens[i]) for i in range(batch.n) if (d["pass"], tier) in walked[i]}
        print("W", flags, sorted(got), n_walked)
        assert got >= ({15, 16, 17, 31, 32, 33, 47, 48, 49} if tier else {3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49}), (flags, sorted(got))
        assert (d["pass"], tier) in walked[batch.n - 1], "the arena's last request is not walked"
    check_against_the_oracle(case, covs)


def test_case_s_one_gap_pass_on_the_owners_list_with_its_need_bit_set_and_clear():
    case = LC.case_s()
    rs, descs = LC.m_descriptors()
    _, gd, gm = descs["sharing gap pass"]
    _, rd, _ = descs["R as built"]
    covs = coverage(case, (0,))
    for label, batch in case.batches:
        walked = covs[label][0].walked
        # (the device also sends a request through the R-tier walk when a LITERAL factor of the gap pass was confirmed: it is how the request
        # gets on the list the gap pass shares; the table walker has no list, its verdicts do not depend on it)
        owner = [i for i in range(batch.n) if (rd["pass"], 1) in walked[i] or (gd["pass"], 0) in walked[i]]
        shared = [i for i in owner if (gd["pass"], 0) in walked[i]]
        print(label, len(owner), len(shared))
        assert len(shared) >= 100 and len(owner) - len(shared) >= 50, "requests on the owner's list with and without the gap pass's need bit"
    check_against_the_oracle(case, covs)


def test_case_d_is_walked_whole():
    case = LC.case_d()
    print("D", case.measured)
    assert case.measured["flagged_chunks"] > case.measured["dense_thresh"]
    rs, descs = LC.m_descriptors()
    covs = coverage(case, (0,), dense=True)
    (label, batch), = case.batches
    _, d, m = descs["dense alternative"]
    row = covs[label][0].row(dense_mode=1, **{"pass": d["pass"]})
    assert row[2] == batch.n
    LC.assert_tiers_at_every_position(row, "D, dense alternative")
    gap = covs[label][0].row(dense_mode=3)
    assert 0 < gap[2] < batch.n
    assert not [r for r in covs[label][0].rows if r[0]["dense_mode"] == 2]
    check_against_the_oracle(case, covs)


@pytest.mark.parametrize("n_list", LC.P_LENGTHS)
def test_case_p_list_lengths_on_both_sides_of_an_eighth(n_list):
    case = LC.case_p(n_list)
    print(case.name, case.measured)
    assert case.measured["n_list"] == n_list and case.measured["long_list"] == (n_list >= 512) and case.measured["n"] == LC.N_P
    # the candidates and as many of the others through the table walker, as built and without the confirm tier
    batch = case.batches[0][1]
    cands, _ = LC.candidates_by_model(case.rs, batch, NC)
    rest = [i for i in range(batch.n) if i not in set(cands)]
    covs = coverage(case, (0, NC), only=sorted(cands + rest[:max(64, len(cands))]))
    for flags, tier in ((0, 1), (NC, 0)):
        row = covs[case.batches[0][0]][flags].row(phase=0, tier=tier, behind_filter=1, **{"pass": LC.m_descriptors()[1]["R as built"][1]["pass"]})
        assert row[2] == n_list, (flags, row[2])  # (every candidate holds a whole regex match: as built the walk list is the candidate list)
    check_against_the_oracle(case, covs, alike_ok=n_list == 0)


@pytest.mark.parametrize("blocked", LC.WAVE_COUNTS)
def test_case_p_waves_with_blocked_lanes(blocked):
    """the builder proves that the tiled batch fills the launch's waves (entries_per_item == 64 for 256 compute units, and not for 64
    requests fewer) and that exactly `blocked` of a wave's 64 lanes leave a cold state in the same group; the base batch through the walker"""
    case, times = LC.case_p_waves(blocked)
    print(case.name, case.measured)
    assert case.measured["epi"] == 64 and case.measured["n"] == 64 * times > 32 * case.measured["n_waves"] and case.measured["group"] >= 2
    check_against_the_oracle(case, coverage(case, (NC,)))


def test_the_tuned_set_has_other_states_hot_and_still_every_tier():
    """the tuned leg of the device suite, proved here: the R tier rebuilt for the sample differs from the one as built, is still clamped
    by the 48 KiB launch, and case T still leaves from hot and cold rows at every group position; the table walker over the TUNED
    program gives the oracle's verdicts"""
    sample, host, d, m = LC.tuned_m()
    rs = LC.set_m()
    case = LC.case_t("M")
    (label, batch), = case.batches
    cov = LC.Coverage(rs, 0, batch, prog=host)
    row = cov.row(phase=0, tier=1)
    print("tuned", LC.Coverage.summary(row))
    LC.assert_tiers_at_every_position(row, "tuned, R tier")
    plain = LC.Coverage(rs, 0, batch).row(phase=0, tier=1)
    assert row[1].n_states == plain[1].n_states and (row[1].flat != plain[1].flat).any()
    check_against_the_oracle(case, {label: {"tuned": cov}})


def test_case_sg_six_gap_passes_on_one_owner():
    """the builder proves the need bits (all or none: set_g asserts why never exactly one) and the stale records; both batches through
    the table walker against the oracle"""
    case = LC.case_sg()
    print("SG", case.measured)
    assert case.measured["stale"] >= 60 and case.measured["listed_without"] >= 30
    check_against_the_oracle(case, coverage(case, (0, NC)))


def test_case_lists_an_empty_list_between_two_that_are_not_and_a_single_entry():
    case = LC.case_lists()
    print("lists", case.measured)
    lists = case.measured["lists"]
    assert lists[0] > 1 and lists[1] == 0 == lists[2] and lists[3] == 1
    check_against_the_oracle(case, coverage(case, (0, NC)))


def test_case_sh_need_bits_of_exactly_one_of_both_and_of_none():
    """set H: two gap passes with factors of their own on one owner's walk list (the builder asserts the bits from the walks)"""
    case = LC.case_sh()
    print("SH", case.measured)
    check_against_the_oracle(case, coverage(case, (0, NC)))


def test_case_so_gap_passes_with_lists_of_their_own():
    case = LC.case_so()
    print("SO", case.measured)
    check_against_the_oracle(case, coverage(case, (0, NC)))


# what no case walks, and why (everything else the hooks report must be walked: the test below)
UNREACHED = {
    # (set, flags, pass, tier, dense mode, tier, loop, threads, hot bytes): reason
}
for _p in (0, 1, 3):  # not built: a batch that flags more than half of a slab of the host, the url and the user_agent arena of set Q
    for _t in (LC.HOT, LC.COLD):
        UNREACHED[("Q", 0, _p, 0, 1, _t, "async", 512, 48 * 1024)] = "set Q's dense alternatives: no dense batch is built for it (D, DL, DG, DH, DO walk the other sets')"
SENT = {"M": ["T", "W", "S", "D", "P63", "P513"], "L": ["TL", "DL"], "G": ["SG", "DG"], "H": ["SH", "DH"], "O": ["SO", "DO"], "Q": ["lists", "TQ"]}


def test_every_tier_loop_and_launch_shape_the_hooks_report_is_walked():
    """the combinations are DERIVED from pwaf_program_list_scans for every set the device suite sends, as built and without the confirm
    tier -- per descriptor the tiers it stages or leaves cold, the loops it can take (lscan_cases.loops_of), its launch shape -- and
    each must be walked by a case of the set: the tier by the model's labels over the requests the descriptor walks, the loop by the
    length of its list against n / 8. (The identity and gate passes of other fields than the set's own are left to the cases' verdicts.)"""
    import copy

    sets = {"M": LC.set_m(), "L": LC.set_l(), "G": LC.set_g(), "H": LC.set_h(True), "O": LC.set_h(False), "Q": LC.set_q()}
    cases = dict(LC.CASES, P63=lambda: LC.case_p(63), P513=lambda: LC.case_p(513))
    need, got = {}, {}
    for name, rs0 in sets.items():
        fields = [_abi.FIELD_NAMES.index(f) for f in LC.Q_FIELDS] if name == "Q" else [rs0.field_id]
        for fid in fields:
            rs = copy.copy(rs0)
            rs.field_id = fid
            for flags in (0, NC):
                for d in LC.descriptors_of(rs.program(flags), fid):
                    m = rs.model(rs.program(flags), d["pass"], d["tier"])
                    for c in LC.combinations(d, m):
                        need[(name, flags, d["pass"], d["tier"], d["dense_mode"]) + c] = None
            for cname in SENT[name]:
                case = cases[cname]()
                dense = cname.startswith("D")
                for label, batch in case.batches:
                    only = None
                    if cname.startswith("P"):
                        only, _ = LC.candidates_by_model(rs, batch, NC)
                    for flags in ((0,) if dense else (0, NC)):
                        cov = LC.Coverage(rs, flags, batch, dense=dense, only=only)
                        # (a list behind a prefilter holds every request some pass of the field walks: an owner's walk list also the requests
                        # a LITERAL factor of a sharing gap pass put there, which the table walker sends through the gap pass alone)
                        listed = sum(1 for i in cov.only if cov.walked[i])
                        for d, m, n_walked, count in cov.rows:
                            long_list = d["dense_mode"] == 1 or (d["behind_filter"] and 8 * max(listed, n_walked) >= batch.n)
                            tiers = {LC.HOT: any(count.get((LC.HOT, p), 0) for p in range(4)), LC.COLD: any(count.get((LC.COLD, p), 0) for p in range(4)),
                                     "rec": any(count.get((lab, p), 0) for lab in (LC.EX1, LC.EX2, LC.BASE) for p in range(4))}
                            for t, seen in tiers.items():
                                if seen:
                                    got.setdefault((name, flags, d["pass"], d["tier"], d["dense_mode"], t, "async" if long_list else "lockstep", d["threads"], d["hot_bytes"]), cname)
    missing = sorted(k for k in need if k not in got and k not in UNREACHED)
    for k in sorted(need):
        print(k, got.get(k, UNREACHED.get(k)))
    assert not missing, missing
    assert all(k in need for k in UNREACHED), "an entry of UNREACHED names a combination the hooks do not report"
