"""The verdict kernel's launch shape and the cases of its edge suite, without a device (docs/verdict_edges.md).

The shape: csrc/verdictplan.h's verdict_shape through the host harness tests/verdictplan_host.cpp over sizes up to the limits, checked
against what the kernels rely on (the slot-byte encoding, 160 KiB of LDS, the waves their launch bounds are compiled for) and a
restatement of the capacity choice written here from the function's comment; the hook pwaf_program_verdict_shape against the harness.

The cases (tests/verdict_cases.py): every target of the group model is reached at the capacity the hook reports, the numpy reference
equals pyoracle.Oracle on every base request, the tiling of the turn cases puts every ordered pair of group states on one wave."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import verdict_cases as VC
from oracle import pyoracle
from pingoo_amd import _abi
from pingoo_amd.engine import CompiledProgram, PwafError
from plan_harness import tool as plan_tool

HERE = os.path.dirname(os.path.abspath(__file__))
LDS = 160 * 1024
CAPS = (254, 224, 192, 160, 128, 96, 64)
OUT = ("waves", "lds_bytes", "lds_tables", "sparse", "v_cap", "per_cu", "launchable", "bit_regs", "blocks304", "wave_el")


def shapes(sizes):
    """sizes: [(n_cols, n_rules, n_trig, n_lits, force_global, mode, n_passes)] -> [dict by OUT]"""
    exe = plan_tool("verdictplan_host", os.path.join(HERE, "verdictplan_host.cpp"), [])
    r = subprocess.run([exe], input="".join(" ".join(str(int(x)) for x in s) + "\n" for s in sizes), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [dict(zip(OUT, (int(x) for x in line.split()))) for line in r.stdout.splitlines()]
    assert len(rows) == len(sizes)
    return rows


# ---- the layout and the capacity choice, restated from the comments of verdictplan.h ----
def up(x, a):
    return (x + a - 1) // a * a


def tables_bytes(n_cols, n_rules, n_trig, n_lits):
    """trigger offsets (u16, n_cols + 1), trigger rules (u16), rule headers (8 bytes), literals (4), public indices (u16)"""
    return up((n_cols + 1) * 2, 4) + up(n_trig * 2, 8) + n_rules * 8 + n_lits * 4 + up(n_rules * 2, 4)


def wave_el(n_cols, n_rules, cap):
    """vals | rule bitmap | entry columns (u16) | candidates (u16) | slot bytes"""
    return up(cap * 8 + (n_rules + 31) // 32 * 4 + up(cap * 2, 4) + up(n_rules * 2, 4) + up(n_cols, 8), 16)


def occupancy(n_cols, n_rules, n_trig, n_lits, force_global, n_passes, cap):
    """(waves, workgroups per CU, tables in LDS): as many 12-wave workgroups per CU as LDS holds, at most 24 (16 beyond 64 passes) waves per
    CU; the tables in LDS when eight waves still fit beside them"""
    wave, t = wave_el(n_cols, n_rules, cap), tables_bytes(n_cols, n_rules, n_trig, n_lits)
    lt = not force_global and n_trig < 65536 and t + 8 * wave <= LDS
    tables = t if lt else 0
    best = (0, 1)
    for k in (1, 2, 3):
        share = LDS // k
        if share <= tables + wave:
            continue
        w = min(12, (24 if n_passes <= 64 else 16) // k, (share - tables) // wave)
        if w * k > best[0] * best[1]:
            best = (w, k)
    return best[0], best[1], int(lt)


def chosen_capacity(*size):
    """the largest of the seven capacities that keeps the occupancy capacity 64 reaches"""
    w0, k0, _ = occupancy(*size, 64)
    for cap in CAPS:
        w, k, _ = occupancy(*size, cap)
        if w * k >= w0 * k0:
            return cap
    raise AssertionError("capacity 64 reaches its own occupancy")


def sweep():
    cols = (1, 2, 63, 64, 1000, 4500, 20000, 50000, 65535, 65536)
    out = []
    for n_cols, n_rules, passes, mode, fg in itertools.product(cols, (1, 3, 1024, 2048, 2100, 10000, 30000, 65519), (1, 64, 65, 252), range(5), (0, 1)):
        for n_trig in sorted({0, n_rules, 3 * n_rules, 65535, 65536, 200000}):
            for n_lits in (n_rules, 4 * n_rules):
                out.append((n_cols, n_rules, n_trig, n_lits, fg, mode, passes))
    return out


def test_the_shape_over_sizes_up_to_the_limits():
    sizes = sweep()
    rows = shapes(sizes)
    seen_caps, refused, launchable = set(), 0, 0
    for (n_cols, n_rules, n_trig, n_lits, fg, mode, passes), r in zip(sizes, rows):
        what = (n_cols, n_rules, n_trig, n_lits, fg, mode, passes, r)
        assert r["launchable"] == (1 if r["waves"] != 0 and n_cols < 65536 else 0), what
        assert r["bit_regs"] == (1 if passes <= 64 else 4), what
        if n_trig >= 65536 or fg:
            assert r["lds_tables"] == 0, what
        if r["waves"] == 0:
            refused += 1
            continue
        launchable += r["launchable"]
        assert r["lds_bytes"] <= LDS, what
        assert r["waves"] * r["per_cu"] <= (24 if passes <= 64 else 16) if mode else r["waves"] <= 16 and r["per_cu"] == 1, what
        assert r["blocks304"] == 304 * r["per_cu"], what
        if mode >= 3:
            # a slot byte is 1 + entry index, 255 = spilled: entry indices 0 .. 253
            assert r["sparse"] == 2 and r["v_cap"] <= 254 and r["waves"] <= 12, what
            assert r["wave_el"] == wave_el(n_cols, n_rules, r["v_cap"]), what
            size = (n_cols, n_rules, n_trig, n_lits, fg, passes)
            cap = 8 if mode == 4 else chosen_capacity(*size)
            assert r["v_cap"] == cap and (r["waves"], r["per_cu"], r["lds_tables"]) == occupancy(*size, cap), (what, cap, occupancy(*size, cap))
            t = tables_bytes(n_cols, n_rules, n_trig, n_lits) if r["lds_tables"] else 0
            assert r["lds_bytes"] == t + r["waves"] * r["wave_el"], what
            seen_caps.add(r["v_cap"])
    assert seen_caps == set(CAPS) | {8}, seen_caps  # (every capacity of the seven is some size's choice)
    assert refused > 100 and launchable > 10000, (refused, launchable)
    # what pwaf_engine_create refuses does not depend on the pass count: it asks with the batches' own
    by_size = {}
    for s, r in zip(sizes, rows):
        by_size.setdefault(s[:6], set()).add(r["launchable"])
    assert all(len(v) == 1 for v in by_size.values())


def test_the_cases_know_the_kernels_prefetch_depth():
    """kPre of verdict2_kernel — what 'kPre, kPre + 1 non-empty passes' and 'the rest loop' stand at — is read from the sources"""
    import re
    csrc = os.path.join(os.path.dirname(HERE), "pingoo_amd", "csrc")
    general = int(re.search(r"static constexpr int kVerdictPre = (\d+);", open(os.path.join(csrc, "kernels.h")).read()).group(1))
    hip = open(os.path.join(csrc, "verdict.hip")).read()
    body = hip[hip.index("void verdict2_kernel(VerdictArgs a)"):]
    m = re.search(r"constexpr int kPre = BR == 1 \? (\d+) : kVerdictPre;", body)
    assert m is not None and VC.K_PRE_BY_BR == {1: int(m.group(1)), 4: general}
    assert re.search(r"constexpr int kBRmax = \(kMaxPasses \+ 1 \+ 63\) / 64;", hip) and "kMaxPasses = 250" in open(os.path.join(csrc, "kernels.h")).read()  # (BR = 4)
    assert VC.k_pre(64) == VC.K_PRE_BY_BR[1] and VC.k_pre(65) == VC.K_PRE_BY_BR[4]


def test_the_tables_leave_lds_at_65536_triggers():
    # 65535 triggers (128 KiB of 16-bit rule indices) fit beside eight small waves; one more no longer has a 16-bit offset
    for mode in (3, 4, 1, 0):
        (a, b) = shapes([(64, 32, 65535, 64, 0, mode, 3), (64, 32, 65536, 64, 0, mode, 3)])
        assert a["lds_tables"] == 1 and a["waves"] > 0 and tables_bytes(64, 32, 65535, 64) < a["lds_bytes"] <= LDS, (mode, a)
        assert b["lds_tables"] == 0 and b["waves"] > 0 and b["lds_bytes"] < tables_bytes(64, 32, 65535, 64), (mode, b)
    (c, d) = shapes([(1000, 1024, 20000, 4096, 0, 3, 3), (1000, 1024, 20000, 4096, 1, 3, 3)])
    assert c["lds_tables"] == 1 and d["lds_tables"] == 0 and d["lds_bytes"] < c["lds_bytes"]


SETS = ["A", "C", "W", "P8", "P65", "Z", "H"]
LEG_FLAGS = (0, VC.TINY, VC.GLOBAL, VC.TINY | VC.GLOBAL, VC.HITS, VC.SPARSE, VC.DENSE)


@pytest.mark.parametrize("name", SETS)
def test_the_hook_answers_what_the_harness_answers(name):
    rs = VC.rule_set(name)
    for flags, routed in [(f, False) for f in LEG_FLAGS] + [(0, True)]:
        prog = rs.program(flags, routed)
        got = prog.verdict_shape()
        plan, tabs = rs.tables(flags, routed)  # (routed: the harness plans the rules AND the routes, as pwaf_engine_create_routed does)
        if True:
            mode = {0: 3, VC.TINY: 4, VC.SPARSE: 1, VC.DENSE: 0}[flags & (VC.TINY | VC.SPARSE | VC.DENSE)]
            n_lits = len(plan.dev_lits)
            (r,) = shapes([(plan.n_cols, len(plan.rules), plan.n_trig, n_lits, 1 if flags & VC.GLOBAL else 0, mode, got["n_passes"])])
            assert (got["mode"], got["capacity"], got["waves"], got["per_cu"], got["lds_tables"], got["lds_bytes"], got["bit_regs"]) == \
                (mode, r["v_cap"], r["waves"], r["per_cu"], r["lds_tables"], r["lds_bytes"], r["bit_regs"]), (flags, got, r)
            assert got["n_passes"] == len(tabs.groups) + (1 if plan.n_residual else 0) and got["bit_regs"]  # (+ the residual rules' pseudo pass)
            assert got["bit_regs"] == (1 if got["n_passes"] <= 64 else 4)
        assert got["waves"] > 0 and (got["capacity"] <= 254 if got["mode"] >= 3 else True)
    with pytest.raises(PwafError, match="pwaf_program_verdict_shape"):
        CompiledProgram._borrow(None).verdict_shape()


@pytest.mark.parametrize("name", SETS)
def test_the_numpy_reference_equals_the_oracle_on_every_base_request(name):
    c = VC.case(name)
    rs = c.rs
    want = pyoracle.Oracle(rs.rule_tuples(), rs.lists).evaluate(c.batch)
    bad = np.nonzero((want["action"] != c.want["action"]) | (want["rule_idx"] != c.want["rule_idx"]))[0]
    assert len(bad) == 0, (len(bad), int(bad[0]), want[bad[0]], c.want["action"][bad[0]], c.want["rule_idx"][bad[0]])
    assert c.batch.n == c.T.shape[1] and c.batch.n % 64 == 37 and set(c.want["action"].tolist()) == ({1, 2, 3} if name in "AWH" else {0, 1, 2} if name == "Z" else {0, 1, 2, 3})
    assert 0.25 < c.ver.mean() < 0.4
    # the rules that decide somebody include compound rules and a negation-only rule
    decided = set(c.want["rule_idx"].tolist())
    if name.startswith("P") or name == "Z":
        return
    assert any(r < rs.atom_rule0 for r in decided) and any(rs.atom_rule0 + VC.N_ATOMS <= r < len(rs.rules) - 3 for r in decided), sorted(decided)[-5:]
    for k, (_, dnf, _) in enumerate(rs.rules):  # the negation-only rules and (set A) the match-all rule decide somebody
        if dnf is None or all(neg for t in dnf for _, neg in t):
            assert k in decided or (name != "W" and k == len(rs.rules) - (2 if name in "AH" else 1)), k
    # routes: the oracle of the routes as rules answers the first route
    ro = pyoracle.Oracle([(n, e, [VC.B]) for n, e in rs.route_tuples()], rs.lists, flags=_abi.OPT_NO_UA_GATE | _abi.OPT_NO_CAPTCHA_BYPASS).evaluate(c.batch)
    assert (np.where(ro["rule_idx"] == _abi.RULE_NONE, -1, ro["rule_idx"].astype(np.int64)) == c.route).all() and (c.route >= 0).sum() > 20


@pytest.mark.parametrize("name", SETS)
def test_every_target_is_reached_at_the_capacity_the_hook_reports(name):
    c = VC.case(name)
    for flags in (0, VC.TINY, VC.GLOBAL, VC.TINY | VC.GLOBAL, VC.HITS):
        VC.assert_targets(c, flags)
    if name == "Z":
        return
    ms = c.models(0)
    assert ms[0].e_cap == c.rs.program(0).verdict_shape()["capacity"] and c.models(VC.TINY)[0].e_cap == 8
    # a group of the model and its kind agree where the kind names a figure
    for g, m in zip(c.groups, ms):
        if g.kind.startswith("pairs") and "+" not in g.kind and not name.startswith("P"):
            assert m.n_pairs == int(g.kind[5:]) and m.n_entries == 1 + m.n_pairs, g.kind
        if g.kind.startswith("nothing"):
            assert m.n_entries == 1 and m.n_pairs == 0 and not m.passes
    assert name.startswith("P") or VC.targets(c, 0)["spilled, full and clean groups"]


@pytest.mark.parametrize("flags", [0, VC.TINY], ids=["as built", "tiny slots"])
@pytest.mark.parametrize("name", ["A", "C"])
def test_the_tiling_puts_every_pair_of_states_on_one_wave_for_8_to_304_compute_units(name, flags):
    c = VC.case(name)
    ms = c.models(flags)[:-1]  # (whole groups; the states at the leg's own capacity)
    sh = c.rs.program(flags).verdict_shape()
    states, columns = [m.state for m in ms], [m.columns for m in ms]
    seq = VC.turn_sequence(states, columns)
    assert sorted(set(seq)) == list(range(len(ms)))
    for cus in list(range(8, 305, 8)) + [9, 31, 104, 110, 228, 255, 303]:
        stride = cus * sh["per_cu"] * sh["waves"]
        kinds = VC.turn_groups(seq, stride)
        idx = VC.turn_indices(kinds)
        assert len(kinds) > 2 * stride and len(idx) == 64 * len(kinds) and idx.max() < 64 * len(ms) and (idx[::64] // 64 == kinds).all()
        # from the tiled batch's own group list: every ordered pair of states on some wave in consecutive turns, under the column conditions;
        # some wave takes a third group
        got = {(states[i], states[j]) for i, j in VC.turn_pairs(kinds, stride) if VC.pair_ok(states[i], states[j], columns[i], columns[j])}
        assert len(got) == 9, (cus, got)
        assert len(kinds) - 2 * stride >= 1
