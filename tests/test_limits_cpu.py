"""The engine's capacity limits on the CPU (no device): rule sets pinned to exact scan-pass counts (helpers.pinned_passes) at the
250-pass limit and around the 64-pass, 128-pass and 32-gap-pass boundaries, and the split of the list-scan launches
(csrc/lscan_split.h: at most 256 descriptors per launch_scan_gated call) through the very header pipeline.cpp plans them with."""
import json
import os
import subprocess

import pytest

import helpers as H
from pingoo_amd.engine import CompiledProgram, UnsupportedExpression

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "lscan_split_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "pingoo_amd", "csrc", "lscan_split.h")]

# one rule on a header no other rule reads: a field of its own is a pass of its own
ONE_MORE_PASS = ("one_more", 'http_request.headers["x-limit-probe"].contains("qq")', [H.B])


def _refused_past_250(rules, opts):
    with pytest.raises(UnsupportedExpression) as ei:
        CompiledProgram(rules, **opts)
    assert ei.value.rule_index is None, ei.value.rule_index
    assert "250" in str(ei.value), str(ei.value)


def _mix_extra():
    ident, _ = H.kind_rules("identity", 3, prefix="x")
    lit, _ = H.kind_rules("confirm_literal", 40, seed=3, prefix="x")
    gap, _ = H.kind_rules("gap", 12, seed=3, prefix="x")
    return ident + lit + gap


@pytest.mark.parametrize("case", ["confirm_walk", "gap", "mix"])
def test_250_passes_compile_and_251_are_refused(case):
    if case == "confirm_walk":
        extra = ()
    elif case == "gap":
        extra = tuple(H.kind_rules("gap", 70, seed=5, prefix="x")[0])  # counted gaps (at this table budget: passes behind a prefilter, not gated)
    else:
        extra = tuple(_mix_extra())
    at = H.pinned_passes("confirm_walk", 250, extra=extra)
    assert at.n_passes == 250
    if case == "mix":
        assert at.n_confirm > at.n_walk + 1 and at.n_confirm < 250, (at.n_confirm, at.n_walk)  # (literal passes without walk, identity passes)
    # the probe rule adds exactly one pass: 249 + 1 compile to 250 ...
    below = H.pinned_passes("confirm_walk", 249, extra=extra)
    assert CompiledProgram(below.rules + [ONE_MORE_PASS], **below.opts).stats()["n_dfa_groups"] == 250
    # ... and 250 + 1 are refused at compilation, with no rule to blame and the limit named
    _refused_past_250(at.rules + [ONE_MORE_PASS], at.opts)


@pytest.mark.parametrize("n", [61, 62, 63, 127, 128, 129, 250])
def test_pinned_confirm_walk_counts_are_exact(n):
    ps = H.pinned_passes("confirm_walk", n)
    assert ps.n_passes == n
    # every pass has a confirm tier; all but the built-in captcha-path pass (a literal) walk
    assert ps.n_confirm == n and ps.n_walk == n - 1, (ps.n_confirm, ps.n_walk)
    assert CompiledProgram(ps.rules, **ps.opts).stats()["n_dfa_groups"] == n  # (deterministic: the same set compiles the same again)
    # the tokens make the rules' literals occur: the whole match flags some pass behind the prefilter
    for k in (0, len(ps.rules) // 2, len(ps.rules) - 1):
        assert ps.pass_of_input(ps.tokens[k][1][0].encode()), ps.rules[k]


@pytest.mark.parametrize("n", [31, 32, 33, 40])
def test_pinned_gap_counts_are_exact(n):
    ps = H.pinned_passes("gap", n)
    assert ps.n_gated == n
    # the counted gaps' literal factors live in filtered passes (those feed the gap passes' lists)
    assert ps.n_filtered >= 1 and ps.n_passes == n + ps.n_filtered, (ps.n_passes, ps.n_filtered)


def test_pinned_search_names_the_nearest_counts_when_it_fails():
    with pytest.raises(AssertionError, match="nearest counts found"):
        H.pinned_passes("confirm_walk", 251, max_seeds=1, max_tries=3)  # (251 passes are refused: never reached)


# ---------------------------------------------------------------------------------------------------------
# the list-scan launch split (csrc/lscan_split.h)
# ---------------------------------------------------------------------------------------------------------
def split_tool():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "lscan_split_host")
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", out], check=True)
    return out


# (identity, gated, filtered, confirm, confirm_walk, dense_alt) of the pass kinds run_pipeline distinguishes
WALK2 = (0, 1, 1, 1, 1, 1)     # a confirm pass that walks, dense switch on: dense alternative + R-tier walk
WALK1 = (0, 1, 1, 1, 1, 0)     # ... PWAF_OPT_NO_DENSE_SWITCH: the walk alone
LIT1 = (0, 1, 1, 1, 0, 1)      # a confirm pass without walk: the dense alternative alone
NOCONF = (0, 1, 1, 0, 0, 1)    # behind a prefilter without confirm tier (PWAF_OPT_NO_CONFIRM): its candidate walk
IDENT = (1, 0, 0, 0, 0, 0)     # a plain pass over a short field: the identity list
GAP = (0, 1, 0, 0, 0, 0)       # a gated gap pass (phase 1)
PLAIN = (0, 0, 0, 0, 0, 0)     # walks every request in the streaming scan kernel: no list-scan descriptor


def plan(passes):
    r = subprocess.run([split_tool()], input="".join(" ".join(map(str, p)) + "\n" for p in passes), capture_output=True, text=True, timeout=60, check=True)
    return json.loads(r.stdout)


def check_plan(passes):
    out = plan(passes)
    cap = out["max_per_launch"]
    assert cap == 256
    words = 0
    for phase in (0, 1):
        per, launches = out["per_pass"][phase], out["launches"][phase]
        assert all(0 <= d <= 2 for d in per)
        total = sum(per)
        # every descriptor launched exactly once, in order; no launch empty or above the plan kernel's 256 threads
        assert sum(launches) == total and all(0 < c <= cap for c in launches), (launches, total)
        # a pass's descriptors (dense alternative + walk) never straddle two launches: every launch boundary is a pass boundary
        ends = set()
        acc = 0
        for d in per:
            acc += d
            ends.add(acc)
        acc = 0
        for c in launches:
            acc += c
            assert acc in ends, (launches, per)
        # greedy: no launch could have taken the next pass as well
        acc = 0
        for i, c in enumerate(launches[:-1]):
            acc += c
            nxt = next(d for d, e in zip(per, _prefix(per)) if e > acc and d)
            assert c + nxt > cap, (launches, i)
        # one launch whenever the phase fits one: a rule set below the limit keeps its launch chain
        if 0 < total <= cap:
            assert launches == [total]
        words += sum(2 * c + 1 for c in launches)
    # the plan regions laid one behind the other fill exactly what run_pipeline reserves (lsplit::plan_words)
    assert out["plan_words"] == words
    return out


def _prefix(per):
    acc, out = 0, []
    for d in per:
        acc += d
        out.append(acc)
    return out


@pytest.mark.parametrize("count", [0, 1, 255, 256, 257, 500])
def test_list_scan_split_at_descriptor_counts(count):
    passes = [WALK2] * (count // 2) + [IDENT] * (count % 2) + [PLAIN, GAP, GAP]
    out = check_plan(passes)
    assert sum(out["launches"][0]) == count and out["launches"][1] == [2]
    assert len(out["launches"][0]) == (0 if count == 0 else 1 if count <= 256 else 2)


def test_list_scan_split_at_250_confirm_passes_plus_identity_passes():
    passes = [WALK2] * 250 + [IDENT] * 4 + [GAP] * 32
    out = check_plan(passes)
    assert out["launches"][0] == [256, 248] and out["launches"][1] == [32]
    # identity passes between confirm passes, odd counts, every kind of pass: still whole passes per launch
    mixed = [WALK2, LIT1, IDENT, WALK1, NOCONF, PLAIN, GAP] * 60
    out = check_plan(mixed)
    assert len(out["launches"][0]) >= 2
    assert out["launches"][0][0] in (255, 256)


def _program_passes(prog, dense=True):
    """the pass kinds of a compiled program, taking for every pass the MOST descriptors the engine can give it (tuning may turn a plain
    pass into an identity pass or move prefilters)"""
    from table_walker import Tables

    kinds = []
    for g in Tables(prog.dump()).groups:
        if g.get("filter_cols"):
            kinds.append(GAP)
        elif "f_table" in g:
            kinds.append((0, 1, 1, 1, 1, 1 if dense else 0))
        else:
            kinds.append(IDENT)
    return kinds


@pytest.mark.parametrize("config", [3, 5])
def test_benchmark_rule_sets_never_split_their_list_scans(config):
    """The benchmark's rule sets (BASELINE configs 3 and 5) stay far below 256 descriptors per phase even when every filtered pass is
    counted with both descriptors: their launch chain is one list-scan launch per phase, as before the split existed."""
    from synth import pysynth

    wl = pysynth.Workload(config)
    prog = CompiledProgram(wl.rules, wl.lists, wl.geoip)
    out = check_plan(_program_passes(prog))
    assert all(len(ls) <= 1 for ls in out["launches"]), out["launches"]
    assert sum(out["launches"][0]) <= 160, out["launches"]


def test_the_182_pass_confirm_set_needs_two_phase_0_launches():
    """The shape the split exists for: every one of ~180 passes has a confirm tier that walks — two descriptors each, more than 256."""
    ps = H.pinned_passes("confirm_walk", 182)
    out = check_plan(_program_passes(ps.program))
    assert sum(out["launches"][0]) == 2 * 182 and len(out["launches"][0]) == 2
    # without the dense switch one descriptor per pass: one launch
    out = check_plan(_program_passes(ps.program, dense=False))
    assert out["launches"][0] == [182]
