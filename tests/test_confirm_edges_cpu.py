"""The resolve / confirm edge cases (tests/confirm_cases.py) on the host: the numpy model of filter_kernel that every case proves its shape
with agrees with the per-field restatement (table_walker.Tables.filter_flags); every case is BUILT here and its shape assertions made
-- with the model and pwaf_program_confirm_shape, by the same functions the device suite calls -- so a shape that cannot be reached
fails on the CPU; where a case's requests can be judged one field at a time, the host form of the confirm tier
(pwaf_program_confirm_field: csrc/confirm.h, the code the device compiles) gives the oracle's verdicts."""
import random

import numpy as np
import pytest

import confirm_cases as CC
import table_walker
from oracle import pyoracle
from pingoo_amd import _abi
from pingoo_amd.engine import CompiledProgram, PwafError

LEG_FLAGS = {"as built": 0, "stride 2": _abi.OPT_FILTER_STRIDE2, "no dense switch": _abi.OPT_NO_DENSE_SWITCH, "rule hits": _abi.OPT_RULE_HITS}


def test_the_shape_hook_reports_the_tables_and_refuses_a_pass_without_a_confirm_tier():
    rs = CC.set_s()
    gi, g = rs.pass_of()
    cs = rs.confirm_shape()
    assert cs["entries"] == g["confirm_entries"] > len(CC.S_LITS) and cs["longest"] == 5 and cs["has_walk"] == 1  # (the literals and the regex's factor)
    assert cs["top_class_pos"] == 2 and cs["widest_bin"] >= 1  # "zz[0-9]y": the class is the factor's byte 2
    assert cs["bytes"] % 4 == 0 and cs["bytes"] >= sum(2 * ((len(x) + 3) & ~3) for x in CC.S_LITS) and cs["class_words"] % 8 == 0
    assert cs["in_lds"] == int(cs["entries"] * 3 + cs["bytes"] // 4 + cs["class_words"] <= CC.POOL_WORDS) == 1
    prog = rs.program()[0]
    with pytest.raises(PwafError):
        prog.confirm_shape(len(rs.program()[1].groups))  # no such pass
    off = CompiledProgram(rs.verdict_rules, {}, flags=_abi.OPT_NO_CONFIRM)
    with pytest.raises(PwafError):
        off.confirm_shape(gi)  # filtered, without a confirm tier
    plain = CompiledProgram(rs.verdict_rules, {}, flags=_abi.OPT_NO_PREFILTER)
    with pytest.raises(PwafError):
        plain.confirm_shape(0)  # not filtered


def test_the_arena_model_agrees_with_the_per_field_model_at_every_offset_and_both_strides():
    rng = random.Random(77)
    strides = set()
    for rs, lits in ((CC.set_s(), CC.S_LITS), (CC.set_s2(), CC.S2_LITS),
                     (CC.set_h(), list(CC.H_CONTAINS.values()) + [CC.H_LIT5, CC.H_LIT20, CC.H_FOLD] + CC.I_LITS[:5])):
        for flags in (0, _abi.OPT_FILTER_STRIDE2):
            prog, t = rs.program(flags)
            gi, g = rs.pass_of(flags)
            strides.add(g["f_stride"])
            fields = []
            for _ in range(150):
                parts = []
                for _ in range(rng.randint(0, 3)):
                    lit = rng.choice(lits)
                    parts.append(rng.choice([lit, lit[:-1], lit[1:], CC.wrong(lit, len(lit) - 1), lit.upper()]))
                    parts.append("".join(rng.choice("aqz.#k/=") for _ in range(rng.randint(0, 9))))
                fields.append("".join(parts).encode())
            for o in range(16):
                t.arena_offset = o
                for data in fields[o::4]:
                    want = t.filter_flags(g, data)
                    arena = np.frombuffer(b"~" * o + data + b"~" * 32, dtype=np.uint8)
                    w = CC.window_positions(g, arena, len(arena) - 16)
                    first = (o + 1) & ~1 if g["f_stride"] == 2 else o  # (the field's first sampled byte)
                    got = set((np.nonzero(w[first:o + len(data)])[0] + first) // 16) if len(data) else set()
                    assert got == want, (rs.name, flags, o, data, sorted(got), sorted(want))
            t.arena_offset = 0
    assert strides == {1, 2}, strides


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_every_case_reaches_its_shape(name):
    """(the builders assert their shapes themselves; here also: the legs' own tables keep the case on the confirm path)"""
    case = CC.CASES[name]()
    print(name, {k: v for k, v in case.measured.items() if k != "observed"})
    legs = LEG_FLAGS
    for label, batch in case.batches:
        base = case.rs.shape(batch)
        for leg, flags in legs.items():
            sh = case.rs.shape(batch, flags)
            CC.below_dense(sh, f"{name}, {leg}")
            if flags in (_abi.OPT_RULE_HITS, _abi.OPT_NO_DENSE_SWITCH):
                assert (sh.chunks == base.chunks).all() if sh.pairs == base.pairs else False, f"{name}, {leg}: the leg's filter flags other chunks than the engine as built"
    # the oracle's verdicts are not all alike: the case observes hits and misses
    want = pyoracle.Oracle(case.rs.verdict_rules, {}).evaluate(case.batches[0][1])
    assert len(set(want["action"].tolist())) >= 2, name


def test_case_j_reaches_its_shape():
    case, times = CC.case_j()
    print("J", case.measured)
    assert times * 4 * 48 < 2 ** 31
    want = pyoracle.Oracle(case.rs.verdict_rules, {}).evaluate(case.batches[0][1])
    assert want["action"].tolist() == [1, 0, 1, 0]


@pytest.mark.parametrize("name", ["B", "H", "I"])
def test_single_field_cases_through_the_host_form_of_the_confirm_tier(name):
    """the cases whose probes lie alone in their chunks: the table interpreter, which runs the filter and the confirm tier of one field
    through pwaf_program_confirm_field, gives the oracle's verdict for every probe, at three offsets of a chunk"""
    case = CC.CASES[name]()
    batch = case.batches[0][1]
    want = pyoracle.Oracle(case.rs.verdict_rules, {}).evaluate(batch)
    prog, t = case.rs.program()
    off = batch.offsets[case.rs.field_id]
    filler = CC.Arena.filler_head.encode()
    picked = [i for i in range(batch.n) if not batch.field_bytes(case.rs.field_id, i).startswith(filler)]
    assert len(picked) > 100
    hits = 0
    for i in picked[:: max(1, len(picked) // 400)]:
        t.arena_offset = int(off[i]) % 16
        got = t.evaluate(batch, i)
        assert got == (int(want[i]["action"]), int(want[i]["rule_idx"])), (name, i, batch.field_bytes(case.rs.field_id, i), got, want[i])
        hits += got[0] != 0
    t.arena_offset = 0
    assert hits > 10 and t.n_confirm_hits > 0


def test_which_side_of_the_lds_pool_the_synthetic_workloads_fall_on():
    """Workload 3's largest confirm pass (428 entries, 4 057 words) is compared from LDS; workload 5's largest (1 240 entries, 11 628
    words against the pool's 10 240) is compared from global memory: confirm_entry<1> is on the benchmark's path for config 5."""
    from synth import pysynth

    sides = {}
    for cfg in (3, 5):
        wl = pysynth.Workload(cfg)
        prog = CompiledProgram(wl.rules, wl.lists, wl.geoip)
        shapes = []
        for gi in range(prog.stats()["n_dfa_groups"]):
            try:
                shapes.append(prog.confirm_shape(gi))
            except PwafError:
                pass
        top = max(shapes, key=lambda cs: cs["entries"])
        assert top["in_lds"] == int(top["entries"] * 3 + top["bytes"] // 4 + top["class_words"] <= CC.POOL_WORDS)
        sides[cfg] = (top["entries"], top["in_lds"], sum(1 for cs in shapes if not cs["in_lds"]))
    assert sides[3][:2] == (428, 1) and sides[3][2] == 0, sides
    assert sides[5][:2] == (1240, 0), sides
