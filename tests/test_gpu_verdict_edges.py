"""verdict2_kernel's entry list at its edges on the device (docs/verdict_edges.md). The cases are built by tests/verdict_cases.py, whose
group model proves on the host — from the program's tables and the shape hook, before anything is sent — that the batch holds groups of
n_entries = capacity - 1, capacity and capacity + 1 reached through each append site, an append_batch that straddles the capacity, the
pair counts around 64 and 128, overflow chains that merge into LDS and into spilled entries, and a chain that appends the entry that
spills; tests/test_verdict_edges_cpu.py makes the same assertions without a device and pins the reference to the oracle.

Legs: each set as built, with 8 entry slots (PWAF_OPT_TINY_VERDICT_SLOTS), with the program tables in global memory, with both; on a
PWAF_OPT_RULE_HITS engine (the whole hit matrix and the per-rule counts); on a routed engine (the first route). The sparse and the dense
column file run the same batches: a case that fails only on the entry list is an entry-list bug. Set H (rules without actions, which only
a rule-hits engine keeps) runs on the rule-hits leg alone; set C also runs without prefilters, where one lane walks a request's field and
the step at which a chain names an atom is defined by the field.

Every leg: (action, rule_idx) of every request and the four counters against the numpy reference written from the rule list, the match
compaction of the device-resident call (match_idx as a set, n_matches), batches of 1, 63, 64, 65 and 129 requests, then a small batch
and the case again on the same engine (stale spill words and slot bytes across batches). The engine's program answers the shape the
case was proved for, and the launch list shows the verdict kernel once per batch.

The turn cases tile the base groups past the persistent grid of THIS device (compute units x workgroups per CU x waves), so that every
wave takes a second group and some a third, in an order that puts every ordered pair of {clean, exactly full, spilled} on some wave."""
import numpy as np
import pytest

import helpers as H
import verdict_cases as VC
from pingoo_amd import _abi
from pingoo_amd.engine import DeviceBatch, RuleEngine

pytestmark = pytest.mark.gpu
LEGS = {"as built": (0, False), "tiny slots": (VC.TINY, False), "global tables": (VC.GLOBAL, False), "tiny slots, global tables": (VC.TINY | VC.GLOBAL, False),
        "rule hits": (VC.HITS, False), "routed": (0, True), "sparse column file": (VC.SPARSE, False), "dense column file": (VC.DENSE, False)}
SIZES = (1, 63, 64, 65, 129)


def make_engine(rs, flags, routed):
    eng = RuleEngine(rs.rule_tuples(), rs.lists, routes=rs.route_tuples() if routed else None, flags=flags, **rs.opts)
    # the engine's own program answers the shape the case was proved for
    assert eng.program.verdict_shape() == rs.program(flags, routed).verdict_shape()
    return eng


def assert_answers(what, got, want, kinds=None):
    """kinds: the kind of every group of the batch (named in the message)"""
    n = len(got["action"])
    bad = np.nonzero((got["action"][:n] != want["action"][:n]) | (got["rule_idx"][:n] != want["rule_idx"][:n]))[0]
    groups = sorted({int(b) // 64 for b in bad})
    assert len(bad) == 0, (f"{what}: {len(bad)} of {n} verdicts differ; first at {bad[0]} (group {bad[0] // 64}, lane {bad[0] % 64}): got ({got['action'][bad[0]]}, "
                           f"{got['rule_idx'][bad[0]]}) want ({want['action'][bad[0]]}, {want['rule_idx'][bad[0]]}); groups: "
                           f"{[(g, kinds[g]) if kinds is not None and g < len(kinds) else g for g in groups[:12]]}")


def check_host(what, c, eng, flags, routed, batch, want, M, route):
    counts_want = np.bincount(want["action"], minlength=4).tolist()
    eng.set_profiling(1)
    if flags & VC.HITS:
        got, hits, rule_hits, counts = eng.evaluate_batch_hits(batch, with_counts=True)
    elif routed:
        got, got_route, counts = eng.evaluate_batch_routes(batch, with_counts=True)
    else:
        got, counts = eng.evaluate_batch(batch, with_counts=True)
    names = [k[0] for k in eng.kernel_times()]
    eng.set_profiling(0)
    assert_answers(what, got, want, [g.kind for g in c.groups] if batch is c.batch else None)
    assert counts.tolist() == counts_want, what
    if flags & VC.HITS:
        H.assert_hits(what, hits, rule_hits, M)
    if routed:
        assert (got_route == route).all(), f"{what}: first routes differ at {np.nonzero(got_route != route)[0][:5]}"
    # (evaluate_batch_hits fetches a hit list that outgrew its first capacity again, once)
    assert names.count("verdict") == 1 or (flags & VC.HITS and names.count("verdict") == 2), (what, names)


def check_device(what, eng, batch, want):
    import torch

    db = DeviceBatch(batch)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    midx = torch.full((batch.n,), -1, dtype=torch.int32, device="cuda")
    nm = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = eng.evaluate_device(db, counts=counts, match_idx=midx, n_matches=nm)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert_answers(what + ", device-resident", {"action": got[:, 0], "rule_idx": got[:, 1]}, want)
    assert counts.cpu().tolist() == np.bincount(want["action"], minlength=4).tolist(), what
    k = int(nm.item())
    flagged = np.nonzero(want["action"] != 0)[0]
    assert k == len(flagged) and np.sort(midx[:k].cpu().numpy()).tolist() == flagged.tolist(), f"{what}: the match compaction"


@pytest.mark.parametrize("leg", list(LEGS))
@pytest.mark.parametrize("name", ["A", "C", "W", "P8", "P65", "Z"])
def test_set_on_leg(name, leg):
    flags, routed = LEGS[leg]
    run_leg(name, leg, flags, routed)


def run_leg(name, leg, flags, routed):
    c = VC.case(name)
    if not flags & (VC.SPARSE | VC.DENSE | _abi.OPT_NO_PREFILTER):
        VC.assert_targets(c, flags)  # (proved again for this leg's program before anything is sent)
    eng = make_engine(c.rs, flags, routed)
    try:
        what = f"set {name}, {leg}"
        if name == "Z" and leg == "as built":
            assert eng.residual_mode == 2, eng.residual_fallback  # (the specialized residual program: its result words are the residual entries)
        check_host(what, c, eng, flags, routed, c.batch, c.want, c.M, c.route)
        check_device(what, eng, c.batch, c.want)
        for n in SIZES:
            sub = {k: v[:n] for k, v in c.want.items()}
            check_host(f"{what}, batch of {n}", c, eng, flags, routed, c.batch.slice(0, n), sub, c.M[:, :n], c.route[:n])
        # a batch of heavily spilled groups, a small one, then the case again: stale spill words and slot bytes across batches
        heavy = [k for k, g in enumerate(c.groups) if g.kind.startswith(("heavy", "every"))]
        lo, hi = 64 * heavy[0], 64 * (heavy[-1] + 1)
        sub = {k: v[lo:hi] for k, v in c.want.items()}
        check_host(f"{what}, the heavy groups alone", c, eng, flags, routed, c.batch.slice(lo, hi), sub, c.M[:, lo:hi], c.route[lo:hi])
        check_host(f"{what}, again", c, eng, flags, routed, c.batch, c.want, c.M, c.route)
    finally:
        eng.close()


def test_rules_without_actions_on_the_rule_hits_leg():
    """set H: A's rules and twelve without actions, which only a PWAF_OPT_RULE_HITS engine keeps — proved from that program's own plan; the
    hit matrix holds their matches, no verdict is theirs"""
    run_leg("H", "rule hits", VC.HITS, False)


def test_chains_left_by_one_walker_per_request():
    """set C without prefilters: every request's field is walked by one lane, so a chain's order is the field's (reversed) — two chained lanes
    then name the same atom at the same step, two others at different steps (the targets are proved from the groups' token lists)"""
    c = VC.case("C")
    t = VC.targets(c, 0)
    assert t["two chained lanes name the same atoms at the same steps"] and t["two chained lanes name an atom at different steps"]
    run_leg("C", "no prefilter", _abi.OPT_NO_PREFILTER, False)


@pytest.mark.parametrize("name", ["A", "C"])
def test_turns_of_the_persistent_grid(name):
    """every wave of the launch on this device takes two groups, some a third; from the model, every ordered pair among {clean, exactly
    full, spilled} stands on some wave in consecutive turns — spilled then clean over a common column, spilled then spilled over different
    columns, clean then clean over disjoint ones. Expected: the base batch's reference answers, gathered."""
    c = VC.case(name)
    for leg in ("as built", "tiny slots"):
        flags, routed = LEGS[leg]
        ms = c.models(flags)[:-1]  # (the states at THIS leg's capacity: with 8 slots most groups spill)
        states, columns = [m.state for m in ms], [m.columns for m in ms]
        seq = VC.turn_sequence(states, columns)
        eng = make_engine(c.rs, flags, routed)
        try:
            sh = eng.program.verdict_shape()
            stride = eng.compute_units() * sh["per_cu"] * sh["waves"]
            kinds = VC.turn_groups(seq, stride)
            pairs = {(states[i], states[j]) for i, j in VC.turn_pairs(kinds, stride) if VC.pair_ok(states[i], states[j], columns[i], columns[j])}
            assert len(pairs) == 9 and len(kinds) > 2 * stride, (stride, pairs)
            idx = VC.turn_indices(kinds)
            batch = c.batch.take(idx)
            want = {k: v[idx] for k, v in c.want.items()}
            got, counts = eng.evaluate_batch(batch, with_counts=True)
            print(f"set {name}, {leg}: {eng.compute_units()} compute units, stride {stride}, {len(kinds)} groups, {batch.n} requests")
            assert_answers(f"set {name}, {leg}: {len(kinds)} groups over a stride of {stride}", got, want, [c.groups[k].kind for k in kinds])
            assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist()
            check_device(f"set {name}, {leg}, turns", eng, batch, want)
        finally:
            eng.close()
