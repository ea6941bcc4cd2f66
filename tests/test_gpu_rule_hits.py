"""Rule hits on the device (PWAF_OPT_RULE_HITS): the list pwaf_evaluate_batch_hits / pwaf_evaluate_device_hits return, turned into a
bool[n_rules, n] matrix, against the oracle's own: M[k, i] = (Oracle.execute_rule(k, batch, i) == 1), cleared for the requests a gate
answers. Verdicts and counters are compared with the oracle's and with the same engine's plain call every time. Cases: fuzzed rule sets
under the verdict kernel's modes, more than 64 candidates in one group, the gates, observe-only rules, lazy comparison atoms, more than 64
scan passes, the list's capacity, the device entry point on a stream, the flag's and NULL's behaviour, many workgroups."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import helpers as H
from oracle import pyoracle
from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.batch import RULE_HIT_DTYPE, hits_to_matrix
from pingoo_amd.engine import DeviceBatch, RuleEngine, UnsupportedExpression, lib

pytestmark = pytest.mark.gpu
B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
HITS = _abi.OPT_RULE_HITS
GATES = (_abi.RULE_UA_GATE, _abi.RULE_CAPTCHA_ENDPOINT)
NO_GATES = _abi.OPT_NO_UA_GATE | _abi.OPT_NO_CAPTCHA_BYPASS


oracle_matrix, assert_hits = H.oracle_matrix, H.assert_hits  # (shared with the confirm edge suite: helpers.py)


def check(label, eng, batch, m, want):
    """the engine's hit call against the oracle's matrix and verdicts, and against its own plain call; -> the hit list"""
    got, hits, rule_hits, counts = eng.evaluate_batch_hits(batch, with_counts=True)
    H.assert_verdicts_equal(got, want, batch, label)
    assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist(), label
    plain, plain_counts = eng.evaluate_batch(batch, with_counts=True)
    assert (plain == got).all() and (plain_counts == counts).all(), f"{label}: the plain call disagrees"
    assert_hits(label, hits, rule_hits, m)
    return hits


def run(label, rules, batch, lists=None, geo=None, flags=0, oracle_flags=0, m_want=None, **opts):
    m, want = m_want if m_want is not None else oracle_matrix(pyoracle.Oracle(rules, lists, geo, flags=oracle_flags), batch)
    eng = RuleEngine(rules, lists, geo, flags=flags | HITS, **opts)
    try:
        return check(label, eng, batch, m, want), m, want
    finally:
        eng.close()


def effects(actions):
    """(effect for an unverified client, for a verified one): http_listener.rs:253-262"""
    eff_u = 0 if not actions else (_abi.ACTION_BLOCK if actions[0] == B else _abi.ACTION_CAPTCHA)
    return eff_u, _abi.ACTION_BLOCK if B in actions else 0


def deciding_rule(m, rules, verified):
    """per request the first rule that matches AND takes effect for the client (n_rules: none), and its effect"""
    n_rules, n = m.shape
    eff = np.array([effects(a) for _, _, a in rules], dtype=np.int64)  # [n_rules, 2]
    fires = m & (eff[:, verified.astype(np.int64)] != 0)
    first = np.where(fires.any(axis=0), fires.argmax(axis=0), n_rules)
    action = np.where(first < n_rules, eff[np.minimum(first, n_rules - 1), verified.astype(np.int64)], 0)
    return first, action


# ---------------------------------------------------------------------------------------------------------
# 1. fuzz parity
# ---------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
FUZZ_SIZES = [1, 63, 64, 65, 129, 1000]
FUZZ_MODES = {"default": 0, "tiny": _abi.OPT_TINY_VERDICT_SLOTS, "global_tables": _abi.OPT_GLOBAL_VERDICT_TABLES, "no_residual_jit": _abi.OPT_NO_RESIDUAL_JIT,
              "eager_cmp": _abi.OPT_EAGER_CMP}


def fuzz_inputs(seed):
    """40 fuzzed rules (a few without an expression, every kind of action list, the empty one included), lists, a GeoIP table, 1000
    requests (captcha-verified or not; every second seed's batch carries asn / country itself)"""
    rng = random.Random(41000 + seed)
    lists = H.fuzz_lists(rng)
    geo = H.fuzz_geoip(rng)
    with_geo = seed % 2 == 1
    rules = [(f"r{k}", H.rexpr(rng, lists) if rng.random() < 0.95 else None, H.fuzz_actions(rng)) for k in range(40)]
    reqs = H.fuzz_requests(rng, max(FUZZ_SIZES), with_geo)
    return rules, lists, geo, reqs


@functools.lru_cache(maxsize=None)
def fuzz_case(seed):
    rules, lists, geo, reqs = fuzz_inputs(seed)
    batch = RequestBatch.from_requests(reqs)
    m, want = oracle_matrix(pyoracle.Oracle(rules, lists, geo), batch)
    assert_not_vacuous(m, want, rules, batch)
    return rules, lists, geo, batch, m, want


def assert_not_vacuous(m, want, rules, batch):
    """on the oracle's own matrix: the report says more than the verdicts do"""
    n_rules = len(rules)
    assert (m.sum(axis=0) >= 3).any(), "no request matches three rules"
    decided = np.where(want["rule_idx"] < n_rules, want["rule_idx"].astype(np.int64), n_rules)
    last = np.where(m.any(axis=0), n_rules - 1 - m[::-1].argmax(axis=0), -1)
    assert (last > decided).any(), "no request matches a rule after its deciding rule"
    k_idx = np.arange(n_rules)[:, None]
    shadowed = m.any(axis=1) & ~(m & (decided[None, :] >= k_idx)).any(axis=1)
    assert shadowed.any(), "no rule matches only requests an earlier rule decided"
    assert any(not a for _, _, a in rules) and (batch.flags & _abi.FLAG_CAPTCHA_VERIFIED).any() and not (batch.flags & _abi.FLAG_CAPTCHA_VERIFIED).all()


@pytest.mark.parametrize("mode", list(FUZZ_MODES))
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_hits_match_the_oracle(seed, mode):
    rules, lists, geo, batch, m, want = fuzz_case(seed)
    eng = RuleEngine(rules, lists, geo, flags=HITS | FUZZ_MODES[mode] | _abi.OPT_LENIENT)
    try:
        H.as_the_engine_sees(rules, eng.program)  # (asserts that the engine evaluates every rule of the set)
        for n in FUZZ_SIZES:
            check(f"seed {seed}, {mode}, n {n}", eng, batch.slice(0, n), m[:, :n], want[:n])
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------
# 2. more than 64 candidates in one group
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 200])
@pytest.mark.parametrize("first", ["match_all", "token"])
def test_more_than_64_candidates_in_one_group(n, first):
    """160 token rules that all match the same few requests, a match-all rule and a rule of negations only: three chunks of 64 candidates in
    those requests' groups. With the match-all rule first every request is decided after candidate 0 and the kernel still walks the list."""
    rng = random.Random(n)
    tokens = [f"q{k:03d}z" for k in range(160)]
    acts = [[], [CAP], [B], [CAP, B], [B, CAP]]
    token_rules = [(f"t{k}", f'http_request.path.contains("{t}")', acts[k % 5]) for k, t in enumerate(tokens)]
    everyone = ("all", None, [B] if first == "match_all" else [CAP])
    negations = ("neg", '!http_request.path.contains("nope") && !http_request.url.contains("never")', [CAP])
    rules = ([everyone] + token_rules if first == "match_all" else token_rules[:100] + [everyone] + token_rules[100:]) + [negations]
    full = "/" + "/".join(tokens)
    reqs = H.fuzz_requests(rng, n, False)
    for i in (3, 17, 62, 63, 64, 130, 199):
        if i < n:
            reqs[i].path = reqs[i].url = full if i != 17 else "/" + "/".join(tokens[40:150]) + "/nope"
    batch = RequestBatch.from_requests(reqs)
    for flags in (0, _abi.OPT_TINY_VERDICT_SLOTS, _abi.OPT_GLOBAL_VERDICT_TABLES):
        hits, m, want = run(f"{len(rules)} rules, n {n}, {first}, flags {flags}", rules, batch, flags=flags)
    per_group = np.bincount(hits["group"], minlength=(n + 63) // 64)
    assert per_group[0] > 128 and (m.sum(axis=0) > 128).any(), per_group
    if first == "match_all":
        ungated = ~np.isin(want["rule_idx"], GATES)
        assert (want["rule_idx"][ungated] == 0).all() and m[1:].any()


# ---------------------------------------------------------------------------------------------------------
# 3. the gates
# ---------------------------------------------------------------------------------------------------------
def test_gated_requests_match_nothing():
    rng = random.Random(3)
    reqs = H.fuzz_requests(rng, 150, False)
    for i, r in enumerate(reqs):
        r.user_agent, r.path = "Mozilla/5.0", "/index"
        r.url = r.path
        if i % 5 == 1:
            r.user_agent = ["", "x" * 256, "x" * 300][i % 3]
        if i % 7 == 2:
            r.path = r.url = "/__pingoo/captcha" + ["", "/init", "x"][i % 3]
    batch = RequestBatch.from_requests(reqs)
    rules = [("watch", None, []), ("all", None, [CAP, B]), ("ua", 'http_request.user_agent == ""', [B])]
    hits, m, want = run("gates", rules, batch)
    gated = np.isin(want["rule_idx"], GATES)
    assert gated.sum() >= 40 and (want["rule_idx"] == _abi.RULE_UA_GATE).sum() >= 20 and (want["rule_idx"] == _abi.RULE_CAPTCHA_ENDPOINT).sum() >= 15
    assert (m[0] == ~gated).all() and (m[1] == ~gated).all() and not m[2].any()
    for flags, oracle_flags in ((NO_GATES, NO_GATES), (_abi.OPT_NO_UA_GATE, _abi.OPT_NO_UA_GATE)):
        hits, m, want = run(f"gates off ({flags})", rules, batch, flags=flags, oracle_flags=oracle_flags)
        if flags == NO_GATES:
            assert m[0].all() and m[1].all() and m[2].sum() >= 10
            mine = np.sort(hits[hits["rule_idx"] == 0], order="group")
            assert mine["group"].tolist() == [0, 1, 2] and mine["mask"].tolist() == [2 ** 64 - 1, 2 ** 64 - 1, 2 ** (150 - 128) - 1]


# ---------------------------------------------------------------------------------------------------------
# 4. observe-only rules
# ---------------------------------------------------------------------------------------------------------
def test_observe_only_rules_are_reported_and_decide_nothing():
    rng = random.Random(4)
    lists = H.fuzz_lists(rng)
    deciding = [("a", 'http_request.path.contains("a/")', [CAP]), ("b", 'lists["nets"].contains(client.ip)', [B]), ("c", "client.remote_port < 80", [CAP, B]),
                ("d", 'http_request.url.ends_with("b")', [B])]
    observers = {0: ("o0", 'http_request.path.contains("a")', []), 2: ("o2", None, []), 6: ("o6", 'http_request.host.length() > 2 && http_request.method == "GET"', [])}
    rules, keep = [], []
    for k in range(7):
        if k in observers:
            rules.append(observers[k])
        else:
            keep.append(k)
            rules.append(deciding[len(keep) - 1])
    batch = RequestBatch.from_requests(H.fuzz_requests(rng, 500, False))
    hits, m, want = run("observers", rules, batch, lists=lists)
    for k in observers:
        assert m[k].sum() > 20 and not (want["rule_idx"] == k).any()
    # the verdicts are those of the rule set without the observers (indices mapped), from the oracle and from an engine without the flag
    bare = pyoracle.Oracle(deciding, lists, None).evaluate(batch)
    mapped = np.array(keep + [0], dtype=np.uint32)[np.minimum(bare["rule_idx"], len(keep))]
    expect_idx = np.where(bare["rule_idx"] < len(keep), mapped, bare["rule_idx"])
    assert (want["action"] == bare["action"]).all() and (want["rule_idx"] == expect_idx).all()
    assert len(set(want["rule_idx"].tolist())) >= 5
    eng = RuleEngine(rules, lists, None)  # (no flag: the observers are dropped at compile time, the caller's indices stay)
    H.assert_verdicts_equal(eng.evaluate_batch(batch), want, batch, "observers, no flag")
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# 5. lazy comparison atoms
# ---------------------------------------------------------------------------------------------------------
def test_lazy_comparison_atoms_report_exact_matches():
    """`literal && length / port op constant`: the comparison is evaluated by the verdict kernel only for rules whose literal holds for
    somebody in the group, and for a hit report also when no action of the rule takes effect for those requests (a Captcha rule and verified
    clients; an observe-only rule)"""
    rng = random.Random(5)
    words = ["admin", "login", ".php", "select", "passwd"] + ["".join(rng.choice("bcdfgklmnprstvz") for _ in range(5)) for _ in range(25)]
    rules = []
    for k, w in enumerate(words):
        cmp_ = [f"http_request.path.length() > {10 + k}", f"client.remote_port <= {1000 * (k + 1)}", f"http_request.path.length() == {12 + k % 7}",
                f"!(http_request.url.length() < {15 + k})"][k % 4]
        rules.append((f"l{k}", f'http_request.path.contains("{w}") && {cmp_}', [[CAP], [B], [], [CAP, B], [CAP, CAP]][k % 5]))
    rules.append(("two", 'http_request.path.contains("admin") && http_request.path.length() > 30 || http_request.url.contains("zz") && client.remote_port == 443', [CAP]))
    reqs = []
    for i in range(700):
        w = rng.choice(words) if rng.random() < 0.6 else "aeiou"
        path = "/" + "y" * rng.randint(0, 30) + w + "u" * rng.randint(0, 6)
        reqs.append(Request(host="h", url=path + rng.choice(["", "?zz", "?a=1"]), path=path, method="GET", user_agent="Mozilla/5.0", ip="9.9.9.9",
                            remote_port=rng.choice([443, 80, 999, 5000, 20000, 65535]), captcha_verified=rng.random() < 0.5))
    batch = RequestBatch.from_requests(reqs)
    m_want = oracle_matrix(pyoracle.Oracle(rules, None, None), batch)
    m, want = m_want
    verified = (batch.flags & _abi.FLAG_CAPTCHA_VERIFIED) != 0
    captcha_only = [k for k, (_, _, a) in enumerate(rules) if a and B not in a]
    literal = np.array([[words[k].encode() in batch.field_bytes(2, i) for i in range(batch.n)] for k in range(len(words))])
    # verified clients of the Captcha-only rules (no action takes effect for them): some satisfy literal and comparison, some the literal alone
    both = [int((m[k] & verified).sum()) for k in captcha_only[:-1]]
    literal_alone = [int((literal[k] & ~m[k] & verified).sum()) for k in captcha_only[:-1]]
    assert sum(both) >= 10 and sum(literal_alone) >= 10 and sum(1 for x, y in zip(both, literal_alone) if x and y) >= 3, (both, literal_alone)
    assert (m[len(rules) - 1] & verified).any()
    hits_lazy, _, _ = run("lazy", rules, batch, m_want=m_want)
    hits_eager, _, _ = run("eager", rules, batch, flags=_abi.OPT_EAGER_CMP, m_want=m_want)
    assert (np.sort(hits_lazy, order=["rule_idx", "group"]) == np.sort(hits_eager, order=["rule_idx", "group"])).all()
    run("lazy, tiny", rules, batch, flags=_abi.OPT_TINY_VERDICT_SLOTS, m_want=m_want)
    run("lazy, global tables", rules, batch, flags=_abi.OPT_GLOBAL_VERDICT_TABLES, m_want=m_want)


# ---------------------------------------------------------------------------------------------------------
# 6. more than 64 scan passes
# ---------------------------------------------------------------------------------------------------------
def test_more_than_64_passes():
    ps = H.pinned_passes("confirm_walk", 65)
    assert ps.n_passes == 65
    batch = RequestBatch.from_requests(H.pinned_requests(random.Random(6), ps, 130, hit=0.5))
    m_want = oracle_matrix(pyoracle.Oracle(ps.rules, {}, None), batch)
    assert m_want[0].any(axis=1).sum() > 20 and (m_want[0].sum(axis=0) >= 2).any()
    for flags in (0, _abi.OPT_GLOBAL_VERDICT_TABLES):
        run(f"65 passes, flags {flags}", ps.rules, batch, flags=flags, m_want=m_want, **ps.opts)


# ---------------------------------------------------------------------------------------------------------
# 7. capacity
# ---------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5


def test_capacity():
    import torch

    rules, lists, geo, batch, m, want = fuzz_case(FUZZ_SEEDS[0])
    batch, m, want = batch.slice(0, 300), m[:, :300], want[:300]
    eng = RuleEngine(rules, lists, geo, flags=HITS | _abi.OPT_LENIENT)
    full = check("capacity: full list", eng, batch, m, want)
    E = len(full)
    assert E > 8
    entries = {bytes(h.tobytes()) for h in full}
    db = DeviceBatch(batch)
    for cap in (0, 1, E - 1, E, E + 7):
        # host: the caller's array beyond the entries written is left alone
        buf = np.frombuffer(bytes([SENTINEL]) * (16 * (cap + 64)), dtype=RULE_HIT_DTYPE).copy()
        got, counts, n_hits, rule_hits = eng.evaluate_batch_hits_into(batch, buf, cap)
        k = min(cap, E)
        assert n_hits == E and (got == want).all() and rule_hits.tolist() == m.sum(axis=1).tolist(), cap
        assert (buf[k:].view(np.uint8) == SENTINEL).all(), cap
        assert len({bytes(h.tobytes()) for h in buf[:k]}) == k and {bytes(h.tobytes()) for h in buf[:k]} <= entries, cap
        # device: the kernel itself never writes at or beyond hits + hits_cap
        d_hits = torch.full((cap + 64, 16), SENTINEL, dtype=torch.uint8, device="cuda:0")
        d_n, d_rule = torch.zeros(1, dtype=torch.int32, device="cuda:0"), torch.zeros(len(rules), dtype=torch.int64, device="cuda:0")
        out = eng.evaluate_device(db, hits=d_hits, n_hits=d_n, rule_hits=d_rule, hits_cap=cap)
        eng.device_status()
        back = d_hits.cpu().numpy().reshape(-1).view(RULE_HIT_DTYPE)
        assert int(d_n.item()) == E and d_rule.cpu().tolist() == m.sum(axis=1).tolist(), cap
        assert (out.cpu().numpy().view(want.dtype).reshape(-1) == want).all()
        assert (back[k:].view(np.uint8) == SENTINEL).all(), cap
        assert len({bytes(h.tobytes()) for h in back[:k]}) == k and {bytes(h.tobytes()) for h in back[:k]} <= entries, cap
    # rule_hits alone, and the list alone
    got, counts, n_hits, rule_hits = eng.evaluate_batch_hits_into(batch, None)
    assert n_hits is None and rule_hits.tolist() == m.sum(axis=1).tolist()
    buf = np.zeros(E, dtype=RULE_HIT_DTYPE)
    got, counts, n_hits, rule_hits = eng.evaluate_batch_hits_into(batch, buf, E, with_rule_hits=False)
    assert n_hits == E and rule_hits is None and (hits_to_matrix(buf, batch.n, len(rules)) == m).all()
    # the Python wrapper fetches a list that did not fit again, once
    got, hits, rule_hits = eng.evaluate_batch_hits(batch, cap=3)
    assert_hits("retry", hits, rule_hits, m)
    # a batch too large for the packed staging block: the column-by-column path
    big = batch.tile(40)
    got, hits, rule_hits, counts = eng.evaluate_batch_hits(big, with_counts=True)
    assert (got == np.tile(want, 40)).all() and rule_hits.tolist() == (40 * m.sum(axis=1)).tolist()
    assert_hits("large host batch", hits, rule_hits, np.tile(m, (1, 40)))
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# 8. the device entry point
# ---------------------------------------------------------------------------------------------------------
def test_device_path_accumulates_on_a_stream():
    import torch

    rules, lists, geo, batch, m, want = fuzz_case(FUZZ_SEEDS[1])
    eng = RuleEngine(rules, lists, geo, flags=HITS | _abi.OPT_LENIENT)
    db = DeviceBatch(batch)
    E = len({(k, i // 64) for k, i in np.argwhere(m)})
    d_hits = torch.zeros((2 * E + 8, 16), dtype=torch.uint8, device="cuda:0")
    d_n, d_rule = torch.zeros(1, dtype=torch.int32, device="cuda:0"), torch.zeros(len(rules), dtype=torch.int64, device="cuda:0")
    # (n_matches accumulates like n_hits: the second call's indices land behind the first call's, so the list holds both)
    d_idx, d_nm = torch.zeros(2 * batch.n, dtype=torch.int32, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
    d_counts = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    hist = np.bincount(want["action"], minlength=4)
    for rounds in (1, 2):
        out = eng.evaluate_device(db, counts=d_counts, match_idx=d_idx, n_matches=d_nm, stream=stream.cuda_stream, hits=d_hits, n_hits=d_n, rule_hits=d_rule)
        stream.synchronize()
        eng.device_status()
        assert (out.cpu().numpy().view(want.dtype).reshape(-1) == want).all()
        assert int(d_n.item()) == rounds * E and d_rule.cpu().tolist() == (rounds * m.sum(axis=1)).tolist() and d_counts.cpu().tolist() == (rounds * hist).tolist()
        assert int(d_nm.item()) == rounds * int((want["action"] != 0).sum())
        back = d_hits.cpu().numpy().reshape(-1).view(RULE_HIT_DTYPE)
        for r in range(rounds):
            assert_hits(f"device, call {r + 1}", back[r * E:(r + 1) * E], m.sum(axis=1), m)
    assert sorted(d_idx.cpu().numpy()[:int((want["action"] != 0).sum())].tolist()) == np.nonzero(want["action"])[0].tolist()
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# 9. off means off
# ---------------------------------------------------------------------------------------------------------
def test_without_the_flag_unsupported_and_all_null_is_the_plain_call():
    import torch

    rules, lists, geo, batch, m, want = fuzz_case(FUZZ_SEEDS[2])
    off_eng = RuleEngine(rules, lists, geo, flags=_abi.OPT_LENIENT)
    on_eng = RuleEngine(rules, lists, geo, flags=HITS | _abi.OPT_LENIENT)
    db = DeviceBatch(batch)
    d_hits, d_n = torch.zeros((8, 16), dtype=torch.uint8, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
    d_rule = torch.zeros(len(rules), dtype=torch.int64, device="cuda:0")
    for call in (lambda: off_eng.evaluate_batch_hits(batch), lambda: off_eng.evaluate_batch_hits_into(batch, None), lambda: off_eng.evaluate_device(db, hits=d_hits, n_hits=d_n),
                 lambda: off_eng.evaluate_device(db, rule_hits=d_rule)):
        off_eng.set_profiling(1)
        with pytest.raises(UnsupportedExpression, match="PWAF_OPT_RULE_HITS") as ei:
            call()
        assert ei.value.code == _abi.E_UNSUPPORTED and off_eng.kernel_times() == []  # (nothing was launched)
        off_eng.set_profiling(0)
    assert int(d_n.item()) == 0 and not d_rule.any()
    with pytest.raises(Exception, match="together"):
        on_eng.evaluate_device(db, n_hits=d_n)
    st = batch.as_struct(on_eng.header_names)

    def names(eng, call):
        eng.set_profiling(1)
        out = call(eng)
        t = [k[0] for k in eng.kernel_times()]
        eng.set_profiling(0)
        return t, out

    def all_null(eng):
        out = np.zeros(batch.n, dtype=want.dtype)
        assert lib().pwaf_evaluate_batch_hits(eng._h, C.byref(st), out.ctypes.data, None, None, 0, None, None) == 0
        return out

    base, plain = names(off_eng, lambda e: e.evaluate_batch(batch))
    assert "verdict" in base
    for label, (t, out) in {"flag, plain call": names(on_eng, lambda e: e.evaluate_batch(batch)), "flag, all NULL": names(on_eng, all_null), "no flag, all NULL": names(off_eng, all_null),
                            "flag, hits": names(on_eng, lambda e: e.evaluate_batch_hits(batch)[0])}.items():
        assert t == base, label  # (the report adds no launch either)
        assert (out == plain).all(), label
    H.assert_verdicts_equal(plain, want, batch, "no flag")
    off_eng.close()
    on_eng.close()


# ---------------------------------------------------------------------------------------------------------
# 10. many workgroups
# ---------------------------------------------------------------------------------------------------------
def test_many_workgroups():
    rng = random.Random(10)
    rules = H.lit_rules(rng, 60) + [("watch", 'http_request.url.contains("id=")', [])]
    base = RequestBatch.from_requests(H.lit_requests(rng, 5000))  # (5000 is no multiple of 64: every copy sits differently in its groups)
    batch = base.take(np.arange(200000) % 5000)
    n, n_rules = batch.n, len(rules)
    assert n == 200000
    eng = RuleEngine(rules, None, None, flags=HITS | _abi.OPT_LENIENT)
    seen, _ = H.as_the_engine_sees(rules, eng.program)
    got, hits, rule_hits, counts = eng.evaluate_batch_hits(batch, with_counts=True)
    plain = eng.evaluate_batch(batch)
    eng.close()
    assert (plain == got).all()
    g = hits_to_matrix(hits, n, n_rules)
    assert (hits["mask"] != 0).all() and len(np.unique(hits["rule_idx"].astype(np.uint64) << np.uint64(32) | hits["group"])) == len(hits)
    assert rule_hits.tolist() == g.sum(axis=1).tolist() and len(hits) > 3 * ((n + 63) // 64)
    # the verdict again, on the host, from the hit list, the rules' actions, the verified flag and the gate verdicts
    gated = np.isin(got["rule_idx"], GATES)
    assert not g[:, gated].any() and 0 < gated.sum() < n // 4
    first, action = deciding_rule(g, rules, (batch.flags & _abi.FLAG_CAPTCHA_VERIFIED) != 0)
    expect_rule = np.where(first < n_rules, first, _abi.RULE_NONE).astype(np.uint32)
    bad = np.nonzero(~gated & ((got["rule_idx"] != expect_rule) | (got["action"] != action)))[0]
    assert len(bad) == 0, (len(bad), int(bad[0]), got[bad[0]], int(first[bad[0]]), int(action[bad[0]]))
    assert counts.tolist() == np.bincount(got["action"], minlength=4).tolist()
    assert len(set(got["rule_idx"].tolist())) > 10 and (g.sum(axis=0) >= 3).any()
    # and the oracle's matrix on a sample
    sample = np.sort(np.random.default_rng(10).choice(n, 2000, replace=False))
    sub = batch.take(sample)
    m, want = oracle_matrix(pyoracle.Oracle(seen, None, None), sub)
    H.assert_verdicts_equal(got[sample], want, sub, "sample")
    bad = np.argwhere(g[:, sample] != m)
    assert len(bad) == 0, (len(bad), bad[0])
