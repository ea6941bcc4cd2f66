"""GPU parity at the engine's capacity limits: phase-0 list-scan descriptors across 256 (one launch_scan_gated call each 256), 250 scan
passes plus both pseudo passes (the top bit of the 4-word pass bitmap), the verdict kernels' 64-pass bitmap switch, gated gap passes
across 32, and lazy comparison constants across 0xFFFF. Rule sets come from helpers.pinned_passes (exact pass counts); every case
compares (action, rule_idx) with the CPU oracle and the action counters with its histogram."""
import random

import numpy as np
import pytest

import helpers as H
from oracle import pyoracle
from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.engine import DeviceBatch, RuleEngine

pytestmark = pytest.mark.gpu
VERDICT_VARIANTS = {"verdict2": 0, "sparse": _abi.OPT_SPARSE_VERDICT, "dense": _abi.OPT_DENSE_VERDICT, "tiny": _abi.OPT_TINY_VERDICT_SLOTS,
                    "global_tables": _abi.OPT_GLOBAL_VERDICT_TABLES}
# a field-against-field rule (the fcmp pseudo pass) and a residual rule (arithmetic on request values: the residual pseudo pass)
PSEUDO = [("fcmp", "http_request.path == http_request.url && http_request.method == \"PUT\"", [H.B]),
          ("residual", "http_request.url.length() - http_request.path.length() > 41 && client.remote_port % 2 == 1", [H.CAP])]


def oracle(rules, batch):
    return pyoracle.Oracle(rules, {}, None).evaluate(batch, threads=8)


def run(rules, batch, want, label, tune=None, popts=None, **opts):
    eng = RuleEngine(rules, {}, None, **{**(popts or {}), **opts})  # (popts: the options the set was pinned with)
    try:
        if tune is not None:
            eng.tune(tune)
        got, counts = eng.evaluate_batch(batch, with_counts=True)
        H.assert_verdicts_equal(got, want, batch, label)
        assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist(), label
        return eng.stats()
    finally:
        eng.close()


def lscan_launches(rules, batch, **opts):
    """the list-scan launches of one batch, from the engine's own kernel marks (lscan_x<descriptors>)"""
    eng = RuleEngine(rules, {}, None, **opts)
    try:
        eng.set_profiling(1)
        eng.evaluate_batch(batch)
        kt = eng.kernel_times()
        return [int(name[len("lscan_x"):]) for name, _, _ in kt if name.startswith("lscan_x")]
    finally:
        eng.close()


def deciding(want, rules, first_rule=0):
    return {int(r) for r in want["rule_idx"].tolist() if first_rule <= r < len(rules)}


def saturated(rng, ps, n, rule):
    """every url filled with one rule's factors: more than half of the url arena's 16-byte chunks flag that rule's pass (its dense
    alternative runs), the rest of the traffic benign"""
    tok = ps.tokens[rule][1][0]
    a, b = tok[:6], tok[-6:]  # (helpers.kind_rules: six-consonant words around the digits)
    reqs = H.pinned_requests(rng, ps, n, hit=0.2)
    for q in reqs:
        q.url = "/" + "".join(f"{a}{rng.randint(0, 99)}{b}" if rng.random() < 0.9 else f"{a}-{b}" for _ in range(rng.randint(8, 14)))
    return reqs


# phase-0 descriptors = 2 n - n_ident - 1: 254, 255, 256, 257, 360, 495
@pytest.mark.parametrize("n,n_ident", [(128, 1), (129, 2), (129, 1), (130, 2), (182, 3), (250, 4)])
def test_phase_0_descriptors_across_256(n, n_ident):
    rng = random.Random(n)
    ident = H.kind_rules("identity", n_ident, prefix="x")[0]
    ps = H.pinned_passes("confirm_walk", n, extra=tuple(ident))
    assert ps.n_passes == n and ps.n_confirm == n - n_ident and ps.n_walk == n - n_ident - 1, (ps.n_confirm, ps.n_walk)
    rules = ps.rules
    batch = RequestBatch.from_requests(H.pinned_requests(rng, ps, 8000, hit=0.35))
    want = oracle(rules, batch)
    dec = deciding(want, rules)
    assert len(dec) > 10, len(dec)
    # traffic reaches the last four passes (past the 128th; those whose descriptors come last in phase 0): a deciding rule's match flags one
    late = [k for k in sorted(dec, reverse=True)[:60] if ps.tokens[k][1] and ps.pass_of_input(ps.tokens[k][1][0].encode(), first=n - 4)]
    assert late, "no deciding rule of the last four passes"
    run(rules, batch, want, f"{n} passes, benign", popts=ps.opts)
    # phase 0: a dense alternative + an R-tier walk per walking confirm pass, + the dense alternative of the captcha-path pass, + identity passes
    launches = lscan_launches(rules, batch, **ps.opts)
    phase0 = 2 * (n - n_ident - 1) + 1 + n_ident
    assert sum(launches) == phase0 and max(launches) <= 256 and len(launches) == (1 if phase0 <= 256 else 2), (phase0, launches)
    run(rules, batch, want, f"{n} passes, no dense switch", flags=_abi.OPT_NO_DENSE_SWITCH, popts=ps.opts)
    run(rules, batch, want, f"{n} passes, no confirm tier", flags=_abi.OPT_NO_CONFIRM, popts=ps.opts)
    if n >= 182:
        # saturated: a rule of the LAST pass filled into every url — its dense alternative lands past the 256th descriptor
        last = max(k for k in range(len(rules)) if ps.tokens[k][1] and ps.pass_of_input(ps.tokens[k][1][0].encode(), first=n - 2))
        sat = RequestBatch.from_requests(saturated(rng, ps, 6000, last))
        want_s = oracle(rules, sat)
        assert (want_s["rule_idx"] == last).sum() > 1000
        run(rules, sat, want_s, f"{n} passes, saturated", popts=ps.opts)
        run(rules, sat, want_s, f"{n} passes, saturated, no dense switch", flags=_abi.OPT_NO_DENSE_SWITCH, popts=ps.opts)
        # two batches in flight on two streams (bench.py's two-in-flight leg): the split launches' plan regions are per batch
        import torch

        eng = RuleEngine(rules, {}, None, **ps.opts)
        try:
            dev = torch.device("cuda:0")
            db = [DeviceBatch(batch, dev), DeviceBatch(sat, dev)]
            streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
            outs = [None, None]
            for rep in range(3):
                for k in (0, 1):
                    with torch.cuda.stream(streams[k]):
                        outs[k] = eng.evaluate_device(db[k], stream=streams[k].cuda_stream)
                torch.cuda.synchronize(dev)
                eng.device_status()
                for k, w in ((0, want), (1, want_s)):
                    o = outs[k].cpu().numpy()
                    got = np.zeros(len(w), dtype=w.dtype)
                    got["action"], got["rule_idx"] = o[:, 0], o[:, 1]
                    H.assert_verdicts_equal(got, w, None, f"{n} passes, two in flight, stream {k}, round {rep}")
        finally:
            eng.close()


def test_250_passes_plus_both_pseudo_passes():
    rng = random.Random(252)
    ps = H.pinned_passes("confirm_walk", 250, extra=tuple(PSEUDO))
    rules = ps.rules
    reqs = H.pinned_requests(rng, ps, 6000, hit=0.35)
    for q in reqs[::7]:
        q.path, q.method = q.url, "PUT"
    for q in reqs[3::5]:
        q.url = q.url + "?" + "q" * rng.randint(30, 60)
    batch = RequestBatch.from_requests(reqs)
    want = oracle(rules, batch)
    assert {0, 1} <= deciding(want, rules) and len(deciding(want, rules)) > 10
    assert any(ps.pass_of_input(ps.tokens[k][1][0].encode(), first=240) for k in sorted(deciding(want, rules))[-10:] if ps.tokens[k][1])
    for label, fl in VERDICT_VARIANTS.items():
        run(rules, batch, want, f"252 passes, {label}", flags=fl, popts=ps.opts)


@pytest.mark.parametrize("n_scan,pseudo", [(63, False), (64, False), (65, False), (62, False), (63, True)])
def test_the_64_pass_bitmap_switch(n_scan, pseudo):
    """n_passes (scan passes + pseudo passes) 62..65: BR == 1 up to 64, else the 4-word bitmap; 65 once through scan passes alone and
    once through 63 scan passes + the field-against-field and residual pseudo passes"""
    rng = random.Random(n_scan * 2 + pseudo)
    ps = H.pinned_passes("confirm_walk", n_scan, extra=tuple(PSEUDO) if pseudo else ())
    rules = ps.rules
    reqs = H.pinned_requests(rng, ps, 5000, hit=0.4)
    if pseudo:
        for q in reqs[::6]:
            q.path, q.method = q.url, "PUT"
        for q in reqs[1::4]:
            q.url = q.url + "?" + "q" * rng.randint(30, 60)
    batch = RequestBatch.from_requests(reqs)
    want = oracle(rules, batch)
    dec = deciding(want, rules)
    assert len(dec) > 10 and max(dec) >= len(rules) - 20, (len(dec), max(dec))
    if pseudo:
        assert {0, 1} <= dec
    for label, fl in VERDICT_VARIANTS.items():
        run(rules, batch, want, f"{n_scan} scan passes{' + 2 pseudo' if pseudo else ''}, {label}", flags=fl, popts=ps.opts)


@pytest.mark.parametrize("n", [31, 32, 33, 40])
def test_gated_gap_passes_across_32(n):
    rng = random.Random(4000 + n)
    lit = H.kind_rules("confirm_literal", 6, seed=9, prefix="x")
    ps = H.pinned_passes("gap", n, extra=tuple(lit[0]))
    rules = ps.rules
    ps.tokens[:len(lit[1])] = lit[1]
    reqs = H.pinned_requests(rng, ps, 6000, hit=0.35)
    batch = RequestBatch.from_requests(reqs)
    want = oracle(rules, batch)
    dec = deciding(want, rules)
    assert len(dec) > 10, len(dec)
    # gap rules decide on both sides of the 32nd gated pass (the rules are packed in order: the last ones sit in the last passes)
    assert any(k >= len(rules) - 6 for k in dec) and any(len(lit[0]) <= k < len(lit[0]) + 10 for k in dec), sorted(dec)
    run(rules, batch, want, f"{n} gap passes, untuned", popts=ps.opts)
    run(rules, batch, want, f"{n} gap passes, tuned", tune=batch, popts=ps.opts)


LAZY_CONSTS = [0, 1, 65534, 65535, 65536, 65537]
OPS = ["==", "!=", "<", "<=", ">", ">="]


def test_lazy_constants_across_0xffff():
    rng = random.Random(0xFFFF)
    words = H.pass_words(77, 3 * len(LAZY_CONSTS) * len(OPS))
    rules, rare = [], []
    for var in ("client.remote_port", "http_request.url.length()", 'http_request.headers["x-len"].length()'):
        for c in LAZY_CONSTS:
            for op in OPS:
                w = words[len(rules)]
                rules.append((f"r{len(rules)}", f'http_request.path.contains("{w}") && {var} {op} {c}', [H.B] if len(rules) % 2 else [H.CAP]))
                rare.append((var, w, c))
    near = lambda c: [v for v in (c - 1, c, c + 1) if v >= 0]  # noqa: E731
    reqs = []
    for i in range(5000):
        var, w, c = rare[rng.randrange(len(rare))]
        path = "/" + w if rng.random() < 0.8 else "/" + rstr(rng)
        port = rng.randrange(65536)
        url_len, hdr_len = rng.randint(len(path), len(path) + 30), rng.randint(0, 30)
        v = rng.choice(near(c))
        if var == "client.remote_port":
            port = min(v, 65535)
        elif i % 25 == 0:  # (a long value now and then: the values next to 65535 cost 64 KiB each)
            if var.startswith("http_request.url"):
                url_len = max(v, len(path))
            else:
                hdr_len = v
        elif v <= 1:
            if var.startswith("http_request.url"):
                url_len = len(path) + v
            else:
                hdr_len = v
        url = (path + "?" + "u" * max(0, url_len - len(path) - 1)) if url_len > len(path) else path
        reqs.append(Request(host="h", url=url, path=path, method="GET", user_agent="ua", ip="1.2.3.4", remote_port=port, captcha_verified=rng.random() < 0.3,
                            headers={"x-len": "h" * hdr_len} if rng.random() < 0.9 else None))
    batch = RequestBatch.from_requests(reqs)
    want = oracle(rules, batch)
    dec = deciding(want, rules)
    assert len(dec) > 60, len(dec)
    for label, fl in [("lazy", 0), ("eager", _abi.OPT_EAGER_CMP), ("tiny", _abi.OPT_TINY_VERDICT_SLOTS), ("sparse", _abi.OPT_SPARSE_VERDICT),
                      ("sparse+tiny", _abi.OPT_SPARSE_VERDICT | _abi.OPT_TINY_VERDICT_SLOTS)]:
        run(rules, batch, want, f"lazy constants, {label}", flags=fl)


def rstr(rng):
    return H.rstr(rng, 1, 8, "abcxyz/")


def test_a_refusal_of_the_table_planner_reaches_the_caller():
    """Creation only (no batch): a refusal of csrc/tableplan.cpp comes back as PWAF_E_UNSUPPORTED without a rule index, its text in the
    compile error and in pwaf_last_error, and the device is left usable. 513 ip lists are the planner refusal a rule set reaches; 129
    integer sets on one variable are not one — the rule compiler counts that width too and runs the 129th rule as a residual program
    (tests/test_tableplan_cpu.py: test_attribute_row_widths_at_and_past_the_limit) — so that rule set must still create."""
    from pingoo_amd.engine import UnsupportedExpression, lib

    rules = [("r", 'lists["l0"].contains(client.ip) || client.ip in lists.l512', [H.B])]
    lists = {f"l{k}": (_abi.LIST_IP, [f"10.{k >> 8}.{k & 255}.0/24"]) for k in range(513)}
    with pytest.raises(UnsupportedExpression) as ei:
        RuleEngine(rules, lists, None)
    assert ei.value.code == _abi.E_UNSUPPORTED and ei.value.rule_index is None  # (err.rule_index == 0xFFFFFFFF)
    assert ei.value.message == "more than 512 ip lists" and lib().pwaf_last_error() == b"more than 512 ip lists"
    sets = [(f"r{k}", f"[{k + 2}, {70000 + k}].contains(client.remote_port)", [H.B]) for k in range(129)]
    eng = RuleEngine(sets, {}, None, flags=_abi.OPT_NO_RESIDUAL_JIT)
    try:
        assert eng.residual_mode == 1  # (one rule runs in the residual interpreter)
    finally:
        eng.close()
    lists.pop("l512")
    rules = [("r", 'lists["l0"].contains(client.ip) || client.ip in lists.l511', [H.B])]
    RuleEngine(rules, lists, None).close()  # 512 lists, the widest membership set, on the same device
