"""Service routes on the device (engines created with pwaf_engine_create_routed): each request's first matching route beside its verdict,
from one pass. Verdicts against pyoracle.Oracle over the rules; routes against the oracle over the routes (route k 'blocks' with rule
index k, no gate — the construction of test_gpu_paths.py's routing test) and against pingoo_amd.engine.ServiceRouter. Cases: known
answers, group edges, more than 64 candidates in one group, lazy comparison atoms in a route, the kernel's variants, fuzzed sets, the
entry points, many workgroups."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import helpers as H
import routed_walker as RW
from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.batch import GEO_DTYPE
from pingoo_amd.engine import DeviceBatch, RuleEngine, ServiceRouter, UnsupportedExpression, lib

pytestmark = pytest.mark.gpu
B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
VERIFIED = _abi.FLAG_CAPTCHA_VERIFIED


def check(label, eng, batch, want, want_routes):
    """the routed call against both oracles, and the same engine's plain call against the routed one; -> (verdicts, routes)"""
    got, routes, counts = eng.evaluate_batch_routes(batch, with_counts=True)
    H.assert_verdicts_equal(got, want, batch, label)
    assert routes.dtype == np.int32 and len(routes) == batch.n
    bad = np.nonzero(routes != want_routes)[0]
    assert len(bad) == 0, f"{label}: {len(bad)} of {batch.n} routes differ; first at {bad[0]}: got {routes[bad[0]]} want {want_routes[bad[0]]}, verdict {got[bad[0]]}"
    assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist(), label
    assert (eng.evaluate_batch(batch) == got).all(), f"{label}: the plain call disagrees"
    return got, routes


def run(label, rules, routes, batch, lists=None, geo=None, flags=0, wants=None, **opts):
    want, want_routes = wants if wants is not None else (RW.oracle_verdicts(rules, lists, geo, batch, flags & RW.NO_GATES), RW.oracle_routes(routes, lists, geo, batch))
    eng = RuleEngine(rules, lists, geo, routes=routes, flags=flags, **opts)
    try:
        assert lib().pwaf_engine_route_count(eng._h) == len(routes)
        return check(label, eng, batch, want, want_routes)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------
# 1. known answers: the five routes, lists and 800 requests of test_gpu_paths.py's routing test, beside a small rule set with both gates
# ---------------------------------------------------------------------------------------------------------
KNOWN_ROUTES = [("api", 'http_request.host.starts_with("api.")'), ("static", 'http_request.path.starts_with("/static/") || http_request.path.ends_with(".css")'),
                ("admin", 'http_request.host == "admin.example.com" && lists["office"].contains(client.ip)'), ("broken", "http_request.path"), ("v2", 'http_request.url.matches("^/v2/[0-9]+")')]
KNOWN_LISTS = {"office": (_abi.LIST_IP, ["10.0.0.0/8"])}
KNOWN_RULES = [("css", 'http_request.path.ends_with(".css")', [CAP]), ("office", 'lists["office"].contains(client.ip) && http_request.host.starts_with("api")', [B]),
               ("v2", 'http_request.url.contains("/v2/abc")', [CAP, B]), ("index", 'http_request.path == "/index.html" && http_request.host == ""', [B])]


@functools.lru_cache(maxsize=None)
def known_case():
    rng = random.Random(4)
    hosts = ["api.example.com", "www.example.com", "admin.example.com", "api", ""]
    paths = ["/static/a.js", "/x/y.css", "/v2/123/items", "/v2/abc", "", "/index.html"]
    reqs = [Request(host=rng.choice(hosts), path=(p := rng.choice(paths)), url=p or "/", ip=rng.choice(["10.1.1.1", "8.8.8.8"]), user_agent="") for _ in range(800)]
    for i, r in enumerate(reqs):  # (the routing test's requests all carry an empty User-Agent: gate A. Here most pass the gates)
        r.user_agent = "" if i % 9 == 0 else "x" * 300 if i % 31 == 0 else "Mozilla/5.0"
        r.captcha_verified = i % 3 == 0
        if i % 23 == 0:
            r.path = r.url = "/__pingoo/captcha/init"
    batch = RequestBatch.from_requests(reqs)
    return batch, RW.oracle_verdicts(KNOWN_RULES, KNOWN_LISTS, None, batch), RW.oracle_routes(KNOWN_ROUTES, KNOWN_LISTS, None, batch)


def test_known_answers():
    batch, want, want_routes = known_case()
    assert set(want_routes.tolist()) == {-1, 0, 1, 2, 4}  # "broken" (a non-Bool route) never matches
    assert {(int(v["action"]), int(v["rule_idx"])) for v in want} >= {(1, _abi.RULE_UA_GATE), (3, _abi.RULE_CAPTCHA_ENDPOINT), (2, 0), (1, 1), (2, 2), (1, 2), (1, 3), (0, _abi.RULE_NONE)}
    # requests the rules block, captcha or gate still have their route
    assert ((want["action"] != 0) & (want_routes >= 0)).sum() > 50
    eng = RuleEngine(KNOWN_RULES, KNOWN_LISTS, None, routes=KNOWN_ROUTES)
    got, routes = check("known answers", eng, batch, want, want_routes)
    router = ServiceRouter(KNOWN_ROUTES, KNOWN_LISTS)
    assert (router.route_batch(batch) == routes).all()
    router.close()
    # the verified flag (and any other value of the flags column) does not enter the route
    for value in (0, VERIFIED, 0xFF):
        b2 = batch.take(np.arange(batch.n))  # (a copy: the cached batch keeps its flags)
        b2.flags[:] = value
        assert not (batch.flags == 0xFF).any()
        v2, r2 = eng.evaluate_batch_routes(b2)
        assert (r2 == want_routes).all(), value
        H.assert_verdicts_equal(v2, RW.oracle_verdicts(KNOWN_RULES, KNOWN_LISTS, None, b2), b2, f"flags {value}")
    eng.close()
    # with a catch-all route at the end nothing is unrouted; with the gates off the routes are the same
    _, r3 = run("catch-all", KNOWN_RULES, KNOWN_ROUTES + [("default", None)], batch, KNOWN_LISTS)
    assert (r3[want_routes >= 0] == want_routes[want_routes >= 0]).all() and (r3[want_routes < 0] == len(KNOWN_ROUTES)).all()
    _, r4 = run("no gates", KNOWN_RULES, KNOWN_ROUTES, batch, KNOWN_LISTS, flags=RW.NO_GATES)
    assert (r4 == want_routes).all()


# ---------------------------------------------------------------------------------------------------------
# 2. group edges
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_group_edges(n):
    batch, want, want_routes = known_case()
    for lo in (0, 300):
        run(f"n {n} from {lo}", KNOWN_RULES, KNOWN_ROUTES, batch.slice(lo, lo + n), KNOWN_LISTS, wants=(want[lo:lo + n], want_routes[lo:lo + n]))


# ---------------------------------------------------------------------------------------------------------
# 3. more than 64 candidates in one group (built like test_gpu_rule_hits.py::test_more_than_64_candidates_in_one_group)
# ---------------------------------------------------------------------------------------------------------
TOKENS = [f"q{k:03d}z" for k in range(160)]


def token_requests(n, seed, full_at, partial=None):
    reqs = H.fuzz_requests(random.Random(seed), n, False)
    for i in full_at:
        if i < n:
            reqs[i].path = reqs[i].url = "/" + "/".join(TOKENS) if partial is None or i % 2 else "/" + "/".join(TOKENS[k] for k in partial)
            reqs[i].method, reqs[i].user_agent, reqs[i].captcha_verified = "GET", "Mozilla/5.0", False  # (no gate answers it; a Captcha rule takes effect)
    return RequestBatch.from_requests(reqs)


@pytest.mark.parametrize("layout", ["second_chunk", "third_chunk", "decided_first", "routes_before_rules_end"])
def test_more_than_64_candidates_in_one_group(layout):
    acts = [[CAP], [B], [CAP, B], [B, CAP], [CAP, CAP]]
    rule_tok = lambda k: (f"t{k}", f'http_request.path.contains("{TOKENS[k]}")', acts[k % 5])
    route_tok = lambda k: (f"s{k}", f'http_request.path.contains("{TOKENS[k]}") && http_request.method == "GET"')
    n, at = 200, (3, 17, 62, 63, 64, 130, 199)
    if layout == "second_chunk":
        # 70 token rules that all match the marked requests, then routes: the deciding route is candidate ~75
        rules, routes = [rule_tok(k) for k in range(70)], [("never", 'http_request.host == "~"')] + [route_tok(k) for k in range(70, 100)]
        batch = token_requests(n, 31, at)
    elif layout == "third_chunk":
        # 100 matching rules and 40 routes over tokens the odd marked requests lack: their first route is candidate ~ 145
        rules, routes = [rule_tok(k) for k in range(100)], [route_tok(k) for k in range(100, 160)]
        batch = token_requests(n, 32, at, partial=list(range(100)) + list(range(145, 160)))
    elif layout == "decided_first":
        # a match-all Block rule first: every request's verdict is known in the first chunk (pending == 0) while the routes are still ahead
        rules, routes = [("all", None, [B])] + [rule_tok(k) for k in range(130)], [route_tok(k) for k in range(130, 160)] + [("default", None)]
        batch = token_requests(n, 33, at)
    else:
        # the catch-all is the FIRST route: every request's route is known (rpending == 0) at the first route candidate, in the chunk
        # where the rules' candidates end, while 60 more route candidates follow and nobody's verdict is decided (pending != 0 to the end)
        rules = [(f"t{k}", f'http_request.path.contains("{TOKENS[k]}") && http_request.host == "~"', acts[k % 5]) for k in range(100)]
        routes = [("default", None)] + [route_tok(k) for k in range(100, 160)]
        batch = token_requests(n, 34, at)
    for flags in (0, _abi.OPT_TINY_VERDICT_SLOTS, _abi.OPT_GLOBAL_VERDICT_TABLES):
        got, r = run(f"{layout}, flags {flags}", rules, routes, batch, flags=flags)
    marked = np.array([i for i in at if i < n])
    if layout == "second_chunk":
        assert (r[marked] == 1).all() and (got["rule_idx"][marked] == 0).all()
    elif layout == "third_chunk":
        assert set(r[marked].tolist()) == {0, 45}
    elif layout == "decided_first":
        ungated = ~np.isin(got["rule_idx"], (_abi.RULE_UA_GATE, _abi.RULE_CAPTCHA_ENDPOINT))
        assert (got["rule_idx"][ungated] == 0).all() and (r[marked] == 0).all() and (np.delete(r, marked) == 30).all()
    else:
        assert (r == 0).all() and (got["action"][~np.isin(got["rule_idx"], (_abi.RULE_UA_GATE, _abi.RULE_CAPTCHA_ENDPOINT))] == 0).all()


# ---------------------------------------------------------------------------------------------------------
# 4. lazy comparison atoms in a route
# ---------------------------------------------------------------------------------------------------------
def test_lazy_comparison_atoms_in_a_route():
    """`http_request.url.length() > c && <rare literal>`: the comparison is no trigger, so the verdict kernel evaluates it only for the
    routes whose literal holds for somebody in the group — exactly, although a route never fires"""
    rng = random.Random(5)
    words = ["".join(rng.choice("bcdfgklmnprstvz") for _ in range(5)) for _ in range(24)]
    cmp_ = lambda k: [f"http_request.url.length() > {12 + k}", f"client.remote_port <= {1000 * (k + 1)}", f"http_request.path.length() == {12 + k % 7}", f"!(http_request.url.length() < {15 + k})"][k % 4]
    routes = [(f"s{k}", f'{cmp_(k)} && http_request.path.contains("{w}")') for k, w in enumerate(words[:16])]
    rules = [(f"l{k}", f'http_request.path.contains("{w}") && {cmp_(k)}', [[CAP], [B], [CAP, B]][k % 3]) for k, w in enumerate(words[12:], 12)]
    reqs = []
    for i in range(700):
        w = rng.choice(words) if rng.random() < 0.7 else "aeiou"
        path = "/" + "y" * rng.randint(0, 30) + w + "u" * rng.randint(0, 6)
        reqs.append(Request(host="h", url=path + rng.choice(["", "?zz", "?a=1"]), path=path, method="GET", user_agent="Mozilla/5.0", ip="9.9.9.9",
                            remote_port=rng.choice([443, 80, 999, 5000, 20000, 65535]), captcha_verified=rng.random() < 0.5))
    batch = RequestBatch.from_requests(reqs)
    wants = RW.oracle_verdicts(rules, None, None, batch), RW.oracle_routes(routes, None, None, batch)
    literal = np.array([[w.encode() in batch.field_bytes(2, i) for i in range(batch.n)] for w in words[:16]])
    hit = np.array([wants[1] == k for k in range(16)])
    # for several routes: requests with literal and comparison, and requests with the literal alone (no route)
    assert sum(1 for k in range(16) if hit[k].any() and (literal[k] & ~hit[k]).any()) >= 8 and (wants[1] == -1).sum() > 100
    _, lazy = run("lazy", rules, routes, batch, wants=wants)
    _, eager = run("eager", rules, routes, batch, flags=_abi.OPT_EAGER_CMP, wants=wants)
    assert (lazy == eager).all()
    run("lazy, tiny", rules, routes, batch, flags=_abi.OPT_TINY_VERDICT_SLOTS, wants=wants)
    run("lazy, global tables", rules, routes, batch, flags=_abi.OPT_GLOBAL_VERDICT_TABLES, wants=wants)


# ---------------------------------------------------------------------------------------------------------
# 5. kernel variants
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [_abi.OPT_GLOBAL_VERDICT_TABLES, _abi.OPT_TINY_VERDICT_SLOTS, _abi.OPT_GLOBAL_VERDICT_TABLES | _abi.OPT_TINY_VERDICT_SLOTS])
def test_verdict_kernel_variants(flags):
    batch, want, want_routes = known_case()
    run(f"flags {flags}", KNOWN_RULES, KNOWN_ROUTES, batch, KNOWN_LISTS, flags=flags, wants=(want, want_routes))


def test_more_than_64_passes():
    ps = H.pinned_passes("confirm_walk", 65)
    assert ps.n_passes == 65
    batch = RequestBatch.from_requests(H.pinned_requests(random.Random(6), ps, 130, hit=0.5))
    cut = len(ps.rules) * 2 // 3
    rules, routes = ps.rules[:cut], [(n, e) for n, e, _ in ps.rules[cut:]]
    for flags in (0, _abi.OPT_GLOBAL_VERDICT_TABLES):
        eng = RuleEngine(rules, {}, None, routes=routes, flags=flags, **ps.opts)
        assert eng.stats()["n_dfa_groups"] == 65  # (the routes' patterns stay in the passes they had as rules)
        eng.close()
        _, r = run(f"65 passes, flags {flags}", rules, routes, batch, {}, flags=flags, **ps.opts)
    assert len(set(r.tolist())) > 8


@pytest.mark.parametrize("jit", [True, False])
def test_a_residual_route(jit):
    rng = random.Random(8)
    rules = [("long", "http_request.url.length() - http_request.path.length() > 2 && client.remote_port % 2 == 1", [CAP]), ("a", 'http_request.path.contains("a/")', [B])]
    routes = [("odd", "client.remote_port % 3 == 1 && http_request.url.length() - http_request.path.length() >= 1"), ("b", 'http_request.path.contains("b")'),
              ("sum", 'http_request.host.length() + http_request.path.length() == 7'), ("default", None)]
    batch = RequestBatch.from_requests(H.fuzz_requests(rng, 400, False))
    eng = RuleEngine(rules, None, None, routes=routes, flags=0 if jit else _abi.OPT_NO_RESIDUAL_JIT)
    assert eng.residual_mode == (2 if jit else 1), eng.residual_fallback
    want, want_routes = RW.oracle_verdicts(rules, None, None, batch), RW.oracle_routes(routes, None, None, batch)
    assert set(want_routes.tolist()) == {0, 1, 2, 3}
    check(f"residual route, jit {jit}", eng, batch, want, want_routes)
    # the routes' execution-error counters follow the rules'; asking for the rules' alone still works
    assert eng.rule_errors(len(rules) + len(routes)) == [0] * 6 and eng.rule_errors(len(rules)) == [0, 0]
    eng.close()


def test_routes_beside_rule_hits_and_geo_answers():
    """one engine with routes, PWAF_OPT_RULE_HITS and PWAF_OPT_GEO_ANSWERS: each report through its own entry point"""
    from pingoo_amd.batch import hits_to_matrix

    rng = random.Random(9)
    lists, geo = H.fuzz_lists(rng), H.fuzz_geoip(rng)
    rules = [("a", 'http_request.path.contains("a/")', [CAP]), ("nets", 'lists["nets"].contains(client.ip)', [B]), ("watch", 'http_request.url.ends_with("b")', []), ("port", "client.remote_port < 80", [CAP, B])]
    routes = [("fr", 'client.country == "FR"'), ("ab", 'http_request.host.contains("ab")'), ("nets2", 'lists["nets2"].contains(client.ip)')]
    batch = RequestBatch.from_requests(H.fuzz_requests(rng, 500, True))  # (the batch carries asn / country itself)
    want, want_routes = RW.oracle_verdicts(rules, lists, geo, batch), RW.oracle_routes(routes, lists, geo, batch)
    assert set(want_routes.tolist()) == {-1, 0, 1, 2}
    eng = RuleEngine(rules, lists, geo, routes=routes, flags=_abi.OPT_RULE_HITS | _abi.OPT_GEO_ANSWERS)
    check("routes + hits + geo", eng, batch, want, want_routes)
    got, hits, rule_hits = eng.evaluate_batch_hits(batch)
    H.assert_verdicts_equal(got, want, batch, "hits call")
    m = hits_to_matrix(hits, batch.n, len(rules))  # (asserts that no entry names an index >= n_rules: a route is never reported as a rule)
    assert rule_hits.tolist() == m.sum(axis=1).tolist() and m[2].any() and not (want["rule_idx"] == 2).any()
    bare = RuleEngine(rules, lists, geo, flags=_abi.OPT_RULE_HITS | _abi.OPT_GEO_ANSWERS)
    got_b, hits_b, rule_hits_b = bare.evaluate_batch_hits(batch)
    assert (np.sort(hits, order=["rule_idx", "group"]) == np.sort(hits_b, order=["rule_idx", "group"])).all() and rule_hits.tolist() == rule_hits_b.tolist()
    got_g, geo_rec = eng.evaluate_batch(batch, with_geo=True)
    assert geo_rec.dtype == GEO_DTYPE and (got_g == want).all() and (geo_rec == bare.evaluate_batch(batch, with_geo=True)[1]).all()
    bare.close()
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# 6. fuzz
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fuzz_routes_match_the_oracles(seed):
    rng = random.Random(52000 + seed)
    if seed % 2 == 0:  # the mixed grammar: column predicates, residual programs, static errors, lists, GeoIP
        lists, geo = H.fuzz_lists(rng), H.fuzz_geoip(rng)
        exprs = [H.rexpr(rng, lists) if rng.random() < 0.95 else None for _ in range(40)]
        reqs = H.fuzz_requests(rng, 300, seed % 4 == 2)
        rules, routes = RW.split(exprs, 24, rng, H.fuzz_actions)
    else:  # the literal-heavy grammar: prefilters, confirm tiers, header fields
        lists, geo = None, None
        exprs = [r[1] for r in H.lit_rules(rng, 40)]
        reqs = H.lit_requests(rng, 300)
        rules, routes = RW.split(exprs, 24, rng, H.fuzz_actions)
        rules, routes = [("names", RW.NAMES_EXPR, [B])] + rules, [("names", RW.NAMES_EXPR)] + routes
    batch = RequestBatch.from_requests(reqs)
    want, want_routes = RW.oracle_verdicts(rules, lists, geo, batch), RW.oracle_routes(routes, lists, geo, batch)
    assert len(set(want_routes.tolist())) >= 2
    for flags in (0, _abi.OPT_TINY_VERDICT_SLOTS, _abi.OPT_NO_RESIDUAL_JIT):
        eng = RuleEngine(rules, lists, geo, routes=routes, flags=flags | _abi.OPT_LENIENT)
        try:
            assert not eng.partial and (seed % 2 == 0 or eng.header_names == RW.HEADERS)
            for n in (65, 300):
                check(f"seed {seed}, flags {flags}, n {n}", eng, batch.slice(0, n), want[:n], want_routes[:n])
        finally:
            eng.close()


# ---------------------------------------------------------------------------------------------------------
# 7. entry points
# ---------------------------------------------------------------------------------------------------------
def test_device_entry_point_on_a_stream_with_match_idx():
    import torch

    batch, want, want_routes = known_case()
    eng = RuleEngine(KNOWN_RULES, KNOWN_LISTS, None, routes=KNOWN_ROUTES)
    db = DeviceBatch(batch)
    d_route = torch.full((batch.n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    d_idx, d_nm = torch.zeros(batch.n, dtype=torch.int32, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
    d_counts = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    out = eng.evaluate_device(db, counts=d_counts, match_idx=d_idx, n_matches=d_nm, stream=stream.cuda_stream, route=d_route)
    stream.synchronize()
    eng.device_status()
    assert (out.cpu().numpy().view(want.dtype).reshape(-1) == want).all()
    back = d_route.cpu().numpy()
    assert (back[:batch.n] == want_routes).all() and (back[batch.n:] == 0x5A5A5A5A).all()  # (nothing beyond route + n is written)
    n_hit = int((want["action"] != 0).sum())
    assert int(d_nm.item()) == n_hit and sorted(d_idx.cpu().numpy()[:n_hit].tolist()) == np.nonzero(want["action"])[0].tolist()
    assert d_counts.cpu().tolist() == np.bincount(want["action"], minlength=4).tolist()
    eng.close()


def test_one_request_and_large_host_batch():
    batch, want, want_routes = known_case()
    eng = RuleEngine(KNOWN_RULES, KNOWN_LISTS, None, routes=KNOWN_ROUTES)
    reqs = [Request(host="api.example.com", path="/x/y.css", url="/x/y.css", ip="10.1.1.1", user_agent="Mozilla/5.0"),
            Request(host="www.example.com", path="/v2/123/items", url="/v2/123/items", ip="8.8.8.8", user_agent=""),
            Request(host="www.example.com", path="/nothing", url="/nothing", ip="8.8.8.8", user_agent="Mozilla/5.0", captcha_verified=True)]
    one = RequestBatch.from_requests(reqs)
    w, wr = RW.oracle_verdicts(KNOWN_RULES, KNOWN_LISTS, None, one), RW.oracle_routes(KNOWN_ROUTES, KNOWN_LISTS, None, one)
    assert wr.tolist() == [0, 4, -1]
    for i, r in enumerate(reqs):
        v, k = eng.evaluate_routed(r)
        assert (int(v.decision), k) == (int(w[i]["action"]), int(wr[i])) and int(eng.evaluate(r).decision) == int(w[i]["action"])
    # pwaf_evaluate_one_route with route == NULL is pwaf_evaluate_one
    from pingoo_amd.engine import _request_struct
    st, _keep = _request_struct(reqs[0], eng.header_names)
    out = _abi.Verdict()
    assert lib().pwaf_evaluate_one_route(eng._h, C.byref(st), C.byref(out), None) == 0 and out.action == w[0]["action"]
    # a batch too large for the packed staging block: the column-by-column path and its staging buffer
    big = batch.tile(40)
    check("large host batch", eng, big, np.tile(want, 40), np.tile(want_routes, 40))
    eng.close()


def test_null_route_is_the_plain_call_and_no_routes_is_unsupported():
    import torch

    batch, want, want_routes = known_case()
    plain_eng = RuleEngine(KNOWN_RULES, KNOWN_LISTS, None)
    empty_eng = RuleEngine(KNOWN_RULES, KNOWN_LISTS, None, routes=[])
    routed = RuleEngine(KNOWN_RULES, KNOWN_LISTS, None, routes=KNOWN_ROUTES)
    db = DeviceBatch(batch)
    d_route = torch.full((batch.n,), 7, dtype=torch.int32, device="cuda:0")
    for eng in (plain_eng, empty_eng):
        assert lib().pwaf_engine_route_count(eng._h) == 0
        for call in (lambda: eng.evaluate_batch_routes(batch), lambda: eng.evaluate_device(db, route=d_route), lambda: eng.evaluate_routed(Request(host="h", path="/", url="/"))):
            eng.set_profiling(1)
            with pytest.raises(UnsupportedExpression, match="without routes") as ei:
                call()
            assert ei.value.code == _abi.E_UNSUPPORTED and eng.kernel_times() == []  # (nothing was launched)
            eng.set_profiling(0)
    assert (d_route.cpu().numpy() == 7).all()
    st = batch.as_struct(routed.header_names)

    def names(eng, call):
        eng.set_profiling(1)
        out = call(eng)
        t = [k[0] for k in eng.kernel_times()]
        eng.set_profiling(0)
        return t, out

    def null_route(eng):
        out = np.zeros(batch.n, dtype=want.dtype)
        assert lib().pwaf_evaluate_batch_routes(eng._h, C.byref(st), out.ctypes.data, None, None) == 0
        return out

    def null_route_device(eng):
        out = torch.zeros((batch.n, 2), dtype=torch.int32, device="cuda:0")
        stc = db.as_struct(eng.header_names)
        assert lib().pwaf_evaluate_device_routes(eng._h, C.byref(stc), out.data_ptr(), None, None, None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        return out.cpu().numpy().view(want.dtype).reshape(-1)

    # the launch list of an engine is its own (a routed program has more atoms, so other passes): per engine, the NULL-route call and the
    # route call launch what its plain call launches; the verdicts are the same across the engines
    base, plain = names(plain_eng, lambda e: e.evaluate_batch(batch))
    assert "verdict" in base
    H.assert_verdicts_equal(plain, want, batch, "no routes")
    base_routed, out = names(routed, lambda e: e.evaluate_batch(batch))
    assert "verdict" in base_routed and (out == plain).all()  # a routed engine through the plain entry point: the verdicts of the engine without routes
    cases = {"routed engine, NULL route": (base_routed, names(routed, null_route)), "no routes, NULL route": (base, names(plain_eng, null_route)),
             "routed engine, routes": (base_routed, names(routed, lambda e: e.evaluate_batch_routes(batch)[0]))}
    for label, (expect, (t, out)) in cases.items():
        assert t == expect, label  # (the route answer adds no launch either)
        assert (out == plain).all(), label
    device = lambda e: e.evaluate_device(db).cpu().numpy().view(want.dtype).reshape(-1)
    for eng in (plain_eng, routed):
        base_dev, out = names(eng, device)
        t, out2 = names(eng, null_route_device)
        assert t == base_dev and (out == plain).all() and (out2 == plain).all()
    for eng in (plain_eng, empty_eng, routed):
        eng.close()


# ---------------------------------------------------------------------------------------------------------
# 8. many workgroups
# ---------------------------------------------------------------------------------------------------------
def test_many_workgroups():
    rng = random.Random(10)
    exprs = [r[1] for r in H.lit_rules(rng, 60)]
    rules, routes = RW.split(exprs, 44, rng, H.fuzz_actions)
    rules, routes = [("names", RW.NAMES_EXPR, [B])] + rules, [("names", RW.NAMES_EXPR)] + routes
    base = RequestBatch.from_requests(H.lit_requests(rng, 5000))  # (5000 is no multiple of 64: every copy sits differently in its groups)
    batch = base.take(np.arange(100000) % 5000)
    eng = RuleEngine(rules, None, None, routes=routes)
    got, r, counts = eng.evaluate_batch_routes(batch, with_counts=True)
    assert (eng.evaluate_batch(batch) == got).all() and counts.tolist() == np.bincount(got["action"], minlength=4).tolist()
    eng.close()
    router = ServiceRouter(routes)
    assert (router.route_batch(batch) == r).all()
    router.close()
    assert len(set(r.tolist())) > 6 and (r == -1).any() and len(set(got["rule_idx"].tolist())) > 5
    sample = np.sort(np.random.default_rng(10).choice(batch.n, 2000, replace=False))
    sub = batch.take(sample)
    H.assert_verdicts_equal(got[sample], RW.oracle_verdicts(rules, None, None, sub), sub, "sample")
    assert (r[sample] == RW.oracle_routes(routes, None, None, sub)).all()
