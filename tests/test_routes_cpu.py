"""Service routes compiled beside the rules (pwaf_program_compile_routed), the part that needs no device: without routes nothing differs;
the compiled tables — read by tests/routed_walker.py — give the rules' oracle's verdicts and the routes' oracle's routes; today's
table walker still reads a routed dump; routes share the rules' atoms and scan passes; what is refused; struct layout and NULL checks."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import helpers as H
import routed_walker as RW
from pingoo_amd import Request, RequestBatch, _abi, geoip_entries
from pingoo_amd.engine import CompiledProgram, PwafError, UnsupportedExpression, lib
from table_walker import Tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
RULES = [("env", 'http_request.path.starts_with("/.env")', [B]), ("bot", 'http_request.user_agent.contains("bot") && client.remote_port < 1024', [CAP]),
         ("office", 'lists["office"].contains(client.ip) && http_request.path.starts_with("/admin")', [CAP, B]),
         ("len", "http_request.url.length() - http_request.path.length() > 9", [B])]
LISTS = {"office": (_abi.LIST_IP, ["10.0.0.0/8", "2001:db8::/32"])}
GEO = geoip_entries([("8.8.8.0/24", 15169, "US"), ("5.5.0.0/16", 64512, "KP"), ("10.0.0.0/8", 3, "FR")])
ROUTES = [("api", 'http_request.host.starts_with("api.")'), ("broken", "http_request.path"), ("office", 'lists["office"].contains(client.ip) && http_request.host == "admin.example.com"'),
          ("kp", 'client.country == "KP"'), ("residual", "http_request.url.length() - http_request.path.length() > 3 && client.remote_port % 2 == 1"),
          ("static", 'http_request.path.starts_with("/static/") || http_request.path.ends_with(".css")'), ("never", "false"), ("v2", 'http_request.url.matches("^/v2/[0-9]+")'),
          ("default", None), ("shadowed", 'http_request.host == "x"')]


def hand_requests(n=160):
    rng = random.Random(12)
    hosts = ["api.example.com", "www.example.com", "admin.example.com", "api", "", "x"]
    paths = ["/static/a.js", "/x/y.css", "/v2/123/items", "/v2/abc", "", "/index.html", "/.env", "/admin/x", "/__pingoo/captcha/init"]
    reqs = []
    for _ in range(n):
        p = rng.choice(paths)
        reqs.append(Request(host=rng.choice(hosts), path=p, url=(p or "/") + rng.choice(["", "?a=1", "?q=0123456789"]), ip=rng.choice(["10.1.1.1", "8.8.8.8", "5.5.1.1", "2001:db8::7", "9.9.9.9"]),
                            user_agent=rng.choice(["Mozilla/5.0", "bot/1", "", "x" * 256]), remote_port=rng.choice([80, 443, 1023, 40001, 40002]), captcha_verified=rng.random() < 0.3))
    return RequestBatch.from_requests(reqs)


def walk_routed(prog, batch):
    t = RW.RoutedTables(prog)
    got = np.zeros(batch.n, dtype=[("action", np.uint8), ("rule_idx", np.uint32)])
    route = np.zeros(batch.n, dtype=np.int32)
    for i in range(batch.n):
        a, r, k = t.evaluate_routed(batch, i)
        got[i], route[i] = (a, r), k
    return got, route


def walk_plain(prog, batch):
    """today's walker, unmodified, on the same dump"""
    t = Tables(prog)
    got = np.zeros(batch.n, dtype=[("action", np.uint8), ("rule_idx", np.uint32)])
    for i in range(batch.n):
        got[i] = t.evaluate(batch, i)
    return got


def check_program(label, rules, routes, lists, geo, batch, flags=0, **opts):
    prog = CompiledProgram(rules, lists, geo, routes=routes, flags=flags, **opts)
    assert [prog.rule_status(i)[0] for i in range(len(rules) + len(routes))] == [0] * (len(rules) + len(routes)), label
    assert prog.stats()["n_routes"] == len(routes) == lib().pwaf_program_route_count(prog._h)
    want, want_routes = RW.oracle_verdicts(rules, lists, geo, batch, flags & RW.NO_GATES), RW.oracle_routes(routes, lists, geo, batch)
    got, got_routes = walk_routed(prog, batch)
    H.assert_verdicts_equal(got, want, batch, label)
    bad = np.nonzero(got_routes != want_routes)[0]
    assert len(bad) == 0, f"{label}: {len(bad)} routes differ; first at {bad[0]}: got {got_routes[bad[0]]} want {want_routes[bad[0]]} ({routes})"
    H.assert_verdicts_equal(walk_plain(prog, batch), want, batch, label + " (table_walker.Tables)")
    return prog, want, want_routes


@pytest.mark.parametrize("flags", [0, _abi.OPT_NO_UA_GATE, RW.NO_GATES | _abi.OPT_EAGER_CMP, _abi.OPT_TINY_VERDICT_SLOTS | _abi.OPT_GLOBAL_VERDICT_TABLES, _abi.OPT_RULE_HITS | _abi.OPT_GEO_ANSWERS,
                                   _abi.OPT_SPARSE_VERDICT, _abi.OPT_DENSE_VERDICT, _abi.OPT_NO_PREFILTER | _abi.OPT_NO_RESIDUAL_JIT])
def test_without_routes_the_dump_is_the_plain_one(flags):
    plain = CompiledProgram(RULES, LISTS, GEO, flags=flags)
    routed = CompiledProgram(RULES, LISTS, GEO, routes=[], flags=flags)
    assert routed.dump() == plain.dump() and b"ROUT" not in plain.dump()
    assert routed.stats() == plain.stats() and routed.stats()["n_routes"] == 0 and routed.warnings() == plain.warnings()
    assert b"ROUT" in CompiledProgram(RULES, LISTS, GEO, routes=ROUTES[:1], flags=flags & ~(_abi.OPT_SPARSE_VERDICT | _abi.OPT_DENSE_VERDICT)).dump()


@pytest.mark.parametrize("flags", [0, RW.NO_GATES, _abi.OPT_NO_RESIDUAL])
def test_hand_written_set_through_the_compiled_tables(flags):
    batch = hand_requests()
    routes = [r for r in ROUTES if not (flags & _abi.OPT_NO_RESIDUAL and r[0] == "residual")]
    rules = [r for r in RULES if not (flags & _abi.OPT_NO_RESIDUAL and r[0] == "len")]
    prog, want, want_routes = check_program(f"hand-written, flags {flags}", rules, routes, LISTS, GEO, batch, flags)
    names = [n for n, _ in routes]
    seen = {names[k] if k >= 0 else None for k in set(want_routes.tolist())}
    # every kind of route decides somebody; the non-Bool route, the constant-false one and the one behind the catch-all nobody
    assert seen == set(names) - {"broken", "never", "shadowed"}, seen
    t = RW.RoutedTables(prog)
    assert t.n_routes == len(routes) and t.n_user_rules == len(rules)
    assert [int(x) for x in t.rules["public_idx"][t.route_base:]] == [k for k, n in enumerate(names) if n not in ("broken", "never")]  # (never-matching routes are dropped)
    if not flags & _abi.OPT_NO_RESIDUAL:
        assert any("route #4" in w and "residual" in w for w in prog.warnings()), prog.warnings()
    # the routes answer whatever the verdict is: some blocked and some gated request has a route other than the catch-all
    decided = want["action"] != _abi.ACTION_ALLOW
    assert (decided & (want_routes >= 0) & (want_routes != names.index("default"))).any()
    # without the catch-all some request has no route
    no_default = [r for r in routes if r[1] is not None]
    _, _, r2 = check_program("no catch-all", rules, no_default, LISTS, GEO, batch, flags)
    assert (r2 == -1).any() and (r2[r2 >= 0] == want_routes[r2 >= 0]).all()


@pytest.mark.parametrize("seed", range(6))
def test_fuzzed_sets_through_the_compiled_tables(seed):
    """helpers.rexpr (the mixed grammar: columns, residual programs, static errors) and helpers.lit_pred (literal-heavy, header fields),
    each generated set split into rules and routes"""
    rng = random.Random(7100 + seed)
    if seed % 2 == 0:
        lists, geo = H.fuzz_lists(rng), H.fuzz_geoip(rng)
        exprs = [H.rexpr(rng, lists) if rng.random() < 0.93 else None for _ in range(rng.randint(4, 14))]
        batch = RequestBatch.from_requests(H.fuzz_requests(rng, 48, seed % 4 == 0))
        n_rules = rng.randint(0, len(exprs) - 1)
        rules, routes = RW.split(exprs, n_rules, rng, H.fuzz_actions)
    else:
        lists, geo = {}, None
        exprs = [r[1] for r in H.lit_rules(rng, rng.randint(4, 14))]
        batch = RequestBatch.from_requests(H.lit_requests(rng, 48))
        rules, routes = RW.split(exprs, rng.randint(1, len(exprs) - 1), rng, H.fuzz_actions)
        rules, routes = [("names", RW.NAMES_EXPR, [B])] + rules, [("names", RW.NAMES_EXPR)] + routes
    flags = rng.choice([0, _abi.OPT_NO_UA_GATE, RW.NO_GATES])
    prog, _, _ = check_program(f"seed {seed}", rules, routes, lists, geo, batch, flags, max_table_bytes=rng.choice([0, 2048]))
    if seed % 2:
        assert prog.header_names == RW.HEADERS


def test_routes_share_the_rules_atoms_and_passes():
    rules = [("h", 'http_request.host.contains("internal")', [B]), ("p", 'http_request.path.starts_with("/admin") && client.remote_port == 7', [CAP])]
    base = CompiledProgram(rules).stats()
    same = CompiledProgram(rules, routes=[("again", 'http_request.host.contains("internal")'), ("both", 'http_request.path.starts_with("/admin") && !(client.remote_port == 7)')]).stats()
    assert same["n_atoms"] == base["n_atoms"] and same["n_dfa_groups"] == base["n_dfa_groups"] and same["n_rules"] == base["n_rules"] + 2
    more = CompiledProgram(rules, routes=[("api", 'http_request.host.starts_with("api.")')]).stats()
    assert more["n_atoms"] == base["n_atoms"] + 1 and more["n_scan_atoms"] == base["n_scan_atoms"] + 1
    assert more["n_dfa_groups"] == base["n_dfa_groups"]  # the new literal over `host` joins the pass the rules' pattern already streams
    # ... and the header names are collected over the rules, then the routes
    prog = CompiledProgram([("r", 'http_request.headers["x-b"] == "1"', [B])], routes=[("s", 'http_request.headers["x-a"] == "1"'), ("t", 'http_request.headers["x-b"] == "2"')])
    assert prog.header_names == ["x-b", "x-a"]


def test_a_route_no_compiler_takes_is_refused_by_its_index():
    bad = ("bad", "http_request.path.matches(http_request.host)")
    for k, routes in ((0, [bad, ROUTES[0]]), (2, ROUTES[:2] + [bad])):
        with pytest.raises(UnsupportedExpression, match=rf"^\[-3\] route #{k}|route #{k}") as ei:
            CompiledProgram(RULES, LISTS, GEO, routes=routes)
        assert ei.value.code == _abi.E_UNSUPPORTED and ei.value.rule_index == len(RULES) + k and str(ei.value).split("] ", 1)[-1].startswith(f"route #{k}")
        prog = CompiledProgram(RULES, LISTS, GEO, routes=routes, flags=_abi.OPT_LENIENT)
        assert prog.partial
        status = [prog.rule_status(i) for i in range(len(RULES) + len(routes))]
        assert [s[0] for s in status] == [0] * (len(RULES) + k) + [_abi.E_UNSUPPORTED] + [0] * (len(routes) - k - 1)
        assert status[len(RULES) + k][1].startswith(f"route #{k}") and prog.rule_status(len(RULES) + len(routes))[0] == _abi.E_INVALID_ARG
        batch = hand_requests(64)
        _, route = walk_routed(prog, batch)
        assert (route != k).all()  # that route never matches; the others are the oracle's with `false` in its place
        seen = [(n, "false" if n == "bad" else e) for n, e in routes]
        assert (route == RW.oracle_routes(seen, LISTS, GEO, batch)).all()
    # a syntax error in a route names the route too
    with pytest.raises(PwafError, match="route #1") as ei:
        CompiledProgram(RULES, LISTS, GEO, routes=[ROUTES[0], ("syntax", "a ==")])
    assert ei.value.code == _abi.E_SYNTAX and ei.value.rule_index == len(RULES) + 1


def test_a_route_refused_at_dnf_conversion_names_the_route_too():
    """the second place a route can be refused: its DNF is larger than the device limit (and no residual program may take it)"""
    big = " && ".join(f'(http_request.path.contains("a{k}x") || http_request.url.contains("b{k}y"))' for k in range(14))
    routes, flags = [("ok", None), ("big", big)], _abi.OPT_NO_RESIDUAL
    with pytest.raises(UnsupportedExpression, match="route #1: expression too complex") as ei:
        CompiledProgram(RULES[:1], routes=routes, flags=flags)
    assert ei.value.rule_index == 2
    prog = CompiledProgram(RULES[:1], routes=routes, flags=flags | _abi.OPT_LENIENT)
    assert prog.partial and prog.rule_status(1)[0] == 0
    code, text = prog.rule_status(2)
    assert code == _abi.E_UNSUPPORTED and text.startswith("route #1: expression too complex"), text
    assert any(w.startswith("route #1 is NOT evaluated") for w in prog.warnings())


@pytest.mark.parametrize("variant", [_abi.OPT_SPARSE_VERDICT, _abi.OPT_DENSE_VERDICT, _abi.OPT_SPARSE_VERDICT | _abi.OPT_TINY_VERDICT_SLOTS])
def test_routes_are_refused_beside_the_column_file_verdict_kernels(variant):
    with pytest.raises(PwafError, match="routes") as ei:
        CompiledProgram(RULES, LISTS, GEO, routes=ROUTES, flags=variant)
    assert ei.value.code == _abi.E_INVALID_ARG
    CompiledProgram(RULES, LISTS, GEO, routes=[], flags=variant)
    CompiledProgram(RULES, LISTS, GEO, flags=variant)
    CompiledProgram(RULES, LISTS, GEO, routes=ROUTES, flags=_abi.OPT_TINY_VERDICT_SLOTS | _abi.OPT_GLOBAL_VERDICT_TABLES | _abi.OPT_RULE_HITS)


def test_struct_layout_against_c_compiler_and_null_engine(tmp_path):
    prog = tmp_path / "sizes.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pwaf.h"\nint main(void){printf("%zu %zu %zu %zu %u\\n",sizeof(pwaf_route_desc),offsetof(pwaf_route_desc,name),'
                    'offsetof(pwaf_route_desc,expression),offsetof(pwaf_route_desc,reserved),PWAF_ROUTE_NONE);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = _abi.RouteDesc
    assert got == [C.sizeof(D), D.name.offset, D.expression.offset, D.reserved.offset, _abi.ROUTE_NONE] == [24, 0, 8, 16, 0xFFFFFFFF]
    L = lib()
    st, req = _abi.Batch(), _abi.Request()
    out, route, h = (C.c_uint64 * 4)(7, 7, 7, 7), (C.c_uint32 * 4)(9, 9, 9, 9), C.c_void_p(5)
    assert L.pwaf_evaluate_batch_routes(None, C.byref(st), out, None, route) == _abi.E_INVALID_ARG
    assert L.pwaf_evaluate_device_routes(None, C.byref(st), out, None, None, None, route, None) == _abi.E_INVALID_ARG
    assert L.pwaf_evaluate_one_route(None, C.byref(req), C.cast(out, C.POINTER(_abi.Verdict)), route) == _abi.E_INVALID_ARG
    assert L.pwaf_engine_route_count(None) == 0 and L.pwaf_program_route_count(None) == 0
    err = _abi.CompileError()
    assert L.pwaf_program_compile_routed(None, 1, None, 0, None, 0, None, None, C.byref(h), C.byref(err)) == _abi.E_INVALID_ARG
    assert L.pwaf_program_compile_routed(None, 0, None, 1, None, 0, None, None, C.byref(h), C.byref(err)) == _abi.E_INVALID_ARG
    assert L.pwaf_engine_create_routed(None, 0, None, 0, None, 0, None, None, None, C.byref(err)) == _abi.E_INVALID_ARG
    assert list(out) == [7] * 4 and list(route) == [9] * 4 and h.value == 5
    assert L.pwaf_abi_version() == 4 == _abi.ABI_VERSION
