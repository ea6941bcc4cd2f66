"""pwaf_respond (HOST mode) and pwaf_respond_one against the Python restatement of the listener's control flow (tests/respond_oracle.py:
http_listener.rs:196-272, captcha.rs:158-174): the full cross product of the table's inputs, every path edge, the lists at every cap edge
behind guard bytes, every refusal with its text, the per-request walk of a small routed rule set with a key set against a walk of the
listener assembled from the existing oracles, and csrc/respond.h under AddressSanitizer + UBSan as a stand-alone program
(tools/respond_host.cpp) over exact-size heap blocks. No GPU. docs/respond_edges.md says what each test pins."""
import ctypes as C
import ipaddress
import os
import subprocess

import numpy as np
import pytest

import cookie_oracle as CO
import respond_cases as RC
import respond_oracle as O
import routed_walker as RW
from pingoo_amd import RESPONSE_DTYPE, VERDICT_DTYPE, KeySet, Request, RequestBatch, _abi, respond, respond_one, respond_scan_shape, verify_cookie
from pingoo_amd.engine import CompiledProgram, PwafError, lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(ROOT, "tools", "respond_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "pingoo_amd", "csrc", "respond.h"), os.path.join(ROOT, "pingoo_amd", "csrc", "service.h"), os.path.join(ROOT, "include", "pwaf.h")]
HOST = RC.HostMem()
ALL = tuple(range(O.KINDS))
ENDPOINTS = (O.CAPTCHA_ASSET, O.CAPTCHA_INIT, O.CAPTCHA_VERIFY, O.CAPTCHA_NOT_FOUND)


def err():
    return lib().pwaf_last_error().decode()


def one(verdict, status, route, path):
    return respond_one(verdict, O.ABSENT if status is None else status, route, path)


def test_the_constants_and_layouts_are_the_header_s(tmp_path):
    prog = tmp_path / "resp.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pwaf.h"\nint main(void){printf("%u %u %u %u %u %u %u %u %u %u %u %u %zu %zu %zu %zu %zu\\n",PWAF_RESP_FORWARD,'
                    "PWAF_RESP_NOT_FOUND,PWAF_RESP_BLOCKED,PWAF_RESP_CAPTCHA_PAGE,PWAF_RESP_CAPTCHA_ASSET,PWAF_RESP_CAPTCHA_INIT,PWAF_RESP_CAPTCHA_VERIFY,PWAF_RESP_CAPTCHA_NOT_FOUND,"
                    "PWAF_RESP_HOST_DECIDES,PWAF_RESP_KINDS,PWAF_RESP_MAX_LISTS,PWAF_RULE_COOKIE,sizeof(pwaf_response),offsetof(pwaf_response,arg),sizeof(pwaf_resp_list),"
                    "offsetof(pwaf_resp_list,idx),offsetof(pwaf_resp_list,n));return 0;}\n")
    exe = tmp_path / "resp"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    kinds = [_abi.RESP_FORWARD, _abi.RESP_NOT_FOUND, _abi.RESP_BLOCKED, _abi.RESP_CAPTCHA_PAGE, _abi.RESP_CAPTCHA_ASSET, _abi.RESP_CAPTCHA_INIT, _abi.RESP_CAPTCHA_VERIFY,
             _abi.RESP_CAPTCHA_NOT_FOUND, _abi.RESP_HOST_DECIDES]
    assert got[:9] == kinds == list(range(9)) == [O.FORWARD, O.NOT_FOUND, O.BLOCKED, O.CAPTCHA_PAGE, O.CAPTCHA_ASSET, O.CAPTCHA_INIT, O.CAPTCHA_VERIFY, O.CAPTCHA_NOT_FOUND, O.HOST_DECIDES]
    assert got[9:12] == [_abi.RESP_KINDS, _abi.RESP_MAX_LISTS, _abi.RULE_COOKIE] == [O.KINDS, O.MAX_LISTS, O.RULE_COOKIE] and len(_abi.RESP_KIND_NAMES) == O.KINDS
    assert got[12:] == [C.sizeof(_abi.Response), _abi.Response.arg.offset, C.sizeof(_abi.RespList), _abi.RespList.idx.offset, _abi.RespList.n.offset] == [8, 4, 24, 8, 16]
    assert RESPONSE_DTYPE.itemsize == 8 and RESPONSE_DTYPE.fields["arg"][1] == 4
    shape = respond_scan_shape()
    assert shape["tile"] % 64 == 0 and shape["step"] % 64 == 0 and shape["max_lists"] == O.MAX_LISTS and shape["kinds"] == O.KINDS
    assert lib().pwaf_respond_scan_shape(None) == _abi.E_INVALID_ARG and lib().pwaf_respond_scratch_bytes(0) >= 64
    assert lib().pwaf_respond_scratch_bytes(shape["tile"] + 1) % 16 == 0


def test_the_full_cross_product_one_request_at_a_time():
    cases = O.cross_product()
    assert len(cases) == 4 * 4 * 5 * 3 * 6
    seen = set()
    for verdict, status, route, path in cases:
        want = O.decide(verdict, status, route, path)
        assert one(verdict, status, route, path) == want, (verdict, status, route, path)
        seen.add(want[0])
    assert seen == set(ALL), "the cross product reaches every kind"


@pytest.mark.parametrize("status, route", [(s, r) for s in ("column", None) for r in ("column", None)])
def test_the_full_cross_product_as_batches(status, route):
    """the HOST mode over the cross product, with and without a status and a route column (no column: the cases that name none)"""
    cases = [c for c in O.cross_product() if (c[1] is None) == (status is None) and (c[2] is None) == (route is None)]
    assert len(cases) >= 4 * 4 * 6
    verdicts, statuses, routes, paths = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases]
    got = RC.check(f"status {status} route {route}", HOST, verdicts, statuses if status else None, routes if route else None, paths, [ALL, ENDPOINTS, (O.BLOCKED,), (O.HOST_DECIDES, O.CAPTCHA_PAGE)])
    assert got[2][0][0] == list(range(len(cases)))


def test_the_rows_where_the_old_prose_and_the_reference_disagree():
    """an INVALID cookie does not turn gate A's or gate B's answer into a captcha page (:196 and :200 run before :222), and it does hide a Block rule's"""
    assert one((O.BLOCK, O.RULE_UA_GATE), O.INVALID, None, b"/x") == (O.BLOCKED, O.RULE_UA_GATE)
    assert one((O.BYPASS, O.RULE_CAPTCHA_ENDPOINT), O.INVALID, None, O.INIT) == (O.CAPTCHA_INIT, O.RULE_CAPTCHA_ENDPOINT)
    assert one((O.BYPASS, O.RULE_CAPTCHA_ENDPOINT), O.UNDECIDED, 2, O.VERIFY) == (O.CAPTCHA_VERIFY, O.RULE_CAPTCHA_ENDPOINT)
    assert one((O.BLOCK, 7), O.INVALID, None, b"/x") == (O.CAPTCHA_PAGE, O.RULE_COOKIE)
    assert one((O.BLOCK, 7), O.UNDECIDED, None, b"/x") == (O.HOST_DECIDES, 7)
    assert one((O.ALLOW, O.RULE_NONE), O.UNDECIDED, 1, b"/x") == (O.HOST_DECIDES, O.RULE_NONE)
    assert one((O.BLOCK, 7), O.VERIFIED, None, b"/x") == (O.BLOCKED, 7) and one((O.CAPTCHA, 8), O.ABSENT, 0, b"/x") == (O.CAPTCHA_PAGE, 8)
    assert one((O.ALLOW, O.RULE_NONE), O.VERIFIED, None, b"/x") == (O.FORWARD, O.ROUTE_NONE)
    assert one((O.ALLOW, O.RULE_NONE), O.ABSENT, 0, b"/x") == (O.FORWARD, 0) and one((O.ALLOW, O.RULE_NONE), O.ABSENT, O.ROUTE_NONE, b"/x") == (O.NOT_FOUND, O.ROUTE_NONE)


PATHS = O.path_cases()


def test_every_path_edge_one_request_at_a_time():
    by_hand = {"assets": O.CAPTCHA_ASSET, "assets + x": O.CAPTCHA_ASSET, "assets + /": O.CAPTCHA_ASSET, "assets less its last byte": O.CAPTCHA_NOT_FOUND, "init": O.CAPTCHA_INIT,
               "init + /": O.CAPTCHA_NOT_FOUND, "init + x": O.CAPTCHA_NOT_FOUND, "init less its last byte": O.CAPTCHA_NOT_FOUND, "verify": O.CAPTCHA_VERIFY, "verify + x": O.CAPTCHA_NOT_FOUND,
               "verify less its last byte": O.CAPTCHA_NOT_FOUND, "the prefix alone": O.CAPTCHA_NOT_FOUND, "the prefix + X": O.CAPTCHA_NOT_FOUND, "empty": O.CAPTCHA_NOT_FOUND,
               "outside the prefix": O.CAPTCHA_NOT_FOUND, "init in upper case": O.CAPTCHA_NOT_FOUND, "assets with byte 16 wrong": O.CAPTCHA_NOT_FOUND,
               "init with its last byte wrong": O.CAPTCHA_NOT_FOUND, "verify with byte 24 wrong": O.CAPTCHA_NOT_FOUND, "assets + 300": O.CAPTCHA_ASSET}
    assert {len(p) for _, p in PATHS} >= {0, 15, 16, 17, 23, 24, 25, 26, 27, 28, 29, 32, 300}
    for label, path in PATHS:
        want = O.decide((O.BYPASS, O.RULE_CAPTCHA_ENDPOINT), O.INVALID, 3, path)
        assert want[0] == by_hand.get(label, want[0]), label
        assert one((O.BYPASS, O.RULE_CAPTCHA_ENDPOINT), O.INVALID, 3, path) == want, label
        # the path counts for BYPASS alone
        assert one((O.ALLOW, O.RULE_NONE), O.ABSENT, 3, path) == (O.FORWARD, 3), label
    assert all(label in dict(PATHS) for label in by_hand)


@pytest.mark.parametrize("lead", [0, 1, 13])
def test_every_path_edge_as_one_batch_in_an_arena_without_a_pad(lead):
    """HOST mode reads no byte outside a path: the arena ends with the last path, and every path takes its turn at being the last"""
    paths = [p for _, p in PATHS]
    verdicts = [(O.BYPASS, O.RULE_CAPTCHA_ENDPOINT)] * len(paths)
    RC.check(f"lead {lead}", HOST, verdicts, None, None, paths, [ENDPOINTS, (O.CAPTCHA_VERIFY,)], lead=lead, pad=0)
    for k in (1, 2, 3, len(paths) // 2):
        RC.check(f"lead {lead}, rotated {k}", HOST, verdicts, None, None, paths[k:] + paths[:k], [(O.CAPTCHA_INIT, O.CAPTCHA_VERIFY)], lead=lead, pad=0)


def sample(n=300):
    return O.mixed_batch(n, seed=3)


def test_no_list_four_lists_every_mask_and_overlaps():
    v, s, r, p = sample()
    RC.check("no list", HOST, v, s, r, p)
    RC.check("no list, no counts", HOST, v, s, r, p, with_counts=False)
    RC.check("four lists", HOST, v, s, r, p, [(), ALL, (O.BLOCKED, O.CAPTCHA_PAGE), (O.CAPTCHA_PAGE, O.HOST_DECIDES, O.FORWARD)])
    for k in ALL:
        RC.check(f"kind {k} alone", HOST, v, s, r, p, [(k,)])
    RC.check("one kind a list, four at a time", HOST, v, s, r, p, [(0,), (1,), (2,), (3,)])
    RC.check("the same mask four times", HOST, v, s, r, p, [ENDPOINTS] * 4)
    got = RC.check("masks as integers", HOST, v, s, r, p, [0, 0x1FF, 0x100, 0x0F0])
    assert got[2][0] == ([], 0) and got[2][1][1] == len(v) == sum(got[1])


def test_every_cap_edge_and_count_only_lists():
    v, s, r, p = sample()
    _, counts, _ = O.expect_batch(v, s, r, p)
    for kinds in ((O.BLOCKED,), ENDPOINTS, ALL, (O.NOT_FOUND,)):
        c = sum(counts[k] for k in kinds)
        assert c > 1
        got = RC.check(f"kinds {kinds}", HOST, v, s, r, p, [kinds] * 4, caps=[0, c - 1, c, c + 1])
        assert [len(e) for e, _ in got[2]] == [0, c - 1, c, c] and all(m == c for _, m in got[2])
    RC.check("count only, with a list that has room", HOST, v, s, r, p, [ALL, (O.FORWARD,)], caps=[0, 1])


def test_no_request():
    got = RC.check("n == 0", HOST, [], [], [], [], [ALL, (), ENDPOINTS, (O.BLOCKED,)], caps=[4, 0, 1, 0])
    assert got[1] == [0] * O.KINDS and got[2] == [([], 0)] * 4
    RC.check("n == 0, no columns", HOST, [], None, None, [])
    c = RC.Call(HOST, [], None, None, [], [ALL])
    c.batch.field[2].data = c.batch.field[2].offsets = None  # (an empty batch may carry no path column)
    assert c.run() == _abi.OK and c.results()[2] == [([], 0)]


def test_the_wrapper_and_the_engine_s_method():
    v, s, r, p = sample(64)
    batch = RequestBatch.from_requests([Request(path=x, url=x or b"/") for x in p])
    verdicts = np.zeros(len(v), dtype=VERDICT_DTYPE)
    verdicts["action"], verdicts["rule_idx"] = [a for a, _ in v], [x for _, x in v]
    route = (np.array(r, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)  # (as evaluate_batch_routes returns them: -1 for none)
    resp, counts, lists = respond(batch, verdicts, np.array(s, dtype=np.uint8), route, lists=[ENDPOINTS, (O.BLOCKED,), ALL], caps=[len(v), 0, 5])
    want = O.expect_batch(v, s, r, p, [ENDPOINTS, (O.BLOCKED,), ALL], [len(v), 0, 5])
    assert resp.dtype == RESPONSE_DTYPE and [(int(k), int(a)) for k, a in zip(resp["kind"], resp["arg"])] == want[0] and not resp["pad"].any()
    assert [int(x) for x in counts] == want[1] and [([int(x) for x in e], m) for e, m in lists] == want[2]
    resp2, counts2, lists2 = respond(batch, verdicts)
    assert [(int(k), int(a)) for k, a in zip(resp2["kind"], resp2["arg"])] == O.expect_batch(v, None, None, p)[0] and lists2 == []
    with pytest.raises(PwafError):
        respond(batch, verdicts, lists=[ALL] * 5)
    assert respond_one(verdicts[0], s[0], None if r[0] is None else r[0], p[0]) == O.decide(v[0], s[0], r[0], p[0])


def test_every_refusal_before_anything_is_written():
    v, s, r, p = sample(40)
    L = lib()

    def refused(label, text, code=_abi.E_INVALID_ARG, masks=(ALL, (O.BLOCKED,)), caps=None, edit=None, **override):
        c = RC.Call(HOST, v, s, r, p, list(masks), caps)
        if edit:
            edit(c)
        assert c.run(**override) == code, label
        assert text in err(), (label, err())
        assert c.untouched(), label

    refused("NULL in", "pwaf_respond: NULL argument", batch=None)
    refused("NULL verdicts", "pwaf_respond: NULL argument", verdicts=None)
    refused("NULL out", "pwaf_respond: NULL argument", out=None)
    refused("struct_size", "pwaf_batch.struct_size mismatch", edit=lambda c: setattr(c.batch, "struct_size", C.sizeof(_abi.Batch) - 8))
    refused("memory", "pwaf_batch.memory is neither HOST nor DEVICE", edit=lambda c: setattr(c.batch, "memory", 2))
    refused("NULL path data", "pwaf_respond: pwaf_batch path column is NULL", edit=lambda c: setattr(c.batch.field[2], "data", None))
    refused("NULL path offsets", "pwaf_respond: pwaf_batch path column is NULL", edit=lambda c: setattr(c.batch.field[2], "offsets", None))
    refused("five lists", "pwaf_respond: more than PWAF_RESP_MAX_LISTS lists", n_lists=5)
    refused("NULL lists", "pwaf_respond: lists is NULL with n_lists != 0", lists=None, n_lists=1)
    refused("NULL idx with a cap", "pwaf_respond: list 1: idx is NULL with cap != 0", edit=lambda c: setattr(c.arr[1], "idx", None))
    refused("NULL n", "pwaf_respond: list 0: n is NULL", edit=lambda c: setattr(c.arr[0], "n", None))
    refused("a mask bit at PWAF_RESP_KINDS", "pwaf_respond: list 1: kinds has a bit at or above PWAF_RESP_KINDS", masks=(ALL, 1 << O.KINDS))
    refused("a mask's top bit", "pwaf_respond: list 0: kinds has a bit at or above PWAF_RESP_KINDS", masks=(0x80000001,))

    def batch_refusal(label, text, at, action=None, status=None, offsets=False):
        c = RC.Call(HOST, v, s, r, p, [ALL])
        if action is not None:
            c.keep[0][8 * at] = action
        if status is not None:
            c.statuses[at] = status
        if offsets:
            off = c.keep[2][:4 * (len(v) + 1)].view(np.uint32)
            off[at + 1] = off[at] - 1
        assert c.run() == _abi.E_BATCH and err() == f"pwaf_respond: request {at}: {text}", (label, err())
        assert c.untouched(), label

    batch_refusal("an action of 4", "an action above 3", 17, action=4)
    batch_refusal("an action of 255", "an action above 3", 39, action=255)
    batch_refusal("a status of 4", "a cookie status above 3", 0, status=4)
    batch_refusal("offsets that decrease", "path offsets decrease", 5, offsets=True)
    # the first failing request is named, whatever fails in it
    c = RC.Call(HOST, v, s, r, p, [ALL])
    c.keep[0][8 * 9], c.statuses[3] = 9, 200
    assert c.run() == _abi.E_BATCH and err() == "pwaf_respond: request 3: a cookie status above 3" and c.untouched()
    # HOST mode needs no scratch and no stream
    c = RC.Call(HOST, v, s, r, p, [ALL])
    assert c.run(scratch=None, scratch_bytes=0) == _abi.OK

    out = _abi.Response()
    ver = _abi.Verdict()
    assert L.pwaf_respond_one(None, 0, 0, 0, None, 0, C.byref(out)) == _abi.E_INVALID_ARG and err() == "pwaf_respond_one: NULL argument"
    assert L.pwaf_respond_one(C.byref(ver), 0, 0, 0, None, 0, None) == _abi.E_INVALID_ARG and err() == "pwaf_respond_one: NULL argument"
    assert L.pwaf_respond_one(C.byref(ver), 0, 0, 0, None, 3, C.byref(out)) == _abi.E_INVALID_ARG and err() == "pwaf_respond_one: NULL argument"
    assert L.pwaf_respond_one(C.byref(ver), 0, 0, 0, None, 0, C.byref(out)) == _abi.OK and (out.kind, out.arg) == (O.FORWARD, O.ROUTE_NONE)
    ver.action = 4
    assert L.pwaf_respond_one(C.byref(ver), 0, 0, 0, None, 0, C.byref(out)) == _abi.E_BATCH and err() == "pwaf_respond_one: an action above 3"
    ver.action = 0
    assert L.pwaf_respond_one(C.byref(ver), 4, 0, 0, None, 0, C.byref(out)) == _abi.E_BATCH and err() == "pwaf_respond_one: a cookie status above 3"


# ---- the listener, end to end, one request at a time ---------------------------------------------------------------------------------------
NOW = 1_800_000_000
SEED, KID = bytes([11] * 32), "walk-1"
KEYS = [(KID, CO.public_key(SEED))]
B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
WALK_RULES = [("env", 'http_request.path.starts_with("/.env")', [B]), ("bot", 'http_request.user_agent.contains("bot")', [CAP]), ("admin", 'http_request.path.starts_with("/admin")', [CAP, B])]
WALK_ROUTES = [("api", 'http_request.host.starts_with("api.")'), ("static", 'http_request.path.starts_with("/static/")')]


def cookie_of(kind, ip, ua, host):
    """the first Cookie header of a walk request: None, a valid token, one for another client, or one the batch service leaves to the host"""
    sub = CO.client_id(ipaddress.ip_address(ip).packed, ua, host)
    if kind == "none":
        return None
    if kind == "valid":
        tok = CO.mint(SEED, CO.header_json(KID), CO.claims_json(sub, NOW))
    elif kind == "invalid":
        tok = CO.mint(SEED, CO.header_json(KID), CO.claims_json("somebody else", NOW))
    else:  # signed by the set's key, with a claim the flat subset does not read
        tok = CO.mint(SEED, CO.header_json(KID), CO.claims_json(sub, NOW, extra={"nested": 1}))
    return b"theme=dark; " + CO.COOKIE.encode() + b"=" + tok


def walk_requests():
    """(request, cookie kind): the three inputs where the old prose and the reference disagree first, then one of everything else"""
    ua, bot = b"Mozilla/5.0 (walk)", b"a bot/1.0"
    rows = [("/.env", ua, "www.example.com", "invalid"),                       # an INVALID cookie on a request a Block rule matches
            ("/index.html", b"", "www.example.com", "invalid"),                # an INVALID cookie on an empty User-Agent
            ("/__pingoo/captcha/api/verify", ua, "www.example.com", "invalid"),  # an INVALID cookie on a captcha endpoint
            ("/__pingoo/captcha/api/init", ua, "api.example.com", "none"), ("/__pingoo/captcha/assets/index.js", ua, "www.example.com", "valid"),
            ("/__pingoo/captcha/other", ua, "www.example.com", "none"), ("/__pingoo/captcha", b"x" * 256, "www.example.com", "none"),
            ("/.env", ua, "www.example.com", "valid"), ("/.env", ua, "api.example.com", "none"), ("/x", bot, "www.example.com", "none"), ("/x", bot, "api.example.com", "valid"),
            ("/admin/x", ua, "www.example.com", "valid"), ("/admin/x", ua, "www.example.com", "none"), ("/x", ua, "api.example.com", "none"), ("/static/a.css", ua, "www.example.com", "valid"),
            ("/x", ua, "www.example.com", "none"), ("/x", ua, "www.example.com", "undecided"), ("/.env", ua, "www.example.com", "undecided"), ("/x", b"", "api.example.com", "undecided"),
            ("/static/b.js", ua, "www.example.com", "invalid")]
    return [(Request(host=h, path=p, url=p, user_agent=u, ip=f"198.51.100.{k + 1}", remote_port=40000 + k), c) for k, (p, u, h, c) in enumerate(rows)]


def listener_walk(requests_and_cookies):
    """the listener per request, assembled from the existing oracles: gates A and B from the derived fields themselves (:196, :200), the
    cookie from cookie_oracle (:222-236), the rule loop and the routes from the pyoracle without its gates (:251-270)"""
    out = []
    for req, kind in requests_and_cookies:
        ua, path = bytes(req.user_agent), req.path.encode() if isinstance(req.path, str) else bytes(req.path)
        host = req.host.encode() if isinstance(req.host, str) else bytes(req.host)
        if len(ua) == 0 or len(ua) >= 256:
            out.append((O.BLOCKED, O.RULE_UA_GATE))
            continue
        if path.startswith(b"/__pingoo/captcha"):
            kind_ = O.CAPTCHA_ASSET if path.startswith(O.ASSETS) else O.CAPTCHA_INIT if path == O.INIT else O.CAPTCHA_VERIFY if path == O.VERIFY else O.CAPTCHA_NOT_FOUND
            out.append((kind_, O.RULE_CAPTCHA_ENDPOINT))
            continue
        status = CO.decide(KEYS, cookie_of(kind, req.ip, ua, host), NOW, ipaddress.ip_address(req.ip).packed, ua, host)
        if status == CO.INVALID:
            out.append((O.CAPTCHA_PAGE, O.RULE_COOKIE))
            continue
        one_req = RequestBatch.from_requests([Request(host=req.host, path=req.path, url=req.url, user_agent=req.user_agent, ip=req.ip, remote_port=req.remote_port,
                                                      captcha_verified=status == CO.VERIFIED)])
        verdict = RW.oracle_verdicts(WALK_RULES, {}, None, one_req, RW.NO_GATES)[0]
        if status == CO.UNDECIDED:
            out.append((O.HOST_DECIDES, int(verdict["rule_idx"])))
            continue
        if verdict["action"] == _abi.ACTION_BLOCK:
            out.append((O.BLOCKED, int(verdict["rule_idx"])))
        elif verdict["action"] == _abi.ACTION_CAPTCHA:
            out.append((O.CAPTCHA_PAGE, int(verdict["rule_idx"])))
        else:
            k = int(RW.oracle_routes(WALK_ROUTES, {}, None, one_req)[0])
            out.append((O.NOT_FOUND, O.ROUTE_NONE) if k < 0 else (O.FORWARD, k))
    return out


def test_the_per_request_walk_equals_a_walk_of_the_listener():
    """verify_cookie -> the verdict and the route of the compiled tables (what pwaf_evaluate_one_route answers on a device) -> respond_one,
    per request, against the listener walked in Python"""
    assert CO.ABSENT == _abi.COOKIE_ABSENT and CO.INVALID == _abi.COOKIE_INVALID and CO.UNDECIDED == _abi.COOKIE_UNDECIDED and CO.VERIFIED == _abi.COOKIE_VERIFIED
    rows = walk_requests()
    want = listener_walk(rows)
    assert want[:3] == [(O.CAPTCHA_PAGE, O.RULE_COOKIE), (O.BLOCKED, O.RULE_UA_GATE), (O.CAPTCHA_VERIFY, O.RULE_CAPTCHA_ENDPOINT)]
    assert {k for k, _ in want} == set(ALL), "the walk reaches every kind"
    ks = KeySet(KEYS)
    tables = RW.RoutedTables(CompiledProgram(WALK_RULES, {}, None, routes=WALK_ROUTES))
    got, statuses, verdicts, routes = [], [], [], []
    for req, kind in rows:
        status = verify_cookie(ks, req, cookie_of(kind, req.ip, bytes(req.user_agent), req.host.encode()), NOW)
        seen = Request(host=req.host, path=req.path, url=req.url, user_agent=req.user_agent, ip=req.ip, remote_port=req.remote_port, captcha_verified=status == _abi.COOKIE_VERIFIED)
        action, rule, route = tables.evaluate_routed(RequestBatch.from_requests([seen]), 0)
        got.append(respond_one((action, rule), status, route, req.path))
        statuses.append(status), verdicts.append((int(action), int(rule))), routes.append(route)
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    # and the same inputs as one HOST batch
    RC.check("the walk as a batch", HOST, verdicts, statuses, routes, [r.path.encode() for r, _ in rows], [ALL, ENDPOINTS])
    assert RC.Call(HOST, verdicts, statuses, routes, [r.path.encode() for r, _ in rows]).run() == _abi.OK


# ---- the shared header under the sanitizers ------------------------------------------------------------------------------------------------
def test_the_shared_header_under_asan_and_ubsan_reads_no_byte_outside_a_path():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "respond_host")
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                        os.path.join(ROOT, "include"), SRC, "-o", exe], check=True)
    for with_route in (True, False):
        cases = [c for c in O.cross_product() if (c[2] is None) != with_route]
        paths = [p for _, p in PATHS]
        cases += [((O.BYPASS, O.RULE_CAPTCHA_ENDPOINT), O.INVALID, 1 if with_route else None, p) for p in paths + paths[::-1]]  # (each path edge ends the arena once)
        cases.append(((O.BYPASS, O.RULE_CAPTCHA_ENDPOINT), O.ABSENT, 1 if with_route else None, O.VERIFY))
        text = "".join(f"{v[0]} {v[1]} {O.ABSENT if s is None else s} {'-' if t is None else t} {p.hex() or '-'}\n" for v, s, t, p in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
        lines = r.stdout.split("\n")
        want = [O.decide(v, s, t, p) for v, s, t, p in cases]
        assert [tuple(int(x) for x in ln.split()[1:]) for ln in lines[:len(cases)]] == want
        counts = [sum(1 for k, _ in want if k == kind) for kind in ALL]
        assert lines[len(cases)] == "H " + " ".join(str(x) for x in [len(cases)] + counts)
