"""pwaf_respond on the device (respond_classify_kernel, respond_base_kernel, respond_scatter_kernel): responses, counts and every list equal
the HOST mode's and the independent oracle's (tests/respond_oracle.py), with guard regions behind the responses, the counts, each idx and
each n — for batches at every edge of the scan's shape, lists whose members sit in one lane only, in every lane and in none, BYPASS paths at
every start alignment and at the arena's end, every cap edge, overlapping masks, the chain verify_cookies -> evaluate_device(route=) ->
respond -> {parse_pow_bodies -> verify_pow, client_ids, export_records} on one stream without a synchronisation, two streams, and the
refusals. Small batches. docs/respond_edges.md says what each test pins."""
import ctypes as C
import functools

import numpy as np
import pytest

import respond_cases as RC
import respond_oracle as O
from pingoo_amd import Request, RequestBatch, _abi, client_ids, generate_captcha_client_id, parse_pow_bodies, parse_pow_body_one, respond, respond_one, verify_cookie, verify_cookies, verify_pow, verify_pow_one
from pingoo_amd.engine import DeviceBatch, RuleEngine, export_records, export_stats, lib, respond_scan_shape

pytestmark = pytest.mark.gpu
HOST = RC.HostMem()
ALL = tuple(range(O.KINDS))
ENDPOINTS = (O.CAPTCHA_ASSET, O.CAPTCHA_INIT, O.CAPTCHA_VERIFY, O.CAPTCHA_NOT_FOUND)
GATE_B = (O.BYPASS, O.RULE_CAPTCHA_ENDPOINT)


@functools.lru_cache(maxsize=None)
def device():
    return RC.DeviceMem()


def sync():
    import torch

    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def shape():
    return respond_scan_shape()


def both(label, verdicts, statuses, routes, paths, lists=(), caps=None, **kw):
    """DEVICE mode, HOST mode and the oracle agree on everything the call writes, and neither mode writes into a guard region"""
    got = RC.check(f"{label}, DEVICE", device(), verdicts, statuses, routes, paths, lists, caps, sync=sync, **kw)
    assert got == RC.check(f"{label}, HOST", HOST, verdicts, statuses, routes, paths, lists, caps, **kw)
    return got


# ---- whole batches at the edges of the scan's shape ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ["0", "1", "63", "64", "65", "tile - 1", "tile", "tile + 1", "tile * step + 1"])
def test_every_request_of_a_batch(n):
    count = eval(n, {}, shape())  # noqa: S307 (the names of the scan's shape)
    v, s, r, p = O.mixed_batch(count, seed=count % 97)
    got = both(f"n = {n}", v, s, r, p, [ENDPOINTS, (O.BLOCKED, O.CAPTCHA_PAGE), ALL, (O.HOST_DECIDES,)], lead=count % 16)
    assert got[2][2][1] == count == sum(got[1])
    if count > 10000:
        assert all(c > 0 for c in got[1]), "every kind occurs"


def test_no_status_and_no_route_column_and_no_counts():
    v, s, r, p = O.mixed_batch(300, seed=5)
    both("no status", v, None, r, p, [ALL, ENDPOINTS])
    both("no route", v, s, None, p, [(O.FORWARD,), (O.NOT_FOUND,)])
    both("neither, no counts, no list", v, None, None, p, with_counts=False)
    both("neither, counts alone", v, None, None, p)
    both("lists alone", v, s, r, p, [(O.BLOCKED,)], with_counts=False)


# ---- where a list's members sit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["the last lane of a wave", "the first lane of a tile", "every lane", "no lane", "the last lane of the batch"])
def test_members_that_sit_only_in(where):
    tile = shape()["tile"]
    n = 2 * tile + 70
    member = {"the last lane of a wave": lambda i: i % 64 == 63, "the first lane of a tile": lambda i: i % tile == 0, "every lane": lambda i: True, "no lane": lambda i: False,
              "the last lane of the batch": lambda i: i == n - 1}[where]
    v = [(O.BLOCK, 9) if member(i) else (O.ALLOW, O.RULE_NONE) for i in range(n)]
    count = sum(1 for i in range(n) if member(i))
    got = both(where, v, None, [4] * n, [b"/x"] * n, [(O.BLOCKED,), (O.FORWARD,), (O.BLOCKED, O.FORWARD), (O.NOT_FOUND,)])
    assert [m for _, m in got[2]] == [count, n - count, n, 0]
    assert got[2][0][0] == [i for i in range(n) if member(i)]


# ---- the paths of BYPASS requests --------------------------------------------------------------------------------------------------------
def test_bypass_paths_at_every_start_alignment():
    paths, total = [], 0
    for k in range(32):  # a filler, then a literal that begins at alignment k % 16: each alignment under two literals
        lit = (O.VERIFY, O.INIT, O.ASSETS + b"/app.js", O.VERIFY[:-1], O.INIT + b"/", O.ASSETS)[k % 6]
        filler = b"/" * ((k - total) % 16)
        paths += [filler, lit]
        total += len(filler) + len(lit)
    starts = np.cumsum([0] + [len(x) for x in paths])[:-1]
    assert {int(a) % 16 for a, x in zip(starts, paths) if len(x) >= 24} == set(range(16)), "every alignment of a path that is read"
    v = [GATE_B] * len(paths)
    got = both("alignments", v, None, None, paths, [ENDPOINTS])
    assert {k for k, _ in got[0]} == set(ENDPOINTS)
    cases = [x for _, x in O.path_cases()]
    for lead in range(16):
        both(f"every path case, the arena shifted by {lead}", [GATE_B] * len(cases), [O.INVALID] * len(cases), None, cases, [(O.CAPTCHA_VERIFY,), (O.CAPTCHA_INIT, O.CAPTCHA_ASSET)], lead=lead)


def test_bypass_paths_at_the_arena_s_end_with_exactly_the_pad_behind():
    """the arena is the paths and PWAF_ARENA_PAD zero bytes; the block's guard bytes behind it are 0x5A: a comparison that looked at a byte
    behind a path's end would see a difference between the two"""
    for label, last in O.path_cases():
        paths = [O.INIT, b"/a", last]
        both(f"the arena ends with {label}", [GATE_B] * 3, None, [1, 2, 3], paths, [ENDPOINTS], pad=O.ARENA_PAD)
    both("the arena is one empty path", [GATE_B], None, None, [b""], [ENDPOINTS])
    both("the arena is verify", [GATE_B], None, None, [O.VERIFY], [(O.CAPTCHA_VERIFY,)])


# ---- caps and masks ----------------------------------------------------------------------------------------------------------------------
def test_every_cap_edge_inside_a_wave_and_on_a_tile_edge():
    tile = shape()["tile"]
    n = 2 * tile + 70
    v = [(O.BLOCK, i) for i in range(n)]  # every request a member: entry k is request k, so a cap of `tile` cuts on the tile's edge
    for caps in ([tile, tile + 5, n - 1, n + 1], [0, 64, 63, 1], [n, tile - 1, 2 * tile, 2 * tile + 1]):
        got = both(f"caps {caps}", v, None, None, [b"/x"] * n, [(O.BLOCKED,)] * 4, caps=caps)
        assert [len(e) for e, _ in got[2]] == [min(c, n) for c in caps]
    v, s, r, p = O.mixed_batch(n, seed=11)
    counts = O.expect_batch(v, s, r, p)[1]
    for kinds in ((O.BLOCKED,), ENDPOINTS, (O.HOST_DECIDES, O.NOT_FOUND)):
        c = sum(counts[k] for k in kinds)
        assert c > 65
        both(f"sparse members, kinds {kinds}", v, s, r, p, [kinds] * 4, caps=[0, c - 1, c, c + 1])
        both(f"sparse members, kinds {kinds}, a cut inside the first wave and one behind it", v, s, r, p, [kinds] * 2, caps=[3, 65])


def test_overlapping_masks_mask_zero_and_count_only_lists():
    v, s, r, p = O.mixed_batch(700, seed=2)
    both("overlaps", v, s, r, p, [(O.CAPTCHA_INIT, O.CAPTCHA_VERIFY), (O.CAPTCHA_VERIFY,), ALL, (O.CAPTCHA_VERIFY, O.BLOCKED)])
    both("mask 0 among others", v, s, r, p, [(), ALL, (), (O.FORWARD,)])
    both("count only", v, s, r, p, [ALL, ENDPOINTS, (O.BLOCKED,), ()], caps=[0, 0, 0, 0])
    both("count only beside a list with room", v, s, r, p, [ALL, (O.BLOCKED,)], caps=[0, 700])
    for k in ALL:
        both(f"kind {k} alone", v, s, r, p, [(k,)])


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
RULES = [("shop", 'http_request.path.starts_with("/shop")', [_abi.RULE_ACTION_BLOCK]), ("bot", 'http_request.user_agent.contains("bot")', [_abi.RULE_ACTION_CAPTCHA])]
ROUTES = [("api", 'http_request.host.starts_with("h")'), ("about", 'http_request.path == "/about"')]


def test_the_chain_on_one_stream_without_a_synchronisation():
    """verify_cookies -> evaluate_device(route=) -> respond -> parse_pow_bodies -> verify_pow on the VERIFY list, client_ids on the INIT | VERIFY
    list, export_records on the BLOCKED list: one stream, no synchronisation; against the same steps per request on the host"""
    import torch

    import cookie_oracle as CO
    import powbody_oracle as BO
    from test_gpu_verify_pow import clients, host_keyset, keyset, upload
    from test_verify_pow_cpu import KIDS, NOW, SEEDS, VERIFIED_NAME, flip, packed

    people = clients()
    reqs, cookies, bodies = [], [], []
    for k in range(300):
        c = people[(7 * k) % len(people)]
        path, ua, body = ((O.VERIFY, c.ua, BO.genuine(c.nonce, c.digest)), (O.INIT, c.ua, b""), (b"/shop/%d" % k, c.ua, b""), (b"/about", c.ua, b""),
                          (O.VERIFY, c.ua, BO.genuine(c.nonce, flip(c.digest, 9 + k % 200))), (b"/about", b"" if k % 12 == 5 else c.ua + b" bot", b""), (b"/nowhere", c.ua, b""))[k % 7]
        seen_ua = ua
        verified = b""
        if k % 4 < 2:  # a verified cookie: the client's own, or one bound to another client (INVALID)
            sub = CO.client_id(packed(c.ip), seen_ua if k % 4 == 0 else seen_ua + b"?", c.host)
            verified = b"; " + VERIFIED_NAME + b"=" + CO.mint(SEEDS[k % 3], CO.header_json(KIDS[k % 3]), CO.claims_json(sub, NOW))
        reqs.append(Request(host=c.host, url=path, path=path, method=b"POST" if body else b"GET", user_agent=ua, ip=c.ip, remote_port=2000 + k))
        cookies.append(c.cookie + verified), bodies.append(body)
    batch = RequestBatch.from_requests(reqs)
    lists = [(O.CAPTCHA_VERIFY,), (O.CAPTCHA_INIT, O.CAPTCHA_VERIFY), (O.BLOCKED,)]
    eng = RuleEngine(RULES, {}, None, routes=ROUTES)
    try:
        # the host, request by request
        hks = host_keyset()
        h_status = [verify_cookie(hks, q, ck, NOW) for q, ck in zip(reqs, cookies)]
        flagged = RequestBatch.from_requests([Request(host=q.host, url=q.url, path=q.path, method=q.method, user_agent=q.user_agent, ip=q.ip, remote_port=q.remote_port,
                                                      captcha_verified=st == _abi.COOKIE_VERIFIED) for q, st in zip(reqs, h_status)])
        h_verdicts, h_routes = eng.evaluate_batch_routes(flagged)
        want = [respond_one(h_verdicts[i], h_status[i], int(h_routes[i]), reqs[i].path) for i in range(batch.n)]
        assert {k for k, _ in want} >= {O.FORWARD, O.NOT_FOUND, O.BLOCKED, O.CAPTCHA_PAGE, O.CAPTCHA_INIT, O.CAPTCHA_VERIFY} and {_abi.COOKIE_VERIFIED, _abi.COOKIE_INVALID, _abi.COOKIE_ABSENT} == set(h_status)
        assert (O.CAPTCHA_PAGE, O.RULE_COOKIE) in want and (O.BLOCKED, O.RULE_UA_GATE) in want and (O.BLOCKED, 0) in want and (O.CAPTCHA_PAGE, 1) in want
        want_lists = [[i for i, (k, _) in enumerate(want) if k in kinds] for kinds in lists]
        assert all(len(x) >= 20 for x in want_lists)
        # the device, one stream
        db = DeviceBatch(batch)
        col, d_bodies = upload(cookies, db.device), upload(bodies, db.device)
        d_route = torch.zeros(batch.n, dtype=torch.int32, device=db.device)
        ks = keyset()
        s = torch.cuda.current_stream(db.device)  # the stream torch allocates on: outputs and scratch of every call are ordered with them
        d_status = verify_cookies(ks, db, col, NOW, flags_out=db.flags, stream=s.cuda_stream)
        verdicts = eng.evaluate_device(db, route=d_route, stream=s.cuda_stream)
        resp, counts, (l_verify, l_ids, l_blocked) = respond(db, verdicts, d_status, d_route, lists=lists, stream=s.cuda_stream)
        b_status, hashes, nonce_col, _ = parse_pow_bodies(d_bodies, idx=l_verify[0], n_idx=l_verify[1], stream=s.cuda_stream)
        p_status = verify_pow(ks, db, col, hashes, nonce_col, NOW, idx=l_verify[0], n_idx=l_verify[1], stream=s.cuda_stream)
        ids = client_ids(db, idx=l_ids[0], n_idx=l_ids[1], stream=s.cuda_stream)
        buf, rec_off, stats = export_records(db, l_blocked[0], l_blocked[1], stream=s.cuda_stream)
        s.synchronize()
        eng.device_status()
        got = [(int(k) & 0xFF, int(a) & 0xFFFFFFFF) for k, a in resp.cpu().numpy()]
        assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]
        assert [int(x) for x in counts.cpu().numpy()] == [sum(1 for k, _ in want if k == kind) for kind in ALL]
        for (idx, cnt), members in zip((l_verify, l_ids, l_blocked), want_lists):
            assert int(cnt.item()) == len(members) and [int(x) for x in idx.cpu().numpy()[:len(members)]] == members
        # what the consumers made of the lists
        got_body, got_pow = b_status.cpu().numpy(), p_status.cpu().numpy()
        n_passed = 0
        for j, i in enumerate(want_lists[0]):
            st, h, nonce = parse_pow_body_one(bodies[i])
            assert int(got_body[j]) == st == _abi.BODY_OK
            assert int(got_pow[j]) == verify_pow_one(hks, reqs[i], cookies[i], h, nonce, NOW), i
            n_passed += int(got_pow[j]) == _abi.POW_PASSED
        assert 0 < n_passed < len(want_lists[0])
        rows = ids.cpu().numpy()
        for j, i in enumerate(want_lists[1]):
            assert rows[j].tobytes().split(b"\0", 1)[0].decode() == generate_captcha_client_id(reqs[i].ip, reqs[i].user_agent, reqs[i].host), i
        # (the device batch carries the flags verify_cookies wrote: the host batch that does is `flagged`)
        h_buf, h_off, h_stats = export_records(flagged, np.array(want_lists[2], dtype=np.uint32), header_names=[])
        st = export_stats(stats)
        assert (st["n_selected"], st["n_written"], st["bytes_needed"]) == (len(want_lists[2]), len(want_lists[2]), h_stats["bytes_needed"])
        d_buf, d_off = buf.cpu().numpy(), rec_off.cpu().numpy().view(np.uint32)
        for j in range(len(want_lists[2])):
            size = int(h_buf[h_off[j]:h_off[j] + 4].view(np.uint32)[0])
            assert d_buf[d_off[j]:d_off[j] + size].tobytes() == h_buf[h_off[j]:h_off[j] + size].tobytes(), j
    finally:
        eng.close()


def test_two_calls_on_two_streams():
    import torch

    a, b = O.mixed_batch(700, seed=21), O.mixed_batch(900, seed=22)
    eng = RuleEngine(RULES, {}, None)  # (for its stream: a second HIP stream beside torch's current one)
    try:
        streams = [C.c_void_p(lib().pwaf_engine_stream(eng._h)).value, torch.cuda.current_stream().cuda_stream]
        assert streams[0] and streams[0] != streams[1]
        calls = [RC.Call(device(), v, s, r, p, [ENDPOINTS, ALL, (O.BLOCKED,)], caps=[len(v), 100, 7]) for v, s, r, p in (a, b)]
        torch.cuda.synchronize()  # (the uploads ran on torch's current stream)
        for c, st in zip(calls, streams):
            assert c.run(stream=st) == _abi.OK
        torch.cuda.synchronize()
        for c, (v, s, r, p) in zip(calls, (a, b)):
            got, want = c.results("two streams"), O.expect_batch(v, s, r, p, [ENDPOINTS, ALL, (O.BLOCKED,)], c.caps)
            assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
    finally:
        eng.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_the_device_refusals_write_nothing():
    v, s, r, p = O.mixed_batch(40, seed=4)
    err = lambda: lib().pwaf_last_error().decode()  # noqa: E731

    def refused(label, text, edit=None, masks=(ALL, (O.BLOCKED,)), **override):
        c = RC.Call(device(), v, s, r, p, list(masks))
        if edit:
            edit(c)
        assert c.run(**override) == _abi.E_INVALID_ARG, label
        assert text in err(), (label, err())
        sync()
        assert c.untouched(), label
        return c

    scratch_text = "pwaf_respond: scratch is NULL, not 16-byte aligned or smaller than pwaf_respond_scratch_bytes(n)"
    refused("NULL scratch", scratch_text, scratch=None)
    c = RC.Call(device(), v, s, r, p, [ALL])
    refused("a short scratch", scratch_text, scratch_bytes=c.scratch_bytes - 1)
    refused("a misaligned scratch", scratch_text, scratch=c.mem.ptr(c.scratch) + 8)
    refused("NULL verdicts", "pwaf_respond: NULL argument", verdicts=None)
    refused("NULL out", "pwaf_respond: NULL argument", out=None)
    refused("NULL path column", "pwaf_respond: pwaf_batch path column is NULL", edit=lambda c: setattr(c.batch.field[2], "data", None))
    refused("five lists", "pwaf_respond: more than PWAF_RESP_MAX_LISTS lists", n_lists=5)
    refused("NULL lists", "pwaf_respond: lists is NULL with n_lists != 0", lists=None, n_lists=2)
    refused("NULL idx with a cap", "pwaf_respond: list 0: idx is NULL with cap != 0", edit=lambda c: setattr(c.arr[0], "idx", None))
    refused("NULL n", "pwaf_respond: list 1: n is NULL", edit=lambda c: setattr(c.arr[1], "n", None))
    refused("a mask bit at PWAF_RESP_KINDS", "pwaf_respond: list 0: kinds has a bit at or above PWAF_RESP_KINDS", masks=(1 << O.KINDS,))
    assert c.run() == _abi.OK
    sync()
    assert c.results()[2][0][1] == len(v)
