"""pwaf_parse_pow_bodies on the device (powbody_parse_kernel, powbody_base_kernel, powbody_copy_kernel): statuses, hash rows, nonce offsets,
nonce bytes and stats equal the HOST mode's and the independent oracle's (tests/powbody_oracle.py), with guard regions behind everything
the call may write — for batches at every edge of the scan's shape, body lengths around the 16-byte load, every start alignment and
every phase of the hash text against a load edge, bodies and nonces at the arena's end, nonces that make a copy chunk cross requests and
a tile edge, every cap, lists (duplicates, entries that name no request, a device-side length), the mutated corpus, the chain
evaluate_device -> parse_pow_bodies -> verify_pow on one stream without a synchronisation, two streams, and the refusals. Small batches."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import powbody_oracle as O
from pingoo_amd import Request, RequestBatch, _abi, body_stats, parse_pow_bodies, verify_pow
from pingoo_amd.engine import DeviceBatch, RuleEngine, lib, parse_pow_scan_shape
from test_parse_pow_cpu import check_outputs, raw_call

pytestmark = pytest.mark.gpu
K, M, U = O.OK, O.MALFORMED, O.UNDECIDED
CANARY = 64
DEVICE = "cuda:0"


def device_call(bodies, lead=0, idx=None, n_idx=None, cap=None, stream=None, sync=True):
    """pwaf_parse_pow_bodies in DEVICE mode over a column with exactly PWAF_ARENA_PAD bytes behind its last body, whose offsets begin at
    `lead`, into outputs pre-filled with 0x5A that have guard regions behind them -> what test_parse_pow_cpu.raw_call returns (numpy),
    or with sync=False the tensors to read later"""
    import torch

    data, off = O.column(bodies, lead)
    assert len(data) == off[-1] + _abi.ARENA_PAD
    n = len(bodies)
    d_data, d_off = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(DEVICE), torch.tensor(off, dtype=torch.int64).to(torch.int32).to(DEVICE)
    m = n if idx is None else len(idx)
    looked = m if n_idx is None else min(n_idx, m)
    if cap is None:
        cap = sum(len(x) for x in O.expect_batch(bodies, idx, n_idx)[2]) + _abi.ARENA_PAD
    fill = lambda count, dtype, value: torch.full((count,), value, dtype=dtype, device=DEVICE)  # noqa: E731
    status, hashes = fill(looked + CANARY, torch.uint8, 0x5A), fill((n + 1) * 32, torch.uint8, 0x5A)
    ndata, noff, stats = fill((cap + 15) // 16 * 16 + CANARY, torch.uint8, 0x5A), fill(n + 1 + CANARY, torch.int32, 0x5A5A5A5A), fill(5, torch.int64, 0x5A5A5A5A5A5A5A5A)
    need = int(lib().pwaf_parse_pow_bodies_scratch_bytes(n))
    scratch = fill(need, torch.uint8, 0xEE)
    d_idx = None if idx is None else torch.tensor([int(np.uint32(i).astype(np.int32)) for i in idx] or [0], dtype=torch.int32, device=DEVICE)
    d_n = None if n_idx is None else torch.tensor([n_idx], dtype=torch.int32, device=DEVICE)
    col, ncol = _abi.StrCol(), _abi.DerivedCol()
    col.data, col.offsets = d_data.data_ptr(), d_off.data_ptr()
    ncol.data, ncol.offsets, ncol.cap = ndata.data_ptr(), noff.data_ptr(), cap
    assert ndata.data_ptr() % 16 == 0
    if stream is not None:
        torch.cuda.current_stream().synchronize()  # the fills above ran on torch's current stream: they are done before another stream is given the call
    rc = lib().pwaf_parse_pow_bodies(C.byref(col), n, _abi.MEM_DEVICE, None if idx is None else d_idx.data_ptr(), 0 if idx is None else m, None if d_n is None else d_n.data_ptr(),
                                     status.data_ptr(), hashes.data_ptr(), C.byref(ncol), stats.data_ptr(), scratch.data_ptr(), need,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream))
    assert rc == 0, lib().pwaf_last_error()
    tensors = (status, hashes, ndata, noff, stats, (d_data, d_off, d_idx, d_n, scratch))

    def read():
        st = stats.cpu().numpy().view(np.uint64)
        assert st[4] == 0x5A5A5A5A5A5A5A5A, "written beyond stats + 1"
        return 0, status.cpu().numpy(), hashes.cpu().numpy().reshape(n + 1, 32), ndata.cpu().numpy(), noff.cpu().numpy().view(np.uint32), body_stats(st[:4].tobytes())

    if not sync:
        return tensors, read
    torch.cuda.synchronize()
    return read()


def assert_all_agree(label, bodies, lead=0, idx=None, n_idx=None, cap=None):
    """DEVICE mode, HOST mode and the oracle agree on everything the call writes, and neither mode writes into a guard region"""
    check_outputs(f"{label}, DEVICE", bodies, device_call(bodies, lead, idx, n_idx, cap), idx, n_idx, cap, canary=CANARY)
    check_outputs(f"{label}, HOST", bodies, raw_call(bodies, lead, idx, n_idx, cap), idx, n_idx, cap)


@functools.lru_cache(maxsize=None)
def shape():
    return parse_pow_scan_shape()


@functools.lru_cache(maxsize=None)
def mixed(count):
    """`count` bodies: the fixed corpus' shorter bodies and genuine ones with nonces of many lengths, shuffled; all statuses early"""
    pool = [b for _, b, _ in O.fixed_corpus() if len(b) <= 200] + [O.genuine(b"%d" % (7 ** k), O.digest_of(k), order="hn" if k % 3 == 0 else "nh") for k in range(150)]
    random.Random(count).shuffle(pool)
    bodies = [pool[k % len(pool)] for k in range(count)]
    assert count < 40 or {O.decide(b)[0] for b in bodies[:40]} == {K, M, U}
    return bodies


# ---- whole batches at the edges of the scan's shape ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ["0", "1", "63", "64", "65", "tile - 1", "tile", "tile + 1", "tile * step + 1"])
def test_every_request_of_a_batch(n):
    count = eval(n, {}, shape())  # noqa: S307 (the names of the scan's shape)
    assert_all_agree(f"n = {n}", mixed(count), lead=count % 16)


def test_body_lengths_around_the_16_byte_load_and_the_limit():
    g = O.genuine()
    bodies = []
    for length in (0, 1, 15, 16, 17, 31, 32, 33, O.MAX_BYTES, O.MAX_BYTES + 1, O.MAX_BYTES - 1, 2 * O.MAX_BYTES):
        bodies.append(b" " * length)
        if length:
            bodies.append(b"{" + b"\n" * (length - 1))
        if length >= 10:
            bodies.append(b'{"nonce":"' + b"1" * (length - 10))
        if length >= len(g):
            bodies += [b" " * (length - len(g)) + g, g + b" " * (length - len(g)), O.genuine(nonce=b"5" * (length - len(g) + 4))]
    assert {O.decide(b)[0] for b in bodies} == {K, M, U} and {len(b) for b in bodies} >= {0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097}
    for tail in (0, 1, 15, O.MAX_BYTES):  # the arena ends with a body of this length
        ordered = [b for b in bodies if len(b) != tail] + [b for b in bodies if len(b) == tail]
        assert_all_agree(f"body lengths, the arena ends with one of {tail}", ordered, lead=3)


def test_every_start_alignment_and_every_phase_of_the_hash_text_against_a_load_edge():
    bodies = [O.genuine(b"3" * k, O.digest_of(k), order="nh" if k < 32 else "hn", case=("lower", "upper", "mixed")[k % 3]) for k in range(64)]
    starts = np.cumsum([5] + [len(b) for b in bodies])[:-1]
    assert {int(s) % 16 for s in starts} == set(range(16)), "every alignment of a body's first byte"
    assert {b.index(b'"hash":"') + 8 & 15 for b in bodies} == set(range(16)), "every phase of the hash text"
    assert all(O.decide(b)[0] == K for b in bodies)
    assert_all_agree("alignments and phases", bodies, lead=5)
    for lead in range(16):
        assert_all_agree(f"one genuine body at alignment {lead}", [O.genuine()], lead=lead)


def test_a_body_and_a_nonce_that_end_at_the_arena_s_last_byte():
    g = O.genuine(b"12345678901234567890")
    for label, last in (("a genuine body", g), ("a nonce without its closing quote", b'{"nonce":"1234567'), ("a hash without its closing quote", g[:-2]), ("an escape", g[:-3] + b"\\"),
                        ("an empty body", b""), ("one byte", b"{")):
        assert_all_agree(f"the arena ends with {label}", [g, b"", last])  # (device_call asserts the PWAF_ARENA_PAD bytes behind)
        assert_all_agree(f"the arena is {label}", [last])


def test_nonces_whose_copy_chunks_cross_requests_and_a_tile_edge():
    tile = shape()["tile"]
    lengths = [0, 1, 16, 300, 1, 1, 1, 0, 0, 16, 15, 17, 300, 300, 2]
    bodies = [O.genuine(bytes(0x30 + (k + j) % 10 for j in range(lengths[k % len(lengths)])), O.digest_of(k)) for k in range(tile + 70)]
    bodies[tile - 1], bodies[tile] = O.genuine(b"8" * 300, O.digest_of(1)), O.genuine(b"9" * 300, O.digest_of(2))  # the tile edge inside a chunk's reach
    bodies[7] = b'{"nonce":"not counted\\"}'
    assert_all_agree("nonce lengths 0, 1, 16, 300", bodies)
    assert_all_agree("only empty nonces", [O.genuine(b"", O.digest_of(k)) for k in range(70)])
    assert_all_agree("one byte each", [O.genuine(b"%d" % (k % 10), O.digest_of(k)) for k in range(tile + 3)])


@pytest.mark.parametrize("short", [0, 1, 16, 17, "all"])
def test_every_cap(short):
    bodies = mixed(300)
    total = O.expect_batch(bodies)[3]["nonce_bytes"]
    cap = 0 if short == "all" else total + _abi.ARENA_PAD - short
    assert_all_agree(f"cap short by {short}", bodies, cap=cap)


# ---- lists -------------------------------------------------------------------------------------------------------------------------------
def test_a_list_with_duplicates_and_entries_that_name_no_request():
    bodies = mixed(300)
    n = len(bodies)
    idx = [3, 3, n, 0, 2**32 - 1, n - 1, 3, n + 5, 0, 299, 256, 255]
    assert_all_agree("the list", bodies, idx=idx)
    rng = random.Random(5)
    long = [rng.randrange(n + 20) for _ in range(5 * n)]  # more entries than requests: the parse launch strides
    assert_all_agree("a list longer than the batch", bodies, idx=long, lead=9)
    assert_all_agree("a list over no request", [], idx=[0, 1, 2])
    assert_all_agree("a list of 20 000 entries over 3 requests", bodies[:3], idx=[k % 4 for k in range(20000)])


@pytest.mark.parametrize("n_idx", [0, 1, 100, 299, 300, 100000])
def test_a_device_side_n_idx_below_and_above_idx_cap(n_idx):
    bodies = mixed(300)
    idx = [(7 * k) % 310 for k in range(300)]
    assert_all_agree(f"n_idx {n_idx}", bodies, idx=idx, n_idx=n_idx)


def test_the_first_4096_bodies_of_the_mutated_corpus():
    bodies = list(O.mutated_corpus()[:4096])
    assert_all_agree("the mutated corpus", bodies, lead=11)
    assert_all_agree("the mutated corpus through a list", bodies, idx=list(range(4095, -1, -3)))


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
RULES = [("shop", 'http_request.path.starts_with("/shop")', [_abi.RULE_ACTION_BLOCK])]
VERIFY_PATH = b"/__pingoo/captcha/api/verify"


def test_evaluate_parse_verify_on_one_stream_without_a_synchronisation():
    import torch

    import pow_oracle as PO
    from test_gpu_verify_pow import clients, host_keyset, keyset, upload
    from test_verify_pow_cpu import NOW, flip

    people = clients()
    rng = random.Random(77)
    reqs, cookies, bodies, kinds = [], [], [], []
    for k in range(300):
        c = people[rng.randrange(len(people))]
        kind = ("passing", "wrong hash", "malformed", "escaped nonce", "swapped members")[k % 5]
        body = {"passing": O.genuine(c.nonce, c.digest), "wrong hash": O.genuine(c.nonce, flip(c.digest, 8 + k % 200)), "malformed": O.genuine(c.nonce, c.digest)[:-(1 + k % 60)],
                "escaped nonce": O.genuine(b"\\u003" + c.nonce[:1] + c.nonce[1:], c.digest), "swapped members": O.genuine(c.nonce, c.digest, order="hn", case="upper")}[kind]
        path = VERIFY_PATH if k % 3 else b"/about"
        reqs.append(Request(host=c.host, url=path, path=path, method=b"POST", user_agent=c.ua, ip=c.ip, remote_port=1000 + k))
        cookies.append(c.cookie), bodies.append(body), kinds.append(kind)
    batch = RequestBatch.from_requests(reqs)
    parsed = [O.decide(b) for b in bodies]
    assert [p[0] for p in parsed[:5]] == [K, K, M, U, K]
    # what the host made until now: its own parse, uploaded as two columns
    host_status = verify_pow(host_keyset(), batch, cookies, [p[1] for p in parsed], [p[2] for p in parsed], NOW)
    eng = RuleEngine(RULES, {}, None)
    try:
        db = DeviceBatch(batch)
        col = upload(cookies, db.device)
        d_bodies = upload(bodies, db.device)
        d_idx, d_nm = torch.zeros(batch.n, dtype=torch.int32, device=db.device), torch.zeros(1, dtype=torch.int32, device=db.device)
        ks = keyset()
        s = torch.cuda.current_stream(db.device)  # the stream torch allocates on: outputs and scratch of the three calls are ordered with them
        verdicts = eng.evaluate_device(db, match_idx=d_idx, n_matches=d_nm, stream=s.cuda_stream)
        b_status, hashes, nonce_col, stats = eng.parse_pow_bodies(d_bodies, idx=d_idx, n_idx=d_nm, stream=s.cuda_stream)  # no synchronisation in between
        p_status = eng.verify_pow(ks, db, col, hashes, nonce_col, NOW, idx=d_idx, n_idx=d_nm, stream=s.cuda_stream)
        s.synchronize()
        eng.device_status()
        k = int(d_nm.item())
        match_idx = [int(i) for i in d_idx.cpu().numpy()[:k]]
        assert k == 200 and sorted(match_idx) == [i for i in range(300) if i % 3], "requests on the verify endpoint are in match_idx"
        assert ((verdicts.cpu().numpy()[match_idx, 0] & 0xFF) == _abi.ACTION_BYPASS).all()
        got_body, got_pow = b_status.cpu().numpy()[:k], p_status.cpu().numpy()[:k]
        assert [int(x) for x in got_body] == [parsed[i][0] for i in match_idx], "a listed request's body status differs from the oracle's"
        decided = [j for j, i in enumerate(match_idx) if parsed[i][0] == K]
        assert len(decided) >= 100
        assert [int(got_pow[j]) for j in decided] == [int(host_status[match_idx[j]]) for j in decided], "verify_pow behind the device parse differs from verify_pow behind the host's"
        seen = {(kinds[match_idx[j]], int(got_pow[j])) for j in decided}
        assert seen == {("passing", PO.PASSED), ("wrong hash", PO.FAILED), ("swapped members", PO.PASSED)}, seen
        st = body_stats(stats)
        assert (st["n"], st["n_ok"], st["overflow"]) == (200, len(decided), 0) and st["nonce_bytes"] == sum(len(parsed[i][2]) for i in match_idx)
        rows, noff = hashes.cpu().numpy(), nonce_col[1].cpu().numpy()
        ndata = nonce_col[0].cpu().numpy()
        for i in match_idx:
            assert bytes(rows[i]) == parsed[i][1] and bytes(ndata[noff[i]:noff[i + 1]]) == parsed[i][2]
        assert all(noff[i] == noff[i + 1] for i in range(300) if i % 3 == 0), "an unlisted request has no nonce"
    finally:
        eng.close()


def test_two_calls_on_two_streams():
    import torch

    halves = [mixed(300)[:200], mixed(300)[100:]]
    eng = RuleEngine(RULES, {}, None)  # (for its stream: a second HIP stream beside torch's current one)
    try:
        streams = [C.c_void_p(lib().pwaf_engine_stream(eng._h)).value, torch.cuda.current_stream().cuda_stream]
        assert streams[0] and streams[0] != streams[1]
        runs = [device_call(bodies, lead=2, stream=s, sync=False) for bodies, s in zip(halves, streams)]
        torch.cuda.synchronize()
        for (keep, read), bodies in zip(runs, halves):
            check_outputs("two streams", bodies, read(), canary=CANARY)
    finally:
        eng.close()


def test_a_short_scratch_is_refused():
    import torch

    bodies = mixed(8)
    d, o = O.column(bodies)
    d_data, d_off = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).to(DEVICE), torch.tensor(o, dtype=torch.int32, device=DEVICE)
    status, hashes = torch.full((8,), 0x5A, dtype=torch.uint8, device=DEVICE), torch.full((8 * 32,), 0x5A, dtype=torch.uint8, device=DEVICE)
    ndata, noff, stats = torch.full((256,), 0x5A, dtype=torch.uint8, device=DEVICE), torch.full((9,), 0x5A5A5A5A, dtype=torch.int32, device=DEVICE), torch.zeros(4, dtype=torch.int64, device=DEVICE)
    need = int(lib().pwaf_parse_pow_bodies_scratch_bytes(8))
    scratch = torch.empty(need + 16, dtype=torch.uint8, device=DEVICE)
    col, ncol = _abi.StrCol(), _abi.DerivedCol()
    col.data, col.offsets = d_data.data_ptr(), d_off.data_ptr()
    ncol.data, ncol.offsets, ncol.cap = ndata.data_ptr(), noff.data_ptr(), 256
    call = lambda ptr, size: lib().pwaf_parse_pow_bodies(C.byref(col), 8, _abi.MEM_DEVICE, None, 0, None, status.data_ptr(), hashes.data_ptr(), C.byref(ncol), stats.data_ptr(), ptr, size, None)  # noqa: E731
    assert call(None, need) == _abi.E_INVALID_ARG
    assert call(scratch.data_ptr(), need - 1) == _abi.E_INVALID_ARG
    assert call(scratch.data_ptr() + 8, need) == _abi.E_INVALID_ARG
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0x5A).all() and (noff.cpu().numpy().view(np.uint32) == 0x5A5A5A5A).all()


def test_a_plain_evaluation_launches_none_of_the_new_kernels():
    batch = RequestBatch.from_requests([Request(host=b"shop.example.com", url=b"/shop/%d" % k, path=b"/shop/%d" % k, method=b"GET", user_agent=b"ua", ip="10.0.0.%d" % (k % 200 + 1)) for k in range(300)])
    eng = RuleEngine(RULES, {}, None)
    try:
        eng.set_profiling(True)
        eng.evaluate_batch(batch)
        names = [name for name, _, _ in eng.kernel_times()]
        assert "verdict" in names and not [x for x in names if "body" in x or "parse" in x], names
    finally:
        eng.close()
