"""pwaf_verify_pow on the device (pow_check_kernel, pow_verify_kernel): the statuses it writes equal the HOST mode's and the independent
oracle's (tests/pow_oracle.py), and scratch word 0 the number of entries the oracle hands to the signature stage, for batches of every
size around a wave, a flood of wrong hashes under valid tokens (nothing reaches the curve), everybody passing and everybody with the
neighbour's token, one submission in 16, a cookie value and a nonce that end at their arena's last byte, a list that a preceding
evaluation wrote on the same stream, and two calls on two streams with one key set. Small batches: every case is a few launches."""
import ctypes as C
import functools
import hashlib
import random

import numpy as np
import pytest

import pow_oracle as O
from pingoo_amd import KeySet, Request, RequestBatch, _abi, pow_handed, verify_pow
from pingoo_amd.engine import DeviceBatch, RuleEngine, cookie_column, lib
from test_verify_pow_cpu import HOST, KEYS, KIDS, NAME, NOW, SEEDS, UA, Case, batch_of, corpus, corpus_oracle, hash_flip_cases, flip, packed, raw, signature_flip_cases, work

pytestmark = pytest.mark.gpu
A, P, F, U = O.ABSENT, O.PASSED, O.FAILED, O.UNDECIDED
CANARY = 64
VERIFY_PATH = b"/__pingoo/captcha/api/verify"


@functools.lru_cache(maxsize=None)
def keyset():
    return KeySet(KEYS, device="cuda:0")


@functools.lru_cache(maxsize=None)
def host_keyset():
    return KeySet(KEYS)


@functools.lru_cache(maxsize=None)
def mixed():
    """the corpus, every fourth hash flip and every fourth signature flip, shuffled until the first 64 hold all four statuses
    -> (cases, [(oracle status, handed to the signature stage)])"""
    flips, sigs = hash_flip_cases()[::4], signature_flip_cases()[::4]
    cases = list(corpus()) + flips + sigs
    want = corpus_oracle() + [(F, False)] * len(flips) + [(F, True)] * len(sigs)
    order = list(range(len(cases)))
    random.Random(64).shuffle(order)
    cases, want = [cases[k] for k in order], [want[k] for k in order]
    assert len(cases) >= 256 and {A, P, F, U} == {s for s, _ in want[:64]}, "all four statuses among the first 64"
    return cases, want


def upload(values, device):
    """a string column with exactly PWAF_ARENA_PAD bytes behind its last value -> (data, offsets) tensors"""
    import torch

    data, off = cookie_column(values)
    assert len(data) == int(off[-1]) + _abi.ARENA_PAD
    return torch.from_numpy(data).to(device), torch.from_numpy(off.view(np.int32)).to(device)


def device_call(db, col, hashes, ncol, idx=None, n_idx=None, stream=None, ks=None):
    """pwaf_verify_pow in DEVICE mode into a tensor pre-filled with 0x5A that has CANARY entries more than the call may write, enqueued on
    `stream` (default: torch's current stream) -> (the status tensor, the scratch, everything that must outlive the launches)"""
    import torch

    cap = db.n if idx is None else idx.numel()
    out = torch.full((cap + CANARY,), 0x5A, dtype=torch.uint8, device=db.device)
    need = int(lib().pwaf_verify_pow_scratch_bytes(cap))
    scratch = torch.full((max(16, need),), 0xEE, dtype=torch.uint8, device=db.device)
    st, c, nc = db.as_struct(), _abi.StrCol(), _abi.StrCol()
    c.data, c.offsets, nc.data, nc.offsets = col[0].data_ptr(), col[1].data_ptr(), ncol[0].data_ptr(), ncol[1].data_ptr()
    rc = lib().pwaf_verify_pow((ks or keyset())._h, C.byref(st), C.byref(c), hashes.data_ptr(), C.byref(nc), NOW, None if idx is None else idx.data_ptr(), 0 if idx is None else cap,
                               None if n_idx is None else n_idx.data_ptr(), out.data_ptr(), scratch.data_ptr(), need,
                               C.c_void_p(torch.cuda.current_stream(db.device).cuda_stream if stream is None else stream))
    assert rc == 0, lib().pwaf_last_error()
    return out, scratch, (st, c, nc, hashes)


def word0(scratch):
    return int(scratch[:4].cpu().numpy().view(np.uint32)[0])


def on_device(cases):
    import torch

    batch, cookies, hashes, nonces = batch_of(cases)
    db = DeviceBatch(batch)
    return batch, db, upload(cookies, db.device), torch.from_numpy(hashes).to(db.device), upload(nonces, db.device), (cookies, hashes, nonces)


def assert_whole_batch(label, cases, want):
    """idx == NULL: status i is request i's, equal to the oracle's and the HOST mode's; word 0 counts the oracle's signature-stage
    entries; nothing is written at or beyond status + n -> word 0"""
    import torch

    batch, db, col, d_hashes, ncol, (cookies, hashes, nonces) = on_device(cases)
    out, scratch, keep = device_call(db, col, d_hashes, ncol)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    host = verify_pow(host_keyset(), batch, cookies, hashes, nonces, NOW)
    bad = [i for i in range(batch.n) if got[i] != want[i][0] or host[i] != want[i][0]]
    assert not bad, f"{label}: {len(bad)} statuses differ, first at request {bad[0]} ({cases[bad[0]].label}): device {got[bad[0]]}, host {host[bad[0]]}, oracle {want[bad[0]][0]}"
    assert (got[batch.n:] == 0x5A).all(), f"{label}: written at or beyond status + n"
    handed = word0(scratch)
    assert handed == sum(h for _, h in want), f"{label}: {handed} entries were handed to the signature stage, the oracle hands {sum(h for _, h in want)}"
    del keep
    return handed


# ---- whole batches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_every_request_of_a_batch(n):
    cases, want = mixed()
    assert_whole_batch(f"n = {n}", cases[:n], want[:n])


def test_the_rest_of_the_corpus():
    cases, want = mixed()
    assert_whole_batch("the corpus behind its first 130", cases[130:], want[130:])


@functools.lru_cache(maxsize=None)
def clients():
    """130 clients with a passing submission of their own: addresses of both families, User-Agents and hosts of many lengths, all three keys,
    difficulty 1 or 2, challenges with the NUL (genuine-shaped) -> [Case]"""
    cases = []
    for k in range(130):
        ip, ua, host = (f"10.1.{k}.9" if k % 3 else f"2001:db8::{k + 1:x}"), UA + b"/%d" % k, HOST if k % 2 else b"h%d.example.com" % k
        challenge = O.heapless44(hashlib.sha256(b"challenge %d" % k).digest())
        d = 1 + k % 2
        nonce, digest = O.search_nonce(raw(challenge), d, exactly=False)
        claims = O.claims_json(O.client_sub(packed(ip), ua, host), NOW, challenge, d, jti="j" * (k % 40))
        cases.append(Case(f"client {k}", P, NAME + b"=" + O.mint(SEEDS[k % 3], O.header_json(KIDS[k % 3]), claims), digest, nonce, ip=ip, ua=ua, host=host))
    return cases


def test_wrong_hashes_under_valid_tokens_never_reach_the_signature_stage():
    rng = random.Random(130)
    cases = [Case(c.label, F, c.cookie, flip(c.digest, rng.randrange(8, 256)), c.nonce, ip=c.ip, ua=c.ua, host=c.host) for c in clients()]
    assert [c.oracle() for c in cases[::13]] == [(F, False)] * 10
    assert assert_whole_batch("130 wrong hashes", cases, [(F, False)] * 130) == 0


def test_everybody_passes_with_a_token_of_their_own_and_fails_with_the_neighbour_s():
    cases = clients()
    assert [c.oracle() for c in cases[::13]] == [(P, True)] * 10
    assert assert_whole_batch("everybody", cases, [(P, True)] * 130) == 130
    swapped = [Case(c.label, F, cases[(k + 1) % 130].cookie, c.digest, c.nonce, ip=c.ip, ua=c.ua, host=c.host) for k, c in enumerate(cases)]  # the hash no longer fits the challenge
    assert swapped[5].oracle() == (F, False)
    assert assert_whole_batch("everybody, the neighbour's token", swapped, [(F, False)] * 130) == 0


def test_one_submission_in_16_at_random_places():
    cases, want = mixed()
    carriers = [(c, w) for c, w in zip(cases, want) if w[0] != A]
    rng = random.Random(16)
    n = 400
    places = set(rng.sample(range(n), n // 16))
    batch_cases, expect = [], []
    for k in range(n):
        if k in places:
            c, w = carriers[rng.randrange(len(carriers))]
        else:
            c, w = Case(f"none {k}", A, b"lang=en; id=%d" % k if k % 2 else None, ip=f"10.2.{k % 200}.1"), (A, False)
        batch_cases.append(c), expect.append(w)
    assert {P, F, U} <= {s for s, _ in expect}
    assert_whole_batch("one in 16", batch_cases, expect)


def test_a_cookie_value_and_a_nonce_that_end_at_their_arena_s_last_byte():
    good, (nonce, digest) = corpus()[0].cookie, work()
    for tail, tail_nonce, status in ((good, nonce, P), (b"a=b; " + good, nonce, P), (good + b";", nonce, P), (good[:-1], nonce, F), (good, nonce + b"0", F), (good, b"", F)):
        cases = [Case("first", P, good), Case("none", A, None), Case("last", status, tail, digest, tail_nonce)]
        want = [(P, True), (A, False), cases[2].oracle()]
        assert want[2][0] == status
        assert_whole_batch(f"the arenas end with ...{tail[-6:]!r} and ...{tail_nonce[-3:]!r}", cases, want)  # (upload() asserts the PWAF_ARENA_PAD bytes behind)
    challenge = "c" * 20
    cases = [Case("an empty nonce last", P, NAME + b"=" + O.mint(SEEDS[0], O.header_json(KIDS[0]), O.claims_json(O.client_sub(packed("203.0.113.7"), UA, HOST), NOW, challenge, 0)),
                  hashlib.sha256(raw(challenge)).digest(), b"")]
    assert_whole_batch("an empty nonce at the arena's end", cases, [(P, True)])


# ---- lists, chained with an evaluation -------------------------------------------------------------------------------
RULES = [("shop", 'http_request.path.starts_with("/shop")', [_abi.RULE_ACTION_BLOCK])]


def test_the_match_list_of_a_preceding_evaluation_on_the_same_stream():
    import torch

    cases, want = mixed()
    rng = random.Random(300)
    reqs, picked, expect, handed = [], [], [], []
    for k in range(300):
        j = rng.randrange(len(cases))
        c = cases[j]
        path = VERIFY_PATH if k % 3 else b"/about"
        reqs.append(Request(host=c.host, url=path, path=path, method=b"POST", user_agent=c.ua, ip=c.ip, remote_port=1000 + k))
        picked.append(c), expect.append(want[j][0]), handed.append(want[j][1])
    batch = RequestBatch.from_requests(reqs)
    _, cookies, hashes, nonces = batch_of(picked)
    eng = RuleEngine(RULES, {}, None)
    try:
        db = DeviceBatch(batch)
        col, ncol, d_hashes = upload(cookies, db.device), upload(nonces, db.device), torch.from_numpy(hashes).to(db.device)
        s = torch.cuda.Stream()
        d_idx, d_nm = torch.zeros(batch.n, dtype=torch.int32, device=db.device), torch.zeros(1, dtype=torch.int32, device=db.device)
        s.wait_stream(torch.cuda.current_stream())
        verdicts = eng.evaluate_device(db, match_idx=d_idx, n_matches=d_nm, stream=s.cuda_stream)
        out, scratch, keep = device_call(db, col, d_hashes, ncol, idx=d_idx, n_idx=d_nm, stream=s.cuda_stream)  # no synchronisation in between
        s.synchronize()
        eng.device_status()
        k = int(d_nm.item())
        v = verdicts.cpu().numpy()
        bypass = np.nonzero((v[:, 0] & 0xFF) == _abi.ACTION_BYPASS)[0]
        match_idx = d_idx.cpu().numpy()[:k]
        assert k == 200 and sorted(match_idx) == sorted(bypass) == [i for i in range(300) if i % 3], "requests on the verify endpoint are BYPASS and in match_idx"
        assert (v[bypass, 1].astype(np.uint32) == _abi.RULE_CAPTCHA_ENDPOINT).all()
        got = out.cpu().numpy()
        assert list(got[:k]) == [expect[i] for i in match_idx], "a listed request's status differs from the oracle's"
        assert (got[k:] == 0x5A).all(), "entries at or past n_matches were written"
        # the Python call with the same list, and a list with entries that name no request
        py = eng.verify_pow(keyset(), db, col, d_hashes, ncol, NOW, idx=d_idx, n_idx=d_nm)
        odd = torch.tensor([5, batch.n, 5, -1, 0], dtype=torch.int32, device=db.device)
        py_odd = verify_pow(keyset(), db, cookies, [c.digest for c in picked], nonces, NOW, idx=odd)
        want_handed = [handed[5], handed[5], handed[0]]
        torch.cuda.synchronize()
        assert list(py.cpu().numpy()[:k]) == [expect[i] for i in match_idx] and pow_handed(py) == word0(scratch) and pow_handed(py_odd) == sum(want_handed)
        assert list(py_odd.cpu().numpy()) == [expect[5], A, expect[5], A, expect[0]]
        del keep
    finally:
        eng.close()


def test_two_calls_on_two_streams_with_one_key_set():
    import torch

    cases, want = mixed()
    halves = [(cases[:150], want[:150]), (cases[100:260], want[100:260])]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    runs = []
    for (cs, _), s in zip(halves, streams):
        _, db, col, d_hashes, ncol, _ = on_device(cs)
        s.wait_stream(torch.cuda.current_stream())
        runs.append((device_call(db, col, d_hashes, ncol, stream=s.cuda_stream), db, col, ncol))
    for s in streams:
        s.synchronize()
    for ((out, scratch, keep), db, _, _), (_, w) in zip(runs, halves):
        got = out.cpu().numpy()
        assert list(got[:db.n]) == [s for s, _ in w] and (got[db.n:] == 0x5A).all() and word0(scratch) == sum(h for _, h in w)


def test_a_host_only_key_set_and_a_short_scratch_are_refused():
    import torch

    _, db, col, d_hashes, ncol, _ = on_device(corpus()[:4])
    st, c, nc = db.as_struct(), _abi.StrCol(), _abi.StrCol()
    c.data, c.offsets, nc.data, nc.offsets = col[0].data_ptr(), col[1].data_ptr(), ncol[0].data_ptr(), ncol[1].data_ptr()
    out = torch.full((8,), 0x5A, dtype=torch.uint8, device=db.device)
    need = int(lib().pwaf_verify_pow_scratch_bytes(4))
    assert need == 16 + 24 * 4
    scratch = torch.empty(need + 16, dtype=torch.uint8, device=db.device)
    call = lambda ks, ptr, size: lib().pwaf_verify_pow(ks._h, C.byref(st), C.byref(c), d_hashes.data_ptr(), C.byref(nc), NOW, None, 0, None, out.data_ptr(), ptr, size, None)  # noqa: E731
    assert call(host_keyset(), scratch.data_ptr(), need) == _abi.E_DEVICE
    assert call(keyset(), None, need) == _abi.E_INVALID_ARG
    assert call(keyset(), scratch.data_ptr(), need - 1) == _abi.E_INVALID_ARG
    assert call(keyset(), scratch.data_ptr() + 8, need) == _abi.E_INVALID_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A).all()
