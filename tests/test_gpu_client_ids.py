"""pwaf_client_ids on the device (client_id_kernel): the captcha client ids it writes equal Python's own
base64url(SHA-256(ip octets || user_agent || host)) for whole batches of every size around a wave, every message length around the padding
edges (neighbouring lanes with different block counts), a host value at every byte phase of a chunk and of its source, one very long
User-Agent in the first and the last lane of a wave; lists with duplicates, entries that name no request and a length word read on the
device, against a pre-fill and a canary; a slab view; the chain evaluate_device -> client_ids on one stream without a synchronisation in
between; and the HOST mode of the same call, byte for byte. Small batches: every case is a few launches."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from pingoo_amd import Request, RequestBatch, _abi, client_ids
from pingoo_amd.engine import DeviceBatch, RuleEngine, lib
from test_client_ids_cpu import HOST, UA, batch_oracle, length_sweep, noise, request
from test_records_cpu import random_batch

pytestmark = pytest.mark.gpu
B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
CANARY = 64  # entries behind the ones a call may write


def device_call(db, idx=None, n_idx=None):
    """pwaf_client_ids in DEVICE mode into a tensor pre-filled with 0x5A that has CANARY entries more than the call may write
    -> (rows, 44) uint8 on the host, after one synchronisation"""
    import torch

    if idx is not None:
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
    cap = db.n if idx is None else len(idx)
    d_idx = None if idx is None else torch.from_numpy(idx.view(np.int32).copy()).to(db.device)
    d_n = None if n_idx is None else torch.tensor([n_idx], dtype=torch.int32, device=db.device)
    d_out = torch.full((cap + CANARY, 44), 0x5A, dtype=torch.uint8, device=db.device)
    st = db.as_struct()
    rc = lib().pwaf_client_ids(C.byref(st), None if d_idx is None else d_idx.data_ptr(), 0 if idx is None else len(idx), None if d_n is None else d_n.data_ptr(),
                               d_out.data_ptr(), C.c_void_p(torch.cuda.current_stream(db.device).cuda_stream))
    assert rc == 0, lib().pwaf_last_error()
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def texts(rows):
    return [r.tobytes().split(b"\0", 1)[0].decode("ascii") for r in rows]


def assert_whole_batch(label, batch, want=None):
    """idx == NULL: entry i is request i's id, 43 characters and a NUL, and nothing is written at or beyond out + n"""
    want = batch_oracle(batch) if want is None else want
    out = device_call(DeviceBatch(batch))
    got = texts(out[:batch.n])
    bad = [i for i in range(batch.n) if got[i] != want[i]]
    assert not bad, f"{label}: {len(bad)} ids differ from hashlib's, first at request {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"
    assert (out[:batch.n, 43] == 0).all() and (out[batch.n:] == 0x5A).all(), f"{label}: written at or beyond out + n"
    return out


@functools.lru_cache(maxsize=None)
def mixed():
    """400 requests of random_batch: both families, empty values, a few values of tens of KiB -> (batch, ids, DeviceBatch)"""
    import torch  # noqa: F401

    batch, _ = random_batch(random.Random(167), 400, 0, False)
    return batch, batch_oracle(batch), DeviceBatch(batch)


# ---- whole batches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 400])
def test_every_request_of_a_batch(n):
    batch, want, _ = mixed()
    assert_whole_batch(f"n = {n}", batch.take(np.arange(n)), want[:n])


def test_every_message_length_around_the_padding_edges_as_one_batch():
    batch, want = length_sweep()
    assert_whole_batch("length sweep", batch, want)


def test_a_host_value_at_every_byte_phase_of_a_chunk_and_of_its_source():
    rng = random.Random(16)
    reqs = []
    for ip in ("198.51.100.7", "2001:db8::77"):
        for ua_len in range(16):  # the host begins at message byte 4 + ua_len (16 + ua_len): every phase of a 16-byte chunk
            for k in range(16):  # 17 or 33 bytes: the next host value begins one source phase further
                reqs.append(request(ip, noise(rng, ua_len), noise(rng, 17 if k % 2 else 33)))
    batch = RequestBatch.from_requests(reqs)
    ho = batch.offsets[HOST].astype(np.int64)
    uo = batch.offsets[UA].astype(np.int64)
    seen = {(int(batch.ip_is_v6[i]), int(uo[i + 1] - uo[i]), int(ho[i]) % 16) for i in range(batch.n)}
    assert len(seen) == 2 * 16 * 16, "every (family, message phase, source phase) occurs"
    assert_whole_batch("alignment", batch)


@pytest.mark.parametrize("at", [0, 63, 64, 127])
def test_one_very_long_user_agent_among_short_ones(at):
    rng = random.Random(at)
    reqs = [request(f"10.0.{i}.1" if i % 3 else f"2001:db8::{i:x}", noise(rng, rng.randint(0, 90)), noise(rng, rng.randint(0, 30))) for i in range(128)]
    reqs[at] = request("10.9.9.9", noise(rng, 40 * 1024 + 13), b"long.example.com")
    assert_whole_batch(f"a 40 KiB User-Agent in lane {at % 64}", RequestBatch.from_requests(reqs))


# ---- lists -----------------------------------------------------------------------------------------------------
def test_lists_with_duplicates_entries_out_of_range_and_the_length_read_on_the_device():
    batch, want, db = mixed()
    n = batch.n
    g = np.random.default_rng(5)
    idx = np.concatenate([g.permutation(n), g.integers(0, n, 40), [n, n + 1, 0xFFFFFFFF, 7, 7, 7]]).astype(np.uint32)
    g.shuffle(idx)
    assert len(idx) > n + 5
    for n_idx in (None, 0, 17, n, n + 5, len(idx), len(idx) + 5):  # one above the capacity is clamped
        m = len(idx) if n_idx is None else min(n_idx, len(idx))
        out = device_call(db, idx, n_idx)
        for j in range(m):
            if idx[j] < n:
                assert texts(out[j:j + 1])[0] == want[idx[j]] and out[j, 43] == 0, (n_idx, j)
            else:
                assert not out[j].any(), "an entry that names no request is 44 zero bytes"
        assert (out[m:] == 0x5A).all(), f"n_idx {n_idx}: entries past m were written (pre-fill or canary)"
    out = device_call(db, idx[:1], None)
    assert texts(out[:1]) == [want[idx[0]] if idx[0] < n else ""] and (out[1:] == 0x5A).all()


def test_a_slab_view_on_the_device():
    batch, want, _ = mixed()
    lo, hi = 101, 283
    view = batch.view(lo, hi)
    assert int(view.offsets[UA][0]) > 0 and int(view.offsets[HOST][0]) > 0
    assert_whole_batch("view", view, want[lo:hi])
    out = device_call(DeviceBatch(view), [0, hi - lo - 1, hi - lo])
    assert texts(out[:3]) == [want[lo], want[hi - 1], ""], "the slab's n bounds the indices, not the arenas"


def test_device_mode_equals_host_mode_byte_for_byte():
    import torch

    batch, _, db = mixed()
    idx = np.random.default_rng(9).integers(0, batch.n + 3, 700).astype(np.uint32)
    for ix in (None, idx):
        m = batch.n if ix is None else len(ix)
        host = np.zeros((m, 44), dtype=np.uint8)
        st = batch.as_struct()
        rc = lib().pwaf_client_ids(C.byref(st), None if ix is None else ix.ctypes.data, 0 if ix is None else m, None, host.ctypes.data, None)
        assert rc == 0
        dev = client_ids(db, None if ix is None else torch.from_numpy(ix.view(np.int32)).to(db.device))  # the Python call, on torch's current stream
        torch.cuda.synchronize()
        assert dev.shape == (m, 44) and (dev.cpu().numpy() == host).all()
        assert client_ids(batch, ix) == texts(host)


# ---- chained with an evaluation ------------------------------------------------------------------------------------
RULES = [("admin", 'http_request.path.contains("/admin")', [B]), ("bots", 'http_request.user_agent.contains("curl")', [CAP]),
         ("bad_ips", 'lists["bad"].contains(client.ip)', [CAP])]
LISTS = {"bad": (_abi.LIST_IP, ["10.9.0.0/16", "2001:db8::/64"])}


def test_evaluate_then_client_ids_on_one_stream_without_a_synchronisation_in_between():
    import torch

    rng = random.Random(77)
    paths = ["/", "/index.html", "/admin/login", "/static/app.js", "/__pingoo/captcha/verify"]
    reqs = [Request(host=rng.choice(["example.com", "a.example.org", ""]), path=(p := rng.choice(paths)), url=p, method="GET",
                    user_agent=rng.choice(["Mozilla/5.0 (X11; Linux x86_64) " + "x" * rng.randint(0, 120), "curl/8.5.0", "ua"]),
                    ip=rng.choice(["10.9.3.4", "10.8.3.4", "192.0.2.7", "2001:db8::9", "2001:db9::9"]), remote_port=rng.randint(1, 65535)) for _ in range(600)]
    batch = RequestBatch.from_requests(reqs)
    want = batch_oracle(batch)
    eng = RuleEngine(RULES, LISTS, None)
    try:
        db = DeviceBatch(batch)
        plain = eng.evaluate_device(db)
        torch.cuda.synchronize()
        plain = plain.cpu().numpy()
        s = torch.cuda.Stream()
        runs = []
        for _ in range(2):  # the same chain twice back to back, into different tensors
            d_idx, d_nm = torch.zeros(batch.n, dtype=torch.int32, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
            s.wait_stream(torch.cuda.current_stream())  # (the zeroing above ran on torch's stream)
            out = eng.evaluate_device(db, match_idx=d_idx, n_matches=d_nm, stream=s.cuda_stream)
            runs.append((out, d_idx, d_nm, eng.client_ids(db, d_idx, n_idx=d_nm, stream=s.cuda_stream)))
        s.synchronize()
        eng.device_status()
        for out, d_idx, d_nm, d_ids in runs:
            verdicts = out.cpu().numpy()
            assert (verdicts == plain).all(), "the verdicts differ from a plain evaluation's"
            k = int(d_nm.item())
            flagged = np.nonzero(verdicts[:, 0] & 0xFF)[0]
            actions = {int(a) & 0xFF for a in verdicts[flagged, 0]}
            assert k == len(flagged) and 50 < k < batch.n - 50 and _abi.ACTION_CAPTCHA in actions, (k, actions)
            match_idx = d_idx.cpu().numpy()[:k]
            assert sorted(match_idx) == sorted(flagged)
            assert texts(d_ids.cpu().numpy()[:k]) == [want[i] for i in match_idx], "a listed request's id differs from hashlib's"
    finally:
        eng.close()
