"""Request records (pwaf_evaluate_records, unpack_records_kernel) and the non-blocking queue (pwaf_async_*) on the device: the verdicts are
pwaf_evaluate_batch's and the oracle's, whatever the records' order, memory kind, GeoIP source or header columns; a malformed buffer is
refused before anything is launched; every submitted tag completes exactly once with its own verdict."""
import random
import select
import threading
import time

import numpy as np
import pytest

import helpers as H
from oracle import pyoracle
from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.engine import AsyncBatcher, PwafError, RuleEngine, lib

pytestmark = pytest.mark.gpu
B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA


def fuzz_engine(seed):
    rng = random.Random(7000 + seed)
    lists = H.fuzz_lists(rng)
    geo = H.fuzz_geoip(rng) if rng.random() < 0.7 else None
    rules = [(f"r{k}", H.rexpr(rng, lists) if rng.random() < 0.95 else None, H.fuzz_actions(rng)) for k in range(rng.randint(1, 14))]
    eng = RuleEngine(rules, lists, geo, flags=_abi.OPT_LENIENT)
    seen, _ = H.as_the_engine_sees(rules, eng.program)
    return rng, eng, pyoracle.Oracle(seen, lists, geo)


class Pinned:
    """buf copied into pwaf_host_alloc'd memory (the direct, one-copy path)."""

    def __init__(self, buf):
        import ctypes as C

        p = C.c_void_p()
        assert lib().pwaf_host_alloc(max(1, buf.nbytes), C.byref(p)) == 0
        self.p = p
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(1, buf.nbytes)).from_address(p.value))[: buf.nbytes]
        self.array[:] = buf

    def free(self):
        lib().pwaf_host_free(self.p)


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_records_match_batch_and_oracle(seed, n):
    rng, eng, oracle = fuzz_engine(seed)
    batch = RequestBatch.from_requests(H.fuzz_requests(rng, n, with_geo=seed % 2 == 1))
    want = oracle.evaluate(batch)
    got_b, counts_b = eng.evaluate_batch(batch, with_counts=True)
    H.assert_verdicts_equal(got_b, want, batch, f"batch, seed {seed}")
    order = np.random.default_rng(seed).permutation(n) if seed % 4 >= 2 else None
    buf, rec_off = batch.to_records(order=order)
    got, counts = eng.evaluate_records(buf, rec_off, with_counts=True)
    H.assert_verdicts_equal(got, want, batch, f"records, seed {seed}")
    assert counts.tolist() == counts_b.tolist() == np.bincount(want["action"], minlength=4).tolist()
    # page-locked: the same verdicts through the one-copy path
    pin = Pinned(buf)
    try:
        H.assert_verdicts_equal(eng.evaluate_records(pin.array, rec_off), want, batch, f"pinned records, seed {seed}")
    finally:
        pin.free()
    # rec_off in any order: verdict i belongs to the record at rec_off[i]
    perm = np.random.default_rng(100 + seed).permutation(n)
    H.assert_verdicts_equal(eng.evaluate_records(buf, rec_off[perm]), want[perm], batch.take(perm), f"shuffled rec_off, seed {seed}")
    eng.close()


def test_records_with_header_columns_and_fewer_values():
    rules = [("tok", 'http_request.headers["x-token"].contains("evil") && http_request.method == "POST"', [B]),
             ("ref", 'http_request.headers["referer"].starts_with("http://spam.") || http_request.headers["cookie"].matches("sid=[0-9]{4}")', [CAP]),
             ("len", 'http_request.headers["x-token"].length() > 20', [B]),
             ("mix", 'http_request.headers["cookie"] + http_request.path == "a=1/p"', [B])]
    eng = RuleEngine(rules)
    rng = random.Random(3)
    vals = ["", "evil", "x" * 25 + "evil", "http://spam.x", "sid=1234", "a=1", "\xff\xfe", "ok"]
    reqs = [Request(path=rng.choice(["/p", "", "/q"]), method=rng.choice(["GET", "POST"]),
                    headers={k: rng.choice(vals) for k in ("x-token", "referer", "cookie", "unused") if rng.random() < 0.7} or None) for _ in range(3000)]
    batch = RequestBatch.from_requests(reqs)
    want = pyoracle.Oracle(rules).evaluate(batch)
    buf, rec_off = batch.to_records(order=np.random.default_rng(1).permutation(batch.n), header_names=eng.header_names)
    assert len(set(np.frombuffer(buf.tobytes(), np.uint8)[rec_off.astype(np.int64)[:, None] + np.arange(4, 6)].view(np.uint16).ravel())) > 1  # n_values varies
    H.assert_verdicts_equal(eng.evaluate_records(buf, rec_off), want, batch, "headers")
    H.assert_verdicts_equal(eng.evaluate_batch(batch), want, batch, "headers, batch")
    eng.close()


@pytest.mark.parametrize("caller_geo", [False, True])
def test_records_geoip_caller_supplied_and_looked_up(caller_geo):
    rules = [("kp", '["KP", "FR"].contains(client.country)', [B]), ("asn", "client.asn == 64512", [CAP])]
    geo = H.fuzz_geoip(random.Random(11))
    eng = RuleEngine(rules, None, geo)
    batch = RequestBatch.from_requests(H.fuzz_requests(random.Random(12), 4000, caller_geo))
    assert (batch.asn is not None) == caller_geo
    want = pyoracle.Oracle(rules, None, geo).evaluate(batch)
    buf, rec_off = batch.to_records()
    H.assert_verdicts_equal(eng.evaluate_records(buf, rec_off), want, batch, f"geo {caller_geo}")
    eng.close()


def test_full_size_config2_records_equal_batch():
    from synth import pysynth

    w = pysynth.Workload(2)
    eng = RuleEngine(w.rules, w.lists, w.geoip)
    n = 1_000_000
    batch = w.batch(0, n)
    want, wc = eng.evaluate_batch(batch, with_counts=True)
    buf, rec_off = batch.to_records(order=np.random.default_rng(5).permutation(n))
    got, counts = eng.evaluate_records(buf, rec_off, with_counts=True)
    assert (got["action"] == want["action"]).all() and (got["rule_idx"] == want["rule_idx"]).all()
    assert counts.tolist() == wc.tolist() == np.bincount(got["action"], minlength=4).tolist()
    eng.close()


def test_malformed_records_are_refused_before_launch():
    eng = RuleEngine([("r", 'http_request.path == "/x"', [B])])
    batch = RequestBatch.from_requests(H.fuzz_requests(random.Random(4), 50, True))
    buf, rec_off = batch.to_records()
    cases = []
    cases.append(("misaligned", buf, np.where(np.arange(50) == 7, rec_off + 8, rec_off).astype(np.uint32), 7))
    cases.append(("past the end", buf[: int(rec_off[49]) + 20], rec_off, 49))
    b2 = buf.copy()
    b2[int(rec_off[3]) + 4: int(rec_off[3]) + 6] = np.frombuffer(np.uint16(4).tobytes(), np.uint8)  # n_values 4
    cases.append(("n_values", b2, rec_off, 3))
    b3 = buf.copy()
    b3[int(rec_off[9]) + 36: int(rec_off[9]) + 40] = np.frombuffer(np.uint32(1 << 20).tobytes(), np.uint8)  # host length overflows size
    cases.append(("lengths", b3, rec_off, 9))
    b4 = buf.copy()
    b4[int(rec_off[11]) + 28] = ord("a")  # country
    cases.append(("country", b4, rec_off, 11))
    b5 = buf.copy()
    b5[int(rec_off[20]) + 32] = 0  # has_geoip differs
    cases.append(("mixed geoip", b5, rec_off, 20))
    for what, b, off, idx in cases:
        with pytest.raises(PwafError) as ei:
            eng.evaluate_records(b, off)
        assert ei.value.code == _abi.E_BATCH and f"record {idx} " in ei.value.message, (what, ei.value.message)
    # the engine is fine afterwards
    assert len(eng.evaluate_records(buf, rec_off)) == 50
    eng.close()


def run_async(q, reqs, threads, results, lock, busy):
    """Python submitters (ctypes releases the GIL around each call): request k tagged k; BUSY is retried after a short sleep."""

    def sub(t):
        for k in range(t, len(reqs), threads):
            while not q.submit(reqs[k], k):
                busy[0] += 1
                time.sleep(0.0005)

    ths = [threading.Thread(target=sub, args=(t,)) for t in range(threads)]
    for th in ths:
        th.start()
    deadline = time.time() + 120
    while len(results) < len(reqs) and time.time() < deadline:
        r, _, _ = select.select([q.fileno()], [], [], 0.2)
        if r:
            q.drain_fd()
        while True:
            got = q.poll(4096)
            if not got:
                break
            with lock:
                for tag, v, st in got:
                    assert tag not in results, f"tag {tag} completed twice"
                    results[tag] = (v, st)
    for th in ths:
        th.join()


def test_async_batcher_every_tag_once_with_the_oracle_verdict():
    rules = [("p", 'http_request.path.starts_with("/a") || http_request.user_agent.contains("b")', [B]),
             ("h", 'http_request.headers["x-k"].contains("z")', [CAP]),
             ("geo", '["FR"].contains(client.country) && client.remote_port < 1000', [B])]
    geo = H.fuzz_geoip(random.Random(21))
    eng = RuleEngine(rules, H.fuzz_lists(random.Random(22)), geo)
    rng = random.Random(23)
    reqs = H.fuzz_requests(rng, 10000, True) + H.fuzz_requests(rng, 10000, False)  # mixed GeoIP
    for r in reqs:
        if rng.random() < 0.5:
            r.headers = {"x-k": rng.choice(["", "z", "azb", "q"])}
    rng.shuffle(reqs)
    want_geo = pyoracle.Oracle(rules, H.fuzz_lists(random.Random(22)), geo)
    want = {}
    for flag in (True, False):
        idx = [k for k, r in enumerate(reqs) if (r.asn is not None) == flag]
        w = want_geo.evaluate(RequestBatch.from_requests([reqs[k] for k in idx], with_geoip=flag))
        want.update({k: (int(w[i]["action"]), int(w[i]["rule_idx"])) for i, k in enumerate(idx)})
    q = AsyncBatcher(eng, max_batch=1024, max_delay_us=300, max_in_flight=4096)
    results, lock, busy = {}, threading.Lock(), [0]
    run_async(q, reqs, 8, results, lock, busy)
    assert len(results) == len(reqs)
    bad = [k for k, (v, st) in results.items() if st != 0 or (int(v.decision), _ridx(v)) != want[k]]
    assert not bad, [(k, results[k], want[k]) for k in bad[:5]]
    nb, nr, fl = q.stats()
    assert nr == len(reqs) and fl == 0 and nb < len(reqs) / 4, (nb, nr, fl)
    q.close()
    eng.close()


def _ridx(v):
    return {"user_agent": _abi.RULE_UA_GATE, "captcha_endpoint": _abi.RULE_CAPTCHA_ENDPOINT}.get(v.gate, _abi.RULE_NONE if v.rule_idx is None else v.rule_idx)


def test_async_batcher_busy_flush_and_close_in_flight():
    rules = [("p", 'http_request.path.starts_with("/a")', [B])]
    eng = RuleEngine(rules)
    reqs = [Request(path=f"/{'a' if k % 3 == 0 else 'b'}{k}") for k in range(3000)]
    want = {k: B if k % 3 == 0 else 0 for k in range(3000)}
    # BUSY and recovery: 64 in flight at most
    q = AsyncBatcher(eng, max_batch=4096, max_delay_us=200, max_in_flight=64)
    results, lock, busy = {}, threading.Lock(), [0]
    run_async(q, reqs, 8, results, lock, busy)
    assert busy[0] > 0 and len(results) == len(reqs)
    assert all(st == 0 and int(v.decision) == want[k] for k, (v, st) in results.items())
    q.close()
    # flush: a 10 s deadline, yet the requests come back at once
    q = AsyncBatcher(eng, max_batch=65536, max_delay_us=10_000_000, max_in_flight=65536)
    for k in range(100):
        assert q.submit(reqs[k], k)
    t0 = time.time()
    q.flush()
    got = []
    while len(got) < 100 and time.time() - t0 < 5:
        select.select([q.fileno()], [], [], 0.1)
        q.drain_fd()
        got += q.poll(4096)
    assert len(got) == 100 and time.time() - t0 < 5
    # close with requests in flight: every accepted request is evaluated first
    for k in range(100, 2100):
        assert q.submit(reqs[k], k)
    q.close()
    eng.close()
