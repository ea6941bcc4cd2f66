"""pwaf_evaluate_records_device: request records that lie in device memory are validated, scanned into column offsets and evaluated
without visiting the host. Verdicts, counters and the match_idx set equal pwaf_evaluate_records' (host) on the same bytes and the oracle's,
at every tile and step boundary of the scan; a malformed call is refused with the host call's text and touches no output; the chain
evaluate_device -> export_records -> evaluate_records_device runs on one stream with no synchronisation by the caller; the record count is
read on the device; two calls overlap on two streams; and the launch list is the three scan launches, the unpack, then a plain device
batch's. Every case is a handful of launches."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from oracle import pyoracle
from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.engine import DeviceBatch, PwafError, RuleEngine, export_stats, lib, records_scan_shape
from test_records_cpu import random_batch
from test_records_device_cpu import malformed_set

pytestmark = pytest.mark.gpu
B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
CANARY = 0x5A5A5A5A
SCAN_NAMES = ["records_check_kernel", "records_bases_kernel", "records_offsets_kernel"]
FIELDS = ["host", "url", "path", "method", "user_agent"]
HEADERS = ["h0", "h1", "h2"]
COLUMNS = [f"http_request.{f}" for f in FIELDS] + [f'http_request.headers["{h}"]' for h in HEADERS]
KINDS = ["starts_with", "ends_with", "length", "equals"]


def trigger(c, kind):
    """the value of column c that only column c's rule of that kind matches (every other trigger and every filler is 10 bytes or shorter)"""
    return {"starts_with": f"S{c}x-tail-q", "ends_with": f"q-head-x{c}E", "length": "q" * (23 + c), "equals": f"EQ-value-{c}"}[kind].encode()


def column_rules():
    """a starts_with, an ends_with, a length() == and an == over each of the five fields and over three headers; then one rule on the port"""
    rules = []
    for c, col in enumerate(COLUMNS):
        rules += [(f"sw{c}", f'{col}.starts_with("S{c}x")', [B]), (f"ew{c}", f'{col}.ends_with("x{c}E")', [CAP]), (f"len{c}", f"{col}.length() == {23 + c}", [B]),
                  (f"eq{c}", f'{col} == "EQ-value-{c}"', [CAP])]
    return rules + [("lowport", "client.remote_port < 1024", [CAP])]


RULES = column_rules()


def request(rng, values, port=None, verified=None):
    f = [values.get(c, rng.choice([b"", b"n0", b"filler/1", b"zz"] if c < 5 else [b"", b"", b"", b"", b"n0"])) for c in range(8)]
    return Request(host=f[0], url=f[1], path=f[2], method=f[3], user_agent=f[4], ip=f"10.{rng.randint(0, 255)}.1.2",
                   remote_port=rng.randint(1024, 65535) if port is None else port, captcha_verified=rng.random() < 0.5 if verified is None else verified,
                   headers={h: f[5 + k] for k, h in enumerate(HEADERS) if f[5 + k]})


@functools.lru_cache(maxsize=None)
def traffic():
    """Rich requests — one per (column, kind) that only that rule matches, then mixtures — followed by 1024 MINIMAL ones (every value
    empty: a 64-byte record; the empty user agent makes the user-agent gate answer them). -> (batch, the oracle's verdicts, first minimal request)"""
    rng = random.Random(31)
    reqs = [request(rng, {c: trigger(c, k)}, verified=False) for c in range(8) for k in KINDS]
    for _ in range(232):
        reqs.append(request(rng, {c: trigger(c, rng.choice(KINDS)) for c in rng.sample(range(8), rng.randint(0, 2))}, port=rng.choice([None, None, 80])))
    n_rich = len(reqs)
    reqs += [Request(host=b"", url=b"", path=b"", method=b"", user_agent=b"", ip="10.0.0.1", remote_port=rng.choice([22, 443, 8080, 50000])) for _ in range(1024)]
    batch = RequestBatch.from_requests(reqs)
    want = pyoracle.Oracle(RULES, None, None).evaluate(batch)
    decided = {int(r) for r in want["rule_idx"][want["action"] != 0]}
    assert decided >= set(range(len(RULES))), f"rules that decide no request: {sorted(set(range(len(RULES))) - decided)}"
    return batch, want, n_rich


@functools.lru_cache(maxsize=None)
def engine():
    eng = RuleEngine(RULES, None, None)
    assert sorted(eng.header_names) == HEADERS
    return eng


@functools.lru_cache(maxsize=None)
def records():
    batch, want, n_rich = traffic()
    buf, rec_off = batch.to_records(header_names=engine().header_names)
    sizes = [int(np.frombuffer(buf[int(o):int(o) + 4].tobytes(), np.uint32)[0]) for o in rec_off[n_rich:n_rich + 8]]
    assert sizes == [64] * 8, "the minimal records are 64 bytes each"
    return np.ascontiguousarray(buf), rec_off


def device_call(eng, buf, rec_off, n_rec=None, stream=None, raw=False):
    """One call with canaries everywhere -> dict of device tensors (and rc / error text with raw=True). Nothing is synchronised here."""
    import torch

    n = len(rec_off)
    t = dict(buf=torch.from_numpy(np.ascontiguousarray(buf, np.uint8)).to("cuda:0") if len(buf) else torch.zeros(16, dtype=torch.uint8, device="cuda:0")[:0],
             off=torch.from_numpy(np.ascontiguousarray(rec_off, np.uint32).view(np.int32).copy()).to("cuda:0"),
             out=torch.full((max(n, 1), 2), CANARY, dtype=torch.int32, device="cuda:0"), counts=torch.zeros(4, dtype=torch.int64, device="cuda:0"),
             idx=torch.full((max(n, 1),), CANARY, dtype=torch.int32, device="cuda:0"), nm=torch.zeros(1, dtype=torch.int32, device="cuda:0"),
             n_rec=None if n_rec is None else torch.tensor([n_rec], dtype=torch.int64, device="cuda:0").view(torch.int32)[:1])
    assert t["buf"].data_ptr() % 16 == 0
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())  # (the tensors above were filled on torch's stream)
    s = (torch.cuda.current_stream() if stream is None else stream).cuda_stream
    if raw:
        t["counts"].fill_(0x77)
        t["nm"].fill_(0x77)
        torch.cuda.synchronize()
        t["rc"] = lib().pwaf_evaluate_records_device(eng._h, t["buf"].data_ptr(), len(buf), t["off"].data_ptr(), n, None if n_rec is None else t["n_rec"].data_ptr(),
                                                     t["out"].data_ptr(), t["counts"].data_ptr(), t["idx"].data_ptr(), t["nm"].data_ptr(), C.c_void_p(s))
        t["text"] = lib().pwaf_last_error()
    else:
        eng.evaluate_records_device(t["buf"], t["off"][:n], n_rec=t["n_rec"], out=t["out"], counts=t["counts"], match_idx=t["idx"], n_matches=t["nm"], stream=s)
    return t


def assert_answers(label, t, want, m=None):
    """the synchronised call's verdicts, counters and match_idx set against `want` (the first m of the call's records)"""
    m = len(want) if m is None else m
    out = t["out"].cpu().numpy()
    got = out.view(want.dtype).reshape(-1)[:m]
    bad = np.nonzero(got != want[:m])[0]
    assert not len(bad), f"{label}: {len(bad)} of {m} verdicts differ; first at {int(bad[0])}: got {got[bad[0]]} want {want[bad[0]]}"
    assert (out[m:] == np.int32(CANARY)).all(), f"{label}: out[m:] was written"
    assert (t["counts"].cpu().numpy() == np.bincount(want["action"][:m], minlength=4)).all(), label
    k = int(t["nm"].item())
    flagged = np.nonzero(want["action"][:m] != 0)[0]
    assert k == len(flagged) and sorted(t["idx"].cpu().numpy()[:k].tolist()) == flagged.tolist(), f"{label}: the match_idx set"


# ---- verdicts ------------------------------------------------------------------------------------------------
def test_verdicts_counters_and_matches_at_every_scan_boundary():
    import torch

    batch, want_all, n_rich = traffic()
    eng = engine()
    buf, rec_off = records()
    shape = records_scan_shape()
    T, step = shape["tile"], shape["step"]
    g = np.random.default_rng(12)
    for n in (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, step * T + 1):
        # duplicated, permuted and skipped; the largest list names mostly minimal records
        pick = g.integers(0, n_rich, n) if n <= 2 * T + 1 else np.where(g.random(n) < 0.05, g.integers(0, n_rich, n), g.integers(n_rich, batch.n, n))
        if n == T + 1 and n_rich >= T:
            pick = np.concatenate([np.arange(T), [0]])  # a tile of records once each, in order, and a shared one
        want = want_all[pick]
        t = device_call(eng, buf, rec_off[pick])
        torch.cuda.synchronize()
        eng.device_status()
        assert_answers(f"n = {n}", t, want)
        if n in (65, 2 * T + 1, step * T + 1):
            host, counts = eng.evaluate_records(buf, rec_off[pick], with_counts=True)
            assert (host == want).all() and (counts == np.bincount(want["action"], minlength=4)).all(), f"n = {n}: the host call on the same bytes"


def test_sixty_four_header_columns():
    import torch

    rng = random.Random(64)
    batch, names = random_batch(rng, 200, 64, True)
    rules = [(f"r{k}", f'http_request.headers["{nm}"].starts_with("a")', [B if k % 2 else CAP]) for k, nm in enumerate(names)]
    want = pyoracle.Oracle(rules, None, None).evaluate(batch)
    assert len({int(r) for r in want["rule_idx"][want["action"] != 0]}) >= 20
    eng = RuleEngine(rules, None, None)
    try:
        assert len(eng.header_names) == 64
        buf, rec_off = batch.to_records(order=np.random.default_rng(1).permutation(200), header_names=eng.header_names)
        nv = buf[rec_off.astype(np.int64)[:, None] + np.arange(4, 6)].copy().view(np.uint16).ravel()
        assert nv.max() > 64 and nv.min() < 69, "records on both sides of 64 lengths"
        t = device_call(eng, buf, rec_off)
        torch.cuda.synchronize()
        eng.device_status()
        assert_answers("64 headers", t, want)
        assert (eng.evaluate_records(buf, rec_off) == want).all()
    finally:
        eng.close()


def test_values_of_tens_of_kib():
    import torch

    rng = random.Random(46)
    batch, names = random_batch(rng, 300, 3, True)
    assert names == HEADERS
    big = max(int(np.diff(batch.offsets[1].astype(np.int64)).max()), int(np.diff(batch.offsets[4].astype(np.int64)).max()))
    assert big >= 32768, "the batch carries values of tens of KiB"
    rules = RULES + [("long", "http_request.url.length() > 1000", [B]), ("ua", 'http_request.user_agent.ends_with("a")', [CAP])]
    want = pyoracle.Oracle(rules, None, None).evaluate(batch)
    assert {len(RULES), len(RULES) + 1} <= {int(r) for r in want["rule_idx"][want["action"] != 0]}
    eng = RuleEngine(rules, None, None)
    try:
        buf, rec_off = batch.to_records(header_names=eng.header_names)
        pick = np.random.default_rng(2).integers(0, 300, 700)
        t = device_call(eng, buf, rec_off[pick])
        torch.cuda.synchronize()
        eng.device_status()
        assert_answers("large values", t, want[pick])
        assert (eng.evaluate_records(buf, rec_off[pick]) == want[pick]).all()
    finally:
        eng.close()


# ---- malformed calls -----------------------------------------------------------------------------------------
def host_refusal(eng, buf, rec_off):
    buf, rec_off = np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(rec_off, np.uint32)
    out = np.zeros(len(rec_off), dtype=[("action", np.uint32), ("rule_idx", np.uint32)])
    rc = lib().pwaf_evaluate_records(eng._h, buf.ctypes.data, buf.nbytes, rec_off.ctypes.data, len(rec_off), out.ctypes.data, None)
    return rc, lib().pwaf_last_error()


def assert_refused(label, eng, buf, rec_off):
    import torch

    rc, text = host_refusal(eng, buf, rec_off)
    assert rc == _abi.E_BATCH and text, label
    t = device_call(eng, buf, rec_off, raw=True)
    torch.cuda.synchronize()
    assert t["rc"] == _abi.E_BATCH and t["text"] == text, (label, t["rc"], t["text"], text)
    assert (t["out"].cpu().numpy() == np.int32(CANARY)).all() and (t["idx"].cpu().numpy() == np.int32(CANARY)).all(), f"{label}: out / match_idx written"
    assert (t["counts"].cpu().numpy() == 0x77).all() and int(t["nm"].item()) == 0x77, f"{label}: counts / n_matches written"
    return text


def test_malformed_calls_are_refused_with_the_host_text_and_touch_nothing():
    import torch

    whole, rec_off, n_cols, bad = malformed_set(3)
    eng = engine()
    assert n_cols == _abi.N_FIELDS + len(eng.header_names)
    T = records_scan_shape()["tile"]
    n = T + 9
    g = np.random.default_rng(8)
    seen = set()
    for k, (name, check, at) in enumerate(bad):  # one per check a record can fail, at a different place each
        off = rec_off[g.integers(0, 40, n)].copy()
        p = [0, T - 1, T, n - 1, 77][k % 5] if check != 8 else 77
        off[p] = at
        text = assert_refused(name, eng, whole, off)
        assert text.startswith(f"record {p} (offset {int(np.uint32(at))}): ".encode()), (name, text)
        seen.add(text.split(b"): ", 1)[1])
    assert len(seen) == 8, "kMisaligned .. kMixedGeo, each with its own message"
    off = rec_off[g.integers(0, 40, n)].copy()
    off[T + 3], off[T - 5] = bad[0][2], bad[7][2]  # two bad records: the lower index, whatever its check
    assert assert_refused("two bad records", eng, whole, off).startswith(f"record {T - 5} ".encode())
    # a column over 4 GiB without 4 GiB of data: one record with a 64 KiB url, named 70 000 times
    batch = RequestBatch.from_requests([Request(url=b"u" * 65536)])
    big, big_off = batch.to_records(header_names=eng.header_names)
    text = assert_refused("column overflow", eng, big, np.zeros(70000, np.uint32))
    assert b"4 GiB" in text
    # a valid call on the same engine right after
    _, want_all, n_rich = traffic()
    buf, ok_off = records()
    pick = g.integers(0, n_rich, 300)
    t = device_call(eng, buf, ok_off[pick])
    torch.cuda.synchronize()
    eng.device_status()
    assert_answers("after the refusals", t, want_all[pick])


# ---- the chain -----------------------------------------------------------------------------------------------
RULES_A = [(f"a{k}", f'http_request.headers["{h}"].length() > 0', [B if k else CAP]) for k, h in enumerate(HEADERS)]


@pytest.mark.parametrize("short", [False, True])
def test_evaluate_export_evaluate_on_one_stream_without_a_synchronisation(short):
    import torch

    batch, want_all, n_rich = traffic()
    # short: few enough flagged requests for ONE 64-entry group of the export, whose records then fill the buffer in list order — the
    # records that do not fit a smaller buffer are the list's last ones, and n_written counts a prefix of rec_off
    lo, hi = (0, 60) if short else (0, n_rich + 100)
    view = batch.view(lo, hi)
    want_a = pyoracle.Oracle(RULES_A, None, None).evaluate(view)
    n_flagged = int((want_a["action"] != 0).sum())
    assert 10 < n_flagged < view.n - 10 and (not short or n_flagged <= 64)
    eng_a, eng_b = RuleEngine(RULES_A, None, None), engine()
    try:
        assert eng_a.header_names == eng_b.header_names
        db = DeviceBatch(view)
        cap = None
        if short:
            _, _, stats = eng_a.export_records(db, torch.from_numpy(np.nonzero(want_a["action"] != 0)[0].astype(np.int32)).to("cuda:0"))
            torch.cuda.synchronize()
            cap = export_stats(stats)["bytes_needed"] - 16
        s = torch.cuda.Stream()
        d_idx, d_nm = torch.zeros(view.n, dtype=torch.int32, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
        out_b = torch.full((view.n, 2), CANARY, dtype=torch.int32, device="cuda:0")
        s.wait_stream(torch.cuda.current_stream())
        out_a = eng_a.evaluate_device(db, match_idx=d_idx, n_matches=d_nm, stream=s.cuda_stream)
        d_buf, d_off, d_stats = eng_a.export_records(db, d_idx, n_idx=d_nm, cap=cap, stream=s.cuda_stream)
        n_written = d_stats.view(torch.int32)[3:4]  # pwaf_export_stats::n_written, where the export leaves it
        eng_b.evaluate_records_device(d_buf, d_off, n_rec=n_written, out=out_b, stream=s.cuda_stream)
        s.synchronize()
        eng_a.device_status()
        eng_b.device_status()
        assert (out_a.cpu().numpy().view(want_a.dtype).reshape(-1) == want_a).all()
        stats = export_stats(d_stats)
        k = stats["n_written"]
        assert stats["n_selected"] == n_flagged and (k < n_flagged if short else k == n_flagged), stats
        exported = d_idx.cpu().numpy()[:k] + lo
        assert (d_off.cpu().numpy().view(np.uint32)[:k] != _abi.RECORD_NONE).all()
        got = out_b.cpu().numpy()
        assert (got[:k].view(want_all.dtype).reshape(-1) == want_all[exported]).all(), "engine B's verdicts for exactly the exported requests"
        assert (got[k:] == np.int32(CANARY)).all()
    finally:
        eng_a.close()


# ---- the record count ----------------------------------------------------------------------------------------
def test_the_record_count_is_read_on_the_device():
    import torch

    _, want_all, n_rich = traffic()
    eng = engine()
    buf, rec_off = records()
    T = records_scan_shape()["tile"]
    n = T + 30
    pick = np.random.default_rng(3).integers(0, n_rich, n)
    for n_rec in (0, 1, T, T + 1, n, n + 1, 0xFFFFFFFF):
        t = device_call(eng, buf, rec_off[pick], n_rec=n_rec)
        torch.cuda.synchronize()
        eng.device_status()
        assert_answers(f"n_rec = {n_rec}", t, want_all[pick], m=min(n_rec, n))
    # a bad record behind the count is never looked at
    off = rec_off[pick].copy()
    off[T + 5] = 4
    t = device_call(eng, buf, off, n_rec=T + 5)
    torch.cuda.synchronize()
    assert_answers("bad record behind the count", t, want_all[pick], m=T + 5)
    with pytest.raises(PwafError):
        device_call(eng, buf, off, n_rec=T + 6)


# ---- re-entrancy ---------------------------------------------------------------------------------------------
def test_two_calls_in_flight_on_two_streams():
    import torch

    batch, want_all, n_rich = traffic()
    eng = engine()
    buf, rec_off = records()
    g = np.random.default_rng(5)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    picks = [np.where(g.random(20000) < 0.1, g.integers(0, n_rich, 20000), g.integers(n_rich, batch.n, 20000)), g.integers(0, n_rich, 3000), g.integers(0, n_rich, 700)]
    calls = [device_call(eng, buf, rec_off[p], stream=streams[k % 2]) for k, p in enumerate(picks)]  # (the third call follows the first on its stream)
    for s in streams:
        s.synchronize()
    eng.device_status()
    for k, (t, p) in enumerate(zip(calls, picks)):
        assert_answers(f"call {k}", t, want_all[p])


# ---- launch lists --------------------------------------------------------------------------------------------
def test_the_launch_list_is_the_scan_the_unpack_and_a_plain_device_batch():
    import torch

    batch, want_all, n_rich = traffic()
    eng = engine()
    buf, rec_off = records()
    pick = np.random.default_rng(6).integers(0, n_rich, 1000)
    want = want_all[pick]

    def launches(call):
        eng.set_profiling(1)
        call()
        torch.cuda.synchronize()
        names = [k[0] for k in eng.kernel_times()]
        eng.set_profiling(0)
        return names

    db = DeviceBatch(batch.take(pick))
    plain = launches(lambda: eng.evaluate_device(db))
    got = {}
    new = launches(lambda: got.update(device_call(eng, buf, rec_off[pick])))
    assert_answers("profiled", got, want)
    host = launches(lambda: eng.evaluate_records(buf, rec_off[pick]))
    assert new[:4] == SCAN_NAMES + ["unpack_records_kernel"], new
    assert new[4:] == plain and len(plain) > 0, (new, plain)
    assert not set(SCAN_NAMES) & set(plain) and not set(SCAN_NAMES) & set(host) and len(host) > 0
