"""pwaf_export_records on the device (pack_records_kernel): the records it writes for a list of requests equal, entry by entry, what the
HOST mode of the same call writes (tests/test_export_records_cpu.py holds that one against RequestBatch.to_records); overflow against a
canary; an out-of-range index; the chain evaluate_device -> export_records -> evaluate_records on one stream without a synchronisation in
between; and the engine's launch list, which an export does not change. Small batches: every case is a few launches."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from oracle import pyoracle
from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.engine import DeviceBatch, RuleEngine, export_records, export_stats, lib
from test_records_cpu import random_batch

pytestmark = pytest.mark.gpu
NONE = _abi.RECORD_NONE
B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
CANARY = 1 << 16


def record_at(buf, off):
    size = int(np.frombuffer(buf[off:off + 4].tobytes(), np.uint32)[0])
    return buf[off:off + size].tobytes()


def device_call(db, names, idx, n_idx=None, cap=0, room=None):
    """pwaf_export_records in DEVICE mode into a buffer of `room` bytes filled with 0xC3, of which the call may use `cap`
    -> (buf, rec_off, stats dict) on the host after one synchronisation; rec_off is pre-filled with 0x5A5A5A5A."""
    import torch

    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    d_idx = torch.from_numpy(idx.view(np.int32).copy()).to(db.device)
    d_n = None if n_idx is None else torch.tensor([n_idx], dtype=torch.int32, device=db.device)
    room = cap if room is None else room
    d_buf = torch.full((max(16, room),), 0xC3, dtype=torch.uint8, device=db.device)
    d_off = torch.full((max(1, len(idx)),), 0x5A5A5A5A, dtype=torch.int32, device=db.device)
    d_stats = torch.full((16,), 0x77, dtype=torch.uint8, device=db.device)
    st = db.as_struct(names)
    rc = lib().pwaf_export_records(C.byref(st), d_idx.data_ptr() if len(idx) else None, len(idx), None if d_n is None else d_n.data_ptr(), d_buf.data_ptr(), cap,
                                   d_off.data_ptr(), d_stats.data_ptr(), C.c_void_p(torch.cuda.current_stream(db.device).cuda_stream))
    assert rc == 0, lib().pwaf_last_error()
    torch.cuda.synchronize()
    return d_buf.cpu().numpy(), d_off.cpu().numpy().view(np.uint32), export_stats(d_stats)


def host_records(batch, names, idx, n_idx=None):
    """the HOST mode's answer for the same arguments -> (one record's bytes per list entry, None where it has none; stats)"""
    buf, rec_off, stats = export_records(batch, idx, n_idx=n_idx, header_names=names)
    return [None if o == NONE else record_at(buf, int(o)) for o in rec_off[:stats["n_selected"]]], stats


def assert_device_equals_host(label, batch, db, names, idx, n_idx=None):
    want, hstats = host_records(batch, names, idx, n_idx)
    need = hstats["bytes_needed"]
    buf, rec_off, stats = device_call(db, names, idx, n_idx, cap=need, room=need + CANARY)
    assert stats == hstats, label
    m = stats["n_selected"]
    assert (rec_off[m:len(idx)] == 0x5A5A5A5A).all(), f"{label}: entries past the list are not written"
    spans = []
    for j, w in enumerate(want):
        if w is None:
            assert rec_off[j] == NONE, (label, j)
            continue
        assert rec_off[j] != NONE and rec_off[j] % 16 == 0 and int(rec_off[j]) + len(w) <= need, (label, j)
        assert record_at(buf, int(rec_off[j])) == w, f"{label}: list entry {j} (request {idx[j]}) differs from the HOST mode's record"
        spans.append((int(rec_off[j]), int(rec_off[j]) + len(w)))
    spans.sort()
    assert not spans or (spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == need), f"{label}: holes or overlaps"
    assert (buf[need:] == 0xC3).all(), f"{label}: written beyond buf_cap"
    return stats


@functools.lru_cache(maxsize=None)
def case(n_hdr, geo, n=300):
    import torch  # noqa: F401

    batch, names = random_batch(random.Random(40 + n_hdr * 2 + geo), n, n_hdr, geo)
    return batch, names, DeviceBatch(batch)


# ---- device equals host --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hdr,geo", [(0, False), (0, True), (3, False), (3, True), (64, False), (64, True)])
def test_device_records_equal_the_host_modes(n_hdr, geo):
    batch, names, db = case(n_hdr, geo, 200 if n_hdr == 64 else 400)
    g = np.random.default_rng(n_hdr + geo)
    big = max(int(np.diff(batch.offsets[1].astype(np.int64)).max()), int(np.diff(batch.offsets[4].astype(np.int64)).max()))
    assert big >= 32768, "the batch carries values of tens of KiB"
    for k in (0, 1, 63, 64, 65, 4200):  # (4200: 66 workgroups, every request about ten times)
        idx = g.integers(0, batch.n, k).astype(np.uint32)
        stats = assert_device_equals_host(f"{n_hdr} headers geo={geo} list of {k}", batch, db, names, idx)
        assert stats["n_written"] == k
    idx = g.permutation(batch.n).astype(np.uint32)
    for n_idx in (0, 17, batch.n, batch.n + 5):  # the list's length is read on the device; one above the capacity is clamped
        stats = assert_device_equals_host(f"{n_hdr} headers n_idx {n_idx}", batch, db, names, idx, n_idx=n_idx)
        assert stats["n_selected"] == min(n_idx, batch.n)


def test_a_slab_view_and_a_null_header_column():
    batch, names, _ = case(3, True)
    lo, hi = 101, 283
    view = batch.view(lo, hi)
    assert all(int(o[0]) > 0 for o in view.offsets)
    dv = DeviceBatch(view)
    idx = np.random.default_rng(5).integers(0, hi - lo, 500).astype(np.uint32)
    assert_device_equals_host("view", view, dv, names, idx)
    # a name the device batch does not carry: its descriptor stays NULL and reads as "" (the host batch hands an empty column over)
    wider = [names[0], "absent", names[1], names[2]]
    st = dv.as_struct(wider)
    assert not st.headers[1].data and not st.headers[1].offsets
    assert_device_equals_host("NULL header column", view, dv, wider, idx)


# ---- overflow, out of range ----------------------------------------------------------------------------------
def test_overflow_leaves_the_canary_alone_and_the_written_records_whole():
    batch, names, db = case(3, True)
    idx = np.random.default_rng(9).integers(0, batch.n, 1000).astype(np.uint32)
    want, hstats = host_records(batch, names, idx)
    need = hstats["bytes_needed"]
    _, rec_off, stats = device_call(db, names, idx, cap=0, room=CANARY)  # the size query
    assert stats == {"bytes_needed": need, "n_selected": 1000, "n_written": 0} and (rec_off == NONE).all()
    cap = need - 16
    buf, rec_off, stats = device_call(db, names, idx, cap=cap, room=cap + CANARY)
    assert (buf[cap:] == 0xC3).all(), "written at or beyond buf + buf_cap"
    kept = np.nonzero(rec_off != NONE)[0]
    assert stats == {"bytes_needed": need, "n_selected": 1000, "n_written": len(kept)} and 0 < len(kept) < 1000
    used = 0
    for j in kept:
        assert record_at(buf, int(rec_off[j])) == want[j] and int(rec_off[j]) + len(want[j]) <= cap, j
        used += len(want[j])
    assert used == max(int(rec_off[j]) + len(want[j]) for j in kept), "the written records are a prefix of buf without holes"


def test_an_index_equal_to_n_has_no_record():
    batch, names, db = case(0, False)
    idx = np.array([5, batch.n, 6, batch.n, 7], dtype=np.uint32)
    stats = assert_device_equals_host("idx == n", batch, db, names, idx)
    assert stats["n_selected"] == 5 and stats["n_written"] == 3


# ---- chained with an evaluation ------------------------------------------------------------------------------
RULES = [("admin", 'http_request.path.contains("/admin")', [B]), ("bad_ips", 'lists["bad"].contains(client.ip)', [B]),
         ("token", 'http_request.headers["x-token"] == "evil"', [CAP])]
LISTS = {"bad": (_abi.LIST_IP, ["10.9.0.0/16", "2001:db8::/64"])}


@functools.lru_cache(maxsize=None)
def traffic():
    rng = random.Random(77)
    paths = ["/", "/index.html", "/admin/login", "/x/admin", "/static/app.js", "/a" * 300]
    reqs = [Request(host="example.com", path=(p := rng.choice(paths)), url=p + rng.choice(["", "?a=1"]), method=rng.choice(["GET", "POST"]),
                    user_agent=rng.choice(["Mozilla/5.0 (X11)", "curl/8.5.0", ""]), ip=rng.choice(["10.9.3.4", "10.8.3.4", "192.0.2.7", "2001:db8::9", "2001:db9::9"]),
                    remote_port=rng.randint(1, 65535), captcha_verified=rng.random() < 0.3,
                    headers={"x-token": rng.choice(["evil", "fine", ""])} if rng.random() < 0.6 else None) for _ in range(600)]
    batch = RequestBatch.from_requests(reqs)
    return batch, pyoracle.Oracle(RULES, LISTS, None).evaluate(batch)


def test_evaluate_then_export_on_one_stream_without_a_synchronisation_in_between():
    import torch

    batch, want = traffic()
    eng = RuleEngine(RULES, LISTS, None)
    try:
        assert eng.header_names == ["x-token"]
        db = DeviceBatch(batch)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        runs = []
        for _ in range(2):  # the same chain twice back to back, into different buffers
            d_idx, d_nm = torch.zeros(batch.n, dtype=torch.int32, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
            s.wait_stream(torch.cuda.current_stream())  # (the zeroing above ran on torch's stream)
            out = eng.evaluate_device(db, match_idx=d_idx, n_matches=d_nm, stream=s.cuda_stream)
            runs.append((out, d_idx, d_nm) + eng.export_records(db, d_idx, n_idx=d_nm, stream=s.cuda_stream))
        s.synchronize()
        eng.device_status()
        n_flagged = int((want["action"] != 0).sum())
        assert 50 < n_flagged < batch.n - 50 and {int(r) for r in want["rule_idx"][want["action"] != 0]} >= {0, 1, 2}, "every rule decides some request"
        results = []
        for out, d_idx, d_nm, d_buf, d_off, d_stats in runs:
            verdicts = out.cpu().numpy().view(want.dtype).reshape(-1)
            assert (verdicts == want).all()
            stats = export_stats(d_stats)
            k = int(d_nm.item())
            assert stats["n_selected"] == k == n_flagged and stats["n_written"] == k, stats
            match_idx = d_idx.cpu().numpy()[:k]
            buf, rec_off = d_buf.cpu().numpy()[:stats["bytes_needed"]], d_off.cpu().numpy().view(np.uint32)[:k]
            again = eng.evaluate_records(buf, rec_off)  # the exported bytes, fed back to the same engine as records
            assert (again == verdicts[match_idx]).all(), "the records' verdicts differ from the verdicts of the requests they were exported from"
            assert (pyoracle.Oracle(RULES, LISTS, None).evaluate(batch.take(match_idx)) == again).all()
            results.append({int(i): record_at(buf, int(o)) for i, o in zip(match_idx, rec_off)})
        assert results[0] == results[1], "the two chains exported different records"
        href, _ = host_records(batch, eng.header_names, np.array(sorted(results[0]), dtype=np.uint32))
        assert href == [results[0][i] for i in sorted(results[0])]
    finally:
        eng.close()


def test_an_export_does_not_change_the_engines_launch_list():
    import torch

    batch, want = traffic()
    eng = RuleEngine(RULES, LISTS, None)
    try:
        db = DeviceBatch(batch)
        stream = torch.cuda.current_stream().cuda_stream

        def launches():
            eng.set_profiling(1)
            out = eng.evaluate_device(db, stream=stream)
            names = [k[0] for k in eng.kernel_times()]
            eng.set_profiling(0)
            assert (out.cpu().numpy().view(want.dtype).reshape(-1) == want).all()
            return names

        before = launches()
        d_idx = torch.arange(batch.n, dtype=torch.int32, device="cuda:0")
        _, _, d_stats = eng.export_records(db, d_idx, stream=stream)
        after = launches()
        assert export_stats(d_stats)["n_written"] == batch.n
        assert before == after and len(before) > 0 and not any("pack" in k or "export" in k for k in after)
    finally:
        eng.close()
