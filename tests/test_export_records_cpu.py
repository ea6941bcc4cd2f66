"""pwaf_export_records in HOST mode (no GPU, no HIP call): selected requests of a batch come out as the records RequestBatch.to_records
builds for them, byte for byte, through the C ABI; list shapes, slab views, NULL header columns, out-of-range indices, overflow against a
canary and every refusal; and the packing half of csrc/records.h alone under AddressSanitizer + UBSan as a stand-alone program
(tests/records_pack_host.cpp)."""
import ctypes as C
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest

from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.engine import PwafError, export_records, lib
from test_records_cpu import random_batch, value

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "records_pack_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "pingoo_amd", "csrc", "records.h"), os.path.join(ROOT, "pingoo_amd", "csrc", "service.h"), os.path.join(ROOT, "include", "pwaf.h")]
NONE = _abi.RECORD_NONE


def test_export_stats_layout_against_c_compiler(tmp_path):
    prog = tmp_path / "sizes.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pwaf.h"\nint main(void){printf("%zu %zu %zu %zu %u\\n",sizeof(pwaf_export_stats),'
                    'offsetof(pwaf_export_stats,bytes_needed),offsetof(pwaf_export_stats,n_selected),offsetof(pwaf_export_stats,n_written),PWAF_RECORD_NONE);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _abi.ExportStats
    assert got == [C.sizeof(S), S.bytes_needed.offset, S.n_selected.offset, S.n_written.offset, _abi.RECORD_NONE] == [16, 0, 8, 12, 0xFFFFFFFF]
    assert _abi.ABI_VERSION == 4 and lib().pwaf_abi_version() == 4


# ---- helpers ------------------------------------------------------------------------------------------------
def aligned(nbytes, fill=0):
    raw = np.full(nbytes + 16, fill, dtype=np.uint8)
    at = -raw.ctypes.data % 16
    return raw[at:at + nbytes]


def raw_call(st, idx, n_idx=None, buf=None, cap=0, idx_cap=None, rec_off=None, stats="own", idx_ptr="own"):
    """pwaf_export_records as it is -> (rc, rec_off, ExportStats); every argument can be bent for the refusal cases."""
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    idx_cap = len(idx) if idx_cap is None else idx_cap
    if rec_off is None:
        rec_off = np.full(max(1, idx_cap), 0x5A5A5A5A, dtype=np.uint32)
    s = _abi.ExportStats(0x7777777777777777, 0x77777777, 0x77777777)
    n_ref = None if n_idx is None else np.array([n_idx], dtype=np.uint32)
    rc = lib().pwaf_export_records(C.byref(st) if st is not None else None, (idx.ctypes.data if len(idx) else None) if idx_ptr == "own" else idx_ptr, idx_cap,
                                   None if n_ref is None else n_ref.ctypes.data, buf if isinstance(buf, (int, type(None))) else buf.ctypes.data, cap,
                                   rec_off.ctypes.data if isinstance(rec_off, np.ndarray) else rec_off, C.addressof(s) if stats == "own" else stats, None)
    return rc, rec_off, s


def record_at(buf, off):
    size = int(np.frombuffer(buf[off:off + 4].tobytes(), np.uint32)[0])
    return buf[off:off + size].tobytes()


def references(batch, names, req):
    """the record RequestBatch builds for each request of `req` (a list of request indices), as bytes"""
    wb, wo = batch.take(np.asarray(req, dtype=np.int64)).to_records(header_names=names)
    return [record_at(wb, int(o)) for o in wo]


def assert_records(buf, rec_off, want, label=""):
    for j, w in enumerate(want):
        assert rec_off[j] != NONE and rec_off[j] % 16 == 0, (label, j)
        assert record_at(buf, int(rec_off[j])) == w, f"{label}: list entry {j} differs from to_records"


# ---- byte parity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hdr,geo", [(0, False), (0, True), (3, False), (3, True), (64, False), (64, True)])
def test_exported_records_equal_to_records_byte_for_byte(n_hdr, geo):
    rng = random.Random(100 + n_hdr * 2 + geo)
    n = 600 if n_hdr == 64 else 1200
    batch, names = random_batch(rng, n, n_hdr, geo)
    g = np.random.default_rng(n_hdr + geo)
    idx = np.concatenate([g.permutation(n), g.integers(0, n, 300)]).astype(np.uint32)  # shuffled, with duplicates
    g.shuffle(idx)
    buf, rec_off, stats = export_records(batch, idx, header_names=names)
    want = references(batch, names, idx)
    if n_hdr == 64:
        nv = [int(np.frombuffer(w[4:6], np.uint16)[0]) for w in want]
        assert max(nv) > 64 and min(nv) < 69, "records on both sides of the 64-lane round of the length prefix"
    assert_records(buf, rec_off, want, f"{n_hdr} headers geo={geo}")
    assert stats == {"bytes_needed": sum(len(w) for w in want), "n_selected": len(idx), "n_written": len(idx)}
    assert len(buf) == stats["bytes_needed"]
    # without holes: the records tile the buffer
    spans = sorted((int(o), int(o) + len(w)) for o, w in zip(rec_off, want))
    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == len(buf)


# ---- shapes -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_batch():
    """90 random requests with three header columns and GeoIP, then an all-empty request and two with values of 15, 16 and 17 bytes"""
    rng = random.Random(5)
    names = ["h0", "h1", "h2"]
    reqs = [Request(host=value(rng), url=value(rng, True), path=value(rng), method=value(rng), user_agent=value(rng), ip=f"10.{rng.randint(0, 255)}.1.2",
                    remote_port=rng.randint(0, 65535), captcha_verified=rng.random() < 0.5, asn=rng.randint(0, 2**32 - 1), country=rng.choice(["FR", "US"]),
                    headers={nm: value(rng) for nm in names if rng.random() < 0.4}) for _ in range(90)]
    reqs += [Request(host=b"", url=b"", path=b"", method=b"", user_agent=b"", ip="10.0.0.1", asn=1, country="FR"),  # all empty: no value bytes
             Request(host=b"h" * 15, url=b"u" * 16, path=b"p" * 17, method=b"", user_agent=b"x", ip="10.0.0.2", asn=2, country="US", headers={"h1": b"v" * 16}),
             Request(host=b"", url=b"u" * 17, path=b"", method=b"m" * 15, user_agent=b"", ip="::1", asn=3, country="KP", headers={"h2": b"w" * 15, "h0": b"z" * 17})]
    batch = RequestBatch.from_requests(reqs, with_geoip=True)
    assert list(batch.headers) == names or sorted(batch.headers) == names
    return batch, names


def test_list_lengths_and_the_length_word():
    batch, names = shape_batch()
    n = batch.n
    st = batch.as_struct(names)
    g = np.random.default_rng(3)
    for idx_cap in (0, 1, 63, 64, 65):
        idx = g.integers(0, n, idx_cap).astype(np.uint32)
        want = references(batch, names, idx) if idx_cap else []
        for n_idx in (None, 0, idx_cap // 2, idx_cap, idx_cap + 1, 0xFFFFFFFF):
            m = idx_cap if n_idx is None else min(n_idx, idx_cap)
            need = sum(len(w) for w in want[:m])
            rc, rec_off, s = raw_call(st, idx, n_idx=n_idx)  # the size query
            assert rc == 0 and (s.bytes_needed, s.n_selected, s.n_written) == (need, m, 0), (idx_cap, n_idx)
            assert (rec_off[:m] == NONE).all() and (rec_off[m:] == 0x5A5A5A5A).all()
            buf = aligned(need + 32, 0xA5)
            rc, rec_off, s = raw_call(st, idx, n_idx=n_idx, buf=buf, cap=need)
            assert rc == 0 and (s.bytes_needed, s.n_selected, s.n_written) == (need, m, m), (idx_cap, n_idx)
            assert_records(buf, rec_off, want[:m], f"idx_cap {idx_cap} n_idx {n_idx}")
            assert (rec_off[m:] == 0x5A5A5A5A).all(), "entries past the list are not written"
            assert (buf[need:] == 0xA5).all()


def test_edge_requests_and_value_lengths_around_a_chunk():
    batch, names = shape_batch()
    n = batch.n
    idx = np.array([0, n - 1, n - 3, n - 2, n - 1, 0], dtype=np.uint32)  # first, last, the all-empty one, lengths 15 / 16 / 17
    buf, rec_off, stats = export_records(batch, idx, header_names=names)
    want = references(batch, names, idx)
    assert_records(buf, rec_off, want)
    assert len(want[2]) == 64 and int(np.frombuffer(want[2][4:6], np.uint16)[0]) == 5, "the all-empty request: head + 5 zero lengths, no value bytes"
    assert want[2][56:] == b"\0" * 8
    assert stats["n_written"] == 6


def test_a_slab_view_whose_offsets_begin_above_zero():
    batch, names = shape_batch()
    lo, hi = 37, 81
    view = batch.view(lo, hi)
    assert all(int(o[0]) > 0 for o in view.offsets)
    idx = np.random.default_rng(8).integers(0, hi - lo, 100).astype(np.uint32)
    buf, rec_off, stats = export_records(view, idx, header_names=names)
    assert_records(buf, rec_off, references(batch, names, idx.astype(np.int64) + lo), "view")
    rc, rec_off, s = raw_call(view.as_struct(names), [hi - lo])  # the slab's n bounds the indices, not the arenas
    assert rc == 0 and rec_off[0] == NONE and s.bytes_needed == 0


def test_a_null_header_descriptor_reads_as_empty():
    batch, names = shape_batch()
    st = batch.as_struct(names)
    st.headers[1].data, st.headers[1].offsets = None, None
    st.headers[2].data = None  # (either pointer NULL)
    less = RequestBatch(batch.data, batch.offsets, batch.ip, batch.ip_is_v6, batch.port, batch.flags, batch.asn, batch.country, {names[0]: batch.headers[names[0]]})
    idx = np.arange(batch.n, dtype=np.uint32)
    want = references(less, names, idx)
    need = sum(len(w) for w in want)
    buf = aligned(need)
    rc, rec_off, s = raw_call(st, idx, buf=buf, cap=need)
    assert rc == 0 and s.bytes_needed == need and s.n_written == batch.n
    assert_records(buf, rec_off, want, "NULL header columns")
    assert need < sum(len(w) for w in references(batch, names, idx)), "the dropped columns carried values"


def test_out_of_range_indices_get_no_record_and_are_not_counted():
    batch, names = shape_batch()
    n = batch.n
    idx = np.array([3, n, 4, n + 1, 0xFFFFFFFF, 5, n], dtype=np.uint32)
    good = [0, 2, 5]
    want = references(batch, names, idx[good])
    need = sum(len(w) for w in want)
    buf = aligned(need)
    rc, rec_off, s = raw_call(batch.as_struct(names), idx, buf=buf, cap=need)
    assert rc == 0 and (s.bytes_needed, s.n_selected, s.n_written) == (need, 7, 3)
    assert (rec_off[[1, 3, 4, 6]] == NONE).all()
    assert_records(buf, rec_off[good], want)
    empty = RequestBatch.from_requests([])
    rc, rec_off, s = raw_call(empty.as_struct(), [0, 1])
    assert rc == 0 and (rec_off == NONE).all() and (s.bytes_needed, s.n_selected, s.n_written) == (0, 2, 0)


# ---- overflow -----------------------------------------------------------------------------------------------
def test_overflow_keeps_the_written_records_intact_and_the_canary_untouched():
    rng = random.Random(21)
    batch, names = random_batch(rng, 400, 3, True)
    idx = np.random.default_rng(2).integers(0, 400, 500).astype(np.uint32)
    st = batch.as_struct(names)
    want = references(batch, names, idx)
    need = sum(len(w) for w in want)
    rc, rec_off, s = raw_call(st, idx, buf=None, cap=0)
    assert rc == 0 and s.bytes_needed == need and s.n_written == 0 and (rec_off == NONE).all()
    rc, rec_off, s = raw_call(st, idx, buf=aligned(16), cap=0)  # a non-NULL buf with buf_cap == 0 is a query too
    assert rc == 0 and s.bytes_needed == need and s.n_written == 0
    for cap, everything in ((need - 16, False), (need, True)):
        buf = aligned(need + 4096, 0xC3)
        rc, rec_off, s = raw_call(st, idx, buf=buf, cap=cap)
        assert rc == 0 and s.bytes_needed == need and s.n_selected == 500
        assert (buf[cap:] == 0xC3).all(), "written at or beyond buf + buf_cap"
        kept = np.nonzero(rec_off != NONE)[0]
        assert s.n_written == len(kept) and (len(kept) == 500) == everything and (everything or len(kept) < 500)
        used = 0
        for j in kept:
            assert record_at(buf, int(rec_off[j])) == want[j], j
            assert int(rec_off[j]) + len(want[j]) <= cap
            used += len(want[j])
        assert used == max(int(rec_off[j]) + len(want[j]) for j in kept), "the written records are a prefix of buf without holes"


# ---- refusals -----------------------------------------------------------------------------------------------
def test_every_invalid_argument_is_refused_before_anything_is_written():
    batch, names = shape_batch()
    idx = np.arange(10, dtype=np.uint32)
    good = lambda: batch.as_struct(names)  # noqa: E731
    buf = aligned(1 << 16, 0xEE)

    def bent(**kw):
        st = good()
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    many = (_abi.StrCol * 121)()
    cases = [
        ("NULL in", dict(st=None, idx=idx)),
        ("NULL rec_off", dict(st=good(), idx=idx, rec_off=0)),
        ("NULL stats", dict(st=good(), idx=idx, stats=None)),
        ("NULL idx with idx_cap > 0", dict(st=good(), idx=idx, idx_ptr=None)),
        ("struct_size", dict(st=bent(struct_size=C.sizeof(_abi.Batch) - 8), idx=idx)),
        ("memory", dict(st=bent(memory=2), idx=idx)),
        ("n_headers above 120", dict(st=bent(n_headers=121, headers=many), idx=idx)),
        ("buf not 16-byte aligned", dict(st=good(), idx=idx, buf=buf.ctypes.data + 8, cap=4096)),
        ("buf NULL with buf_cap != 0", dict(st=good(), idx=idx, buf=None, cap=16)),
        ("buf_cap above 0xFFFFFFF0", dict(st=good(), idx=idx, buf=buf, cap=0xFFFFFFF1)),
    ]
    for what, kw in cases:
        rec_off = kw.pop("rec_off", None)
        if rec_off is None:
            rec_off = np.full(16, 0x5A5A5A5A, dtype=np.uint32)
        rc, rec_off, s = raw_call(kw.pop("st"), kw.pop("idx"), rec_off=rec_off, **kw)
        assert rc == _abi.E_INVALID_ARG, what
        assert lib().pwaf_last_error(), what
        assert (s.bytes_needed, s.n_selected, s.n_written) == (0x7777777777777777, 0x77777777, 0x77777777), what
        assert not isinstance(rec_off, np.ndarray) or (rec_off == 0x5A5A5A5A).all(), what
    assert (buf == 0xEE).all()
    # the largest legal header count passes (all 120 descriptors NULL: every header reads as "")
    ok = (_abi.StrCol * 120)()
    rc, rec_off, s = raw_call(bent(n_headers=120, headers=ok), idx, buf=buf, cap=len(buf))
    assert rc == 0 and s.n_written == 10
    assert_records(buf, rec_off, references(RequestBatch(batch.data, batch.offsets, batch.ip, batch.ip_is_v6, batch.port, batch.flags, batch.asn, batch.country), [], idx))


def test_decreasing_offsets_of_a_selected_request_are_a_malformed_batch():
    batch, names = shape_batch()
    o = batch.offsets[1].copy()
    o[21] = o[20] - 1  # request 20's url ends before it begins
    broken = RequestBatch(batch.data[:1] + [batch.data[1]] + batch.data[2:], batch.offsets[:1] + [o] + batch.offsets[2:], batch.ip, batch.ip_is_v6, batch.port, batch.flags,
                          batch.asn, batch.country, batch.headers)
    st = broken.as_struct(names)
    buf = aligned(1 << 16, 0xEE)
    rc, rec_off, s = raw_call(st, [3, 4, 20, 5], buf=buf, cap=len(buf))
    assert rc == _abi.E_BATCH and b"entry 2" in lib().pwaf_last_error()
    assert (buf == 0xEE).all() and (rec_off == 0x5A5A5A5A).all() and s.n_selected == 0x77777777, "nothing is written for a refused call"
    rc, rec_off, s = raw_call(st, [3, 4, 19, 22], buf=buf, cap=len(buf))  # requests that are not selected are not looked at
    assert rc == 0 and s.n_written == 4
    with pytest.raises(PwafError):
        export_records(broken, np.array([20], dtype=np.uint32), header_names=names)


# ---- the shared header under the sanitizers -----------------------------------------------------------------
def test_packing_half_of_the_shared_header_under_asan_and_ubsan():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "records_pack_host")
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                        os.path.join(ROOT, "include"), SRC, "-o", exe], check=True)
    r = subprocess.run([exe, "20261019", "200"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"ok": True, "rounds": 200}
