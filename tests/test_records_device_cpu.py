"""The device form of record validation on the CPU (pwaf_evaluate_records_device's three scan launches, csrc/records_scan.hip): the
per-record and per-column arithmetic they run lives in csrc/records.h, and tests/records_scan_host.cpp runs it as loops over tiles against
records::validate and records::column_offsets — as a plain g++ program and a second time under AddressSanitizer + UBSan, the buffer a
heap block of exactly buf_bytes bytes. Every case runs in both builds."""
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest

from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.engine import records_scan_shape
from test_records_cpu import random_batch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "records_scan_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "pingoo_amd", "csrc", "records.h"), os.path.join(ROOT, "pingoo_amd", "csrc", "staging.h"), os.path.join(ROOT, "pingoo_amd", "csrc", "service.h"), os.path.join(ROOT, "include", "pwaf.h")]
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
NONE = _abi.RECORD_NONE


@functools.lru_cache(maxsize=None)
def tool(build):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "records_scan_host_" + build)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *FLAGS[build], "-I", os.path.join(ROOT, "include"), SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(params=["plain", "sanitized"])
def build(request):
    return request.param


def run(build, tmp_path, n_cols, buf, lists, cut=-1):
    """one process: `buf` (its first `cut` bytes), then every (rec_off, n_rec) of `lists` -> one result dict per list"""
    b = tmp_path / "buf"
    b.write_bytes(np.ascontiguousarray(buf, np.uint8).tobytes())
    args = [tool(build), str(n_cols), str(b), str(cut)]
    for k, (off, n_rec) in enumerate(lists):
        o = tmp_path / f"off{k}"
        o.write_bytes(np.ascontiguousarray(off, np.uint32).tobytes())
        args += [str(o), str(-1 if n_rec is None else n_rec)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    res = [json.loads(line) for line in r.stdout.strip().splitlines()]
    assert len(res) == len(lists)
    return res


def sizes():
    """the n of the issue's list, on the real tile and step: 1, 63, 64, 65, T - 1, T, T + 1, 2T + 1 and one above a phase-2 step"""
    s = records_scan_shape()
    T, step = s["tile"], s["step"]
    return T, step, [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, step * T + 1]


def test_the_scan_shape_hook_reports_whole_waves():
    s = records_scan_shape()
    assert s["tile"] >= 64 and s["tile"] % 64 == 0 and s["step"] >= 64 and s["step"] % 64 == 0 and s["zero2"] == 0 and s["zero3"] == 0


@pytest.mark.parametrize("n_hdr,geo", [(0, False), (0, True), (3, False), (3, True), (64, False), (64, True)])
def test_random_record_sets_scan_to_the_host_offsets(build, tmp_path, n_hdr, geo):
    rng = random.Random(500 + 2 * n_hdr + geo)
    nb = 150 if n_hdr == 64 else 400
    batch, names = random_batch(rng, nb, n_hdr, geo)
    buf, rec_off = batch.to_records(header_names=names)
    g = np.random.default_rng(n_hdr + geo)
    T, step, ns = sizes()
    lists = [(rec_off, None), (rec_off[g.permutation(nb)], None)]  # as written, and permuted
    lists += [(rec_off[g.integers(0, nb, n)], None) for n in ns]  # duplicated and skipped
    res = run(build, tmp_path, _abi.N_FIELDS + n_hdr, buf, lists)
    for (off, _), r in zip(lists, res):
        assert r["same"] and r["ok"] and r["ref_ok"], r
        assert r["m"] == r["n"] == len(off) and r["has_geoip"] == int(geo), r


def bad_record_cases(n_cols):
    """(name, check, mutation of a copy of a record: list of (byte offset, bytes)) — every Check code a single record can carry"""
    return [
        ("size not a multiple of 16", 3, lambda size: [(0, np.uint32(size + 4).tobytes())]),
        ("size below the head", 3, lambda size: [(0, np.uint32(32).tobytes())]),
        ("n_values below 5", 4, lambda size: [(4, np.uint16(4).tobytes())]),
        ("n_values above the columns", 4, lambda size: [(4, np.uint16(n_cols + 1).tobytes())]),
        ("a length overflows size", 5, lambda size: [(36, np.uint32(size).tobytes())]),
        ("lengths wrap 32 bits", 5, lambda size: [(36, np.uint32(0xFFFFFFF0).tobytes()), (40, np.uint32(0x20).tobytes())]),
        ("has_geoip 2", 6, lambda size: [(32, b"\x02")]),
        ("country not A-Z", 7, lambda size: [(28, b"F1")]),
        ("mixed has_geoip", 8, lambda size: [(32, b"\x00")]),
    ]


@functools.lru_cache(maxsize=None)
def malformed_set(n_hdr=2):
    """A valid buffer (40 records, n_hdr headers, GeoIP) with one bent copy of record 5 per case appended behind it: a list names a bent
    copy where it wants a bad record and leaves every other record as it was."""
    rng = random.Random(9)
    batch, names = random_batch(rng, 40, n_hdr, True)
    buf, rec_off = batch.to_records(header_names=names)
    n_cols = _abi.N_FIELDS + n_hdr
    o5 = int(rec_off[5])
    size = int(np.frombuffer(buf[o5:o5 + 4].tobytes(), np.uint32)[0])
    parts, at, bad = [buf], len(buf), []
    for name, check, bend in bad_record_cases(n_cols):
        copy = buf[o5:o5 + size].copy()
        for where, raw in bend(size):
            copy[where:where + len(raw)] = np.frombuffer(raw, np.uint8)
        parts.append(copy)
        bad.append((name, check, at))
        at += size
    whole = np.concatenate(parts)
    bad += [("misaligned", 1, o5 + 4), ("PWAF_RECORD_NONE", 1, NONE), ("offset past the end", 2, len(whole) + 16), ("head past the end", 2, len(whole) - 16)]
    return whole, rec_off, n_cols, bad


def test_every_check_is_reported_with_the_host_index(build, tmp_path):
    whole, rec_off, n_cols, bad = malformed_set()
    T, step, _ = sizes()
    n = 2 * T + 1
    g = np.random.default_rng(4)
    places = [0, T // 2 + 3, T - 1, T, n - 1]  # first, mid-tile, a tile's last slot, the next tile's first, last of the call
    lists, want = [], []
    for name, check, at in bad:
        for p in places:
            off = rec_off[g.integers(0, 40, n)].copy()
            off[p] = at
            lists.append((off, None))
            # (a first record without GeoIP is no mixed call by itself: every record after it is)
            want.append((name, p, (1, 8) if check == 8 and p == 0 else (p, check)))
    # two bad records: the lower index is reported, whatever its check
    for (_, c1, at1), (_, c2, at2) in [(bad[0], bad[7]), (bad[7], bad[0]), (bad[9], bad[4]), (bad[8], bad[11])]:
        off = rec_off[g.integers(0, 40, n)].copy()
        off[T + 7], off[T - 2] = at1, at2
        lists.append((off, None))
        want.append(("two bad records", T - 2, (T - 2, c2)))
    res = run(build, tmp_path, n_cols, whole, lists)
    for (name, p, (index, check)), r in zip(want, res):
        assert r["same"] and not r["ok"] and not r["ref_ok"], (name, p, r)
        assert (r["index"], r["check"]) == (r["ref_index"], r["ref_check"]) == (index, check), (name, p, r)


def test_a_truncated_final_record_is_refused_wherever_the_buffer_ends(build, tmp_path):
    whole, rec_off, n_cols, _ = malformed_set()
    last = int(rec_off[39])
    size = int(np.frombuffer(whole[last:last + 4].tobytes(), np.uint32)[0])
    off = rec_off.copy()
    off[[3, 17]] = rec_off[39]  # the first entry that names the cut record is the one reported
    for what, cut in (("inside its head", last + 20), ("inside its lengths", last + 40), ("inside its values", last + size - 16), ("one byte short", last + size - 1)):
        (r,) = run(build, tmp_path, n_cols, whole, [(off, None)], cut=cut)
        assert r["same"] and (r["index"], r["check"]) == (r["ref_index"], r["ref_check"]) == (3, 2), (what, r)
    (r,) = run(build, tmp_path, n_cols, whole, [(off, None)], cut=last + size)
    assert r["same"] and r["ok"], "the buffer that ends with the record is whole"


def test_a_column_over_4_gib_is_found_at_the_host_index(build, tmp_path):
    # one record with a 64 KiB url, named 70 000 times: the url column passes 2^32 - 16 bytes while the buffer stays one record long
    batch = RequestBatch.from_requests([Request(url=b"u" * 65536)])
    buf, rec_off = batch.to_records()
    (r,) = run(build, tmp_path, _abi.N_FIELDS, buf, [(np.zeros(70000, np.uint32), None)])
    assert r["same"] and not r["ok"] and r["check"] == r["ref_check"] == 9 and r["index"] == r["ref_index"], r
    assert 65536 - 64 <= r["ref_index"] <= 65536, "what validate itself reports: entry 65 536 less the head's share"
    (r,) = run(build, tmp_path, _abi.N_FIELDS, buf, [(np.zeros(70000, np.uint32), r["ref_index"])])  # one entry fewer: a valid call
    assert r["same"] and r["ok"], r
    # behind the first phase-2 step: 300 small records in front move the crossing into the second step's tiles
    T, step, _ = sizes()
    batch = RequestBatch.from_requests([Request(url=b"x"), Request(url=b"u" * 65536)])
    buf, rec_off = batch.to_records()
    lead = step * T - 65536 + 300
    (r,) = run(build, tmp_path, _abi.N_FIELDS, buf, [(np.concatenate([np.full(lead, rec_off[0]), np.full(70000, rec_off[1])]), None)])
    assert r["same"] and not r["ok"] and r["check"] == r["ref_check"] == 9 and r["index"] == r["ref_index"], r
    assert r["ref_index"] // T >= step, "the crossing lies behind the first phase-2 step"


def test_the_record_count_cuts_the_call(build, tmp_path):
    whole, rec_off, n_cols, bad = malformed_set()
    T, _, _ = sizes()
    n = T + 40
    off = rec_off[np.random.default_rng(6).integers(0, 40, n)].copy()
    off[T + 5] = bad[0][2]  # a bad record the shorter calls never look at
    cases = [(0, True), (1, True), (T, True), (T + 5, True), (T + 6, False), (n, False), (n + 1, False), (0xFFFFFFFF, False), (None, False)]
    res = run(build, tmp_path, n_cols, whole, [(off, k) for k, _ in cases])
    for (k, ok), r in zip(cases, res):
        assert r["same"] and r["ok"] == ok and r["m"] == (n if k is None else min(k, n)), (k, r)
        assert ok or (r["index"], r["check"]) == (T + 5, bad[0][1]), (k, r)
