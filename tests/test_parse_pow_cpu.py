"""pwaf_parse_pow_bodies in HOST mode and pwaf_parse_pow_body_one against the independent oracle (tests/powbody_oracle.py): every decision
D-B1 to D-B10 of DESIGN.md §5.1.8 by name, the fixed corpus and 20 000 mutated bodies on status, hash and nonce, Python's json on every
body the oracle calls OK, the batch semantics of the HOST mode (offsets that do not begin at 0, lists with duplicates and entries that
name no request, n_idx below idx_cap, n == 0, a cap one byte short, decreasing offsets), every refusal, and csrc/powbody.h alone under
AddressSanitizer + UBSan as a stand-alone program (tools/powbody_host.cpp) over exact-size heap blocks. No GPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import powbody_oracle as O
from pingoo_amd import _abi, body_column, body_stats, parse_pow_bodies, parse_pow_body_one
from pingoo_amd.engine import PwafError, RuleEngine, _aligned_bytes, lib, parse_pow_scan_shape

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(ROOT, "tools", "powbody_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "pingoo_amd", "csrc", "powbody.h"), os.path.join(ROOT, "pingoo_amd", "csrc", "service.h"), os.path.join(ROOT, "include", "pwaf.h")]
N, K, M, U = O.NONE, O.OK, O.MALFORMED, O.UNDECIDED
NAMES = {N: "NONE", K: "OK", M: "MALFORMED", U: "UNDECIDED"}


def host_batch(bodies, idx=None, n_idx=None, cap=None):
    """parse_pow_bodies in HOST mode -> (status list, hash rows as bytes, nonces as bytes per request, stats dict, raw offsets)"""
    status, hashes, (ndata, noff), stats = parse_pow_bodies(list(bodies), idx=idx, n_idx=n_idx, cap=cap)
    st = body_stats(stats)
    nonces = [bytes(ndata[int(noff[i]):int(noff[i + 1])]) for i in range(len(bodies))] if not st["overflow"] else None
    return [int(s) for s in status], [bytes(h) for h in hashes], nonces, st, noff


def assert_agree(label, bodies):
    """the HOST mode over `bodies` as one batch and _one over each equal the oracle on status, hash and nonce"""
    want = [O.decide(b) for b in bodies]
    status, rows, nonces, st, _ = host_batch(bodies)
    for i, (body, w) in enumerate(zip(bodies, want)):
        assert (status[i], rows[i], nonces[i]) == w, f"{label}: HOST mode, body {i} {body[:80]!r}: {NAMES[status[i]]}, the oracle says {NAMES[w[0]]}"
    for i in range(0, len(bodies), max(1, len(bodies) // 4000)):  # (_one costs a Python call a body)
        assert parse_pow_body_one(bodies[i]) == want[i], f"{label}: _one, body {i} {bodies[i][:80]!r}"
    assert st == dict(O.expect_batch(bodies)[3], overflow=0)


# ---- the constants and the shape -----------------------------------------------------------------------------------------------------------
def test_the_constants_are_the_header_s(tmp_path):
    prog = tmp_path / "body.c"
    prog.write_text('#include <stdio.h>\n#include "pwaf.h"\nint main(void){printf("%u %u %u %u %u %zu\\n",PWAF_BODY_NONE,PWAF_BODY_OK,PWAF_BODY_MALFORMED,PWAF_BODY_UNDECIDED,'
                    "PWAF_POW_BODY_MAX_BYTES,sizeof(pwaf_body_stats));return 0;}\n")
    exe = tmp_path / "body"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [_abi.BODY_NONE, _abi.BODY_OK, _abi.BODY_MALFORMED, _abi.BODY_UNDECIDED, _abi.POW_BODY_MAX_BYTES, C.sizeof(_abi.BodyStats)] == [N, K, M, U, O.MAX_BYTES, 32]
    shape = parse_pow_scan_shape()
    assert shape["tile"] % 64 == 0 and shape["copy_group"] == shape["tile"] and shape["step"] >= 64
    assert lib().pwaf_parse_pow_bodies_scratch_bytes(0) % 16 == 0 and lib().pwaf_parse_pow_bodies_scratch_bytes(1000) >= 4 * 1000
    assert lib().pwaf_parse_pow_scan_shape(None) == _abi.E_INVALID_ARG


# ---- the decisions ---------------------------------------------------------------------------------------------------------------------------
CASES = O.fixed_corpus()


def test_every_decision_has_cases_of_its_own():
    for d in range(1, 11):
        assert any(label.startswith(f"D-B{d} ") for label, _, _ in CASES), f"D-B{d} has no named case"
    statuses = {(label.split()[0], st) for label, _, st in CASES}
    for d, st in ((1, U), (2, M), (2, U), (3, M), (4, M), (4, U), (5, U), (5, M), (6, M), (7, M), (8, U), (9, M), (10, K)):
        assert (f"D-B{d}", st) in statuses, f"D-B{d} has no {NAMES[st]} case"


@pytest.mark.parametrize("decision", ["genuine"] + [f"D-B{d}" for d in range(1, 11)])
def test_decision(decision):
    """each named case: the status written by hand, the oracle's and the library's (HOST mode and _one) are one"""
    cases = [c for c in CASES if c[0].split()[0] == decision]
    assert cases
    for label, body, status in cases:
        want = O.decide(body)
        assert want[0] == status, f"{label}: the oracle says {NAMES[want[0]]}, the case was written for {NAMES[status]}"
        assert parse_pow_body_one(body) == want, f"{label}: {body[:100]!r}"
        if status != K:
            assert want[1:] == (O.ZERO, b"")
    assert_agree(decision, [body for _, body, _ in cases])


def test_the_fixed_corpus_as_one_batch():
    assert_agree("the fixed corpus", [body for _, body, _ in CASES])


def test_20000_mutated_bodies():
    bodies = O.mutated_corpus()
    assert len(bodies) == 20000
    statuses = [O.decide(b)[0] for b in bodies]
    ok, decided = statuses.count(K), statuses.count(K) + statuses.count(M)
    assert decided * 2 >= len(bodies) and ok * 10 >= len(bodies) and statuses.count(U) * 20 >= len(bodies), (ok, decided, len(bodies))
    assert_agree("the mutated corpus", list(bodies))


def test_python_s_json_reads_every_ok_body_to_the_same_members():
    bodies = [body for _, body, _ in CASES] + list(O.mutated_corpus())
    n_ok = 0
    for body in bodies:
        status, row, nonce = O.decide(body)
        if status != K:
            continue
        n_ok += 1
        got = json.loads(body.decode("ascii"))
        assert set(got) == {"hash", "nonce"} and bytes.fromhex(got["hash"]) == row and got["nonce"].encode("ascii") == nonce, body
    assert n_ok >= 2000


# ---- the HOST mode's batch semantics -----------------------------------------------------------------------------------------------------
def sample(count=40):
    bodies = [b for _, b, _ in CASES[::max(1, len(CASES) // count)]][:count]
    assert {O.decide(b)[0] for b in bodies} == {K, M, U}
    return bodies


def raw_call(bodies, lead=0, idx=None, n_idx=None, cap=None, n=None, canary=8):
    """pwaf_parse_pow_bodies in HOST mode on a column whose offsets begin at `lead`, into outputs with guard regions
    -> (rc, status with guard, hash rows with guard, nonce data with guard, offsets with guard, stats dict)"""
    data, off = O.column(bodies, lead)
    n = len(bodies) if n is None else n
    darr, oarr = np.frombuffer(data, dtype=np.uint8)[:off[-1]].copy(), np.array(off, dtype=np.uint32)  # (no pad: the HOST mode assumes none)
    col, ncol = _abi.StrCol(), _abi.DerivedCol()
    col.data, col.offsets = darr.ctypes.data, oarr.ctypes.data
    m = n if idx is None else (len(idx) if n_idx is None else min(n_idx, len(idx)))
    if cap is None:
        cap = sum(len(x) for x in O.expect_batch(bodies[:n], idx, n_idx)[2]) + _abi.ARENA_PAD
    status = np.full(m + canary, 0x5A, dtype=np.uint8)
    hashes = np.full((n + 1, 32), 0x5A, dtype=np.uint8)
    ndata = _aligned_bytes(cap + canary)
    ndata[:] = 0x5A
    noff = np.full(n + 1 + canary, 0x5A5A5A5A, dtype=np.uint32)
    stats = np.full(5, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    ncol.data, ncol.offsets, ncol.cap = ndata.ctypes.data, noff.ctypes.data, cap
    iarr = None if idx is None else np.array(list(idx) or [0], dtype=np.uint32)
    narr = None if n_idx is None else np.array([n_idx], dtype=np.uint32)
    rc = lib().pwaf_parse_pow_bodies(C.byref(col), n, _abi.MEM_HOST, None if idx is None else iarr.ctypes.data, 0 if idx is None else len(idx), None if narr is None else narr.ctypes.data,
                                     status.ctypes.data, hashes.ctypes.data, C.byref(ncol), stats.ctypes.data, None, 0, None)
    assert stats[4] == 0x5A5A5A5A5A5A5A5A, "written beyond stats + 1"
    return rc, status, hashes, ndata, noff, body_stats(stats[:4].tobytes())


def check_outputs(label, bodies, out, idx=None, n_idx=None, cap=None, canary=8):
    rc, status, hashes, ndata, noff, st = out
    assert rc == 0, (label, lib().pwaf_last_error())
    n = len(bodies)
    want_status, rows, nonces, want_stats = O.expect_batch(bodies, idx, n_idx)
    m = len(want_status)
    assert list(status[:m]) == want_status and (status[m:] == 0x5A).all(), f"{label}: statuses, or a write at or beyond status + m"
    want_rows = np.frombuffer(b"".join(r if r is not None else b"\x5a" * 32 for r in rows), dtype=np.uint8).reshape(n, 32)
    wrong = np.nonzero((hashes[:n] != want_rows).any(axis=1))[0]
    assert not len(wrong), f"{label}: hash row {wrong[:1]} (unselected rows stay as they were)"
    assert (hashes[n] == 0x5A).all(), f"{label}: written beyond the hash rows"
    total = want_stats["nonce_bytes"]
    cap = total + _abi.ARENA_PAD if cap is None else cap
    ends = np.cumsum([0] + [len(x) for x in nonces])
    assert list(noff[:n + 1]) == list(ends) and (noff[n + 1:] == 0x5A5A5A5A).all(), f"{label}: offsets, or a write beyond offsets + n + 1"
    assert st == dict(want_stats, overflow=int(total + _abi.ARENA_PAD > cap)), label
    if not st["overflow"]:
        assert bytes(ndata[:total]) == b"".join(nonces), f"{label}: nonce bytes"
        assert not ndata[total:total + _abi.ARENA_PAD].any(), f"{label}: the pad"
        assert (ndata[total + _abi.ARENA_PAD:] == 0x5A).all(), f"{label}: written beyond the pad"
    assert (ndata[cap:] == 0x5A).all(), f"{label}: written at or beyond cap"


@pytest.mark.parametrize("lead", [0, 1, 7, 16, 1000])
def test_offsets_that_do_not_begin_at_0(lead):
    bodies = sample()
    check_outputs(f"lead {lead}", bodies, raw_call(bodies, lead=lead))


def test_a_list_with_duplicates_and_entries_that_name_no_request():
    bodies = sample()
    n = len(bodies)
    idx = [3, 3, n, 0, 2**32 - 1, n - 1, 3, n + 5, 0]
    check_outputs("the list", bodies, raw_call(bodies, idx=idx), idx=idx)
    every = list(range(n - 1, -1, -1)) * 2
    check_outputs("every request twice, backwards", bodies, raw_call(bodies, idx=every, lead=5), idx=every)


@pytest.mark.parametrize("n_idx", [0, 1, 5, 9, 10, 1000])
def test_n_idx_below_and_above_idx_cap(n_idx):
    bodies = sample()
    idx = [k * 3 % len(bodies) for k in range(9)]
    check_outputs(f"n_idx {n_idx}", bodies, raw_call(bodies, idx=idx, n_idx=n_idx), idx=idx, n_idx=n_idx)


def test_no_request_and_no_entry():
    check_outputs("n == 0", [], raw_call([]))
    check_outputs("n == 0 with a list", [], raw_call([], idx=[0, 1, 7]), idx=[0, 1, 7])
    bodies = sample()
    check_outputs("an empty list", bodies, raw_call(bodies, idx=[1, 2], n_idx=0), idx=[1, 2], n_idx=0)
    status, hashes, (ndata, noff), stats = parse_pow_bodies([])
    assert len(status) == 0 and len(hashes) == 0 and list(noff) == [0] and body_stats(stats)["n"] == 0
    status, _, (_, noff), stats = parse_pow_bodies(bodies, idx=np.zeros(0, dtype=np.uint32))
    assert len(status) == 0 and not noff.any() and body_stats(stats)["n"] == 0


@pytest.mark.parametrize("short", [1, 2, 16, 17])
def test_a_cap_too_small_sets_overflow_and_still_completes_the_offsets(short):
    bodies = sample()
    total = O.expect_batch(bodies)[3]["nonce_bytes"]
    assert total > 17
    cap = total + _abi.ARENA_PAD - short
    out = raw_call(bodies, cap=cap)
    check_outputs(f"cap short by {short}", bodies, out, cap=cap)
    assert out[5]["overflow"] == 1
    check_outputs("cap 0", bodies, raw_call(bodies, cap=0), cap=0)
    exact = raw_call(bodies, cap=total + _abi.ARENA_PAD)
    assert exact[5]["overflow"] == 0


def test_decreasing_offsets_refuse_the_call_before_anything_is_written():
    bodies = sample()
    data, off = body_column(bodies)
    bad = off.copy()
    bad[6] = bad[5] - 1  # request 5's offsets decrease
    with pytest.raises(PwafError) as e:
        parse_pow_bodies((data, bad))
    assert e.value.code == _abi.E_BATCH and "entry 5" in str(e.value)
    with pytest.raises(PwafError) as e:
        parse_pow_bodies((data, bad), idx=np.array([1, 5], dtype=np.uint32))
    assert e.value.code == _abi.E_BATCH and "entry 1 (request 5)" in str(e.value)
    status, _, _, _ = parse_pow_bodies((data, bad), idx=np.array([1, 2, 9], dtype=np.uint32))  # request 5 is not selected
    assert [int(s) for s in status] == [O.decide(bodies[i])[0] for i in (1, 2, 9)]


def test_every_invalid_argument_is_refused():
    bodies = sample(8)
    data, off = body_column(bodies)
    n = len(bodies)
    status, hashes, ndata, noff = np.zeros(n, dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8), _aligned_bytes(4096), np.zeros(n + 1, dtype=np.uint32)
    stats, idx, n_idx = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint32), np.ones(1, dtype=np.uint32)
    scratch = _aligned_bytes(int(lib().pwaf_parse_pow_bodies_scratch_bytes(n)) + 16)

    def call(**change):
        a = dict(bodies=(data.ctypes.data, off.ctypes.data), n=n, memory=_abi.MEM_HOST, idx=None, idx_cap=0, n_idx=None, status=status.ctypes.data, hash=hashes.ctypes.data,
                 nonce=(ndata.ctypes.data, noff.ctypes.data, 4096), stats=stats.ctypes.data, scratch=None, scratch_bytes=0)
        a.update(change)
        col, ncol = _abi.StrCol(), _abi.DerivedCol()
        if a["bodies"] is not None:
            col.data, col.offsets = a["bodies"]
        if a["nonce"] is not None:
            ncol.data, ncol.offsets, ncol.cap = a["nonce"]
        return lib().pwaf_parse_pow_bodies(None if a["bodies"] is None else C.byref(col), a["n"], a["memory"], a["idx"], a["idx_cap"], a["n_idx"], a["status"], a["hash"],
                                           None if a["nonce"] is None else C.byref(ncol), a["stats"], a["scratch"], a["scratch_bytes"], None)

    assert call() == 0
    refused = {
        "NULL bodies": dict(bodies=None), "NULL status": dict(status=None), "NULL hash": dict(hash=None), "NULL nonce": dict(nonce=None), "NULL stats": dict(stats=None),
        "memory 2": dict(memory=2), "memory 0xFFFFFFFF": dict(memory=0xFFFFFFFF),
        "idx NULL with idx_cap": dict(idx_cap=1), "idx NULL with n_idx": dict(n_idx=n_idx.ctypes.data),
        "too many requests": dict(n=0xFFFFFFF0 // 4096 + 1),
        "stats not 8-byte aligned": dict(stats=stats.ctypes.data + 4),
        "NULL bodies data": dict(bodies=(None, off.ctypes.data)), "NULL bodies offsets": dict(bodies=(data.ctypes.data, None)),
        "NULL nonce offsets": dict(nonce=(ndata.ctypes.data, None, 4096)), "NULL nonce data with a cap": dict(nonce=(None, noff.ctypes.data, 16)),
        "nonce data not 16-byte aligned": dict(nonce=(ndata.ctypes.data + 8, noff.ctypes.data, 4000)),
        "nonce offsets not 4-byte aligned": dict(nonce=(ndata.ctypes.data, noff.ctypes.data + 2, 4096)),
        "DEVICE: NULL scratch": dict(memory=_abi.MEM_DEVICE, scratch=None, scratch_bytes=1 << 20),
        "DEVICE: scratch not 16-byte aligned": dict(memory=_abi.MEM_DEVICE, scratch=scratch.ctypes.data + 8, scratch_bytes=len(scratch) - 8),
        "DEVICE: scratch too small": dict(memory=_abi.MEM_DEVICE, scratch=scratch.ctypes.data, scratch_bytes=int(lib().pwaf_parse_pow_bodies_scratch_bytes(n)) - 1),
    }
    for label, change in refused.items():
        assert call(**change) == _abi.E_INVALID_ARG, label
        assert lib().pwaf_last_error()
    assert call(nonce=(None, noff.ctypes.data, 0)) == 0 and list(noff) == list(np.cumsum([0] + [len(O.decide(b)[2]) for b in bodies]))
    # _one
    one = lib().pwaf_parse_pow_body_one
    st, h, at, ln = C.c_uint8(0), (C.c_uint8 * 32)(), C.c_uint32(0), C.c_uint32(0)
    good = (C.c_uint8 * 4).from_buffer_copy(b"{} x")
    assert one(C.addressof(good), 4, C.byref(st), C.addressof(h), C.byref(at), C.byref(ln)) == 0 and st.value == M
    assert one(None, 0, C.byref(st), C.addressof(h), C.byref(at), C.byref(ln)) == 0 and st.value == M
    assert one(None, 1, C.byref(st), C.addressof(h), C.byref(at), C.byref(ln)) == _abi.E_INVALID_ARG
    assert one(C.addressof(good), 4, None, C.addressof(h), C.byref(at), C.byref(ln)) == _abi.E_INVALID_ARG
    assert one(C.addressof(good), 4, C.byref(st), None, C.byref(at), C.byref(ln)) == _abi.E_INVALID_ARG
    assert one(C.addressof(good), 4, C.byref(st), C.addressof(h), None, C.byref(ln)) == _abi.E_INVALID_ARG
    assert one(C.addressof(good), 4, C.byref(st), C.addressof(h), C.byref(at), None) == _abi.E_INVALID_ARG


def test_the_engine_s_method_and_what_verify_pow_takes():
    bodies = sample()
    a = parse_pow_bodies(bodies)
    b = RuleEngine.parse_pow_bodies(None, bodies)
    assert list(a[0]) == list(b[0]) and (a[1] == b[1]).all() and (a[2][1] == b[2][1]).all()
    assert RuleEngine.parse_pow_body_one(None, bodies[0]) == O.decide(bodies[0])
    assert a[1].shape == (len(bodies), 32) and a[1].dtype == np.uint8 and a[2][1].dtype == np.uint32 and len(a[2][1]) == len(bodies) + 1


# ---- the shared header under the sanitizers -----------------------------------------------------------------------------------------
def test_the_shared_header_under_asan_and_ubsan_reads_no_byte_outside_a_body():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "powbody_host")
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                        os.path.join(ROOT, "include"), SRC, "-o", exe], check=True)
    bodies = [body for _, body, _ in CASES] + list(O.mutated_corpus()[:4000])
    r = subprocess.run([exe], input="".join((b.hex() or "-") + "\n" for b in bodies), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    lines = r.stdout.split("\n")
    got = [ln.split() for ln in lines if ln.startswith("R")]
    assert len(got) == len(bodies)
    for body, g in zip(bodies, got):
        st, row, nonce = O.decide(body)
        assert (int(g[1]), bytes.fromhex(g[2]), b"" if g[3] == "-" else bytes.fromhex(g[3])) == (st, row, nonce), body
    want = O.expect_batch(bodies)[3]
    summary = next(ln.split() for ln in lines if ln.startswith("H"))
    assert [int(x) for x in summary[1:]] == [want["n"], want["nonce_bytes"], want["n_ok"], want["n_malformed"], want["n_undecided"]]
