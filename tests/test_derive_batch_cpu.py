"""pwaf_derive_batch in HOST mode (no GPU, no HIP call): the derived host, path and User-Agent columns of a raw batch against the oracle's
derive_host / derive_path / derive_user_agent applied request by request (tests/derive_cases.py): the known-answer vectors as one batch, a
mixed batch of about 2000 requests (kept lengths and whitespace runs around 16 and 256, bad bytes, 40 KiB values, URI hosts, every
combination of the present bits, paths), slab views, n == 0, extra == NULL, cap exact and one short against canaries, every refusal, the
Python derive_batch; and csrc/derive.h alone under AddressSanitizer + UBSan as a stand-alone program (tests/derive_host.cpp) over
exact-size heap blocks, which also runs the three scan phases as loops over tiles."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import derive_cases as dc
from pingoo_amd import RequestBatch, _abi, derive_batch, derive_stats
from pingoo_amd.engine import PwafError, RuleEngine, derive_scan_shape, lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "derive_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "pingoo_amd", "csrc", "derive.h"), os.path.join(ROOT, "pingoo_amd", "csrc", "service.h"), os.path.join(ROOT, "include", "pwaf.h")]


def kat_cases():
    d = json.load(open(os.path.join(HERE, "golden", "kat.json")))["derive"]
    enc = lambda s: b"" if s is None else s.encode("latin-1")  # noqa: E731
    raws, want = [], ([], [], [])
    for value, w in d["user_agent"]:
        raws.append(dc.raw(present=dc.HDR_BIT | (dc.UA_BIT if value is not None else 0), ua=enc(value)))
        want[0].append(b"h.example"), want[1].append(b"/p"), want[2].append(enc(w))
    for uri, hdr, w in d["host"]:
        raws.append(dc.raw(present=dc.UA_BIT | (dc.URI_BIT if uri is not None else 0) | (dc.HDR_BIT if hdr is not None else 0), uri=enc(uri), host=enc(hdr)))
        want[0].append(enc(w)), want[1].append(b"/p"), want[2].append(b"agent/1.0")
    for value, w in d["path"]:
        raws.append(dc.raw(path=enc(value)))
        want[0].append(b"h.example"), want[1].append(enc(w)), want[2].append(b"agent/1.0")
    return raws, want


# ---- vectors, the mixed batch -----------------------------------------------------------------------------------------
def test_the_known_answer_vectors_as_one_batch():
    raws, want = kat_cases()
    assert len(raws) >= 15 and dc.oracle(raws) == [list(w) for w in want], "the oracle disagrees with tests/golden/kat.json"
    batch, uri, present = dc.raw_batch(raws)
    rc, out = dc.derive_host_mode(batch, uri, present)
    assert rc == 0, lib().pwaf_last_error()
    dc.check_host_out(want, out, "kat")


def test_struct_layouts_against_c_compiler_and_the_abi_version(tmp_path):
    prog = tmp_path / "sizes.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pwaf.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n",sizeof(pwaf_raw_columns),'
                    'offsetof(pwaf_raw_columns,uri_host),offsetof(pwaf_raw_columns,present),sizeof(pwaf_derived_col),sizeof(pwaf_derive_stats),'
                    'offsetof(pwaf_derive_stats,n),offsetof(pwaf_derive_stats,overflow));return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_abi.RawColumns), _abi.RawColumns.uri_host.offset, _abi.RawColumns.present.offset, C.sizeof(_abi.DerivedCol), C.sizeof(_abi.DeriveStats),
                   _abi.DeriveStats.n.offset, _abi.DeriveStats.overflow.offset] == [32, 8, 24, 24, 32, 24, 28]
    assert _abi.ABI_VERSION == 4 and lib().pwaf_abi_version() == 4
    shape = derive_scan_shape()
    assert shape["tile"] % 64 == 0 and shape["step"] >= 64 and shape["copy_group"] % 64 == 0 and shape["zero3"] == 0
    assert lib().pwaf_derive_scratch_bytes(0) % 16 == 0 and lib().pwaf_derive_scratch_bytes(100000) >= 2 * 4 * 100000


def test_the_mixed_batch_offsets_bytes_and_pads_equal_the_oracles():
    raws = dc.mixed_cases()
    want = dc.oracle(raws)
    assert len(raws) >= 2000
    # the case list holds what it claims to
    assert {len(v) for v in want[2]} >= {0, 1, 255, 256} and max(len(v) for v in want[0] + want[2]) == 256
    assert sum(1 for r in raws if len(r.ua) >= 40 * 1024) >= 3 and any(len(r.ua) >= 40 * 1024 and len(w) == 200 for r, w in zip(raws, want[2]))
    assert {r.present & 7 for r in raws} == set(range(8))
    batch, uri, present = dc.raw_batch(raws)
    rc, out = dc.derive_host_mode(batch, uri, present)
    assert rc == 0, lib().pwaf_last_error()
    dc.check_host_out(want, out, "mixed")


def test_a_slab_view_whose_offsets_begin_above_zero():
    raws = dc.mixed_cases()
    want = dc.oracle(raws)
    batch, uri, present = dc.raw_batch(raws)
    lo, hi = 700, 1903
    view = batch.view(lo, hi)
    assert all(int(view.offsets[f][0]) > 0 for f in dc.FIELDS) and int(uri[1][lo]) > 0
    rc, out = dc.derive_host_mode(view, (uri[0], np.ascontiguousarray(uri[1][lo:hi + 1])), np.ascontiguousarray(present[lo:hi]))
    assert rc == 0, lib().pwaf_last_error()
    dc.check_host_out([w[lo:hi] for w in want], out, "view")


def test_an_empty_batch_writes_offsets_zero_the_pads_and_stats():
    batch, uri, present = dc.raw_batch([])
    rc, out = dc.derive_host_mode(batch, uri, present)
    assert rc == 0, lib().pwaf_last_error()
    dc.check_host_out(([], [], []), out, "n == 0")
    st = batch.as_struct()  # with n == 0 the columns are not looked at
    for f in dc.FIELDS:
        st.field[f].data = st.field[f].offsets = None
    out = dc.HostOut(0, [16, 16, 16])
    assert lib().pwaf_derive_batch(C.byref(st), None, out.cols, out.stats.ctypes.data, None, 0, None) == 0
    dc.check_host_out(([], [], []), out, "n == 0, NULL columns")


def test_without_extra_every_request_has_both_headers_and_no_uri_host():
    raws = [r._replace(present=dc.HDR_BIT | dc.UA_BIT) for r in dc.mixed_cases()[:700]]
    want = dc.oracle(raws)
    batch, uri, _ = dc.raw_batch(raws)
    rc, out = dc.derive_host_mode(batch, extra=None)
    assert rc == 0, lib().pwaf_last_error()
    dc.check_host_out(want, out, "extra == NULL")
    # present without URI hosts: PWAF_RAW_HAS_URI_HOST counts as clear
    bits = np.array([r.present for r in dc.mixed_cases()[:700]], dtype=np.uint8)
    rc, out = dc.derive_host_mode(batch, None, bits)
    assert rc == 0, lib().pwaf_last_error()
    dc.check_host_out(dc.oracle([r._replace(present=int(b) & ~dc.URI_BIT) for r, b in zip(raws, bits)]), out, "no URI column")
    # URI hosts without present bytes: nobody has one
    rc, out = dc.derive_host_mode(batch, uri, None)
    assert rc == 0, lib().pwaf_last_error()
    dc.check_host_out(want, out, "present == NULL")


def test_a_batch_that_keeps_every_byte_of_both_host_sources_fits_the_sum_of_them():
    """Requests that take their host from the URI beside requests that take it from the header, absent values stored empty: the derived
    host column is as large as BOTH raw columns together, so the room that always suffices is their sum + 16, not the larger + 16."""
    raws = [dc.raw(present=7, uri=b"u" * 100, host=b""), dc.raw(present=6, uri=b"", host=b"h" * 100)] * 20 + [dc.raw(present=6, host=b" trimmed ")]
    want = dc.oracle(raws)
    batch, uri, present = dc.raw_batch(raws)
    total = len(b"".join(want[0]))
    assert total == 4000 + 7 and total > max(int(batch.offsets[dc.HOST][-1]), int(uri[1][-1])) + dc.PAD
    rc, out = dc.derive_host_mode(batch, uri, present)  # the documented room: both sources' bytes + 16
    assert rc == 0 and out.stats_dict()["overflow"] == 0 and out.caps[0] == 2000 + 9 + 2000 + dc.PAD
    dc.check_host_out(want, out, "both sources kept")
    derived = derive_batch(batch, uri_host=[r.uri if r.present & dc.URI_BIT else None for r in raws])  # the list form stores an absent value empty
    assert [derived.field_bytes(dc.HOST, i) for i in range(derived.n)] == want[0]
    assert len(derived.data[dc.HOST]) >= total + dc.PAD and not derived.data[dc.HOST][total:total + dc.PAD].any()
    derived = derive_batch(batch, uri_host=uri, present=present)
    assert [derived.field_bytes(dc.HOST, i) for i in range(derived.n)] == want[0]
    rc, out = dc.derive_host_mode(batch, uri, present, caps=[2009 + dc.PAD, out.caps[1], out.caps[2]])  # the larger source + 16 is too little
    assert rc == 0 and out.stats_dict()["overflow"] == 1
    dc.check_host_out(want, out, "the larger source alone")


# ---- cap and overflow -----------------------------------------------------------------------------------------------------
def test_cap_exact_is_complete_and_one_byte_short_sets_the_overflow_bit():
    raws = dc.mixed_cases()[:900]
    want = dc.oracle(raws)
    batch, uri, present = dc.raw_batch(raws)
    exact = [len(b"".join(w)) + dc.PAD for w in want]
    rc, out = dc.derive_host_mode(batch, uri, present, caps=exact)
    assert rc == 0 and out.stats_dict()["overflow"] == 0
    dc.check_host_out(want, out, "cap exact")
    for c in range(3):
        caps = list(exact)
        caps[c] -= 1
        rc, out = dc.derive_host_mode(batch, uri, present, caps=caps)
        assert rc == 0 and out.stats_dict()["overflow"] == 1 << c
        dc.check_host_out(want, out, f"cap one short in column {c}")
    for caps in ([0, 0, 0], [5, 17, 1000]):  # a size query; caps in the middle of the bytes
        rc, out = dc.derive_host_mode(batch, uri, present, caps=caps)
        assert rc == 0 and out.stats_dict()["overflow"] == 7
        dc.check_host_out(want, out, f"caps {caps}")
    st = batch.as_struct()  # cap 0 with NULL data
    out = dc.HostOut(batch.n, [0, 0, 0])
    for c in range(3):
        out.cols[c].data = None
    e = dc.extra_struct(uri, present)
    assert lib().pwaf_derive_batch(C.byref(st), C.byref(e), out.cols, out.stats.ctypes.data, None, 0, None) == 0
    assert out.stats_dict()["bytes"] == [x - dc.PAD for x in exact]


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_every_invalid_argument_is_refused_before_anything_is_written():
    raws = dc.mixed_cases()[:300]
    batch, uri, present = dc.raw_batch(raws)
    e = dc.extra_struct(uri, present)

    def call(st="own", extra="own", out=None, cols="own", stats="own", scratch=None, scratch_bytes=0):
        out = out or dc.HostOut(batch.n, [4096 * 64] * 3)
        own = batch.as_struct()
        rc = lib().pwaf_derive_batch(C.byref(own) if st == "own" else (None if st is None else C.byref(st)), C.byref(e) if extra == "own" else (None if extra is None else C.byref(extra)),
                                     out.cols if cols == "own" else cols, out.stats.ctypes.data if stats == "own" else stats, scratch, scratch_bytes, None)
        return rc, out

    def bent(**kw):
        st = batch.as_struct()
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def no_column(f, part):
        st = batch.as_struct()
        setattr(st.field[f], part, None)
        return st

    def bent_out(c, **kw):
        out = dc.HostOut(batch.n, [4096 * 64] * 3)
        for k, v in kw.items():
            setattr(out.cols[c], k, v(getattr(out.cols[c], k)) if callable(v) else v)
        return out

    bad_extra = dc.extra_struct(uri, present)
    bad_extra.struct_size -= 8
    cases = [("NULL raw", dict(st=None)), ("NULL out", dict(cols=None)), ("NULL stats", dict(stats=None)),
             ("struct_size", dict(st=bent(struct_size=C.sizeof(_abi.Batch) - 8))), ("memory", dict(st=bent(memory=2))),
             ("extra struct_size", dict(extra=bad_extra)), ("too many requests", dict(st=bent(n=0xFFFFFFF0 // 256 + 1))),
             ("stats not 8-byte aligned", dict(stats=dc.aligned(64).ctypes.data + 4))]
    for f in dc.FIELDS:
        cases += [(f"NULL field {f} data", dict(st=no_column(f, "data"))), (f"NULL field {f} offsets", dict(st=no_column(f, "offsets")))]
    for c in range(3):
        cases += [(f"NULL out[{c}].offsets", dict(out=bent_out(c, offsets=None))), (f"NULL out[{c}].data with a cap", dict(out=bent_out(c, data=None))),
                  (f"out[{c}].data misaligned", dict(out=bent_out(c, data=lambda p: p + 8))), (f"out[{c}].offsets misaligned", dict(out=bent_out(c, offsets=lambda p: p + 2)))]
    for what, kw in cases:
        rc, out = call(**kw)
        assert rc == _abi.E_INVALID_ARG, what
        assert lib().pwaf_last_error(), what
        assert out.untouched(), what
    # DEVICE mode's scratch is checked before any HIP call (the block is host memory: a call that went on would fault, not return)
    need = lib().pwaf_derive_scratch_bytes(batch.n)
    block = dc.aligned(need + 64)
    assert need >= 2 * 4 * batch.n and need % 16 == 0
    for what, kw in [("NULL scratch", dict(scratch=None, scratch_bytes=need)), ("scratch not 16-byte aligned", dict(scratch=block.ctypes.data + 8, scratch_bytes=need)),
                     ("scratch one byte too small", dict(scratch=block.ctypes.data, scratch_bytes=need - 1)), ("scratch of no bytes", dict(scratch=block.ctypes.data, scratch_bytes=0))]:
        rc, out = call(st=bent(memory=_abi.MEM_DEVICE), **kw)
        assert rc == _abi.E_INVALID_ARG and b"scratch" in lib().pwaf_last_error(), what
        assert out.untouched() and (block == dc.FILL).all(), what
    rc, out = call(st=bent(port=None, flags=None, ip=None, ip_is_v6=None, asn=None, country=None))  # the other members are not looked at
    assert rc == 0
    dc.check_host_out(dc.oracle(raws), out, "other members NULL")


def test_decreasing_offsets_in_a_column_a_request_reads_refuse_the_call_with_outputs_untouched():
    raws = list(dc.mixed_cases()[:200])
    raws[5] = dc.raw(present=7, uri=b"early.example")  # (the URI hosts' offsets are above 0 where they are bent)
    raws[20] = dc.raw(present=7, uri=b"uri.example", host=b"hdr.example")
    raws[30] = dc.raw(present=dc.HDR_BIT, ua=b"unread")
    batch, uri, present = dc.raw_batch(raws)
    want = dc.oracle(raws)

    def broken(f, i):
        o = batch.offsets[f].copy()
        o[i + 1] = o[i] - 1
        offsets = list(batch.offsets)
        offsets[f] = o
        return RequestBatch(batch.data, offsets, batch.ip, batch.ip_is_v6, batch.port, batch.flags)

    for f, name in ((dc.HOST, b"host"), (dc.PATH, b"path"), (dc.UA, b"User-Agent")):
        rc, out = dc.derive_host_mode(broken(f, 11), uri, present, caps=[1 << 20] * 3)
        assert rc == _abi.E_BATCH and b"request 11" in lib().pwaf_last_error() and name in lib().pwaf_last_error(), lib().pwaf_last_error()
        assert out.untouched(), "nothing is written for a refused call"
    uo = uri[1].copy()
    uo[21] = uo[20] - 1
    rc, out = dc.derive_host_mode(batch, (uri[0], uo), present, caps=[1 << 20] * 3)
    assert rc == _abi.E_BATCH and b"request 20" in lib().pwaf_last_error() and b"URI host" in lib().pwaf_last_error() and out.untouched()
    # a column the request does not read is not checked: the Host header beside a URI host, a User-Agent whose bit is clear
    for b in (broken(dc.HOST, 20), broken(dc.UA, 30)):
        rc, out = dc.derive_host_mode(b, uri, present, caps=[1 << 20] * 3)
        assert rc == 0, lib().pwaf_last_error()
        for c in (0, 2):
            o = out.offsets(c)
            assert [bytes(out.data[c][o[i]:o[i + 1]]) for i in (20, 30)] == [want[c][20], want[c][30]]
    with pytest.raises(PwafError):
        derive_batch(broken(dc.PATH, 3), uri_host=uri, present=present)


# ---- Python ---------------------------------------------------------------------------------------------------------------
def test_python_derive_batch_on_a_request_batch():
    raws = dc.mixed_cases()[:800]
    want = dc.oracle(raws)
    batch, uri, present = dc.raw_batch(raws)
    for derived in (derive_batch(batch, uri_host=uri, present=present), RuleEngine.derive_batch(None, batch, uri_host=uri, present=present),
                    derive_batch(batch, uri_host=[r.uri if r.present & dc.URI_BIT else None for r in raws], present=present)):
        assert isinstance(derived, RequestBatch) and derived.n == batch.n
        for c, f in enumerate(dc.FIELDS):
            assert [derived.field_bytes(f, i) for i in range(derived.n)] == want[c], f
            assert not derived.data[f][int(derived.offsets[f][-1]):][:dc.PAD].any()
        for f in (1, 3):
            assert derived.data[f] is batch.data[f] and derived.offsets[f] is batch.offsets[f], "the other columns are shared"
        assert np.shares_memory(derived.ip, batch.ip) and derived.port is batch.port
    plain = [r._replace(present=dc.HDR_BIT | dc.UA_BIT) for r in raws]
    derived = derive_batch(batch)
    assert [[derived.field_bytes(f, i) for i in range(derived.n)] for f in dc.FIELDS] == dc.oracle(plain)
    hosts = [None if k % 3 else b" from.uri\n" for k in range(len(raws))]  # a list without present bytes: both headers, a URI host where given
    derived = derive_batch(batch, uri_host=hosts)
    assert [derived.field_bytes(0, i) for i in range(derived.n)] == dc.oracle([r._replace(present=6 | (h is not None), uri=h or b"") for r, h in zip(plain, hosts)])[0]
    with pytest.raises(ValueError):
        derive_batch(batch, uri_host=uri)
    assert derive_stats(np.array([1, 2, 3, (5 << 32) | 4], dtype=np.uint64).tobytes()) == {"bytes": [1, 2, 3], "n": 4, "overflow": 5}


# ---- the shared header under the sanitizers ---------------------------------------------------------------------------------
def test_the_shared_header_under_asan_and_ubsan_reads_no_byte_outside_a_value():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "derive_host")
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                        os.path.join(ROOT, "include"), SRC, "-o", exe], check=True)
    hexed = lambda b: b.hex() or "-"  # noqa: E731
    for raws in (dc.mixed_cases(), kat_cases()[0], ()):
        want = dc.oracle(raws)
        lines = [f"{r.present} {hexed(r.host)} {hexed(r.path)} {hexed(r.ua)} {hexed(r.uri)}" for r in raws]
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
        assert r.stdout.split() == [hexed(w[i]) for i in range(len(raws)) for w in want]
