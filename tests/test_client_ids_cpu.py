"""pwaf_client_ids in HOST mode and pwaf_client_id_one (no GPU, no HIP call): the captcha client id of a request,
base64url_nopad(SHA-256(ip octets || user_agent || host)) (the reference's generate_captcha_client_id, pingoo/captcha.rs:409-421), against
Python's own hashlib and base64: three fixed vectors, every message length around the padding edges in both address families, every split
of a payload between the two strings, the ignored bytes of an IPv4 row, slab views, list shapes against a canary, every refusal; and
csrc/clientid.h alone under AddressSanitizer + UBSan as a stand-alone program (tests/client_id_host.cpp) over exact-size heap blocks."""
import base64
import ctypes as C
import functools
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

from pingoo_amd import Request, RequestBatch, _abi, client_ids, generate_captcha_client_id
from pingoo_amd.engine import PwafError, RuleEngine, lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "client_id_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "pingoo_amd", "csrc", "clientid.h"), os.path.join(ROOT, "pingoo_amd", "csrc", "service.h"), os.path.join(ROOT, "include", "pwaf.h")]
UA, HOST = 4, 0  # PWAF_FIELD_USER_AGENT, PWAF_FIELD_HOST

VECTORS = [("97.98.99.100", b"", b"", "iNQmb9TmM40TuEX88olXnSCciXgjuSF9o-Fhk28DFYk"),
           ("203.0.113.7", b"Mozilla/5.0 (X11; Linux x86_64)", b"example.com", "4ZIHo4_k0ldsaHMLWkhLC7AZU6ApVEftf_XNsDldl4g"),
           ("2001:db8::1", b"curl/8.5.0", b"a.example.org", "5BxiJXSoCiYwKna8Xl8XShEjPsLVs7FYDIsjU9rnYaU")]


# ---- the oracle: Python's own ---------------------------------------------------------------------------------
def oracle(ip: bytes, ua: bytes, host: bytes) -> str:
    return base64.urlsafe_b64encode(hashlib.sha256(ip + ua + host).digest()).rstrip(b"=").decode()


def batch_oracle(batch):
    """the id of every request of a RequestBatch, from its columns (a nonzero ip_is_v6 means all 16 octets)"""
    uo, ho = batch.offsets[UA].astype(np.int64), batch.offsets[HOST].astype(np.int64)
    return [oracle(batch.ip[i].tobytes()[:16 if batch.ip_is_v6[i] else 4], batch.data[UA][uo[i]:uo[i + 1]].tobytes(), batch.data[HOST][ho[i]:ho[i + 1]].tobytes())
            for i in range(batch.n)]


def request(ip, ua, host):
    return Request(host=host, url=b"/u", path=b"/p", method=b"GET", user_agent=ua, ip=ip)


def noise(rng, k):
    return bytes(rng.getrandbits(8) for _ in range(k))


@functools.lru_cache(maxsize=None)
def length_sweep():
    """Every total message length 4..200 for IPv4 and 16..200 for IPv6 (the padding edges 55/56/63/64/65 and 119/120/128 in both families),
    about two thirds of the payload in the User-Agent: neighbouring requests have different block counts -> (batch, ids)"""
    rng = random.Random(409)
    reqs = []
    for ip, ip_len in (("198.51.100.23", 4), ("2001:db8:0:7::9", 16)):
        for total in range(ip_len, 201):
            ua_len = (total - ip_len) * 2 // 3
            reqs.append(request(ip, noise(rng, ua_len), noise(rng, total - ip_len - ua_len)))
    batch = RequestBatch.from_requests(reqs)
    ids = batch_oracle(batch)
    assert len(ids) == 197 + 185 and len(set(ids)) == len(ids)
    return batch, ids


def aligned4(nbytes, fill):
    raw = np.full(nbytes + 4, fill, dtype=np.uint8)
    at = -raw.ctypes.data % 4
    return raw[at:at + nbytes]


def raw_call(st, idx=None, n_idx=None, idx_cap=None, room=None, out="own", idx_ptr="own", n_ptr="own"):
    """pwaf_client_ids as it is, into `room` entries pre-filled with 0x5A -> (rc, out as a (room, 44) uint8 array); every argument can be bent"""
    if idx is not None:
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
    idx_cap = (0 if idx is None else len(idx)) if idx_cap is None else idx_cap
    n_ref = None if n_idx is None else np.array([n_idx], dtype=np.uint32)
    room = (idx_cap if idx is not None else (st.n if st is not None else 0)) + 2 if room is None else room
    buf = aligned4(44 * room, 0x5A)
    rc = lib().pwaf_client_ids(C.byref(st) if st is not None else None, (None if idx is None else idx.ctypes.data) if idx_ptr == "own" else idx_ptr, idx_cap,
                               (None if n_ref is None else n_ref.ctypes.data) if n_ptr == "own" else n_ptr, buf.ctypes.data if out == "own" else out, None)
    return rc, buf.reshape(room, 44)


def text(row):
    return row.tobytes().split(b"\0", 1)[0].decode("ascii")


# ---- layout, vectors --------------------------------------------------------------------------------------------
def test_client_id_layout_against_c_compiler(tmp_path):
    prog = tmp_path / "sizes.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pwaf.h"\nint main(void){printf("%zu %zu\\n",sizeof(pwaf_client_id),offsetof(pwaf_client_id,text));return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_abi.ClientId), _abi.ClientId.text.offset] == [44, 0]
    assert _abi.ABI_VERSION == 4 and lib().pwaf_abi_version() == 4


def test_the_three_fixed_vectors_pin_the_order_and_the_alphabet():
    assert any("-" in v[3] for v in VECTORS) and any("_" in v[3] for v in VECTORS)
    for ip, ua, host, want in VECTORS:
        import ipaddress

        assert oracle(ipaddress.ip_address(ip).packed, ua, host) == want
        assert generate_captcha_client_id(ip, ua, host) == want
        assert generate_captcha_client_id(ipaddress.ip_address(ip), ua.decode(), host.decode()) == want
    batch = RequestBatch.from_requests([request(ip, ua, host) for ip, ua, host, _ in VECTORS])
    assert client_ids(batch) == [v[3] for v in VECTORS]
    assert RuleEngine.client_ids(None, batch, idx=[2, 0]) == [VECTORS[2][3], VECTORS[0][3]]  # the method needs nothing of the engine


# ---- message shapes -------------------------------------------------------------------------------------------------
def test_every_message_length_around_the_padding_edges_in_both_families():
    batch, want = length_sweep()
    assert client_ids(batch) == want
    uo, ho = batch.offsets[UA], batch.offsets[HOST]
    for i in range(batch.n):  # pwaf_client_id_one
        ip = batch.ip[i].tobytes()
        import ipaddress

        addr = ipaddress.ip_address(ip if batch.ip_is_v6[i] else ip[:4])
        assert generate_captcha_client_id(addr, batch.data[UA][uo[i]:uo[i + 1]].tobytes(), batch.data[HOST][ho[i]:ho[i + 1]].tobytes()) == want[i], i


def test_every_split_of_a_payload_between_user_agent_and_host():
    payload = noise(random.Random(70), 70)
    for ip in ("192.0.2.1", "2001:db8::2"):
        batch = RequestBatch.from_requests([request(ip, payload[:k], payload[k:]) for k in range(71)])
        got = client_ids(batch)
        assert got == batch_oracle(batch)
        assert len(set(got)) == 1, "the id depends on the concatenation alone"


def test_long_values():
    rng = random.Random(3)
    batch = RequestBatch.from_requests([request("10.1.2.3", noise(rng, 40000), noise(rng, 300)), request("::1", b"", noise(rng, 70000)), request("10.0.0.1", b"x", b"")])
    assert client_ids(batch) == batch_oracle(batch)


def test_ipv4_rows_ignore_bytes_4_to_15_and_any_nonzero_family_byte_means_v6():
    batch, want = length_sweep()
    ip = batch.ip.copy()
    v4 = np.nonzero(batch.ip_is_v6 == 0)[0]
    ip[v4, 4:] = np.random.default_rng(1).integers(1, 256, (len(v4), 12), dtype=np.uint8)
    dirty = RequestBatch(batch.data, batch.offsets, ip, batch.ip_is_v6, batch.port, batch.flags)
    assert client_ids(dirty) == want, "garbage behind an IPv4 address changed its id"
    fam = np.where(np.arange(batch.n) % 2 == 0, 2, 255).astype(np.uint8)
    six = RequestBatch(batch.data, batch.offsets, ip, fam, batch.port, batch.flags)
    got = client_ids(six)
    assert got == batch_oracle(six) and all(g != w for g, w in zip(got[:len(v4)], want))


def test_a_slab_view_whose_offsets_begin_above_zero():
    batch, want = length_sweep()
    lo, hi = 61, 333
    view = batch.view(lo, hi)
    assert int(view.offsets[UA][0]) > 0 and int(view.offsets[HOST][0]) > 0
    assert client_ids(view) == want[lo:hi]
    assert client_ids(view, idx=[0, hi - lo - 1, hi - lo]) == [want[lo], want[hi - 1], ""], "the slab's n bounds the indices, not the arenas"


# ---- lists ------------------------------------------------------------------------------------------------------
def test_lists_with_duplicates_out_of_range_entries_and_the_length_word_against_a_canary():
    batch, want = length_sweep()
    n = batch.n
    st = batch.as_struct()
    idx = np.array([5, 5, n - 1, n, 0, 0xFFFFFFFF, 77, 5, n + 1, 120], dtype=np.uint32)
    for n_idx in (None, 0, 1, len(idx), len(idx) + 5):
        m = len(idx) if n_idx is None else min(n_idx, len(idx))
        rc, out = raw_call(st, idx, n_idx=n_idx, room=len(idx) + 3)
        assert rc == 0
        for j in range(m):
            if idx[j] < n:
                assert text(out[j]) == want[idx[j]] and out[j][43] == 0, (n_idx, j)
            else:
                assert not out[j].any(), "an entry that names no request is 44 zero bytes"
        assert (out[m:] == 0x5A).all(), f"n_idx {n_idx}: written at or beyond out + m"
        assert client_ids(batch, idx, n_idx=n_idx) == [want[i] if i < n else "" for i in idx[:m]]
    rc, out = raw_call(st, room=n + 3)  # idx == NULL: every request, and the canary behind out + n
    assert rc == 0 and [text(r) for r in out[:n]] == want and (out[n:] == 0x5A).all()
    rc, out = raw_call(st, idx, idx_cap=0, room=4)  # a list without room for an entry
    assert rc == 0 and (out == 0x5A).all()
    assert client_ids(batch, np.zeros(0, dtype=np.uint32)) == []
    empty = RequestBatch.from_requests([])
    assert client_ids(empty) == [] and client_ids(empty, [0, 1]) == ["", ""]


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_every_invalid_argument_is_refused_before_anything_is_written():
    batch, _ = length_sweep()
    idx = np.arange(10, dtype=np.uint32)
    one = np.array([3], dtype=np.uint32)
    good = batch.as_struct

    def bent(**kw):
        st = good()
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def no_column(f, part):
        st = good()
        setattr(st.field[f], part, None)
        return st

    spare = aligned4(44 * 16 + 8, 0x5A)
    cases = [
        ("NULL in", dict(st=None, idx=idx)),
        ("NULL out", dict(st=good(), idx=idx, out=None)),
        ("struct_size", dict(st=bent(struct_size=C.sizeof(_abi.Batch) - 8), idx=idx)),
        ("memory", dict(st=bent(memory=2), idx=idx)),
        ("NULL idx with idx_cap != 0", dict(st=good(), idx=idx, idx_ptr=None)),
        ("NULL idx with n_idx", dict(st=good(), idx=None, n_ptr=one.ctypes.data)),
        ("out not 4-byte aligned", dict(st=good(), idx=idx, out=spare.ctypes.data + 2)),
        ("NULL ip", dict(st=bent(ip=None), idx=idx)),
        ("NULL ip_is_v6", dict(st=bent(ip_is_v6=None), idx=idx)),
        ("NULL User-Agent data", dict(st=no_column(UA, "data"), idx=idx)),
        ("NULL User-Agent offsets", dict(st=no_column(UA, "offsets"), idx=idx)),
        ("NULL host data", dict(st=no_column(HOST, "data"), idx=idx)),
        ("NULL host offsets", dict(st=no_column(HOST, "offsets"), idx=idx)),
    ]
    for what, kw in cases:
        rc, out = raw_call(kw.pop("st"), kw.pop("idx"), room=16 if "NULL idx with n_idx" != what else batch.n + 2, **kw)
        assert rc == _abi.E_INVALID_ARG, what
        assert lib().pwaf_last_error(), what
        assert (out == 0x5A).all(), what
    assert (spare == 0x5A).all()
    # with n == 0 the columns are not looked at
    st = RequestBatch.from_requests([]).as_struct()
    st.ip = st.ip_is_v6 = None
    st.field[UA].data = st.field[HOST].offsets = None
    rc, out = raw_call(st, [0], room=3)
    assert rc == 0 and not out[0].any() and (out[1:] == 0x5A).all()


def test_decreasing_offsets_of_a_selected_request_refuse_the_call_with_out_untouched():
    batch, want = length_sweep()
    for f in (UA, HOST):
        o = batch.offsets[f].copy()
        o[21] = o[20] - 1  # request 20's value ends before it begins
        offsets = list(batch.offsets)
        offsets[f] = o
        broken = RequestBatch(batch.data, offsets, batch.ip, batch.ip_is_v6, batch.port, batch.flags)
        st = broken.as_struct()
        rc, out = raw_call(st, [3, 4, 20, 5])
        assert rc == _abi.E_BATCH and b"entry 2" in lib().pwaf_last_error()
        assert (out == 0x5A).all(), "nothing is written for a refused call"
        rc, out = raw_call(st)
        assert rc == _abi.E_BATCH and b"entry 20" in lib().pwaf_last_error() and (out == 0x5A).all()
        rc, out = raw_call(st, [3, 4, 19, 22])  # requests that are not selected are not looked at
        assert rc == 0 and [text(r) for r in out[:4]] == [want[3], want[4], want[19], want[22]]
        with pytest.raises(PwafError):
            client_ids(broken, [20])


def test_the_other_columns_of_the_batch_may_be_null():
    batch, want = length_sweep()
    st = batch.as_struct()
    for f in (1, 2, 3):  # url, path, method
        st.field[f].data = st.field[f].offsets = None
    st.port = st.flags = st.asn = st.country = None
    rc, out = raw_call(st)
    assert rc == 0 and [text(r) for r in out[:batch.n]] == want


# ---- the shared header under the sanitizers -------------------------------------------------------------------------
def test_the_shared_header_under_asan_and_ubsan_reads_no_byte_outside_a_value():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "client_id_host")
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                        os.path.join(ROOT, "include"), SRC, "-o", exe], check=True)
    batch, want = length_sweep()
    uo, ho = batch.offsets[UA], batch.offsets[HOST]
    hexed = lambda b: b.hex() or "-"  # noqa: E731
    lines = [f"{int(batch.ip_is_v6[i])} {batch.ip[i].tobytes().hex()} {hexed(batch.data[UA][uo[i]:uo[i + 1]].tobytes())} {hexed(batch.data[HOST][ho[i]:ho[i + 1]].tobytes())}"
             for i in range(batch.n)]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.split() == want
