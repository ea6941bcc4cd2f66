"""Request records (include/pwaf.h pwaf_record_head, csrc/records.h) on the CPU: the struct layouts agree between the C compiler and the
ctypes mirror, RequestBatch.to_records() decodes — through the very header pwaf_evaluate_records validates with and unpack_records_kernel
decodes with — to the batch's own columns byte for byte, and every malformed call is refused with the index of the offending record."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

from pingoo_amd import Request, RequestBatch, _abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "records_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "pingoo_amd", "csrc", "records.h"), os.path.join(ROOT, "pingoo_amd", "csrc", "service.h"), os.path.join(ROOT, "include", "pwaf.h")]


def test_record_structs_against_c_compiler(tmp_path):
    prog = tmp_path / "sizes.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pwaf.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",sizeof(pwaf_record_head),'
                    'sizeof(pwaf_completion),offsetof(pwaf_record_head,ip),offsetof(pwaf_record_head,has_geoip),offsetof(pwaf_completion,verdict),'
                    'offsetof(pwaf_completion,status));return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_abi.RecordHead), C.sizeof(_abi.Completion), _abi.RecordHead.ip.offset, _abi.RecordHead.has_geoip.offset, _abi.Completion.verdict.offset,
            _abi.Completion.status.offset]
    assert got == want == [36, 24, 8, 32, 8, 16]
    assert _abi.ABI_VERSION == 4 and _abi.E_BUSY == -8


def host_tool():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "records_host")
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), SRC, "-o", out], check=True)
    return out


def decode(tmp_path, buf, rec_off, n_cols):
    b, o, out = tmp_path / "buf", tmp_path / "off", tmp_path / "out"
    b.write_bytes(np.ascontiguousarray(buf, np.uint8).tobytes())
    o.write_bytes(np.ascontiguousarray(rec_off, np.uint32).tobytes())
    r = subprocess.run([host_tool(), str(b), str(o), str(n_cols), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-1000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    return res, (out.read_bytes() if res["ok"] else None)


def value(rng, big=False):
    k = rng.random()
    if k < 0.2:
        return b""
    if big and k > 0.97:
        return bytes(rng.getrandbits(8) for _ in range(rng.randint(1, 64))) * (65536 // 64)  # up to 64 KiB
    alpha = [b"a", b"/", b"\xc3\xa9", b"\xe2\x82\xac", b"\xff", b"\x80", b"\xc3", b"\xed\xa0\x80", b" ", b"\0"]  # non-ASCII and ill-formed UTF-8
    return b"".join(rng.choice(alpha) for _ in range(rng.randint(1, 40)))


def random_batch(rng, n, n_hdr, geo):
    names = [f"h{k}" for k in range(n_hdr)]
    reqs = []
    for _ in range(n):
        hdrs = {nm: value(rng) for nm in names if rng.random() < 0.3} if n_hdr else None
        kw = dict(asn=rng.randint(0, 2**32 - 1), country=rng.choice(["FR", "US", "KP", "ZZ"])) if geo else {}
        ip = f"{rng.randint(0, 255)}.{rng.randint(0, 255)}.1.2" if rng.random() < 0.7 else f"2001:db8::{rng.randint(0, 65535):x}"
        reqs.append(Request(host=value(rng), url=value(rng, True), path=value(rng), method=value(rng), user_agent=value(rng, True), ip=ip,
                            remote_port=rng.randint(0, 65535), captcha_verified=rng.random() < 0.5, headers=hdrs, **kw))
    return RequestBatch.from_requests(reqs, with_geoip=geo), names


@pytest.mark.parametrize("n_hdr,geo,shuffle", [(0, False, False), (0, True, True), (64, False, True), (64, True, False), (3, True, True)])
def test_records_decode_to_the_batch_columns(tmp_path, n_hdr, geo, shuffle):
    rng = random.Random(n_hdr * 10 + geo * 2 + shuffle)
    n = 2000 if n_hdr != 64 else 600
    batch, names = random_batch(rng, n, n_hdr, geo)
    order = np.random.default_rng(n_hdr).permutation(n) if shuffle else None
    buf, rec_off = batch.to_records(order=order, header_names=names)
    nv = buf[rec_off.astype(np.int64)[:, None] + np.arange(4, 6)].copy().view(np.uint16).ravel()
    if n_hdr:
        assert nv.min() < _abi.N_FIELDS + n_hdr and nv.max() > _abi.N_FIELDS, "some records carry fewer values than the engine has columns"
    perm = np.random.default_rng(1 + n_hdr).permutation(n) if shuffle else np.arange(n)  # a shuffled rec_off: output i = request perm[i]
    n_cols = _abi.N_FIELDS + n_hdr
    res, raw = decode(tmp_path, buf, rec_off[perm], n_cols)
    assert res["ok"] and res["has_geoip"] == int(geo), res
    want = batch.take(perm)
    at = 0
    for f in range(n_cols):
        off = np.frombuffer(raw, np.uint32, n + 1, at)
        at += 4 * (n + 1)
        d, o = (want.data[f], want.offsets[f]) if f < _abi.N_FIELDS else want.headers.get(names[f - _abi.N_FIELDS], (np.zeros(16, np.uint8), np.zeros(n + 1, np.uint32)))
        assert (off == o).all(), f
        assert raw[at: at + int(off[-1])] == d[: int(o[-1])].tobytes(), f
        at += int(off[-1])
    for name, arr, dt in (("ip", want.ip, np.uint8), ("v6", want.ip_is_v6, np.uint8), ("port", want.port, np.uint16), ("flags", want.flags, np.uint8)):
        got = np.frombuffer(raw, dt, arr.size, at)
        at += arr.nbytes
        assert (got == arr.ravel()).all(), name
    asn, cc = np.frombuffer(raw, np.uint32, n, at), np.frombuffer(raw, np.uint16, n, at + 4 * n)
    if geo:
        assert (asn == want.asn).all() and (cc == want.country).all()


def test_validation_refuses_each_malformed_case_with_its_index(tmp_path):
    rng = random.Random(9)
    batch, names = random_batch(rng, 40, 2, True)
    buf, rec_off = batch.to_records(header_names=names)
    n_cols = _abi.N_FIELDS + 2
    res, _ = decode(tmp_path, buf, rec_off, n_cols)
    assert res["ok"]
    assert decode(tmp_path, buf, rec_off[[5, 5, 0]], n_cols)[0]["ok"]  # a record may be used twice, others skipped

    def put(b, i, at, raw):
        b = b.copy()
        b[int(rec_off[i]) + at: int(rec_off[i]) + at + len(raw)] = np.frombuffer(raw, np.uint8)
        return b

    def size_of(i):
        return int(np.frombuffer(buf[int(rec_off[i]):int(rec_off[i]) + 4].tobytes(), np.uint32)[0])

    cases = [
        ("misaligned", buf, np.where(np.arange(40) == 7, rec_off + 4, rec_off), 7, 1),
        ("head past the end", buf[: int(rec_off[39]) + 20], rec_off, 39, 2),
        ("record past the end", buf[: int(rec_off[39]) + size_of(39) - 16], rec_off, 39, 2),
        ("offset past the end", buf, np.where(np.arange(40) == 12, np.uint32(len(buf) + 16), rec_off), 12, 2),
        ("size not a multiple of 16", put(buf, 3, 0, np.uint32(size_of(3) + 4).tobytes()), rec_off, 3, 3),
        ("size below the head", put(buf, 4, 0, np.uint32(32).tobytes()), rec_off, 4, 3),
        ("n_values below 5", put(buf, 6, 4, np.uint16(4).tobytes()), rec_off, 6, 4),
        ("n_values above the columns", put(buf, 8, 4, np.uint16(n_cols + 1).tobytes()), rec_off, 8, 4),
        ("a length overflows size", put(buf, 9, 36, np.uint32(size_of(9)).tobytes()), rec_off, 9, 5),
        ("lengths wrap 32 bits", put(put(buf, 10, 36, np.uint32(0xFFFFFFF0).tobytes()), 10, 40, np.uint32(0x20).tobytes()), rec_off, 10, 5),
        ("has_geoip 2", put(buf, 11, 32, b"\x02"), rec_off, 11, 6),
        ("country not A-Z", put(buf, 13, 28, b"F1"), rec_off, 13, 7),
        ("mixed has_geoip", put(buf, 20, 32, b"\x00"), rec_off, 20, 8),
    ]
    for what, b, off, idx, check in cases:
        res, _ = decode(tmp_path, b, off.astype(np.uint32), n_cols)
        assert not res["ok"] and res["index"] == idx and res["check"] == check, (what, res)


def test_a_column_over_4_gib_is_refused_at_the_record_that_crosses_it(tmp_path):
    # rec_off may name one record many times: a record whose url is 64 KiB, named 65 600 times, makes a url column of 4 GiB + 4 MiB while the
    # buffer stays one record long. Column totals are u32 offsets with PWAF_ARENA_PAD behind them: the 65 536th reference (index 65 535)
    # brings the column to 2^32 bytes, past the limit of 2^32 - 16.
    batch = RequestBatch.from_requests([Request(url=b"u" * 65536)])
    buf, rec_off = batch.to_records()
    res, _ = decode(tmp_path, buf, np.zeros(65600, np.uint32), _abi.N_FIELDS)
    assert not res["ok"] and res["index"] == 65535 and res["check"] == 9, res
