"""Raw requests for pwaf_derive_batch's tests (tests/test_derive_batch_cpu.py, tests/test_gpu_derive_batch.py): the case list of the mixed
batch, the oracle applied request by request (oracle/pyoracle.py's derive_host / derive_path / derive_user_agent, the restatement that
tests/test_abi.py pins with tests/golden/kat.json — never the code under test), and the plumbing that calls pwaf_derive_batch as it is,
into pre-filled blocks with canaries behind every output."""
import ctypes as C
import functools
import random
from typing import NamedTuple

import numpy as np

from oracle import pyoracle
from pingoo_amd import RequestBatch, _abi
from pingoo_amd.engine import lib

HOST, PATH, UA = 0, 2, 4  # PWAF_FIELD_HOST, _PATH, _USER_AGENT
FIELDS = (HOST, PATH, UA)  # pwaf_derive_batch's out[0..2]
URI_BIT, HDR_BIT, UA_BIT = _abi.RAW_HAS_URI_HOST, _abi.RAW_HAS_HOST_HEADER, _abi.RAW_HAS_USER_AGENT
PAD = _abi.ARENA_PAD
FILL, CANARY = 0x5A, 64  # what every output block holds before the call; the bytes behind every output that must keep it


class Raw(NamedTuple):
    present: int
    host: bytes  # the Host header's value
    path: bytes  # uri.path()
    ua: bytes    # the User-Agent header's value
    uri: bytes   # uri.host()


def raw(present=HDR_BIT | UA_BIT, host=b"h.example", path=b"/p", ua=b"agent/1.0", uri=b""):
    return Raw(present, host, path, ua, uri)


def oracle_one(r: Raw):
    """(host, path, user_agent) of one raw request, by the oracle; a value whose present bit is clear does not exist for it"""
    return (pyoracle.derive_host(r.uri if r.present & URI_BIT else None, r.host if r.present & HDR_BIT else None), pyoracle.derive_path(r.path),
            pyoracle.derive_user_agent(r.ua if r.present & UA_BIT else None))


def oracle(raws):
    """-> a list of three lists of bytes: the derived host, path and user_agent of every request"""
    got = [oracle_one(r) for r in raws]
    return [[g[c] for g in got] for c in range(3)]


def column(values, first=0):
    """values back to back behind `first` filler bytes, with the pad -> (data, offsets)"""
    o = np.full(len(values) + 1, first, dtype=np.uint32)
    if values:
        o[1:] += np.cumsum([len(v) for v in values], dtype=np.uint64).astype(np.uint32)
    return np.frombuffer(b"\xEE" * first + b"".join(values) + b"\0" * PAD, dtype=np.uint8).copy(), o


def raw_batch(raws):
    """-> (RequestBatch whose host, path and user_agent columns hold the raw values, (uri data, uri offsets), present)"""
    n = len(raws)
    cols = {HOST: column([r.host for r in raws]), PATH: column([r.path for r in raws]), UA: column([r.ua for r in raws]),
            1: column([b"https://x/u"] * n), 3: column([b"GET"] * n)}
    ip = np.zeros((n, 16), dtype=np.uint8)
    ip[:, 0], ip[:, 3] = 10, 7
    batch = RequestBatch([cols[f][0] for f in range(5)], [cols[f][1] for f in range(5)], ip, np.zeros(n, dtype=np.uint8), np.full(n, 443, dtype=np.uint16),
                         np.zeros(n, dtype=np.uint8))
    return batch, column([r.uri for r in raws]), np.array([r.present for r in raws], dtype=np.uint8)


# ---- the mixed batch ------------------------------------------------------------------------------------------------------------------
BLANKS = b" \t"
RUNS = (0, 1, 15, 16, 17, 300)
KEPT = (0, 1, 255, 256, 257)
BAD = (0x00, 0x1F, 0x7F, 0x80, 0xFF)


def blanks(rng, k):
    return bytes(rng.choice(BLANKS) for _ in range(k))


def text(rng, k):
    """k bytes of header text that begin and end with a byte trim() keeps; blanks inside"""
    if k == 0:
        return b""
    body = bytearray(rng.choice(b"abcxyz0189-._/;()" + BLANKS) for _ in range(k))
    body[0], body[-1] = rng.choice(b"MmCc"), rng.choice(b"0z)")
    return bytes(body)


@functools.lru_cache(maxsize=None)
def mixed_cases():
    """About 2000 raw requests; the header cases stand in the Host header and in the User-Agent alike. -> a tuple of Raw"""
    rng = random.Random(284)
    out = []
    headers = []
    for kept in KEPT:  # kept lengths x whitespace runs at either end
        for lead in RUNS:
            for trail in RUNS:
                headers.append(blanks(rng, lead) + text(rng, kept) + blanks(rng, trail))
    headers += [blanks(rng, k) for k in (1, 15, 16, 17, 33, 300)]  # nothing but whitespace
    for bad in BAD:  # one byte that is not text: first, last, and inside a run that would be trimmed
        b = bytes([bad])
        good = text(rng, 40)
        headers += [b + good, good + b, b, blanks(rng, 3) + b + blanks(rng, 20) + good + blanks(rng, 5), blanks(rng, 2) + good + blanks(rng, 18) + b + blanks(rng, 21),
                    good[:20] + b + good[20:], blanks(rng, 17) + text(rng, 255) + b + blanks(rng, 16)]
    big = 40 * 1024
    for kept in (200, 300):  # 40 KiB values: only the ends are looked at
        lead = (big - kept) // 2
        headers.append(blanks(rng, lead) + text(rng, kept) + blanks(rng, big - kept - lead))
    headers.append(text(rng, big))
    for k, h in enumerate(headers):
        out.append(raw(host=h, ua=headers[(k * 7 + 3) % len(headers)] if len(h) < 1000 else b"ua"))
        out.append(raw(ua=h, path=b"/" + text(rng, k % 23) + b"/" * (k % 4)))
    # URI hosts
    ws = bytes(range(0x09, 0x0E)) + b" "
    for k in range(40):
        lead, trail = bytes(rng.choice(ws) for _ in range(RUNS[k % 6])), bytes(rng.choice(ws) for _ in range(RUNS[(k // 6) % 6]))
        body = bytearray(text(rng, KEPT[k % 5]))
        if len(body) > 2:
            body[len(body) // 2] = rng.choice(b"\xC3\xA9\xFF\x80\x00\x1F\x7F")  # not text for a header; kept in a URI host
        out.append(raw(present=URI_BIT | HDR_BIT | UA_BIT, uri=lead + bytes(body) + trail, host=b"good.example"))
    out += [raw(present=URI_BIT | HDR_BIT | UA_BIT, uri=u, host=b" header.example ") for u in
            (b"", b"\n\x0b\x0c\r", b"\nuri.example\r", b"u" * 257, b"u" * 256, b"\x0c" + b"u" * 257 + b" ", b" " * 300 + b"u" * 256 + b"\n" * 17,
             b"\r" * (20 * 1024) + b"u.example" + b"\x0b" * (20 * 1024))]
    # every combination of the present bits, with garbage under a clear bit
    garbage = (b"\xff\x00 garbage \x80", b"  \t", b"g" * 300, b"")
    for bits in range(8):
        for g in garbage:
            out.append(Raw(bits, g if not bits & HDR_BIT else b"\thdr.example ", b"/bits/%d//" % bits, g if not bits & UA_BIT else b" ua/%d\t" % bits,
                           g if not bits & URI_BIT else b"\n uri.example\r"))
        out.append(Raw(bits | 0xF8, b"hdr.example", b"/unknown/bits/", b"ua", b"uri.example"))  # unknown bits are ignored
    # paths
    for p in (b"", b"/", b"////", b"/a/", b"/a//b///", b"x" * 15 + b"/" * 33, b"/" * 16, b"/" * 17, b"a" + b"/" * 16, b"/" * 300, b"/a" * 200 + b"/" * 31, b"/\xc3\xa9/", b"/a/ "):
        out.append(raw(path=p))
    # and a crowd of ordinary and odd requests
    alpha = [b" ", b"\t", b"a", b"/", b"\x7f", b"\x80", b"\n", b"~", b"\x1f", b"Mozilla/5.0", b".example"]
    while len(out) < 2000:
        v = [b"".join(rng.choice(alpha) for _ in range(rng.randint(0, 12))) * rng.choice([1, 1, 1, 1, 9]) for _ in range(4)]
        if rng.random() < 0.6:
            v = [b"www.shop%d.example" % rng.randrange(50), b"/cat/%d/item/" % rng.randrange(999), b"Mozilla/5.0 (X11; Linux x86_64) r%d " % rng.randrange(99), v[3]]
        out.append(Raw(rng.choice([6, 6, 6, 7, 2, 4, 0, 1, 3, 5]), *v))
    return tuple(out)


# ---- calling pwaf_derive_batch as it is ---------------------------------------------------------------------------------------------------
def aligned(nbytes, fill=FILL, align=16):
    block = np.full(nbytes + align, fill, dtype=np.uint8)
    at = -block.ctypes.data % align
    return block[at:at + nbytes]


def extra_struct(uri=None, present=None, ptr=lambda a: a.ctypes.data):
    e = _abi.RawColumns()
    e.struct_size = C.sizeof(_abi.RawColumns)
    if uri is not None:
        e.uri_host.data, e.uri_host.offsets = ptr(uri[0]), ptr(uri[1])
    if present is not None:
        e.present = ptr(present)
    return e


class HostOut:
    """Output blocks in host memory: data (cap bytes), offsets (n + 1 words) and stats, each with CANARY bytes behind it, all holding FILL."""

    def __init__(self, n, caps):
        self.n, self.caps = n, [int(c) for c in caps]
        self.data = [aligned(c + CANARY) for c in self.caps]
        self.off = [aligned(4 * (n + 1) + CANARY) for _ in self.caps]
        self.stats = aligned(32 + CANARY)
        self.cols = (_abi.DerivedCol * 3)()
        for c in range(3):
            self.cols[c].data, self.cols[c].offsets, self.cols[c].cap = self.data[c].ctypes.data, self.off[c].ctypes.data, self.caps[c]

    def untouched(self):
        return all((a == FILL).all() for a in self.data + self.off + [self.stats])

    def offsets(self, c):
        return self.off[c][:4 * (self.n + 1)].view(np.uint32)

    def stats_dict(self):
        s = _abi.DeriveStats.from_buffer_copy(self.stats[:32].tobytes())
        return {"bytes": [int(b) for b in s.bytes], "n": int(s.n), "overflow": int(s.overflow)}


def check_outputs(want, caps, data, offsets, stats, canaries, what=""):
    """The contract of include/pwaf.h against what the oracle derived. want: three lists of bytes; data[c]: the cap[c] bytes of column c as
    a uint8 array; offsets[c]: n + 1 words; stats: the dict; canaries: the arrays behind every output."""
    n = len(want[0])
    overflow = 0
    for c in range(3):
        blob = b"".join(want[c])
        o = np.zeros(n + 1, dtype=np.uint32)
        if n:
            o[1:] = np.cumsum([len(v) for v in want[c]], dtype=np.uint64).astype(np.uint32)
        assert np.array_equal(offsets[c], o), (what, c, "offsets")
        assert stats["bytes"][c] == len(blob), (what, c, stats)
        cap = caps[c]
        if len(blob) + PAD <= cap:
            assert data[c][:len(blob)].tobytes() == blob, (what, c, "bytes")
            assert not data[c][len(blob):len(blob) + PAD].any(), (what, c, "pad")
            assert (data[c][len(blob) + PAD:cap] == FILL).all(), (what, c, "written between bytes + 16 and cap")
        else:
            overflow |= 1 << c
            tail = data[c][len(blob):cap]  # what lies below cap of the pad is written, whatever became of the bytes
            assert not tail.any(), (what, c, "pad below cap")
    assert stats["n"] == n and stats["overflow"] == overflow, (what, stats, overflow)
    for k, a in enumerate(canaries):
        assert (a == FILL).all(), (what, "canary", k)


def derive_host_mode(batch, uri=None, present=None, caps=None, extra="own"):
    """pwaf_derive_batch in HOST mode on a RequestBatch -> (rc, HostOut). caps None: the raw column's bytes + 16 (host: both sources' bytes + 16)."""
    st = batch.as_struct()
    if caps is None:
        span = lambda o: int(o[-1]) - int(o[0])  # noqa: E731
        caps = [span(batch.offsets[HOST]) + (span(uri[1]) if uri is not None else 0) + PAD, span(batch.offsets[PATH]) + PAD, span(batch.offsets[UA]) + PAD]
    out = HostOut(batch.n, caps)
    e = extra_struct(uri, present) if extra == "own" else extra
    rc = lib().pwaf_derive_batch(C.byref(st), None if e is None else C.byref(e), out.cols, out.stats.ctypes.data, None, 0, None)
    return rc, out


def check_host_out(want, out: HostOut, what=""):
    n = out.n
    check_outputs(want, out.caps, [d[:c] for d, c in zip(out.data, out.caps)], [out.offsets(c) for c in range(3)], out.stats_dict(),
                  [d[c:] for d, c in zip(out.data, out.caps)] + [o[4 * (n + 1):] for o in out.off] + [out.stats[32:]], what)
