"""TEST-ONLY reference for the address predicates: longest-prefix match and list membership by comparing addresses with prefixes.

It owes nothing to the project: no oracle, no library code, no trie. A prefix is `(value, length)` — an integer with the host bits
clear and the number of leading bits that count; an address is inside it when its leading `length` bits equal the prefix's.

* GeoIP answer = the record of the LONGEST prefix that contains the address; none: the default record `{0, "XX"}`. Loopback and
  multicast addresses are never looked up (pingoo/geoip.rs:73-91: "not found"): they read the default record too.
* list answer = the address is inside ANY prefix of the list (pingoo/lists.rs:102-108,119-121).
* Duplicates: when the same prefix (same value, same length) occurs twice in a GeoIP table, the LATER row wins. The reference
  builds a map with insert(), which replaces (oracle/oracle_engine.cpp: geo_insert, "later duplicates override earlier ones"), and
  the product sorts equal ranges by input order so that the later one is innermost (csrc/iptrie.cpp: family). Here: prefixes are
  applied in the order (length, row), each overwriting what a shorter or earlier one left. A prefix twice in one list, or in two
  lists, needs no rule: membership is an OR.

Two ways to the same answer, pinned against each other and against the standard library's `ipaddress` in tests/test_addresses_cpu.py:
`brute=True` compares every address with every prefix; the default groups the IPv4 prefixes by length and looks the address's leading
bits up among the sorted prefixes of that length (still nothing but "leading bits equal"), which is what makes tables of millions
of prefixes against all 2^24 /24s a matter of seconds. IPv6 (two uint64 halves) is always brute force.
"""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
U = np.uint64


def parse_v4(s: str) -> int:
    parts = s.split(".")
    assert len(parts) == 4, s
    v = 0
    for p in parts:
        assert p.isdigit() and int(p) <= 255, s
        v = v << 8 | int(p)
    return v


def parse_v6(s: str) -> int:
    head, gap, tail = s.partition("::")
    groups = lambda t: [int(g, 16) for g in t.split(":")] if t else []
    h, t = groups(head), groups(tail)
    assert (len(h) + len(t) <= 7) if gap else (len(h) == 8 and not t), s
    full = h + [0] * (8 - len(h) - len(t)) + t
    v = 0
    for g in full:
        assert 0 <= g <= 0xFFFF, s
        v = v << 16 | g
    return v


def parse_addr(s: str):
    """text -> (is_v6, value)"""
    return (True, parse_v6(s)) if ":" in s else (False, parse_v4(s))


def parse_prefix(s: str):
    """"a.b.c.d/len" or "x:y::/len" (host bits are cleared, as every consumer of such a list does) -> (is_v6, value, length)"""
    a, _, ln = s.strip().partition("/")
    v6, v = parse_addr(a)
    bits = 128 if v6 else 32
    length = int(ln) if ln else bits
    assert 0 <= length <= bits, s
    mask = ((1 << length) - 1) << (bits - length)
    return v6, v & mask, length


def fmt_addr(v6: bool, v: int) -> str:
    if not v6:
        return ".".join(str((v >> s) & 255) for s in (24, 16, 8, 0))
    return ":".join("%x" % ((v >> s) & 0xFFFF) for s in range(112, -16, -16))


def fmt_prefix(v6: bool, v: int, length: int) -> str:
    return f"{fmt_addr(v6, v)}/{length}"


# --- addresses as arrays: IPv4 = one uint64 array; IPv6 = (hi, lo) uint64 arrays --------------------------------------------------
def v6_arrays(values):
    vals = list(values)
    return np.array([v >> 64 for v in vals], dtype=U), np.array([v & M64 for v in vals], dtype=U)


def contains4(addr: np.ndarray, value: int, length: int) -> np.ndarray:
    if length == 0:
        return np.ones(len(addr), dtype=bool)
    return (addr >> U(32 - length)) == U(value >> (32 - length))


def contains6(hi: np.ndarray, lo: np.ndarray, value: int, length: int) -> np.ndarray:
    vhi, vlo = value >> 64, value & M64
    if length == 0:
        return np.ones(len(hi), dtype=bool)
    if length <= 64:
        return (hi >> U(64 - length)) == U(vhi >> (64 - length))
    return (hi == U(vhi)) & ((lo >> U(128 - length)) == U(vlo >> (128 - length)))


def _by_length(prefixes):
    """[(value, length, row)] or (values, lengths, rows) arrays -> {length: (sorted distinct leading bits, the LAST row holding each)}"""
    if not isinstance(prefixes, tuple):
        prefixes = (np.array([p[0] for p in prefixes], dtype=U), np.array([p[1] for p in prefixes], dtype=np.int64), np.array([p[2] for p in prefixes], dtype=np.int64))
    values, lengths, all_rows = (np.asarray(x) for x in prefixes)
    out = {}
    for length in np.unique(lengths).tolist():
        sel = lengths == length
        keys = values[sel].astype(U) >> U(32 - length) if length else np.zeros(int(sel.sum()), dtype=U)
        rows = all_rows[sel].astype(np.int64)
        order = np.lexsort((rows, keys))  # by leading bits, then by row: the last of equal ones is the latest row
        keys, rows = keys[order], rows[order]
        last = np.ones(len(keys), dtype=bool)
        last[:-1] = keys[1:] != keys[:-1]
        out[int(length)] = (keys[last], rows[last])
    return out


def lpm4(addr: np.ndarray, prefixes, brute: bool = False) -> np.ndarray:
    """For every IPv4 address (uint64 array) the row of the longest containing prefix (later row among duplicates), -1 for none.
    prefixes: [(value, length, row)], or for very large tables a tuple of arrays (values uint64, lengths, rows int64)."""
    out = np.full(len(addr), -1, dtype=np.int64)
    if brute:
        for value, length, row in sorted(prefixes, key=lambda p: (p[1], p[2])):
            out[contains4(addr, value, length)] = row
        return out
    for length, (keys, rows) in sorted(_by_length(prefixes).items()):  # shorter first: longer ones overwrite
        lead = addr >> U(32 - length) if length else np.zeros(len(addr), dtype=U)
        if len(keys) <= 8:  # (a handful of prefixes of this length: compare with each)
            for key, row in zip(keys, rows):
                out[lead == key] = row
            continue
        at = np.minimum(np.searchsorted(keys, lead), len(keys) - 1)
        hit = keys[at] == lead
        out[hit] = rows[at][hit]
    return out


def lpm6(hi: np.ndarray, lo: np.ndarray, prefixes) -> np.ndarray:
    out = np.full(len(hi), -1, dtype=np.int64)
    for value, length, row in sorted(prefixes, key=lambda p: (p[1], p[2])):
        out[contains6(hi, lo, value, length)] = row
    return out


def member4(addr: np.ndarray, prefixes, brute: bool = False) -> np.ndarray:
    """prefixes: [(value, length)] of ONE list -> bool per address"""
    return lpm4(addr, [(v, ln, 0) for v, ln in prefixes], brute) >= 0


def member6(hi: np.ndarray, lo: np.ndarray, prefixes) -> np.ndarray:
    out = np.zeros(len(hi), dtype=bool)
    for value, length in prefixes:
        out |= contains6(hi, lo, value, length)
    return out


def geo_excluded4(addr: np.ndarray) -> np.ndarray:
    """pingoo/geoip.rs:73-91: loopback (127/8) and multicast (224/4) are "not found" """
    b0 = addr >> U(24)
    return (b0 == U(127)) | ((b0 >> U(4)) == U(0xE))


def geo_excluded6(hi: np.ndarray, lo: np.ndarray) -> np.ndarray:
    """::1 and ff00::/8"""
    return ((hi == U(0)) & (lo == U(1))) | ((hi >> U(56)) == U(0xFF))


class Geo:
    """A GeoIP table: rows of (prefix text, asn, country). `lookup4/6` -> the row index per address (-1: the default record)."""

    def __init__(self, rows):
        self.rows = list(rows)
        self.p4, self.p6 = [], []
        for i, (cidr, _, _) in enumerate(self.rows):
            v6, value, length = parse_prefix(cidr)
            (self.p6 if v6 else self.p4).append((value, length, i))

    def lookup4(self, addr, brute=False):
        out = lpm4(addr, self.p4, brute) if self.p4 else np.full(len(addr), -1, dtype=np.int64)
        out[geo_excluded4(addr)] = -1
        return out

    def lookup6(self, hi, lo):
        out = lpm6(hi, lo, self.p6)
        out[geo_excluded6(hi, lo)] = -1
        return out

    def record(self, row: int):
        """(asn, country) of a lookup result; the default record is {0, "XX"}"""
        return (0, "XX") if row < 0 else (self.rows[row][1], self.rows[row][2])


class Lists:
    """Named address lists: {name: [prefix text]}. `member4/6(name, ...)` -> bool per address."""

    def __init__(self, lists):
        self.p4, self.p6 = {}, {}
        for name, items in lists.items():
            self.p4[name], self.p6[name] = [], []
            for s in items:
                v6, value, length = parse_prefix(s)
                (self.p6 if v6 else self.p4)[name].append((value, length))

    def member4(self, name, addr, brute=False):
        return member4(addr, self.p4[name], brute) if self.p4[name] else np.zeros(len(addr), dtype=bool)

    def member6(self, name, hi, lo):
        return member6(hi, lo, self.p6[name])
