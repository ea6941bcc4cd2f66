"""Table shapes and edge addresses for the address-path tests (tests/test_addresses_cpu.py on the CPU, tests/test_gpu_addresses.py on
the device). A case is `(geo_rows, lists)`: GeoIP rows `(prefix text, asn, country)` — every row an asn of its own, 1 + its index
unless stated — and `{name: [prefix text]}` address lists. Everything here is plain data; the expected answers come from
tests/lpm_reference.py."""
from __future__ import annotations

import numpy as np

import lpm_reference as R


def country(k: int) -> str:
    """country k of 676: AA, AB, ... — never XX (the default record's)"""
    k = k % 675
    k += k >= 23 * 26 + 23
    return chr(65 + k // 26) + chr(65 + k % 26)


def geo_rows(prefixes, asn0: int = 1):
    return [(p, asn0 + i, country(i)) for i, p in enumerate(prefixes)]


def v4(a, b, c, d=0):
    return f"{a}.{b}.{c}.{d}"


# --- runs: what the 16-byte records of the compressed table have to get right ----------------------------------------------------
def runs_prefixes():
    p = [v4(10, 0, c) + "/24" for c in range(256)]  # a /16 whose 256 /24s all differ: 32 run starts in every group
    # 11.1/16: groups with 1 (bit 0), 0, 0, 0, 1 (bit 0 again: the /17 ends), 2, 3 and 1 starts
    p += ["11.1.0.0/17", "11.1.170.0/24", "11.1.200.0/24", "11.1.222.0/23"]
    p += ["11.2.31.0/24"]  # a start at bit 31 of group 0, then at bit 0 of group 1
    for c in range(1, 8):  # the empty run between two /24s crosses exactly c group boundaries
        p += [v4(12, c, 5) + "/24", v4(12, c, 32 * c + 5) + "/24"]
    p += ["13.0.0.0/15", "14.7.0.0/16", "15.0.128.0/17", "15.1.0.0/18"]  # runs across a /16 boundary, a whole /16, half ones
    return p


# --- every prefix length, nesting, adjacency, both ends of the space -------------------------------------------------------------
def chain4(addr: str, lengths):
    _, v = R.parse_addr(addr)
    return [R.fmt_prefix(False, v & (((1 << ln) - 1) << (32 - ln)), ln) for ln in lengths]


def lengths_geo_prefixes():
    p = chain4("200.100.50.25", range(0, 33))  # lengths 0..32 nested 33 deep
    p += ["255.255.255.255/32", "255.255.255.0/24", "255.255.0.0/16", "0.0.0.0/8", "0.0.0.0/32", "0.0.0.0/25"]
    p += ["30.0.0.0/24", "30.0.1.0/24", "30.0.2.0/23", "30.0.4.0/25", "30.0.4.128/25"]  # adjacent, different records
    p += ["127.0.0.0/8", "127.0.0.1/32", "224.0.0.0/4", "239.255.255.0/24", "126.255.255.0/24", "128.0.0.0/24", "223.255.255.0/24", "240.0.0.0/24"]  # never looked up, and their neighbours
    p += ["30.0.1.0/24", "200.100.50.0/24", "200.100.50.25/32", "0.0.0.0/0"]  # the same prefixes once more, with records of their own: the later row wins
    return p


def lengths_lists():
    return {
        "even": chain4("100.64.77.200", range(0, 33, 2)),
        "odd": chain4("100.64.77.200", range(1, 33, 2)),
        "ends": ["255.255.255.255", "255.255.255.254/31", "0.0.0.0/32", "0.0.0.0/9", "255.128.0.0/9"],
        # adjacent prefixes with the same payload (one run), next to a list that splits them
        "adj": ["30.0.0.0/24", "30.0.1.0/24", "30.0.2.0/24", "30.0.3.0/25", "30.0.3.128/25", "30.0.31.0/24", "30.0.32.0/24"],
        "split": ["30.0.1.0/24", "30.0.3.128/25"],
        "dup": ["40.1.2.0/24", "40.1.2.0/24", "40.1.0.0/16", "30.0.0.0/24"],  # the same prefix twice in one list, and in two lists
    }


# --- escapes: prefixes longer than /24 in one trie, in the other, in both, nested --------------------------------------------------
def escape_case():
    geo = ["50.0.0.0/8"] + [v4(50, 1, 1, 0) + "/25", "50.1.1.128/26", "50.1.1.192/27", "50.1.1.224/28", "50.1.1.240/29", "50.1.1.248/30", "50.1.1.252/31", "50.1.1.254/32"]  # /25 ... /32, GeoIP only
    geo += ["50.2.2.0/24", "50.2.2.64/26", "50.2.2.65/32", "50.2.2.96/27", "50.2.2.100/30"]  # nested inside one /24
    geo += ["50.3.3.128/25", "50.9.40.17/32", "50.9.255.255/32", "50.10.0.0/32"]  # both tries (lists below); hosts at a /16's edges
    lists = {
        "deep": ["60.1.1.0/25", "60.1.1.128/26", "60.1.1.192/27", "60.1.1.224/28", "60.1.1.240/29", "60.1.1.248/30", "60.1.1.252/31", "60.1.1.254/32"],  # the list trie only
        "both": ["50.3.3.0/26", "50.3.3.130/31", "50.9.40.0/28"],
        "nest": ["60.2.2.0/24", "60.2.2.16/28", "60.2.2.17/32", "60.2.0.0/16", "60.3.3.0/24", "60.3.3.16/28"],  # (inside their own list's /24: one set, no escape)
        "host": ["50.9.40.17", "60.255.255.255", "61.0.0.0", "60.3.3.17/32", "60.3.3.16/29"],  # nested across lists
    }
    return geo, lists


# --- escapes by id: n lists, list k holds the /24s of a 2^n-/24 region whose index has bit k set --------------------------------------
BITS_BASE = 64 << 24  # 64.0.0.0


def bit_lists(n: int):
    """list k: 2^(n-1-k) prefixes of length 24-k; the /24 with index i of the region is in list k iff bit k of i is set, so the
    region's 2^n /24s have 2^n different membership sets"""
    lists = {}
    for k in range(n):
        step = 1 << (k + 1)
        lists[f"b{k}"] = [R.fmt_prefix(False, BITS_BASE + ((m * step + (1 << k)) << 8), 24 - k) for m in range(1 << (n - 1 - k))]
    return lists


# --- the summary: blocks of 2^s /24s, alternately empty and under a prefix of their own, over 60 % of the space ---------------------
def summary_prefix_arrays(s: int):
    """(values uint64, length) of the /(24-s) prefixes: the odd blocks below 0.6 * 2^(24-s)"""
    n_blk = int(0.6 * (1 << (24 - s)))
    blocks = np.arange(1, n_blk, 2, dtype=np.uint64)
    return blocks << np.uint64(8 + s), 24 - s


def summary_flat(s: int) -> np.ndarray:
    flat = np.zeros(1 << 24, dtype=np.uint32)
    blk = np.arange(1 << 24, dtype=np.uint32) >> s
    on = (blk & 1).astype(bool) & (blk < int(0.6 * (1 << (24 - s))))
    flat[on] = (blk[on] & 0x7FFF) + 1  # a value per block (0 stays the common entry)
    return flat


# --- IPv6 ----------------------------------------------------------------------------------------------------------------------------
V6_DEEP = "2001:db8:a1b2:c3d4:e5f6:1728:394a:5b6c"


def chain6(addr: str, lengths):
    _, v = R.parse_addr(addr)
    return [R.fmt_prefix(True, v & (((1 << ln) - 1) << (128 - ln)), ln) for ln in lengths]


def v6_case():
    geo = chain6(V6_DEEP, range(0, 129, 3)) + ["::/0", "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff/128", "::1/128", "ff00::/8", "::/128", "fe80::/10", "2001:db8::/32",
                                                "2001:db8:a1b2::/56"]  # a GeoIP trie that ends early where the list trie goes on (below), and the reverse at /126
    lists = {
        "l0": chain6(V6_DEEP, range(1, 129, 3)),
        "l1": chain6(V6_DEEP, range(2, 129, 3)) + [V6_DEEP + "/128", "::1", "ff02::1", "ffff:ffff:ffff:ffff:ffff:ffff:ffff:fffe/127"],
        "l2": ["2001:db8:a1b2:c3d4:e5f6:1728:394a:5b00/120", "2001:db8:a1b2:c300::/56", "::/1", "8000::/1"],
    }
    return geo, lists


# --- edge addresses --------------------------------------------------------------------------------------------------------------------
def edges4(prefix_texts, summary_shift: int = 4):
    """For every IPv4 prefix: its first and last address, the one before and the one after, and the first and last address of every /24,
    32-/24 group, /16 and summary block (2^shift /24s) its two ends touch -> sorted distinct uint64 values"""
    out = set()
    for t in prefix_texts:
        v6, v, ln = R.parse_prefix(t)
        if v6:
            continue
        lo, hi = v, v | ((1 << (32 - ln)) - 1)
        for a in (lo, hi):
            for bits in (8, 13, 16, 8 + summary_shift):
                out.update((a >> bits << bits, (a >> bits << bits) | ((1 << bits) - 1)))
        out.update((lo, hi, lo - 1, hi + 1))
    return np.array(sorted(a for a in out if 0 <= a < 1 << 32), dtype=np.uint64)


def edges6(prefix_texts):
    """first / last / before / after of every IPv6 prefix, and for every byte position 2..15 a pair of neighbours of the first prefix's
    first address that differ first in that byte"""
    out = set()
    base = None
    for t in prefix_texts:
        v6, v, ln = R.parse_prefix(t)
        if not v6:
            continue
        base = v if base is None else base
        lo, hi = v, v | ((1 << (128 - ln)) - 1)
        out.update((lo, hi, lo - 1, hi + 1))
    if base is not None:
        for byte in range(2, 16):
            out.update((base ^ (1 << (8 * (15 - byte))), base ^ (0x80 << (8 * (15 - byte)))))
    return sorted(a for a in out if 0 <= a < 1 << 128)


def whole_16s(*tops):
    """every third octet of the /16s `tops` (first two octets as one number), host bytes 0 and 255"""
    c = np.arange(256, dtype=np.uint64)
    return np.concatenate([(np.uint64(t) << np.uint64(16)) | (c << np.uint64(8)) | np.uint64(h) for t in tops for h in (0, 255)])
