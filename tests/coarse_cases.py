"""Table shapes for the coarse level of the IPv4 lookup table (csrc/dirtable.h), shared by tests/test_addresses_coarse_cpu.py and
tests/test_gpu_ipres_coarse.py. A coarse block is 2^shift /24s (shift 5: a /19, shift 6: a /18); the named /24s below keep their role
at both shifts."""
import numpy as np

import lpm_reference as R

U = np.uint64


def sparse_geo_prefixes():
    """Mostly empty space (common entry 0). Set blocks: block 0, the last block, one set block whose two neighbours are clear at /19
    and at /18 (60.1.0.0), a region of many set blocks (70.0.0.0/12), prefixes inside 127/8 and 224/4 (set blocks whose addresses the
    GeoIP lookup excludes), runs that start inside a 32-/24 group."""
    p = ["0.0.5.0/24", "255.255.255.0/24", "60.1.0.0/24", "70.0.0.0/12", "70.3.7.0/24", "70.3.9.0/23", "127.5.0.0/16", "230.1.0.0/16"]
    p += ["80.0.0.0/21", "80.0.3.0/24", "80.0.4.0/22", "81.0.31.0/24", "81.0.32.0/24", "81.0.63.0/24", "81.0.64.0/24"]  # at the ends of /19 and /18 blocks
    return p


def sparse_lists():
    return {"l": ["90.0.0.0/20", "90.0.16.128/25", "60.1.0.0/24", "100.0.0.0/24"], "m": ["70.0.0.0/13", "100.0.0.0/24"]}


# the /24s whose blocks play a part (first three octets as one number)
X = lambda a, b, c: (a << 16) | (b << 8) | c
CLEAR_24 = X(20, 0, 0)       # a clear block: 20.0.0.0/18
SET_24 = X(70, 0, 0)         # a set block inside the /12
ISOLATED_24 = X(60, 1, 0)    # set; 60.0.192.0/18 before it and 60.1.64.0/18 behind it are clear
LOOPBACK_SET_24 = X(127, 5, 0)
LOOPBACK_CLEAR_24 = X(127, 200, 0)
MULTICAST_SET_24 = X(230, 1, 0)
MULTICAST_CLEAR_24 = X(225, 0, 0)


def block_ends(x24: int, shift: int):
    """first and last /24 of the block of 2^shift /24s that holds x24"""
    first = (x24 >> shift) << shift
    return first, first + (1 << shift) - 1


def edge_24s(shift: int):
    """first and last /24 of: a clear block, a set block, block 0, the last block, the isolated set block and both its clear
    neighbours, the loopback / multicast blocks"""
    out = []
    for x in (CLEAR_24, SET_24, 0, (1 << 24) - 1, ISOLATED_24, ISOLATED_24 - (1 << shift), ISOLATED_24 + (1 << shift), LOOPBACK_SET_24, LOOPBACK_CLEAR_24,
              MULTICAST_SET_24, MULTICAST_CLEAR_24, X(81, 0, 31), X(81, 0, 63), X(80, 0, 0), X(90, 0, 16)):
        out += list(block_ends(x, shift))
    return sorted(set(out))


def dense_geo_prefixes():
    """three quarters of the /19s hold a /24 with a record: a summary at /24 ... /20 granularity is still worth having (few of ITS blocks
    are set) while more than half of the coarse blocks are, so the coarse level is switched off"""
    return ["%d.%d.%d.0/24" % (b >> 11, (b >> 3) & 255, (b & 7) << 5) for b in range(1 << 19) if b % 4]  # the first /24 of /19 number b


def quarters_geo_prefixes():
    """four /2s with a record each: no summary (tests/test_addresses_cpu.py), hence no coarse level"""
    return ["0.0.0.0/2", "64.0.0.0/2", "128.0.0.0/2", "192.0.0.0/2"]


def common_not_zero():
    """a record and a list over the whole space, other records over a /4 and two /24s: the most common entry is (record 1, set {l}), not 0"""
    return ["0.0.0.0/0", "128.0.0.0/4", "200.1.2.0/24", "10.1.0.0/24"], {"l": ["0.0.0.0/0"], "m": ["200.1.2.0/24"]}


def flat_from_prefixes(geo_prefixes, lists=None):
    """the 2^24-entry table the engine would build for prefixes no longer than /24: (row + 1) | set bits << 16, by the brute-force reference"""
    all24 = np.arange(1 << 24, dtype=U) << U(8)
    pre = [R.parse_prefix(x) for x in geo_prefixes]
    assert all(not v6 and ln <= 24 for v6, _, ln in pre)
    flat = (R.lpm4(all24, [(v, ln, row) for row, (_, v, ln) in enumerate(pre)]) + 1).astype(np.uint32)
    for k, items in enumerate((lists or {}).values()):
        lp = [R.parse_prefix(x) for x in items]
        flat |= R.member4(all24, [(v, ln) for _, v, ln in lp if ln <= 24]).astype(np.uint32) << np.uint32(16 + k)
    return flat
