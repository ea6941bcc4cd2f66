"""The address path on the CPU (no device): tries (csrc/iptrie.cpp) -> the flattening of their first 24 bits (dir24_kernel, restated)
-> run compression and summary choice (csrc/dirtable.h, the header pwaf_engine_create calls) -> the lookup (ipres_kernel, restated),
for ALL 2^24 /24s and for chosen full addresses, against the brute-force reference of tests/lpm_reference.py. The host harness is
tests/dirtable_host.cpp; every table shape asserts, on the counts the harness returns, that the shape was really produced."""
import ipaddress
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import address_cases as AC
import lpm_reference as R
from pingoo_amd import _abi
from pingoo_amd.batch import GEOIP_DTYPE
from pingoo_amd.engine import CompiledProgram
from table_walker import TRIE_LEAF, Tables

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "dirtable_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "pingoo_amd", "csrc", "dirtable.h")]
U = np.uint64
ALL24 = None


def all24():
    global ALL24
    if ALL24 is None:
        ALL24 = np.arange(1 << 24, dtype=U) << U(8)
    return ALL24


# ---------------------------------------------------------------------------------------------------------
# 1. the reference itself
# ---------------------------------------------------------------------------------------------------------
def test_reference_containment_matches_ipaddress():
    rng = random.Random(11)
    n = 0
    for v6 in (False, True):
        bits = 128 if v6 else 32
        for length in range(bits + 1):
            for _ in range(40 if not v6 else 12):
                net_v = rng.getrandbits(bits) & (((1 << length) - 1) << (bits - length))
                net = (ipaddress.IPv6Network if v6 else ipaddress.IPv4Network)((net_v, length))
                lo, hi = net_v, net_v | ((1 << (bits - length)) - 1)
                addrs = [a for a in (lo, hi, lo - 1, hi + 1, rng.getrandbits(bits), lo + rng.getrandbits(bits - length) if length < bits else lo) if 0 <= a < 1 << bits]
                want = np.array([ipaddress.IPv6Address(a) in net for a in addrs]) if v6 else None
                if v6:
                    got = R.contains6(*R.v6_arrays(addrs), net_v, length)
                else:
                    want = np.array([ipaddress.IPv4Address(a) in net for a in addrs])
                    got = R.contains4(np.array(addrs, dtype=U), net_v, length)
                assert got.tolist() == want.tolist(), (net, addrs)
                # the text forms agree with the standard library's
                assert R.parse_prefix(str(net)) == (v6, net_v, length) and R.parse_addr(str(net.network_address)) == (v6, net_v)
                assert ipaddress.ip_network(R.fmt_prefix(v6, net_v, length)) == net
                n += len(addrs)
    assert n > 5000


def test_reference_longest_match_matches_ipaddress_and_both_ways_agree():
    rng = random.Random(12)
    for trial in range(30):
        prefixes = []
        for row in range(rng.randint(1, 60)):
            length = rng.choice([0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, rng.randint(0, 32)])
            v = rng.getrandbits(32) & (((1 << length) - 1) << (32 - length)) if rng.random() < 0.5 or not prefixes else prefixes[rng.randrange(len(prefixes))][0] & (((1 << length) - 1) << (32 - length))
            prefixes.append((v, length, row))
        addrs = [rng.getrandbits(32) for _ in range(60)] + [p[0] for p in prefixes] + [min((1 << 32) - 1, p[0] | ((1 << (32 - p[1])) - 1)) for p in prefixes]
        a = np.array(addrs, dtype=U)
        nets = [ipaddress.IPv4Network((v, ln)) for v, ln, _ in prefixes]
        want = []
        for x in addrs:
            best = -1
            for row, net in enumerate(nets):
                if ipaddress.IPv4Address(x) in net and (best < 0 or net.prefixlen >= nets[best].prefixlen):
                    best = row  # (>=: the later of equal prefixes)
            want.append(best)
        assert R.lpm4(a, prefixes, brute=True).tolist() == want
        assert R.lpm4(a, prefixes).tolist() == want
        vals, lens, rows = (np.array([p[k] for p in prefixes]) for k in range(3))
        assert R.lpm4(a, (vals.astype(U), lens, rows)).tolist() == want
        assert R.member4(a, [(v, ln) for v, ln, _ in prefixes]).tolist() == [w >= 0 for w in want]
    # IPv6: all lengths
    for trial in range(10):
        base = rng.getrandbits(128)
        prefixes = [(base & (((1 << ln) - 1) << (128 - ln)), ln, row) for row, ln in enumerate(rng.sample(range(129), 40))]
        addrs = [base ^ (1 << rng.randrange(128)) for _ in range(80)] + [base, 0, (1 << 128) - 1]
        nets = [ipaddress.IPv6Network((v, ln)) for v, ln, _ in prefixes]
        want = [max((row for row, net in enumerate(nets) if ipaddress.IPv6Address(x) in net), key=lambda r: nets[r].prefixlen, default=-1) for x in addrs]
        assert R.lpm6(*R.v6_arrays(addrs), prefixes).tolist() == want


def test_reference_duplicates_and_exclusions():
    geo = R.Geo([("9.9.0.0/16", 1, "AA"), ("9.9.0.0/16", 2, "BB"), ("9.0.0.0/8", 3, "CC"), ("9.0.0.0/8", 4, "DD"), ("127.0.0.0/8", 5, "EE"), ("::/0", 6, "FF"), ("::/0", 7, "GG")])
    a = np.array([R.parse_v4(x) for x in ("9.9.1.1", "9.8.1.1", "127.0.0.1", "224.0.0.1", "239.255.255.255", "240.0.0.0", "126.255.255.255", "128.0.0.0")], dtype=U)
    for brute in (True, False):
        assert [geo.record(r) for r in geo.lookup4(a, brute)] == [(2, "BB"), (4, "DD"), (0, "XX"), (0, "XX"), (0, "XX"), (0, "XX"), (0, "XX"), (0, "XX")]
    got = geo.lookup6(*R.v6_arrays([R.parse_v6(x) for x in ("::1", "::2", "ff02::1", "feff::1", "::")]))
    assert [geo.record(r) for r in got] == [(0, "XX"), (7, "GG"), (0, "XX"), (7, "GG"), (7, "GG")]
    lists = R.Lists({"a": ["1.2.3.0/24", "1.2.3.0/24"], "b": ["1.2.3.0/24", "::1"]})
    x = np.array([R.parse_v4("1.2.3.4"), R.parse_v4("1.2.4.0")], dtype=U)
    assert lists.member4("a", x).tolist() == [True, False] == lists.member4("b", x).tolist()
    assert lists.member6("b", *R.v6_arrays([1, 2])).tolist() == [True, False] and lists.member6("a", *R.v6_arrays([1])).tolist() == [False]


# ---------------------------------------------------------------------------------------------------------
# 2. the harness
# ---------------------------------------------------------------------------------------------------------
def tool():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "dirtable_host")
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", SRC, "-o", out], check=True)
    return out


def run_harness(tmp_path, tables=None, flat=None, addrs=(), no_summary=False, per24=True):
    """-> (stats, eg[2^24], ei[2^24], results[n_addr, 2]); addrs: [(is_v6, value)], or an array of IPv4 addresses.
    The GeoIP trie of a dump has RECORD leaves and record 0 is the default, so geo_default is 0 here: that an empty family answers the
    default record's CLASS and not class 0 (which differ once a rule holds for the default record) is visible on the device only
    (tests/test_gpu_addresses.py: the empty-family cases)."""
    flags = (1 if no_summary else 0) | (2 if flat is not None else 0) | (8 if per24 else 0)
    sections = [np.zeros(0, dtype="<u4")] * 6
    n_ip_lists = geo_default = 0
    if tables is not None:
        flags |= 4 if tables.has_geo else 0
        n_ip_lists = tables.n_ip_lists
        sections = [np.asarray(getattr(tables, k), dtype="<u4") for k in ("gr4", "gr6", "gnod", "ir4", "ir6", "inod")]  # (a dump always has the six sections; an empty root = no prefix of that family)
    a4 = np.asarray([v for v6, v in addrs if not v6], dtype=">u4") if not isinstance(addrs, np.ndarray) else addrs.astype(">u4")
    a6 = [] if isinstance(addrs, np.ndarray) else [v for v6, v in addrs if v6]
    assert isinstance(addrs, np.ndarray) or all(not v6 for v6, _ in addrs[:len(a4)]), "IPv4 addresses first"
    rec = np.zeros((len(a4) + len(a6), 20), dtype=np.uint8)
    rec[:len(a4), :4] = a4.view(np.uint8).reshape(-1, 4)
    for i, v in enumerate(a6):
        rec[len(a4) + i, :16] = np.frombuffer(v.to_bytes(16, "big"), dtype=np.uint8)
        rec[len(a4) + i, 16] = 1
    ab = rec.tobytes()
    sections += [np.zeros(0, dtype="<u4") if flat is None else np.asarray(flat, dtype="<u4"), np.frombuffer(bytes(ab), dtype="<u4")]
    fin, fout = str(tmp_path / "dir.in"), str(tmp_path / "dir.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4I", 0x54524944, flags, n_ip_lists, geo_default))
        for s in sections:
            f.write(struct.pack("<I", len(s)))
            f.write(s.tobytes())
    r = subprocess.run([tool(), fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    stats = json.loads(r.stdout)
    out = np.fromfile(fout, dtype="<u4")
    os.remove(fin)
    os.remove(fout)
    eg = ei = None
    if per24 and stats["dir"]:
        eg, ei, out = out[:1 << 24], out[1 << 24:2 << 24], out[2 << 24:]
    assert stats["out_of_range"] == 0, stats
    return stats, eg, ei, out.reshape(-1, 2)


def compile_case(geo_rows, lists, geo_array=None):
    geo = geo_array
    if geo is None and geo_rows is not None:
        from pingoo_amd import geoip_entries

        geo = geoip_entries(geo_rows)
    ll = {name: (_abi.LIST_IP, items) for name, items in (lists or {}).items()}
    prog = CompiledProgram([("r", "client.remote_port == 1", [_abi.RULE_ACTION_BLOCK])], ll, geo)
    return Tables(prog.dump())


def check_case(tmp_path, geo_rows, lists, addrs4=(), addrs6=(), no_summary=False, geo_ref=None, tables=None, deep24_limit=4096):
    """Compiles the tables, runs the harness and compares every /24 and the given addresses (plus all 256 addresses of every /24 that
    holds a longer prefix) with the reference. -> (stats, tables)"""
    t = tables if tables is not None else compile_case(geo_rows, lists)
    lists = lists or {}
    geo = geo_ref if geo_ref is not None else (R.Geo(geo_rows) if geo_rows is not None else None)
    lref = R.Lists(lists)
    # the /24s that hold a prefix longer than /24: all their addresses are looked up one by one; every other /24 has one answer
    deep = set()
    if geo is not None and isinstance(geo, R.Geo):
        deep |= {v >> 8 for v, ln, _ in geo.p4 if ln > 24}
    for name in lists:
        deep |= {v >> 8 for v, ln in lref.p4[name] if ln > 24}
    assert len(deep) <= deep24_limit
    extra = (np.repeat(np.array(sorted(deep), dtype=U) << U(8), 256) + np.tile(np.arange(256, dtype=U), len(deep))) if deep else np.zeros(0, dtype=U)
    a4 = np.unique(np.concatenate([np.asarray(addrs4, dtype=U), extra]))
    a6 = list(addrs6)
    stats, eg, ei, res = run_harness(tmp_path, t, addrs=a4 if not a6 else [(False, int(x)) for x in a4] + [(True, x) for x in a6], no_summary=no_summary)
    names = list(lists)
    assert t.n_ip_lists == len(names)
    setm = np.asarray(t.set_masks, dtype=np.uint32) if names else None

    def in_list(set_ids, k):
        return ((setm[set_ids.astype(np.int64) * t.set_words + (k >> 5)] >> np.uint32(k & 31)) & 1).astype(bool)

    def rec_rows(recs):  # record id -> GeoIP row: records are the default, then the rows in order (every country here is valid)
        return recs.astype(np.int64) - 1

    if stats["dir"]:
        plain = np.ones(1 << 24, dtype=bool)
        if deep:
            plain[np.array(sorted(deep), dtype=np.int64)] = False
        if geo is not None:
            assert ((eg & TRIE_LEAF) != 0)[plain].all(), "a /24 without a longer GeoIP prefix does not end in a leaf"
            want = geo.lookup4(all24())
            got = rec_rows(eg & np.uint32(~TRIE_LEAF & 0xFFFFFFFF))
            bad = np.nonzero((got != want) & plain)[0]
            assert len(bad) == 0, f"GeoIP: {len(bad)} /24s differ; first {R.fmt_addr(False, int(bad[0]) << 8)}: got row {got[bad[0]]} want {want[bad[0]]}"
        if names:
            assert ((ei & TRIE_LEAF) != 0)[plain].all()
            sets = ei & np.uint32(~TRIE_LEAF & 0xFFFFFFFF)
            sets = np.where(plain, sets, 0)
            for k, name in enumerate(names):
                want = lref.member4(name, all24())
                bad = np.nonzero((in_list(sets, k) != want) & plain)[0]
                assert len(bad) == 0, f"list {name}: {len(bad)} /24s differ; first {R.fmt_addr(False, int(bad[0]) << 8)}"
    # full addresses
    r4, r6 = res[:len(a4)], res[len(a4):]
    if geo is not None:
        want = geo.lookup4(a4)
        bad = np.nonzero(rec_rows(r4[:, 0]) != want)[0]
        assert len(bad) == 0, f"GeoIP: {len(bad)} addresses differ; first {R.fmt_addr(False, int(a4[bad[0]]))}: got row {int(r4[bad[0], 0]) - 1} want {want[bad[0]]}"
        if a6:
            want = geo.lookup6(*R.v6_arrays(a6))
            bad = np.nonzero(rec_rows(r6[:, 0]) != want)[0]
            assert len(bad) == 0, f"GeoIP: {len(bad)} IPv6 addresses differ; first {R.fmt_addr(True, a6[bad[0]])}: got row {int(r6[bad[0], 0]) - 1} want {want[bad[0]]}"
    else:
        assert (res[:, 0] == 0).all()
    for k, name in enumerate(names):
        bad = np.nonzero(in_list(r4[:, 1], k) != lref.member4(name, a4))[0]
        assert len(bad) == 0, f"list {name}: {len(bad)} addresses differ; first {R.fmt_addr(False, int(a4[bad[0]]))}"
        if a6:
            bad = np.nonzero(in_list(r6[:, 1], k) != lref.member6(name, *R.v6_arrays(a6)))[0]
            assert len(bad) == 0, f"list {name}: {len(bad)} IPv6 addresses differ; first {R.fmt_addr(True, a6[bad[0]])}"
    if geo_rows is not None and geo is not None and isinstance(geo, R.Geo) and len(geo.rows) < 100000:
        assert [(int(r["asn"]), int(r["country"]).to_bytes(2, "little").decode()) for r in t.geo_recs[1:]] == [(a, c) for _, a, c in geo.rows]
    return stats, t


def random4(seed, n=100000):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------
# 3. table shapes
# ---------------------------------------------------------------------------------------------------------
def test_run_records_every_start_count_and_carry(tmp_path):
    p = AC.runs_prefixes()
    rows = AC.geo_rows(p)
    addrs = np.concatenate([AC.edges4(p), AC.whole_16s(10 << 8, (11 << 8) | 1, (12 << 8) | 7), random4(1)])
    for no_summary in (False, True):
        stats, _ = check_case(tmp_path, rows, {}, addrs, no_summary=no_summary)
        h = stats["starts_hist"]
        assert h[32] == 8 and h[0] > 0 and h[1] > 0 and h[2] > 0 and h[3] > 0, h
        assert stats["starts_at_bit0"] > 0 and stats["starts_at_bit31"] > 0
        assert all(c > 0 for c in stats["cross_hist"][1:8]), stats["cross_hist"]  # runs carried across 1 ... 7 group boundaries
        assert stats["runs_across_16"] >= 1
        assert stats["n_vals"] >= 8 * 30 and stats["escapes"] == 0
        assert stats["has_summary"] == (0 if no_summary else 1) and stats["common"] == 0
    # the 11.1/16 groups, one by one: 1, 0, 0, 0, 1, 2, 3, 1 starts
    flat = np.zeros(1 << 24, dtype=np.uint32)
    t = ((11 << 8) | 1) << 8
    flat[t:t + 128] = 5
    flat[t + 170] = 6
    flat[t + 200] = 7
    flat[t + 222:t + 224] = 8
    stats, e24, _, _ = run_harness(tmp_path, flat=flat)
    assert (e24 == flat).all()
    assert stats["starts_hist"][:4] == [3 + 65535 * 7, 3 + 65535, 1, 1], stats["starts_hist"][:4]


def test_every_prefix_length_nesting_adjacency_and_both_ends(tmp_path):
    p = AC.lengths_geo_prefixes()
    lists = AC.lengths_lists()
    assert {R.parse_prefix(x)[2] for x in p} == set(range(33)) and {R.parse_prefix(x)[2] for x in lists["even"] + lists["odd"]} == set(range(33))
    every = p + [x for items in lists.values() for x in items]
    addrs = np.concatenate([AC.edges4(every), AC.whole_16s((30 << 8), (200 << 8) | 100, (255 << 8) | 255, 0), random4(2)])
    stats, t = check_case(tmp_path, AC.geo_rows(p), lists, addrs)
    assert stats["esc_len_geo"] > 0 and stats["esc_len_list"] > 0 and stats["escapes"] < 64


def test_escapes_by_prefix_length(tmp_path):
    geo, lists = AC.escape_case()
    every = geo + [x for items in lists.values() for x in items]
    addrs = np.concatenate([AC.edges4(every), random4(3)])
    for no_summary in (False, True):
        stats, _ = check_case(tmp_path, AC.geo_rows(geo), lists, addrs, no_summary=no_summary)
        assert stats["esc_len_geo"] >= 4 and stats["esc_len_list"] >= 4 and stats["esc_len_both"] >= 2 and stats["esc_id_class"] == 0 and stats["esc_id_set"] == 0, stats
    # one trie alone
    stats, _ = check_case(tmp_path, AC.geo_rows(geo), {}, addrs)
    assert stats["esc_len_geo"] >= 6 and stats["esc_len_list"] == 0
    stats, _ = check_case(tmp_path, None, lists, addrs)
    assert stats["esc_len_list"] >= 6 and stats["esc_len_geo"] == 0


@pytest.mark.parametrize("n", [16, 17])
def test_escapes_by_membership_set_id(tmp_path, n):
    lists = AC.bit_lists(n)
    assert sum(len(v) for v in lists.values()) == (1 << n) - 1
    region = (np.arange(1 << n, dtype=U) << U(8)) + U(AC.BITS_BASE)
    addrs = np.concatenate([region, region + U(255), random4(4), AC.edges4(["64.0.0.0/%d" % (24 - n)])])
    stats, t = check_case(tmp_path, None, lists, addrs)
    n_sets = len(t.set_masks) // t.set_words
    assert n_sets == 1 << n
    # sets from 32768 on do not fit the packed entry; every /24 of the region is a run of its own
    assert stats["esc_id_set"] == stats["escapes"] == (1 << n) - 32768 and stats["esc_len_list"] == 0
    assert stats["starts_hist"][32] == (1 << n) // 32
    # an escaped /24 has an index of its own, so no two escape entries are equal and none can be the most common entry
    assert stats["has_summary"] == 1 and stats["common"] == 0
    # the region's membership is one bit test
    got = run_harness(tmp_path, t, addrs=region[::37], per24=False)[3][:, 1].astype(np.int64)
    masks = np.asarray(t.set_masks, dtype=np.uint32)[got * t.set_words]
    assert (masks == np.arange(1 << n, dtype=np.uint32)[::37]).all()


def test_escapes_by_record_id(tmp_path):
    """2^17 /24 records: on the CPU the trie's leaves are record ids (the engine maps them to classes first), so ids from 65536 on take
    the escape the engine takes for more than 65536 classes."""
    n = 1 << 17
    geo = np.zeros(n, dtype=GEOIP_DTYPE)
    vals = (np.arange(n, dtype=np.uint32) << 8) + np.uint32(AC.BITS_BASE)
    geo["addr"][:, :4] = vals.astype(">u4").view(np.uint8).reshape(n, 4)
    geo["prefix_len"], geo["country"], geo["asn"] = 24, np.frombuffer(b"QQ", dtype=np.uint8), np.arange(n)
    t = compile_case(None, None, geo_array=geo)

    class Ref:  # rows by the by-length lookup over arrays
        def lookup4(self, a, brute=False):
            out = R.lpm4(a, (vals.astype(U), np.full(n, 24), np.arange(n)))
            out[R.geo_excluded4(a)] = -1
            return out

    stats, _ = check_case(tmp_path, None, {}, np.concatenate([vals.astype(U)[::5] + U(7), random4(5)]), geo_ref=Ref(), tables=t)
    assert stats["esc_id_class"] == stats["escapes"] == n - 65535 and stats["esc_len_geo"] == 0  # (record 0 is the default: row r is record r + 1)
    assert stats["has_summary"] == 1 and stats["common"] == 0


@pytest.mark.parametrize("s", [0, 1, 2, 3, 4])
def test_summary_granularity_is_chosen_by_cost(tmp_path, s):
    """cost of a granularity = (share of its blocks that need the table) + 2^(-2-shift); more than half of the blocks uncommon: not
    eligible. Blocks of 2^s /24s alternating over 60 % of the space: finer granularities cost more, coarser ones are not eligible."""
    flat = AC.summary_flat(s)
    stats, e24, _, _ = run_harness(tmp_path, flat=flat)
    assert (e24 == flat).all()
    assert stats["has_summary"] == 1 and stats["shift"] == s and stats["common"] == 0, stats
    assert stats["summary_set"] == int(0.6 * (1 << (24 - s))) // 2
    stats, e24, _, _ = run_harness(tmp_path, flat=flat, no_summary=True)
    assert (e24 == flat).all() and stats["has_summary"] == 0


@pytest.mark.parametrize("s", [0, 1, 2, 3, 4])
def test_summary_granularity_on_compiled_tries(tmp_path, s):
    vals, length = AC.summary_prefix_arrays(s)
    n = len(vals)
    geo = np.zeros(n, dtype=GEOIP_DTYPE)
    geo["addr"][:, :4] = vals.astype(">u4").view(np.uint8).reshape(n, 4)
    geo["prefix_len"], geo["country"], geo["asn"] = length, np.frombuffer(b"QQ", dtype=np.uint8), np.arange(n) & 0xFFFFFFFF
    t = compile_case(None, None, geo_array=geo)

    class Ref:
        def lookup4(self, a, brute=False):
            out = R.lpm4(a, (vals, np.full(n, length), np.arange(n)))
            out[R.geo_excluded4(a)] = -1
            return out

    stats, _ = check_case(tmp_path, None, {}, random4(6 + s), geo_ref=Ref(), tables=t)
    assert n == {0: 5033164, 1: 2516582, 2: 1258291, 3: 629145, 4: 314572}[s]
    assert stats["has_summary"] == 1 and stats["shift"] == s and stats["common"] == 0, stats


def test_no_summary_when_most_of_the_space_is_uncommon_and_a_common_entry_that_is_not_zero(tmp_path):
    # four /2s with a record each: whatever is most common covers a quarter, three quarters of the blocks need the table
    rows = AC.geo_rows(["0.0.0.0/2", "64.0.0.0/2", "128.0.0.0/2", "192.0.0.0/2"])
    stats, _ = check_case(tmp_path, rows, {}, np.concatenate([AC.edges4([r[0] for r in rows]), random4(7)]))
    assert stats["has_summary"] == 0 and stats["shift"] == 0 and stats["common"] == 0
    # a /1 and a /2 under records, the rest empty: the most common entry is the /1's record
    rows = AC.geo_rows(["128.0.0.0/2", "0.0.0.0/1"])
    lists = {"l": ["0.0.0.0/1", "200.1.2.0/24"]}
    stats, t = check_case(tmp_path, rows, lists, np.concatenate([AC.edges4([r[0] for r in rows] + lists["l"]), random4(8)]))
    assert stats["has_summary"] == 1 and stats["shift"] == 4, stats
    assert stats["common"] & 0xFFFF == 2 and stats["common"] >> 16 != 0  # record 2 = the second row; the set {l}
    stats, _ = check_case(tmp_path, rows, lists, random4(9), no_summary=True)
    assert stats["has_summary"] == 0


def test_ipv6_tries_every_length_shared_byte_index_and_empty_families(tmp_path):
    geo, lists = AC.v6_case()
    every = geo + [x for items in lists.values() for x in items]
    assert {R.parse_prefix(x)[2] for x in every} >= set(range(129))
    rng = random.Random(21)
    _, deep = R.parse_addr(AC.V6_DEEP)
    a6 = AC.edges6(every) + [deep ^ (1 << k) for k in range(128)] + [rng.getrandbits(128) for _ in range(2000)] + [1, 0, (1 << 128) - 1, 0xFF << 120, R.parse_v6("ff02::1")]
    stats, _ = check_case(tmp_path, AC.geo_rows(geo), lists, random4(10, 1000), a6)
    assert stats["dir"] == 0  # no IPv4 prefix anywhere: no table, IPv4 addresses read the default record through the roots
    # IPv4-only lists beside an IPv6-only GeoIP table, and the reverse: the empty family answers the default record / the empty set
    l4 = {"a": ["10.0.0.0/8"], "b": ["10.1.2.3", "10.1.2.128/25"]}
    stats, _ = check_case(tmp_path, AC.geo_rows(geo), l4, np.concatenate([AC.edges4(l4["a"] + l4["b"]), random4(11, 1000)]), a6)
    assert stats["dir"] == 1 and stats["esc_len_list"] == 1
    g4 = ["10.0.0.0/8", "10.1.2.0/25", "0.0.0.0/0"]
    stats, _ = check_case(tmp_path, AC.geo_rows(g4), lists, np.concatenate([AC.edges4(g4), random4(12, 1000)]), a6)
    assert stats["dir"] == 1 and stats["esc_len_geo"] == 1
