"""GeoIP answers on the CPU (no device): the ABI additions, and the record tables of PWAF_OPT_GEO_ANSWERS — the record-leaf trie of a
program dump -> csrc/georec.h's flattening -> csrc/dirtable.h's run compression and summary choice (the headers pwaf_engine_create
calls) -> the scalar restatement of georec_kernel's lookup — for ALL 2^24 /24s, all 256 addresses of every /24 that holds a longer
prefix, the edge addresses, 100 000 random addresses and IPv6 pools, against the brute-force reference of tests/lpm_reference.py.
The host harness is tests/georec_host.cpp; the table shapes are those of tests/address_cases.py."""
import ctypes as C
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import address_cases as AC
import lpm_reference as R
from pingoo_amd import _abi, engine
from pingoo_amd.batch import GEO_DTYPE, GEOIP_DTYPE, geoip_entries
from pingoo_amd.engine import CompiledProgram
from table_walker import Tables

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "georec_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "pingoo_amd", "csrc", "georec.h"), os.path.join(ROOT, "pingoo_amd", "csrc", "dirtable.h")]
U = np.uint64
ESCAPE = 0x80000000
NEW_SYMBOLS = ["pwaf_geoip_lookup", "pwaf_evaluate_batch_geo", "pwaf_evaluate_device_geo", "pwaf_evaluate_records_geo", "pwaf_evaluate_one_geo", "pwaf_async_create_geo",
               "pwaf_async_poll_geo", "pwaf_engine_geo_answer_tables"]


# ---------------------------------------------------------------------------------------------------------
# 1. the interface
# ---------------------------------------------------------------------------------------------------------
def test_pwaf_geo_layout_against_the_c_compiler(tmp_path):
    prog = tmp_path / "geo.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pwaf.h"\nint main(void){printf("%zu %zu %zu %zu %u %u\\n", sizeof(pwaf_geo), offsetof(pwaf_geo, asn), '
                    'offsetof(pwaf_geo, country), offsetof(pwaf_geo, reserved), PWAF_OPT_GEO_ANSWERS, PWAF_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "geo"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [8, 0, 4, 6, 256, 4]
    assert C.sizeof(_abi.Geo) == 8 and (_abi.Geo.asn.offset, _abi.Geo.country.offset, _abi.Geo.reserved.offset) == (0, 4, 6)
    assert GEO_DTYPE.itemsize == 8 and [GEO_DTYPE.fields[k][1] for k in ("asn", "country", "reserved")] == [0, 4, 6]
    assert _abi.OPT_GEO_ANSWERS == 256 and _abi.ABI_VERSION == 4 and engine.lib().pwaf_abi_version() == 4


def test_flag_collides_with_no_other_flag():
    src = open(os.path.join(ROOT, "include", "pwaf.h")).read()
    flags = {name: int(val) for name, val in re.findall(r"#define (PWAF_OPT_[A-Z0-9_]+)\s+(\d+)u", src)}
    assert flags["PWAF_OPT_GEO_ANSWERS"] == 256 and len(flags) >= 17
    for name, val in flags.items():
        assert val & (val - 1) == 0, name
        assert name == "PWAF_OPT_GEO_ANSWERS" or val != 256, name
    assert len(set(flags.values())) == len(flags)
    mine = {k: v for k, v in vars(_abi).items() if k.startswith("OPT_")}
    assert all(flags["PWAF_" + k] == v for k, v in mine.items())


def test_new_symbols_are_exported_and_declared():
    L = engine.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pwaf.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, src), name


def test_null_arguments_need_no_device():
    L = engine.lib()
    one = np.zeros(16, dtype=np.uint8)
    assert L.pwaf_geoip_lookup(None, one.ctypes.data, one.ctypes.data, 1, _abi.MEM_HOST, one.ctypes.data, None) == _abi.E_INVALID_ARG
    assert b"NULL" in L.pwaf_last_error()
    assert L.pwaf_evaluate_batch_geo(None, None, None, None, None) == _abi.E_INVALID_ARG
    assert L.pwaf_evaluate_device_geo(None, None, None, None, None, None, None, None) == _abi.E_INVALID_ARG
    assert L.pwaf_evaluate_records_geo(None, None, 0, None, 0, None, None, None) == _abi.E_INVALID_ARG
    assert L.pwaf_evaluate_one_geo(None, None, None, None) == _abi.E_INVALID_ARG
    h = C.c_void_p()
    assert L.pwaf_async_create_geo(None, 16, 100, 16, C.byref(h)) == _abi.E_INVALID_ARG and not h.value
    assert L.pwaf_async_poll_geo(None, None, None, 4) == 0
    out = (C.c_uint32 * 8)()
    assert L.pwaf_engine_geo_answer_tables(None, out) == _abi.E_INVALID_ARG


# ---------------------------------------------------------------------------------------------------------
# 2. the harness
# ---------------------------------------------------------------------------------------------------------
def tool():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "georec_host")
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", SRC, "-o", out], check=True)
    return out


def run_harness(tmp_path, dump, a4=(), a6=(), no_summary=False, per24=True):
    """-> (stats, per24[2^24] or None, ids[n], geo[n] as GEO_DTYPE); IPv4 addresses (uint64 array) first, then IPv6 (ints)"""
    a4 = np.asarray(a4, dtype=U).astype(">u4")
    rec = np.zeros((len(a4) + len(a6), 20), dtype=np.uint8)
    rec[:len(a4), :4] = a4.view(np.uint8).reshape(-1, 4)
    for i, v in enumerate(a6):
        rec[len(a4) + i, :16] = np.frombuffer(v.to_bytes(16, "big"), dtype=np.uint8)
        rec[len(a4) + i, 16] = 1
    fd, fa, fo = (str(tmp_path / k) for k in ("geo.dump", "geo.addr", "geo.out"))
    open(fd, "wb").write(dump)
    rec.tofile(fa)
    r = subprocess.run([tool(), fd, fa, fo, str((1 if no_summary else 0) | (8 if per24 else 0))], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    stats = json.loads(r.stdout)
    out = np.fromfile(fo, dtype="<u4")
    for f in (fd, fa, fo):
        os.remove(f)
    p24 = None
    if per24 and stats["dir"]:
        p24, out = out[:1 << 24], out[1 << 24:]
    out = out.reshape(-1, 3)
    assert stats["out_of_range"] == 0, stats
    return stats, p24, out[:, 0], np.ascontiguousarray(out[:, 1:]).view(GEO_DTYPE).reshape(-1)


def compile_dump(geo_rows=None, geo_array=None):
    geo = geo_array if geo_array is not None else (geoip_entries(geo_rows) if geo_rows is not None else None)
    return CompiledProgram([("r", "client.remote_port == 1", [_abi.RULE_ACTION_BLOCK])], {}, geo).dump()


def valid_country(c) -> bool:
    c = c.encode("latin-1") if isinstance(c, str) else bytes(c)
    return len(c) == 2 and all(65 <= b <= 90 for b in c)


class Want:
    """row index (lpm_reference: -1 = none) -> the record the engine must answer. The reference's Geo.record does not know that a row whose
    country is not two letters A-Z reads the default record (csrc/compile.cpp maps it to record 0; http_listener.rs:148-153): mapped here."""

    def __init__(self, asns, countries):
        n = len(asns)
        self.tab = np.zeros(n + 1, dtype=GEO_DTYPE)
        self.tab["country"][0] = b"XX"
        for i in range(n):
            ok = valid_country(countries[i])
            self.tab["asn"][i + 1] = asns[i] if ok else 0
            self.tab["country"][i + 1] = (countries[i].encode("latin-1") if isinstance(countries[i], str) else bytes(countries[i])) if ok else b"XX"

    def __call__(self, rows):
        return self.tab[np.asarray(rows, dtype=np.int64) + 1]


def same(got, want):
    return (got["asn"] == want["asn"]) & (got["country"] == want["country"]) & (got["reserved"] == 0)


def random4(seed, n=100000):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64)


ALL24 = None


def all24():
    global ALL24
    if ALL24 is None:
        ALL24 = np.arange(1 << 24, dtype=U) << U(8)
    return ALL24


def check_case(tmp_path, geo_rows, addrs4=(), addrs6=(), no_summary=False, ref=None, want=None, dump=None, deep=None, deep24_limit=4096):
    """Compiles the table, runs the harness and compares every /24, all 256 addresses of every /24 that holds a longer prefix, the given
    addresses and 100 000 random ones with the reference. -> stats"""
    geo = ref if ref is not None else R.Geo(geo_rows)
    if want is None:
        want = Want([r[1] for r in geo.rows], [r[2] for r in geo.rows])
    if dump is None:
        dump = compile_dump(geo_rows)
    if deep is None:
        deep = {v >> 8 for v, ln, _ in geo.p4 if ln > 24}
    assert len(deep) <= deep24_limit
    extra = (np.repeat(np.array(sorted(deep), dtype=U) << U(8), 256) + np.tile(np.arange(256, dtype=U), len(deep))) if deep else np.zeros(0, dtype=U)
    a4 = np.unique(np.concatenate([np.asarray(addrs4, dtype=U), extra, random4(len(deep) + 17)]))
    a6 = list(addrs6)
    stats, p24, ids, got = run_harness(tmp_path, dump, a4, a6, no_summary=no_summary)
    recs = Tables(dump).geo_recs
    assert stats["records"] == len(recs)
    # the harness's records are the dump's
    assert (got["asn"] == recs["asn"][ids]).all() and (got["country"].view("<u2") == recs["country"][ids]).all()
    if stats["dir"]:
        esc = (p24 & np.uint32(ESCAPE)) != 0
        assert stats["escapes"] == int(esc.sum()) and set(np.nonzero(esc)[0].tolist()) <= deep
        w = want(geo.lookup4(all24()))
        g = np.zeros(1 << 24, dtype=GEO_DTYPE)
        plain = ~esc
        g["asn"][plain] = recs["asn"][p24[plain]]
        g["country"][plain] = recs["country"][p24[plain]].astype("<u2").view("S2")
        bad = np.nonzero(~same(g, w) & plain)[0]
        assert len(bad) == 0, f"{len(bad)} /24s differ; first {R.fmt_addr(False, int(bad[0]) << 8)}: got {g[bad[0]]} want {w[bad[0]]}"
    w4 = want(geo.lookup4(a4))
    bad = np.nonzero(~same(got[:len(a4)], w4))[0]
    assert len(bad) == 0, f"{len(bad)} addresses differ; first {R.fmt_addr(False, int(a4[bad[0]]))}: got {got[bad[0]]} want {w4[bad[0]]}"
    if a6:
        w6 = want(geo.lookup6(*R.v6_arrays(a6)))
        bad = np.nonzero(~same(got[len(a4):], w6))[0]
        assert len(bad) == 0, f"{len(bad)} IPv6 addresses differ; first {R.fmt_addr(True, a6[bad[0]])}: got {got[len(a4) + bad[0]]} want {w6[bad[0]]}"
    return stats


# ---------------------------------------------------------------------------------------------------------
# 3. table shapes (tests/address_cases.py)
# ---------------------------------------------------------------------------------------------------------
def test_run_records_every_start_count_and_carry(tmp_path):
    p = AC.runs_prefixes()
    addrs = np.concatenate([AC.edges4(p), AC.whole_16s(10 << 8, (11 << 8) | 1, (12 << 8) | 7), random4(1)])
    for no_summary in (False, True):
        stats = check_case(tmp_path, AC.geo_rows(p), addrs, no_summary=no_summary)
        assert stats["dir"] == 1 and stats["n_vals"] >= 8 * 30 and stats["escapes"] == 0
        assert stats["has_summary"] == (0 if no_summary else 1) and stats["common"] == 0


def test_every_prefix_length_nesting_adjacency_both_ends_and_later_duplicates(tmp_path):
    p = AC.lengths_geo_prefixes()
    assert {R.parse_prefix(x)[2] for x in p} == set(range(33)) and len(set(p)) < len(p)  # (the same prefixes twice: the later row wins)
    addrs = np.concatenate([AC.edges4(p), AC.whole_16s((30 << 8), (200 << 8) | 100, (255 << 8) | 255, 0), random4(2)])
    stats = check_case(tmp_path, AC.geo_rows(p), addrs)
    assert 0 < stats["escapes"] < 64
    # 0.0.0.0/0 carries a record: the most common entry is not record 0, and loopback / multicast below it still read the default
    assert stats["common"] != 0 or stats["has_summary"] == 0


def test_escapes_by_prefix_length(tmp_path):
    geo, _ = AC.escape_case()
    addrs = np.concatenate([AC.edges4(geo), random4(3)])
    for no_summary in (False, True):
        stats = check_case(tmp_path, AC.geo_rows(geo), addrs, no_summary=no_summary)
        assert stats["escapes"] >= 6, stats


@pytest.mark.parametrize("s", [0, 1, 2, 3, 4])
def test_summary_granularity_on_compiled_tries(tmp_path, s):
    vals, length = AC.summary_prefix_arrays(s)
    n = len(vals)
    geo = np.zeros(n, dtype=GEOIP_DTYPE)
    geo["addr"][:, :4] = vals.astype(">u4").view(np.uint8).reshape(n, 4)
    geo["prefix_len"], geo["country"], geo["asn"] = length, np.frombuffer(b"QQ", dtype=np.uint8), np.arange(n) & 0xFFFFFFFF

    class Ref:
        rows, p4 = (), ()

        def lookup4(self, a, brute=False):
            out = R.lpm4(a, (vals, np.full(n, length), np.arange(n)))
            out[R.geo_excluded4(a)] = -1
            return out

    class W:
        tab = np.zeros(n + 1, dtype=GEO_DTYPE)

        def __call__(self, rows):
            return self.tab[np.asarray(rows, dtype=np.int64) + 1]

    W.tab["asn"][1:] = np.arange(n)
    W.tab["country"][1:] = b"QQ"
    W.tab["country"][0] = b"XX"
    stats = check_case(tmp_path, None, random4(6 + s), ref=Ref(), want=W(), dump=compile_dump(geo_array=geo), deep=set())
    assert stats["has_summary"] == 1 and stats["shift"] == s and stats["common"] == 0, stats
    if s == 2:
        stats = check_case(tmp_path, None, random4(60), ref=Ref(), want=W(), dump=compile_dump(geo_array=geo), deep=set(), no_summary=True)
        assert stats["has_summary"] == 0


def test_no_summary_when_most_of_the_space_is_uncommon_and_a_common_entry_that_is_not_record_0(tmp_path):
    rows = AC.geo_rows(["0.0.0.0/2", "64.0.0.0/2", "128.0.0.0/2", "192.0.0.0/2"])
    stats = check_case(tmp_path, rows, AC.edges4([r[0] for r in rows]))
    assert stats["has_summary"] == 0 and stats["shift"] == 0 and stats["common"] == 0
    rows = AC.geo_rows(["128.0.0.0/2", "0.0.0.0/1", "200.1.2.0/24"])
    stats = check_case(tmp_path, rows, AC.edges4([r[0] for r in rows]))
    assert stats["has_summary"] == 1 and stats["shift"] == 4 and stats["common"] == 2, stats  # record 2 = the second row
    stats = check_case(tmp_path, rows, random4(9), no_summary=True)
    assert stats["has_summary"] == 0


def test_more_than_65536_records(tmp_path):
    """2^17 /24 records: the class table of ipres_kernel escapes ids from 65536 on; a record table entry IS the id, so nothing escapes"""
    n = 1 << 17
    geo = np.zeros(n, dtype=GEOIP_DTYPE)
    vals = (np.arange(n, dtype=np.uint32) << 8) + np.uint32(AC.BITS_BASE)
    geo["addr"][:, :4] = vals.astype(">u4").view(np.uint8).reshape(n, 4)
    geo["prefix_len"], geo["country"], geo["asn"] = 24, np.frombuffer(b"QQ", dtype=np.uint8), np.arange(n) + 7

    class Ref:
        rows, p4 = (), ()

        def lookup4(self, a, brute=False):
            out = R.lpm4(a, (vals.astype(U), np.full(n, 24), np.arange(n)))
            out[R.geo_excluded4(a)] = -1
            return out

    class W:
        tab = np.zeros(n + 1, dtype=GEO_DTYPE)

        def __call__(self, rows):
            return self.tab[np.asarray(rows, dtype=np.int64) + 1]

    W.tab["asn"][1:] = np.arange(n) + 7
    W.tab["country"][1:] = b"QQ"
    W.tab["country"][0] = b"XX"
    stats = check_case(tmp_path, None, np.concatenate([vals.astype(U)[::5] + U(7), random4(5)]), ref=Ref(), want=W(), dump=compile_dump(geo_array=geo), deep=set())
    assert stats["records"] == n + 1 and stats["escapes"] == 0 and stats["has_summary"] == 1 and stats["common"] == 0


def test_ipv6_every_length_and_empty_families(tmp_path):
    geo, _ = AC.v6_case()
    assert {R.parse_prefix(x)[2] for x in geo} >= set(range(0, 129, 3))
    rng = random.Random(21)
    _, deep = R.parse_addr(AC.V6_DEEP)
    a6 = AC.edges6(geo) + [deep ^ (1 << k) for k in range(128)] + [rng.getrandbits(128) for _ in range(2000)] + [1, 0, (1 << 128) - 1, 0xFF << 120, R.parse_v6("ff02::1")]
    # every length 0..128 along one address
    every = geo + AC.chain6(AC.V6_DEEP, range(129))
    assert {R.parse_prefix(x)[2] for x in every} >= set(range(129))
    stats = check_case(tmp_path, AC.geo_rows(every), random4(10, 1000), a6 + AC.edges6(every))
    assert stats["dir"] == 0  # no IPv4 prefix: no table, IPv4 addresses read the default record
    # an IPv4-only table: IPv6 clients read the default record
    g4 = ["10.0.0.0/8", "10.1.2.0/25", "0.0.0.0/0"]
    stats = check_case(tmp_path, AC.geo_rows(g4), AC.edges4(g4), a6)
    assert stats["dir"] == 1 and stats["escapes"] == 1
    # both families
    stats = check_case(tmp_path, AC.geo_rows(g4 + geo), AC.edges4(g4), a6)
    assert stats["dir"] == 1
    # no table at all
    stats, _, ids, got = run_harness(tmp_path, compile_dump(None), random4(12, 1000), a6[:100])
    assert stats["dir"] == 0 and stats["records"] == 1 and (ids == 0).all() and (got["asn"] == 0).all() and (got["country"] == b"XX").all()


def test_duplicates_later_wins_and_invalid_country_reads_the_default(tmp_path):
    rows = [("9.9.0.0/16", 1, "AA"), ("9.9.0.0/16", 2, "BB"), ("9.0.0.0/8", 3, "CC"), ("9.0.0.0/8", 4, "DD"), ("127.0.0.0/8", 5, "EE"), ("::/0", 6, "FF"), ("::/0", 7, "GG"),
            ("0.0.0.0/0", 8, "HH"), ("9.9.9.0/24", 9, "x1"), ("9.9.9.128/25", 10, "II"), ("9.9.10.64/26", 11, "zz"), ("2001:db8::/32", 12, "a?"), ("2001:db8:1::/48", 13, "JJ")]
    a4 = np.array([R.parse_v4(x) for x in ("9.9.1.1", "9.8.1.1", "127.0.0.1", "224.0.0.1", "239.255.255.255", "240.0.0.0", "126.255.255.255", "128.0.0.0", "9.9.9.1", "9.9.9.129",
                                           "9.9.10.63", "9.9.10.64", "9.9.10.127", "9.9.10.128")], dtype=U)
    a6 = [R.parse_v6(x) for x in ("::1", "::2", "ff02::1", "feff::1", "::", "2001:db8::1", "2001:db8:1::1", "2001:db9::")]
    check_case(tmp_path, rows, np.concatenate([a4, AC.edges4([r[0] for r in rows])]), a6 + AC.edges6([r[0] for r in rows]))
    dump = compile_dump(rows)
    _, _, _, got = run_harness(tmp_path, dump, a4, a6, per24=False)
    g = [(int(r["asn"]), r["country"].decode()) for r in got]
    assert g[:len(a4)] == [(2, "BB"), (4, "DD"), (0, "XX"), (0, "XX"), (0, "XX"), (8, "HH"), (8, "HH"), (8, "HH"), (0, "XX"), (10, "II"), (2, "BB"), (0, "XX"), (0, "XX"), (2, "BB")]
    assert g[len(a4):] == [(0, "XX"), (7, "GG"), (0, "XX"), (7, "GG"), (7, "GG"), (0, "XX"), (13, "JJ"), (7, "GG")]
