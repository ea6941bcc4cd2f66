"""GeoIP answers on the device (PWAF_OPT_GEO_ANSWERS): georec_kernel through pwaf_geoip_lookup against the brute-force reference
(tests/lpm_reference.py) on every address and against the oracle's geoip_lookup on all of them or a fixed sample; every entry point
(batch, device, records, one, async queue) gives that record beside the verdicts of its plain counterpart; the rules see the record that
is returned; caller-supplied columns are echoed; defaults; the flag's and NULL's behaviour; verdicts do not depend on the flag.
Table shapes: tests/address_cases.py, as in tests/test_geo_answers_cpu.py; every case asserts on pwaf_engine_geo_answer_tables that the
path it was written for exists."""
import random
import time

import numpy as np
import pytest

import address_cases as AC
import helpers as H
import lpm_reference as R
from oracle import pyoracle
from pingoo_amd import Request, RequestBatch, _abi, geoip_entries
from pingoo_amd.batch import GEO_DTYPE, GEOIP_DTYPE
from pingoo_amd.engine import AsyncBatcher, DeviceBatch, PwafError, RuleEngine, UnsupportedExpression
from test_gpu_addresses import Pool, make_batch, pool_for, random4

pytestmark = pytest.mark.gpu
B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
U = np.uint64
GEO = _abi.OPT_GEO_ANSWERS
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1025]
GEOREC_U, GEOREC_BLOCKS_PER_CU = 4, 8  # georec_kernel: requests a lane walks in lockstep; launch_georec: at most 8 workgroups of 256 per CU
ORACLE_ALL, ORACLE_SAMPLE = 50000, 20000
ANY_RULE = [("r", "client.remote_port == 1", [B])]


def valid_country(c: str) -> bool:
    return len(c) == 2 and all("A" <= ch <= "Z" for ch in c)


def record_table(rows):
    """row index + 1 -> record (0: the default). A row whose country is not two letters A-Z reads the default record (csrc/compile.cpp;
    http_listener.rs:148-153) — lpm_reference.Geo.record does not know this rule."""
    tab = np.zeros(len(rows) + 1, dtype=GEO_DTYPE)
    tab["country"][0] = b"XX"
    for i, (_, asn, cc) in enumerate(rows):
        ok = valid_country(cc)
        tab["asn"][i + 1], tab["country"][i + 1] = (asn, cc.encode()) if ok else (0, b"XX")
    return tab


def same(got, want):
    return (got["asn"] == want["asn"]) & (got["country"] == want["country"]) & (got["reserved"] == 0)


def assert_same(label, got, want, describe=lambda j: str(j)):
    assert len(got) == len(want)
    bad = np.nonzero(~same(got, want))[0]
    assert len(bad) == 0, f"{label}: {len(bad)} of {len(want)} records differ; first at {bad[0]}: {describe(int(bad[0]))} got {got[bad[0]]} want {want[bad[0]]}"


def oracle_records(oracle, pool, idx):
    out = np.zeros(len(idx), dtype=GEO_DTYPE)
    for k, j in enumerate(idx):
        out["asn"][k], out["country"][k] = oracle.geoip_lookup(pool.ip[j].tobytes(), bool(pool.v6[j]))
    return out


def lookup_case(label, geo, want, pool, hook):
    """Engines with and without the summary: pwaf_geoip_lookup over the pool equals the reference everywhere, the oracle on all addresses
    or a fixed sample, and at the small batch sizes."""
    for flags in (0, _abi.OPT_NO_DIR_SUMMARY):
        t0 = time.time()
        eng = RuleEngine(ANY_RULE, None, geo, flags=GEO | flags)
        t = eng.geo_answer_tables()
        print(f"{label}: engine created in {time.time() - t0:.2f} s (flags {flags}); {pool.n} addresses; tables {t}")
        hook(t, bool(flags))
        assert t["has_summary"] == 0 or not flags
        assert t["zero"] == 0
        got = eng.lookup_geoip(pool.ip, pool.v6)
        assert_same(f"{label} (flags {flags})", got, want, pool.text)
        if not flags:
            idx = np.arange(pool.n) if pool.n < ORACLE_ALL else np.sort(np.random.default_rng(7).choice(pool.n, ORACLE_SAMPLE, replace=False))
            assert_same(f"{label}: oracle", oracle_records(pyoracle.Oracle(ANY_RULE, None, geo), pool, idx), want[idx], lambda k: pool.text(int(idx[k])))
        for size in SIZES:
            if size <= pool.n:
                assert_same(f"{label}: {size} addresses", eng.lookup_geoip(pool.ip[:size], pool.v6[:size]), want[:size], pool.text)
        eng.close()


def rows_case(label, rows, pool, hook):
    want = record_table(rows)[pool.geo_rows(R.Geo(rows)) + 1]
    assert len(np.unique(want)) >= min(len(rows), 8)
    lookup_case(label, geoip_entries(rows), want, pool, hook)
    return want


def table(min_escapes=0, max_escapes=None, summary=None, common=None, min_vals=1):
    def hook(t, no_summary):
        assert t["has_table"] == 1 and t["n_vals"] >= min_vals and t["escapes"] >= min_escapes, t
        assert max_escapes is None or t["escapes"] <= max_escapes, t
        if not no_summary and summary is not None:
            assert t["has_summary"] == summary, t
        if not no_summary and common is not None:
            assert (t["common"] == 0) == (common == 0), t
    return hook


# ---------------------------------------------------------------------------------------------------------
# 1. the lookup against the references
# ---------------------------------------------------------------------------------------------------------
def test_run_records_every_start_count_and_carry():
    p = AC.runs_prefixes()
    rows_case("runs", AC.geo_rows(p), pool_for(p, 1, whole=(10 << 8, (11 << 8) | 1, (12 << 8) | 7)), table(max_escapes=0, summary=1, common=0, min_vals=8 * 30))


def test_every_prefix_length_both_ends_adjacency_and_later_duplicates():
    p = AC.lengths_geo_prefixes()
    want = rows_case("lengths", AC.geo_rows(p), pool_for(p, 2, whole=(30 << 8, (200 << 8) | 100, (255 << 8) | 255, 0)), table(min_escapes=3, max_escapes=63))
    # 0.0.0.0/0 occurs twice with records of their own: nothing but loopback / multicast reads the default, and those do
    assert (want["country"] == b"XX").sum() > 0 and (want["country"] != b"XX").sum() > len(want) // 2


def test_escapes_by_prefix_length():
    geo, _ = AC.escape_case()
    deep = sorted({R.parse_prefix(x)[1] >> 8 for x in geo if R.parse_prefix(x)[2] > 24})
    inside = np.repeat(np.array(deep, dtype=U) << U(8), 256) + np.tile(np.arange(256, dtype=U), len(deep))  # every address of every escaped /24
    rows_case("escapes", AC.geo_rows(geo), Pool(np.concatenate([AC.edges4(geo), inside, random4(3)]), [], 5), table(min_escapes=len(deep), max_escapes=len(deep)))


@pytest.mark.parametrize("s", [0, 1, 2, 3, 4])
def test_summary_granularity(s):
    vals, length = AC.summary_prefix_arrays(s)
    n = len(vals)
    geo = np.zeros(n, dtype=GEOIP_DTYPE)
    geo["addr"][:, :4] = vals.astype(">u4").view(np.uint8).reshape(n, 4)
    geo["prefix_len"], geo["country"], geo["asn"] = length, np.frombuffer(b"QQ", dtype=np.uint8), np.arange(n) + 1
    edge = vals[:: max(1, n // 20000)]
    a4 = np.concatenate([edge, edge - U(1), edge + U((1 << (32 - length)) - 1), edge + U(1 << (32 - length)), random4(13 + s)])
    pool = Pool(a4, [1], 13)
    row = R.lpm4(pool.a4, (vals, np.full(n, length), np.arange(n)))
    row[R.geo_excluded4(pool.a4)] = -1
    want = np.zeros(pool.n, dtype=GEO_DTYPE)
    want["country"] = b"XX"
    w4 = np.zeros(len(row), dtype=GEO_DTYPE)
    w4["asn"], w4["country"] = np.where(row >= 0, row + 1, 0), np.where(row >= 0, b"QQ", b"XX")
    want[~pool.v6] = w4

    def hook(t, no_summary):
        assert t["has_table"] == 1 and t["records"] == n + 1 and t["escapes"] == 0, t
        assert no_summary or (t["has_summary"] == 1 and t["shift"] == s and t["common"] == 0), t

    lookup_case(f"summary/{s}", geo, want, pool, hook)


def test_no_summary_when_most_blocks_are_uncommon_and_a_common_entry_that_is_not_record_0():
    rows = AC.geo_rows(["0.0.0.0/2", "64.0.0.0/2", "128.0.0.0/2", "192.0.0.0/2"])

    def none(t, no_summary):
        assert t["has_table"] == 1 and t["has_summary"] == 0 and t["shift"] == 0, t

    rows_case("no-summary", rows, pool_for([r[0] for r in rows], 14), none)
    rows = AC.geo_rows(["128.0.0.0/2", "0.0.0.0/1", "200.1.2.0/24"])

    def common(t, no_summary):
        assert no_summary or (t["has_summary"] == 1 and t["shift"] == 4 and t["common"] == 2), t  # record 2 = the second row

    rows_case("common!=0", rows, pool_for([r[0] for r in rows], 15), common)


def test_more_than_65536_records():
    n = 1 << 17
    geo = np.zeros(n, dtype=GEOIP_DTYPE)
    vals = (np.arange(n, dtype=np.uint32) << 8) + np.uint32(AC.BITS_BASE)
    geo["addr"][:, :4] = vals.astype(">u4").view(np.uint8).reshape(n, 4)
    geo["prefix_len"], geo["country"], geo["asn"] = 24, np.frombuffer(b"QQ", dtype=np.uint8), np.arange(n) + 7
    region = vals.astype(U)
    pool = Pool(np.concatenate([region, region + U(255), random4(12)]), [1, R.parse_v6("2001:db8::1")], 12)
    row = R.lpm4(pool.a4, (region, np.full(n, 24), np.arange(n)))
    row[R.geo_excluded4(pool.a4)] = -1
    want = np.zeros(pool.n, dtype=GEO_DTYPE)
    want["country"] = b"XX"
    w4 = np.zeros(len(row), dtype=GEO_DTYPE)
    w4["asn"], w4["country"] = np.where(row >= 0, row + 7, 0), np.where(row >= 0, b"QQ", b"XX")
    want[~pool.v6] = w4
    assert (want["asn"] > 65536 + 7).sum() > 10000

    def hook(t, no_summary):
        assert t["has_table"] == 1 and t["records"] == n + 1 and t["escapes"] == 0, t  # (a table entry IS the record id: no escape by id)

    lookup_case("records/2^17", geo, want, pool, hook)


def test_ipv6_every_length_and_empty_families():
    g6, _ = AC.v6_case()
    every = g6 + AC.chain6(AC.V6_DEEP, range(129))
    assert {R.parse_prefix(x)[2] for x in every} >= set(range(129))
    _, deep = R.parse_addr(AC.V6_DEEP)
    rng = np.random.default_rng(8)
    extra = [deep ^ (1 << k) for k in range(128)] + [int.from_bytes(rng.bytes(16), "big") for _ in range(4000)] + [1, 0, (1 << 128) - 1, R.parse_v6("ff02::1")]

    def no_table(t, no_summary):
        assert t["has_table"] == 0 and t["n_vals"] == 0 and t["has_summary"] == 0 and t["escapes"] == 0, t

    pool = pool_for(every, 8, n_random=20000, v6_extra=extra)
    want = rows_case("v6", AC.geo_rows(every), pool, no_table)
    assert (want["country"][~pool.v6] == b"XX").all()  # an IPv4 client against an IPv6-only table
    g4 = ["10.0.0.0/8", "10.1.2.0/25", "0.0.0.0/0"]
    pool = pool_for(every + g4, 10, n_random=20000, v6_extra=extra)
    want = rows_case("v4 only", AC.geo_rows(g4), pool, table(min_escapes=1, max_escapes=1))
    assert (want["country"][pool.v6] == b"XX").all() and pool.v6.sum() > 1000  # an IPv6 client against an IPv4-only table


def test_lockstep_walks_mix_families_depths_and_escapes():
    """One batch above 4 x 256 x the launch's block count: every lane of georec_kernel walks four live requests and its loop runs again
    with dead slots; asserted: lanes whose slots hold two IPv6 walks of different depths AND an IPv4 escape."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    T = 256 * GEOREC_BLOCKS_PER_CU * cus
    g4, _ = AC.escape_case()
    g6, _ = AC.v6_case()
    rows = AC.geo_rows(g4 + g6)
    deep24 = np.array(sorted({R.parse_prefix(x)[1] >> 8 for x in g4 if R.parse_prefix(x)[2] > 24}), dtype=U)
    inside = np.repeat(deep24 << U(8), 256) + np.tile(np.arange(256, dtype=U), len(deep24))
    _, deep = R.parse_addr(AC.V6_DEEP)
    rng = np.random.default_rng(16)
    a6 = AC.edges6(g6) + [deep ^ (1 << k) for k in range(128)] + [int.from_bytes(rng.bytes(16), "big") for _ in range(1000)]
    n_addr = GEOREC_U * T * 64 // 63 + 16384  # (the pool keeps 63 of 64: an eighth goes, an IPv6 address per eight IPv4 ones comes)
    a4 = np.concatenate([AC.edges4(g4), np.tile(inside, 200), random4(16, n_addr - n_addr // 8 - 200 * len(inside))])
    pool = Pool(a4, a6, 16)
    n = pool.n
    full = GEOREC_U * T
    assert full < n < 2 * full, (n, cus)
    geo = R.Geo(rows)
    r = pool.geo_rows(geo)
    plen = np.array([R.parse_prefix(x)[2] for x, _, _ in rows] + [0])[r]
    escaped = np.zeros(n, dtype=bool)
    escaped[~pool.v6] = np.isin(pool.a4 >> U(8), deep24)
    slot_v6 = pool.v6[:full].reshape(GEOREC_U, T)
    slot_depth = np.where(slot_v6, (plen[:full].reshape(GEOREC_U, T) + 7) // 8, 0)
    slot_esc = escaped[:full].reshape(GEOREC_U, T)
    two_depths = np.zeros(T, dtype=bool)
    for u in range(GEOREC_U):
        for v in range(u + 1, GEOREC_U):
            two_depths |= (slot_depth[u] > 2) & (slot_depth[v] > 2) & (slot_depth[u] != slot_depth[v])
    mixed = int((slot_esc.any(axis=0) & two_depths).sum())
    mixed_family = int((slot_v6.any(axis=0) & ~slot_v6.all(axis=0)).sum())
    assert mixed >= 100 and mixed_family >= T // 4, (mixed, mixed_family)
    want = record_table(rows)[r + 1]
    lookup_case("lockstep", geoip_entries(rows), want, pool, table(min_escapes=len(deep24)))


# ---------------------------------------------------------------------------------------------------------
# 2. - 4. the entry points
# ---------------------------------------------------------------------------------------------------------
CASE_ROWS = [("8.8.8.0/24", 15169, "US"), ("1.0.0.0/8", 13335, "AU"), ("5.5.0.0/16", 64512, "KP"), ("2001:db8::/32", 64512, "FR"), ("1.2.3.0/25", 7, "DE"), ("3.0.0.0/8", 9, "x1"),
             ("3.3.0.0/16", 11, "GB"), ("127.0.0.0/8", 3, "US"), ("::/0", 2, "NL"), ("2.0.0.0/7", 64500, "FR")]
CASE_LISTS = {"bad": (_abi.LIST_IP, ["10.0.0.0/8", "2001:db8::/32", "1.2.3.4"])}
CASE_RULES = [("ip", 'lists["bad"].contains(client.ip)', [B]), ("ua", 'http_request.user_agent.contains("sqlmap")', [B]),
              ("adm", 'http_request.path.starts_with("/a") && client.country != "FR"', [CAP, B]), ("asn", "client.asn == 64500", [B]),
              ("res", "http_request.url.length() - http_request.path.length() > 2 && client.remote_port % 2 == 1", [CAP])]


def case_requests(n, with_geo, seed=5):
    rng = random.Random(seed)
    reqs = H.fuzz_requests(rng, n, with_geo)
    ips = ["8.8.8.8", "1.2.3.4", "1.2.3.200", "5.5.1.1", "10.1.2.3", "2001:db8::7", "2001:db9::1", "127.0.0.1", "224.0.0.1", "3.1.1.1", "3.3.3.3", "::1", "ff02::1", "2.2.2.2", "200.1.1.1"]
    for i, r in enumerate(reqs):
        if i % 2:
            r.ip = ips[(i // 2) % len(ips)]
    return reqs


def test_entry_points_agree_with_the_lookup_and_their_plain_counterparts():
    import torch

    geo = geoip_entries(CASE_ROWS)
    eng = RuleEngine(CASE_RULES, CASE_LISTS, geo, flags=GEO)
    reqs = case_requests(3000, False)
    batch = RequestBatch.from_requests(reqs)
    want = eng.lookup_geoip(batch.ip, batch.ip_is_v6)
    assert len(np.unique(want)) >= 8
    oracle = pyoracle.Oracle(CASE_RULES, CASE_LISTS, geo)
    for j in range(0, batch.n, 7):
        assert (int(want["asn"][j]), bytes(want["country"][j])) == oracle.geoip_lookup(batch.ip[j].tobytes(), bool(batch.ip_is_v6[j]))
    plain, plain_counts = eng.evaluate_batch(batch, with_counts=True)
    H.assert_verdicts_equal(plain, oracle.evaluate(batch), batch, "plain")
    assert len(set(plain["rule_idx"].tolist())) >= 5  # gates, rules and allow: every kind of verdict gets its record
    # evaluate_batch
    got, counts, g = eng.evaluate_batch(batch, with_counts=True, with_geo=True)
    assert (got == plain).all() and (counts == plain_counts).all()
    assert_same("evaluate_batch", g, want)
    got, g = eng.evaluate_batch(batch, with_geo=True)
    assert (got == plain).all() and same(g, want).all()
    # a batch too large for the packed block: the column-by-column path
    big = batch.tile(12)
    bp, bc = eng.evaluate_batch(big, with_counts=True)
    got, counts, g = eng.evaluate_batch(big, with_counts=True, with_geo=True)
    assert (got == bp).all() and (counts == bc).all()
    assert_same("evaluate_batch (large)", g, np.tile(want, 12))
    # evaluate_records
    buf, off = batch.to_records()
    rp, rc = eng.evaluate_records(buf, off, with_counts=True)
    got, counts, g = eng.evaluate_records(buf, off, with_counts=True, with_geo=True)
    assert (rp == plain).all() and (got == plain).all() and (counts == rc).all() and (rc == plain_counts).all()
    assert_same("evaluate_records", g, want)
    # evaluate
    for j in range(0, 200):
        v, (asn, cc) = eng.evaluate(reqs[j], with_geo=True)
        v0 = eng.evaluate(reqs[j])
        assert v == v0 and int(v.decision) == int(plain["action"][j]), j
        assert (asn, cc.encode()) == (int(want["asn"][j]), bytes(want["country"][j])), j
    # evaluate_device
    db = DeviceBatch(batch)
    out0 = eng.evaluate_device(db)
    c0 = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    eng.evaluate_device(db, counts=c0)
    dgeo = torch.zeros((batch.n, 2), dtype=torch.int32, device="cuda:0")
    c1 = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    out1 = eng.evaluate_device(db, counts=c1, geo=dgeo)
    eng.device_status()
    assert torch.equal(out0, out1) and torch.equal(c0, c1) and c0.cpu().tolist() == plain_counts.tolist()
    assert (out1.cpu().numpy().view(plain.dtype).reshape(-1) == plain).all()
    assert_same("evaluate_device", dgeo.cpu().numpy().view(GEO_DTYPE).reshape(-1), want)
    # a DEVICE batch through pwaf_evaluate_batch_geo, and a device-resident pwaf_geoip_lookup on a stream
    from pingoo_amd.engine import lib
    import ctypes as C

    st = db.as_struct(eng.header_names)
    dv = torch.zeros((batch.n, 2), dtype=torch.int32, device="cuda:0")
    dgeo.zero_()
    assert lib().pwaf_evaluate_batch_geo(eng._h, C.byref(st), dv.data_ptr(), None, dgeo.data_ptr()) == 0
    assert torch.equal(dv, out0)
    assert_same("evaluate_batch_geo (device)", dgeo.cpu().numpy().view(GEO_DTYPE).reshape(-1), want)
    dgeo.zero_()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    assert lib().pwaf_geoip_lookup(eng._h, db.ip.data_ptr(), db.ip_is_v6.data_ptr(), batch.n, _abi.MEM_DEVICE, dgeo.data_ptr(), C.c_void_p(stream.cuda_stream)) == 0
    stream.synchronize()
    assert_same("pwaf_geoip_lookup (device)", dgeo.cpu().numpy().view(GEO_DTYPE).reshape(-1), want)
    # the async queue
    for geo_queue in (True, False):
        q = AsyncBatcher(eng, max_batch=256, max_delay_us=200, max_in_flight=4096, geo=geo_queue)
        done = {}
        m = 1500
        for j in range(m):
            while not q.submit(reqs[j], j):
                for c in (q.poll(512, with_geo=True) if geo_queue else q.poll(512)):
                    done[c[0]] = c
        q.flush()
        t0 = time.time()
        while len(done) < m and time.time() - t0 < 60:
            for c in (q.poll(512, with_geo=True) if geo_queue and len(done) % 2 == 0 else q.poll(512)):
                done[c[0]] = c
        assert len(done) == m
        n_geo = 0
        for j, c in done.items():
            assert c[2] == 0 and int(c[1].decision) == int(plain["action"][j]), j
            if len(c) == 4:
                n_geo += 1
                assert (c[3][0], c[3][1].encode()) == (int(want["asn"][j]), bytes(want["country"][j])), j
        if geo_queue:
            assert n_geo > 100  # (the plain poll of a geo queue hands out completions and drops the records)
        else:
            assert n_geo == 0
            with pytest.raises(UnsupportedExpression, match="pwaf_async_create_geo"):
                q.poll(16, with_geo=True)
            assert q.stats()[2] == 0
        q.close()
    eng.close()


def test_rules_see_the_returned_record():
    """country == ".." and asn == N rules: for every request, the rule the engine and the oracle report is the first one its RETURNED record
    satisfies"""
    geo_rows = AC.geo_rows(AC.lengths_geo_prefixes()) + [("2001:db8::/32", 900, "FR"), ("::/0", 901, "NL"), ("2001:db8:7::/48", 902, "x1")]
    ccs = []
    for _, _, c in geo_rows:
        if valid_country(c) and c not in ccs:
            ccs.append(c)
    rules = [(f"c{c}", f'client.country == "{c}"', [B]) for c in ccs[0::2]] + [(f"a{a}", f"client.asn == {a}", [CAP]) for _, a, c in geo_rows if valid_country(c)] + \
            [("xx", 'client.country == "XX"', [B])]
    geo = geoip_entries(geo_rows)
    eng = RuleEngine(rules, None, geo, flags=GEO)
    pool = pool_for([r[0] for r in geo_rows], 31, n_random=30000)
    batch = make_batch(pool.ip, pool.v6, np.full(pool.n, 40000, dtype=np.uint16))
    got, g = eng.evaluate_batch(batch, with_geo=True)
    assert_same("lookup", g, eng.lookup_geoip(pool.ip, pool.v6))
    sample = np.sort(np.random.default_rng(3).choice(pool.n, 20000, replace=False))
    want = pyoracle.Oracle(rules, None, geo).evaluate(batch.take(sample), threads=8)
    assert (want["rule_idx"] == got["rule_idx"][sample]).all() and (want["action"] == got["action"][sample]).all()
    first_cc = {c: k for k, c in enumerate(ccs[0::2])}
    n_cc = len(first_cc)
    first_asn = {}
    for k, (_, a, c) in enumerate(r for r in geo_rows if valid_country(r[2])):
        first_asn.setdefault(a, n_cc + k)
    expect = np.array([first_cc.get(c.decode(), first_asn.get(int(a), len(rules) - 1 if c == b"XX" else -1)) for a, c in zip(g["asn"], g["country"])], dtype=np.int64)
    assert (expect >= 0).all()
    assert (got["rule_idx"].astype(np.int64) == expect).all()
    assert len(set(expect.tolist())) >= 30
    eng.close()


def test_caller_columns_and_has_geoip_records_are_echoed():
    geo = geoip_entries(CASE_ROWS)
    eng = RuleEngine(CASE_RULES, CASE_LISTS, geo, flags=GEO)
    reqs = case_requests(2000, True, seed=9)
    batch = RequestBatch.from_requests(reqs)
    assert batch.asn is not None
    want = np.zeros(batch.n, dtype=GEO_DTYPE)
    want["asn"], want["country"] = batch.asn, batch.country.view("S2")
    plain = eng.evaluate_batch(batch)
    H.assert_verdicts_equal(plain, pyoracle.Oracle(CASE_RULES, CASE_LISTS, geo).evaluate(batch), batch, "columns")
    got, g = eng.evaluate_batch(batch, with_geo=True)
    assert (got == plain).all()
    assert_same("columns", g, want)
    assert not same(g, eng.lookup_geoip(batch.ip, batch.ip_is_v6)).all()  # (the table says otherwise: it was not consulted)
    buf, off = batch.to_records()
    got, g = eng.evaluate_records(buf, off, with_geo=True)
    assert (got == plain).all()
    assert_same("has_geoip records", g, want)
    v, (asn, cc) = eng.evaluate(reqs[3], with_geo=True)
    assert (asn, cc) == (reqs[3].asn, reqs[3].country)
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# 5. defaults
# ---------------------------------------------------------------------------------------------------------
def test_defaults():
    pool = pool_for(["10.0.0.0/8", "2001:db8::/32"], 41, n_random=5000, v6_extra=[1, R.parse_v6("ff02::1"), R.parse_v6("2001:db8::1")])
    batch = make_batch(pool.ip, pool.v6, np.full(pool.n, 1, dtype=np.uint16))
    # an engine without a table
    eng = RuleEngine(ANY_RULE, None, None, flags=GEO)
    t = eng.geo_answer_tables()
    assert t["has_table"] == 0 and t["records"] == 1 and t["escapes"] == 0
    for g in (eng.lookup_geoip(pool.ip, pool.v6), eng.evaluate_batch(batch, with_geo=True)[1], eng.evaluate_records(*batch.to_records(), with_geo=True)[1]):
        assert (g["asn"] == 0).all() and (g["country"] == b"XX").all() and (g["reserved"] == 0).all() and len(g) == pool.n
    assert eng.evaluate(Request(host="h", url="/", path="/", method="GET", user_agent="Mozilla/5.0", ip="9.9.9.9", remote_port=1), with_geo=True)[1] == (0, "XX")
    assert len(eng.lookup_geoip(np.zeros((0, 16), dtype=np.uint8), np.zeros(0, dtype=np.uint8))) == 0
    eng.close()
    # loopback and multicast below 0.0.0.0/0 and ::/0; every other address reads the covering record
    eng = RuleEngine(ANY_RULE, None, geoip_entries([("0.0.0.0/0", 5, "AA"), ("::/0", 6, "BB"), ("127.0.0.0/8", 7, "CC"), ("224.0.0.0/4", 8, "DD"), ("::1/128", 9, "EE"), ("ff00::/8", 10, "FF")]), flags=GEO)
    g = eng.lookup_geoip(pool.ip, pool.v6)
    ex = np.zeros(pool.n, dtype=bool)
    ex[~pool.v6] = R.geo_excluded4(pool.a4)
    ex[pool.v6] = R.geo_excluded6(pool.hi, pool.lo)
    assert ex.sum() >= 5 and (g["country"][ex] == b"XX").all() and (g["asn"][ex] == 0).all()
    assert (g["country"][~ex & ~pool.v6] == b"AA").all() and (g["country"][~ex & pool.v6] == b"BB").all()
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# 6. the flag and NULL
# ---------------------------------------------------------------------------------------------------------
def test_without_the_flag_every_entry_point_is_unsupported_and_the_launch_list_is_unchanged():
    import ctypes as C

    import torch

    from pingoo_amd.engine import lib

    geo = geoip_entries(CASE_ROWS)
    reqs = case_requests(1000, False)
    batch = RequestBatch.from_requests(reqs)
    off_eng = RuleEngine(CASE_RULES, CASE_LISTS, geo)
    on_eng = RuleEngine(CASE_RULES, CASE_LISTS, geo, flags=GEO)
    for call in (lambda: off_eng.lookup_geoip(batch.ip, batch.ip_is_v6), lambda: off_eng.evaluate_batch(batch, with_geo=True), lambda: off_eng.evaluate_records(*batch.to_records(), with_geo=True),
                 lambda: off_eng.evaluate(reqs[0], with_geo=True), lambda: AsyncBatcher(off_eng, geo=True), lambda: off_eng.geo_answer_tables(),
                 lambda: off_eng.evaluate_device(DeviceBatch(batch), geo=torch.zeros((batch.n, 2), dtype=torch.int32, device="cuda:0"))):
        with pytest.raises(UnsupportedExpression, match="PWAF_OPT_GEO_ANSWERS") as ei:
            call()
        assert ei.value.code == _abi.E_UNSUPPORTED
    # (also with geo == NULL)
    st = batch.as_struct(off_eng.header_names)
    out = np.zeros(batch.n, dtype=np.dtype([("a", "u1", (4,)), ("r", "<u4")]))
    assert lib().pwaf_evaluate_batch_geo(off_eng._h, C.byref(st), out.ctypes.data, None, None) == _abi.E_UNSUPPORTED

    def names(eng, **kw):
        eng.set_profiling(1)
        eng.evaluate_batch(batch, **kw)
        t = [k[0] for k in eng.kernel_times()]
        eng.set_profiling(0)
        return t

    # the parent commit's launch list for this rule set: no kernel of this change in it; the flag alone, and the flag with geo == NULL,
    # launch exactly the same
    base = names(off_eng)
    assert "ipres" in base and "attr" in base and "verdict" in base and "georec" not in base
    assert names(on_eng) == base
    assert lib().pwaf_evaluate_batch_geo(on_eng._h, C.byref(st), out.ctypes.data, None, None) == 0
    on_eng.set_profiling(1)
    assert lib().pwaf_evaluate_batch_geo(on_eng._h, C.byref(st), out.ctypes.data, None, None) == 0
    assert [k[0] for k in on_eng.kernel_times()] == base
    on_eng.set_profiling(0)
    with_geo = names(on_eng, with_geo=True)
    assert with_geo.count("georec") == 1 and [k for k in with_geo if k != "georec"] == base
    assert with_geo.index("georec") == with_geo.index("ipres") + 1
    on_eng.set_profiling(1)
    on_eng.lookup_geoip(batch.ip, batch.ip_is_v6)  # (a HOST lookup is not a profiled launch; a DEVICE one is)
    d_ip, d_v6 = torch.from_numpy(batch.ip).cuda(), torch.from_numpy(batch.ip_is_v6).cuda()
    d_out = torch.zeros((batch.n, 2), dtype=torch.int32, device="cuda:0")
    assert lib().pwaf_geoip_lookup(on_eng._h, d_ip.data_ptr(), d_v6.data_ptr(), batch.n, _abi.MEM_DEVICE, d_out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert [k[0] for k in on_eng.kernel_times()] == ["georec"]
    on_eng.set_profiling(0)
    assert (off_eng.evaluate_batch(batch) == on_eng.evaluate_batch(batch)).all()
    off_eng.close()
    on_eng.close()


# ---------------------------------------------------------------------------------------------------------
# 7. verdicts do not depend on the flag
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_fuzz_verdicts_do_not_depend_on_the_flag(seed):
    rng = random.Random(23000 + seed)
    wide = seed % 2 == 1
    lists = H.fuzz_lists(rng, wide)
    geo = H.fuzz_geoip(rng, wide) if rng.random() < 0.8 else None
    with_geo = rng.random() < 0.3
    rules = [(f"r{k}", H.rexpr(rng, lists) if rng.random() < 0.95 else None, H.fuzz_actions(rng)) for k in range(rng.randint(1, 14))]
    flags = rng.choice([0, 0, _abi.OPT_NO_UA_GATE, _abi.OPT_NO_CAPTCHA_BYPASS]) | _abi.OPT_LENIENT
    batch = RequestBatch.from_requests(H.fuzz_requests(rng, rng.choice([1, 63, 64, 65, 200, 777]), with_geo, wide, H.address_edges(lists, geo) if wide else ()))
    off_eng = RuleEngine(rules, lists, geo, flags=flags)
    on_eng = RuleEngine(rules, lists, geo, flags=flags | GEO)
    v0, c0 = off_eng.evaluate_batch(batch, with_counts=True)
    v1, c1 = on_eng.evaluate_batch(batch, with_counts=True)
    v2, c2, g = on_eng.evaluate_batch(batch, with_counts=True, with_geo=True)
    assert (v0 == v1).all() and (v0 == v2).all() and (c0 == c1).all() and (c0 == c2).all()
    # and the record is the oracle's (or the caller's)
    if with_geo:
        assert (g["asn"] == batch.asn).all() and (g["country"].view("<u2") == batch.country).all()
    else:
        oracle = pyoracle.Oracle([("r", None, [B])], None, geo)
        for j in range(batch.n):
            assert (int(g["asn"][j]), bytes(g["country"][j])) == oracle.geoip_lookup(batch.ip[j].tobytes(), bool(batch.ip_is_v6[j])), j
    off_eng.close()
    on_eng.close()
