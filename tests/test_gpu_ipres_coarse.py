"""ipres_kernel<.., COARSE> on the device: the coarse bitmap staged in LDS in front of the summary (csrc/dirtable.h). One-answer rule
sets as in tests/test_gpu_addresses.py — a verdict reads out an (address, list) bit or a GeoIP record's country — compared with the
brute-force reference (tests/lpm_reference.py) on every request. Table shapes: tests/coarse_cases.py (shared with the CPU suite).

A batch is laid out by waves (a wave of the kernel holds 64 consecutive requests while the batch fits one sweep of the grid):
requests 0..63 are IPv4 addresses in CLEAR coarse blocks (no lane goes on to a global load), 64..127 IPv4 addresses in SET blocks,
128..255 alternate IPv4 (clear and set in turn) and IPv6, then both ends of the first and last /24 of the blocks the CPU suite names
(block 0, the last block, a set block between clear neighbours, 127/8 and multicast inside clear and set blocks), then prefix edges and
random addresses. Every address appears with every port, i.e. reads out every answer; the batch sizes are prefixes of that order."""
import numpy as np
import pytest

import address_cases as AC
import coarse_cases as CC
import lpm_reference as R
from pingoo_amd import RequestBatch, _abi, geoip_entries
from pingoo_amd.batch import GEOIP_DTYPE
from pingoo_amd.engine import RuleEngine
from test_gpu_addresses import PORT0, const_col, make_batch, verdicts

pytestmark = pytest.mark.gpu
B = _abi.RULE_ACTION_BLOCK
U = np.uint64
SIZES = [1, 63, 64, 257, 4096 + 37]
V6_GEO, V6_LIST = "2001:db8::/32", "2001:db8:1::/48"


class Case:
    """rules, lists, geo, the addresses in wave order and the rule every (address, port) request must report"""

    def __init__(self, geo, lists, rules, n_ports, clear24, set24, edges24, prefixes4, a6, expect, seed):
        rng = np.random.default_rng(seed)
        pick = lambda xs, n: (np.array([xs[i % len(xs)] for i in range(n)], dtype=U) << U(8)) | rng.integers(0, 256, n, dtype=U)
        clear, sset = pick(clear24, 128), pick(set24, 128)
        a6 = list(a6)
        seq = [(False, int(x)) for x in clear[:64]] + [(False, int(x)) for x in sset[:64]]
        for i in range(64):
            seq += [(False, int((clear if i % 2 else sset)[64 + i])), (True, a6[i % len(a6)])]
        for x in edges24:
            seq += [(False, x << 8), (False, (x << 8) | 255)]
        seq += [(False, int(x)) for x in AC.edges4(prefixes4)[:600]] + [(True, v) for v in a6] + [(False, int(x)) for x in rng.integers(0, 1 << 32, 1000, dtype=U)]
        self.v6 = np.array([s[0] for s in seq], dtype=bool)
        m = len(seq)
        self.ip = np.zeros((m, 16), dtype=np.uint8)
        for i, (six, v) in enumerate(seq):
            self.ip[i, :16 if six else 4] = np.frombuffer(v.to_bytes(16 if six else 4, "big"), dtype=np.uint8)
        a4 = np.array([v for six, v in seq if not six], dtype=U)
        hi, lo = R.v6_arrays([v for six, v in seq if six])
        # request j: address j mod m with port PORT0 + ((j + j // m) mod n_ports): every address meets every port
        j = np.arange(m * n_ports)
        self.addr, self.which = j % m, (j + j // m) % n_ports
        self.rule = expect(self.v6, a4, hi, lo, self.addr, self.which)
        self.geo, self.lists, self.rules = geo, lists, rules
        self.n = len(j)
        assert not self.v6[:128].any() and self.v6[128:256].sum() == 64
        self.first_v4 = a4[:128]

    def batch(self, n=None):
        n = self.n if n is None else n
        return make_batch(self.ip[self.addr[:n]], self.v6[self.addr[:n]], (PORT0 + self.which[:n]).astype(np.uint16))


def ranges_set(prefixes4, x24s, shift):
    """is the block of 2^shift /24s around each x24 touched by a prefix (first /24, last /24)?"""
    out = []
    for x in x24s:
        lo, hi = CC.block_ends(x, shift)
        out.append(any(not (p_hi < lo or p_lo > hi) for p_lo, p_hi in prefixes4))
    return out


def span24(text):
    _, v, ln = R.parse_prefix(text)
    return v >> 8, (v | ((1 << (32 - ln)) - 1)) >> 8


def sparse_case():
    g4, lists4 = CC.sparse_geo_prefixes(), CC.sparse_lists()
    rows = AC.geo_rows(g4 + [V6_GEO])
    lists = dict(lists4)
    lists["l"] = lists["l"] + [V6_LIST]
    names = list(lists)
    L = len(names)
    cc = [c for _, _, c in rows]
    rules = [(f"l{k}", f'lists["{nm}"].contains(client.ip) && client.remote_port == {PORT0 + k}', [B]) for k, nm in enumerate(names)]
    rules += [(c, f'client.country == "{c}" && client.remote_port == {PORT0 + L}', [B]) for c in cc]
    geo, lref = R.Geo(rows), R.Lists(lists)

    def expect(v6, a4, hi, lo, addr, which):
        row = np.full(len(v6), -1, dtype=np.int64)
        row[~v6], row[v6] = geo.lookup4(a4), geo.lookup6(hi, lo)
        member = np.zeros((len(v6), L), dtype=bool)
        for k, nm in enumerate(names):
            member[~v6, k], member[v6, k] = lref.member4(nm, a4), lref.member6(nm, hi, lo)
        return np.where(which < L, np.where(member[addr, np.minimum(which, L - 1)], which, -1), np.where(row[addr] >= 0, L + row[addr], -1))

    every4 = g4 + [x for items in lists4.values() for x in items]
    spans = [span24(x) for x in every4]
    clear24 = [CC.CLEAR_24, CC.CLEAR_24 + 63, CC.LOOPBACK_CLEAR_24, CC.MULTICAST_CLEAR_24, CC.ISOLATED_24 - 1, CC.ISOLATED_24 + 64, CC.X(200, 7, 9), CC.X(1, 2, 3)]
    set24 = [CC.SET_24, CC.SET_24 + 31, CC.LOOPBACK_SET_24, CC.MULTICAST_SET_24, CC.ISOLATED_24, CC.ISOLATED_24 + 31, CC.X(70, 3, 8), CC.X(90, 0, 16), CC.X(80, 0, 3), 0, (1 << 24) - 1]
    for shift in (5, 6):
        assert not any(ranges_set(spans, clear24, shift)) and all(ranges_set(spans, set24, shift))
    _, deep = R.parse_addr("2001:db8:1:2::7")
    a6 = [deep, deep ^ (1 << 90), R.parse_v6("2001:db8::1"), R.parse_v6("2001:db9::1"), 1, R.parse_v6("ff02::1"), R.parse_v6("2001:db8:1::"), R.parse_v6("2001:db8:2::5")]
    case = Case(geoip_entries(rows), {k: (_abi.LIST_IP, v) for k, v in lists.items()}, rules, L + 1, clear24, set24, sorted(set(CC.edge_24s(5) + CC.edge_24s(6))), every4, a6, expect, 31)
    case.spans = spans
    assert (case.rule[:64] == -1).all() and (case.rule >= 0).sum() > 200 and len(set(case.rule.tolist())) >= 12
    return case


@pytest.fixture(scope="module")
def sparse():
    return sparse_case()


@pytest.fixture(scope="module")
def sparse_engines(sparse):
    engs = {flags: RuleEngine(sparse.rules, sparse.lists, sparse.geo, flags=flags) for flags in (0, _abi.OPT_NO_DIR_SUMMARY)}
    yield engs
    for e in engs.values():
        e.close()


def check_sizes(eng, case, label):
    act, idx = verdicts(case.rule)
    assert case.n >= SIZES[-1], case.n
    for n in SIZES + [case.n]:
        got, counts = eng.evaluate_batch(case.batch(n), with_counts=True)
        bad = np.nonzero((got["action"] != act[:n]) | (got["rule_idx"] != idx[:n]))[0]
        assert len(bad) == 0, (f"{label}, batch of {n}: {len(bad)} verdicts differ from the reference; first at {bad[0]}: address "
                               f"{R.fmt_addr(bool(case.v6[case.addr[bad[0]]]), int.from_bytes(case.ip[case.addr[bad[0]]].tobytes()[:16 if case.v6[case.addr[bad[0]]] else 4], 'big'))} port {case.which[bad[0]]}"
                               f" got ({got['action'][bad[0]]}, {got['rule_idx'][bad[0]]}) want ({act[bad[0]]}, {idx[bad[0]]})")
        assert counts.tolist() == np.bincount(act[:n], minlength=4).tolist()


def test_default_engine_has_the_level_and_answers_like_the_reference(sparse, sparse_engines):
    eng = sparse_engines[0]
    t, c = eng.address_tables(), eng.coarse_tables()
    print("tables", t, "coarse", c)
    assert t["has_summary"] == 1 and t["common"] == 0 and t["packed"] == 1 and t["escapes"] >= 1, t
    assert c["present"] == 1 and c["shift"] in (5, 6) and c["bytes"] == (1 << 21) >> c["shift"] and c["threads"] * c["wg_per_cu"] <= 2048, c
    # blocks set = blocks a prefix touches (every record has a rule of its own, so no prefix's entry is the common one)
    n_blk = 1 << (24 - c["shift"])
    touched = np.zeros(n_blk, dtype=bool)
    for lo, hi in sparse.spans:
        touched[lo >> c["shift"]:(hi >> c["shift"]) + 1] = True
    assert c["blocks_set"] == int(touched.sum()) and 0 < c["blocks_set"] * 2 <= n_blk, (c, int(touched.sum()))
    assert c["summary_blocks_set"] > c["blocks_set"] and c["rec_present"] == 0
    # the first wave's blocks are clear, the second wave's set, in the engine's own granularity
    first = (sparse.first_v4 >> U(8 + c["shift"])).astype(np.int64)
    assert not touched[first[:64]].any() and touched[first[64:]].all()
    check_sizes(eng, sparse, "default")


def test_no_summary_engine_has_no_level_and_answers_the_same(sparse, sparse_engines):
    eng = sparse_engines[_abi.OPT_NO_DIR_SUMMARY]
    t, c = eng.address_tables(), eng.coarse_tables()
    assert t["has_summary"] == 0 and c["present"] == 0 and c["bytes"] == 0 and c["blocks_set"] == 0 and c["threads"] == 256, (t, c)
    check_sizes(eng, sparse, "no summary")


def test_level_switched_off_when_most_coarse_blocks_are_set():
    """three quarters of the /19s hold a /24 with a record (coarse_cases.dense_geo_prefixes): a summary, no coarse level"""
    p = CC.dense_geo_prefixes()
    n = len(p)
    vals = np.array([R.parse_prefix(x)[1] for x in p], dtype=U)
    geo = np.zeros(n, dtype=GEOIP_DTYPE)
    geo["addr"][:, :4] = vals.astype(">u4").view(np.uint8).reshape(n, 4)
    geo["prefix_len"], geo["country"], geo["asn"] = 24, np.frombuffer(b"QQ", dtype=np.uint8), 7

    def expect(v6, a4, hi, lo, addr, which):
        row = np.full(len(v6), -1, dtype=np.int64)
        r4 = R.lpm4(a4, (vals, np.full(n, 24), np.arange(n)))
        r4[R.geo_excluded4(a4)] = -1
        row[~v6] = r4
        return np.where(row[addr] >= 0, 0, -1)

    set24 = [int(v) >> 8 for v in vals[~R.geo_excluded4(vals)][:: n // 40]]
    clear24 = [x + 1 for x in set24]  # (the /24 behind a record's: same block, no record)
    case = Case(geo, None, [("q", 'client.country == "QQ"', [B])], 1, clear24, set24, CC.edge_24s(5), p[:50], [1, R.parse_v6("2001:db8::1")], expect, 32)
    case.addr, case.which, case.rule = np.tile(case.addr, 4), np.tile(case.which, 4), np.tile(case.rule, 4)  # (one port: repeat the addresses up to the largest size)
    case.n = len(case.addr)
    assert case.n >= SIZES[-1] and (case.rule[64:128] == 0).all()
    eng = RuleEngine(case.rules, None, geo)
    t, c = eng.address_tables(), eng.coarse_tables()
    assert t["has_summary"] == 1 and t["shift"] == 2 and c["present"] == 0 and c["shift"] == 0 and c["threads"] == 256, (t, c)
    assert c["summary_blocks_set"] == n
    check_sizes(eng, case, "dense")
    eng.close()


def test_unpacked_results_behind_the_level():
    """17 bit-lists: 2^17 membership sets, so ipres_kernel<false, COARSE> and two result words per request (tests/test_gpu_addresses.py)"""
    nb = 17
    lists = AC.bit_lists(nb)
    names = list(lists)
    rules = [(f"l{k}", f'lists["{nm}"].contains(client.ip) && client.remote_port == {PORT0 + k}', [B]) for k, nm in enumerate(names)]
    lref = R.Lists(lists)
    base24 = AC.BITS_BASE >> 8
    ports = [0, 1, 8, 16]  # the lists a request asks about

    def expect(v6, a4, hi, lo, addr, which):
        member = np.zeros((len(v6), len(ports)), dtype=bool)
        for i, k in enumerate(ports):
            member[~v6, i] = lref.member4(names[k], a4)
        return np.where(member[addr, which], np.array(ports)[which], -1)

    set24 = [base24 + i for i in (1, 2, 255, 256, 65535, 65536, 99999, (1 << nb) - 1)]
    clear24 = [base24 - 1, base24 - 64, base24 + (1 << nb), base24 + (1 << nb) + 63, CC.X(1, 2, 3), CC.X(200, 0, 0), 0, (1 << 24) - 1]
    edges = [x for b in (base24, base24 + (1 << nb) - 1, base24 - 1, base24 + (1 << nb), 0, (1 << 24) - 1) for x in CC.block_ends(b, 5) + CC.block_ends(b, 6)]
    case = Case(None, {k: (_abi.LIST_IP, v) for k, v in lists.items()}, rules, len(ports), clear24, set24, sorted(set(edges)), ["64.0.0.0/%d" % (24 - nb)], [1, R.parse_v6("2001:db8::1")], expect, 33)
    case.which = np.array(ports)[case.which]  # (ports are PORT0 + the list's index)
    assert (case.rule[:64] == -1).all() and (case.rule >= 0).sum() > 200
    eng = RuleEngine(case.rules, case.lists, None)
    t, c = eng.address_tables(), eng.coarse_tables()
    assert t["packed"] == 0 and t["sets"] == 1 << nb and t["has_summary"] == 1, t
    assert c["present"] == 1 and c["blocks_set"] == (1 << nb) >> c["shift"], c
    check_sizes(eng, case, "unpacked")
    eng.close()


def test_more_than_one_sweep_of_the_grid_default_against_no_summary(sparse, sparse_engines):
    """n = the grid's capacity (workgroups x threads x 4 requests per lane) + 1000, so the kernel's loop runs again with dead lanes and
    dead slots and reads the staged bitmap a second time; empty string fields (but for a one-byte User-Agent: an empty one is blocked by
    the User-Agent gate before any rule, PWAF_RULE_UA_GATE, and no verdict would depend on its address); the two engines' verdicts, device
    against device."""
    import torch

    c = sparse_engines[0].coarse_tables()
    assert c["present"] == 1
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = c["wg_per_cu"] * cus * c["threads"] * 4 + 1000
    rng = np.random.default_rng(34)
    m = len(sparse.ip)
    pick = rng.integers(0, m, n)
    pick[: 4 * m] = np.tile(np.arange(m), 4)
    pick[-m:] = np.arange(m)  # (the second sweep sees the named addresses too)
    which = rng.integers(0, int(sparse.which.max()) + 1, n)
    cols = [const_col(b"", n)] * 4 + [const_col(b"M", n)]
    batch = RequestBatch([x[0] for x in cols], [x[1] for x in cols], sparse.ip[pick], sparse.v6[pick].astype(np.uint8), (PORT0 + which).astype(np.uint16), np.zeros(n, dtype=np.uint8))
    got = [sparse_engines[f].evaluate_batch(batch, with_counts=True) for f in (0, _abi.OPT_NO_DIR_SUMMARY)]
    assert (got[0][0]["action"] == got[1][0]["action"]).all() and (got[0][0]["rule_idx"] == got[1][0]["rule_idx"]).all()
    assert got[0][1].tolist() == got[1][1].tolist() and got[0][1][_abi.ACTION_BLOCK] > 1000
    # and the named addresses of the tail against the reference (their ports are random: recompute the expectation from the case's table)
    want = {(int(a), int(w)): int(r) for a, w, r in zip(sparse.addr, sparse.which, sparse.rule)}
    tail = np.arange(n - m, n)
    exp = np.array([want[(int(pick[j]), int(which[j]))] for j in tail])
    act, idx = verdicts(exp)
    assert (got[0][0]["action"][tail] == act).all() and (got[0][0]["rule_idx"][tail] == idx).all()
