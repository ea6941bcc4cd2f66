"""attr_kernel's group loop: the tables it keeps in LDS (the (source word, bit) -> column table, the comparison atoms and short
literals beyond the 64 held in registers) and the rotation of its input prefetch, read through rule sets of ONE predicate per rule —
ip lists, countries, port sets, asn sets, asn comparisons, port comparisons, method literals — so that the expected verdict of a
request is the first rule its attributes satisfy, computed here with numpy.

Every rule set puts atoms on bit 0, bit 31 and the last used bit of every source word it has. The four engines are the two SMALL
settings of the kernel (more than 128 ip lists and more than 64 countries force the wide instantiation) times the two sources of
asn / country (the engine's GeoIP table, or columns of the batch). The wide sets also carry more comparison atoms and short literals
than the kernel stages (256 / 128), the small ones more than its registers hold (64) but fewer than that.

The batch is laid out by 64-request groups: a group is mixed, empty (no source word has a bit), carries ONE kind of predicate (one
present source word class) or has every request satisfy every kind (all words present) — a transpose that returns early must not
disturb the words after it. The large batch gives every wave of the launch at least three groups; its slices give the sizes around
one group."""
import numpy as np
import pytest

from pingoo_amd import RequestBatch, _abi, geoip_entries
from pingoo_amd.engine import RuleEngine

pytestmark = pytest.mark.gpu
B = _abi.RULE_ACTION_BLOCK
SIZES = [1, 63, 64, 65, 4097]
ATTR_BLOCKS_PER_CU = 6  # launch_attr: at most 6 workgroups of 4 waves per CU, one 64-request group per wave and turn
NONE = np.int64(1 << 40)

# attributes that satisfy no rule (the default GeoIP record is {0, "XX"})
IP_NONE, PORT_NONE, ASN_NONE, CC_NONE, METHOD_NONE = (192 << 24) | (0 << 16) | (2 << 8) | 1, 9, 0, "XX", b"GET"
K_IP, K_CC, K_PCMP, K_ACMP, K_PSET, K_ASET, K_METHOD, N_KINDS = 0, 1, 2, 3, 4, 5, 6, 7  # (rule order: a comparison decides before the set that holds its constant)


def cc_name(k):
    """country k: AA, AB, ... without XX"""
    k += k >= 23 * 26 + 23
    return chr(65 + k // 26) + chr(65 + k % 26)


class Shape:
    """how many rules of each kind: SMALL needs <= 128 ip lists, <= 64 countries, <= 32 port sets, asn sets and asn comparisons"""

    def __init__(self, wide):
        self.n_ip, self.n_cc = (136, 70) if wide else (40, 34)          # ip-set words 5 / 2 (bits 0, 31, last: 7), country words 3 / 2 (last: bit 5 / 1)
        self.n_pset = self.n_aset = self.n_acmp = 40 if wide else 32     # two words (last: bit 7) / one full word
        self.n_pcmp = 230 if wide else 80                                # with the asn comparisons of a batch that carries asns: 270 / 112 comparison atoms
        self.n_method = 140 if wide else 70
        self.counts = np.array([self.n_ip, self.n_cc, self.n_pcmp, self.n_acmp, self.n_pset, self.n_aset, self.n_method])
        self.first = np.concatenate([[0], np.cumsum(self.counts)])


    def methods(self):
        return [b"M%03d" % k + (b"x" * (k % 4)) for k in range(self.n_method)]  # 4 to 7 bytes

    def rules_and_lists(self):
        rules, lists = [], {}
        for k in range(self.n_ip):
            lists[f"ip{k}"] = (_abi.LIST_IP, [f"10.{k >> 8}.{k & 255}.0/24"])
            rules.append((f"ip{k}", f'lists["ip{k}"].contains(client.ip)', [B]))
        for k in range(self.n_cc):
            rules.append((f"cc{k}", f'client.country == "{cc_name(k)}"', [B]))
        for k in range(self.n_pcmp):
            rules.append((f"pc{k}", f"client.remote_port == {3000 + k}", [B]))
        for k in range(self.n_acmp):
            rules.append((f"ac{k}", f"client.asn == {500000 + k}", [B]))
        for k in range(self.n_pset):  # (the set holds the port of its own requests and the constant of port comparison k)
            lists[f"ps{k}"] = (_abi.LIST_INT, [str(2000 + k), str(3000 + k)])
            rules.append((f"ps{k}", f'lists["ps{k}"].contains(client.remote_port)', [B]))
        for k in range(self.n_aset):
            lists[f"as{k}"] = (_abi.LIST_INT, [str(100000 + k), str(500000 + k)])
            rules.append((f"as{k}", f'lists["as{k}"].contains(client.asn)', [B]))
        for k, m in enumerate(self.methods()):
            rules.append((f"m{k}", f'http_request.method == "{m.decode()}"', [B]))
        return rules, lists


def build(shape, n, seed, tie_geo):
    """per request: the index within each kind that it is BUILT to satisfy (-1: none), by its group's pattern. tie_geo: the country
    and asn picks of a request inside an ip list follow from the list and one of four variants (the engine's table answers them from
    the address: a list's /24 has room for 254 records)."""
    rng = np.random.default_rng(seed)
    g = np.arange(n) // 64
    pattern = g % 4  # 0 mixed, 1 nothing, 2 one kind, 3 every kind
    counts = shape.counts
    # the edge atoms (first, bit 31, bit 32, last) come up far more often than a uniform draw would make them
    draw = rng.integers(0, 1 << 30, (n, N_KINDS))
    edge = np.stack([np.array([0, 31, 32 % c, c - 1])[rng.integers(0, 4, n)] for c in counts], axis=1)
    pick = np.where(rng.random((n, N_KINDS)) < 0.25, edge, draw % counts)
    on = np.zeros((n, N_KINDS), dtype=bool)
    mixed = rng.random((n, N_KINDS)) < 0.15
    on[pattern == 0] = mixed[pattern == 0]
    one = (g // 4) % N_KINDS
    sel = pattern == 2
    on[sel, one[sel]] = rng.random(int(sel.sum())) < 0.5
    on[pattern == 3] = True
    if tie_geo:
        li, v = pick[:, K_IP], draw[:, K_IP] >> 28
        for kind, mul in ((K_CC, 7), (K_ASET, 3), (K_ACMP, 5)):
            pick[:, kind] = np.where(on[:, K_IP], (li * mul + v) % counts[kind], pick[:, kind])
    # a request that satisfies both an asn set and an asn comparison has asn 500000 + k: set k and comparison k
    both_a = on[:, K_ASET] & on[:, K_ACMP]
    pick[both_a, K_ACMP] = pick[both_a, K_ASET] = np.minimum(pick[both_a, K_ASET], pick[both_a, K_ACMP])
    both_p = on[:, K_PSET] & on[:, K_PCMP]
    pick[both_p, K_PCMP] = pick[both_p, K_PSET] = np.minimum(pick[both_p, K_PSET], pick[both_p, K_PCMP])  # (port 3000 + k, k < n_pset)
    return np.where(on, pick, -1)


def attributes(shape, idx):
    """-> port, asn, country index (-1: XX) of every request"""
    port = np.where(idx[:, K_PCMP] >= 0, 3000 + idx[:, K_PCMP], np.where(idx[:, K_PSET] >= 0, 2000 + idx[:, K_PSET], PORT_NONE)).astype(np.int64)
    asn = np.where(idx[:, K_ACMP] >= 0, 500000 + idx[:, K_ACMP], np.where(idx[:, K_ASET] >= 0, 100000 + idx[:, K_ASET], ASN_NONE)).astype(np.int64)
    return port, asn, idx[:, K_CC]


def expected(shape, idx):
    """first rule (rule order = kind order) that holds for the request's attribute VALUES (a port or asn that equals a comparison's
    constant is also in the set of that number)"""
    port, asn, ci = attributes(shape, idx)

    def within(v, base, cnt):
        return np.where((v >= base) & (v < base + cnt), v - base, -1)

    holds = {K_IP: idx[:, K_IP], K_CC: ci, K_METHOD: idx[:, K_METHOD], K_PCMP: within(port, 3000, shape.n_pcmp), K_ACMP: within(asn, 500000, shape.n_acmp),
             K_PSET: np.maximum(within(port, 2000, shape.n_pset), within(port, 3000, shape.n_pset)),
             K_ASET: np.maximum(within(asn, 100000, shape.n_aset), within(asn, 500000, shape.n_aset))}
    rule = np.full(len(idx), NONE)
    for kind in range(N_KINDS):
        rule = np.minimum(rule, np.where(holds[kind] >= 0, shape.first[kind] + holds[kind], NONE))
    return np.where(rule == NONE, -1, rule)


def const_col(val, n):
    return np.concatenate([np.tile(np.frombuffer(val, dtype=np.uint8), n), np.zeros(_abi.ARENA_PAD, dtype=np.uint8)]), (np.arange(n + 1, dtype=np.uint64) * len(val)).astype(np.uint32)


def make_batch(shape, idx, from_row):
    """-> (batch, GeoIP rows or None). The engine's table answers asn / country from the ADDRESS, so with from_row every combination of
    (list, country, asn) in use gets an address and a /32 record of its own; otherwise the batch carries the two columns."""
    n = len(idx)
    port, asn, _ = attributes(shape, idx)
    port = port.astype(np.uint16)
    names = np.array([cc_name(k) for k in range(shape.n_cc)] + [CC_NONE], dtype="S2")
    cc = names[idx[:, K_CC]]  # (-1 -> XX)
    ip = np.where(idx[:, K_IP] >= 0, (10 << 24) | (np.maximum(idx[:, K_IP], 0) << 8) | 1, IP_NONE).astype(np.int64)
    rows = None
    if from_row:
        # one address per distinct (list, asn, country): list k's /24 holds 254 of them, the rest of the space is 20.0.0.0/8
        key, inv = np.unique(((idx[:, K_IP] + 1) << 40) | (asn << 10) | (idx[:, K_CC] + 1), return_inverse=True)
        uniq = np.stack([(key >> 40) - 1, (key >> 10) & ((1 << 30) - 1), (key & 1023) - 1], axis=1)
        addr = np.zeros(len(uniq), dtype=np.int64)
        used = {}
        for u, (li, a, ci) in enumerate(uniq.tolist()):
            slot = used.get(li, 0)
            used[li] = slot + 1
            if li >= 0:
                assert slot < 254, "too many (asn, country) combinations inside one list's /24"
                addr[u] = (10 << 24) | (li << 8) | (1 + slot)
            else:
                addr[u] = (20 << 24) | slot
        rows = [(f"{x >> 24}.{(x >> 16) & 255}.{(x >> 8) & 255}.{x & 255}/32", int(a), cc_name(ci) if ci >= 0 else CC_NONE)
                for x, (li, a, ci) in zip(addr.tolist(), uniq.tolist()) if not (a == ASN_NONE and ci < 0)]
        ip = addr[inv]
    ipb = np.zeros((n, 16), dtype=np.uint8)
    ipb[:, :4] = ip.astype(">u4").view(np.uint8).reshape(-1, 4)
    meth = shape.methods() + [METHOD_NONE]
    lens = np.array([len(m) for m in meth], dtype=np.int64)[idx[:, K_METHOD]]
    moff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    width = max(len(m) for m in meth)
    table = np.zeros((len(meth), width), dtype=np.uint8)
    for k, m in enumerate(meth):
        table[k, :len(m)] = np.frombuffer(m, dtype=np.uint8)
    picked = table[idx[:, K_METHOD]]
    mdata = np.concatenate([picked[np.arange(width)[None, :] < lens[:, None]], np.zeros(_abi.ARENA_PAD, dtype=np.uint8)])
    cols = [const_col(b"h.example", n), const_col(b"/", n), const_col(b"/", n), (mdata, moff), const_col(b"Mozilla/5.0", n)]
    extra = {} if from_row else {"asn": asn.astype(np.uint32), "country": np.frombuffer(cc.tobytes(), dtype="<u2")}
    return RequestBatch([c[0] for c in cols], [c[1] for c in cols], ipb, np.zeros(n, dtype=np.uint8), port, np.zeros(n, dtype=np.uint8), **extra), rows


def big_n():
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 3 * 64 * 4 * ATTR_BLOCKS_PER_CU * cus + 64 * 4 * 7 + 29  # every wave takes three groups, some a fourth; the last group is partial


@pytest.mark.parametrize("from_row", [True, False], ids=["geoip-table", "batch-columns"])
@pytest.mark.parametrize("wide", [False, True], ids=["small", "wide"])
def test_groups_of_every_kind_through_every_source_word(wide, from_row):
    shape = Shape(wide)
    n = big_n()
    idx = build(shape, n, 41 + 2 * wide + from_row, tie_geo=from_row)
    rule = expected(shape, idx)
    # every kind's edge atoms decide some request, and groups of every pattern exist beyond the second turn of the waves
    for kind, cnt in enumerate(shape.counts.tolist()):
        for k in sorted({0, 31, 32, cnt - 1}):
            assert (rule == shape.first[kind] + k).any(), (kind, k)
    per_group = (idx >= 0).any(axis=1)[: n // 64 * 64].reshape(-1, 64)
    assert (~per_group.any(axis=1)).sum() > n // 64 // 5 and per_group.all(axis=1).sum() > n // 64 // 5
    batch, rows = make_batch(shape, idx, from_row)
    rules, lists = shape.rules_and_lists()
    eng = RuleEngine(rules, lists, geoip_entries(rows) if rows else None)
    tabs = eng.address_tables()
    assert tabs["packed"] == 1, tabs
    act = np.where(rule >= 0, _abi.ACTION_BLOCK, _abi.ACTION_ALLOW).astype(np.uint8)
    want = np.where(rule >= 0, rule, _abi.RULE_NONE).astype(np.uint32)
    got, counts = eng.evaluate_batch(batch, with_counts=True)
    bad = np.nonzero((got["action"] != act) | (got["rule_idx"] != want))[0]
    assert len(bad) == 0, f"{len(bad)} of {n} verdicts differ; first at {bad[0]} (group {bad[0] // 64}, pattern {bad[0] // 64 % 4}): attributes {idx[bad[0]].tolist()} got ({got['action'][bad[0]]}, {got['rule_idx'][bad[0]]}) want ({act[bad[0]]}, {want[bad[0]]})"
    assert counts.tolist() == np.bincount(act, minlength=4).tolist()
    for size in SIZES:
        g, c = eng.evaluate_batch(batch.slice(0, size), with_counts=True)
        assert (g["action"] == act[:size]).all() and (g["rule_idx"] == want[:size]).all(), f"batch of {size}"
        assert c.tolist() == np.bincount(act[:size], minlength=4).tolist()
    eng.close()
