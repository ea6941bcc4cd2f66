"""Filter heads on the device: filter_kernel compares an anchored literal against the first 16 bytes of every request
that starts in the bytes its wave streams and stores the record of EVERY request of the pass, zero included, so that nothing clears
those records between batches. Every case here: (action, rule_idx) and the four action counters against the CPU oracle, for the engine
as built, with stride 2 forced, and with the same rules under PWAF_OPT_NO_PREFILTER; every case first asserts, through the program dump
(table_walker: f_heads), that the passes under test really have their heads. The positions are the ones at which the wave's walk of the
offsets column changes its step: every offset of a 16-byte chunk, the last chunk of a row, of an iteration and of a slab, a slab's first
byte, runs of short and empty fields, more than 128 starts in an iteration, the arena's end.

A rule of a set reads `path == "/h<k>" && !<head k holds>`: the request's path picks WHICH head decides its verdict, so every head of a
pass is observed by itself, fillers included."""
import numpy as np
import pytest

import confirm_cases
import helpers as H
import table_walker
from oracle import pyoracle
from pingoo_amd import _abi
from pingoo_amd.engine import CompiledProgram, NodeEngine, RuleEngine

pytestmark = pytest.mark.gpu
B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
ROW, ITER, SLAB = 1024, 4096, 128 * 1024  # filter_kernel: a lane's chunk is 16 bytes, a row 64 chunks, an iteration 4 rows, a wave's slab 32 iterations

# (field, literal, exact): lengths 1, 7, 8, 9, 15, 16; every pass has two heads; set A's User-Agent pass and both passes of set B have an
# exact and a prefix head side by side
SETS = {
    "A": [("user_agent", "Mozilla/", False), ("user_agent", "curl/8.5.0-abcde", True), ("url", "/", False), ("url", "/static/assets/", False)],
    "B": [("user_agent", "Mozilla", False), ("user_agent", "Mozilla/5", True), ("url", "/api/v1/accounts", False), ("url", "/health", True)],
}
assert sorted(len(lit) for heads in SETS.values() for _, lit, _ in heads) == [1, 7, 7, 8, 9, 15, 16, 16]


def rules_of(heads):
    rules = []
    for k, (f, lit, exact) in enumerate(heads):
        holds = f"http_request.{f} == {H.q(lit)}" if exact else f"http_request.{f}.starts_with({H.q(lit)})"
        rules.append((f"h{k}", f'http_request.path == "/h{k}" && !({holds})', [B] if k % 2 == 0 else [CAP]))
    # one `contains` per field: the pass is filtered
    return rules + [("ua_c", 'http_request.user_agent.contains("sqlmap")', [B]), ("url_c", 'http_request.url.contains("x9k2")', [CAP])]


class Engines:
    """One rule set: the engine as built, with stride 2 forced, without prefilters; the oracle."""

    def __init__(self, name):
        self.heads = SETS[name]
        self.rules = rules_of(self.heads)
        self.oracle = pyoracle.Oracle(self.rules, {})
        self.legs = []
        for label, flags in (("stride as chosen", 0), ("stride 2", _abi.OPT_FILTER_STRIDE2), ("no prefilter", _abi.OPT_NO_PREFILTER)):
            if flags != _abi.OPT_NO_PREFILTER:
                self.assert_heads(flags, 2 if flags else None)
            self.legs.append((label, RuleEngine(self.rules, {}, flags=flags)))

    def assert_heads(self, flags, stride):
        t = table_walker.Tables(CompiledProgram(self.rules, {}, flags=flags))
        strides = set()
        for field in ("user_agent", "url"):
            g = [g for g in t.groups if g["field"] == _abi.FIELD_NAMES.index(field) and "f_table" in g]
            assert len(g) == 1, (field, "the pass is not filtered")
            got = sorted((bytes(lit), bool(exact)) for lit, exact, _ in g[0]["f_heads"])
            assert got == sorted((lit.encode(), exact) for f, lit, exact in self.heads if f == field), (field, got)
            assert stride is None or g[0]["f_stride"] == stride
            strides.add(g[0]["f_stride"])
        # both strides with heads: the forced leg is all stride 2, so the leg as built must keep a head pass at stride 1
        assert stride is not None or 1 in strides, strides

    def check(self, batch, what, want=None):
        want = self.oracle.evaluate(batch) if want is None else want
        hist = np.bincount(want["action"], minlength=4).tolist()
        for label, eng in self.legs:
            got, counts = eng.evaluate_batch(batch, with_counts=True)
            H.assert_verdicts_equal(got, want, batch, f"{what}, {label}")
            assert counts.tolist() == hist, (what, label)
        return want

    def close(self):
        for _, eng in self.legs:
            eng.close()


@pytest.fixture(scope="module", params=["A", "B"])
def engines(request):
    e = Engines(request.param)
    yield e
    e.close()


def probes(lit, exact):
    """field values around one head: it holds; it fails in its last byte; the literal cut short by one byte (its successor's bytes must not
    complete it); the bare literal; an exact head with one byte too many"""
    alt = chr(ord(lit[-1]) ^ 1)
    tail = "" if exact else "-tail of a field that is longer than a chunk"
    return [lit + tail, lit[:-1] + alt + tail, lit[:-1], lit] + ([lit + "x"] if exact else [])


class Arena(confirm_cases.Arena):
    """A batch in which the values of ONE field are placed at chosen bytes of its arena (a request's value begins where its predecessor's
    ends: confirm_cases.Arena). Fillers carry the paths of the field's heads in turn, so their records count too."""

    def __init__(self, heads, field):
        super().__init__(field, [k for k, (f, _, _) in enumerate(heads) if f == field])
        self.heads = heads

    def place_all(self, start, step, piece=200, skip=lambda p: False):
        """every probe of every head of the field, each at the next byte == start (mod step)"""
        for k in self.ks:
            for v in probes(self.heads[k][1], self.heads[k][2]):
                p = self.at(start, step)
                while skip(p):
                    p += step
                self.pad_to(p, piece)
                self.add(v, k)


@pytest.mark.parametrize("field", ["user_agent", "url"])
def test_every_offset_in_a_chunk_and_the_last_chunk_of_rows_and_iterations(engines, field):
    a = Arena(engines.heads, field)
    for o in range(16):
        a.place_all(o, 16)  # every offset of a chunk, chunks anywhere in a row
    for o in range(16):
        a.place_all(ROW - 16 + o, ROW, skip=lambda p: p % ITER > ITER - ROW)  # bytes 1008..1023 of a KiB: the bytes continue in lane 0 of the next row
    for o in range(16):
        a.place_all(ITER - 16 + o, ITER, piece=1500, skip=lambda p: p % SLAB > SLAB - ITER)  # 4080..4095 of 4 KiB: ... in the next iteration's row 0
    batch = a.batch()
    assert a.cur > 3 * SLAB
    want = engines.check(batch, f"offsets, rows, iterations ({field})")
    assert len(set(want["action"].tolist())) == 3


@pytest.mark.parametrize("field", ["user_agent", "url"])
def test_starts_at_the_end_of_a_slab_and_at_its_first_byte(engines, field):
    """within the last 15 bytes of a wave's slab (the bytes continue behind the slab) and exactly at the next slab's first byte; fields
    of 2 - 40 KiB between them"""
    a = Arena(engines.heads, field)
    for o in range(16):
        a.place_all(SLAB - o, SLAB, piece=(2048, 40000, 9000)[o % 3])
    batch = a.batch()
    want = engines.check(batch, f"slab edges ({field})")
    assert len(set(want["action"].tolist())) == 3


@pytest.mark.parametrize("field", ["user_agent", "url"])
def test_neighbours_short_fields_and_more_than_128_starts_in_an_iteration(engines, field):
    a = Arena(engines.heads, field)
    lits = [(k, engines.heads[k][1]) for k in a.ks]
    for k, lit in lits:
        for cut in range(1, len(lit)):  # "Mozi" then "lla/5.0": two fields whose bytes together read as the literal
            a.pad_to(a.at(cut % 16, 16))
            a.add(lit[:cut], k)
            a.add(lit[cut:] + "5.0", k)
    # two to sixteen requests that start in one chunk: empty fields, fields of 1 - 3 bytes, the shortest literal and its near misses
    short = min(lits, key=lambda x: len(x[1]))
    for count in range(2, 17):
        for o in (0, 16 - count if count < 16 else 0, 15):
            a.pad_to(a.at(o, 16))
            for j in range(count):
                a.add(["", "a", short[1][:1], "zz", "", short[1][:3], "q"][(j + count) % 7], short[0] if j % 2 else None)
            a.add(short[1] + "-after a run", short[0])
    for k, lit in lits:  # the literal as a whole field several times over: every one of them holds, wherever in a chunk it starts
        for reps in range(2, 6):
            a.pad_to(a.at(0, 16))
            for _ in range(reps):
                a.add(lit, k)
    # more than 128 starts inside 4 KiB (the synchronous loop), twice: from an iteration's first byte and from its middle
    for start in (0, 2000):
        a.pad_to(a.at(start, ITER), piece=1500)
        for j in range(330):
            k, lit = lits[j % len(lits)]
            a.add([lit, lit[:-1], "no", lit + "/x", ""][j % 5], k)
    # long fields between probes
    for j, size in enumerate((2048, 40000, 4096, 17000)):
        k, lit = lits[j % len(lits)]
        a.add(lit + "L" * size, k)
        a.add(lit[:-1] + "~" + "L" * size, k)
    batch = a.batch()
    want = engines.check(batch, f"neighbours ({field})")
    assert len(set(want["action"].tolist())) == 3


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches_and_empty_fields_at_the_arena_end(engines, n):
    heads = engines.heads
    for field in ("user_agent", "url"):
        a = Arena(heads, field)
        vals = [v for k in a.ks for v in probes(heads[k][1], heads[k][2])]
        for j in range(n):
            a.add(vals[j % len(vals)] if j % 3 else vals[j % len(vals)] + "+" * (j % 40), a.ks[j % 2])
        engines.check(a.batch(), f"n = {n} ({field})")
        # the last requests' fields empty: they start AT the arena's end, where no wave enumerates a request
        for empties in (1, 2, 70):
            b = Arena(heads, field)
            b.reqs, b.cur = list(a.reqs), a.cur
            for j in range(empties):
                b.add("", a.ks[j % 2])
            engines.check(b.batch(), f"n = {n} + {empties} empty at the end ({field})")
        # the field empty for every request: an arena without a byte
        c = Arena(heads, field)
        for j in range(n):
            c.add("", c.ks[j % 2])
        want = engines.check(c.batch(), f"n = {n}, every field empty ({field})")
        assert (want["action"] != 0).all()


@pytest.mark.parametrize("field", ["user_agent", "url"])
def test_slab_views_and_node_shares(engines, field):
    """an arena whose offsets[0] > 0: views that begin inside a chunk, inside a slab and exactly on a slab; the shares of a two-replica node"""
    a = Arena(engines.heads, field)
    for o in (0, 5, 15):
        a.place_all(o, 16)
    a.place_all(SLAB - 3, SLAB, piece=9000)
    a.place_all(0, SLAB, piece=9000)
    for _ in range(3):
        a.add("")
    batch = a.batch()
    want = engines.oracle.evaluate(batch)
    offs = batch.offsets[_abi.FIELD_NAMES.index(field)]
    on_slab = [i for i in range(1, batch.n) if int(offs[i]) % SLAB == 0 and int(offs[i]) > 0][0]
    for lo in (1, 2, 7, on_slab - 1, on_slab, on_slab + 1, batch.n - 2):
        view = batch.view(lo, batch.n)
        engines.check(view, f"view from request {lo} ({field})", want=want[lo:])
    node = NodeEngine(engines.rules, devices=[0, 0])
    got, counts = node.evaluate_batch(batch, with_counts=True)
    H.assert_verdicts_equal(got, want, batch, f"node ({field})")
    assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist()
    node.close()


@pytest.mark.parametrize("field", ["user_agent", "url"])
def test_a_context_used_again_sees_no_record_of_the_batch_before(engines, field):
    """Two batches of the same shape in turn through the same engines (every scratch context of an engine meets both): the second has a
    head miss exactly where the first has a hit, and the other way round. Nothing clears the records between batches, so a record the
    filter failed to rewrite would show as a stale hit (or a stale miss)."""
    heads = engines.heads

    def build(flip):
        a, at = Arena(heads, field), []
        j = 0
        for o in (0, 3, 8, 13):
            for k in a.ks:
                lit, exact = heads[k][1], heads[k][2]
                hit, miss = probes(lit, exact)[0], probes(lit, exact)[1]
                assert len(hit) == len(miss)
                for _ in range(6):
                    a.pad_to(a.at(o, 16))
                    at.append(len(a.reqs))
                    a.add(hit if (j % 2 == 0) != flip else miss, k)
                    j += 1
        for _ in range(5):  # (and at the arena's end: the records the last slab's wave writes)
            a.add("", a.ks[0])
        return a.batch(), at

    (b0, at), (b1, _) = build(False), build(True)
    w0, w1 = engines.oracle.evaluate(b0), engines.oracle.evaluate(b1)
    assert ((w0["action"] != 0) != (w1["action"] != 0))[at].all() and len(at) == 48
    for turn in range(4):
        engines.check(b0, f"first batch, turn {turn} ({field})", want=w0)
        engines.check(b1, f"second batch, turn {turn} ({field})", want=w1)
