"""Shared builders of the resolve / confirm edge suites (tests/test_confirm_edges_cpu.py, tests/test_gpu_confirm_edges.py); no GPU import.

The chain under test: filter_kernel flags 16-byte arena chunks, resolve_kernel turns the flagged chunks of a pass with a confirm tier
into (owning request, chunk) pairs and zeroes the records of the requests that have a byte in them, confirm_kernel compares the
windows that completed in a pair's chunk (csrc/confirm.h) and merges the literal atoms it confirms into those records. Here:

  * RuleSet: one rule per literal predicate under observation. Verdict form `http_request.path == "/h<k>" && <predicate k>`: the
    request's path picks WHICH predicate decides its verdict; bare form `<predicate k>` for the hit-matrix leg (PWAF_OPT_RULE_HITS).
  * Arena: a batch in which the values of ONE field are placed at chosen bytes of its arena.
  * PassShape: a whole-arena numpy model of filter_kernel over a pass's dumped filter table -- the flagged chunks, their number per
    slab, the pair list, each pair's owner, the requests that start in a chunk -- so that every case PROVES its shape before a device
    is involved.
  * the cases, A to J, each returning the batches it sends and what the model measured."""
import functools
import random

import numpy as np

import helpers as H
import table_walker
from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.engine import CompiledProgram

B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
CHUNK = 16
SLAB = 128 * 1024      # csrc/kernels.h, kStreamSlab: the bytes one wave of filter_kernel / resolve_kernel owns
RESOLVE_SPARSE = 128   # csrc/filter.hip, resolve_kernel: kResolveSparse, flagged chunks up to which a slab is resolved chunk by chunk
OWNER_BOUND = 4096     # csrc/filter.hip, resolve_kernel: `h = min(a.n, lo + 4096u)`, the owner search of the chunk-driven path
RESET_BOUND = 48       # csrc/filter.hip, resolve_kernel: `steps < 48u`, the record reset of the chunk-driven path
QUEUE = 1024           # csrc/confirm.hip, confirm_kernel: kConfirmQueue, a workgroup's queue of walk-list appends
POOL_WORDS = 10240     # csrc/kernels.h, kConfirmPoolBytes / 4: confirm_kernel's LDS pool for entries + bytes + classes
CONFIRM_THREADS = 1024  # csrc/kernels.h, kConfirmThreads: pairs per work item of confirm_kernel
MI355X_CUS = 256       # launch_confirm's grid is 2 workgroups per compute unit; the CPU suite builds case J for this device


class Arena:
    """A batch in which the values of ONE field are placed at chosen bytes of its arena (a request's value begins where its predecessor's
    ends). `ks`: the keys (the k of path "/h<k>") that fillers carry in turn, so that their records count too."""

    filler_head, filler_byte = "filler-", "q"

    def __init__(self, field, ks):
        self.field, self.reqs, self.cur, self.turn = field, [], 0, 0
        self.ks = list(ks)

    def add(self, value, k=None):
        if k is None:
            k, self.turn = self.ks[self.turn % len(self.ks)], self.turn + 1
        other = {"url": "/i", "user_agent": "ua"}
        other[self.field] = value
        self.reqs.append(Request(host="h", path=f"/h{k}", **other))
        self.cur += len(value)

    def fill(self, size, k=None):
        """one filler of exactly `size` bytes (shorter than the filler's head: a cut of it)"""
        self.add((self.filler_head + self.filler_byte * max(0, size - len(self.filler_head)))[:size], k)

    def pad_to(self, pos, piece=200):
        """fillers of 16 bytes or more each (one start per chunk) up to arena byte pos"""
        assert pos >= self.cur and (pos == self.cur or pos - self.cur >= 16), (pos, self.cur)
        while self.cur < pos:
            k = pos - self.cur
            self.fill(k if k < piece + 16 else piece)

    def at(self, start, step, lo=16):
        """the first byte == start (mod step) that leaves room for a filler"""
        p = (self.cur + lo - start + step - 1) // step * step + start
        return p

    def batch(self):
        return RequestBatch.from_requests(self.reqs)


# ---------------------------------------------------------------------------------------------------------
# the numpy model of filter_kernel over a whole arena
# ---------------------------------------------------------------------------------------------------------
def window_positions(g, data, total, behind=None):
    """filter_kernel restated (csrc/filter.hip, filter_rows): ONE shift-or automaton over the arena as a flat byte stream, started in
    the pass's init state at byte 0, a lookup table[bin(fold(b[i]), fold(b[i + 1]))] at every stride-th byte i, state = state << 8 |
    mask; a window completed at i when the state's top byte has a zero bit. Nothing depends on where requests begin or end.
    -> bool per arena byte of the chunks that begin before `total` (the bytes behind `total` are the arena's slack).
    `behind`: the byte the stream's LAST position -- byte n - 1 of the last chunk, n = total rounded up to whole chunks -- is paired with
    at stride 1. None: the arena's own byte n, which is what a case needs to prove its shape; the byte the kernel really pairs it with
    is not the arena's (tests/filter_cases.py: byte_behind, which the device comparison uses)."""
    n = (int(total) + CHUNK - 1) // CHUNK * CHUNK
    d = np.zeros(n + 1, dtype=np.uint32)
    k = min(len(data), n + 1)
    d[:k] = data[:k]
    if behind is not None:
        d[n] = int(behind)
    d &= ~((d >> 1) & 0x20)  # program.h: filter_fold
    bins = (((d[:-1] | (d[1:] << 8)) * int(g["f_mul"])) & 0xFFFF) >> 4
    s = int(g["f_stride"])
    m = np.asarray(g["f_table"], dtype=np.uint32)[bins][::s]
    top = (m >> 24) & 0xFF
    init = int(g["f_init"])
    for j in (1, 2, 3):
        prev = np.concatenate([np.zeros(j, dtype=np.uint32), m[:-j]]) if len(m) > j else np.zeros(len(m), dtype=np.uint32)
        top |= (prev >> (24 - 8 * j)) & 0xFF
    for t in range(min(3, len(m))):  # the first three positions still see the init state
        top[t] |= (init >> (16 - 8 * t)) & 0xFF
    out = np.zeros(n, dtype=bool)
    out[::s] = top != 0xFF
    return out


class PassShape:
    """What resolve_kernel and confirm_kernel are handed for one pass of one batch, by the model."""

    def __init__(self, g, batch, field_id):
        off = batch.offsets[field_id].astype(np.int64)
        self.off, self.n, self.total, self.stride = off, batch.n, int(off[-1]), int(g["f_stride"])
        self.windows = window_positions(g, batch.data[field_id], self.total)
        pos = np.nonzero(self.windows)[0]
        self.chunks = np.unique(pos // CHUNK)  # the flagged chunks = the pass's pairs, one each
        self.windows_in = dict(zip(*[x.tolist() for x in np.unique(pos // CHUNK, return_counts=True)]))  # chunk -> completed windows
        self.n_slabs = (self.total + SLAB - 1) // SLAB
        self.per_slab = np.bincount(self.chunks // (SLAB // CHUNK), minlength=self.n_slabs)
        byte0 = self.chunks * CHUNK
        # the request that holds the chunk's first byte: the first r with off[r + 1] > byte0 (resolve_kernel, both paths)
        self.owner = np.searchsorted(off[1:], byte0, side="right")
        assert (self.owner < self.n).all(), "a flagged chunk that no request owns"
        self.starts = np.searchsorted(off[:-1], byte0 + CHUNK, side="left") - np.searchsorted(off[:-1], byte0, side="left")
        # the chunk-driven path: `lo`, the first request with off[r + 1] + 3 stride > the slab's first byte, bounds the owner search
        # to [lo, lo + OWNER_BOUND); the reset loop steps from the owner over the requests that start before the chunk's end
        slab_b0 = self.chunks // (SLAB // CHUNK) * SLAB
        self.slab_first = np.searchsorted(off[1:] + 3 * self.stride, slab_b0, side="right")
        self.owner_rel = self.owner - self.slab_first
        self.reset_steps = np.searchsorted(off[:-1], byte0 + CHUNK, side="left") - self.owner
        # the flag-density switch (pipeline.cpp: dense_thresh): above it the pass is walked whole and nothing is confirmed
        self.dense_thresh = self.n_slabs * (SLAB // CHUNK) // 2

    @property
    def pairs(self):
        return len(self.chunks)

    def chunks_of(self, r):
        """flagged chunks with a byte of request r"""
        lo, hi = int(self.off[r]), int(self.off[r + 1])
        return [] if hi <= lo else [int(c) for c in self.chunks[(self.chunks >= lo // CHUNK) & (self.chunks <= (hi - 1) // CHUNK)]]

    def requests_in(self, c):
        """the requests that start in chunk c"""
        lo = int(np.searchsorted(self.off[:-1], c * CHUNK, side="left"))
        return list(range(lo, int(np.searchsorted(self.off[:-1], (c + 1) * CHUNK, side="left"))))

    def summary(self):
        redo_owner = self.owner_rel >= OWNER_BOUND
        return dict(pairs=self.pairs, slabs=int(self.n_slabs), per_slab=self.per_slab.tolist(), max_owner_rel=int(self.owner_rel.max()) if self.pairs else 0,
                    max_starts=int(self.starts.max()) if self.pairs else 0, max_windows=max(self.windows_in.values()) if self.pairs else 0,
                    owner_redo=int(redo_owner.sum()), dense_thresh=int(self.dense_thresh))


# ---------------------------------------------------------------------------------------------------------
# rule sets
# ---------------------------------------------------------------------------------------------------------
class RuleSet:
    """preds[k] = (predicate text, or a bare literal standing for `<field>.contains(literal)`). Programs are compiled on the host only
    and cached per flags; pass_of() is the ONE filtered pass with a confirm tier on the field."""

    def __init__(self, name, field, preds, verdict_form=True):
        self.name, self.field, self.field_id = name, field, _abi.FIELD_NAMES.index(field)
        self.preds = [p if p.startswith("http_request.") else f"http_request.{field}.contains({H.q(p)})" for p in preds]
        self.bare_rules = [(f"b{k}", p, [B] if k % 2 == 0 else [CAP]) for k, p in enumerate(self.preds)]
        self.verdict_rules = [(f"h{k}", f'http_request.path == "/h{k}" && {p}', [B] if k % 2 == 0 else [CAP]) for k, p in enumerate(self.preds)] if verdict_form else self.bare_rules
        self.keys = list(range(len(self.preds)))
        self._programs = {}

    def rules(self, flags=0):
        return self.bare_rules if flags & _abi.OPT_RULE_HITS else self.verdict_rules

    def program(self, flags=0):
        if flags not in self._programs:
            p = CompiledProgram(self.rules(flags), {}, flags=flags)
            self._programs[flags] = (p, table_walker.Tables(p))
        return self._programs[flags]

    def pass_of(self, flags=0):
        """-> (pass index, its dump entry): the field's filtered pass with a confirm tier"""
        _, t = self.program(flags)
        found = [(gi, g) for gi, g in enumerate(t.groups) if g["field"] == self.field_id and "f_table" in g]
        assert len(found) == 1, (self.name, self.field, "filtered passes on the field:", len(found))
        assert found[0][1].get("confirm") == 1, (self.name, "the pass has no confirm tier")
        return found[0]

    def confirm_shape(self, flags=0):
        return self.program(flags)[0].confirm_shape(self.pass_of(flags)[0])

    def shape(self, batch, flags=0):
        return PassShape(self.pass_of(flags)[1], batch, self.field_id)

    def arena(self):
        return Arena(self.field, self.keys)


class Case:
    """batches: [(label, batch)] sent in this order (a case with more than one sends them in turn, several times); measured: what the
    model and the shape hook said, for the report."""

    def __init__(self, name, rs, batches, measured, turns=1):
        self.name, self.rs, self.batches, self.measured, self.turns = name, rs, batches, measured, turns


def below_dense(sh, what):
    assert sh.pairs <= sh.dense_thresh, f"{what}: {sh.pairs} flagged chunks of {sh.n_slabs} slabs: the pass would be walked whole and nothing confirmed"


# --- set S: short literals on the url, a pass without heads (its records are zeroed by resolve_kernel alone) ---
S_LITS = ["aaa", "zq", "kw#7x", "x9k2", "Zm", "pp=1", "#!b"]
S_REGEX, S_REGEX_HIT = "zz[0-9]y", "zz7y"  # a short regex: a walk entry next to the literals (its requests go through the walk list and the R-tier DFA)
K_AAA, K_ZQ, K_KW, K_X9, K_ZM, K_PP, K_HB, K_RX = range(8)


@functools.lru_cache(maxsize=None)
def set_s():
    rs = RuleSet("S", "url", S_LITS + [f"http_request.url.matches({H.q(S_REGEX)})"])
    for flags in (0, _abi.OPT_RULE_HITS):
        gi, g = rs.pass_of(flags)
        assert len(g["f_heads"]) == 0 and g["f_stride"] == 1 and g["confirm_literals"] == len(S_LITS) and g["confirm_walk"], (flags, g["f_stride"])
    return rs


def assert_fillers_flag_nothing(rs, sizes=(16, 17, 31, 200, 216, 1500, 3000)):
    a = rs.arena()
    for _ in range(3):
        for s in sizes:
            a.fill(s)
    for flags in (0, _abi.OPT_RULE_HITS):
        assert rs.shape(a.batch(), flags).pairs == 0, "fillers flag a chunk"


@functools.lru_cache(maxsize=None)
def case_b():
    """B. windows per chunk (confirm_bin_of past the fourth window: the bin is recomputed from a reload), and the arena's first and last
    chunks (the narrow form of confirm_chunk_bytes): runs of 'a' of 1..40 bytes under `contains("aaa")`, each starting at every offset
    of a chunk; the batch begins with a run at arena byte 0 and ends with one."""
    rs = set_s()
    assert_fillers_flag_nothing(rs)
    a = rs.arena()
    a.add("a" * 21, K_AAA)
    for length in range(1, 41):
        for o in range(16):
            a.pad_to(a.at(o, 16))
            a.add("a" * length, K_AAA if (length + o) % 5 else K_ZQ)  # (under another literal's key the run decides nothing)
    # a fifth and later window whose bigram is NOT the run's: the bin recomputed from the reload must be that window's own
    tails = []
    for o in range(16):
        for tail, k in (("zq", K_ZQ), ("#!b", K_HB), ("x9k2", K_X9), (S_REGEX_HIT, K_RX), ("zp", K_ZQ)):
            a.pad_to(a.at(o, 16))
            if o == 0:
                tails.append(len(a.reqs))
            a.add("a" * 6 + tail, k)
    a.pad_to(a.at(3, 16))
    a.add("a" * 19, K_AAA)
    batch = a.batch()
    sh = rs.shape(batch)
    below_dense(sh, "B")
    counts = set(sh.windows_in.values())
    assert {1, 4, 5, 16} <= counts, sorted(counts)
    assert all(sh.windows_in[int(sh.off[r]) // CHUNK] >= 5 for r in tails[:4]), "no fifth window of another bin"
    assert 0 in sh.chunks and (sh.total - 1) // CHUNK in sh.chunks and sh.total % CHUNK != 0, "the arena's first and last chunks are not flagged"
    # one request alone in its arena: its chunk is the first and the last at once
    single = [("B one request", RequestBatch.from_requests([Request(host="h", path=f"/h{K_AAA}", url="a" * n, user_agent="ua")])) for n in (2, 3, 7, 16, 20)]
    return Case("B", rs, [("B runs", batch)] + single, dict(model=sh.summary(), windows_per_chunk=sorted(counts)))


S2_LITS = ["aaa", "kw#7x", "x9k2", "pp=1", "#!b"]


@functools.lru_cache(maxsize=None)
def set_s2():
    """set S without its 2-byte literals: a pass that PWAF_OPT_FILTER_STRIDE2 really samples at every second byte"""
    rs = RuleSet("S2", "url", S2_LITS + [f"http_request.url.matches({H.q(S_REGEX)})"])
    assert rs.pass_of(0)[1]["f_stride"] == 1 and rs.pass_of(_abi.OPT_FILTER_STRIDE2)[1]["f_stride"] == 2 and rs.pass_of(_abi.OPT_FILTER_STRIDE2 | _abi.OPT_RULE_HITS)[1]["f_stride"] == 2
    return rs


@functools.lru_cache(maxsize=None)
def case_c():
    return _case_c("C", set_s(), [(K_ZQ, "zq"), (K_HB, "#!b"), (K_KW, "kw#7x"), (K_RX, S_REGEX_HIT)], [(K_X9, "x9k2"), (K_AAA, "aaa")], 0)


@functools.lru_cache(maxsize=None)
def case_c2():
    """C at stride 2 (literals of 3, 4 and 5 bytes: a 2-byte literal keeps its pass at stride 1); the shape is asserted on the stride-2 tables"""
    return _case_c("C2", set_s2(), [(3, "pp=1"), (4, "#!b"), (1, "kw#7x"), (5, S_REGEX_HIT)], [(2, "x9k2"), (0, "aaa")], _abi.OPT_FILTER_STRIDE2)


def _case_c(name, rs, lits, more, flags):
    """C. several requests in one chunk (confirm_kernel's `while (pos >= fe && r + 1u < a.n)`, settle(r, ..., false) for the earlier
    ones): 2 to 16 requests that start in one chunk, empty fields between them, literals of 2, 3 and 5 bytes; the hit in the first, a
    middle and the last request of the chunk; two different hits in one chunk; a literal split across two adjacent requests, which
    must not match although its chunk is flagged."""
    a = rs.arena()
    k_other = more[1][0]
    groups, splits = [], []
    for count in range(2, 17):
        for where in ("first", "middle", "last"):
            for k, lit in lits:
                at = {"first": 0, "middle": count // 2, "last": count - 1}[where]
                budget = 15 - len(lit)  # bytes the other requests of the chunk may take: the last one still starts inside it
                vals = []
                for j in range(count):
                    if j == at:
                        vals.append(lit)
                    elif j % 2 and budget > 0:
                        vals.append("zk#qx!"[j % 6])  # one byte, often the literal's own: must not complete it across a boundary
                        budget -= 1
                    else:
                        vals.append("")
                a.pad_to(a.at(0, 16))
                first = len(a.reqs)
                for j, v in enumerate(vals):
                    a.add(v, k if (j + count) % 4 else k_other)  # (most requests of the chunk are observed under the hit's own key)
                groups.append((first, count, first + at))
                a.add("-tail of the group, longer than a chunk-", k)
    # two different hits in one chunk, each observed under its own key and under the other's
    # (the regex factor in an EARLIER request of the chunk than a literal: the walk it calls for is settled as the lane moves on)
    for (ka, la), (kb, lb) in ((lits[0], lits[1]), (lits[1], lits[2]), (lits[2], lits[0]), (lits[3], lits[0]), (lits[3], lits[1]), (lits[2], lits[3])):
        for own in (True, False):
            a.pad_to(a.at(1, 16))
            two = len(a.reqs)
            a.add(la, ka if own else kb)
            a.add("", ka)
            a.add(lb, kb if own else ka)
            groups.append((two, 3, two))
    for k, lit in lits + more:
        for cut in range(1, len(lit)):
            for gap in (0, 1, 3):
                for o in (0, 7, 16 - len(lit) + cut - 1):  # (the last: the boundary is the chunk's too)
                    a.pad_to(a.at(o % 16, 16))
                    splits.append((len(a.reqs), len(a.reqs) + gap + 1))
                    a.add(lit[:cut], k)
                    for _ in range(gap):
                        a.add("", k)
                    a.add(lit[cut:], k)
    a.pad_to(a.at(0, 16))
    batch = a.batch()
    sh = rs.shape(batch, flags)
    below_dense(sh, name)
    for first, count, hit in groups:
        c = int(sh.off[hit]) // CHUNK
        assert c in sh.windows_in, ("the hit's chunk is not flagged", first, count)
        assert set(range(first, first + count)) <= set(sh.requests_in(c)), ("the group does not start in one chunk", first, count)
    assert {count for _, count, _ in groups} >= set(range(2, 17)) and sh.starts.max() >= 16
    flagged_splits = sum(1 for r, last in splits if sh.chunks_of(r) or sh.chunks_of(last))
    assert flagged_splits == len(splits), f"only {flagged_splits} of {len(splits)} split literals flag their chunk"
    return Case(name, rs, [(name, batch)], dict(model=sh.summary(), stride=sh.stride, groups=len(groups), splits=len(splits)))


def _hit_value(k):
    return "--" + S_LITS[k] + "--"


@functools.lru_cache(maxsize=None)
def case_d():
    """D. the sparse switch of resolve_kernel (`cnt <= kResolveSparse`): slabs with exactly 0, 1, 1, 64, 65, 127, 128, 129 and 200
    flagged chunks (counted by the model), fillers that flag nothing between them; the one flagged chunk as a slab's chunk 0 and as
    its chunk 8191; a literal straddling a slab boundary."""
    rs = set_s()
    assert_fillers_flag_nothing(rs)
    a = rs.arena()
    plan = [0, "first", "last", 64, 65, 127, 128, 129, 200]
    j = 0
    for s, what in enumerate(plan):
        base = s * SLAB
        if what == "first":  # the literal's window completes in the slab's chunk 0 (and the literal straddles the boundary: it begins 2 bytes before)
            a.pad_to(base - 2, piece=3000)
            a.add("x9k2--", K_X9)
            continue
        if what == "last":
            a.pad_to(base + SLAB - 8, piece=3000)
            a.add("-x9k2-", K_X9)
            continue
        for i in range(int(what)):
            p = base + 64 + (SLAB - 128) // int(what) * i // 16 * 16 + 2
            a.pad_to(p, piece=3000)
            k = (K_X9, K_ZQ, K_KW, K_HB)[j % 4]
            a.add(_hit_value(k), k if j % 3 else K_AAA)  # literal at chunk bytes 4..: one flagged chunk each
            j += 1
    a.pad_to(len(plan) * SLAB + 40, piece=3000)
    batch = a.batch()
    sh = rs.shape(batch)
    below_dense(sh, "D")
    per = sh.per_slab.tolist()
    assert per[:9] == [0, 1, 1, 64, 65, 127, 128, 129, 200] and sum(per[9:]) == 0 and sh.n_slabs == 10, per
    in_slab = sh.chunks % (SLAB // CHUNK)
    assert in_slab[sh.chunks // (SLAB // CHUNK) == 1].tolist() == [0] and in_slab[sh.chunks // (SLAB // CHUNK) == 2].tolist() == [SLAB // CHUNK - 1]
    assert (sh.owner_rel < OWNER_BOUND).all() and (sh.reset_steps < RESET_BOUND).all()  # (the switch alone: no fall-back of the chunk-driven path)
    return Case("D", rs, [("D", batch)], dict(model=sh.summary()))


def _small(rng):
    return "f" + "".join(rng.choice("qjv") for _ in range(rng.randint(7, 23)))


E_SECOND = "--pp=1--"  # what the owners hold in the second batch: another literal of the pass, of _hit_value(K_X9)'s length


@functools.lru_cache(maxsize=None)
def case_e():
    """E. the owner bound of the chunk-driven path (`l == h0` -> redo): slabs whose one flagged chunk is owned by the request 4 095,
    4 096 and 4 097 after the slab's first (fields of 8 - 24 bytes in front of it), and a last slab with fewer than 4 096 requests
    left in the batch (h0 == a.n), the owner near its end. Two batches of identical offsets in turn, twice, as in G: the owners hold
    "x9k2" in the first and "pp=1" in the second, observed under x9k2's key, so the fall-back has to zero the owner's record too."""
    rs = set_s()
    want = [OWNER_BOUND - 1, OWNER_BOUND, OWNER_BOUND + 1, OWNER_BOUND - 200]

    def build(second):
        rng = random.Random(4096)
        a = rs.arena()
        a.fill(40)
        hits = []
        for s, rel in enumerate(want):
            a.pad_to((s + 1) * SLAB - 20, piece=3000)
            a.fill(40)  # the slab's first request: the one that holds its first byte
            for _ in range(rel - 2):
                a.add(_small(rng))
            a.pad_to(a.at(0, 16))  # one filler (16 .. 31 bytes); the hit begins its chunk, so it owns the chunk's first byte
            hits.append(len(a.reqs))
            a.add(E_SECOND if second else _hit_value(K_X9), K_X9)
            if s == len(want) - 1:
                for _ in range(100):  # fewer than OWNER_BOUND requests from the slab's first to the batch's end
                    a.add(_small(rng))
        return a.batch(), hits

    (batch, hits), (batch2, _) = build(False), build(True)
    assert len(E_SECOND) == len(_hit_value(K_X9)) and all((batch.offsets[f] == batch2.offsets[f]).all() for f in range(5))
    sh = rs.shape(batch)
    for s in (sh, rs.shape(batch2)):
        below_dense(s, "E")
        assert s.per_slab.tolist() == [0, 1, 1, 1, 1], s.per_slab.tolist()
        assert s.owner.tolist() == hits
        assert (s.owner_rel == sh.owner_rel).all()
    rel = sh.owner_rel.tolist()
    assert set(rel[:3]) == {OWNER_BOUND - 1, OWNER_BOUND, OWNER_BOUND + 1}, rel
    # (the last slab's owner cannot sit AT the bound: with h0 == a.n fewer than 4 096 requests are left. The branch `l == h0 && h0 == a.n`,
    # which writes a kNone pair, is unreachable by construction -- the filter flags no chunk at or beyond off[n] -- and has no test.)
    assert rel[3] < OWNER_BOUND and int(sh.slab_first[3]) + OWNER_BOUND > batch.n, (rel, batch.n)
    return Case("E", rs, [("E first", batch), ("E second", batch2)], dict(model=sh.summary(), owner_rel=rel, n=batch.n), turns=2)


F_STARTS = (45, 46, 47, 48, 49, 70)


@functools.lru_cache(maxsize=None)
def case_f():
    """F. the reset bound of the chunk-driven path (`steps == 48u` -> redo): 45 to 49 and 70 requests that start in one flagged chunk
    (empty fields and 1-byte fields), the last but one of them the hit; the reset loop takes one step more, for the request that owns the
    chunk's first byte. Two batches of identical offsets in turn, twice, as in G: every hit holds another literal of the pass in the
    second batch ("pp=1" for "x9k2", "Zm" for "zq"), observed under the first's key, so the fall-back has to zero the hit's record too."""
    rs = set_s()

    def build(second):
        a = rs.arena()
        hits = []
        for rep, (k, k2) in enumerate(((K_X9, K_PP), (K_ZQ, K_ZM))):
            assert len(S_LITS[k]) == len(S_LITS[k2])
            for starts in F_STARTS:
                a.pad_to(a.at(1, 16))  # the filler before ends one byte into the chunk: it owns the chunk's first byte
                for j in range(starts - 2):  # (+ the hit and the filler behind it, which still starts inside the chunk)
                    a.add("v" if j % 9 == 4 and j < 40 else "", k if j % 2 else K_AAA)
                hits.append(len(a.reqs))
                a.add(_hit_value(k2 if second else k), k)
        a.pad_to(a.at(0, 16))
        return a.batch(), hits

    (batch, hits), (batch2, _) = build(False), build(True)
    assert all((batch.offsets[f] == batch2.offsets[f]).all() for f in range(5))
    measured = []
    for b in (batch, batch2):
        sh = rs.shape(b)
        below_dense(sh, "F")
        at = {int(c): i for i, c in enumerate(sh.chunks)}
        got = []
        for h in hits:
            c = int(sh.off[h]) // CHUNK
            assert c in at, "the run's chunk is not flagged"
            assert sh.owner[at[c]] < h - 40, "the chunk's owner is not the request in front of the run"
            got.append((int(sh.starts[at[c]]), int(sh.reset_steps[at[c]])))
        assert [s for s, _ in got] == list(F_STARTS) * 2 and all(st == s + 1 for s, st in got), got
        assert sh.per_slab.max() <= RESOLVE_SPARSE
        measured.append((sh.summary(), got[:len(F_STARTS)]))
    return Case("F", rs, [("F first", batch), ("F second", batch2)], dict(model=measured[0][0], starts_and_reset_steps=measured[0][1]), turns=2)


G_CELLS = ["aaa.....", "zq......", "kw#7x...", "x9k2....", "Zm......", "pp=1....", "#!b....."]
G_MISS = ["aab.....", "zp......", "kw#7y...", "x9k3....", "Zn......", "pp=2....", "#!c....."]


@functools.lru_cache(maxsize=None)
def case_g():
    """G. stale records: two batches of identical offsets sent in turn, four turns, through the same engines. Every observed request
    holds other literals of the pass in the second batch than in the first, or near misses: one or two literals against three or
    more (an overflow chain in the record pool) both ways round, a literal against another, a literal against none. One slab with at
    most 128 flagged chunks (the chunk-driven path zeroes the records) and one with more (the request-driven walk does)."""
    rs = set_s()

    def value(cells):
        return "".join(G_CELLS[c] if c >= 0 else G_MISS[-c - 1] for c in cells)

    def build(second):
        a, at = rs.arena(), []
        j = 0
        for slab, count in ((0, 36), (1, 150)):
            for i in range(count):
                a.pad_to(slab * SLAB + 64 + i * 800 + (i % 16), piece=500)
                kind = j % 6
                x, y, z = j % 7, (j + 2) % 7, (j + 4) % 7
                first, then = [((x, y, z), (-x - 1, -y - 1, y)), ((x, -y - 1, -z - 1), (y, z, x)), ((x, y, z), (-x - 1, -y - 1, -z - 1)),
                               ((-x - 1, -y - 1, -z - 1), (x, y, z)), ((x, y, -z - 1), (z, -x - 1, y)), ((x, x, x), (y, y, y))][kind]
                at.append(len(a.reqs))
                a.add(value(then if second else first), (x, y, z)[i % 3])
                j += 1
        a.pad_to(a.at(0, 16))
        return a.batch(), at

    (b0, at), (b1, _) = build(False), build(True)
    assert all((b0.offsets[f] == b1.offsets[f]).all() for f in range(5))
    s0, s1 = rs.shape(b0), rs.shape(b1)
    for sh in (s0, s1):
        below_dense(sh, "G")
        assert 0 < sh.per_slab[0] <= RESOLVE_SPARSE < sh.per_slab[1], sh.per_slab.tolist()
    return Case("G", rs, [("G first", b0), ("G second", b1)], dict(model_first=s0.summary(), model_second=s1.summary(), observed=at), turns=4)


# --- set H: confirm_entry itself ---
H_CONTAINS = {n: ("".join("bcdfghjklmnp"[(7 * n + 5 * i) % 12] if i % 3 else "0123456789"[(n + i) % 10] for i in range(n - 2)) + "%c%c" % (65 + n % 26, 97 + n % 26))[-n:] if n > 2 else "Y" + "y"
              for n in (2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65)}
H_LIT5, H_LIT20 = "/w5.p", "/edge-literal-20.php"
H_REGEX = "abc[0-9]efghijklmnopqrs[a-f]uv#Zq~Xj%Kv"  # (rare bigrams at its end: the filter's window, which ends the stored factor, lies behind byte 19)
H_FOLD = "CaseLess-Thirty-Bytes-Of-Text!"
I_LITS = [f"{chr(65 + j // 6)}{chr(107 + j % 6)}{j % 10}QZ" for j in range(40)]
assert len(H_LIT5) == 5 and len(H_LIT20) == 20 and len(H_FOLD) == 30 and all(len(v) == n for n, v in H_CONTAINS.items()) and len(set(I_LITS)) == 40


@functools.lru_cache(maxsize=None)
def set_h():
    f = "http_request.user_agent"
    preds = [H_CONTAINS[n] for n in sorted(H_CONTAINS)]
    for lit in (H_LIT5, H_LIT20):
        preds += [f"{f}.starts_with({H.q(lit)})", f"{f}.ends_with({H.q(lit)})", f"{f} == {H.q(lit)}"]
    preds += [f"{f}.matches({H.q(H_REGEX)})", f"{f}.matches({H.q('(?i)' + H_FOLD)})"]
    preds += I_LITS
    rs = RuleSet("H", "user_agent", preds)
    rs.k_contains = {n: k for k, n in enumerate(sorted(H_CONTAINS))}
    rs.k_lit = {H_LIT5: 13, H_LIT20: 16}
    rs.k_regex, rs.k_fold, rs.k_i = 19, 20, 21
    return rs


def flip(s, i):
    return s[:i] + (s[i].swapcase() if s[i].isalpha() else chr(ord(s[i]) ^ 1)) + s[i + 1:]


def wrong(s, i):
    return s[:i] + chr(ord(s[i]) ^ 1 if ord(s[i]) ^ 1 != ord(s[i].swapcase()) else ord(s[i]) ^ 2) + s[i + 1:]


@functools.lru_cache(maxsize=None)
def case_h():
    """H. confirm_entry on the device: `contains` literals of 2 .. 64 bytes (the second round of 16-byte loads, lengths that are no
    multiple of 4) and one of 65 (past confirm_literal's limit: a walk factor); starts_with / ends_with / == of a 5- and a 20-byte
    literal with the literal at the right end, the wrong end and both (kConfirmAtStart / kConfirmAtEnd); a regex whose factor has
    byte classes at its bytes 3 and 19 (text_byte's load); (?i) over 30 bytes with the case flipped at the first, 16th, 17th and
    last byte; near misses in the first byte, the last and byte 16; every value at every offset of a chunk."""
    rs = set_h()
    gi, g = rs.pass_of()
    cs = rs.confirm_shape()
    assert cs["longest"] >= 64 and cs["top_class_pos"] >= 16 and cs["has_walk"] == 1 and cs["in_lds"] == 1, cs
    # 64 bytes: a confirm literal; 65: not one (the pass keeps a DFA for it)
    n_lits = g["confirm_literals"]
    alone = RuleSet("H65", "user_agent", [H_CONTAINS[65]])
    assert alone.pass_of()[1]["confirm_literals"] == 0 and alone.confirm_shape()["has_walk"] == 1
    alone64 = RuleSet("H64", "user_agent", [H_CONTAINS[64]])
    assert alone64.pass_of()[1]["confirm_literals"] == 1 and alone64.confirm_shape()["has_walk"] == 0
    probes = []  # (value, key)
    for n, lit in H_CONTAINS.items():
        k = rs.k_contains[n]
        vals = ["<" + lit + ">", lit, "<" + wrong(lit, 0) + ">", "<" + wrong(lit, n - 1) + ">", "<" + lit[:-1], lit[1:] + ">"]
        if n > 16:
            vals += ["<" + wrong(lit, 16) + ">", "<" + wrong(lit, 15) + ">"]
        probes += [(v, k) for v in vals]
    for lit in (H_LIT5, H_LIT20):
        for form in range(3):  # starts_with, ends_with, ==
            k = rs.k_lit[lit] + form
            probes += [(v, k) for v in (lit + "-middle-", "-middle-" + lit, lit + "-middle-" + lit, lit, "x" + lit, lit + "x", wrong(lit, len(lit) - 1) + "-middle-" + wrong(lit, 0))]
    rx = H_REGEX.replace("[0-9]", "7").replace("[a-f]", "c")
    assert len(rx) == 31 and rx[3] == "7" and rx[19] == "c"
    probes += [(v, rs.k_regex) for v in ("<" + rx + ">", rx, "<" + rx[:3] + "x" + rx[4:] + ">", "<" + rx[:19] + "g" + rx[20:] + ">", "<" + rx[:19] + "9" + rx[20:] + ">",
                                        "<" + rx[:3] + "0" + rx[4:19] + "f" + rx[20:] + ">", "<" + wrong(rx, 30) + ">", "<" + wrong(rx, 0) + ">", "<" + wrong(rx, 16) + ">")]
    for i in (0, 15, 16, 29):
        probes += [("<" + flip(H_FOLD, i) + ">", rs.k_fold), ("<" + wrong(H_FOLD, i) + ">", rs.k_fold)]
    probes += [("<" + H_FOLD.upper() + ">", rs.k_fold), ("<" + H_FOLD.lower() + ">", rs.k_fold)]
    a = rs.arena()
    for o in range(16):
        for v, k in probes:
            a.pad_to(a.at(o, 16))
            a.add(v, k)
    a.pad_to(a.at(0, 16))
    batch = a.batch()
    sh = rs.shape(batch)
    below_dense(sh, "H")
    return Case("H", rs, [("H", batch)], dict(model=sh.summary(), confirm_shape=cs, confirm_literals=n_lits, probes=len(probes)))


@functools.lru_cache(maxsize=None)
def case_i():
    """I. a head word with many entries (`cnt = hd >> 20`): forty 5-byte literals that end in the same two bytes share the bin of their
    window's last bigram. Hits of the first, the last, several at once, and none."""
    rs = set_h()
    cs = rs.confirm_shape()
    assert cs["widest_bin"] >= 32, cs
    a = rs.arena()
    k0 = rs.k_i
    for o in (0, 5, 11, 12, 15):
        for j in (0, 1, 19, 38, 39):
            for v in ("<" + I_LITS[j] + ">", I_LITS[j], "<" + wrong(I_LITS[j], 0) + ">", "<" + I_LITS[j][:4] + "Y>", "<xx" + I_LITS[j][2:] + ">"):
                a.pad_to(a.at(o, 16))
                a.add(v, k0 + (j if len(a.reqs) % 3 else (j + 1) % 40))
        a.pad_to(a.at(o, 16))
        a.add("".join(I_LITS[j] + "," for j in (0, 7, 39)), k0 + 7)
        a.pad_to(a.at(o, 16))
        a.add("".join(I_LITS), k0 + 20)  # every one of them (in the hit matrix: forty atoms of one request, an overflow chain)
        a.pad_to(a.at(o, 16))
        a.add("..QZ..xxQZ", k0)
    batch = a.batch()
    sh = rs.shape(batch)
    below_dense(sh, "I")
    return Case("I", rs, [("I", batch)], dict(model=sh.summary(), confirm_shape=cs))


# --- set A: comparison tables too large for LDS ---
A_SEED, A_RULES = 20240607, 4000


@functools.lru_cache(maxsize=None)
def set_a():
    rng = random.Random(A_SEED)
    alpha = "abcdefghijklmnop"  # (sixteen letters: the 4 000 literals still share one DFA, so one pass)
    lits = []
    while len(lits) < A_RULES:
        lit = "".join(rng.choice(alpha) for _ in range(rng.randint(8, 12)))
        if not any(lit in x or x in lit for x in lits[-50:]):
            lits.append(lit)
    rs = RuleSet("A", "url", lits, verdict_form=False)  # (bare rules: a request holds at most one literal, the deciding rule names it)
    rs.lits = lits
    return rs


@functools.lru_cache(maxsize=None)
def case_a():
    """A. comparison tables read from global memory (confirm_entry<1> on the L2 copies): 4 000 `url.contains(<8 - 12 bytes>)` rules are
    one filtered pass whose entries alone exceed the LDS pool. About 2 000 requests: hits, misses in the last byte, literals cut by
    one byte, at every offset of a chunk."""
    rs = set_a()
    cs = rs.confirm_shape()
    assert cs["in_lds"] == 0 and cs["entries"] >= 3414 and cs["entries"] * 3 + cs["bytes"] // 4 + cs["class_words"] > POOL_WORDS, cs
    assert rs.pass_of()[1]["confirm_literals"] == A_RULES
    rng = random.Random(A_SEED + 1)
    a = Arena("url", [0])
    a.filler_head, a.filler_byte = "/", "/"
    for i in range(680):
        lit = rs.lits[rng.randrange(A_RULES)] if i % 4 else rs.lits[(0, A_RULES - 1)[i % 8 == 0]]
        for v in ("/p?" + lit + "&z", "/p?" + wrong(lit, len(lit) - 1) + "&z", "/p?" + lit[:-1]):
            a.pad_to(a.at(i % 16, 16), piece=40)
            a.add(v)
    batch = a.batch()
    sh = rs.shape(batch)
    below_dense(sh, "A")
    assert sh.pairs >= 680
    return Case("A", rs, [("A", batch)], dict(model=sh.summary(), confirm_shape=cs, n=batch.n))


# --- set J: the walk queue ---
J_REGEX = "tok=[0-9a-f]+;"


@functools.lru_cache(maxsize=None)
def set_j():
    rs = RuleSet("J", "url", [f"http_request.url.matches({H.q(J_REGEX)})"], verdict_form=False)
    assert rs.confirm_shape()["has_walk"] == 1
    return rs


def case_j(n_cus=MI355X_CUS):
    """J. the walk queue running full (`slot < kConfirmQueue` else the direct append): a regex rule whose factor is confirmed for every
    request; a base batch of four 48-byte requests (one flagged chunk of three each) tiled to the smallest n with more than
    2 * 1024 * blocks pairs, blocks = 2 * compute units (launch_confirm's grid): every workgroup then meets more than 1 024 distinct
    walk requests in one run of the pass. -> (case of the base batch, times to tile it)"""
    rs = set_j()
    vals = ["/item/view?q=1&tok=0123456789abcdef;&pad=......", "/item/view?q=2&tok=9876543210ffffff&pad=.......", "/item/view?q=3&tok=fedcba9876543210;&pad=......",
            "/item/view?q=4&tok=0123456789abcdeg;&pad=......"]
    vals = [v[:48].ljust(48, ".") for v in vals]
    assert all(len(v) == 48 for v in vals)
    base = RequestBatch.from_requests([Request(host="h", path="/i", url=v, user_agent="ua") for v in vals])
    blocks = 2 * n_cus
    times = 2 * CONFIRM_THREADS * blocks // len(vals) + 1
    gi, g = rs.pass_of()
    # the model on a few tiles: the arena is periodic (48 bytes a request, 16-byte chunks, 4 KiB of warm-up at most)
    few = base.tile(400)
    sh = rs.shape(few)
    per_request = [len(sh.chunks_of(r)) for r in range(8, few.n - 8)]
    assert set(per_request) == {1}, set(per_request)  # one flagged chunk per request: every pair is another request, so 2 048 consecutive pairs hold 2 048 distinct ones (> QUEUE)
    assert sh.pairs * 2 <= (sh.total + 15) // 16, "above the flag-density switch"
    pairs = times * len(vals)
    assert pairs > 2 * QUEUE * blocks and (times - 1) * len(vals) <= 2 * QUEUE * blocks
    for r in range(8, 12):  # the factor is CONFIRMED for every request (the host's form of the same code): each is a walk request
        atoms, flagged, walk = rs.program()[0].confirm_field(gi, few.field_bytes(1, r), int(few.offsets[1][r]) % 16)
        assert flagged and walk, r
    return Case("J", rs, [("J base", base)], dict(model_400_tiles=sh.summary(), blocks=blocks, times=times, pairs=pairs, confirm_shape=rs.confirm_shape())), times


CASES = {"A": case_a, "B": case_b, "C": case_c, "C2": case_c2, "D": case_d, "E": case_e, "F": case_f, "G": case_g, "H": case_h, "I": case_i}
