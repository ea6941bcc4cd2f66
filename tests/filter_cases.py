"""Shared builders of the filter edge suites (tests/test_filter_edges_cpu.py, tests/test_gpu_filter_edges.py); no GPU import.

Under test: filter_kernel's chunk bitmap, per-slab counts and pair-list bookkeeping (csrc/filter.hip, filter_rows), read back through
the hook pwaf_engine_filter_flags and compared bit for bit with confirm_cases.window_positions, the numpy restatement of the shift-or
automaton over a whole arena. The kernel cuts the stream at seams the automaton knows nothing of -- lanes (16 bytes), rows (1 KiB),
iterations (4 KiB), slabs (128 KiB, one wave each), workgroups (4 slabs), the two strides' workgroups interleaved in one launch -- and
hands the state across each of them in another way. Here:

  * byte_behind: the ONE respect in which the kernel is not the automaton over the arena's bytes -- what the stream's last position is
    paired with -- and device_chunks, the model with that byte: what the hook must return.
  * Fields: a batch whose host, url, path and user_agent arenas are filled independently, values placed at chosen bytes.
  * set F (a filtered pass with a confirm tier on each of the four fields, strides 2, 1, 2, 2), set Sb (confirm_cases' set S as bare
    rules), and confirm_cases.set_a.
  * the cases A to E, each asserting its shape with the model before a device is involved."""
import collections
import functools
import random

import numpy as np

import confirm_cases as CC
import helpers as H
from pingoo_amd import RequestBatch, _abi

CHUNK, SLAB = CC.CHUNK, CC.SLAB
ROW, ITER, WAVES = 1024, 4096, 4  # csrc/kernels.h: a row of 64 lanes x 16 bytes, kStreamIter, kFilterWaves
SLAB_CHUNKS = SLAB // CHUNK
FIELDS = ("host", "url", "path", "user_agent")
FID = {f: _abi.FIELD_NAMES.index(f) for f in FIELDS}
NO_CONFIRM = _abi.OPT_NO_CONFIRM
FILL = b"q"


# ---------------------------------------------------------------------------------------------------------
# the model, extended by the byte behind the stream
# ---------------------------------------------------------------------------------------------------------
BEHIND_AFTER, BEHIND_BYTE0, BEHIND_BYTE0_SLACK = "after", "byte 0", "byte 0, behind slack"


def byte_behind(data, total):
    """What filter_rows pairs the stream's last position with at stride 1 (read from the code): the position is byte n - 1, the last of
    the arena's last chunk (n = total rounded up to whole chunks), and its second byte is the first of the NEXT lane's chunk, which no
    arena byte is.
      BEHIND_AFTER        n % 4096 == 0: the last chunk is lane 63 of row 3 of the slab's last iteration, whose next dword is `after`,
                          the constant 0 for the arena's last slab.
      BEHIND_BYTE0        otherwise, total % 16 == 0: the next lane (lane 0 of the next row behind lane 63) starts at or beyond `total`
                          and load_row clamps its address to ARENA BYTE 0: the arena's last byte is paired with its first.
      BEHIND_BYTE0_SLACK  otherwise: the same load, but byte n - 1 is slack (zero) behind `total`; the arena's last byte is paired
                          with the slack byte behind it, as in the model as it stood.
    Stride 2 never looks across a dword. No factor's window can need this bigram (a window that ends in the arena's last byte ends
    one bigram earlier), so a chunk flagged by it only costs a comparison: the behaviour is pinned, not a bug. -> (case, byte)"""
    n = (int(total) + CHUNK - 1) // CHUNK * CHUNK
    if n % ITER == 0:
        return BEHIND_AFTER, 0
    return (BEHIND_BYTE0 if total % CHUNK == 0 else BEHIND_BYTE0_SLACK), int(data[0])


def slabs_of(total):
    return (int(total) + SLAB - 1) // SLAB


def device_chunks(g, data, total, extended=True):
    """-> bool per chunk of the arena's every slab, slab 0 first: what filter_kernel's bitmap must hold, zero behind the end.
    extended=False: the model without byte_behind (what the cases prove their shapes with)."""
    out = np.zeros(slabs_of(total) * SLAB_CHUNKS, dtype=bool)
    if total:
        w = CC.window_positions(g, data, total, byte_behind(data, total)[1] if extended else None)
        out[:len(w) // CHUNK] = w.reshape(-1, CHUNK).any(axis=1)
    return out


def expected(rs, flags, batch):
    """-> {field: (pass index, dump entry, slab0, bool per chunk of the slabs the pass streams)} for every filtered pass of the rule set
    under `flags`. A slab view (offsets[0] != 0) shares its arenas with the batch it was cut from: the model runs over the WHOLE
    arena from byte 0 (positions are absolute) and the slabs in front of offsets[0] are left out."""
    out = {}
    for field, (gi, g) in passes(rs, flags).items():
        off = batch.offsets[FID[field]]
        total = int(off[-1])
        slab0 = int(off[0]) // SLAB if total else 0
        out[field] = (gi, g, slab0, device_chunks(g, batch.data[FID[field]], total)[slab0 * SLAB_CHUNKS:])
    return out


def describe_chunk(c, slab0=0):
    """chunk c of the streamed slabs as filter_rows sees it: (slab, iteration, row, lane)"""
    return (slab0 + c // SLAB_CHUNKS, c % SLAB_CHUNKS // 256, c % 256 // 64, c % 64)


# ---------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------
class Fields:
    """A batch whose four string fields are arenas of their own: value i of every field is request i's, a field with fewer values than
    another ends in empty ones. Fillers are runs of 'q'."""

    def __init__(self):
        self.vals = {f: [] for f in FIELDS}
        self.cur = dict.fromkeys(FIELDS, 0)

    def add(self, field, value):
        value = value.encode() if isinstance(value, str) else bytes(value)
        self.vals[field].append(value)
        self.cur[field] += len(value)
        return len(self.vals[field]) - 1

    def pad_to(self, field, pos, piece=3000):
        assert pos >= self.cur[field], (field, pos, self.cur[field])
        while self.cur[field] < pos:
            self.add(field, FILL * min(piece, pos - self.cur[field]))

    def plant(self, field, pos, value):
        """`value` in a request of its own, its first byte at arena byte `pos`"""
        self.pad_to(field, pos)
        return self.add(field, value)

    def batch(self):
        n = max(1, max(len(v) for v in self.vals.values()))
        datas, offs = [], []
        for name in _abi.FIELD_NAMES:
            vals = self.vals.get(name, [])
            o = np.zeros(n + 1, dtype=np.uint32)
            o[1:len(vals) + 1] = np.cumsum([len(v) for v in vals], dtype=np.uint64).astype(np.uint32)
            o[len(vals) + 1:] = o[len(vals)]
            datas.append(np.frombuffer(b"".join(vals) + b"\0" * _abi.ARENA_PAD, dtype=np.uint8).copy())
            offs.append(o)
        return RequestBatch(datas, offs, np.zeros((n, 16), dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.full(n, 4711, dtype=np.uint16), np.zeros(n, dtype=np.uint8))


class Sent:
    """One batch a case sends: `before` (or None) is evaluated on the same engine first, unchecked; `verdicts`: the oracle's are compared too."""

    def __init__(self, label, batch, before=None, verdicts=False):
        self.label, self.batch, self.before, self.verdicts = label, batch, before, verdicts


class Case:
    def __init__(self, name, legs, sent, measured):
        """legs: [(rule set, flags)] every batch is sent through"""
        self.name, self.legs, self.sent, self.measured = name, legs, sent, measured


def passes(rs, flags=0):
    """{field: (pass index, dump entry)} of the rule set's filtered passes, at most one per field"""
    out = {}
    for gi, g in enumerate(rs.program(flags)[1].groups):
        if "f_table" in g:
            name = _abi.FIELD_NAMES[g["field"]]
            assert name in FIELDS and name not in out, (rs.name, name)
            out[name] = (gi, g)
    return out


def flagged(g, batch, field):
    """the flagged chunks of the field's arena by the model as the cases prove their shapes with it (no byte behind the stream)"""
    return np.nonzero(device_chunks(g, batch.data[FID[field]], int(batch.offsets[FID[field]][-1]), extended=False))[0]


# ---------------------------------------------------------------------------------------------------------
# rule sets
# ---------------------------------------------------------------------------------------------------------
F_LITS = {"host": ["evil.example"], "url": ["kw#7x", "zq"], "path": ["/etc/passwd", "wp-config.php"], "user_agent": ["sqlmap/1.7"]}
F_STRIDES = {"host": 2, "url": 1, "path": 2, "user_agent": 2}


def completes_at(g, lit, p):
    """the ONE arena position at which `lit`, planted at byte p of a filler, completes a window: the first byte of the window's last bigram"""
    pre = 64 + p % 2
    a = np.frombuffer(FILL * pre + lit.encode() + FILL * 64 + b"\0" * 16, dtype=np.uint8)
    at = np.nonzero(CC.window_positions(g, a, len(a) - 16))[0]
    assert len(at) == 1, (lit, p, at)
    return p + int(at[0]) - pre


@functools.lru_cache(maxsize=None)
def set_f():
    """F: literals on all four fields, as built one filtered pass with a confirm tier and no heads per field; under PWAF_OPT_NO_CONFIRM
    the same passes without a pair list. Bare rules: the first literal a request holds decides its verdict."""
    rs = CC.RuleSet("F", "url", [f"http_request.{f}.contains({H.q(lit)})" for f in ("url", "host", "path", "user_agent") for lit in F_LITS[f]], verdict_form=False)
    for flags in (0, NO_CONFIRM):
        ps = passes(rs, flags)
        assert {f: g["f_stride"] for f, (_, g) in ps.items()} == F_STRIDES, (flags, {f: g["f_stride"] for f, (_, g) in ps.items()})
        assert all(g.get("confirm", 0) == (0 if flags else 1) and len(g["f_heads"]) == 0 for _, g in ps.values()), flags
    fb = Fields()
    for f in FIELDS:
        for size in (1, 15, 16, 17, 200, 3000, 3000, 5000):
            fb.add(f, FILL * size)
    filler = fb.batch()
    for f, (_, g) in passes(rs).items():
        assert len(flagged(g, filler, f)) == 0, f"fillers flag a chunk of the {f} arena"
        for lit in F_LITS[f]:
            for p in (100, 101):
                c = completes_at(g, lit, p)
                # stride 1: the window ends with the literal, its last bigram is the literal's last two bytes. Stride 2: four sampled
                # bigrams are eight bytes, the factor lies somewhere inside a longer literal; its last bigram starts at an even arena byte
                assert c == p + len(lit) - 2 if g["f_stride"] == 1 else (c % 2 == 0 and p + 6 <= c <= p + len(lit) - 2), (f, lit, p, c)
    return rs


@functools.lru_cache(maxsize=None)
def set_sb():
    """confirm_cases' set S as bare rules: only the url is read"""
    rs = CC.RuleSet("Sb", "url", CC.S_LITS + [f"http_request.url.matches({H.q(CC.S_REGEX)})"], verdict_form=False)
    assert passes(rs)["url"][1]["f_stride"] == 1
    return rs


# ---------------------------------------------------------------------------------------------------------
# A. splits: the pass's literal across every seam, at every displacement
# ---------------------------------------------------------------------------------------------------------
SEAM_KINDS = ("lane", "row", "iteration", "slab", "workgroup")
A_SLAB_SEAMS = (1, 2, 3, 4, 5)  # k of the seam at k * SLAB: k % 4 != 0 a slab seam, k == 4 the workgroup seam


def displacements(lit):
    """first byte of the plant relative to the seam: from "the literal ends three bytes before the seam" (its window is complete two
    bytes before it at the latest) to "the literal begins two bytes behind it", every byte"""
    return list(range(-2 - len(lit), 3))


def a_in_slab_seams(m):
    """the three seams inside block m of 4 KiB (m >= 1, m % 32 != 0): its first byte, an iteration seam; a row seam; a lane seam in mid-row"""
    assert m % 32
    row = 1 + m % 3
    lane_row = (row + 1) % 4  # (lanes 8 .. 55 of another row: no other plant within a hundred bytes)
    return [("iteration", ITER * m), ("row", ITER * m + ROW * row), ("lane", ITER * m + ROW * lane_row + CHUNK * (8 + 7 * m % 48))]


A_BATCHES = max(len(displacements(lit)) for lits in F_LITS.values() for lit in lits)


@functools.lru_cache(maxsize=None)
def case_a():
    rs = set_f()
    ps = passes(rs)
    sent, crossing, per_batch = [], collections.Counter(), []
    seen = collections.defaultdict(set)  # (field, literal, kind) -> displacements planted
    for j in range(A_BATCHES):
        fb, want = Fields(), {}
        for fi, f in enumerate(FIELDS):
            g = ps[f][1]
            plan = []  # (position, literal, kind, seam)
            blocks = (m for m in range(1, 200) if m % 32)
            for lit in F_LITS[f]:
                disp = displacements(lit)
                for i in range(len(disp)):
                    for kind, seam in a_in_slab_seams(next(blocks)):
                        plan.append((seam + disp[(i + j) % len(disp)], lit, kind, seam))
            for k in A_SLAB_SEAMS:
                lit = F_LITS[f][k % len(F_LITS[f])]
                disp = displacements(lit)
                plan.append((k * SLAB + disp[(j + 3 * k) % len(disp)], lit, "workgroup" if k % WAVES == 0 else "slab", k * SLAB))
            chunks = set()
            for p, lit, kind, seam in sorted(plan):
                fb.plant(f, p, lit)
                c = completes_at(g, lit, p)
                chunks.add(c // CHUNK)
                seen[f, lit, kind].add(p - seam)
                if p < seam <= c - c % CHUNK:  # begins before the seam, completes in the chunk behind it
                    crossing[kind, g["f_stride"]] += 1
            assert len(chunks) == len(plan)
            fb.pad_to(f, max(A_SLAB_SEAMS) * SLAB + 2 * ITER + 100 * fi + 7)
            want[f] = chunks
        batch = fb.batch()
        for f in FIELDS:
            got = set(flagged(ps[f][1], batch, f).tolist())
            assert got == want[f], (j, f, "flagged by the model but no plant's chunk:", sorted(got - want[f]), "a plant's chunk not flagged:", sorted(want[f] - got))
            assert slabs_of(batch.offsets[FID[f]][-1]) == 6
        per_batch.append({f: len(want[f]) for f in FIELDS})
        sent.append(Sent(f"A batch {j}", batch, verdicts=True))
    for (f, lit, kind), ds in seen.items():
        assert ds == set(displacements(lit)), (f, lit, kind, "displacements not planted:", sorted(set(displacements(lit)) - ds))
    assert {k for k, _ in crossing} == set(SEAM_KINDS) and {s for _, s in crossing} == {1, 2} and len(crossing) == 10, crossing
    return Case("A", [(rs, 0), (rs, NO_CONFIRM)], sent, dict(batches=A_BATCHES, slabs=6, plants_per_batch=per_batch[0], crossing={f"{k}, stride {s}": n for (k, s), n in sorted(crossing.items())}))


# ---------------------------------------------------------------------------------------------------------
# B. ends: the arena's last chunk, behind a longer batch that flagged every row
# ---------------------------------------------------------------------------------------------------------
B_TOTALS = (1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 131071, 131072, 131073, 131072 + 4096, 4 * 131072, 4 * 131072 + 1)
B_DIRTY_SLABS = 6


@functools.lru_cache(maxsize=None)
def dirty_batch():
    """six slabs per field, a literal every 1 024 bytes: a flagged chunk in every row of every slab, by the model"""
    rs = set_f()
    fb = Fields()
    for f in FIELDS:
        for r in range(B_DIRTY_SLABS * SLAB // ROW):
            fb.plant(f, r * ROW + 500 + r % 2, F_LITS[f][0])
        fb.pad_to(f, B_DIRTY_SLABS * SLAB)
    batch = fb.batch()
    for f, (_, g) in passes(rs).items():
        rows = device_chunks(g, batch.data[FID[f]], B_DIRTY_SLABS * SLAB).reshape(-1, 64)
        assert len(rows) == B_DIRTY_SLABS * SLAB // ROW and rows.any(axis=1).all(), f
    return batch


def b_end_batch(rs, total, back):
    """every field's arena ends at `total`; the pass's literal, cut behind its window's last bigram, ends `back` bytes before it (back =
    1: in the arena's last byte) where it fits -- at stride 2 one byte earlier where that bigram would start at an odd byte"""
    fb, plants = Fields(), {}
    for f in FIELDS:
        g, lit = passes(rs)[f][1], F_LITS[f][0]
        for shift in (0, 1):
            c = total - back - 1 - shift  # where the window is to complete
            fits = [p for p in range(max(0, c - len(lit)), c + 1) if completes_at(g, lit, p) == c]
            if fits:
                fb.plant(f, fits[0], lit[:c + 2 - fits[0]])
                plants[f] = c
                break
        fb.pad_to(f, total)
    batch = fb.batch()
    for f, (_, g) in passes(rs).items():
        assert int(batch.offsets[FID[f]][-1]) == total
        got = flagged(g, batch, f).tolist()
        assert got == ([plants[f] // CHUNK] if f in plants else []), (total, back, f, got)
        assert f in plants or total < 15, (total, back, f)
    return batch, plants


def b_visible(total):
    """the url arena begins with 'q' and ends with 'z': paired, they are the literal "zq" """
    fb = Fields()
    fb.pad_to("url", total - 1)
    fb.add("url", b"z")
    for f in ("host", "path", "user_agent"):
        fb.add(f, b"h")
    return fb.batch()


@functools.lru_cache(maxsize=None)
def case_b():
    rs = set_f()
    g_url = passes(rs)["url"][1]
    sent, in_last, cases = [], 0, collections.Counter()
    for total in B_TOTALS:
        for back in (1, 2):
            batch, plants = b_end_batch(rs, total, back)
            in_last += sum(1 for c in plants.values() if c // CHUNK == (total - 1) // CHUNK)
            cases[byte_behind(batch.data[FID["url"]], total)[0]] += 1
            sent.append(Sent(f"B total {total}, literal ends {back} before", batch, before=dirty_batch(), verdicts=True))
    assert set(cases) == {BEHIND_AFTER, BEHIND_BYTE0, BEHIND_BYTE0_SLACK}, cases
    # the pinned choice made visible: total % 16 == 0 and the arena's byte 0 completes a window behind its last byte ...
    visible = {}
    for total, case in ((ROW + CHUNK, BEHIND_BYTE0), (ITER, BEHIND_AFTER), (ROW + CHUNK + 1, BEHIND_BYTE0_SLACK)):
        batch = b_visible(total)
        data = batch.data[FID["url"]]
        assert byte_behind(data, total) == (case, 0 if case == BEHIND_AFTER else ord("q"))
        plain, ext = device_chunks(g_url, data, total, extended=False), device_chunks(g_url, data, total)
        assert not plain.any(), total
        visible[case] = np.nonzero(ext)[0].tolist()
        sent.append(Sent(f"B byte behind: {case}, total {total}", batch, before=dirty_batch(), verdicts=True))
    # ... in that case alone
    assert visible == {BEHIND_BYTE0: [(ROW + CHUNK - 1) // CHUNK], BEHIND_AFTER: [], BEHIND_BYTE0_SLACK: []}, visible
    return Case("B", [(rs, 0), (rs, NO_CONFIRM)], sent, dict(totals=list(B_TOTALS), plants_completing_in_the_last_chunk=in_last, behind_cases=dict(cases), visible=visible))


# ---------------------------------------------------------------------------------------------------------
# C. mix: the fused launch with unequal classes
# ---------------------------------------------------------------------------------------------------------
C_SLABS = ((1, 9, 5, 2), (6, 1, 6, 6), (3, 3, 3, 3), (0, 5, 0, 0), (2, 0, 3, 1))  # (host, url, path, user_agent)
C_LAST = (SLAB, 70001, ITER + CHUNK + 1, 33000)  # bytes of a field's last slab, in turn


@functools.lru_cache(maxsize=None)
def case_c():
    rs = set_f()
    ps = passes(rs)
    sent, measured = [], []
    for ci, counts in enumerate(C_SLABS):
        fb = Fields()
        for fi, (f, count) in enumerate(zip(FIELDS, counts)):
            if count == 0:
                fb.add(f, b"")
                continue
            last = C_LAST[(fi + ci) % len(C_LAST)]
            for s in range(count):
                size = SLAB if s < count - 1 else last
                rows = (size - 600) // ROW
                for r in sorted(random.Random(7919 * fi + 31 * s + 1).sample(range(rows), min(5, rows))):
                    fb.plant(f, s * SLAB + r * ROW + 500 + (r + s) % 2, F_LITS[f][(r + s) % len(F_LITS[f])])
            fb.pad_to(f, (count - 1) * SLAB + last)
        batch = fb.batch()
        maps = []
        for f, count in zip(FIELDS, counts):
            total = int(batch.offsets[FID[f]][-1])
            assert slabs_of(total) == count, (ci, f, total)
            maps += [m.tobytes() for m in device_chunks(ps[f][1], batch.data[FID[f]], total).reshape(-1, SLAB_CHUNKS)]
        assert len(maps) == sum(counts) == len(set(maps)), (ci, "two slabs of the batch have the same bitmap")
        measured.append(dict(slabs=counts, flagged={f: int(device_chunks(ps[f][1], batch.data[FID[f]], int(batch.offsets[FID[f]][-1])).sum()) for f in FIELDS}))
        sent.append(Sent(f"C slabs {counts}", batch, verdicts=True))
    return Case("C", [(rs, 0), (rs, NO_CONFIRM)], sent, dict(batches=measured))


# ---------------------------------------------------------------------------------------------------------
# D. bytes: random arenas
# ---------------------------------------------------------------------------------------------------------
D_TOTAL = 3 * SLAB - 7
D_ARENAS = {"lowercase": (97, 123), "printable": (32, 127), "all 256 values": (0, 256)}
D_SEED = 20240919


def d_arena(kind):
    """three slabs of the url arena: a few short fields, one long one, a few short ones"""
    lo, hi = D_ARENAS[kind]
    rng = np.random.default_rng(D_SEED + lo)
    body = rng.integers(lo, hi, size=D_TOTAL, dtype=np.uint8).tobytes()
    cuts = [0, 7, 40, 41, 41, 300, D_TOTAL - 500, D_TOTAL - 480, D_TOTAL - 3, D_TOTAL]
    fb = Fields()
    for a, b in zip(cuts, cuts[1:]):
        fb.add("url", body[a:b])
    return fb.batch()


@functools.lru_cache(maxsize=None)
def case_d(which):
    """which: (arena kind, rule set name, flags)"""
    kind, set_name, flags = which
    rs = {"A": CC.set_a, "Sb": set_sb}[set_name]()
    batch = d_arena(kind)
    gi, g = passes(rs, flags)["url"]  # (the program's path pass, which every program has, streams nothing: the arena's other fields are empty)
    n = int(device_chunks(g, batch.data[FID["url"]], D_TOTAL).sum())
    chunks = (D_TOTAL + CHUNK - 1) // CHUNK
    assert chunks == 3 * SLAB_CHUNKS and 100 <= n <= chunks * 6 // 10, (which, n, chunks)
    return Case(f"D {kind}, set {set_name}, stride {g['f_stride']}", [(rs, flags)], [Sent(f"D {kind}", batch)], dict(stride=g["f_stride"], chunks=chunks, flagged=n, share=round(100.0 * n / chunks, 2)))


D_LEGS = [("lowercase", "A", 0), ("lowercase", "A", _abi.OPT_FILTER_STRIDE2), ("printable", "A", 0), ("printable", "A", _abi.OPT_FILTER_STRIDE2), ("all 256 values", "Sb", 0)]


# ---------------------------------------------------------------------------------------------------------
# E. view: a slab view that begins inside slab 2
# ---------------------------------------------------------------------------------------------------------
E_BEGIN = {"host": 40, "url": 2 * SLAB + 5000, "path": 2 * SLAB + 7001, "user_agent": 33}  # offsets[0] of the view
E_END = {"host": 900, "url": 4 * SLAB + 70003, "path": 4 * SLAB + 50000, "user_agent": 777}


@functools.lru_cache(maxsize=None)
def case_e():
    """-> the case; its one Sent is the view, `before` the whole batch: both travel column by column through the same staging buffers
    (the view for being one, the whole batch for its size), so the bytes in front of the view's first request, which the view does not
    send, are the whole batch's on the device too"""
    rs = set_f()
    ps = passes(rs)
    fb, plants = Fields(), {}
    for f in FIELDS:
        lit = F_LITS[f][0]
        if f in ("url", "path"):
            plants[f] = [SLAB + 999, 2 * SLAB - len(lit) // 2,  # ... one straddles the first streamed slab's first byte,
                         2 * SLAB + 2048 + 17]                   # one lies wholly in the bytes in front of offsets[0]
            for p in plants[f]:
                fb.plant(f, p, lit)
        fb.pad_to(f, E_BEGIN[f], piece=1500)
    k = max(len(v) for v in fb.vals.values())  # the view's first request: every field's values in front of it end at E_BEGIN
    for f in FIELDS:
        while len(fb.vals[f]) < k:
            fb.add(f, b"")
    for f in FIELDS:
        lit = F_LITS[f][0]
        for p in ([E_BEGIN[f] + 3, 3 * SLAB - 5, 4 * SLAB + 4096 - 3] if f in ("url", "path") else [E_BEGIN[f] + 20]):
            fb.plant(f, p, lit)
            plants.setdefault(f, []).append(p)
        fb.pad_to(f, E_END[f])
    whole = fb.batch()
    view = whole.view(k, whole.n)
    assert sum(int(whole.offsets[FID[f]][-1]) for f in FIELDS) > 1 << 20, "the whole batch is small enough to travel as one packed block"
    measured = {}
    for f, (gi, g) in ps.items():
        assert int(view.offsets[FID[f]][0]) == E_BEGIN[f] and int(view.offsets[FID[f]][-1]) == E_END[f], f
        got = flagged(g, whole, f).tolist()
        assert got == sorted(completes_at(g, F_LITS[f][0], p) // CHUNK for p in plants[f]), (f, got)
        measured[f] = dict(slab0=E_BEGIN[f] // SLAB, slabs=slabs_of(E_END[f]) - E_BEGIN[f] // SLAB, flagged_chunks=got)
    for f in ("url", "path"):
        _, g, slab0, want = expected(rs, 0, view)[f]
        assert slab0 == 2 and len(want) == 3 * SLAB_CHUNKS
        c = np.nonzero(want)[0].tolist()
        assert c[0] == 0 and plants[f][1] < 2 * SLAB, (f, c)                         # the straddling plant completes in the first streamed chunk
        assert (c[1] + 1) * CHUNK + 2 * SLAB <= E_BEGIN[f], (f, c)                    # a flagged chunk that no request of the view owns
        assert len(c) == 5
    return Case("E", [(rs, 0), (rs, NO_CONFIRM)], [Sent("E view", view, before=whole, verdicts=True)], dict(first_request=k, passes=measured))


CASES = {"A": case_a, "B": case_b, "C": case_c, "E": case_e}
