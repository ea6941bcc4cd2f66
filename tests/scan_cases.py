"""Shared builders of the streaming-scan edge suites (tests/test_scan_edges_cpu.py, tests/test_gpu_scan_edges.py); no GPU import.

scan_kernel<CH, WIDE> (csrc/scan.hip: scan_body) walks a DFA over EVERY request of a pass: every pass of a PWAF_OPT_NO_PREFILTER
engine, every pass without a usable prefilter. A wave takes a contiguous share of the batch in blocks of 64 offsets, a lane pulls the
next request while it is on its last 16 * CH bytes, steps run in speculative groups of four over hot rows in LDS, and a lane that meets
a cold row parks on the sentinel row. Here:

  * the tables and the plan come from tests/plan_harness.py over tests/scanplan_host.cpp: the host build of the build_device_group,
    plan_passes and tune_host the engine runs (sections SSHP, STAB, SCLS, SSPC, SLOF, SLST, LROL, LOWN, UFLT). Nothing is assumed about
    what the compiler or the table builder choose: every builder asserts the property it was written for.
  * StreamModel reads one field byte by byte off the streaming table (scan_walkers.ScanWalker) and says which ROW the kernel stands on
    after every byte and of which tier it is -- plain hot (cell < emit_base), emitting hot (< special_base), cold (a special cell: the
    lane parks) -- next to the raw DFA's walk (scan_walkers.RawWalker) of the same bytes.
  * shares() restates launch_scan's grid and scan_body's split of a batch into per-wave shares.
  * field strings are found by breadth-first search over the streaming table, as tests/lscan_cases.py does over the flat one.

The EXPECTED verdicts never come from the model: pyoracle.Oracle gives them, as everywhere else."""
import functools
import hashlib
import pathlib
import random
import tempfile

import numpy as np

import helpers as H
import test_scanplan_cpu as SP
from scan_walkers import RawWalker, ScanWalker, raw_of
from table_walker import cont_covered, parse_dump, scalar_class
from pingoo_amd import Request, RequestBatch, _abi

B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
NP, HITS = _abi.OPT_NO_PREFILTER, _abi.OPT_RULE_HITS
PLAIN, EMIT, COLD = "plain hot", "emitting hot", "cold"
KINDS = (PLAIN, EMIT, COLD)
# what the cases rest on (csrc/scan.hip: launch_scan, scan_body; csrc/scanplan.cpp: tune_host)
WAVES_PER_WG, MIN_PER_WAVE, OFFSET_BLOCK, CH2_MEAN, CH4_MEAN = 16, 256, 64, 48, 80
MI355X_CUS = 256  # (the CPU suite builds the tiled batch's shape for this device; the device suite for the one it runs on)
FIELD_NAMES = ("host", "url", "path", "method", "user_agent")
URL = 1
HEADER = "x-a"
PAD = _abi.ARENA_PAD
FILL = ord("~")  # (no pattern of the suites holds it)


def shares(n, n_cus=MI355X_CUS):
    """launch_scan and scan_body restated as data: -> (workgroups, requests per wave, [(w0, w1)] of the waves that have a share)"""
    blocks = max(1, min(((n + MIN_PER_WAVE - 1) // MIN_PER_WAVE + WAVES_PER_WG - 1) // WAVES_PER_WG, max(1, n_cus)))
    total = blocks * WAVES_PER_WG
    per = (n + total - 1) // total
    out = []
    for gw in range(total):
        w0 = min(n, gw * per)
        w1 = min(n, w0 + per)
        if w0 < w1:
            out.append((w0, w1))
    return blocks, per, out


# ---------------------------------------------------------------------------------------------------------
# the harness
# ---------------------------------------------------------------------------------------------------------
_TMP = None


def harness(rules, flags=0, budget=0, sample=None, table_bytes=0):
    """one run of tests/scanplan_host over (rules, flags, lds_table_budget, max_table_bytes, tuning sample) -> test_scanplan_cpu.Scan"""
    global _TMP
    if _TMP is None:
        _TMP = tempfile.TemporaryDirectory(prefix="scan_cases")
    case = dict(rules=rules, flags=flags, opts=(budget, 0, table_bytes))
    if sample is not None:
        case["sample"] = sample
    return SP.run_one(pathlib.Path(_TMP.name), **case)


def sample_columns(batch, header_names):
    """a RequestBatch as the harness's tuning sample: the five fields, then the program's header columns"""
    cols = [[batch.field_bytes(f, i) for i in range(batch.n)] for f in range(5)]
    cols += [[batch.header_bytes(h, i) for i in range(batch.n)] for h in header_names]
    return cols


class StreamModel:
    """The streaming table of one pass as the harness dumps it (kernels.h: the cell encoding), walked next to the raw DFA."""

    def __init__(self, sc, k):
        self.k, self.g, self.m = k, sc.groups[k], sc.scan_image(k)
        m, g = self.m, self.g
        self.cpos = SP.class_positions(g, m["cls"], m["ill_class"])
        raw = raw_of(g)
        self.stays = raw["stays"]
        self.raw, self.img = RawWalker(raw, True), ScanWalker(m, self.cpos)
        self.um = g.get("umap")
        self.n_states, self.n_hot, self.stride, self.n_classes = m["n_states"], m["n_hot"], m["stride"], m["n_classes"]
        self.n_plain = m["emit_base"] // m["stride"]
        self._memo = {}
        assert m["emit_base"] % m["stride"] == 0 and m["special_base"] == (m["n_hot"] + 1) * m["stride"]

    def kind(self, row):
        return PLAIN if row < self.n_plain else EMIT if row < self.n_hot else COLD

    def classes(self, data):
        """csrc/utf8.h as table_walker restates it: scalar mode reads a lead byte as the class of the scalar value it begins, a continuation
        byte a well-formed sequence holds keeps its own class (which stays), a stray one is ill-formed"""
        cm, out = self.g["classmap"], []
        for j, b in enumerate(data):
            c = int(cm[b])
            if self.um is not None and b >= 0xC0:
                c = scalar_class(self.um, data, j)
            elif self.um is not None and b >= 0x80 and not cont_covered(data, j):
                c = self.um[0]
            out.append(c)
        return out

    def _step(self, s, q, c):
        """both walkers over one class, memoised (the cases walk some hundred thousand bytes)"""
        key = (s, q, c)
        if key not in self._memo:
            self._memo[key] = (self.raw.step(s, c), self.img.step(q, c))
        return self._memo[key]

    def walk(self, data):
        """-> dict: steps [(byte index, row left, row entered, atoms reported)], the atoms of the streaming table and of the raw DFA
        (distinct, in order of first report), the end row and its atoms, the atoms the start state reports"""
        (s, e), (q, f) = self.raw.start(), self.img.start()
        got, want, steps = sorted(f), sorted(e), []
        start = set(f)
        for j, c in enumerate(self.classes(data)):
            if self.stays[c]:
                steps.append((j, q, q, ()))
                continue
            ((s, e), (t, f)) = self._step(s, q, c)
            want += sorted(e)
            got += sorted(f)
            steps.append((j, q, t, tuple(sorted(f))))
            q = t
        end_got, end_want = self.img.end(q), self.raw.end(s)
        before = list(dict.fromkeys(got))
        reports = got + sorted(end_got)
        return dict(steps=steps, end_row=q, atoms=list(dict.fromkeys(reports)), raw_atoms=list(dict.fromkeys(want + sorted(end_want))), reports=reports, start=start,
                    end_atoms=sorted(end_got), before_end=before, n=len(data))

    def features(self, data):
        """what the walk of `data` exercises in scan_body, as hashable keys"""
        w = self.walk(data)
        f = set()
        for j, q, t, atoms in w["steps"]:
            f.add(("enter", self.kind(t), j % 4))          # the cell a step reads, by the tier of the row it names, at byte j % 4 of its group
            f.add(("leave", self.kind(q), j % 4))          # (a cold row left: the lane is parked, the cell comes from the global table)
            if self.kind(q) == COLD:
                f.add(("cold to", self.kind(t), j % 4))
            if atoms:  # a hot row's EMIT cell holds one atom (0x8000 | atom) or a list id; a special cell always names a list
                single = t < self.n_hot and int(self.m["tab"][t * self.stride + self.n_classes + 2]) & 0x8000
                f.add(("emit", self.kind(t), "single" if single else "list"))
        f.add(("end", self.kind(w["end_row"]), w["n"] % 4))  # the field ends n % 4 bytes into a group, on a row of this tier
        if w["end_atoms"]:
            f.add(("end atoms", self.kind(w["end_row"]), min(len(w["end_atoms"]), 2)))
            if len(w["before_end"]) >= 2 and not set(w["end_atoms"]) <= set(w["before_end"]):
                f.add("end atom, record full" if len(w["end_atoms"]) == 1 else "end list, record full")
        if w["start"]:
            f.add("start emit")
        if len(w["reports"]) != len(set(w["reports"])):
            f.add("atom twice")
        f.add(("atoms", len(w["atoms"])))
        return f

    # -- strings --
    @functools.cached_property
    def reps(self):
        """one printable byte per class that has one (letters and digits first): the alphabet of the searches"""
        order = [ord(ch) for ch in "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-_.=&%+#!/:;,@^*()[]{}<>|?$' "]
        reps = {}
        for b in order:
            reps.setdefault(int(self.g["classmap"][b]), b)
        return reps

    @functools.cached_property
    def next_rows(self):
        """row x representative byte -> row entered (the streaming table's own cells)"""
        cl = sorted(self.reps)
        nx = np.zeros((self.n_states, len(cl)), dtype=np.int64)
        for q in range(self.n_states):
            for i, c in enumerate(cl):
                nx[q, i] = self.img.step(q, c)[0]
        return cl, nx

    @functools.cached_property
    def rest(self):
        """the row a walk is on after a filler byte: every further filler keeps it there and reports nothing"""
        c = int(self.g["classmap"][FILL])
        r, e = self.img.step(0, c)
        assert self.img.step(r, c) == (r, frozenset()) and not e, "a filler byte does not leave the walk at rest"
        return r

    def search(self, src):
        """breadth-first from row src over reps -> (dist, parent (row, byte))"""
        cl, nx = self.next_rows
        dist, par, todo = {src: 0}, {}, [src]
        while todo:
            new = []
            for q in todo:
                for i, c in enumerate(cl):
                    t = int(nx[q, i])
                    if t not in dist:
                        dist[t] = dist[q] + 1
                        par[t] = (q, self.reps[c])
                        new.append(t)
            todo = new
        return dist, par

    def path_to(self, s, par, src):
        out = []
        while s != src:
            s, b = par[s]
            out.append(b)
        return bytes(reversed(out))

    def to_report(self, src, limit=40):
        """the shortest printable bytes from row src after which the walk has reported an atom (on a step or at the field's end)"""
        cl, nx = self.next_rows
        seen, todo = {src}, [(src, b"")]
        while todo:
            new = []
            for q, s in todo:
                if s and self.img.end(q):
                    return s
                for i, c in enumerate(cl):
                    t, e = self.img.step(q, c)
                    if e:
                        return s + bytes([self.reps[c]])
                    if t not in seen and len(s) < limit:
                        seen.add(t)
                        new.append((t, s + bytes([self.reps[c]])))
            todo = new
        return None


# ---------------------------------------------------------------------------------------------------------
# rule sets
# ---------------------------------------------------------------------------------------------------------
def act(k):
    return [B] if k % 2 == 0 else [CAP]


# one rule on each other field and on a header column: under PWAF_OPT_NO_PREFILTER a scan_kernel pass each
EXTRA = [("xh", 'http_request.host.ends_with(".evil.example")', [B]), ("xu", 'http_request.user_agent.matches("sqlmap/[0-9]+")', [CAP]),
         ("xa", f'http_request.headers["{HEADER}"].contains("zzqq")', [B]), ("xm", 'http_request.method.matches("P[A-Z]{5}$")', [CAP])]
LEGS = ("as built", "small budget", "rule hits", "natural")


class RuleSet:
    """preds[k]: predicate texts over the url. Verdict form `http_request.path == "/h<k>" && <predicate k>`: the request's path picks
    which predicate decides its verdict (as in lscan_cases); bare form for the hit-matrix leg. natural: the indices of the predicates no
    prefilter can be built for -- the set of them alone is the leg that runs with flags 0. budget: the small lds_table_budget."""

    def __init__(self, name, preds, budget, natural=(), extra=EXTRA, table_bytes=0):
        self.name, self.preds, self.budget, self.natural, self.field_id, self.table_bytes = name, list(preds), budget, list(natural), URL, table_bytes
        self.bare_rules = [(f"b{k}", p, act(k)) for k, p in enumerate(self.preds)] + list(extra)
        self.verdict_rules = [(f"h{k}", f'http_request.path == "/h{k}" && {p}', act(k)) for k, p in enumerate(self.preds)] + list(extra)
        # (the natural leg keeps the rules' places: an index of the oracle's verdict means the same predicate on every leg)
        self.natural_rules = [r if k in self.natural or k >= len(self.preds) else (r[0], 'http_request.path == "/never"', r[2]) for k, r in enumerate(self.verdict_rules)]
        self._scans, self._models = {}, {}

    def leg(self, leg):
        """-> (rules, engine flags, lds_table_budget)"""
        return {"as built": (self.verdict_rules, NP, 0), "small budget": (self.verdict_rules, NP, self.budget), "tuned": (self.verdict_rules, NP, self.budget),
                "rule hits": (self.bare_rules, NP | HITS, self.budget), "natural": (self.natural_rules, 0, self.budget), "natural tuned": (self.natural_rules, 0, self.budget)}[leg]

    def scan(self, leg, sample=None):
        """the harness's output for a leg; sample: (key, RequestBatch) of the tuned leg"""
        key = (leg, sample[0] if sample else None)
        if key not in self._scans:
            rules, flags, budget = self.leg(leg)
            first = harness(rules, flags, budget, table_bytes=self.table_bytes)
            cols = sample_columns(sample[1], first.tables.header_names) if sample else None
            self._scans[key] = harness(rules, flags, budget, cols, self.table_bytes) if sample else first
        return self._scans[key]

    def pass_of(self, sc, field_id=URL):
        """the ONE pass of the field, asserted to be a plain scan pass (scan_kernel walks it: no gate, no identity list, no short literals)"""
        ks = [k for k, g in enumerate(sc.groups) if g["field"] == field_id and not g.get("filter_cols")]
        assert len(ks) == 1, (self.name, field_id, ks)
        r = sc.roles[ks[0]]
        assert r["gate"] < 0 and not r["filtered"] and not r["identity"] and not r["short_lit"], (self.name, field_id, r)
        return ks[0]

    def model(self, leg, sample=None, field_id=URL):
        key = (leg, sample[0] if sample else None, field_id)
        if key not in self._models:
            sc = self.scan(leg, sample)
            self._models[key] = StreamModel(sc, self.pass_of(sc, field_id))
        return self._models[key]

    def request(self, value, k=0, **other):
        f = {"host": "host.example.com", "url": "/i", "path": f"/h{k}", "user_agent": "Mozilla/5.0 (X11)", "method": "GET", "headers": {HEADER: "none-of-it-00"}}
        f.update(other)
        f["url"] = value
        return Request(**f)


def scan_names(sc):
    """the scan_<field>_g<k> profile entries of one batch, in launch order (csrc/pipeline.cpp: launch_plain_scans)"""
    out = []
    for k, g in enumerate(sc.groups):
        r = sc.roles[k]
        if r["gate"] >= 0 or r["identity"] or r["short_lit"]:
            continue
        out.append(f"scan_{FIELD_NAMES[g['field']]}_g{k}" if g["field"] < 5 else f"scan_hdr{g['field'] - 5}_g{k}")
    return out


def u(f="url"):
    return f"http_request.{f}"


def lits(seed, n, length=9):
    rng = random.Random(seed)
    alpha = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPRSTUVW0123456789-_=&%"  # (no X, Q, Y, Z, ~, #, !: the window cases' own bytes)
    return ["".join(rng.choice(alpha) for _ in range(length)) for _ in range(n)]


UNFILTERABLE = '^[a-z]+[0-9]$'


@functools.lru_cache(maxsize=None)
def set_m():
    """M: literals and regexes whose table has plain hot rows, emitting hot rows and cold rows under the small budget"""
    L = lits(31, 4)
    preds = [f'{u()}.contains({H.q(L[0])})', f'{u()}.contains({H.q(L[1])})', f'{u()}.matches({H.q(L[2][:4] + "[0-9]{2,4}" + L[2][4:7] + "[a-f]+" + L[2][7:])})',
             f'{u()}.matches({H.q("id=[0-9]{3,5}x")})', f'{u()}.matches({H.q(UNFILTERABLE)})', f'{u()}.ends_with(".php")', f'{u()}.contains("XQ")', f'{u()} == ""',
             f'{u()}.ends_with("Z")', f'{u()}.contains("q#7")', f'{u()}.contains({H.q(L[3])})']
    rs = RuleSet("M", preds, budget=2 * 40 * 24, natural=[4])
    rs.lits, rs.k_rx, rs.k_unf, rs.k_xq, rs.k_empty, rs.k_z, rs.k_short = L, 2, 4, 6, 7, 8, 9
    rs.rx_hit = L[2][:4] + "123" + L[2][4:7] + "fe" + L[2][7:]
    return rs


TWIN = "Tw1nSuffix=x"


@functools.lru_cache(maxsize=None)
def set_e():
    """E: emit shapes -- two literals that end in the same state (an emit list), ends_with and $ (the END cell, an END list of two), an atom
    the start state emits, nine literals for records of 0 - 9 atoms, rules that need 3 and 4 atoms of the pass"""
    L = lits(32, 9, 6)
    c = lambda x: f'{u()}.contains({H.q(x)})'  # noqa: E731
    preds = [c(TWIN), c(TWIN[4:]), f'{u()}.ends_with("zq#7end")', f'{u()}.ends_with("7end")', f'{u()}.matches({H.q("kw=[0-9]+$")})', f'{u()}.matches("^Q*")',
             " && ".join(c(x) for x in L[:3]), " && ".join(c(x) for x in L[3:7]), c(L[7]), c(L[8]), f'{u()}.matches({H.q(UNFILTERABLE)})'] + [c(x) for x in L[:7]]
    rs = RuleSet("E", preds, budget=1024, natural=[10])
    rs.lits, rs.k_twin, rs.k_ends, rs.k_dollar, rs.k_start, rs.k_three, rs.k_four = L, 0, 2, 4, 5, 6, 7
    return rs


@functools.lru_cache(maxsize=None)
def set_u():
    """U: a scalar-mode pass (utf8.h): a Unicode class and a negated class beside literals"""
    L = lits(33, 3)
    preds = [f'{u()}.matches({H.q("Uni" + chr(92) + "p{Lu}[0-9]code")})', f'{u()}.matches({H.q("neg[^a-z0-9]end")})', f'{u()}.contains({H.q(L[0])})', f'{u()}.contains("é=1")',
             f'{u()}.matches({H.q("^[a-z]+" + chr(92) + "p{Greek}$")})', f'{u()}.ends_with("Z")', f'{u()}.contains({H.q(L[1])})', f'{u()}.contains("€uro")', f'{u()}.matches({H.q("x.y")})']
    rs = RuleSet("U", preds, budget=1024, natural=[4])
    rs.lits, rs.k_lu, rs.k_neg, rs.k_dot = L, 0, 1, 8
    return rs


WIDE_CHARS = [chr(c) for c in range(0x21, 0x7F) if chr(c) not in '"\\~XQZ'] + [chr(c) for c in range(0xA1, 0x100)]


@functools.lru_cache(maxsize=None)
def set_x():
    """X: more than 127 byte classes (the class table has 32-bit entries): long literals that between them tell every printable byte and
    every byte of the two-byte sequences of U+00A1 - U+00FF apart"""
    rng = random.Random(34)
    chars = list(WIDE_CHARS)
    preds = []
    for k in range(4):
        rng.shuffle(chars)
        preds.append(f'{u()}.contains({H.q("".join(chars[:60]))})')
        preds.append(f'{u()}.ends_with({H.q("".join(chars[60:120]))})')
    preds += [f'{u()}.ends_with("Z")', f'{u()} == ""', f'{u()}.contains("XQ")', f'{u()}.matches({H.q(UNFILTERABLE)})']
    rs = RuleSet("X", preds, budget=2 * 200 * 40, natural=[11])
    rs.k_z, rs.k_empty, rs.k_xq = 8, 9, 10
    return rs


GAP_MAX = 30


@functools.lru_cache(maxsize=None)
def set_g():
    """G: counted-gap patterns under a 64 KiB table budget (as helpers.kind_rules("gap")): each gets a gated gap pass, their literal
    factors join the url's plain patterns as hidden atoms -- the url's plain scan pass owns them and feeds the gap passes from its
    finished records"""
    L = lits(35, 16, 6)
    preds = [f'{u()}.matches({H.q(L[2 * j] + ".{0," + str(GAP_MAX) + "}" + L[2 * j + 1])})' for j in range(6)]
    preds += [f'{u()}.contains({H.q(L[12])})', f'{u()}.contains({H.q(L[13])})', f'{u()}.contains({H.q(L[14])})', f'{u()}.ends_with("Z")', f'{u()}.matches({H.q(UNFILTERABLE)})']
    rs = RuleSet("G", preds, budget=2048, natural=[10], table_bytes=65536)
    rs.lits, rs.gaps = L, [(L[2 * j], L[2 * j + 1]) for j in range(6)]
    rs.elsewhere = range(6)  # (the gap patterns' own atoms are reported by their gap passes: lscan_kernel's)
    return rs


SETS = {"M": set_m, "E": set_e, "U": set_u, "X": set_x, "G": set_g}


# ---------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------
class Case:
    """batches: [(label, batch)] sent in this order, `turns` times; sample: (key, batch) the tuned leg is tuned on; measured: what the
    builder proved, for the report"""

    def __init__(self, name, rs, batches, measured, turns=1, sample=None):
        self.name, self.rs, self.batches, self.measured, self.turns, self.sample = name, rs, batches, measured, turns, sample


def keyed(rs, values, default=0, **other):
    """requests that observe each value under the key of the first bare predicate it satisfies (the oracle says which): its verdict then
    depends on that predicate's atoms; every fifth under another key, a value that satisfies none under a rotating one"""
    from oracle import pyoracle

    probe = RequestBatch.from_requests([rs.request(v) for v in values])
    hit, _ = H.oracle_matrix(pyoracle.Oracle(rs.bare_rules, {}), probe)
    reqs = []
    for i, v in enumerate(values):
        ks = np.nonzero(hit[:len(rs.preds), i])[0].tolist()
        k = ks[i % len(ks)] if ks and i % 5 else (default + i) % len(rs.preds)
        reqs.append(rs.request(v, k, **other))
    return reqs


def sample_of(label, batch):
    """a tuning sample as (key, RequestBatch). The key is the sample's IDENTITY in every cache (RuleSet.scan, RuleSet.model, the device
    suite's engines): a digest of every column's offsets and bytes, so that two samples share a key only if tuning cannot tell them
    apart; the label in front is for the reader"""
    h = hashlib.sha1()
    names = sorted(batch.headers)
    for name, col in zip(list(FIELD_NAMES) + names, sample_columns(batch, names)):
        h.update(name.encode() + b"\0" + len(col).to_bytes(4, "little"))
        for v in col:
            h.update(len(v).to_bytes(4, "little") + v)
    return (f"{label} {h.hexdigest()}", batch)


def same_sample(a, b):
    """the two samples hold the same values in every column (all that tune_host reads of a sample)"""
    na, nb = sorted(a[1].headers), sorted(b[1].headers)
    return na == nb and sample_columns(a[1], na) == sample_columns(b[1], nb)


def fixed_sample(rs, label, total, n=64, pieces=()):
    """a tuning sample of n requests whose url bytes sum to `total`: the pieces (strings of the case, so that the sample's visits re-rank
    the rows they walk) padded with fillers"""
    base, extra = divmod(total, n)
    reqs = []
    for i in range(n):
        want = base + (1 if i < extra else 0)
        piece = pieces[i % len(pieces)] if pieces else b""
        piece = piece if isinstance(piece, bytes) else piece.encode()
        v = (b"~" * max(0, want - len(piece)) + piece)[-want:] if want else b""
        reqs.append(rs.request(v, i % len(rs.preds), host="tuning.host.example", path="/path/of/a/sample", method="PROPPATCH-LONG", user_agent="Mozilla/5.0 (sample)",
                               headers={HEADER: "sample-header-value"}))
    batch = RequestBatch.from_requests(reqs)
    assert int(batch.offsets[URL][-1]) == total
    return sample_of(label, batch)


def chunks_of(rs, sample, leg="tuned"):
    """TuneOut::chunks of the url pass for a sample, from the harness (the fourth word of UFLT)"""
    sc = rs.scan(leg, sample)
    k = rs.pass_of(sc)
    return int(np.frombuffer(sc.img[k]["UFLT"], dtype="<u4")[3])


def assert_tuned_as_planned(program, sc, untuned, what):
    """What a tuned program or engine shows of its tuning (program: a CompiledProgram after tune(), or RuleEngine.program after the engine's
    tune()): pwaf_program_flat_image answers with the flat tables rebuilt for the sample -- states renumbered by the sample's visits, out
    of the same TuneOut the streaming tables' row order and TuneOut::chunks come from. They must be the harness's over THIS sample
    (sc), and the sample must have moved a state against the untuned plan: an engine that kept its tables, or one tuned on another
    case's sample, fails here. No hook gives an engine's chunks per iteration (docs/scan_edges.md)."""
    moved = 0
    for k in range(len(sc.groups)):
        mine = {t: pl for t, _, pl in parse_dump(program.flat_image(k, 0))}
        for sfx in ("SHP", "FLT", "DLT", "EMO", "EML", "ENO", "ENL"):
            assert mine["F" + sfx] == sc.img[k]["F" + sfx], (what, k, sfx)
        moved += any(sc.img[k]["F" + sfx] != untuned.img[k]["F" + sfx] for sfx in ("FLT", "DLT"))
    assert moved, (what, "the sample's visits reorder no table")


def sample_for(rs, ch, pieces=()):
    """the smallest mean url length that tunes the pass to CH chunks per iteration: just below 48 bytes, exactly 48, exactly 80"""
    n = 64
    return fixed_sample(rs, f"CH{ch}", {1: CH2_MEAN * n - 1, 2: CH2_MEAN * n, 4: CH4_MEAN * n}[ch], n, pieces)


def window_items(rs, ch, with_short):
    """fields of every length from 0 to 2 * 16 * CH + 17 at every arena offset mod 16, the deciding byte last; and the same fields ending
    in X (lay_out puts a field that begins with Q behind each) -> [(arena offset mod 16, value, key, tag)]"""
    items = []
    for o in range(16):
        for n in range(0, 2 * 16 * ch + 18):
            hit = (o + n) % 2 == 0
            if n == 0:
                items.append((o, b"", rs.k_empty, "decide"))
            elif with_short and n >= 3 and (o + n) % 3 == 0:
                items.append((o, b"~" * (n - 3) + (b"q#7" if hit else b"q#!"), rs.k_short, "decide"))
            else:
                items.append((o, b"~" * (n - 1) + (b"Z" if hit else b"Y"), rs.k_z, "decide"))
            if n:
                items.append((o, b"~" * (n - 1) + b"X", rs.k_xq, "X"))
    return items


def lay_out(rs, items, last):
    """the items in order, each at its arena offset mod 16 (a request of 1 - 16 bytes that BEGINS WITH Q in between, so that the byte
    behind every field is a Q); `last`: the arena's last request, behind which the pad is filled with Q as well"""
    reqs, tags, cur = [], [], 0
    for o, v, k, tag in items + [last]:
        gap = (o - cur) % 16 or 16
        reqs.append(rs.request(b"Q" + b"~" * (gap - 1), rs.k_xq))
        tags.append("gap")
        cur += gap
        reqs.append(rs.request(v, k))
        tags.append(tag)
        cur += len(v)
    batch = RequestBatch.from_requests(reqs)
    off = batch.offsets[URL]
    batch.data[URL][int(off[-1]):] = ord("Q")  # the slack behind the arena: a read past the last field's end completes "XQ" too
    return batch, tags


@functools.lru_cache(maxsize=None)
def case_w(ch, set_name="M"):
    """W. windows: see window_items; tuned on a sample whose mean url length gives CH chunks per iteration (proved with the harness)"""
    rs = SETS[set_name]()
    kstep = 16 * ch
    items = window_items(rs, ch, with_short=set_name == "M")
    items += [(3, b"~XQ~", rs.k_xq, "control"), (5, b"XQ", rs.k_xq, "control"), (7, b"~" * kstep + b"XQ", rs.k_xq, "control")]
    batch, tags = lay_out(rs, items, (9, b"~" * (kstep + 2) + b"X", rs.k_xq, "X"))
    off, data = batch.offsets[URL].astype(np.int64), batch.data[URL]
    lens = np.diff(off)
    seen = {(int(off[i]) % 16, int(lens[i])) for i in range(batch.n) if tags[i] == "decide"}
    assert seen == {(o, n) for o in range(16) for n in range(2 * kstep + 18)}, "a length is missing at an arena offset"
    xs = [i for i in range(batch.n) if tags[i] == "X"]
    assert {(int(off[i]) % 16, int(lens[i])) for i in xs} >= {(o, n) for o in range(16) for n in range(1, 2 * kstep + 18)}
    assert all(data[off[i + 1] - 1] == ord("X") and data[off[i + 1]] == ord("Q") for i in xs), "the byte behind a field that ends in X is not a Q"
    assert tags[-1] == "X" and bytes(data[off[-1]:off[-1] + PAD]) == b"Q" * PAD
    pieces = [rs.rx_hit, rs.lits[0], rs.lits[1], "id=1234x", "abc7", "q#7", "~.php"] if set_name == "M" else []
    sample = sample_for(rs, ch, pieces)
    got = chunks_of(rs, sample)
    assert got == ch, f"the sample tunes the url pass to {got} chunks per iteration, the case was built for {ch}"
    name = f"W{ch}" if set_name == "M" else f"{set_name}W{ch}"
    return Case(name, rs, [(name, batch)], dict(n=batch.n, chunks=got, mean=float(np.mean(np.diff(sample[1].offsets[URL])))), sample=sample)


def simulate_pulls(lens, w0, w1, kstep):
    """scan_body's pull-ahead loop for ONE wave as a count of events (lengths alone: no bytes, no table): -> dict with the block switches
    served from the offsets prefetched an iteration earlier and those that load on the spot, takes clipped at a block's end and at the
    share's end, requests that finish in the iteration after they were taken. A restatement kept to PROVE a batch's shape; what a
    request's verdict must be is the oracle's to say."""
    NONE = None
    r, left, r2 = [NONE] * 64, [0] * 64, [NONE] * 64
    nxt = blk = w0
    n_base = NONE
    ev = dict(prefetched=0, on_the_spot=0, clip_block=0, clip_share=0, iterations=0, taken=0, spot_blocks=[])
    while True:
        f_base = blk + 64
        last = [r[l] is NONE or left[l] <= kstep for l in range(64)]
        want = [l for l in range(64) if last[l] and r2[l] is NONE]
        if want and nxt < w1:
            avail = min(w1 - nxt, blk + 64 - nxt)
            if len(want) > avail:
                ev["clip_share" if avail == w1 - nxt else "clip_block"] += 1
            for rank, l in enumerate(want[:avail]):
                r2[l] = nxt + rank
            ev["taken"] += min(len(want), avail)
            nxt += min(len(want), avail)
            if nxt == blk + 64 and nxt < w1:
                blk += 64
                ev["prefetched" if n_base == blk else "on_the_spot"] += 1
                if n_base != blk:
                    ev["spot_blocks"].append((blk, n_base))  # (the block loaded on the spot, the block whose offsets the prefetch holds: None = nothing yet)
        if all(x is NONE for x in r) and all(x is NONE for x in r2):
            break
        ev["iterations"] += 1
        for l in range(64):
            if r[l] is not NONE:
                left[l] -= min(kstep, left[l])
                if left[l] <= 0:
                    r[l] = NONE
            if r[l] is NONE and r2[l] is not NONE:
                r[l], left[l], r2[l] = r2[l], int(lens[r2[l]]), NONE
        n_base = f_base
    assert ev["taken"] == w1 - w0
    return ev


PLAIN20 = b"~" * 20
HIT20 = b"~" * 17 + b"q#7"


def share_batch(rs, n, n_cus=MI355X_CUS):
    """n requests with 20-byte urls; the first and the last request of every wave's share and request n - 1 match"""
    _, per, sh = shares(n, n_cus)
    marks = {w0 for w0, _ in sh} | {w1 - 1 for _, w1 in sh} | {n - 1}
    reqs = [rs.request(HIT20 if i in marks else PLAIN20, rs.k_short if i % 7 else rs.k_z) for i in range(n)]
    return RequestBatch.from_requests(reqs), per, sh, marks


B_SIZES = (1, 15, 16, 17, 1024, 1040, 4096, 4097)
RUNS = (63, 64, 65, 128, 130, 200)


@functools.lru_cache(maxsize=None)
def case_b():
    """B. blocks and shares: batch sizes at which a share changes shape, each with matches planted on both sides of every share boundary"""
    rs = set_m()
    batches, measured = [], {}
    want_per = {1: 1, 15: 1, 16: 1, 17: 2, 1024: 64, 1040: 65, 4096: 256, 4097: 129}
    for n in B_SIZES:
        batch, per, sh, marks = share_batch(rs, n)
        assert per == want_per[n], (n, per)
        batches.append((f"B {n}", batch))
        measured[n] = dict(per_wave=per, waves=len(sh), workgroups=shares(n)[0])
    assert measured[4096]["workgroups"] == 1 and measured[4097]["workgroups"] == 2 and shares(4097)[2][-1] == (3999, 4097), "a short last share"
    assert measured[15]["waves"] == 15 and measured[1]["waves"] == 1, "waves without a share (w0 >= w1) leave at once"
    lens = np.full(1040, 20)
    ev = simulate_pulls(lens, 0, 65, 16)
    # one request in a second block; a wave's FIRST switch always loads on the spot (all 64 lanes take in the first iteration: nothing was prefetched)
    assert ev["clip_block"] == 0 and ev["on_the_spot"] == 1 and ev["prefetched"] == 0 and ev["clip_share"] >= 1, ev
    return Case("B", rs, batches, measured, sample=sample_for(rs, 1, [HIT20]))


def runs_batch(rs, value, k_match):
    """4 096 requests (one workgroup, shares of 256): in share 2 j + s a run of RUNS[j] fields `value` (empty, or one byte) from share
    offset 0 (s = 0) or 37 (s = 1), every third observed under the key that matches it, a matching 20-byte request behind the run"""
    n = 4096
    _, per, sh = shares(n)
    assert per == 256 and len(sh) == 16
    urls, keys = [PLAIN20] * n, [rs.k_short] * n
    for j, run in enumerate(RUNS):
        for s, start in enumerate((0, 37)):
            w0 = sh[2 * j + s][0]
            for i in range(run):
                urls[w0 + start + i] = value
                keys[w0 + start + i] = k_match if i % 3 == 0 else rs.k_short
            urls[w0 + start + run] = HIT20
    batch = RequestBatch.from_requests([rs.request(v, k) for v, k in zip(urls, keys)])
    lens = np.diff(batch.offsets[URL].astype(np.int64))
    evs = [simulate_pulls(lens, w0, w1, 16) for w0, w1 in sh[:12]]
    return batch, evs


@functools.lru_cache(maxsize=None)
def case_b_runs():
    """B. runs of empty and of one-byte fields: every request of a run finishes in the iteration after it was taken, so 64 are taken per
    iteration and block switches follow one another -- the second of two consecutive switches cannot use the prefetched offsets"""
    rs = set_m()
    batches, measured = [], {}
    for label, value, k in (("empty", b"", rs.k_empty), ("one byte", b"Z", rs.k_z)):
        batch, evs = runs_batch(rs, value, k)
        measured[label] = dict(on_the_spot=sum(e["on_the_spot"] for e in evs), prefetched=sum(e["prefetched"] for e in evs), clip_block=sum(e["clip_block"] for e in evs))
        # runs of 128 and more from share offset 0 switch twice in a row; every share of 256 switches three times in all
        assert all(e["on_the_spot"] + e["prefetched"] == 3 for e in evs), evs
        # a wave's first switch loads on the spot (nothing was prefetched yet); so does every switch that follows another at once: one more
        # per 64 requests of a run from share offset 0, one more for a run of 128 and more from offset 37
        assert [e["on_the_spot"] for e in evs[0::2]] == [1 + min(2, run // 64) for run in RUNS], [e["on_the_spot"] for e in evs]
        assert [e["on_the_spot"] for e in evs[1::2]] == [1 + (run >= 128) for run in RUNS], [e["on_the_spot"] for e in evs]
        assert measured[label]["clip_block"] > 0, "no take is clipped at a block's end"
        batches.append((f"B runs, {label}", batch))
    return Case("B runs", rs, batches, measured, sample=sample_for(rs, 1, [HIT20]))


LONG = 40 * 1024


@functools.lru_cache(maxsize=None)
def case_b_long():
    """B. one field of 40 KiB at lane 0 and at lane 63 of the first take of a share, among 20-byte fields: the other lanes run through
    the share's four blocks while it walks; the match is at its last byte"""
    rs = set_m()
    n = 4096
    _, per, sh = shares(n)
    reqs = [rs.request(PLAIN20 if i % 5 else HIT20, rs.k_short) for i in range(n)]
    at = [sh[0][0], sh[1][0] + 63, sh[2][0] + 63, sh[3][0]]
    for j, i in enumerate(at):
        reqs[i] = rs.request(b"~" * (LONG - 3) + (b"q#7" if j < 2 else b"q#!"), rs.k_short)
    batch = RequestBatch.from_requests(reqs)
    lens = np.diff(batch.offsets[URL].astype(np.int64))
    for w in range(4):
        ev = simulate_pulls(lens, *sh[w], 16)
        assert ev["iterations"] >= LONG // 16 and ev["prefetched"] == 2 and ev["on_the_spot"] == 1 and ev["clip_block"] >= 1, ev
    return Case("B long", rs, [("B long", batch)], dict(n=n, at=at), sample=sample_for(rs, 1, [HIT20]))


def tiled_shape(n_cus=MI355X_CUS):
    """B. one batch beyond the launch's cap of one workgroup per CU: n = 4096 * CUs + 777, made by tiling the 4 097 case (and cutting the
    last tile): -> (the base batch, times, n); every workgroup then holds more than 16 x 256 requests"""
    rs = set_m()
    base = share_batch(rs, 4097)[0]
    base.headers = {}  # (RequestBatch.tile carries no header columns: an absent header reads as "")
    n = 4096 * n_cus + 777
    times = (n + base.n - 1) // base.n
    blocks, per, sh = shares(n, n_cus)
    assert blocks == n_cus and per > MIN_PER_WAVE and 0 < n_cus * WAVES_PER_WG - len(sh) < WAVES_PER_WG and sh[-1][1] == n, "the cap of one workgroup per CU does not bind"
    return base, times, n


def targets(m, kinds_wanted, per_kind=3):
    """edges (row left, byte, row entered) of the streaming table, reachable from rest over printable bytes, by the tiers of the rows on
    both sides -> {(kind left, kind entered): [(head bytes up to and including the step, tail to the nearest report)]}"""
    dist, par = m.search(m.rest)
    cl, nx = m.next_rows
    out = {}
    for q in sorted(dist, key=lambda s: dist[s]):
        for i, c in enumerate(cl):
            t = int(nx[q, i])
            key = (m.kind(q), m.kind(t))
            if key in kinds_wanted and len(out.setdefault(key, [])) < per_kind and t != m.rest and t != 0:
                head = m.path_to(q, par, m.rest) + bytes([m.reps[c]])
                out[key].append((head, m.to_report(t) or b""))
    return out


T_KINDS = {(PLAIN, PLAIN), (PLAIN, EMIT), (PLAIN, COLD), (EMIT, COLD), (COLD, PLAIN), (COLD, EMIT), (COLD, COLD), (EMIT, PLAIN), (EMIT, EMIT)}


@functools.lru_cache(maxsize=None)
def case_t():
    """T. tiers: over the table of the small budget, for every pair of tiers (row left, row entered) the deciding step at byte 0, 1, 2 and 3
    of a group of four, the field ending there and further on, its near miss; two lanes of one wave in different tiers in the same group"""
    rs = set_m()
    m = rs.model("small budget")
    assert 1 < m.n_hot < m.n_states and 0 < m.m["emit_base"] < m.m["special_base"], "set M: no plain hot, emitting hot and cold rows"
    assert m.kind(m.rest) == PLAIN
    tg = targets(m, T_KINDS)
    values = []
    for key, lst in tg.items():
        for head, tail in lst:
            for p in range(4):
                pad = (p - (len(head) - 1)) % 4 or 4
                values.append(b"~" * pad + head)                      # the field ends behind the step: 1, 2, 3 or 4 bytes into its group
                if tail:
                    values.append(b"~" * pad + head + tail)
                    values.append(b"~" * pad + head + tail[:-1] + b"!")
                    values.append(b"~" * pad + head + tail + b"~")
    # two lanes of the wave's first take: lane 0 on plain rows, lane 1 entering a cold row, in the same group of four
    cold_head = tg[(PLAIN, COLD)][0][0] if (PLAIN, COLD) in tg else tg[(EMIT, COLD)][0][0]
    pair = [b"~" * 40, b"~" * 8 + cold_head + b"~" * 20]
    reqs = keyed(rs, pair + list(dict.fromkeys(values)) + [rs.rx_hit.encode(), b"~" + rs.rx_hit.encode() + b"~.php", b"x.php", b"abc7", b"id=12345x"])
    batch = RequestBatch.from_requests(reqs)
    return Case("T", rs, [("T", batch)], dict(n=batch.n, edges={f"{a} -> {b}": len(v) for (a, b), v in tg.items()}),
                sample=sample_for(rs, 1, [v for v in values[::7]]))


def coverage(m, batch, only=None):
    """feature -> number of requests whose url shows it"""
    count = {}
    for i in (range(batch.n) if only is None else only):
        for f in m.features(batch.field_bytes(URL, i)):
            count[f] = count.get(f, 0) + 1
    return count


def assert_t_coverage(m, batch):
    """the assertions of case T over a model (the small budget's, or a tuned one's): from the row trace of every request"""
    cov = coverage(m, batch)
    for p in range(4):
        for kind in KINDS:
            assert cov.get(("enter", kind, p)), f"no step enters a {kind} row at byte {p} of a group"
        assert cov.get(("cold to", COLD, p)), f"no step from a cold row to a cold row at byte {p} of a group"
        assert cov.get(("cold to", PLAIN, p)) or cov.get(("cold to", EMIT, p)), f"no cold row is left for a hot one at byte {p} of a group"
    for e in (1, 2, 3):
        for kind in KINDS:
            assert cov.get(("end", kind, e)), f"no field ends {e} bytes into a group on a {kind} row"
    assert cov.get(("end atoms", COLD, 1)), "no field ends on a cold row that has an END atom (the END cell read from the global table)"
    assert cov.get(("end atoms", PLAIN, 1)) or cov.get(("end atoms", EMIT, 1)), "no field ends on a hot row that has an END atom"
    w0, w1 = m.walk(batch.field_bytes(URL, 0)), m.walk(batch.field_bytes(URL, 1))
    assert shares(batch.n)[1] >= 2, "requests 0 and 1 are not lanes 0 and 1 of one wave's first take"
    groups = [g for g in range(min(w0["n"], w1["n"]) // 4)
              if all(m.kind(x[2]) == PLAIN for x in w0["steps"][4 * g:4 * g + 4]) and any(m.kind(x[2]) == COLD for x in w1["steps"][4 * g:4 * g + 4])]
    assert groups, "no group of four in which lane 0 stays on plain rows while lane 1 enters a cold one"
    return cov


@functools.lru_cache(maxsize=None)
def case_e():
    """E. emits: every shape of set E, in fields that report 1, 2, 3, 4, 5 and 10 distinct atoms (the start state's atom is in every
    record of this set: fields without any atom are set M's, in W and B)"""
    rs = set_e()
    L = rs.lits
    j = lambda xs: "~".join(xs)  # noqa: E731
    vals = ["", "~", TWIN, "x" + TWIN + "y", TWIN[4:], j([L[0], L[0]]), j([TWIN, TWIN]), j(L[:3]), j(L[:2] + ["x"]), j(L[3:7]), j(L[3:6]), j(L), j(L[:8]), "zq#7end", "--zq#7end", "q#7end", "7end",
            "zq#7end~", "kw=77", "kw=1x", "kw=", j([L[7], L[8], "kw=7"]), j([L[7], "kw=7"]), j([L[7], L[8], "zq#7end"]), j([L[7], "zq#7end"]), j(L[:4] + ["kw=12"]), "Q", "QQQ", "QxQ", "xQ",
            j([L[7], L[7], L[8], L[8], L[7]]), j(L + L), "abc7", "abc", j([L[0], TWIN, "zq#7end"])]
    vals += ["~" * p + v for p in (1, 2, 3) for v in (TWIN, j(L[:3]), "zq#7end", "kw=5")]
    reqs = keyed(rs, [v.encode() for v in vals])
    batch = RequestBatch.from_requests(reqs)
    return Case("E", rs, [("E", batch)], dict(n=batch.n), sample=sample_for(rs, 2, [v for v in vals if v]))


def assert_e_coverage(m, batch, cold):
    """cold: the deciding rows are cold (the small budget) -- else every row is hot"""
    cov = coverage(m, batch)
    tier = COLD if cold else EMIT
    assert m.m["start_emit"] and cov.get("start emit") == batch.n, "the start state emits no atom"
    assert cov.get(("emit", tier, "list")) and (cold or cov.get(("emit", tier, "single"))), f"no {tier} row reports a single atom and a list"
    assert cov.get(("end atoms", tier if cold else PLAIN, 1)) or cov.get(("end atoms", tier, 1)), "a single END atom"
    assert cov.get(("end atoms", tier if cold else PLAIN, 2)) or cov.get(("end atoms", tier, 2)), "an END list of two"
    assert cov.get("atom twice") and cov.get("end atom, record full") and cov.get("end list, record full")
    got = {k[1] for k in cov if k[0] == "atoms"}
    assert got >= {1, 2, 3, 4, 5, 10}, sorted(got)
    if cold:
        assert m.n_hot < m.n_states
    else:
        assert m.n_hot == m.n_states
    return cov


LU2, LU3, LU4, LL2 = "É", "Ḁ", "\U0001d400", "é"  # \p{Lu} in two, three and four bytes; a lower-case letter


@functools.lru_cache(maxsize=None)
def case_u():
    """U. scalar mode: sequences whose lead byte sits at bytes 13 - 15 of a chunk (the continuation in the next chunk, for the chunks
    inside an iteration of CH = 2 and 4 and for its last), truncated sequences at the field's and at the arena's end in front of the
    byte that would complete them, a stray continuation byte at field byte 0 behind a field that ends in a lead byte, overlong forms"""
    rs = set_u()
    vals = []
    for at in (13, 14, 15, 29, 30, 31, 61, 62, 63):
        for ch in (LU2, LU3, LU4, LL2):
            vals.append(b"~" * (at - 3) + b"Uni" + ch.encode() + b"7code")          # the lead byte is field byte `at`
            vals.append(b"~" * (at - 3) + b"neg" + ch.encode() + b"end")
            vals.append(b"~" * (at - 1) + b"x" + ch.encode() + b"y")
    vals += [b"Uni" + LU2.encode() + b"7code", b"neg.end", b"negxend", b"x~y", b"xy", b"abc\xce\xb1", b"abc\xce", "é=1".encode(), "~€uro".encode(), "€ur".encode()]
    vals += [b"Uni\xc0\x817code", b"neg\xe0\x80\xafend", b"neg\xc0\xafend", b"x\xc1\xbfy", b"x\xf4\x90\x80\x80y", b"x\xed\xa0\x80y"]  # overlong, beyond U+10FFFF, a surrogate
    reqs = keyed(rs, vals)
    # a truncated sequence as the field's last byte, the next field begins with the byte that would complete it -- a stray continuation at its byte 0
    for lead, rest in ((b"\xc3", b"\x89"), (b"\xe1\xb8", b"\x80"), (b"\xf0\x9d", b"\x90\x80"), (b"\xe1", b"\xb8\x80")):
        reqs += [rs.request(b"~~Uni" + lead, rs.k_lu), rs.request(rest + b"7code", rs.k_lu), rs.request(b"x" + lead, rs.k_dot), rs.request(rest + b"y", rs.k_dot),
                 rs.request(b"neg" + lead, rs.k_neg), rs.request(rest + b"end", rs.k_neg)]
    reqs.append(rs.request(b"~" * 13 + b"x\xc3", rs.k_dot))  # the arena's last byte is a lead byte: the slack behind it holds its continuation and a y
    batch = RequestBatch.from_requests(reqs)
    end = int(batch.offsets[URL][-1])
    batch.data[URL][end:end + 2] = (0x89, ord("y"))
    lone = [rs.request(b"~" * 20 + b"Uni", rs.k_lu) for _ in range(64)]
    lone[37] = rs.request(b"~" * 10 + b"Uni" + LU2.encode() + b"7code", rs.k_lu)
    lone_batch = RequestBatch.from_requests(lone)
    _, per, sh = shares(64)
    (w,) = [(a, b) for a, b in sh if a <= 37 < b]
    assert per == 4 and all(max(lone_batch.field_bytes(URL, i)) < 0x80 for i in range(*w) if i != 37), "the wave of request 37 holds another byte beyond ASCII"
    return Case("U", rs, [("U", batch), ("U lone", lone_batch)], dict(n=batch.n), sample=sample_for(rs, 2, [v for v in vals[::5]]))


def assert_u_coverage(m, batch):
    assert m.m["scalar_mode"] == 1, "set U: the url pass is not in scalar mode"
    leads, trunc, stray = set(), 0, 0
    for i in range(batch.n):
        d = batch.field_bytes(URL, i)
        for jj, b in enumerate(d):
            if b >= 0xC0:
                ln = 4 if b >= 0xF0 else 3 if b >= 0xE0 else 2
                leads.add((jj % 16, ln))
                trunc += jj + ln > len(d)
        stray += bool(d) and 0x80 <= d[0] < 0xC0
    assert leads >= {(k, ln) for k in (13, 14, 15) for ln in (2, 3, 4)}, sorted(leads)
    assert trunc >= 4 and stray >= 4 and batch.field_bytes(URL, batch.n - 1)[-1] >= 0xC0


@functools.lru_cache(maxsize=None)
def case_x():
    """X. more than 127 byte classes: W's lengths of CH = 1 over set X, and the long literals themselves with their near misses"""
    rs = set_x()
    w = case_w(1, "X")
    m = rs.model("as built")
    assert m.n_classes > 127, f"set X has {m.n_classes} byte classes: the class table is not the wide one"
    vals = []
    for p in rs.preds[:8]:
        lit = p[p.index('("') + 2:p.rindex('")')]
        vals += [lit.encode(), b"~" + lit.encode() + b"~", lit.encode()[:-1] + b"~", lit.encode()[1:], b"~~~" + lit.encode()]
    batch = RequestBatch.from_requests(keyed(rs, vals))
    return Case("X", rs, w.batches + [("X literals", batch)], dict(n_classes=m.n_classes, **w.measured), sample=w.sample)


@functools.lru_cache(maxsize=None)
def case_g():
    """G. the gate feed: the url's plain pass owns the factors of six gap passes and enqueues from its finished records -- records of one
    atom, of two, overflowed ones (the need = 1 path), and records whose atoms gate nothing"""
    rs = set_g()
    L, gaps = rs.lits, rs.gaps
    vals = []
    for j, (a, b) in enumerate(gaps):
        a2, b2 = gaps[(j + 1) % 6]
        a3, _ = gaps[(j + 2) % 6]
        vals += [a + "--" + b, a + b, a + "x" * GAP_MAX + b, a + "x" * (GAP_MAX + 1) + b, a[:-1] + "--" + b, b + "--" + a, a, a + "~" + a2 + "--" + b2, a + "~" + a2 + "~" + a3 + "--" + b,
                 a + "~" + L[12] + "~" + L[13] + "--" + b, L[12] + "~" + L[13] + "~" + L[14] + "~" + a + "-" + b, L[12] + "~" + a + "--" + b[:-1]]
    vals += [L[12], L[12] + "~" + L[13], L[12] + "~" + L[13] + "~" + L[14], "~~~~", "", "abc7", L[12] + "Z"]
    reqs = keyed(rs, [v.encode() for v in vals]) * 3
    batch = RequestBatch.from_requests(reqs)
    return Case("G", rs, [("G", batch)], dict(n=batch.n), sample=sample_for(rs, 1, vals))


def assert_g_coverage(rs, leg, batch, sample=None):
    """from the plan: the url's plain pass owns factors, six gated gap passes hang on it; from the walks: records of 1, 2 and 3 or more
    atoms that gate a pass, records of 1, 2 and 3 or more atoms that gate nothing"""
    sc = rs.scan(leg, sample)
    k = rs.pass_of(sc)
    assert sc.owns_factors[k] == 1 and sc.roles[k]["gate"] < 0, "the url's plain pass owns no factor"
    gated = [q for q, g in enumerate(sc.groups) if g.get("filter_cols")]
    assert len(gated) == 6 and all(0 <= sc.roles[q]["gate"] < 32 and sc.roles[q]["share_owner"] < 0 for q in gated), "six gap passes with lists of their own"
    assert sc.launches[1] == [6]
    m = rs.model(leg, sample)
    base = sc.groups[k]["atom_base"]
    seen = set()
    for i in range(batch.n):
        atoms = m.walk(batch.field_bytes(URL, i))["atoms"]
        need = any(int(sc.colmask[base + a]) for a in atoms)
        seen.add((min(len(atoms), 3), need))
    assert seen >= {(1, True), (2, True), (3, True), (0, False), (1, False), (2, False), (3, False)}, sorted(seen)
    return sorted(seen)


@functools.lru_cache(maxsize=None)
def case_v():
    """V. views: the field passes and a header pass in one batch (records at rec + gi * n), each pass with requests of its own that match;
    two different batches in turn; the device suite also sends a view whose offsets begin above zero and the device-resident entry.
    Under PWAF_OPT_NO_PREFILTER scan_kernel walks host, url, path, user_agent and the header column: the method pass walks the identity
    list (lscan_kernel) whatever the sample says, because tune_host takes mean lengths only when it rebuilds prefilters. The natural leg
    tuned on this case's sample (methods of 14 bytes) makes the method pass a scan_kernel pass too."""
    rs = set_m()

    def build(seed):
        rng = random.Random(seed)
        reqs = []
        for i in range(300):
            kind = (i + seed) % 8
            other = dict(host="long.host.example.org", user_agent="Mozilla/5.0 (X11; Linux)", method="PROPPATCH-LONG", headers={HEADER: "a-header-value-" + str(i)})
            if kind == 1:
                other["host"] = "www.evil.example"
            elif kind == 2:
                other["user_agent"] = "sqlmap/17 (x)"
            elif kind == 3:
                other["headers"] = {HEADER: "abc-zzqq-" + str(i)}
            elif kind == 4:
                other["method"] = "PQQQQQ"
            v = [rs.rx_hit, rs.lits[0], "~" * rng.randrange(40), "abc7", "x.php", ""][i % 6]
            reqs.append(rs.request(("~" * (i % 19) + v).encode() if v else b"", [rs.k_rx, 0, rs.k_z, rs.k_unf, 5, rs.k_empty][i % 6] if kind != 5 else rs.k_short, **other))
        return RequestBatch.from_requests(reqs)

    a, b = build(0), build(3)
    sample = sample_of("V", RequestBatch.from_requests([rs.request(b"~" * 30 + rs.rx_hit.encode(), i % 5, host="long.host.example.org", path="/a/long/path/here", method="PROPPATCH-LONG",
                                                          user_agent="Mozilla/5.0 (X11; Linux)", headers={HEADER: "a-header-value-0"}) for i in range(64)]))
    return Case("V", rs, [("V first", a), ("V second", b)], dict(n=a.n), turns=2, sample=sample)


CASES = {"W1": lambda: case_w(1), "W2": lambda: case_w(2), "W4": lambda: case_w(4), "B": case_b, "B runs": case_b_runs, "B long": case_b_long, "T": case_t, "E": case_e, "U": case_u,
         "X": case_x, "G": case_g, "V": case_v}
