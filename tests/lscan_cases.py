"""Shared builders of the list-scan edge suites (tests/test_lscan_edges_cpu.py, tests/test_gpu_lscan_edges.py); no GPU import.

lscan_kernel (csrc/scan.hip) walks every list-driven DFA pass: the R-tier walks behind the confirm tier, the whole-pass dense
alternative, the candidate lists of a PWAF_OPT_NO_CONFIRM engine, the gap passes and the identity passes. A state it reads is a row staged
in LDS (state < n_hot), an 8-byte delta record over a base row (the next n_delta states) or a row of the L2-resident flat table. Here:

  * FlatModel: a plain reading of the flat image pwaf_program_flat_image returns (the table exactly as an engine uploads it). walk()
    takes one field byte by byte from state 0 and says what a correct walk visits: per step the tier of the state it leaves from and
    the step's position in its group of four, the atoms emitted and where their EMIT cell is read from, the end-of-field atoms, the
    STAY reads that pad the last group, whether the two-slot record overflows. It restates neither of the kernel's two loops.
  * the descriptors come from pwaf_program_list_scans (the plan the engine builds its launches from): which table every descriptor
    walks and the (n_hot, n_delta) it stages. Nothing here assumes a shape: every builder asserts what it was written for.
  * field strings are found by breadth-first search over the image: the shortest byte string that reaches a target state, a filler in
    front that keeps the walk in state 0 and places the step at a chosen group position, a suffix that completes a rule.
  * which requests a descriptor walks is decided by table_walker.Tables (the prefilter and the confirm tier through the program's
    hooks), one field at a time.

The EXPECTED verdicts never come from the model: pyoracle.Oracle gives them, as everywhere else."""
import functools
import random
import struct

import numpy as np

import confirm_cases as CC
import helpers as H
import table_walker
from oracle import pyoracle
from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.engine import CompiledProgram

B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
HOT, EX1, EX2, BASE, STAY, COLD = "hot", "rec-ex1", "rec-ex2", "rec-base", "rec-stay", "cold"
TIERS = (HOT, EX1, EX2, BASE, COLD)
N_P = 4096  # the batch size of the list-length cases (lscan_kernel: a candidate list of n / 8 or more entries is walked by lscan_async)
LEGS = {"as built": 0, "no confirm tier": _abi.OPT_NO_CONFIRM, "no dense switch": _abi.OPT_NO_DENSE_SWITCH, "rule hits": _abi.OPT_RULE_HITS}


# ---------------------------------------------------------------------------------------------------------
# the model of one list walk
# ---------------------------------------------------------------------------------------------------------
class FlatModel:
    """The flat image of (pass, tier) as the hook returns it. Cells: kernels.h (ListScanArgs) / scanplan.h (FlatImage)."""

    def __init__(self, prog, gi, tier):
        sec = {t: pl for t, _, pl in table_walker.parse_dump(prog.flat_image(gi, tier))}
        for k, v in zip(_abi.FLAT_SHAPE_FIELDS, struct.unpack("<7I", sec["FSHP"])):
            setattr(self, k, v)
        S, C = self.n_states, self.n_classes
        self.stride = C + 3
        self.flat = np.frombuffer(sec["FFLT"], dtype="<u2").astype(np.int64).reshape(S, self.stride)
        self.delta = [int(x) for x in np.frombuffer(sec["FDLT"], dtype="<u8")]
        self.cls = sec["FCLS"]
        assert len(self.cls) >= 272 and len(self.delta) == max(1, self.n_delta)
        self.um = bytes([self.ill_class]) + b"\0" * 7 + self.cls[272:] if self.scalar_mode else None  # (table_walker.scalar_class reads the dump's GUMP layout)
        self.emit_off, self.emit_list = np.frombuffer(sec["FEMO"], dtype="<u4"), np.frombuffer(sec["FEML"], dtype="<u2")
        self.end_off, self.end_list = np.frombuffer(sec["FENO"], dtype="<u4"), np.frombuffer(sec["FENL"], dtype="<u2")
        assert len(self.emit_off) == S + 1 == len(self.end_off)
        self.next = self.flat[:, :C] & 0x7FFF
        self.flag = (self.flat[:, :C] & 0x8000) != 0

    # -- classes --
    def classes(self, data):
        """the class of every byte: scalar mode reads a lead byte as the class of the scalar value it begins; a continuation byte of a
        well-formed sequence keeps its byte class (a class whose every cell is the state itself), a stray one is ill-formed"""
        out = []
        for j, b in enumerate(data):
            c = self.cls[b]
            if self.um is not None and b >= 0xC0:
                c = table_walker.scalar_class(self.um, data, j)
            elif self.um is not None and b >= 0x80 and not table_walker.cont_covered(data, j):
                c = self.ill_class
            out.append(c)
        return out

    # -- residency --
    def record(self, q, n_hot):
        rec = self.delta[q - n_hot]
        return rec & 0xFFFF, (rec >> 16) & 0xFF, (rec >> 24) & 0xFF, (rec >> 32) & 0xFFFF, rec >> 48

    def label(self, q, c, n_hot, n_delta):
        if q < n_hot:
            return HOT
        if q - n_hot < n_delta:
            _, c1, c2, _, _ = self.record(q, n_hot)
            return EX1 if c == c1 else EX2 if c == c2 else BASE
        return COLD

    def tier(self, q, n_hot, n_delta):
        return HOT if q < n_hot else "rec" if q - n_hot < n_delta else COLD

    def cell(self, q, c, n_hot, n_delta):
        """the cell a resident walk reads: a record state answers from its record and its base row; it must be the state's own row's"""
        own = int(self.flat[q, c])
        if n_hot <= q < n_hot + n_delta:
            base, c1, c2, t1, t2 = self.record(q, n_hot)
            assert base < n_hot, "a record's base row is staged"
            got = t1 if c == c1 else t2 if c == c2 else int(self.flat[base, c])
            assert got == own, f"state {q}, class {c}: the record gives {got:#x}, the row {own:#x}"
        return own

    def exceptions(self, q, n_hot):
        base = self.record(q, n_hot)[0]
        return int((self.flat[q, :self.n_classes] != self.flat[base, :self.n_classes]).sum())

    def emits(self, q):
        return [int(a) for a in self.emit_list[self.emit_off[q]:self.emit_off[q + 1]]]

    def ends(self, q):
        return [int(a) for a in self.end_list[self.end_off[q]:self.end_off[q + 1]]]

    # -- the walk --
    def walk(self, data, n_hot, n_delta):
        """-> dict: steps [(index, position in its group of four, state left, label, state entered)], emits [(index, state entered, atoms,
        where the EMIT cell is read from: HOT row / 'flat', 'single' | 'list')], the end state and its atoms, the STAY reads that pad the
        last group [(position, label)], the distinct atoms in order"""
        q, steps, emits, atoms = 0, [], [], []
        if self.emits(0):
            emits.append((-1, 0, self.emits(0), "start", "list"))
            atoms += self.emits(0)
        for j, c in enumerate(self.classes(data)):
            lab = self.label(q, c, n_hot, n_delta)
            v = self.cell(q, c, n_hot, n_delta)
            t = v & 0x7FFF
            assert t < self.n_states
            if v & 0x8000:
                code = int(self.flat[t, self.n_classes])
                lst = self.emits(t)
                assert lst and (code == (0x8000 | lst[0]) if len(lst) == 1 and lst[0] < 0x7FFF else code == 1), "the EMIT cell of an emitting state"
                emits.append((j, t, lst, HOT if t < n_hot else "flat", "single" if code & 0x8000 else "list"))
                atoms += lst
            steps.append((j, j % 4, q, lab, t))
            q = t
        end_tier = self.tier(q, n_hot, n_delta)
        stays = [(p, STAY if end_tier == "rec" else end_tier) for p in range(len(data) % 4, 4)] if len(data) % 4 else []
        assert int(self.flat[q, self.n_classes + 1]) == q, "the STAY cell"
        end_atoms = self.ends(q)
        assert int(self.flat[q, self.n_classes + 2]) == (1 if end_atoms else 0), "the END cell"
        distinct = list(dict.fromkeys(atoms + end_atoms))
        return dict(steps=steps, emits=emits, end_state=q, end_tier=end_tier, end_atoms=end_atoms, stays=stays, atoms=distinct, n=len(data))

    def features(self, data, n_hot, n_delta):
        """what the walk of `data` exercises, as hashable keys (the coverage tables count them)"""
        w = self.walk(data, n_hot, n_delta)
        f = set()
        for j, p, q, lab, t in w["steps"]:
            f.add((lab, p))
            f.add(("state", q))
            if lab in (EX1, EX2, BASE) and self.exceptions(q, n_hot) < 2:
                f.add(("rec<2", lab))
        for j, p, q, lab, t in w["steps"]:
            if self.um is not None and data[j] >= 0xC0:
                f.add(("lead", lab, p))  # scalar mode: a lead byte read from a state of this tier, at this position of its group
                if j == len(data) - 1:
                    f.add(("truncated", lab))  # ... and a sequence cut off by the field's end
        for p, lab in w["stays"]:
            f.add(("stay", lab))
        if w["n"] % 4 and w["steps"] and w["steps"][-1][3] == COLD:
            f.add(("cold-tail", w["n"] % 4))  # a cold step in the field's last group, which has 1, 2 or 3 valid bytes
        groups = {}
        for j, p, q, lab, t in w["steps"]:
            groups.setdefault(j // 4, []).append(lab)
        for g, labs in groups.items():
            if COLD in labs and COLD in groups.get(g + 1, []):
                f.add("cold-cold")  # two consecutive cold groups
            if any(a == COLD and b == HOT for a, b in zip(labs, labs[1:])):
                f.add("cold-to-hot")  # back from a cold row to a hot one inside a group
        for j, t, lst, src, kind in w["emits"]:
            f.add(("emit", src, kind))
            if src != "start":
                f.add(("emit-state", self.tier(t, n_hot, n_delta)))
        seen = [a for _, _, lst, _, _ in w["emits"] for a in lst]
        if len(seen) != len(set(seen)):
            f.add("atom-twice")
        if w["end_atoms"]:
            f.add(("end", w["end_tier"]))
        f.add(("atoms", min(len(w["atoms"]), 4)))  # (3 and more: the record's two slots overflow into the pool)
        return f

    # -- strings --
    @functools.cached_property
    def reps(self):
        """one printable byte per class that has one (letters and digits first): the alphabet of the searches"""
        order = [ord(ch) for ch in "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-_.~=&%+#!/:;,@^*()[]{}<>|?$' "]
        reps = {}
        for b in order:
            reps.setdefault(self.cls[b], b)
        return reps  # class -> byte

    def bytes_of_class(self, c):
        return [b for b in range(0x20, 0x7F) if self.cls[b] == c and b not in (0x22, 0x5C)]

    def search(self, src=0, stop_at_emit=False):
        """breadth-first from state src over reps -> (dist, parent (state, byte)); stop_at_emit: -> the shortest bytes from src that end in
        a flagged cell (b"" when none is reachable... never the case for a state of a used pass)"""
        cl = np.array(sorted(self.reps), dtype=np.int64)
        by = [self.reps[int(c)] for c in cl]
        dist = np.full(self.n_states, -1, dtype=np.int64)
        par = {}
        dist[src] = 0
        frontier = np.array([src], dtype=np.int64)
        d = 0
        while len(frontier):
            if stop_at_emit:
                fl = self.flag[frontier][:, cl]
                if fl.any():
                    i, k = np.argwhere(fl)[0]
                    s, out = int(frontier[i]), [by[k]]
                    while s != src:
                        s, b = par[s]
                        out.append(b)
                    return bytes(reversed(out))
            nx = self.next[frontier][:, cl]
            d += 1
            new = []
            flat_t = nx.ravel()
            uniq, first = np.unique(flat_t, return_index=True)
            for t, at in zip(uniq.tolist(), first.tolist()):
                if dist[t] < 0:
                    dist[t] = d
                    par[t] = (int(frontier[at // len(cl)]), by[at % len(cl)])
                    new.append(t)
            frontier = np.array(new, dtype=np.int64)
        if stop_at_emit:
            return None
        return dist, par

    def path_to(self, s, par, src=0):
        out = []
        while s != src:
            s, b = par[s]
            out.append(b)
        return bytes(reversed(out))

    FILLER = ord("~")  # (no pattern of the suites holds it)

    @functools.cached_property
    def rest(self):
        """the state a walk is in after a filler byte: every further filler keeps it there and emits nothing"""
        c = self.cls[self.FILLER]
        r = int(self.next[0, c])
        assert int(self.flat[r, c]) == r and not self.flag[0, c], "a filler byte does not leave the walk at rest"
        return r

    def reachable_exceptions(self, d):
        """the (record state, slot) pairs a printable byte can take: the slot's class has such a byte and its cell is not the base row's"""
        out = []
        for q in range(d["n_hot"], d["n_hot"] + d["n_delta"]):
            base, c1, c2, _, _ = self.record(q, d["n_hot"])
            for slot, c in ((EX1, c1), (EX2, c2)):
                if self.bytes_of_class(c) and (slot == EX1 or c2 != c1):
                    out.append((q, slot))
        return out


# ---------------------------------------------------------------------------------------------------------
# rule sets and which requests a descriptor walks
# ---------------------------------------------------------------------------------------------------------
class Membership(table_walker.Tables):
    """table_walker's pass logic with a log of the DFA walks it takes: (pass, tier) per request"""

    def __init__(self, prog):
        super().__init__(prog)
        self.log = set()

    def scan_field(self, g, data, cols):
        for gi, x in enumerate(self.groups):
            if x is g or x.get("rtier") is g:
                self.log.add((gi, 0 if x is g else 1))
        return super().scan_field(g, data, cols)


class RuleSet:
    """preds[k]: predicate texts over ONE field. Verdict form `http_request.path == "/h<k>" && <predicate k>`: the request's path picks
    which predicate decides its verdict (as in confirm_cases); bare form for the hit-matrix leg. extra: rules on other fields, kept as they are."""

    def __init__(self, name, field, preds, extra=(), opts=None, verdict_form=True):
        self.name, self.field, self.field_id, self.opts = name, field, _abi.FIELD_NAMES.index(field), dict(opts or {})
        self.preds = list(preds)
        act = lambda k: [B] if k % 2 == 0 else [CAP]  # noqa: E731
        self.bare_rules = [(f"b{k}", p, act(k)) for k, p in enumerate(self.preds)] + list(extra)
        self.verdict_rules = [(f"h{k}", f'http_request.path == "/h{k}" && {p}', act(k)) for k, p in enumerate(self.preds)] + list(extra) if verdict_form else self.bare_rules
        self._programs, self._models = {}, {}

    def rules(self, flags=0):
        return self.bare_rules if flags & _abi.OPT_RULE_HITS else self.verdict_rules

    def program(self, flags=0):
        if flags not in self._programs:
            self._programs[flags] = CompiledProgram(self.rules(flags), {}, flags=flags, **self.opts)
        return self._programs[flags]

    def model(self, prog, gi, tier):
        key = (id(prog), gi, tier)
        if key not in self._models:
            self._models[key] = (prog, FlatModel(prog, gi, tier))
        return self._models[key][1]

    def request(self, value, k=0, **other):
        f = {"host": "h", "url": "/i", "path": f"/h{k}", "user_agent": "ua", "method": "GET"}
        f.update(other)
        f[self.field] = value
        return Request(**f)  # (bytes stay bytes: the ill-formed sequences of the scalar-mode cases must arrive as they are)


def descriptors_of(prog, field_id=None):
    """the hook's descriptors (with the field of their pass, from the dump)"""
    t = table_walker.Tables(prog.dump())
    ds = prog.list_scans()
    for d in ds:
        d["field"] = t.groups[d["pass"]]["field"]
    return [d for d in ds if field_id is None or d["field"] == field_id]


def walked_by(prog, batch, field_id, only=None):
    """-> per request the set of (pass, tier) DFA walks table_walker takes over the field's passes, and its verdict (only: the requests
    to walk; the others read an empty set and None)"""
    m = Membership(prog)
    off = batch.offsets[field_id]
    out, verdicts = [set() for _ in range(batch.n)], [None] * batch.n
    for i in (range(batch.n) if only is None else only):
        m.log = set()
        m.arena_offset = int(off[i]) % 16
        verdicts[i] = m.evaluate(batch, i)
        out[i] = {(gi, tr) for gi, tr in m.log if m.groups[gi]["field"] == field_id}
    return out, verdicts


class Coverage:
    """per descriptor: how many walked requests show each feature"""

    def __init__(self, rs, flags, batch, dense=False, prog=None, only=None):
        self.prog = prog if prog is not None else rs.program(flags)
        self.descs = descriptors_of(self.prog, rs.field_id)
        self.only = list(range(batch.n)) if only is None else list(only)
        self.walked, self.verdicts = walked_by(self.prog, batch, rs.field_id, only)
        self.rows = []
        for d in self.descs:
            if d["dense_mode"] == (2 if dense else 1):  # (the flag-density switch gives the untaken form no work)
                continue
            model = rs.model(self.prog, d["pass"], d["tier"])
            count = {}
            n_walked = 0
            for i in self.only:
                if d["dense_mode"] != 1 and (d["pass"], d["tier"]) not in self.walked[i]:
                    continue
                n_walked += 1
                for f in model.features(batch.field_bytes(rs.field_id, i), d["n_hot"], d["n_delta"]):
                    count[f] = count.get(f, 0) + 1
            self.rows.append((d, model, n_walked, count))

    def row(self, **want):
        found = [r for r in self.rows if all(r[0][k] == v for k, v in want.items())]
        assert len(found) == 1, (want, [r[0] for r in self.rows])
        return found[0]

    @staticmethod
    def summary(row):
        d, m, n_walked, count = row
        cold = m.n_states - d["n_hot"] - d["n_delta"]
        per = {lab: [count.get((lab, p), 0) for p in range(4)] for lab in TIERS}
        return dict(phase=d["phase"], **{"pass": d["pass"]}, tier=d["tier"], threads=d["threads"], hot_bytes=d["hot_bytes"], n_states=m.n_states, n_classes=m.n_classes,
                    n_hot=d["n_hot"], n_delta=d["n_delta"], cold=cold, dense_mode=d["dense_mode"], share_owner=d["share_owner"], walked=n_walked, steps=per,
                    stay={lab: count.get(("stay", lab), 0) for lab in (HOT, STAY, COLD)})


def assert_tiers_at_every_position(row, what):
    """every tier the descriptor has is left from at each of the four group positions; a tier it has not is asserted absent"""
    d, m, n_walked, count = row
    slots = {slot for _, slot in m.reachable_exceptions(d)}  # (a slot spent on a class no printable byte has -- the classes that stay, of scalar mode -- is never taken here)
    has = {HOT: True, EX1: EX1 in slots, EX2: EX2 in slots, BASE: d["n_delta"] > 0, COLD: d["n_hot"] + d["n_delta"] < m.n_states}
    for lab in TIERS:
        got = [count.get((lab, p), 0) for p in range(4)]
        if has[lab]:
            assert all(got), f"{what}: tier {lab} is not left from at every group position: {got}"
        else:
            assert not any(got), f"{what}: tier {lab} does not exist here, yet {got}"
    if d["n_delta"]:
        assert count.get(("stay", STAY), 0), f"{what}: no field ends in a record state (the STAY cell answered without a read)"


def emitting_tiers(d, m):
    """which tiers of the descriptor hold a state (reachable over printable bytes from rest) that emits when entered / when the field
    ends in it: the features ("emit-state", tier) and ("end", tier) a suite must then show, and must not show otherwise"""
    dist, _ = m.search(m.rest)
    out = {}
    for key, fn in (("emit-state", m.emits), ("end", m.ends)):
        for tier in (HOT, "rec", COLD):
            out[(key, tier)] = any(dist[s] > 0 and m.tier(s, d["n_hot"], d["n_delta"]) == tier and fn(s) for s in range(1, m.n_states))
    return out


def loops_of(d):
    """the loops of lscan_kernel a descriptor can take: lscan_async needs a list behind a prefilter of n / 8 entries or more; the dense
    alternative's list is the batch, so it takes nothing else; every other list can be short"""
    return {"async"} if d["dense_mode"] == 1 else {"lockstep", "async"} if d["behind_filter"] else {"lockstep"}


def combinations(d, m):
    """(tier, loop, threads, hot bytes) for every tier the descriptor stages or leaves cold, every loop it can take"""
    tiers = [HOT] + (["rec"] if d["n_delta"] else []) + ([COLD] if d["n_hot"] + d["n_delta"] < m.n_states else [])
    return {(t, lp, d["threads"], d["hot_bytes"]) for t in tiers for lp in loops_of(d)}


def boundary_states(d, m):
    """n_hot - 1, n_hot, n_hot + n_delta - 1, n_hot + n_delta, n_states - 1: as many as exist"""
    return sorted({s for s in (d["n_hot"] - 1, d["n_hot"], d["n_hot"] + d["n_delta"] - 1, d["n_hot"] + d["n_delta"], m.n_states - 1) if 0 <= s < m.n_states})


# ---------------------------------------------------------------------------------------------------------
# set M: literals, regexes and gap rules on the url
# ---------------------------------------------------------------------------------------------------------
ALPHA = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-_.=&%+"


def rand_lit(rng, n, alpha=ALPHA):
    return "".join(rng.choice(alpha) for _ in range(n))


RX_ALPHA = ALPHA.replace(".", "").replace("+", "")  # (the pieces of a regex: nothing its syntax reads)


M_SEED = 5
M_LITS, M_REGEX, M_GAPS = 24, 24, 6
TWIN = "Tw1nSuffix=x"  # two literals that end at the same byte: TWIN and TWIN[4:]


@functools.lru_cache(maxsize=None)
def set_m():
    rng = random.Random(M_SEED)
    f = "http_request.url"
    lits = [rand_lit(rng, 12) for _ in range(M_LITS)]
    rx = [(rand_lit(rng, 4, RX_ALPHA), rand_lit(rng, 3, RX_ALPHA), rand_lit(rng, 3, RX_ALPHA)) for _ in range(M_REGEX)]
    gaps = [(rand_lit(rng, 5, RX_ALPHA), rand_lit(rng, 5, RX_ALPHA)) for _ in range(M_GAPS)]
    preds = [f"{f}.contains({H.q(x)})" for x in lits]
    preds += [f"{f}.matches({H.q(a + '[0-9]{2,4}' + b + '[a-f]+' + c)})" for a, b, c in rx]
    preds += [f"{f}.matches({H.q(a + '.*' + b)})" for a, b in gaps]
    k_extra = len(preds)
    preds += [f"{f}.contains({H.q(TWIN)})", f"{f}.contains({H.q(TWIN[4:])})", f"{f}.ends_with({H.q('zq#7end')})", f"{f}.matches({H.q('kw=[0-9]+$')})",
              f"{f}.matches({H.q('Uni' + chr(92) + 'p{Lu}[0-9]code')})", f"{f}.contains({H.q('q#7')})"]
    # an atom emitted at the start state: a pattern that matches the empty string; on the method, whose pass walks the identity list
    extra = [("start", 'http_request.path == "/start" && http_request.method.matches("Q*")', [CAP])]
    rs = RuleSet("M", "url", preds, extra=extra)
    rs.lits, rs.rx, rs.gaps = lits, rx, gaps
    rs.k_lit, rs.k_rx, rs.k_gap, rs.k_twin, rs.k_ends, rs.k_dollar, rs.k_uni, rs.k_short = 0, M_LITS, M_LITS + M_REGEX, k_extra, k_extra + 2, k_extra + 3, k_extra + 4, k_extra + 5
    rs.rx_hit = lambda j, digits="12", hexes="a": rx[j][0] + digits + rx[j][1] + hexes + rx[j][2]  # noqa: E731
    rs.decoy = rs.rx_hit(M_REGEX - 1)  # a whole match of the last regex: its factor sends the request through the R-tier walk
    rs.k_decoy = rs.k_rx + M_REGEX - 1
    return rs


L_LITS = 150


@functools.lru_cache(maxsize=None)
def set_l():
    """set L: literals alone -- no scalar mode, so the delta records spend their slots on byte classes a request can hold (in set M every record
    spends both on the two classes that STAY, which only the bytes behind a lead byte have). The
    confirm tier decides every atom (as built nothing is walked but the dense alternative); PWAF_OPT_NO_CONFIRM walks the full table."""
    rng = random.Random(M_SEED + 1)
    lits = [rand_lit(rng, 12) for _ in range(L_LITS - 40)]
    lits += [x[:10] + rand_lit(rng, 2) for x in lits[:40]]  # siblings that share ten bytes: the state at the fork differs from its base row in two cells
    rs = RuleSet("L", "url", [f"http_request.url.contains({H.q(x)})" for x in lits])
    rs.lits = lits
    rs.decoy = lits[-1]
    rs.k_decoy = L_LITS - 1
    return rs


@functools.lru_cache(maxsize=None)
def l_descriptors():
    rs = set_l()
    nc = _abi.OPT_NO_CONFIRM
    d, m = primary(rs, nc, phase=0, tier=0, behind_filter=1, n_delta_positive=True)
    assert not m.scalar_mode and (d["threads"], d["hot_bytes"]) == (1024, 144 * 1024) and (d["n_hot"], d["n_delta"]) == (m.n_full, m.n_delta)
    slots = {slot for _, slot in m.reachable_exceptions(d)}
    assert slots == {EX1, EX2}, "no record whose exception classes a printable byte has"
    out = {"full, no confirm tier": (nc, d, m)}
    d, m = primary(rs, 0, phase=0, tier=0, dense_mode=1, n_delta_positive=False)
    assert d["hot_bytes"] == 48 * 1024 and d["n_hot"] < m.n_states and [x for x in descriptors_of(rs.program(0), rs.field_id) if x["dense_mode"] != 1] == [], "as built the confirm tier decides every atom of set L"
    out["dense alternative"] = (0, d, m)
    return rs, out


def primary(rs, flags, n_delta_positive=None, **want):
    """the ONE descriptor of the set's field with these properties -> (descriptor, model)"""
    prog = rs.program(flags)
    found = [d for d in descriptors_of(prog, rs.field_id) if all(d[k] == v for k, v in want.items()) and n_delta_positive in (None, d["n_delta"] > 0)]
    assert len(found) == 1, (rs.name, flags, want, found)
    return found[0], rs.model(prog, found[0]["pass"], found[0]["tier"])


@functools.lru_cache(maxsize=None)
def m_descriptors():
    """the descriptors set M was written for, each asserted to have the shape its cases need"""
    rs = set_m()
    out = {}
    # as built: every filtered pass confirms, so phase 0 launches at 48 KiB; the R tier (built for 144 KiB) loses its records and keeps 48 KiB of rows
    d, m = primary(rs, 0, phase=0, tier=1, dense_mode=2)
    assert (d["threads"], d["hot_bytes"]) == (512, 48 * 1024) and m.lds_bytes == 144 * 1024 and d["merge_rec"] == 1 and d["behind_filter"] == 1
    assert d["n_delta"] == 0 and d["n_hot"] == min(m.n_full if m.n_delta else m.n_states, (48 * 1024 - 48) // (2 * m.stride)) < m.n_states, "the R tier fits 48 KiB: no cold row"
    out["R as built"] = (0, d, m)
    d, m = primary(rs, 0, phase=0, tier=0, dense_mode=1)
    assert d["hot_bytes"] == 48 * 1024 and d["n_delta"] == 0 and d["n_hot"] < m.n_states and d["merge_rec"] == 0
    out["dense alternative"] = (0, d, m)
    d, m = primary(rs, 0, phase=1, dense_mode=3)
    assert d["share_owner"] == out["R as built"][1]["pass"] and d["hot_bytes"] == 48 * 1024 and d["n_hot"] + d["n_delta"] < m.n_states
    out["sharing gap pass"] = (0, d, m)
    # without the confirm tier: the full table behind the candidate list, the wide shape, records in use
    nc = _abi.OPT_NO_CONFIRM
    d, m = primary(rs, nc, phase=0, tier=0, **{"pass": out["R as built"][1]["pass"]})
    assert (d["threads"], d["hot_bytes"]) == (1024, 144 * 1024) and (d["n_hot"], d["n_delta"]) == (m.n_full, m.n_delta) and d["n_delta"] > 0 and d["dense_mode"] == 0
    assert d["n_hot"] + d["n_delta"] < m.n_states, "nothing is cold at 144 KiB"
    out["full, no confirm tier"] = (nc, d, m)
    return rs, out


def target_strings(m, d, rng, extra=6):
    """for the boundary states and a few more of every tier: the shortest bytes that reach the state, then each kind of step out of
    it -- the byte of exception 1, of exception 2, a byte answered from the base row (record states), the byte towards the nearest
    emitting cell -- and the field's end; each continued to the nearest emitting cell. -> [(bytes up to and including the step, the
    rest)], and the targets that cannot be reached over printable bytes"""
    r = m.rest
    dist, par = m.search(r)
    targets = list(boundary_states(d, m))
    exc = m.reachable_exceptions(d)
    targets += [q for q, _ in exc if dist[q] > 0][:8]
    tiers = {HOT: range(1, d["n_hot"]), "rec": range(d["n_hot"], d["n_hot"] + d["n_delta"]), COLD: range(d["n_hot"] + d["n_delta"], m.n_states)}
    for name, rg in tiers.items():
        pool = [s for s in rg if dist[s] > 0]
        targets += rng.sample(pool, min(extra, len(pool)))
        if name == "rec":  # a record with fewer than two exceptions
            few = [s for s in pool if m.exceptions(s, d["n_hot"]) < 2]
            targets += few[:2]
        targets += [s for s in pool if m.emits(s)][:2] + [s for s in pool if m.ends(s)][:2]  # what entering / ending in a state of the tier emits
    out, unreached = [], []
    for s in dict.fromkeys(targets):
        if dist[s] < 0:
            unreached.append(s)
            continue
        head = m.path_to(s, par, r)
        nexts = []
        to_emit = m.search(s, stop_at_emit=True)
        if to_emit:
            nexts.append(to_emit[:1])
        if d["n_hot"] <= s < d["n_hot"] + d["n_delta"]:
            _, c1, c2, _, _ = m.record(s, d["n_hot"])
            for c in (c1, c2):
                nexts += [bytes([b]) for b in m.bytes_of_class(c)[:1]]
            other = [c for c in sorted(m.reps) if c not in (c1, c2)]
            nexts += [bytes([m.reps[c]]) for c in other[:2]]
        out.append((head, b""))  # the field ends in the state
        if m.um is not None and s >= d["n_hot"] + d["n_delta"]:  # scalar mode, a cold state: a lead byte, and a sequence the field's end cuts off
            out.append((head + "\u00c9".encode("utf-8"), b"7code"))
            out.append((head + b"\xc3", b""))
        for nb in dict.fromkeys(nexts):
            t = int(m.next[s, m.cls[nb[0]]])
            rest = m.search(t, stop_at_emit=True) or b""
            out.append((head + nb, rest))
    return out, unreached


def at_position(prefix, body, split, p):
    """one to four filler bytes between prefix and body (the walk is at rest in front of the body) so that body[split - 1], the step
    out of the target state -- or, with split == len(body), the field's end -- is byte p (mod 4) of the field"""
    k = (p - (len(prefix) + split - 1)) % 4 or 4
    return prefix + bytes([FlatModel.FILLER]) * k + body


DESCRIPTORS = {"M": lambda: m_descriptors(), "L": lambda: l_descriptors()}


@functools.lru_cache(maxsize=None)
def case_t(set_name="M"):
    """T. tier boundaries, E. emits: for each descriptor of the set the strings of target_strings, each placed so that the step out of its
    target state is byte 0, 1, 2 and 3 of a group, alone and behind a decoy (a whole match of another regex and a byte that takes every
    state back to 0), which puts the request on the walk list whatever the string holds. Observed under the key of the rule the string
    completes (the oracle says which), the decoy's own, and another's."""
    rs, descs = DESCRIPTORS[set_name]()
    rng = random.Random(11)
    oracle = pyoracle.Oracle(rs.bare_rules, {})
    values, unreached = [], {}
    for name, (flags, d, m) in descs.items():
        strings, unreached[name] = target_strings(m, d, rng)
        for prefix in (b"", rs.decoy.encode()):
            assert m.walk(prefix + b"~", d["n_hot"], d["n_delta"])["end_state"] == m.rest, f"{name}: a filler behind the decoy does not leave the walk at rest"
            for head, rest in strings:
                for p in range(4):
                    values.append(at_position(prefix, head + rest, len(head), p))
                    if rest:  # the near miss: the last byte wrong
                        values.append(at_position(prefix, head + rest[:-1] + b"!", len(head), p))
    values += emit_values(rs) if set_name == "M" else []
    values = list(dict.fromkeys(values))
    # the key every value is observed under: the first bare rule it satisfies other than the decoy's (else the decoy's)
    probe = RequestBatch.from_requests([rs.request(v) for v in values])
    hit, _ = H.oracle_matrix(oracle, probe)
    reqs = []
    k_decoy = rs.k_decoy
    for i, v in enumerate(values):
        ks = [k for k in np.nonzero(hit[:len(rs.preds), i])[0].tolist() if k != k_decoy]
        k = ks[0] if ks else (k_decoy if i % 3 else (i * 7) % len(rs.preds))
        reqs.append(rs.request(v, k, method="QQ" if i % 5 == 0 else "GET", **(dict(path="/start") if i % 97 == 0 and set_name == "M" else {})))
    batch = RequestBatch.from_requests(reqs)
    name = "T" if set_name == "M" else "T" + set_name
    batches = [(name, batch)]
    if set_name == "L":  # (nearly every request of TL is a candidate: lscan_async; among eight times as many on no list: the lockstep loop)
        batches.append((name + " padded", RequestBatch.from_requests(reqs + fillers(rs, 8 * len(reqs)))))
    return CC.Case(name, rs, batches, dict(unreached=unreached, n=batch.n))


def emit_values(rs):
    """E. two literals that end at the same byte (an emit LIST), the same atom twice in one field, three and four distinct atoms (the
    record overflows into the pool), end-of-field atoms (ends_with, $), the scalar-mode rule"""
    a, b, c, d = rs.lits[0], rs.lits[1], rs.lits[2], rs.lits[3]
    decoy = rs.decoy
    vals = [TWIN, "x" + TWIN + "y", decoy + "~" + TWIN, a + "~" + a, decoy + "~" + decoy, rs.rx_hit(0) + "~" + rs.rx_hit(0, "345", "fe"),
            a + "~" + b + "~" + c, a + "~" + b + "~" + c + "~" + d, decoy + "~" + a + "~" + b, rs.rx_hit(0) + "~" + rs.rx_hit(1) + "~" + rs.rx_hit(2),
            rs.rx_hit(0) + "~" + rs.rx_hit(1) + "~" + rs.rx_hit(2) + "~" + rs.rx_hit(3), "zq#7end", "--zq#7end", decoy + "~zq#7end", "zq#7end~", "kw=77", decoy + "~kw=1",
            "kw=1x", rs.gaps[0][0] + "--" + rs.gaps[0][1], rs.gaps[0][0] + "--" + rs.gaps[1][1], rs.gaps[0][0] + rs.gaps[1][0] + "~" + rs.gaps[1][1] + rs.gaps[0][1],
            "".join(x for x, _ in rs.gaps) + "~" + "".join(y for _, y in rs.gaps), rs.gaps[2][0] + "~zq#7end", "q#7", "~q#7", "q#"]
    # scalar mode: \p{Lu} with a lead byte at each group position, and a truncated sequence as the field's last byte
    for p in range(4):
        pad = "~" * ((p - 3) % 4)  # "Uni" is three bytes: the lead byte is byte 3 + len(pad)
        vals += [pad + "UniÉ" + "7code", pad + "UniЖ" + "7code", pad + "Unié" + "7code", decoy + "~" + pad + "UniÉ" + "7code"]
    out = [v.encode("utf-8") for v in vals]
    out += [b"Uni\xc3", decoy.encode() + b"~Uni\xc3", b"Uni\xe2\x82", b"Uni\xc9" + b"7code"[:0] + b"\xc3"]
    return out


@functools.lru_cache(maxsize=None)
def case_w():
    """W. windows and alignment: fields of 0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49 bytes whose LAST byte decides (a literal of
    3 or 12 bytes, or a whole regex match, at the field's end behind bytes that keep the walk in state 0), and the same with the last
    byte wrong; each starting at every arena offset mod 16 (the requests in between have fields of 0 - 15 bytes); the batch's last
    request is one of them (the prefetch of the window behind it is clamped to the arena's byte 0)."""
    rs = set_m()
    reqs, cur = [], 0
    hits = [("q#7", rs.k_short), (rs.lits[5], rs.k_lit + 5), (rs.rx_hit(3), rs.k_rx + 3)]
    for o in range(16):
        for n in (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49):
            fit = [(h, k) for h, k in hits if len(h) <= n]
            for h, k in (fit[:1] + fit[-1:] if fit else [("", rs.k_short)]):
                for wrong in (True, False):
                    v = "~" * (n - len(h)) + (h[:-1] + "!" if wrong and h else h)
                    assert len(v) == n
                    gap = (o - cur) % 16  # a request of 0 - 15 bytes in between: the next one starts at offset o
                    reqs.append(rs.request("~" * gap, rs.k_short))
                    cur += gap
                    assert cur % 16 == o
                    reqs.append(rs.request(v, k))
                    cur += n
    batch = RequestBatch.from_requests(reqs)
    assert batch.field_bytes(rs.field_id, batch.n - 1) == b"~" * (49 - len(hits[2][0])) + hits[2][0].encode()
    return CC.Case("W", rs, [("W", batch)], dict(n=batch.n))


def candidates_by_model(rs, batch, flags):
    """the candidate list of the url pass of a PWAF_OPT_NO_CONFIRM engine, by confirm_cases' numpy model of filter_kernel over the whole
    arena: the requests with a byte in a flagged chunk"""
    prog = rs.program(flags)
    t = table_walker.Tables(prog.dump())
    (g,) = [g for g in t.groups if g["field"] == rs.field_id and "f_table" in g]
    sh = CC.PassShape(g, batch, rs.field_id)
    return [r for r in range(batch.n) if sh.chunks_of(r)], sh


P_LENGTHS = (0, 1, 63, 64, 65, 511, 512, 513)


@functools.lru_cache(maxsize=None)
def case_p(n_list):
    """P. one batch of 4 096 requests of which n_list hold a whole regex match (candidates of the url pass, walk requests behind the
    confirm tier) and the others a filler that flags nothing: both sides of `8 * n_l >= n` (512 of 4 096), which decides on the device
    between the lockstep loop and lscan_async for a list behind a prefilter. The candidates' strings are T's cold and record targets
    of the full table at equal depth, so that whole waves of lscan_async block in the same iteration."""
    rs, descs = m_descriptors()
    flags, d, m = descs["full, no confirm tier"]
    rng = random.Random(100 + n_list)
    dist, par = m.search(m.rest)
    depths = np.bincount(dist[d["n_hot"] + d["n_delta"]:][dist[d["n_hot"] + d["n_delta"]:] > 0])
    depth = int(np.argmax(depths))  # the depth most cold states lie at: the targets line up
    cold = [s for s in range(d["n_hot"] + d["n_delta"], m.n_states) if dist[s] == depth][:8]
    assert len(cold) >= 4, "fewer than four cold states at one depth"
    reqs = []
    at = set(rng.sample(range(N_P), n_list)) if n_list else set()
    for i in range(N_P):
        if i in at:
            s = cold[len(reqs) % len(cold)]
            j = i % M_REGEX
            v = rs.rx_hit(j, "123"[: 2 + i % 2], "abcdef"[: 1 + i % 5]).encode() + b"~" + m.path_to(s, par, m.rest) + (m.search(s, stop_at_emit=True) or b"")
            v = b"~" * 19 + v + b"~" * 19  # (a flagged chunk holds no byte of a neighbour, nor one within a window's reach of it: three bigrams back, a byte forward)
            reqs.append(rs.request(v, rs.k_rx + j if i % 4 else rs.k_lit))
        else:
            reqs.append(rs.request("/" + "~" * (i % 23), rs.k_rx + i % M_REGEX))
    batch = RequestBatch.from_requests(reqs)
    cands, sh = candidates_by_model(rs, batch, flags)
    assert cands == sorted(at), (n_list, len(cands))
    return CC.Case(f"P{n_list}", rs, [(f"P{n_list}", batch)], dict(n=batch.n, n_list=len(cands), long_list=8 * len(cands) >= batch.n, flagged_chunks=sh.pairs))


MI355X_CUS = 256  # (the CPU suite builds the wave cases for this device; the device suite for the one it runs on)


def entries_per_item(lists, n_waves):
    """lscan_plan_kernel restated as data (csrc/scan.hip): the list entries ONE WAVE takes of each list of a launch. lists: the
    lengths of the launch's lists in descriptor order; n_waves = compute units x workgroups per CU x threads / 64. A wave walks its
    entries one per lane: lane l of item `it` walks list entry (it - first) * epi + l, so a wave is FULL only from epi == 64 on."""
    room = n_waves - len(lists) if n_waves > len(lists) else 1
    per_wave = (sum(lists) + room - 1) // room
    out = []
    for n_l in lists:
        epi = 1
        while epi < 16 and epi < per_wave:
            epi <<= 1
        while epi < 64 and (n_l + epi - 1) // epi > n_waves:
            epi <<= 1
        out.append(epi)
    return out


WAVE_COUNTS = (1, 31, 32, 33, 64)


def case_p_waves(blocked, n_cus=MI355X_CUS):
    """P, the asynchronous leg with FULL waves. A wave of lscan_kernel takes `epi` consecutive entries of a list, one per lane, and
    lscan_plan_kernel only packs 64 into a wave when the list has more than 32 entries per wave of the launch (entries_per_item): for
    the 1024-thread launch of an engine without confirm tier that is more than 32 x 16 x compute units requests -- 131 072 on an
    MI355X, not a few thousand. So: a base batch of 64 requests, every one a candidate, of which the first `blocked` stand in a COLD
    state at byte 0 of the same group while the others are in hot rows there, tiled to the smallest n above that bound. The
    candidate list ascends (compact_kernel), so list entry li is request li and wave w holds requests 64 w .. 64 w + 63: in the
    iteration of that group exactly `blocked` of its 64 lanes read the sentinel -- below, at and above the 32 lanes from which the slow
    iteration is taken at once, and all 64 (nobody else can move). -> (case of the base batch, times to tile it)"""
    rs, descs = m_descriptors()
    flags, d, m = descs["full, no confirm tier"]
    dist, par = m.search(m.rest)
    cold = sorted((int(dist[s]), s) for s in range(d["n_hot"] + d["n_delta"], m.n_states) if dist[s] > 0)
    depth, s = cold[0]  # a cold state at the least depth: the walk to it meets no other
    k = 8 + (-depth) % 4  # the step out of it is byte 0 of a group, two groups or more into the field
    decoy = rs.decoy.encode()
    deep = b"~" * k + m.path_to(s, par, m.rest) + (m.search(s, stop_at_emit=True) or b"") + b"~" + decoy
    shallow = b"~" * (k + depth + 4) + decoy
    reqs = [rs.request(deep if i < blocked else shallow, rs.k_decoy if i % 2 else rs.k_lit + i % M_LITS) for i in range(64)]
    base = RequestBatch.from_requests(reqs)
    # the launch's waves and the entries a wave takes, from the hook's shape and the plan rule
    n_waves = n_cus * d["wg_per_cu"] * d["threads"] // 64
    times = 32 * n_waves // 64 + 1
    n = 64 * times
    launch = [x for x in descriptors_of(rs.program(flags)) if (x["phase"], x["launch"]) == (d["phase"], d["launch"])]
    at = [x["pass"] for x in launch].index(d["pass"])
    for other in (0, n):  # (whatever the launch's other list holds -- the User-Agent gate's pass -- between nothing and everything)
        lists = [n if x["pass"] == d["pass"] else other for x in launch]
        epi = entries_per_item(lists, n_waves)[at]
        assert epi == 64 and entries_per_item([v - 64 if q == at else v for q, v in enumerate(lists)], n_waves)[at] < 64, "the batch does not just fill the launch's waves"
    assert d["behind_filter"] == 1 and 8 * n >= n, "the list is not walked by lscan_async"
    # every request a candidate, by the numpy model of the filter over a few tiles (the arena is periodic)
    few = base.tile(8)
    cands, sh = candidates_by_model(rs, few, flags)
    assert len(cands) == few.n, len(cands)
    # the blocked lanes of a wave, by the model: who reads a cold row in the group of the deep walk's first cold step
    w = m.walk(deep, d["n_hot"], d["n_delta"])
    first_cold = min(j for j, p, q, lab, _ in w["steps"] if lab == COLD)
    assert first_cold == k + depth and first_cold % 4 == 0
    g0 = first_cold // 4
    in_group = []
    for i in range(64):
        steps = m.walk(base.field_bytes(rs.field_id, i), d["n_hot"], d["n_delta"])["steps"]
        assert len(steps) > 4 * g0 + 4, "a lane's field ends before the group"
        assert all(lab == HOT for _, _, _, lab, _ in steps[:4 * g0]), "a lane is parked before the group: the lanes are not in step"
        in_group.append(any(lab != HOT for _, _, _, lab, _ in steps[4 * g0:4 * g0 + 4]))
    assert sum(in_group) == blocked and in_group == [i < blocked for i in range(64)], in_group
    return CC.Case(f"P waves {blocked}", rs, [(f"P waves {blocked}", base)], dict(n=n, blocked=blocked, group=g0, epi=epi, n_waves=n_waves, times=times)), times


@functools.lru_cache(maxsize=None)
def case_s():
    """S. sharing and stale state: the gap pass of set M rides the R-tier walk list of the url pass through need masks. Requests that
    hold a factor of exactly one gap rule, of all of them and of none (a decoy alone: on the list, need bit clear); two batches of
    identical offsets sent in turn, four turns, in which every observed request holds other hits in the second batch than in the first."""
    rs, descs = m_descriptors()

    def build(second):
        reqs = []
        for i in range(600):
            j, kind = i % M_GAPS, (i // M_GAPS) % 6
            a, b = rs.gaps[j]
            a2, b2 = rs.gaps[(j + 1) % M_GAPS]
            first, then = [(a + "--" + b, a + "--" + b[:-1] + "!"), (rs.decoy + "~~~~", a2 + ".." + b2[:2]), (a + "~" + rs.decoy, rs.decoy + "~" + a[:-1] + "!"),
                           ("".join(x for x, _ in rs.gaps), "".join(y for _, y in rs.gaps)), (a + b2, a2 + b), (b + "--" + a, a + "--" + b)][kind]
            n = max(len(first), len(then))
            v = (then if second else first).ljust(n, "~")  # (identical offsets in both batches)
            reqs.append(rs.request(v, rs.k_gap + j if i % 3 else rs.k_rx + M_REGEX - 1))
        return RequestBatch.from_requests(reqs)

    b0, b1 = build(False), build(True)
    assert all((b0.offsets[f] == b1.offsets[f]).all() for f in range(5))
    return CC.Case("S", rs, [("S first", b0), ("S second", b1)], dict(n=b0.n), turns=4)


def fillers(rs, n, k=0):
    """n requests that flag nothing and are on no list: behind them a list of the batch is shorter than an eighth of it (the lockstep loop)"""
    return [rs.request("/" + "~" * (7 + i % 23), k) for i in range(n)]


def dense_case(name, rs, pieces, n_keys):
    """a batch whose url arena is one slab with more than half of its chunks flagged (every request a run of three of `pieces`, some
    with the last byte wrong): the url pass is walked WHOLE through its full table (dense_mode 1), its gap passes by need bit or list"""
    reqs, total, i = [], 0, 0
    while total < 120 * 1024:
        run = "~".join(pieces[(i + x) % len(pieces)] for x in range(3))
        v = run if i % 3 else run[:-1] + "!"
        reqs.append(rs.request(v, (i + (i % 2) * 2) % n_keys))
        total += len(v)
        i += 1
    batch = RequestBatch.from_requests(reqs)
    (d,) = [x for x in descriptors_of(rs.program(0), rs.field_id) if x["dense_mode"] == 1]
    t = table_walker.Tables(rs.program(0).dump())
    sh = CC.PassShape(t.groups[d["pass"]], batch, rs.field_id)
    assert sh.n_slabs == 1 and sh.pairs > sh.dense_thresh, f"{name}: {sh.pairs} flagged chunks against a threshold of {sh.dense_thresh}: the pass is not walked whole"
    return CC.Case(name, rs, [(name, batch)], dict(n=batch.n, flagged_chunks=sh.pairs, dense_thresh=sh.dense_thresh))


G_GAPS, G_WALKS = 6, 3


@functools.lru_cache(maxsize=None)
def set_g():
    """set G: six counted-gap rules and three regexes on the url, 64 KiB per table: every gap rule gets a gap pass of its own, and all six
    ride the walk list of the ONE filtered url pass through need bits 0 - 5 (one launch of six descriptors)"""
    gr, gt = H.kind_rules("gap", G_GAPS, seed=1)
    cr, ct = H.kind_rules("confirm_walk", G_WALKS, seed=2)
    rs = RuleSet("G", "url", [r[1] for r in gr + cr], opts=dict(max_table_bytes=65536))
    rs.gap_hit = [t[1][0] for t in gt]      # the two words of gap rule j, adjacent
    rs.gap_miss = [t[1][5] for t in gt]     # ... the first word cut by a byte
    rs.walk_hit = [t[1][0] for t in ct]
    for flags in (0, _abi.OPT_NO_CONFIRM, _abi.OPT_NO_DENSE_SWITCH, _abi.OPT_RULE_HITS):
        ds = descriptors_of(rs.program(flags), rs.field_id)
        gaps = [d for d in ds if d["phase"] == 1]
        owners = {d["share_owner"] for d in gaps}
        assert len(gaps) == G_GAPS and len(owners) == 1 and -1 not in owners and sorted(d["need_bit"] for d in gaps) == list(range(G_GAPS)), (flags, gaps)
        assert {(d["launch"], d["launch_count"]) for d in gaps} == {(0, G_GAPS)}, "the gap passes are not one launch"
    rs.gap_pass = {d["need_bit"]: d["pass"] for d in descriptors_of(rs.program(0), rs.field_id) if d["phase"] == 1}
    # These six passes are the halves of ONE chunk of gap rules cut down to the table budget, and the halves keep the chunk's factor
    # columns: a factor of any of the six rules sets all six need bits (asserted here). Set H is the one with disjoint factors.
    t = table_walker.Tables(rs.program(0).dump())
    cols = [tuple(t.groups[p]["filter_cols"]) for p in rs.gap_pass.values()]
    assert len(set(cols)) == 1 and len(cols[0]) == G_GAPS, cols
    return rs


def gap_walks(rs, batch, flags=0):
    """-> per request the need bits whose gap pass walks it, and whether it is on the owner's list at all (some DFA walk of the field)"""
    walked, _ = walked_by(rs.program(flags), batch, rs.field_id)
    of = {p: b for b, p in rs.gap_pass.items()}
    return [frozenset(of[gi] for gi, _ in w if gi in of) for w in walked], [bool(w) for w in walked]


@functools.lru_cache(maxsize=None)
def case_sg():
    """S over set G, an owner whose list serves SIX gap passes: requests that set the need bits of all of them (the words of one rule, of
    every rule) and of none (a regex match alone: on the owner's list, every bit clear) -- in THIS set no request sets exactly one
    (set_g; case SH does) --, near misses; two batches of identical offsets in turn, four turns, in which every request holds another rule's words in the
    second batch, or nothing at all: a gap pass's record of the first batch lies where the pass does not walk in the second, and its
    visited bitmap must hide it."""
    rs = set_g()

    def build(second):
        reqs = []
        for i in range(360):
            j, kind = i % G_GAPS, (i // G_GAPS) % 5
            j2 = (j + 1 + i // 30) % G_GAPS
            first, then = [(rs.gap_hit[j], rs.gap_hit[j2]), (rs.gap_hit[j], "~" * len(rs.gap_hit[j])), ("~".join(rs.gap_hit), "~".join(rs.gap_miss)),
                           (rs.walk_hit[j % G_WALKS], rs.gap_hit[j]), (rs.gap_miss[j], rs.gap_hit[j])][kind]
            n = max(len(first), len(then))
            reqs.append(rs.request((then if second else first).ljust(n, "~"), j if i % 4 else G_GAPS + j % G_WALKS))
        return reqs

    r0, r1 = build(False), build(True)
    pad = fillers(rs, 8 * len(r0))  # (the walk list is shorter than an eighth of the batch: the lockstep loop; "SG short" is the first batch alone: lscan_async)
    b0, b1, short = RequestBatch.from_requests(r0 + pad), RequestBatch.from_requests(r1 + pad), RequestBatch.from_requests(r0)
    assert all((b0.offsets[f] == b1.offsets[f]).all() for f in range(5))
    (g0, on0), (g1, on1) = gap_walks(rs, b0), gap_walks(rs, b1)
    assert 8 * sum(on0) < b0.n and 8 * sum(on1) < b1.n and 8 * sum(gap_walks(rs, short)[1]) >= short.n
    every = frozenset(range(G_GAPS))
    for g in (g0, g1):
        assert set(g) == {every, frozenset()} and sum(1 for x in g if x == every) >= 100, "every need bit, or none"
    assert sum(1 for x, on in zip(g0, on0) if on and not x) >= 30, "requests on the owner's list with no need bit"
    stale = [i for i in range(b0.n) if g0[i] and not g1[i]]
    assert len(stale) >= 60 and sum(1 for i in stale if not on1[i]) >= 30, "records of the first batch where the passes do not walk in the second"
    return CC.Case("SG", rs, [("SG first", b0), ("SG second", b1), ("SG short", short)], dict(n=b0.n, stale=len(stale), with_bits=sum(1 for x in g0 if x), listed_without=sum(1 for x, on in zip(g0, on0) if on and not x)), turns=4)


H_GAPS = 16


@functools.lru_cache(maxsize=None)
def set_h(with_regex=True):
    """set H: sixteen `url.matches("LLLLL.*LLLLL")`, four literals and (with_regex) four regexes, default options: the compiler cuts the gap
    rules into two chunks of eight, each a gap pass with the factor columns of ITS rules alone. With the regexes the url pass walks, and
    both gap passes ride its walk list through need bits 0 and 1; without them (set O) the owner's confirm tier never walks and each gap
    pass has a list of its own, fed by enqueues."""
    rng = random.Random(31)
    f = "http_request.url"
    gaps = [(rand_lit(rng, 5, RX_ALPHA), rand_lit(rng, 5, RX_ALPHA)) for _ in range(H_GAPS)]
    lits = [rand_lit(rng, 12) for _ in range(4)]
    rx = [(rand_lit(rng, 4, RX_ALPHA), rand_lit(rng, 3, RX_ALPHA)) for _ in range(4)]
    preds = [f"{f}.matches({H.q(a + '.*' + b)})" for a, b in gaps] + [f"{f}.contains({H.q(x)})" for x in lits]
    if with_regex:
        preds += [f"{f}.matches({H.q(a + '[0-9]{2,4}' + b)})" for a, b in rx]
    rs = RuleSet("H" if with_regex else "O", "url", preds)
    rs.gaps, rs.lits = gaps, lits
    rs.gap_hit = [a + "--" + b for a, b in gaps]
    rs.gap_miss = [a[:-1] + "!--" + b[:-1] + "!" for a, b in gaps]
    rs.walk_hit = [a + "123" + b for a, b in rx]
    rs.k_walk = H_GAPS + 4
    for flags in (0, _abi.OPT_NO_DENSE_SWITCH, _abi.OPT_RULE_HITS, _abi.OPT_NO_CONFIRM):
        prog = rs.program(flags)
        t = table_walker.Tables(prog.dump())
        gp = [d for d in descriptors_of(prog, rs.field_id) if d["phase"] == 1]
        assert len(gp) == 2 and {(d["launch"], d["launch_count"]) for d in gp} == {(0, 2)}, (flags, gp)
        cols = [set(t.groups[d["pass"]]["filter_cols"]) for d in gp]
        assert not cols[0] & cols[1] and len(cols[0]) == len(cols[1]) == H_GAPS // 2, "the two gap passes do not have factors of their own"
        shares = with_regex or bool(flags & _abi.OPT_NO_CONFIRM)  # (without a confirm tier the owner walks its candidate list: the gap passes share it)
        for d in gp:
            m = rs.model(prog, d["pass"], 0)
            assert (d["share_owner"] >= 0) == shares and (d["need_bit"] if shares else 0) == (gp.index(d) if shares else 0), (flags, d)
            assert d["n_delta"] > 0 and d["n_hot"] + d["n_delta"] < m.n_states and d["behind_filter"] == 0, "a gap pass without records or cold rows"
    rs.gap_pass = {k: d["pass"] for k, d in enumerate(d for d in descriptors_of(rs.program(0), rs.field_id) if d["phase"] == 1)}
    return rs


def _h_batches(rs):
    """two batches of identical offsets: requests with the words of rules of the first pass alone, of the second alone, of both, of
    neither (a literal / a regex match / a near miss); in the second batch every request holds what its neighbour in kind held"""
    def build(second):
        reqs = []
        for i in range(320):
            j, kind = i % 8, (i // 8) % 5
            a, b = rs.gap_hit[j], rs.gap_hit[8 + j]  # (the chunks are rules 0 - 7 and 8 - 15; the later chunk is the launch's first pass: gap_walks proves who walks)
            none = rs.walk_hit[j % 4] if rs.name == "H" else rs.lits[j % 4]
            first, then = [(a, b), (b, none), (a + "~" + b, rs.gap_miss[j]), (none, a), (rs.gap_miss[8 + j], a + "~" + b)][kind]
            n = max(len(first), len(then))
            k = [j, 8 + j, j if i % 2 else 8 + j, H_GAPS + j % 4, 8 + j][kind]
            reqs.append(rs.request((then if second else first).ljust(n, "~"), k if i % 4 else (rs.k_walk if rs.name == "H" else H_GAPS)))
        return reqs

    # the tiers of the two gap passes: T's targets over their tables (boundary, record and cold states at the four group positions); a
    # string deep enough to hold a factor of its pass is walked by it
    rng = random.Random(41)
    targets = []
    for d in descriptors_of(rs.program(0), rs.field_id):
        if d["phase"] == 1:
            strings, _ = target_strings(rs.model(rs.program(0), d["pass"], 0), d, rng, extra=3)
            targets += [at_position(b"", head + rest, len(head), p) for head, rest in strings for p in range(4)]
    tail = [rs.request(v, i % H_GAPS) for i, v in enumerate(dict.fromkeys(targets))]
    r0, r1 = build(False) + tail, build(True) + tail
    pad = fillers(rs, 8 * len(r0))  # (lists shorter than an eighth of the batch: the lockstep loop; the short batch: lscan_async for the owner)
    b0, b1, short = RequestBatch.from_requests(r0 + pad), RequestBatch.from_requests(r1 + pad), RequestBatch.from_requests(r0)
    assert all((b0.offsets[f] == b1.offsets[f]).all() for f in range(5))
    return b0, b1, short


@functools.lru_cache(maxsize=None)
def case_sh():
    """S over set H, an owner whose walk list serves TWO gap passes with factors of their own: requests that set the need bit of exactly
    one of them (each in turn), of both and of none (a regex match alone: on the owner's list, both bits clear); two batches of
    identical offsets in turn, four turns: a pass's record of the first batch lies where it does not walk in the second."""
    rs = set_h(True)
    b0, b1, short = _h_batches(rs)
    assert 8 * sum(gap_walks(rs, b0)[1]) < b0.n and 8 * sum(gap_walks(rs, short)[1]) >= short.n
    measured = {}
    for label, b in (("first", b0), ("second", b1)):
        g, on = gap_walks(rs, b)
        count = {key: sum(1 for x in g if x == frozenset(key)) for key in ((0,), (1,), (0, 1))}
        count["listed, no bit"] = sum(1 for x, o in zip(g, on) if o and not x)
        assert all(v >= 30 for v in count.values()), (label, count)
        measured[label] = {str(k): v for k, v in count.items()}
    g0, g1 = gap_walks(rs, b0)[0], gap_walks(rs, b1)[0]
    stale = [sum(1 for x, y in zip(g0, g1) if bit in x and bit not in y) for bit in (0, 1)]
    assert min(stale) >= 30, stale
    measured["stale per pass"] = stale
    return CC.Case("SH", rs, [("SH first", b0), ("SH second", b1), ("SH short", short)], measured, turns=4)


@functools.lru_cache(maxsize=None)
def case_so():
    """S over set O, two gap passes with lists of their OWN (no sharing owner: the owner's confirm tier never walks, its literal hits
    enqueue the request on the gap pass's list and set the pass's visited bit): requests on the first list alone, on the second alone, on
    both and on neither; two batches of identical offsets in turn, four turns: a pass's record of the first batch lies where its visited
    bit is clear in the second."""
    rs = set_h(False)
    assert all(d["share_owner"] < 0 for d in descriptors_of(rs.program(0), rs.field_id) if d["phase"] == 1)
    b0, b1, short = _h_batches(rs)
    measured = {}
    for label, b in (("first", b0), ("second", b1)):
        g, _ = gap_walks(rs, b)
        count = {key: sum(1 for x in g if x == frozenset(key)) for key in ((), (0,), (1,), (0, 1))}
        assert all(v >= 30 for v in count.values()), (label, count)
        measured[label] = {str(k): v for k, v in count.items()}
    g0, g1 = gap_walks(rs, b0)[0], gap_walks(rs, b1)[0]
    stale = [sum(1 for x, y in zip(g0, g1) if bit in x and bit not in y) for bit in (0, 1)]
    assert min(stale) >= 30, stale
    measured["stale per pass"] = stale
    # a launch in which the first list is empty and the second holds a single entry
    one = RequestBatch.from_requests([rs.request("~" * (i % 9) + (rs.gap_hit[0] if i == 77 else rs.gap_miss[i % 16]), 0 if i == 77 else i % 16) for i in range(128)])
    g, _ = gap_walks(rs, one)
    assert [sum(1 for x in g if bit in x) for bit in (0, 1)] == [0, 1]
    return CC.Case("SO", rs, [("SO first", b0), ("SO second", b1), ("SO short", short), ("SO one entry", one)], measured, turns=4)


Q_FIELDS = ("host", "url", "user_agent")


@functools.lru_cache(maxsize=None)
def set_q():
    """set Q: two counted-gap rules on each of host, url and user_agent (bare rules: the path is no key here): ONE phase-0 launch holds
    the filtered passes of the three fields (and the gate's pass on the path), each with a list of its own"""
    gr, gt = H.kind_rules("gap", 6, seed=1)
    preds = [e.replace("http_request.url", "http_request." + Q_FIELDS[k % 3]) for k, (_, e, _) in enumerate(gr)]
    rs = RuleSet("Q", "url", preds, verdict_form=False)
    rs.hit = {Q_FIELDS[k % 3]: t[1][0] for k, t in enumerate(gt)}
    rs.miss = {Q_FIELDS[k % 3]: t[1][5] for k, t in enumerate(gt)}
    return rs


@functools.lru_cache(maxsize=None)
def case_tq():
    """T over set Q: for the pass of each of its three fields, as built (the full table behind the walk list, 48 KiB) and without the
    confirm tier (144 KiB, records), T's targets at the four group positions, the value in that field and nothing in the others; once
    among eight times as many requests on no list (the lockstep loop) and once alone (lscan_async)"""
    rs = set_q()
    rng = random.Random(51)
    reqs = []
    for field in Q_FIELDS:
        fid = _abi.FIELD_NAMES.index(field)
        values = []
        for flags in (0, _abi.OPT_NO_CONFIRM):
            prog = rs.program(flags)
            for d in descriptors_of(prog, fid):
                if d["dense_mode"] != 1:
                    strings, _ = target_strings(rs.model(prog, d["pass"], d["tier"]), d, rng, extra=3)
                    values += [at_position(b"", head + rest, len(head), p) for head, rest in strings for p in range(4)]
        for v in dict.fromkeys(values):
            f = dict(host="h~~~", url="/~~~~", path="/p", user_agent="~~~~", method="GET")
            f[field] = v
            reqs.append(Request(**f))
    pad = [Request(host="h~~~", url="/" + "~" * (7 + i % 23), path="/p", user_agent="~~~~", method="GET") for i in range(8 * len(reqs))]
    return CC.Case("TQ", rs, [("TQ padded", RequestBatch.from_requests(reqs + pad)), ("TQ short", RequestBatch.from_requests(reqs))], dict(n=len(reqs)))


@functools.lru_cache(maxsize=None)
def case_lists():
    """P, a launch with several passes of which one list is empty between two that are not, and one holds a single entry: set Q's
    phase-0 launch walks the passes of host, url, path and user_agent in this order; 20 requests hold a host rule's words (20 a near miss), none a
    url rule's (nor anything its filter flags), exactly one a user_agent rule's. The list lengths are the numpy filter model's for the
    engine without confirm tier (candidate lists); as built the walk lists are the requests whose factor the confirm tier finds."""
    rs = set_q()
    reqs = []
    for i in range(200):
        f = dict(host="h~~~", url="/~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~", path="/p", user_agent="~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~", method="GET")
        if i % 5 == 0:
            f["host"] = "~" * (16 + i % 3) + (rs.hit["host"] if i % 10 else rs.miss["host"]) + "~" * 20
        if i == 101:
            f["user_agent"] = "~" * 19 + rs.hit["user_agent"] + "~" * 19
        reqs.append(Request(**f))
    batch = RequestBatch.from_requests(reqs)
    nc = _abi.OPT_NO_CONFIRM
    prog = rs.program(nc)
    t = table_walker.Tables(prog.dump())
    ds = [d for d in descriptors_of(prog) if d["phase"] == 0]
    assert [d["field"] for d in ds] == [0, 1, 2, 4] and {(d["launch"], d["launch_count"]) for d in ds} == {(0, 4)}, ds
    lists = []
    for d in ds:
        sh = CC.PassShape(t.groups[d["pass"]], batch, d["field"])
        lists.append(sum(1 for r in range(batch.n) if sh.chunks_of(r)))
    assert lists[0] >= 20 and lists[1:] == [0, 0, 1], lists  # (a near miss of the host rule may or may not be flagged)
    return CC.Case("lists", rs, [("lists", batch)], dict(n=batch.n, lists=lists))


@functools.lru_cache(maxsize=None)
def case_d():
    """D. the dense alternative: a batch whose url arena is one slab in which more than half of the chunks are flagged (every request
    a run of regex matches), so that the full table walks EVERY request (dense_mode 1, under the clamped n_hot of the 48 KiB launch) and
    the sharing gap pass every request with its need bit (dense_mode 3); a few requests hold T's cold targets of the full table."""
    rs, descs = m_descriptors()
    flags, d, m = descs["dense alternative"]
    dist, par = m.search(m.rest)
    cold = [s for s in range(d["n_hot"], m.n_states) if 0 < dist[s] <= 8][:40]
    assert len(cold) == 40
    reqs = []
    i = 0
    total = 0
    while total < 120 * 1024:
        j = i % M_REGEX
        run = "~".join(rs.rx_hit((j + x) % M_REGEX) for x in range(3))
        if i % 9 == 0:
            s = cold[(i // 9) % len(cold)]
            v = run.encode() + b"~" + m.path_to(s, par, m.rest) + (m.search(s, stop_at_emit=True) or b"")
        elif i % 9 == 1:
            a, b = rs.gaps[i % M_GAPS]
            v = (a + run + b).encode()
        elif i % 9 == 2:
            v = (run[:-1] + "!").encode()
        else:
            v = run.encode()
        reqs.append(rs.request(v, rs.k_rx + j if i % 2 else rs.k_gap + i % M_GAPS))
        total += len(v)
        i += 1
    batch = RequestBatch.from_requests(reqs)
    prog = rs.program(0)
    t = table_walker.Tables(prog.dump())
    g = t.groups[d["pass"]]
    sh = CC.PassShape(g, batch, rs.field_id)
    assert sh.n_slabs == 1 and sh.pairs > sh.dense_thresh, f"D: {sh.pairs} flagged chunks against a threshold of {sh.dense_thresh}: the pass is not walked whole"
    return CC.Case("D", rs, [("D", batch)], dict(n=batch.n, flagged_chunks=sh.pairs, dense_thresh=sh.dense_thresh))


@functools.lru_cache(maxsize=None)
def tuned_m():
    """set M tuned on a small sample that makes OTHER states hot: every second request of case T's first third (walks deep into states that are cold
    as built; of T's first third, so that the rest still meets cold rows) among six times as many requests that flag nothing (a filter that flags more than 40 % of its sample is dropped).
    -> (the sample, the host program tuned on it, its R-tier descriptor and model)"""
    rs = set_m()
    t = case_t("M").batches[0][1]
    reqs = []
    for i in range(0, t.n // 3, 2):  # (the first third of T: its states become hot, those of the rest stay cold)
        reqs.append(rs.request(t.field_bytes(rs.field_id, i), i % len(rs.preds)))
        reqs += [rs.request("/benign/" + "~" * (j + i % 7), j) for j in range(6)]
    sample = RequestBatch.from_requests(reqs)
    host = CompiledProgram(rs.verdict_rules, {}, **rs.opts)
    host.tune(sample)
    found = [d for d in descriptors_of(host, rs.field_id) if d["tier"] == 1]
    assert len(found) == 1, "the tuned program has no R-tier walk"
    d = found[0]
    m = FlatModel(host, d["pass"], 1)
    plain = rs.program(0).flat_image(d["pass"], 1)
    assert host.flat_image(d["pass"], 1) != plain, "tuning moved no state of the R tier"
    assert d["n_hot"] < m.n_states and d["hot_bytes"] == 48 * 1024
    return sample, host, d, m


@functools.lru_cache(maxsize=None)
def case_dl():
    """D over set L: every request a run of literals (hits, last byte wrong), one slab with more than half of its chunks flagged: as built
    the only list scan of set L, its dense alternative, walks every request through the full table under the 48 KiB clamp"""
    rs, descs = l_descriptors()
    flags, d, m = descs["dense alternative"]
    reqs, total, i = [], 0, 0
    while total < 120 * 1024:
        run = "~".join(rs.lits[(i + x) % L_LITS] for x in range(3))
        v = run if i % 3 else run[:-1] + "!"
        reqs.append(rs.request(v, (i + 2) % L_LITS if i % 2 else i % L_LITS))
        total += len(v)
        i += 1
    batch = RequestBatch.from_requests(reqs)
    t = table_walker.Tables(rs.program(0).dump())
    sh = CC.PassShape(t.groups[d["pass"]], batch, rs.field_id)
    assert sh.n_slabs == 1 and sh.pairs > sh.dense_thresh, f"DL: {sh.pairs} flagged chunks against a threshold of {sh.dense_thresh}"
    return CC.Case("DL", rs, [("DL", batch)], dict(n=batch.n, flagged_chunks=sh.pairs, dense_thresh=sh.dense_thresh))


CASES = {"T": case_t, "TL": lambda: case_t("L"), "W": case_w, "S": case_s, "SG": case_sg, "SH": case_sh, "SO": case_so, "lists": case_lists, "TQ": case_tq, "D": case_d, "DL": case_dl,
         "DG": lambda: dense_case("DG", set_g(), set_g().gap_hit + set_g().walk_hit, G_GAPS + G_WALKS),
         "DH": lambda: dense_case("DH", set_h(True), set_h(True).gap_hit + set_h(True).walk_hit + set_h(True).lits, H_GAPS + 8),
         "DO": lambda: dense_case("DO", set_h(False), set_h(False).gap_hit + set_h(False).lits, H_GAPS + 4)}
