"""The scan-side planner on the CPU (no device): csrc/scanplan.cpp — the streaming table and the list-scan table of every DFA group, the
roles of the passes and the host half of tuning — through the host harness tests/scanplan_host.cpp.

Everything is checked against the RAW DFA of the program dump (GTRN / GEMO / GEML / GENO / GENL, R* for the R tier) or, for hand-made
groups (harness --synthetic), against the DFA this file made: a Python reading of each image's cell encoding (kernels.h) is paired with
the raw DFA state by state over EVERY class — so every input string reports the same atoms at the same positions — and random strings
are walked on top. The pass plan is recomputed here by brute force from the dump. Nothing is compared with a second run of the code
under test, except where the property IS "twice the same" (tuning is deterministic)."""
import json
import os
import random
import struct
import subprocess
from collections import deque

import numpy as np
import pytest

import helpers as H
from pingoo_amd import _abi
from plan_harness import COMPILER_UNITS, U32, tool as plan_tool, write_case
from scan_walkers import FlatWalker, RawWalker, ScanWalker, raw_of  # noqa: F401  (the walkers live in a helper both edge suites import)
from table_walker import Tables, parse_dump

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "scanplan_host.cpp")
UNITS = COMPILER_UNITS + ["scanplan.cpp"]
B = _abi.RULE_ACTION_BLOCK
K_GAP_LISTS = 32  # (program.h: kGapLists)
LDS_NARROW, LDS_WIDE = 48 * 1024, 144 * 1024  # (csrc/scanplan.cpp: list_shape(0), list_shape(2))
FIELD_METHOD, N_FIELDS = 3, 5
OK = {"stage": "ok", "rc": 0, "rule_index": U32, "message": ""}


# ---------------------------------------------------------------------------------------------------------
# the harness
# ---------------------------------------------------------------------------------------------------------
def tool(name="scanplan_host", *extra):
    return plan_tool(name, SRC, UNITS, *extra)


def pack_sample(cols):
    """cols: per string column a list of n byte strings, or None (the sample does not carry it)"""
    n = len(next(c for c in cols if c is not None))
    out = [struct.pack("<III", 1, n, len(cols))]
    for c in cols:
        if c is None:
            out.append(struct.pack("<I", 0))
            continue
        off = np.zeros(n + 1, dtype="<u4")
        off[1:] = np.cumsum([len(x) for x in c])
        data = b"".join(c)
        out += [struct.pack("<I", 1), off.tobytes(), struct.pack("<I", len(data)), data]
    return b"".join(out)


def scan_tail(lds=(LDS_NARROW, LDS_WIDE), specialized=False, skip_identity=False, mean_len=(), sample=None):
    return (b"SCANPLAN" + struct.pack("<5I", lds[0], lds[1], int(specialized), int(skip_identity), len(mean_len)) + struct.pack(f"<{len(mean_len)}d", *mean_len)
            + (pack_sample(sample) if sample is not None else struct.pack("<I", 0)))


def case_args(tmp_path, cases, stem="case"):
    args = []
    for k, c in enumerate(cases):
        c = dict(c)
        plan = {key: c.pop(key) for key in ("lds", "specialized", "skip_identity", "mean_len", "sample") if key in c}
        fc, fo = str(tmp_path / f"{stem}{k}.bin"), str(tmp_path / f"{stem}{k}.out")
        write_case(fc, tail=scan_tail(**plan), **c)
        args += [fc, fo]
    return args


def run_cases(tmp_path, cases, raw=False):
    """cases: write_case's arguments plus scan_tail's -> [(status, Scan | None)] (raw: the output bytes), one process for all of them"""
    args = case_args(tmp_path, cases)
    r = subprocess.run([tool(), *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(cases), r.stdout[-2000:]
    res = []
    for k, line in enumerate(lines):
        st = json.loads(line)
        blob = open(args[2 * k + 1], "rb").read() if st["stage"] == "ok" else None
        res.append((st, blob if raw or blob is None else Scan(blob)))
    for f in args:
        if os.path.exists(f):
            os.remove(f)
    return res


def run_one(tmp_path, rules, **kw):
    (st, scan), = run_cases(tmp_path, [dict(rules=rules, **kw)])
    assert st == OK, st
    return scan


def group_file(g, hot_budget, lds_bytes, visits=None, class_freq=None):
    e, n = g["emit_list"], g["end_list"]
    return b"".join([b"PWAFDFA1", struct.pack("<7I", g["n_states"], g["n_classes"], hot_budget, lds_bytes, visits is not None, class_freq is not None, len(g["stays"])),
                     bytes(g["classmap"]), bytes(g["stays"]), np.asarray(g["trans"], dtype="<u2").tobytes(), np.asarray(g["emit_off"], dtype="<u4").tobytes(),
                     struct.pack("<I", len(e)), np.asarray(e, dtype="<u2").tobytes(), np.asarray(g["end_off"], dtype="<u4").tobytes(), struct.pack("<I", len(n)),
                     np.asarray(n, dtype="<u2").tobytes(), b"" if visits is None else np.asarray(visits, dtype="<u8").tobytes(),
                     b"" if class_freq is None else np.asarray(class_freq, dtype="<u8").tobytes()])


def synthetic(tmp_path, g, hot_budget=64 * 1024, lds_bytes=LDS_NARROW, visits=None, class_freq=None, exe=None):
    """the two table builders over the hand-made group g -> (status, Scan | None)"""
    fg, fo = str(tmp_path / "group.bin"), str(tmp_path / "group.out")
    with open(fg, "wb") as f:
        f.write(group_file(g, hot_budget, lds_bytes, visits, class_freq))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")  # (read by the sanitizer build alone)
    r = subprocess.run([exe or tool(), "--synthetic", fg, fo], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    st = json.loads(r.stdout)
    return st, Scan(open(fo, "rb").read()) if st["stage"] == "ok" else None


SPECIAL_DTYPE = np.dtype([("next_off", "<u4"), ("emit", "<u4")])
PASS_DTYPE = np.dtype([("base", "<u4"), ("kind_slot", "<u4")])
SHORT_DTYPE = np.dtype([("col", "<u4"), ("len_exact", "<u4"), ("lit", "S8")])
ROLE = ("gate", "filtered", "confirm", "confirm_walk", "share_owner", "shared_bits", "need_slot", "visit_slot", "identity", "short_lit")


class Scan:
    """the harness's output: the program dump (table_walker.Tables reads its groups), then per pass the images, then the pass plan"""

    def __init__(self, blob):
        self.blob = blob
        self.tables = Tables(blob) if len(blob) > 8 and blob[8:12] == b"HEAD" else None
        self.groups = self.tables.groups if self.tables else []
        self.img, self.plan = {}, {}
        for tag, count, pl in parse_dump(blob):
            if tag[0] in "SFTU" and tag not in ("SETM", "FCMP") and tag != "UMLN":
                self.img.setdefault(count, {})[tag] = pl
            elif tag[0] == "L" and tag != "LITS" or tag == "UMLN":
                self.plan[tag] = pl
        if "LROL" in self.plan:
            roles = np.frombuffer(self.plan["LROL"], dtype="<i4").reshape(-1, len(ROLE))
            self.roles = [dict(zip(ROLE, (int(x) for x in row))) for row in roles]
            (self.n_gap, self.n_filtered, self.n_gated, self.n_need, self.n_visit, self.n_short, self.short_field) = (int(x) for x in np.frombuffer(self.plan["LCNT"], dtype="<i4"))
            self.owns_factors = list(self.plan["LOWN"])
            self.colmask = np.frombuffer(self.plan["LCOL"], dtype="<u4")
            self.short_atoms = np.frombuffer(self.plan["LSHA"], dtype=SHORT_DTYPE)
            self.pass_table = np.frombuffer(self.plan["LPTB"], dtype=PASS_DTYPE)
            self.launches = [[int(x) for x in np.frombuffer(self.plan[t], dtype="<u4")] for t in ("LLS0", "LLS1")]
            self.mean_len = np.frombuffer(self.plan["UMLN"], dtype="<f8")

    def scan_image(self, k=0):
        s = self.img[k]
        names = ("n_states", "stride", "n_classes", "n_hot", "start_emit", "emit_base", "special_base", "atom_base", "n_local", "field", "scalar_mode", "ill_class")
        m = dict(zip(names, (int(x) for x in np.frombuffer(s["SSHP"], dtype="<u4"))))
        m.update(tab=np.frombuffer(s["STAB"], dtype="<u2").astype(np.int64), cls=s["SCLS"], special=np.frombuffer(s["SSPC"], dtype=SPECIAL_DTYPE),
                 list_off=np.frombuffer(s["SLOF"], dtype="<u4"), list=np.frombuffer(s["SLST"], dtype="<u2"))
        return m

    def flat_image(self, k=0, tier="F"):
        s = self.img[k]
        names = ("n_states", "n_classes", "scalar_mode", "ill_class", "n_full", "n_delta", "lds_bytes")
        m = dict(zip(names, (int(x) for x in np.frombuffer(s[tier + "SHP"], dtype="<u4"))))
        m.update(flat=np.frombuffer(s[tier + "FLT"], dtype="<u2").astype(np.int64), delta=[int(x) for x in np.frombuffer(s[tier + "DLT"], dtype="<u8")], cls=s[tier + "CLS"],
                 emit_off=np.frombuffer(s[tier + "EMO"], dtype="<u4"), emit_list=np.frombuffer(s[tier + "EML"], dtype="<u2"),
                 end_off=np.frombuffer(s[tier + "ENO"], dtype="<u4"), end_list=np.frombuffer(s[tier + "ENL"], dtype="<u2"))
        return m


# ---------------------------------------------------------------------------------------------------------
# the raw DFA and the two images as walkers: start() -> (state, atoms), step(state, class) -> (state, atoms), end(state) -> atoms
# ---------------------------------------------------------------------------------------------------------
def assert_same_walks(raw, img, classes, rng, n_strings=40):
    """pairs the two walkers state by state from the start over every class: then EVERY string reports the same atoms at the same positions
    (start, each step, the end). Returns raw state -> image state. Random strings are walked too (the property as the issue words it)."""
    (s0, e0), (q0, f0) = raw.start(), img.start()
    assert e0 == f0, "what the start state emits"
    pair, todo = {s0: q0}, deque([s0])
    while todo:
        s = todo.popleft()
        assert raw.end(s) == img.end(pair[s]), f"state {s}: what the field ending here emits"
        for c in classes:
            (t, e), (u, f) = raw.step(s, c), img.step(pair[s], c)
            assert e == f, f"state {s}, class {c}: emits {sorted(f)}, the raw DFA {sorted(e)}"
            if t not in pair:
                pair[t] = u
                todo.append(t)
            assert pair[t] == u, f"state {s}, class {c}: two images of raw state {t}"
    assert len(set(pair.values())) == len(pair)
    for _ in range(n_strings):
        (s, e), (q, f) = raw.start(), img.start()
        want, got = [(-1, e)], [(-1, f)]
        for i in range(rng.randint(0, 40)):
            c = rng.choice(classes)
            (s, e), (q, f) = raw.step(s, c), img.step(q, c)
            want.append((i, e))
            got.append((i, f))
        assert got + [("end", img.end(q))] == want + [("end", raw.end(s))]
    return pair


def class_positions(g, cls_img, ill_class):
    """class -> cell position, read off the class image against the dump's class maps (GCLS, GUMP): every byte and every scalar value reads
    the position of ITS class; the positions are a permutation"""
    n, cpos = g["n_classes"], {}
    assert len(cls_img) >= 272 and not any(cls_img[256:272])
    for b in range(256):
        assert cpos.setdefault(int(g["classmap"][b]), cls_img[b]) == cls_img[b], f"byte {b}"
    um = g.get("umap")
    if um is not None:
        img, want = cls_img[272:], um[8:]
        assert len(img) == len(want) and img[:2 * (0x110000 >> 7)] == want[:2 * (0x110000 >> 7)], "stage 1 is not renumbered"
        for a, b in set(zip(want[2 * (0x110000 >> 7):], img[2 * (0x110000 >> 7):])):
            assert cpos.setdefault(a, b) == b, f"scalar class {a}"
        assert ill_class == cpos[um[0]]
    else:
        assert len(cls_img) == 272 and ill_class == 0
    assert len(set(cpos.values())) == len(cpos) and all(p < n for p in cpos.values())
    return cpos  # (a class no byte and no scalar value has is missing: no input reaches its cells)


def check_scan_image(g, m, rng, cpos=None):
    """g: the raw group (dump or hand-made). Invariants of kernels.h, then the walk."""
    raw = raw_of(g)
    S, C, st, n_hot = g["n_states"], g["n_classes"], m["stride"], m["n_hot"]
    assert (m["n_states"], m["n_classes"], st) == (S, C, C + 3) and 1 <= n_hot <= S and len(m["tab"]) == S * st
    assert m["special_base"] == (n_hot + 1) * st and m["special_base"] + (S - n_hot) <= 65535, "every cell fits 16 bits"
    assert len(m["special"]) == max(1, S - n_hot)
    emitting = [int(m["tab"][q * st + C + 2]) != 0 for q in range(n_hot)]
    n_plain = emitting.index(True) if True in emitting else n_hot
    assert all(emitting[n_plain:]) and m["emit_base"] == n_plain * st, "plain hot rows come before the emitting ones"
    if cpos is None:
        cpos = class_positions(g, m["cls"], m["ill_class"])
    classes = [c for c in sorted(cpos) if not raw["stays"][c]]  # (a class that stays: the lane does not step)
    return assert_same_walks(RawWalker(raw, True), ScanWalker(m, cpos), classes, rng)


def check_flat_image(g, m, rng):
    raw = raw_of(g)
    S, C = g["n_states"], g["n_classes"]
    row_bytes = 2 * (C + 3)
    cap_rows = min(S, (m["lds_bytes"] - 48) // row_bytes)
    assert (m["n_states"], m["n_classes"]) == (S, C) and len(m["flat"]) == S * (C + 3)
    if S <= cap_rows or cap_rows < 8 or C > 255:
        assert (m["n_full"], m["n_delta"]) == (cap_rows, 0) and m["delta"] == [0]
    else:
        assert m["n_full"] <= cap_rows and m["n_full"] + m["n_delta"] <= S
        assert m["n_full"] * row_bytes + 8 * m["n_delta"] + 48 <= m["lds_bytes"], "rows and records fit the LDS budget"
        assert len(m["delta"]) == max(1, m["n_delta"])
    w = FlatWalker(m)
    for q in range(m["n_full"], m["n_full"] + m["n_delta"]):
        base = m["delta"][q - m["n_full"]] & 0xFFFF
        own = [int(m["flat"][q * w.st + c]) for c in range(C)]
        assert [w.cell(q, c) for c in range(C)] == own, f"delta state {q}: the record does not give its row"
        assert sum(int(m["flat"][base * w.st + c]) != own[c] for c in range(C)) <= 2, f"delta state {q} differs from its base row in more than two cells"
    assert bytes(m["cls"][:256]) == bytes(g["classmap"]) and (len(m["cls"]) == 272) == (g.get("umap") is None)
    if g.get("umap") is not None:
        assert m["cls"][272:] == g["umap"][8:] and m["ill_class"] == g["umap"][0]
    pair = assert_same_walks(RawWalker(raw, False), w, list(range(C)), rng)
    for c in range(C):  # a class that stays: the cell is the state itself, unflagged even where the state emits
        if raw["stays"][c]:
            for s, q in pair.items():
                assert w.cell(q, c) == q
    return pair


# ---------------------------------------------------------------------------------------------------------
# hand-made groups
# ---------------------------------------------------------------------------------------------------------
def make_group(rng, n_states, n_classes, start_emits=False, near=0.0, stays=(), emit_share=0.3):
    """a random DFA whose every state is reachable (state s > 0 is entered from an earlier one). near: share of the states that copy an
    earlier row but for at most two cells (what the delta records hold). Lists of no, one, two and three atoms; atoms up to 0x7FFE."""
    trans = np.zeros((n_states, n_classes), dtype=np.int64)
    for s in range(n_states):
        if s and rng.random() < near:
            trans[s] = trans[rng.randrange(min(s, 6))]
            for _ in range(rng.randint(0, 2)):
                trans[s, rng.randrange(n_classes)] = rng.randrange(n_states)
        else:
            trans[s] = [rng.randrange(n_states) for _ in range(n_classes)]
    used, free_classes = set(), [c for c in range(n_classes) if c not in stays]
    for s in range(1, n_states):  # (reachable: an edge of its own from an earlier state; may spoil a copied row: then it is no delta candidate)
        cell = (s - 1, 0)  # (one class: a chain)
        while n_classes > 1 and (cell in used or cell[1] not in free_classes):
            cell = (rng.randrange(s), rng.choice(free_classes))
        used.add(cell)
        trans[cell] = s
    for c in stays:
        trans[:, c] = np.arange(n_states)

    def lists(force0):
        off, lst = [0], []
        for s in range(n_states):
            k = (rng.choice([1, 1, 2, 3]) if rng.random() < emit_share else 0) if s or force0 is None else force0
            lst += [rng.choice([rng.randrange(64), 0x7FFE, 0x7FFF - 2]) for _ in range(k)]
            off.append(len(lst))
        return off, lst

    emit_off, emit_list = lists(2 if start_emits else 0)
    end_off, end_list = lists(None)
    classmap = [b % n_classes for b in range(256)]
    st = [1 if c in stays else 0 for c in range(n_classes)] if stays else []
    return dict(n_states=n_states, n_classes=n_classes, classmap=classmap, trans=trans, emit_off=emit_off, emit_list=emit_list, end_off=end_off, end_list=end_list,
                stays=st or [0] * n_classes)


def synthetic_positions(g, m):
    """class -> cell position of a hand-made group: classmap[b] = b % n_classes, no scalar map"""
    cpos = {c: m["cls"][c] for c in range(g["n_classes"])}
    assert all(m["cls"][b] == cpos[b % g["n_classes"]] for b in range(256)) and len(m["cls"]) == 272
    assert sorted(cpos.values()) == list(range(g["n_classes"]))
    return cpos


def check_synthetic(tmp_path, g, rng, **kw):
    st, sc = synthetic(tmp_path, g, **kw)
    assert st == OK, st
    m, f = sc.scan_image(), sc.flat_image()
    pair = check_scan_image(g, m, rng, synthetic_positions(g, m))
    fpair = check_flat_image(g, f, rng)
    return m, f, pair, fpair


# ---------------------------------------------------------------------------------------------------------
# tests: the two images
# ---------------------------------------------------------------------------------------------------------
def test_one_state_and_emitting_start_state(tmp_path):
    rng = random.Random(1)
    one = make_group(rng, 1, 3)
    one["end_off"], one["end_list"] = [0, 1], [5]  # an END set of one atom: the 0x8000 | atom form
    m, f, _, _ = check_synthetic(tmp_path, one, rng)
    assert (m["n_hot"], m["emit_base"], m["special_base"], m["start_emit"]) == (1, 6, 2 * 6, 0) and int(m["tab"][3 + 1]) == 0x8005 and len(m["list"]) == 0
    assert (f["n_full"], f["n_delta"]) == (1, 0)
    two = make_group(rng, 1, 3)
    two["end_off"], two["end_list"] = [0, 2], [5, 9]  # ... of two atoms: a list id
    m, _, _, _ = check_synthetic(tmp_path, two, rng)
    assert int(m["tab"][3 + 1]) == 1 and m["list"].tolist() == [5, 9]
    big = make_group(rng, 1, 3)
    big["end_off"], big["end_list"] = [0, 1], [0x8000]  # one atom that does not fit the short form
    m, _, _, _ = check_synthetic(tmp_path, big, rng)
    assert int(m["tab"][3 + 1]) == 1 and m["list"].tolist() == [0x8000]
    start = make_group(rng, 9, 5, start_emits=True)
    m, _, _, _ = check_synthetic(tmp_path, start, rng)
    assert m["start_emit"] == 1 and int(m["tab"][5 + 2]) == 0, "the start state's emits are recorded once: its EMIT cell stays empty"


@pytest.mark.parametrize("budget", [0, 1, 2 * 2 * 13, 3 * 2 * 13 + 1, 64 * 1024])
def test_hot_budget_from_nothing_to_everything(tmp_path, budget):
    rng = random.Random(budget)
    g = make_group(rng, 37, 10)
    m, _, _, _ = check_synthetic(tmp_path, g, rng, hot_budget=budget)
    stride2 = 2 * 13
    assert m["n_hot"] == (max(1, min(37, (budget - stride2) // stride2)) if budget > 2 * stride2 else 1)
    assert len(m["special"]) == max(1, 37 - m["n_hot"])


def test_shrink_loop_at_the_budget_cap(tmp_path):
    """700 states x 100 classes at the cap of 131070 bytes: 635 hot rows would need 636 * 103 + 65 = 65573 cells — the loop evicts and
    checks again. (The refusal behind it, "DFA too large for the 16-bit cell space", needs 2 * stride + n_states - 1 > 65535 with one hot
    row: out of reach with at most 259 cells per row and 32767 states.)"""
    rng = random.Random(7)
    g = make_group(rng, 700, 100, emit_share=0.1)
    for budget in (131070, 1 << 30):  # (a larger budget is cut to the cap)
        st, sc = synthetic(tmp_path, g, hot_budget=budget)
        assert st == OK
        m = sc.scan_image()
        assert m["n_hot"] == 634 < (131070 - 206) // 206
        check_scan_image(g, m, rng, synthetic_positions(g, m))


def test_too_many_states_is_refused(tmp_path):
    g = make_group(random.Random(3), 32768, 1, emit_share=0.0)
    st, _ = synthetic(tmp_path, g)
    assert st == {"stage": "plan", "rc": _abi.E_UNSUPPORTED, "rule_index": U32, "message": "DFA has more than 32767 states"}
    g = make_group(random.Random(3), 32767, 1, emit_share=0.0)
    assert synthetic(tmp_path, g)[0] == OK


def test_too_many_match_lists_are_refused(tmp_path):
    """list ids share 15 bits with the atom form: the emit lists come first, then the END lists of more than one atom — 32767 in all"""
    def g(n_emit, n_end):
        n = max(n_emit, n_end) + 1
        d = make_group(random.Random(5), n, 1, emit_share=0.0)
        d["emit_off"] = [0, 0] + [2 * min(k, n_emit) for k in range(1, n)]
        d["emit_list"] = [1, 2] * n_emit
        d["end_off"] = [0, 0] + [2 * min(k, n_end) for k in range(1, n)]
        d["end_list"] = [3, 4] * n_end
        return d
    assert synthetic(tmp_path, g(16384, 16383))[0] == OK
    st, _ = synthetic(tmp_path, g(16384, 16384))
    assert st == {"stage": "plan", "rc": _abi.E_UNSUPPORTED, "rule_index": U32, "message": "too many match lists in one DFA group"}


@pytest.mark.parametrize("profile", [False, True])
def test_more_than_64_classes_with_and_without_a_class_profile(tmp_path, profile):
    rng = random.Random(11)
    g = make_group(rng, 40, 150)
    freq = [rng.randrange(1000) for _ in range(256)]
    m, _, _, _ = check_synthetic(tmp_path, g, rng, class_freq=freq if profile else None)
    cpos = synthetic_positions(g, m)
    if not profile:
        assert [cpos[c] for c in range(150)] == list(range(150))
        return
    # positions ordered by how many positions of the row share their bank (p mod 64): with 150 classes those at 22 .. 63 mod 64 have two, the
    # others three; the most frequent classes take them in that order, ties in class order
    slots = sorted(range(150), key=lambda p: ((150 - 1 - p % 64) // 64 + 1, p))
    by_freq = sorted(range(150), key=lambda c: -freq[c])
    assert [cpos[c] for c in by_freq] == slots and cpos != {c: c for c in range(150)}


def test_a_class_profile_moves_nothing_up_to_64_classes(tmp_path):
    rng = random.Random(12)
    g = make_group(rng, 20, 64)
    m, _, _, _ = check_synthetic(tmp_path, g, rng, class_freq=[rng.randrange(1000) for _ in range(256)])
    assert [m["cls"][c] for c in range(64)] == list(range(64))


def test_a_visits_profile_reorders_the_rows(tmp_path):
    rng = random.Random(13)
    g = make_group(rng, 30, 6, near=0.5)
    visits = [rng.randrange(5) * 100 for _ in range(30)]
    m, f, pair, fpair = check_synthetic(tmp_path, g, rng, hot_budget=2 * 9 * 11, visits=visits)
    order = [0] + sorted(range(1, 30), key=lambda s: -visits[s])
    assert m["n_hot"] == 10
    # the hot rows are the ten most visited states (plain ones first among them), the cold rows follow in visit order
    hot = order[:10]
    want = [0] + [s for s in hot[1:] if g["emit_off"][s] == g["emit_off"][s + 1]] + [s for s in hot[1:] if g["emit_off"][s] != g["emit_off"][s + 1]] + order[10:]
    assert [pair[s] for s in want] == list(range(30))
    assert [fpair[s] for s in order] == list(range(30)) and f["n_delta"] == 0  # (everything fits: rows in visit order, no records)
    assert order != list(range(30))


@pytest.mark.parametrize("n_states,n_classes,lds,deltas", [(60, 20, 46 * 20 + 48 + 45, True), (60, 20, 46 * 7 + 48 + 45, False), (60, 256, 518 * 20 + 48 + 500, False),
                                                           (60, 20, LDS_NARROW, False), (700, 20, 46 * 600 + 48, True)])
def test_flat_rows_and_delta_records(tmp_path, n_states, n_classes, lds, deltas):
    """room for 20 rows and five records; for fewer than 8 rows, or 256 classes (a record's classes are bytes), or for every row: no records;
    room for 600 of 700 rows: rows are given up for records while that covers more states (the candidates' base rows are the first 512)"""
    rng = random.Random(n_states + n_classes + lds)
    g = make_group(rng, n_states, n_classes, near=0.8, emit_share=0.4)
    _, f, _, _ = check_synthetic(tmp_path, g, rng, lds_bytes=lds)
    assert (f["n_delta"] > 0) == deltas
    if n_states == 700:
        assert f["n_full"] < 600 and f["n_full"] + f["n_delta"] > 600, "records buy more resident states than the rows they displace"
    visits = [rng.randrange(1000) for _ in range(n_states)]
    _, f, _, fpair = check_synthetic(tmp_path, g, rng, lds_bytes=lds, visits=visits)
    assert deltas or f["n_delta"] == 0
    order = [0] + sorted(range(1, n_states), key=lambda s: -visits[s])
    assert [fpair[s] for s in order[:f["n_full"]]] == list(range(f["n_full"])), "the whole rows are the most visited states"


def test_flat_cells_of_a_class_that_stays_are_unflagged(tmp_path):
    rng = random.Random(17)
    for lds in (LDS_NARROW, 46 * 12 + 48 + 40):  # (whole rows only; rows and records)
        g = make_group(rng, 40, 20, near=0.7, stays=(3, 19), emit_share=0.6)
        _, f, _, fpair = check_synthetic(tmp_path, g, rng, lds_bytes=lds)
        emitting = [s for s in range(40) if g["emit_off"][s] != g["emit_off"][s + 1]]
        assert emitting and all(int(f["flat"][fpair[s] * 23 + 3]) == fpair[s] for s in emitting)


# ---------------------------------------------------------------------------------------------------------
# rule sets: the images of compiled programs, the pass plan by brute force
# ---------------------------------------------------------------------------------------------------------
def check_images(sc, rng):
    for k, g in enumerate(sc.groups):
        m = sc.scan_image(k)
        assert (m["atom_base"], m["n_local"], m["field"], bool(m["scalar_mode"])) == (g["atom_base"], g["n_local"], g["field"], g.get("umap") is not None)
        check_scan_image(g, m, rng)
        f = sc.flat_image(k)
        wide = "f_table" in g and not g.get("filter_cols")
        assert f["lds_bytes"] == (LDS_WIDE if wide else LDS_NARROW)
        check_flat_image(g, f, rng)
        assert ("rtier" in g) == ("TSHP" in sc.img[k])
        if "rtier" in g:
            t = sc.flat_image(k, "T")
            assert t["lds_bytes"] == LDS_WIDE
            check_flat_image(g["rtier"], t, rng)


def descriptors(r, phase, dense_alt, skip_identity):
    """lscan_split.h restated"""
    if r["identity"] and not skip_identity:
        return 1 if phase == 0 else 0
    if r["gate"] < 0 or bool(r["filtered"]) != (phase == 0):
        return 0
    if phase == 1:
        return 1
    return (1 if dense_alt and r["confirm"] else 0) + (0 if r["confirm"] and not r["confirm_walk"] else 1)


def check_pass_plan(sc, short=None, specialized=False, skip_identity=False):
    """the plan recomputed from the dump: GFLT (a gap pass's factor columns), GFHD / GCNF (the filter in use and its confirm tier), GHDR
    (field, columns), the mean lengths the plan was given. short: (pass, [(literal, exact)]) of the short-literal pass the test expects —
    which atoms are anchored literals is the rule text's to say, not the dump's."""
    G, T = sc.groups, sc.tables
    want = [dict(gate=-1, filtered=0, confirm=0, confirm_walk=0, share_owner=-1, shared_bits=0, need_slot=-1, visit_slot=-1, identity=0, short_lit=0) for _ in G]
    colmask = [0] * T.n_cols
    n_gap = n_filtered = 0
    for k, g in enumerate(G):
        if g.get("filter_cols"):
            if n_gap < K_GAP_LISTS:
                want[k]["gate"] = want[k]["visit_slot"] = n_gap
                for c in g["filter_cols"]:
                    colmask[c] |= 1 << n_gap
                n_gap += 1
        elif "f_table" in g:
            want[k].update(gate=K_GAP_LISTS + n_filtered, filtered=1, confirm=g.get("confirm", 0), confirm_walk=int(g.get("confirm", 0) and g.get("confirm_walk", 0)))
            n_filtered += 1
    owner_of = lambda c: next((q for q, g in enumerate(G) if g["atom_base"] <= c < g["atom_base"] + g["n_local"]), -1)  # noqa: E731
    owns = [int(any(colmask[c] for c in range(g["atom_base"], g["atom_base"] + g["n_local"]))) for g in G]
    for k, g in enumerate(G):
        ml = float(sc.mean_len[g["field"]])
        want[k]["identity"] = int(want[k]["gate"] < 0 and (ml < 12 if g["field"] == FIELD_METHOD else 0 < ml < 12))
    if short is not None:
        want[short[0]].update(short_lit=1, identity=0)
    n_need = 0
    for k, g in enumerate(G):
        if want[k]["gate"] < 0 or want[k]["filtered"]:
            continue
        owners = {owner_of(c) for c in g["filter_cols"]}
        o = next(iter(owners))
        if len(owners) == 1 and o >= 0 and want[o]["filtered"] and not (want[o]["confirm"] and not want[o]["confirm_walk"]):
            want[k]["share_owner"] = o
            want[o]["shared_bits"] |= 1 << want[k]["gate"]
            if want[o]["need_slot"] < 0:
                want[o]["need_slot"] = n_need
                n_need += 1
    for k in range(len(G)):
        assert sc.roles[k] == want[k], (k, sc.roles[k], want[k])
    assert (sc.n_gap, sc.n_filtered, sc.n_gated, sc.n_need, sc.n_visit) == (n_gap, n_filtered, K_GAP_LISTS + n_filtered if n_gap or n_filtered else 0, n_need, n_gap)
    assert sc.owns_factors == owns and sc.colmask.tolist() == colmask
    # short atoms
    if short is None:
        assert (sc.n_short, sc.short_field, len(sc.short_atoms)) == (0, -1, 0)
    else:
        k, lits = short
        assert (sc.n_short, sc.short_field) == (len(lits), G[k]["field"]) and len(sc.short_atoms) == len(lits)
        for a in sc.short_atoms:
            lit = bytes(a["lit"])[:int(a["len_exact"]) & 0xFF]
            assert (lit, bool(int(a["len_exact"]) & 0x100)) in lits and int(a["len_exact"]) >> 9 == 0
            cols = set()
            T.scan_field(G[k], lit, cols)  # (the raw DFA agrees: the literal sets the atom's column)
            assert int(a["col"]) in cols
        assert sorted(int(a["col"]) for a in sc.short_atoms) == list(range(G[k]["atom_base"], G[k]["atom_base"] + G[k]["n_local"]))
    # the list-scan launches: whole passes, at most 256 descriptors each, in pass order
    dense_alt = not T.flags & _abi.OPT_NO_DENSE_SWITCH
    for phase in (0, 1):
        per_pass = [descriptors(r, phase, dense_alt, skip_identity) for r in want]
        launches, cur = [], 0
        for d in per_pass:
            if d and cur + d > 256:
                launches.append(cur)
                cur = 0
            cur += d
        if cur:
            launches.append(cur)
        assert sc.launches[phase] == launches and all(0 < c <= 256 for c in launches) and sum(launches) == sum(per_pass)
    # the verdict kernel's pass table
    pt = sc.pass_table
    assert len(pt) == len(G) + 2
    fi = 0
    for k, g in enumerate(G):
        r = want[k]
        kind = (3 << 24) if r["short_lit"] else 0
        if not r["short_lit"] and r["filtered"]:
            kind = 0 if g["f_heads"] else (1 << 24) | fi  # (a pass with heads has records outside its candidate list: read densely)
        elif not r["short_lit"] and r["visit_slot"] >= 0:
            kind = (2 << 24) | r["visit_slot"]
        fi += r["filtered"]
        assert (int(pt[k]["base"]), int(pt[k]["kind_slot"])) == (g["atom_base"], kind), k
    fcmp = getattr(T, "fcmp", [])
    n_res = getattr(T, "n_residual", 0)
    if len(fcmp):
        assert (int(pt[len(G)]["base"]), int(pt[len(G)]["kind_slot"])) == (min(int(d["col"]) for d in fcmp), 0)
    if n_res:
        at = len(G) + (1 if len(fcmp) else 0)
        assert (int(pt[at]["base"]), int(pt[at]["kind_slot"])) == (T.residual_base, (3 << 24) if specialized else 0)
    return want


GAP_OPTS = (0, 0, 65536)  # with 64 KiB per table every rule of helpers.kind_rules("gap", ..) gets a gap pass of its own


@pytest.mark.parametrize("n_gap", [31, 32, 33])
def test_gap_passes_around_the_32_list_slots(tmp_path, n_gap):
    sc = run_one(tmp_path, H.kind_rules("gap", n_gap, seed=1)[0], opts=GAP_OPTS)
    gaps = [k for k, g in enumerate(sc.groups) if g.get("filter_cols")]
    assert len(gaps) == n_gap
    want = check_pass_plan(sc)
    assert sc.n_gap == min(n_gap, 32) and [want[k]["gate"] for k in gaps] == list(range(min(n_gap, 32))) + [-1] * (n_gap - 32)
    if n_gap == 33:
        last = sc.roles[gaps[-1]]
        assert (last["gate"], last["visit_slot"], last["share_owner"]) == (-1, -1, -1) and int(sc.pass_table[gaps[-1]]["kind_slot"]) == 0, "the 33rd gap pass walks every request"
    check_images(sc, random.Random(n_gap))


def owners_of(sc, k):
    return {next((q for q, g in enumerate(sc.groups) if g["atom_base"] <= c < g["atom_base"] + g["n_local"]), -1) for c in sc.groups[k]["filter_cols"]}


def test_gap_passes_share_their_owners_list_or_enqueue(tmp_path):
    """rule sets: the factors of every gap pass sit in ONE filtered owner — whose confirm tier never walks (literal factors alone: the gap passes
    enqueue) or walks (a regex beside them: they share its list)"""
    gap, walk = H.kind_rules("gap", 31, seed=1)[0], H.kind_rules("confirm_walk", 3, seed=2)[0]
    (_, never), (_, shared) = run_cases(tmp_path, [dict(rules=gap, opts=GAP_OPTS), dict(rules=gap[:6] + walk, opts=GAP_OPTS)])
    for sc, sharing in ((never, False), (shared, True)):
        want = check_pass_plan(sc)
        gaps = [k for k, g in enumerate(sc.groups) if g.get("filter_cols")]
        assert len(gaps) == (6 if sharing else 31)
        for k in gaps:
            (o,) = owners_of(sc, k)
            assert (want[o]["filtered"], want[o]["confirm"], want[o]["confirm_walk"]) == (1, 1, int(sharing)) and (want[k]["share_owner"] == o) == sharing
        assert sc.n_need == int(sharing) and sc.launches[1] == [len(gaps)]
    check_images(shared, random.Random(5))


def passes_spec(groups, n_cols, flags=0):
    """groups: dicts field, atom_base, n_local, filter, confirm, walk, heads, cols (harness --passes)"""
    out = [b"PWAFPAS1", struct.pack("<3I", flags, n_cols, len(groups))]
    for g in groups:
        cols = g.get("cols", [])
        out.append(struct.pack(f"<{8 + len(cols)}I", g.get("field", 1), g["atom_base"], g["n_local"], g.get("filter", 0), g.get("confirm", 0), g.get("walk", 0), g.get("heads", 0), len(cols), *cols))
    return b"".join(out)


def run_passes(tmp_path, groups, n_cols, exe=None):
    fs, fo = str(tmp_path / "spec.bin"), str(tmp_path / "spec.out")
    with open(fs, "wb") as f:
        f.write(passes_spec(groups, n_cols))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")  # (read by the sanitizer build alone)
    r = subprocess.run([exe or tool(), "--passes", fs, fo], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and json.loads(r.stdout) == OK, (r.stdout, r.stderr[-2000:])
    return Scan(open(fo, "rb").read())


HAND_MADE = [dict(atom_base=1, n_local=3, filter=1, confirm=1, walk=1), dict(atom_base=4, n_local=3, filter=1, confirm=1, walk=0), dict(atom_base=7, n_local=2),
             dict(atom_base=9, n_local=2, filter=1, heads=1),
             dict(atom_base=11, n_local=1, cols=[9, 10]),     # one owner without a confirm tier: shares
             dict(atom_base=12, n_local=1, cols=[1, 3]),      # one owner that walks: shares
             dict(atom_base=13, n_local=1, cols=[2, 5]),      # two owners: a list of its own
             dict(atom_base=14, n_local=1, cols=[4]),         # an owner that never walks: enqueues
             dict(atom_base=15, n_local=1, cols=[7]),         # an unfiltered owner
             dict(atom_base=16, n_local=1, cols=[0]),         # a column no pass owns
             dict(atom_base=17, n_local=1, cols=[2])]         # the walking owner again: the same need slot


def test_gap_passes_over_hand_made_owners(tmp_path):
    """what no rule set gives (the compiler keeps a field's factors in one pass): factors in two owners, in an unfiltered owner, in no pass
    at all, in an owner without a confirm tier — and the owners' need slots in pass order"""
    sc = run_passes(tmp_path, HAND_MADE, 18)
    want = check_pass_plan(sc)
    assert [r["share_owner"] for r in want[4:]] == [3, 0, -1, -1, -1, -1, 0] and [r["need_slot"] for r in want[:4]] == [1, -1, -1, 0]
    assert want[0]["shared_bits"] == (1 << 1) | (1 << 6) and want[3]["shared_bits"] == 1 and sc.n_need == 2
    assert [int(p["kind_slot"]) >> 24 for p in sc.pass_table[:4]] == [1, 1, 0, 0]  # (the pass with a head is read densely)


METHOD_RULES = [("m0", 'http_request.method == "POST"', [B]), ("m1", 'http_request.method.starts_with("PU")', [B]), ("p", 'http_request.path.contains("zzqq")', [B])]


def test_short_literal_pass_only_the_first_field(tmp_path):
    rules = METHOD_RULES + [("h", 'http_request.host == "a"', [B])]  # (a second field that qualifies: no bigram, no prefilter)
    sc, off = (sc for _, sc in run_cases(tmp_path, [dict(rules=rules), dict(rules=rules, flags=_abi.OPT_NO_PREFILTER)]))
    method = next(k for k, g in enumerate(sc.groups) if g["field"] == FIELD_METHOD)
    host = next(k for k, g in enumerate(sc.groups) if g["field"] == 0)
    first = min(method, host)
    lits = [(b"POST", True), (b"PU", False)] if first == method else [(b"a", True)]
    want = check_pass_plan(sc, short=(first, lits))
    assert want[first]["short_lit"] and not sc.roles[max(method, host)]["short_lit"] and int(sc.pass_table[first]["kind_slot"]) == 3 << 24
    check_pass_plan(off)  # PWAF_OPT_NO_PREFILTER: no short-literal pass; the method pass is an identity pass again
    assert off.roles[next(k for k, g in enumerate(off.groups) if g["field"] == FIELD_METHOD)]["identity"] == 1 and off.n_short == 0
    check_images(sc, random.Random(2))


@pytest.mark.parametrize("ml", [0.0, 11.999, 12.0])
def test_identity_by_mean_length(tmp_path, ml):
    """a plain pass over a field whose sampled mean length is below 12; the method counts as short without a sample too"""
    rules = [("m", 'http_request.method.matches("P[A-Z]{5}$")', [B]), ("h", 'http_request.host.matches("^[ab]+c?$")', [B])]
    sc = run_one(tmp_path, rules, mean_len=[ml] * 5)
    want = check_pass_plan(sc)
    by_field = {g["field"]: want[k] for k, g in enumerate(sc.groups)}
    assert by_field[FIELD_METHOD]["gate"] < 0 and by_field[0]["gate"] < 0
    assert by_field[FIELD_METHOD]["identity"] == int(ml < 12) and by_field[0]["identity"] == int(0 < ml < 12)
    skipped = run_one(tmp_path, rules, mean_len=[ml] * 5, skip_identity=True)
    check_pass_plan(skipped, skip_identity=True)
    assert skipped.roles == sc.roles and sum(skipped.launches[0]) == sum(sc.launches[0]) - sum(r["identity"] for r in want)


def test_more_than_256_list_scan_descriptors_split_into_launches(tmp_path):
    """passes with a confirm tier that walks take two descriptors each (the dense alternative and the walk): 129 or more of them need a second launch"""
    ps = H.pinned_passes("confirm_walk", 140)
    sc, nod = (sc for _, sc in run_cases(tmp_path, [dict(rules=ps.rules, opts=(0, 0, ps.opts["max_table_bytes"])),
                                                    dict(rules=ps.rules, opts=(0, 0, ps.opts["max_table_bytes"]), flags=_abi.OPT_NO_DENSE_SWITCH)]))
    want = check_pass_plan(sc)
    assert sum(r["confirm_walk"] for r in want) >= 129 and len(sc.launches[0]) >= 2 and sc.launches[0][0] == 256
    check_pass_plan(nod)
    assert len(nod.launches[0]) == 1 and sum(nod.launches[0]) == sum(r["confirm_walk"] for r in want) <= 256 < sum(sc.launches[0])


def test_pass_table_kinds_and_the_residual_pseudo_pass(tmp_path):
    rules = METHOD_RULES + H.kind_rules("gap", 31, seed=1)[0] + [("hd", 'http_request.user_agent.starts_with("Mozilla/") && http_request.user_agent.contains("zqzq")', [B]),
                            ("f", "http_request.url.contains(http_request.host)", [B]), ("r", "http_request.url.length() - http_request.path.length() > 15", [B]),
                            ("d", 'http_request.host.matches("^[ab]+c?$")', [B])]
    for specialized in (False, True):
        sc = run_one(tmp_path, rules, specialized=specialized, mean_len=[20.0] * 5, opts=GAP_OPTS)
        method = next(k for k, g in enumerate(sc.groups) if g["field"] == FIELD_METHOD)
        check_pass_plan(sc, short=(method, [(b"POST", True), (b"PU", False)]), specialized=specialized)
        assert sc.tables.n_residual == 1 and len(sc.tables.fcmp) == 1
        kinds = {int(p["kind_slot"]) >> 24 for p in sc.pass_table[:len(sc.groups)]}
        assert kinds == {0, 1, 2, 3}, kinds
    no_fcmp = run_one(tmp_path, [r for r in rules if r[0] != "f"], specialized=True, opts=GAP_OPTS)
    check_pass_plan(no_fcmp, short=(next(k for k, g in enumerate(no_fcmp.groups) if g["field"] == FIELD_METHOD), [(b"POST", True), (b"PU", False)]), specialized=True)
    assert int(no_fcmp.pass_table[len(no_fcmp.groups)]["kind_slot"]) == 3 << 24  # (the residual pseudo pass takes the field-against-field one's place)


def fuzz_case(seed):
    rng = random.Random(seed)
    lists = H.fuzz_lists(rng)
    rules = [(f"r{k}", H.rexpr(rng, lists), H.fuzz_actions(rng)) for k in range(rng.randint(1, 12))]
    return dict(rules=rules, lists=lists, flags=_abi.OPT_LENIENT, opts=(rng.choice([0, 1024, 2048]), rng.choice([0, 60]), rng.choice([0, 4096])))


def test_fuzzed_rule_sets_every_image_walks_like_the_raw_dfa(tmp_path):
    """helpers' fuzz grammar: regexes over a Unicode alphabet (scalar mode, the permuted scalar map), small hot budgets (cold rows)"""
    res = run_cases(tmp_path, [fuzz_case(8000 + s) for s in range(16)] + [dict(rules=TUNE_RULES, opts=(1024, 0, 0))])  # (and a table of some hundred states: cold rows)
    n_scalar = n_cold = 0
    for k, (st, sc) in enumerate(res):
        assert st == OK, (k, st)
        check_images(sc, random.Random(k))
        n_scalar += sum(1 for g in sc.groups if g.get("umap") is not None)
        n_cold += sum(1 for i in range(len(sc.groups)) if sc.scan_image(i)["n_hot"] < sc.scan_image(i)["n_states"])
    assert n_scalar > 0 and n_cold > 0


# ---------------------------------------------------------------------------------------------------------
# tuning
# ---------------------------------------------------------------------------------------------------------
TUNE_W = H.pass_words(79, 3)
TUNE_RULES = [("u", f'http_request.url.contains("{TUNE_W[0]}{TUNE_W[1]}")', [B]), ("p", f'http_request.path.matches("{TUNE_W[2]}[0-9]+x")', [B]),
              ("h", f'http_request.headers["x-a"].contains("{TUNE_W[1]}{TUNE_W[0]}")', [B]), ("m", 'http_request.method.matches("P[A-Z]{5}$")', [B])]


def tune_sample(rng, n=400, flood=0.0, header=True):
    """flood: the share of urls that carry the url rule's literal without its last byte and again without its first (every window of the
    filter occurs, the atom never holds)"""
    lit = (TUNE_W[0] + TUNE_W[1]).encode()
    filler = lambda: "".join(rng.choice("abcdefxyz/.=-_ %") for _ in range(rng.randint(0, 60))).encode()  # noqa: E731
    urls = [filler() + (lit[:-1] + b"!!" + lit[1:] + filler() if rng.random() < flood else b"") for _ in range(n)]
    paths = [rng.choice([b"/", filler(), (TUNE_W[2] + "12x").encode(), TUNE_W[2].encode()]) for _ in range(n)]
    return [[b"h.example"] * n, urls, paths, [rng.choice([b"GET", b"POST", b"PQQQQQ"]) for _ in range(n)], [b"Mozilla/5.0 " + filler() for _ in range(n)],
            [filler() + rng.choice([b"", (TUNE_W[1] + TUNE_W[0]).encode()]) for _ in range(n)] if header else None]


def filter_sections(blob, k):
    return [(t, pl) for t, c, pl in parse_dump(blob) if c == k and t in ("GFHD", "GFTB", "GCNF")]


def test_tuning_is_deterministic_and_a_tuned_plan_walks_like_the_raw_dfa(tmp_path):
    sample = tune_sample(random.Random(21))
    (s1, b1), (s2, b2), (s3, b3) = run_cases(tmp_path, [dict(rules=TUNE_RULES, sample=sample), dict(rules=TUNE_RULES, sample=sample), dict(rules=TUNE_RULES)], raw=True)
    assert s1 == s2 == s3 == OK and b1 == b2, "the same case twice: byte-identical output"
    sc, plain = Scan(b1), Scan(b3)
    check_images(sc, random.Random(22))
    check_pass_plan(sc)
    # the profile is the sample's: mean lengths per field, visits that sum to the bytes walked, and it moved rows
    assert abs(sc.mean_len[1] - np.mean([len(u) for u in sample[1]])) < 1e-9 and abs(sc.mean_len[3] - np.mean([len(m) for m in sample[3]])) < 1e-9
    method = next(k for k, g in enumerate(sc.groups) if g["field"] == FIELD_METHOD)
    assert int(np.frombuffer(sc.img[method]["UVIS"], dtype="<u8").sum()) == sum(len(m) for m in sample[3])
    assert sc.roles[method]["identity"] == 1 and plain.roles[method]["identity"] == 1
    assert any(sc.img[k]["STAB"] != plain.img[k]["STAB"] or sc.img[k]["FFLT"] != plain.img[k]["FFLT"] for k in range(len(sc.groups))), "the visits reorder no row"


def test_a_sample_without_a_header_column_leaves_that_filter_untouched(tmp_path):
    rng = random.Random(23)
    (_, tuned), (_, lacking), (_, plain) = run_cases(tmp_path, [dict(rules=TUNE_RULES, sample=tune_sample(rng)), dict(rules=TUNE_RULES, sample=tune_sample(rng, header=False)),
                                                              dict(rules=TUNE_RULES)], raw=True)
    groups = Scan(plain).groups
    hdr = next(k for k, g in enumerate(groups) if g["field"] == N_FIELDS)
    assert filter_sections(plain, hdr) and filter_sections(lacking, hdr) == filter_sections(plain, hdr)
    assert Scan(lacking).mean_len[N_FIELDS] == 0 and np.frombuffer(Scan(lacking).img[hdr]["UFLT"], dtype="<u4")[3] == 0  # (chunks: 0 = keep)
    assert any(filter_sections(lacking, k) != filter_sections(plain, k) for k in range(len(groups)) if k != hdr), "the sample tunes no filter at all"
    assert Scan(tuned).mean_len[N_FIELDS] > 0
    check_images(Scan(lacking), rng)


def test_a_filter_that_flags_more_than_40_percent_of_the_sample_is_dropped(tmp_path):
    rng = random.Random(24)
    (_, kept), (_, dropped) = run_cases(tmp_path, [dict(rules=TUNE_RULES, sample=tune_sample(rng, flood=0.2)), dict(rules=TUNE_RULES, sample=tune_sample(rng, flood=0.7))])
    url = next(k for k, g in enumerate(kept.groups) if g["field"] == 1)
    assert "f_table" in kept.groups[url] and kept.roles[url]["filtered"] == 1
    assert "f_table" not in dropped.groups[url] and dropped.roles[url] == dict(kept.roles[url], gate=-1, filtered=0, confirm=0, confirm_walk=0)
    assert bytes(dropped.img[url]["UNOT"]).decode() == "the filter flags more than 40 % of the sample"
    assert np.frombuffer(dropped.img[url]["UFLT"], dtype="<u4")[0] == 0 and np.frombuffer(dropped.img[url]["UFLT"], dtype="<u4")[2] == 0, "enabled, heads"
    check_pass_plan(dropped)
    check_images(dropped, rng)


# ---------------------------------------------------------------------------------------------------------
# sanitizers
# ---------------------------------------------------------------------------------------------------------
def test_the_case_list_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same harness built with -fsanitize=address,undefined (a stand-alone program: nothing is preloaded), run once over the cases above"""
    exe = tool("scanplan_host_asan", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    rng = random.Random(31)
    gap = H.kind_rules("gap", 6, seed=1)[0] + H.kind_rules("confirm_walk", 3, seed=2)[0]
    cases = [fuzz_case(8000 + s) for s in range(8)]
    cases += [dict(rules=TUNE_RULES, sample=tune_sample(rng)), dict(rules=TUNE_RULES, sample=tune_sample(rng, header=False)), dict(rules=TUNE_RULES, sample=tune_sample(rng, flood=0.7))]
    cases += [dict(rules=gap, opts=GAP_OPTS), dict(rules=gap, opts=(0, 0, 1024)), dict(rules=METHOD_RULES), dict(rules=METHOD_RULES, flags=_abi.OPT_NO_PREFILTER, specialized=True, mean_len=[11.0] * 5)]
    cases += [dict(rules=H.kind_rules("gap", 33, seed=1)[0], opts=GAP_OPTS)]
    ps = H.pinned_passes("confirm_walk", 140)
    cases += [dict(rules=ps.rules, opts=(0, 0, ps.opts["max_table_bytes"]))]
    args = case_args(tmp_path, cases, "san")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=900, env=env)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and [json.loads(x)["stage"] for x in r.stdout.strip().splitlines()] == ["ok"] * len(cases), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    for g, kw in ((make_group(rng, 1, 3), {}), (make_group(rng, 9, 5, start_emits=True), dict(hot_budget=0)), (make_group(rng, 700, 100, emit_share=0.1), dict(hot_budget=131070)),
                  (make_group(rng, 40, 150), dict(class_freq=[rng.randrange(9) for _ in range(256)], visits=[rng.randrange(9) for _ in range(40)])),
                  (make_group(rng, 60, 20, near=0.7, stays=(3,)), dict(lds_bytes=46 * 20 + 48)), (make_group(rng, 60, 256, near=0.7), dict(lds_bytes=518 * 20 + 48)),
                  (make_group(rng, 32768, 1, emit_share=0.0), {})):
        synthetic(tmp_path, g, exe=exe, **kw)
    run_passes(tmp_path, HAND_MADE, 18, exe=exe)
