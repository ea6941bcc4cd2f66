"""TEST-ONLY: the raw DFA of a program dump and the two device images of a DFA group (csrc/scanplan.h: the streaming table of scan_kernel,
the flat table of lscan_kernel) as walkers with one interface -- start() -> (state, atoms), step(state, class) -> (state, atoms),
end(state) -> atoms. Shared by tests/test_scanplan_cpu.py (which pairs them state by state) and tests/scan_cases.py (which reads the row
a request stands on, byte by byte, off the streaming table)."""
import numpy as np


def raw_of(g):
    """a dump group (or its R tier) / a hand-made group as the raw walker reads it; stays: the classes that stay (scalar mode: the classes of
    the bytes from 0x80 on whose every transition is a self loop — continuation and lead bytes, whose scalar was read at the lead byte)"""
    trans = np.asarray(g["trans"]).reshape(g["n_states"], g["n_classes"])
    stays = g.get("stays")
    if stays is None:
        stays = [0] * g["n_classes"]
        if g.get("umap") is not None:
            for c in {int(g["classmap"][b]) for b in range(0x80, 0x100)}:
                stays[c] = int(all(int(trans[s, c]) == s for s in range(g["n_states"])))
    return dict(trans=trans, emit_off=g["emit_off"], emit_list=g["emit_list"], end_off=g["end_off"], end_list=g["end_list"], stays=stays, n_classes=g["n_classes"])


class RawWalker:
    """entering a state emits its emit list; a class that stays enters nothing. quiet_start: re-entering the start state emits nothing (the
    streaming table records what the start state emits once, when a request starts: ScanImage::start_emit)"""

    def __init__(self, raw, quiet_start):
        self.r, self.quiet_start = raw, quiet_start

    def emits(self, s):
        return frozenset(int(a) for a in self.r["emit_list"][self.r["emit_off"][s]:self.r["emit_off"][s + 1]])

    def start(self):
        return 0, self.emits(0)

    def step(self, s, c):
        if self.r["stays"][c]:
            return s, frozenset()
        t = int(self.r["trans"][s, c])
        return t, frozenset() if t == 0 and self.quiet_start else self.emits(t)

    def end(self, s):
        return frozenset(int(a) for a in self.r["end_list"][self.r["end_off"][s]:self.r["end_off"][s + 1]])


class ScanWalker:
    """the streaming table as kernels.h documents it; cpos: class -> cell position"""

    def __init__(self, m, cpos):
        self.m, self.cpos = m, cpos

    def lst(self, id1):
        m = self.m
        assert 1 <= id1 < len(m["list_off"])
        return frozenset(int(a) for a in m["list"][m["list_off"][id1 - 1]:m["list_off"][id1]])

    def cell(self, v):
        return frozenset() if v == 0 else frozenset([v & 0x7FFF]) if v & 0x8000 else self.lst(v)

    def start(self):
        return 0, (self.lst(self.m["start_emit"]) if self.m["start_emit"] else frozenset())

    def step(self, q, c):
        m = self.m
        st, C = m["stride"], m["n_classes"]
        v = int(m["tab"][q * st + self.cpos[c]])
        if v < m["special_base"]:
            assert v % st == 0 and v // st < m["n_hot"], "a hot cell is the cell index of a hot row"
            t = v // st
            emit_cell = int(m["tab"][t * st + C + 2])
            if v < m["emit_base"]:
                assert emit_cell == 0, "a plain hot row has an empty EMIT cell"
                return t, frozenset()
            assert emit_cell != 0
            return t, self.cell(emit_cell)
        assert v - m["special_base"] < len(m["special"]), "a special cell names an entry of `special`"
        sp = m["special"][v - m["special_base"]]
        assert int(sp["next_off"]) % (2 * st) == 0
        t = int(sp["next_off"]) // (2 * st)
        assert m["n_hot"] <= t < m["n_states"], "a special cell names a cold row"
        return t, (self.lst(int(sp["emit"])) if sp["emit"] else frozenset())

    def end(self, q):
        m = self.m
        assert int(m["tab"][q * m["stride"] + m["n_classes"]]) == (q * m["stride"] if q < m["n_hot"] else 0xFFFF), "the STAY cell"
        return self.cell(int(m["tab"][q * m["stride"] + m["n_classes"] + 1]))


class FlatWalker:
    """the list scan's table: rows [0, n_full) whole, then n_delta states as records over a base row, then whole rows again"""

    def __init__(self, m):
        self.m, self.st = m, m["n_classes"] + 3

    def entering(self, q):
        m = self.m
        v = int(m["flat"][q * self.st + m["n_classes"]])
        lst = frozenset(int(a) for a in m["emit_list"][m["emit_off"][q]:m["emit_off"][q + 1]])
        if v & 0x8000:
            assert lst == {v & 0x7FFF}
        else:
            assert v == (1 if lst else 0)
        return lst

    def start(self):
        return 0, self.entering(0)

    def cell(self, q, c):
        m = self.m
        if m["n_full"] <= q < m["n_full"] + m["n_delta"]:
            rec = m["delta"][q - m["n_full"]]
            base, c1, c2, t1, t2 = rec & 0xFFFF, (rec >> 16) & 0xFF, (rec >> 24) & 0xFF, (rec >> 32) & 0xFFFF, rec >> 48
            assert base < m["n_full"]
            return t1 if c == c1 else t2 if c == c2 else int(m["flat"][base * self.st + c])
        return int(m["flat"][q * self.st + c])

    def step(self, q, c):
        v = self.cell(q, c)
        t = v & 0x7FFF
        assert t < self.m["n_states"]
        if not v & 0x8000:
            return t, frozenset()
        lst = self.entering(t)
        assert lst, "a flagged cell leads to a state that emits"
        return t, lst

    def end(self, q):
        m = self.m
        self.entering(q)  # (the EMIT cell of every state, emitting or not)
        assert int(m["flat"][q * self.st + m["n_classes"] + 1]) == q, "the STAY cell"
        lst = frozenset(int(a) for a in m["end_list"][m["end_off"][q]:m["end_off"][q + 1]])
        assert int(m["flat"][q * self.st + m["n_classes"] + 2]) == (1 if lst else 0), "the END cell"
        return lst
