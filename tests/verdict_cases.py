"""TEST-ONLY: the cases of the verdict kernel's edge suite (docs/verdict_edges.md) — rule sets whose every atom is true or false for a
request BY CONSTRUCTION, base batches laid out by 64-request groups, and two independent statements about them:

  reference()   numpy, written from the rule list: the first rule in order whose expression holds and whose action takes effect for the
                request's verified bit, the four counters, the hit matrix, the first route. Not the engine, not a model of the kernel.
  GroupModel    what verdict2_kernel (csrc/verdict.hip) does with a group, from the program's tables (the plan of tests/tableplan_host.cpp:
                device rules and literals, trigger lists, the always-bitmap; the dump's pass ranges) and the truth table: the attribute
                pairs, the distinct atoms per scan pass and the lanes with an overflow chain, the entries appended at each of the three
                append sites in the kernel's order, the candidate count, whether the group spills.

The builders assert from the model that every target exists at the capacity the shape hook reports (pwaf_program_verdict_shape) and fail,
naming the target, when one does not. tests/test_verdict_edges_cpu.py runs them without a device; tests/test_gpu_verdict_edges.py sends
the batches."""
import functools
import os
import tempfile
import pathlib

import numpy as np

import helpers as H
from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.engine import CompiledProgram
from table_walker import LIT_ATOM_MASK, LIT_NEG, LIT_TERM_END, Tables, parse_dump

B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
TINY, GLOBAL, HITS, SPARSE, DENSE = _abi.OPT_TINY_VERDICT_SLOTS, _abi.OPT_GLOBAL_VERDICT_TABLES, _abi.OPT_RULE_HITS, _abi.OPT_SPARSE_VERDICT, _abi.OPT_DENSE_VERDICT
LIT_LAZY = 1 << 29
FIELDS = ("url", "path", "host", "user_agent")  # the token fields, in atom order
N_TOK, N_IP, N_PORT = 75, 140, 40                # tokens per field, ip lists, port sets
A_IP, A_PORT, N_ATOMS = 4 * N_TOK, 4 * N_TOK + N_IP, 4 * N_TOK + N_IP + N_PORT
N_SHARED_IP, N_SHARED_PORT = N_IP // 2, N_PORT // 2
IP_NONE, PORT_NONE = (192 << 24) | (2 << 8) | 1, 9
# verdict2_kernel's kPre, the hit records requested one group ahead, by bitmap registers (BR = 1: up to 64 passes; else kVerdictPre):
# tests/test_verdict_edges_cpu.py pins both to the sources
K_PRE_BY_BR = {1: 4, 4: 12}
K_PRE = K_PRE_BY_BR[1]


def k_pre(n_passes):
    return K_PRE_BY_BR[1 if n_passes <= 64 else 4]
ACTIONS = ([B], [CAP], [CAP, B])


# ---------------------------------------------------------------------------------------------------------
# rule sets: a rule is (name, DNF, actions); DNF = [[(atom, negated), ...], ...]
# ---------------------------------------------------------------------------------------------------------
def atom_text(words, a):
    if a < A_IP:
        return f'http_request.{FIELDS[a // N_TOK]}.contains("{words[a]}")'
    if a < A_PORT:
        return f'lists["ip{a - A_IP}"].contains(client.ip)'
    return f'lists["ps{a - A_PORT}"].contains(client.remote_port)'


def dnf_text(words, dnf):
    if dnf is None:  # a match-all rule (`expression: None`): filed under column 0 = TRUE
        return None
    terms = [" && ".join(("!" if neg else "") + atom_text(words, a) for a, neg in term) for term in dnf]
    return terms[0] if len(terms) == 1 else " || ".join("(" + t + ")" for t in terms)


class RuleSet:
    """rules: [(name, dnf, actions)]; routes: [(name, dnf)]. Rules atom_rule0 .. atom_rule0 + N_ATOMS - 1 are the atoms alone, in atom order:
    the column of atom k is the one literal of the device rule whose public index is atom_rule0 + k."""

    n_atoms, n_scan_atoms, opts = N_ATOMS, A_IP, {}  # (atoms below n_scan_atoms are scan atoms, the others attribute atoms)

    def __init__(self, name, compound, seed):
        self.name = name
        self.words = H.pass_words(900 + seed, 4 * N_TOK)
        # (the negation-only rules: CAPTCHA, a verified request passes them; set A ends with a match-all rule that blocks what is left)
        # (a compound entry is a DNF, or (DNF, actions) where the actions matter)
        def rule(j, c):
            if isinstance(c, tuple):
                return (f"c{j}", c[0], list(c[1]))
            return (f"c{j}", c, [B] if c is None else [CAP] if all(neg for t in c for _, neg in t) else ACTIONS[(j + 1) % 3])

        comp = [rule(j, c) for j, c in enumerate(compound)]
        self.atom_rule0 = 20  # twenty compound rules decide before the atoms alone do, the others after them
        self.rules = comp[:20] + [(f"a{k}", [[(k, False)]], ACTIONS[k % 3]) for k in range(N_ATOMS)] + comp[20:]
        self.lists = {}
        for k in range(N_IP):  # its own /24 and one shared with its neighbour: a request in 10.1.j.0/24 is in lists 2j and 2j + 1
            self.lists[f"ip{k}"] = (_abi.LIST_IP, [f"10.0.{k}.0/24", f"10.1.{k // 2}.0/24"])
        for k in range(N_PORT):
            self.lists[f"ps{k}"] = (_abi.LIST_INT, [str(2000 + k), str(3000 + k // 2)])
        self.routes = [(f"r{j}", [[(j * 23 % (4 * N_TOK), False)], [((j * 23 + 7) % (4 * N_TOK), False)]] if j % 2 else [[(j * 23 % (4 * N_TOK), False)]]) for j in range(12)]

    def rule_tuples(self):
        return [(n, dnf_text(self.words, d), list(a)) for n, d, a in self.rules]

    def route_tuples(self):
        return [(n, dnf_text(self.words, d)) for n, d in self.routes]

    @functools.lru_cache(maxsize=None)
    def program(self, flags=0, routed=False):
        return CompiledProgram(self.rule_tuples(), self.lists, routes=self.route_tuples() if routed else None, flags=flags, **self.opts)

    @functools.lru_cache(maxsize=None)
    def tables(self, flags=0, routed=False):
        """(Plan of the table planner, Tables of the dump) for the program with `flags` (routed: compiled with the set's routes)"""
        from test_tableplan_cpu import run_one

        with tempfile.TemporaryDirectory() as d:
            st, plan = run_one(pathlib.Path(d), self.rule_tuples(), lists=self.lists, flags=flags, routes=self.route_tuples() if routed else None,
                               opts=(self.opts.get("lds_table_budget", 0), self.opts.get("max_dfa_states", 0), self.opts.get("max_table_bytes", 0)) if self.opts else None)
        assert st["stage"] == "ok", st
        return plan, Tables(self.program(flags, routed))

    def truth(self, groups):
        return truth(groups)

    def make_batch(self, groups):
        return make_batch(self, groups)

    def extra_columns(self, g, tabs):
        return []

    residual_atoms = range(0)

    def atom_rule(self, a):
        """the rule that holds atom a alone"""
        return self.atom_rule0 + a


def compound_a():
    """short DNFs beside the atoms: a || b, a && !b, a && b over tokens, lists and port sets, and two negation-only rules at the end
    (candidates in every group: the always-bitmap)"""
    out = []
    for j in range(40):
        a, b, c = (j * 7) % (4 * N_TOK), A_IP + (j * 3) % N_IP, A_PORT + j % N_PORT
        out.append([[[(a, False)], [(b, False)]], [[(a, False), (c, True)]], [[(b, False), (c, False)]], [[(a, False), (b, True)], [(c, False)]]][j % 4])
    out.append([[(3, True), (A_IP + 1, True)]])
    out.append([[(N_TOK + 5, True)]])
    out.append(None)  # match-all: reads column 0 = TRUE (entry 0, which a spilled group's clean-up must restore)
    return out


N_OBSERVE = 12


def compound_h():
    """set H, for the rule-hits leg alone: A's rules and twelve rules WITHOUT actions (observe-only: a PWAF_OPT_RULE_HITS engine keeps them as
    device rules and reports their matches; every other engine drops them) — six before the atoms, six behind them"""
    a = compound_a()

    def observe(j):
        t, i, p = (j * 31 + 2) % (4 * N_TOK), A_IP + (j * 13) % N_IP, A_PORT + (j * 7) % N_PORT
        return ([[[(t, False)], [(i, False)]], [[(t, False), (p, True)]], [[(i, False)], [(p, False)]]][j % 3], [])

    return [observe(j) for j in range(6)] + a[:14] + a[14:-3] + [observe(6 + j) for j in range(6)] + a[-3:]


def compound_c():
    """A's, and 40 rules over three tokens of ONE field"""
    out = compound_a()[:-3]
    for j in range(40):
        f, t = j % 4, (j * 5) % (N_TOK - 4)
        out.append([[(f * N_TOK + t, False), (f * N_TOK + t + 1, False), (f * N_TOK + t + 3, False)]])
    return out + compound_a()[-3:-1]  # (no match-all rule: what no rule decides is allowed)


# set W: the four tokens whose own rules are CAPTCHA-only (atom % 3 == 1), one per field: a VERIFIED request that carries some of them
# passes its atoms' rules and is decided by the rules placed at the bitmap's edges
W_B, W_Z, W_A, W_Q = 1, N_TOK + 4, 2 * N_TOK + 1, 3 * N_TOK + 4
W_IP = A_IP + 1  # (an ip list whose own rule is CAPTCHA-only too)
W_RULES, W_GATES = 2100, 2  # caller rules; the two gate pseudo rules are device rules 0 and 1


def compound_w():
    """2100 caller rules = 2102 device rules, 66 bitmap words: the negation-only rules `!B` at device index 2047 (word 63, bit 31: the last
    word of the register copy) and `!Z` at 2048 (word 64: read from memory in step 1, compacted in step 4's second round), the deciding
    rule `B && Z && !A` at 2049, and in the last word `!Q`, `Q && A && ip list 1` and a match-all rule filed under column 0. Between them two-literal
    conjunctions that never name the four tokens: they fill the candidate lists."""
    special = {W_B, W_Z, W_A, W_Q, W_IP}

    def filler(j):
        a = (j * 11) % (4 * N_TOK)
        while a in special:
            a += 1
        b = A_IP + (j * 5) % (N_IP + N_PORT) if j % 3 else (a + 37 + j % 5) % (4 * N_TOK)
        while b in special or b == a:
            b += 1
        return ([[(a, False), (b, False)]], ACTIONS[j % 3])

    out = compound_a()[:20]
    n_before = W_RULES - 20 - N_ATOMS  # compound rules behind the atoms
    at_2047 = 2047 - W_GATES - 20 - N_ATOMS
    out += [filler(j) for j in range(at_2047)]
    out += [([[(W_B, True)]], [CAP, B]), ([[(W_Z, True)]], [CAP, B]), ([[(W_B, False), (W_Z, False), (W_A, True)]], [B])]
    out += [filler(1000 + j) for j in range(n_before - at_2047 - 6)]
    out += [([[(W_Q, True)]], [CAP, B]), ([[(W_Q, False), (W_A, False), (W_IP, False)]], [B]), (None, [B])]
    assert len(out) == 20 + n_before
    return out


class PassSet(RuleSet):
    """helpers.pinned_passes: url.contains("<word>") rules, one atom each, that compile to exactly n_passes scan passes (8: the instantiation
    for up to 64 passes, which requests the records of 4 passes a group ahead; 65: the general one, 12). Atom k = rule k's word."""

    def __init__(self, n_passes):
        ps = H.pinned_passes("confirm_literal", n_passes)
        self.name, self.ps, self.opts, self.n_passes = f"P{n_passes}", ps, dict(ps.opts), n_passes
        self.words = [vals[0] for _, vals in ps.tokens]
        self.n_atoms = self.n_scan_atoms = len(ps.rules)
        self.atom_rule0 = 0
        self._tuples = [(n, e, list(a) if isinstance(a, (list, tuple)) else [a]) for n, e, a in ps.rules]
        self.rules = [(n, [[(k, False)]], a) for k, (n, _, a) in enumerate(self._tuples)]
        self.lists = {}
        self.routes = [(f"r{j}", [[((j * 17) % self.n_atoms, False)]]) for j in range(12)]

    def rule_tuples(self):
        return self._tuples

    def route_tuples(self):
        return [(n, f'http_request.url.contains("{self.words[d[0][0][0]]}")') for n, d in self.routes]

    def truth(self, groups):
        T = np.zeros((self.n_atoms, sum(g.lanes for g in groups)), dtype=bool)
        at = 0
        for g in groups:
            for l, atoms in enumerate(g.words):
                T[atoms, at + l] = True
            at += g.lanes
        return T

    def make_batch(self, groups):
        ver = verified(groups)
        reqs = []
        for g in groups:
            for l in range(g.lanes):
                u = "/" + "/".join(self.words[a] for a in g.words[l])
                reqs.append(Request(url=u, path="/__pingoo/captcha/x" if g.gate[l] == 2 else "/p", host="h.example", user_agent="ua/1", method="GET", ip="192.0.2.1",
                                    remote_port=PORT_NONE, captcha_verified=bool(ver[len(reqs)])))
        return RequestBatch.from_requests(reqs)

    def gate_pass(self, tabs):
        """the one pass that holds no rule's atom: the path prefix of the captcha endpoint's gate (the last pass)"""
        (ps,) = [k for k, p in enumerate(tabs.groups) if p["field"] == 2]
        assert ps == len(tabs.groups) - 1 and tabs.groups[ps]["n_atoms"] == 1
        return ps

    def extra_columns(self, g, tabs):
        ps = self.gate_pass(tabs)
        return [(ps, int(tabs.groups[ps]["atom_base"]))] if (g.gate == 2).any() else []

    def pass_of_atoms(self, flags=0):
        _, tabs = self.tables(flags)
        cols = column_of_atoms(self, flags)
        lo = np.array([p["atom_base"] for p in tabs.groups])
        return np.searchsorted(lo, cols, side="right") - 1


def pass_groups(rs):
    """groups by the number of scan passes with a hit: none, one, kPre, kPre + 1, (65 passes) 13, every pass; all the atoms at once"""
    ps_of = rs.pass_of_atoms()
    n_p = rs.n_passes
    assert rs.gate_pass(rs.tables(0)[1]) == n_p - 1 and set(ps_of.tolist()) == set(range(n_p - 1)), "every pass but the gate's holds an atom of some rule"
    rep = [int(np.nonzero(ps_of == p)[0][0]) for p in range(n_p - 1)] + [-1]  # (-1: the gate's pass, hit by a request under /__pingoo/captcha)
    k_pre = globals()["k_pre"](n_p)

    def over(kind, atoms, lanes=64, two=False):
        g = Group(kind, lanes)
        g.words = [[] for _ in range(lanes)]
        for i, a in enumerate(atoms):
            if a < 0:
                g.gate[lanes - 1] = 2
            else:
                g.words[(i // 2 if two else i) % (lanes - 1)].append(a)
        return g

    gs = [over("nothing", []), over("one pass", rep[:1]), over("last pass", rep[-1:]), over(f"{k_pre} passes", rep[:k_pre]), over(f"{k_pre + 1} passes", rep[n_p - k_pre - 1:])]
    if n_p > 64:
        gs += [over("13 passes", rep[5:18]), over("passes 0, 63 and 64", [rep[0], rep[63], rep[64]])]
        # every rule is one atom and no rule is a candidate of every group: the candidate list is the distinct atoms that hold
        gs += [over(f"{k} atoms", list(range(k)), two=True) for k in (64, 65)]
        # 129: atoms 63, 64 and 128 (list positions 63, 64 and last) alone on lanes of their own — 64's rule is CAPTCHA-only: on three lanes,
        # two of them not verified — the others spread so that a lane's atoms lie in different passes
        g = over("129 atoms", [])
        g.words[0], g.words[1], g.words[2], g.words[3], g.words[4] = [63], [64], [64], [64], [128]
        for i, a in enumerate(a for a in range(129) if a not in (63, 64, 128)):
            g.words[5 + i % 59].append(a)
        gs.append(g)
    gs += [over("every pass", rep), over("every atom", list(range(rs.n_atoms)), two=True), over("every second atom", list(range(0, rs.n_atoms, 2))), over("nothing2", []),
           over("partial", rep[1:3], lanes=37)]
    return gs


class LazySet(RuleSet):
    """set Z: a token beside a comparison of the path's length or of the port — the planner keeps such comparisons LAZY (no column: the
    verdict kernel evaluates them per request when the rule's other literals hold), one variable per lazy slot — with ==, <= and both
    negated; and 70 residual rules (arithmetic on the port: outside the column compiler): three result words per request, and enough for
    one group's residual entries to carry the batch registers through 64. Atoms 0 .. 7: the tokens (url); 8 .. 13: the comparisons, in CMP's
    order (lazy: no column); 14 .. 83: remote_port % 97 == k, whose columns are the residual rules' (residual_base + k)."""
    CMP = (("http_request.path.length() == 20", lambda ln, port: ln == 20), ("http_request.path.length() <= 12", lambda ln, port: ln <= 12),
           ("client.remote_port == 4444", lambda ln, port: port == 4444), ("client.remote_port <= 1000", lambda ln, port: port <= 1000),
           ("http_request.path.length() <= 30", lambda ln, port: ln <= 30), ("client.remote_port == 5555", lambda ln, port: port == 5555))
    N_WORDS, N_RES = 8, 70

    def __init__(self):
        self.name, self.opts, self.lists = "Z", {}, {}
        self.words = H.pass_words(977, self.N_WORDS)
        self.n_scan_atoms = self.N_WORDS
        self.n_atoms = self.N_WORDS + len(self.CMP) + self.N_RES
        c0, r0 = self.N_WORDS, self.N_WORDS + len(self.CMP)
        # token && comparison; the last two negated
        self.rules = [(f"z{k}", [[(k, False), (c0 + k, k >= 4)]], [[B], [B], [CAP, B], [B], [B], [CAP]][k]) for k in range(len(self.CMP))]
        self.rules += [(f"res{k}", [[(r0 + k, False)]], ACTIONS[k % 3]) for k in range(self.N_RES)]
        self.rules += [(f"t{k}", [[(k, False)]], [CAP]) for k in range(self.N_WORDS)]
        self.routes = [(f"r{j}", [[(j % self.N_WORDS, False)]]) for j in range(12)]
        self.residual_atoms = range(r0, r0 + self.N_RES)

    def atom_rule(self, a):
        """the rule that holds atom a alone (None: a lazy comparison, which has no column)"""
        n_cmp = len(self.CMP)
        return n_cmp + self.N_RES + a if a < self.N_WORDS else None if a < self.N_WORDS + n_cmp else n_cmp + a - self.N_WORDS - n_cmp

    def text(self, a):
        if a < self.N_WORDS:
            return f'http_request.url.contains("{self.words[a]}")'
        if a < self.N_WORDS + len(self.CMP):
            return "(" + self.CMP[a - self.N_WORDS][0] + ")"
        return f"client.remote_port % 97 == {a - self.N_WORDS - len(self.CMP)}"

    def rule_tuples(self):
        return [(n, " && ".join(("!" if neg else "") + self.text(a) for a, neg in d[0]), list(acts)) for n, d, acts in self.rules]

    def route_tuples(self):
        return [(n, self.text(d[0][0][0])) for n, d in self.routes]

    def truth(self, groups):
        T = np.zeros((self.n_atoms, sum(g.lanes for g in groups)), dtype=bool)
        at = 0
        for g in groups:
            for l in range(g.lanes):
                T[g.words[l], at + l] = True
                for k, (_, f) in enumerate(self.CMP):
                    T[self.N_WORDS + k, at + l] = f(int(g.path_len[l]), int(g.port[l]))
                if g.port[l] % 97 < self.N_RES:
                    T[self.N_WORDS + len(self.CMP) + int(g.port[l]) % 97, at + l] = True
            at += g.lanes
        return T

    def make_batch(self, groups):
        ver = verified(groups)
        reqs = []
        for g in groups:
            for l in range(g.lanes):
                reqs.append(Request(url="/" + "/".join(self.words[a] for a in g.words[l]), path="/" + "p" * (int(g.path_len[l]) - 1), host="h.example", user_agent="ua/1", method="GET",
                                    ip="192.0.2.1", remote_port=int(g.port[l]), captcha_verified=bool(ver[len(reqs)])))
        return RequestBatch.from_requests(reqs)


def lazy_groups(rs):
    """lane -> (tokens, path length, port). Ports are 97 m + 70 .. 96 where no residual rule is meant to hold."""
    quiet = 97 * 60 + 80

    def grp(kind, spec, lanes=64):
        g = Group(kind, lanes)
        g.words = [[] for _ in range(lanes)]
        g.path_len = np.full(lanes, 40, dtype=np.int64)
        g.port = np.full(lanes, quiet, dtype=np.int64)
        for l, (w, ln, port) in spec.items():
            g.words[l], g.path_len[l], g.port[l] = list(w), ln, port
        return g

    hits = {0: ([0], 20, quiet), 1: ([0], 19, quiet), 2: ([2], 40, 4444), 3: ([2], 40, 4445), 4: ([3], 40, 1000), 5: ([3], 40, 1001 + 96), 6: ([5], 40, 5555), 7: ([5], 40, 5556 + 60),
            8: ([1], 12, quiet), 9: ([1], 13, quiet), 10: ([4], 31, quiet), 11: ([4], 30, quiet), 12: ([0, 1, 2, 3, 4, 5], 20, 4444), 13: ([6], 40, quiet), 14: ([0, 7], 21, quiet), 63: ([4], 31, quiet)}
    gs = [grp("lane 0 of group 0", {0: ([0], 20, quiet), 63: ([1], 12, quiet)}), grp("nothing", {}),
          grp("lane 0 of a later group", {0: ([1], 12, quiet), 1: ([0], 19, quiet), 63: ([4], 31, quiet)}),
          grp("every comparison", hits),
          grp("residual rules", {l: ([], 40, 97 * (3 + l // 40) + (l + 6) % 70) for l in range(64)}),  # (rules 6 .. 69: all three result words)
          grp("every comparison and residual rules", {**{l: ([l % 8], 20 + l % 3, 97 * 7 + l % 50) for l in range(16, 63)}, **hits}),
          # 8 tokens in the batch registers, then 64 distinct residual rules: the 56th residual entry fills them
          grp("residual entries through 64", {l: ([l] if l < 8 else [], 40, 97 * 5 + l) for l in range(64)}),
          grp("nothing2", {}),
          grp("partial", {0: ([2], 40, 4444), 36: ([0], 20, quiet)}, lanes=37)]
    return gs


@functools.lru_cache(maxsize=None)
def rule_set(name):
    if name == "Z":
        return LazySet()
    return {"A": lambda: RuleSet("A", compound_a(), 0), "H": lambda: RuleSet("H", compound_h(), 0), "C": lambda: RuleSet("C", compound_c(), 1), "W": lambda: RuleSet("W", compound_w(), 2),
            "P8": lambda: PassSet(8), "P65": lambda: PassSet(65)}[name]()


# ---------------------------------------------------------------------------------------------------------
# groups: per lane the address, the port and the tokens of every field
# ---------------------------------------------------------------------------------------------------------
class Group:
    def __init__(self, kind, lanes=64):
        self.kind, self.lanes = kind, lanes
        self.ip = np.full(lanes, IP_NONE, dtype=np.int64)
        self.port = np.full(lanes, PORT_NONE, dtype=np.int64)
        self.tok = [[[] for _ in range(lanes)] for _ in FIELDS]  # token indices (0 .. N_TOK - 1) per field and lane
        self.gate = np.zeros(lanes, dtype=np.int64)  # 1: an empty user agent (the UA gate blocks it), 2: a path under /__pingoo/captcha (bypass)


def group(kind, n_pairs=0, s=(0, 0, 0, 0), rot=0, lanes=64, chains=None, first_lane=0):
    """a group with exactly n_pairs attribute atoms that hold for somebody and s[f] distinct tokens in field f, at most two per lane and
    field. chains: {field: [[token, ...] per lane]} replaces that field's lanes (three or more tokens on a lane: an overflow chain).
    first_lane: the lane that gets the first atoms (63: the deciding request in the last lane)."""
    g = Group(kind, lanes)
    order = [(first_lane + q) % lanes for q in range(lanes)]
    n_ip = min(n_pairs, 2 * min(lanes, 64))
    n_port = n_pairs - n_ip
    assert n_port <= N_PORT and n_port <= 2 * lanes, (kind, n_pairs)
    for q in range(n_ip // 2):
        g.ip[order[q]] = (10 << 24) | (1 << 16) | (((rot + q) % N_SHARED_IP) << 8) | 7
    if n_ip % 2:
        g.ip[order[n_ip // 2]] = (10 << 24) | ((2 * ((rot + n_ip // 2) % N_SHARED_IP)) << 8) | 9
    for q in range(n_port // 2):
        g.port[order[q]] = 3000 + (rot + q) % N_SHARED_PORT
    if n_port % 2:
        g.port[order[n_port // 2]] = 2000 + 2 * ((rot + n_port // 2) % N_SHARED_PORT)
    for f in range(4):
        assert s[f] <= N_TOK and s[f] <= 2 * lanes, (kind, s)
        for i in range(s[f]):
            g.tok[f][order[i // 2]].append((rot + i) % N_TOK)
    for f, per_lane in (chains or {}).items():
        g.tok[f] = [list(t) for t in per_lane] + [[] for _ in range(lanes - len(per_lane))]
    return g


def truth(groups):
    """T[atom, request] of the groups laid one behind the other"""
    n = sum(g.lanes for g in groups)
    T = np.zeros((N_ATOMS, n), dtype=bool)
    at = 0
    for g in groups:
        for f in range(4):
            for l, toks in enumerate(g.tok[f]):
                for t in toks:
                    T[f * N_TOK + t, at + l] = True
        own, shared = (g.ip >> 16) == ((10 << 8) | 0), (g.ip >> 16) == ((10 << 8) | 1)
        third = (g.ip >> 8) & 255
        for l in range(g.lanes):
            if own[l]:
                T[A_IP + third[l], at + l] = True
            if shared[l]:
                T[A_IP + 2 * third[l], at + l] = T[A_IP + 2 * third[l] + 1, at + l] = True
            p = int(g.port[l])
            if 2000 <= p < 2000 + N_PORT:
                T[A_PORT + p - 2000, at + l] = True
            if 3000 <= p < 3000 + N_SHARED_PORT:
                T[A_PORT + 2 * (p - 3000), at + l] = T[A_PORT + 2 * (p - 3000) + 1, at + l] = True
        at += g.lanes
    return T


def gates(groups):
    return np.concatenate([g.gate for g in groups])


def verified(groups):
    return np.concatenate([(np.arange(g.lanes) + k) % 3 == 0 for k, g in enumerate(groups)])


def make_batch(rs, groups):
    w = rs.words
    reqs = []
    ver = verified(groups)
    for g in groups:
        for l in range(g.lanes):
            vals = [[w[f * N_TOK + t] for t in g.tok[f][l]] for f in range(4)]
            ip = int(g.ip[l])
            gate = int(g.gate[l])
            assert gate != 1 or not vals[3], "a request with an empty user agent carries no user-agent token"
            reqs.append(Request(url="/" + "/".join(vals[0]), path=("/__pingoo/captcha/" if gate == 2 else "/") + "/".join(vals[1]), host=".".join(vals[2] + ["example"]),
                                user_agent="" if gate == 1 else "ua/1 " + " ".join(vals[3]), method="GET",
                                ip=f"{ip >> 24}.{(ip >> 16) & 255}.{(ip >> 8) & 255}.{ip & 255}", remote_port=int(g.port[l]), captcha_verified=bool(ver[len(reqs)])))
    return RequestBatch.from_requests(reqs)


# ---------------------------------------------------------------------------------------------------------
# the reference: numpy from the rule list
# ---------------------------------------------------------------------------------------------------------
def holds(dnf, T):
    if dnf is None:
        return np.ones(T.shape[1], dtype=bool)
    out = np.zeros(T.shape[1], dtype=bool)
    for term in dnf:
        t = np.ones(T.shape[1], dtype=bool)
        for a, neg in term:
            t &= ~T[a] if neg else T[a]
        out |= t
    return out


def reference(rs, T, ver, gate=None):
    """-> (verdicts as VERDICT_DTYPE-like dict of arrays, counters, hit matrix [rule, request], first route or -1). gate: per request 1 =
    the UA gate answers (BLOCK), 2 = the captcha endpoint's bypass (behind the UA gate); such a request matches no rule in the hit matrix."""
    n = T.shape[1]
    gate = np.zeros(n, dtype=np.int64) if gate is None else gate
    action = np.where(gate == 1, _abi.ACTION_BLOCK, np.where(gate == 2, _abi.ACTION_BYPASS, _abi.ACTION_ALLOW)).astype(np.uint8)
    rule = np.where(gate == 1, _abi.RULE_UA_GATE, np.where(gate == 2, _abi.RULE_CAPTCHA_ENDPOINT, _abi.RULE_NONE)).astype(np.uint32)
    open_ = gate == 0
    M = np.zeros((len(rs.rules), n), dtype=bool)
    for k, (_, dnf, acts) in enumerate(rs.rules):
        M[k] = h = holds(dnf, T) & (gate == 0)
        for a in acts:  # the actions in order: BLOCK takes effect for everybody, CAPTCHA for the requests that are not verified
            eff = h & open_ & (~ver if a == CAP else True)
            action[eff] = _abi.ACTION_CAPTCHA if a == CAP else _abi.ACTION_BLOCK
            rule[eff] = k
            open_ &= ~eff
    route = np.full(n, -1, dtype=np.int32)
    for j in reversed(range(len(rs.routes))):
        route[holds(rs.routes[j][1], T)] = j
    return {"action": action, "rule_idx": rule}, np.bincount(action, minlength=4), M, route


# ---------------------------------------------------------------------------------------------------------
# the group model
# ---------------------------------------------------------------------------------------------------------
class GroupModel:
    """One group under one program (flags) and capacity. events: [(site, first entry, count, chained)] in the kernel's order — site 1 =
    append_batch from the batch registers, 2 = merge_or_append, 3 = append_batch of the pairs beyond the first 64."""

    def __init__(self, rs, flags, g, e_cap):
        plan, tabs = rs.tables(flags)
        cols = column_of_atoms(rs, flags)
        Tg = rs.truth([g])
        true_atoms = np.nonzero(Tg.any(axis=1))[0]
        attr_cols = sorted({int(cols[a]) for a in true_atoms if a >= rs.n_scan_atoms and cols[a] >= 0 and a not in rs.residual_atoms})
        res_cols = sorted({int(cols[a]) for a in true_atoms if a in rs.residual_atoms})
        self.n_residual = len(res_cols)
        self.n_pairs = len(attr_cols)
        pass_lo = np.array([p["atom_base"] for p in tabs.groups])
        pass_hi = pass_lo + np.array([p["n_atoms"] for p in tabs.groups])
        self.passes = []  # (pass, distinct columns of plain lanes, distinct columns of chained lanes, chained lanes)
        for ps in range(len(tabs.groups)):
            in_pass = [a for a in range(rs.n_scan_atoms) if pass_lo[ps] <= cols[a] < pass_hi[ps]]
            if not in_pass:
                continue
            per_lane = Tg[in_pass].sum(axis=0)
            if not per_lane.any():
                continue
            chained = per_lane >= 3
            plain = {int(cols[a]) for a in in_pass if Tg[a][~chained].any()}
            chain = {int(cols[a]) for a in in_pass if Tg[a][chained].any()}
            self.passes.append((ps, plain, chain, int(chained.sum())))
        for ps, col in rs.extra_columns(g, tabs):  # (atoms outside the rules' truth table that the group is built to hit: a gate's)
            self.passes.append((ps, {col}, set(), 0))
        self.passes.sort(key=lambda q: q[0])
        self.events, self.merges = [], []  # merges: (column, "lds" | "spill") of chain atoms OR-ed into an entry that exists
        n, bn = 1, min(self.n_pairs, 64)
        self.bn_through_64_by = set()

        def flush(why):
            nonlocal n, bn
            if bn:
                self.events.append((1, n, bn, False))
                n += bn
                bn = 0

        if bn == 64:
            flush("pairs")
        for ps, plain, chain, n_ch in self.passes:
            if n_ch:
                flush("chain")
                for c in sorted(plain):
                    self.events.append((2, n, 1, False))
                    n += 1
                first_of = {c: k for k, c in enumerate(sorted(plain))}
                base = n - len(plain)
                for c in sorted(chain):
                    if c in plain:
                        self.merges.append((c, "lds" if base + first_of[c] < e_cap else "spill"))
                    else:
                        self.events.append((2, n, 1, True))
                        n += 1
            else:
                for _ in plain:
                    bn += 1
                    if bn == 64:
                        self.bn_through_64_by.add("pass")
                        flush("full")
        for _ in res_cols:  # step 2b: one entry per residual rule that matched anybody, through the batch registers
            bn += 1
            if bn == 64:
                self.bn_through_64_by.add("residual")
                flush("full")
        flush("end")
        for p0 in range(64, self.n_pairs, 64):
            cnt = min(64, self.n_pairs - p0)
            self.events.append((3, n, cnt, False))
            n += cnt
        self.n_entries, self.e_cap = n, e_cap
        self.spilled = n > e_cap
        self.columns = set(attr_cols) | set(res_cols) | {c for _, p, ch, _ in self.passes for c in p | ch}
        assert n == 1 + len(self.columns)
        self.spilled_columns = set()
        # candidates: the always-bitmap, column 0's trigger list, the trigger list of every appended column
        bm = set(np.nonzero(np.unpackbits(plan.always.view(np.uint8), bitorder="little"))[0].tolist())
        for c in self.columns | {0}:
            bm.update(int(r) for r in plan.trig_rules[int(plan.trig_off[c]):int(plan.trig_off[c + 1])])
        self.cand = sorted(bm)
        self.n_cand = len(self.cand)
        self.last_site = self.events[-1][0] if self.events else 0
        self.last_chained = bool(self.events and self.events[-1][3])
        self.straddle = any(site != 2 and first < e_cap < first + cnt for site, first, cnt, _ in self.events)
        self.spill_by_chain = any(site == 2 and ch and first == e_cap for site, first, cnt, ch in self.events)
        self.state = "spilled" if self.spilled else "full" if n == e_cap else "clean"


@functools.lru_cache(maxsize=None)
def column_of_atoms(rs, flags):
    plan, _ = rs.tables(flags)
    cols = np.zeros(rs.n_atoms, dtype=np.int64)
    by_pub = {int(r["public_idx"]): r for r in plan.rules}
    for k in range(rs.n_atoms):
        if rs.atom_rule(k) is None:
            cols[k] = -1
            continue
        r = by_pub[rs.atom_rule(k)]
        assert r["lit_cnt"] == 1, f"atom rule {k} has {r['lit_cnt']} literals"
        lit = int(plan.dev_lits[int(r["lit_off"])])
        assert not lit & (LIT_NEG | LIT_LAZY) and lit & LIT_TERM_END, hex(lit)
        cols[k] = lit & LIT_ATOM_MASK
    have = cols[cols >= 0]
    assert len(set(have.tolist())) == len(have) and have.min() >= 1, "every atom has a column of its own"
    if len(rs.residual_atoms):  # the residual rules' columns, in rule order from the dump's residual base
        (n_res, base), = [np.frombuffer(pl, dtype="<u4")[:2] for tag, _, pl in parse_dump(rs.program(flags).dump()) if tag == "RSDL"]
        assert n_res == len(rs.residual_atoms) and cols[list(rs.residual_atoms)].tolist() == list(range(int(base), int(base) + int(n_res)))
    return cols


# ---------------------------------------------------------------------------------------------------------
# the base batches
# ---------------------------------------------------------------------------------------------------------
def spread(total):
    """`total` distinct tokens over the four fields, the first field full first (its pass then carries the batch registers through 64)"""
    s, left = [], total
    for _ in range(4):
        s.append(min(N_TOK, left))
        left -= s[-1]
    assert left == 0, total
    return tuple(s)


def capacity_groups(cap, tag, chain_field=None):
    """groups around capacity `cap`: n_entries = cap - 1, cap, cap + 1 with the last append at site 1 and (cap > 66) at site 3, a
    straddling append_batch; with chain_field (set C) also at site 2"""
    out = []
    for d in (-1, 0, 1):
        e = cap + d
        p = min(10, max(0, e - 2))
        out.append(group(f"{tag}site1{d:+d}", n_pairs=p, s=spread(e - 1 - p), rot=3 * (d + 1)))
        out.append(group(f"{tag}scan{d:+d}", s=spread(e - 1), rot=31 + 5 * d))  # (scan entries alone; a second exactly full group for the turns)
        if cap > 140:  # the pairs beyond 64 come last: 129 pairs, the 129th alone in step 3's second append_batch
            out.append(group(f"{tag}site3{d:+d}", n_pairs=129, s=spread(e - 1 - 129), rot=11 + d))
            out.append(group(f"{tag}site3b{d:+d}", n_pairs=65 + 30, s=spread(e - 1 - 95), rot=20 + d))
        if chain_field is not None:
            # the last append is a chain's: every atom of the chained field's pass sits on lanes with three tokens; the other fields fill up
            n_chain = 6
            rest = e - 1 - n_chain
            p2 = min(40, max(0, rest - 3 * N_TOK)) if rest > 3 * N_TOK else 0
            s = list(spread_without(rest - p2, chain_field))
            out.append(group(f"{tag}site2{d:+d}", n_pairs=p2, s=tuple(s), rot=5 + d, chains={chain_field: [[40, 41, 42], [43, 44, 45]]}))
    return out


def spread_without(total, skip):
    s, left = [0, 0, 0, 0], total
    for f in range(4):
        if f != skip:
            s[f] = min(N_TOK, left)
            left -= s[f]
    assert left == 0, (total, skip)
    return s


def base_groups(rs, e_caps, chain_field=None):
    """the ordered list of group kinds of a set's base batch (the last group is partial)"""
    gs = [group("nothing"), group("one-pair", n_pairs=1), group("one-token", s=(1, 0, 0, 0), first_lane=63), group("few", n_pairs=3, s=(2, 1, 2, 1), rot=9)]
    for p in (63, 64, 65, 128, 129):
        gs.append(group(f"pairs{p}", n_pairs=p, rot=p % 7))
        gs.append(group(f"pairs{p}+scan", n_pairs=p, s=(3, 2, 0, 1), rot=p % 5))
    gs.append(group("pairs1+scan", n_pairs=1, s=(2, 0, 1, 0), rot=30))
    for cap in sorted(e_caps, reverse=True):  # (the capacities of the set's legs: as built, with global tables, with 8 slots)
        gs += capacity_groups(cap, f"cap{cap}:", chain_field)
    gs.append(group("heavy", n_pairs=100, s=(N_TOK, N_TOK, N_TOK, N_TOK), rot=1))
    gs.append(group("heavy2", n_pairs=70, s=(N_TOK, 60, N_TOK, 50), rot=37))
    gs.append(group("every-pass", n_pairs=0, s=(2, 2, 2, 2), rot=50))
    # one token of each compound rule behind the atoms, on three lanes (one of them verified: where the atom's own rule is CAPTCHA-only, the
    # compound rule decides it)
    lanes = {f: [[] for _ in range(64)] for f in range(4)}
    for q in range(20):
        a = ((20 + q) * 7) % (4 * N_TOK)
        for l in range(3 * q, 3 * q + 3):
            lanes[a // N_TOK][l].append(a % N_TOK)
    gs.append(group("compound", chains=lanes))
    if chain_field is not None:
        f = chain_field
        # a chained lane beside plain lanes that name its columns; two chained lanes with the same atoms, and shifted by one
        gs.append(group("chain+plain", n_pairs=2, s=(1, 1, 1, 1), rot=2, chains={f: [[10, 11, 12, 13, 14], [12, 20], [10, 11, 12], [11, 12, 13], [14], [10, 11, 12]]}))
        # the same behind a group that has spilled already when the chained pass comes (the chain's atoms merge into spilled entries)
        full = [N_TOK, N_TOK, N_TOK, N_TOK]
        gs.append(group("chain-merge-spilled", n_pairs=64, s=tuple(full), rot=0, chains={f: [[10, 11, 12, 13, 14], [12, 20], [10, 11, 12], [11, 12, 13], [14], [10, 11, 12]] + [[21 + 2 * q, 22 + 2 * q] for q in range(25)]}))
    g = group("gates", n_pairs=4, s=(2, 2, 1, 0), rot=17)  # lanes the gate pseudo rules answer (device rules 0 and 1: candidate positions 0 and 1)
    g.gate[[0, 5, 63]] = 1
    g.gate[[1, 6, 62]] = 2
    g.inexact = True  # (the gates' own atoms — a length, a path prefix — are not in the model's truth table)
    gs.append(g)
    if rs.name == "W":
        lanes = {f: [[] for _ in range(64)] for f in range(4)}
        combos = ([], [W_B], [W_B, W_Z], [W_B, W_Z, W_A], [W_B, W_Z, W_A, W_Q], [W_Z], [W_Q, W_A], [W_B, W_Z, W_A, W_Q, W_IP])
        for q, toks in enumerate(combos):
            for l in range(6 * q, 6 * q + 6):
                for a in toks:
                    if a < A_IP:
                        lanes[a // N_TOK][l].append(a % N_TOK)
        for kind, n_pairs in (("bitmap-edges", 0), ("bitmap-edges+heavy", 80)):
            g = group(kind, n_pairs=n_pairs, rot=3, chains=lanes, first_lane=6 * len(combos))
            g.ip[6 * len(combos) - 6:6 * len(combos)] = (10 << 24) | ((W_IP - A_IP) << 8) | 5  # the last combination: inside ip list 1's own /24
            gs.append(g)
    gs.append(group("nothing2"))
    gs.append(group("partial", n_pairs=2, s=(1, 0, 0, 1), rot=4, lanes=37, first_lane=36))
    return gs


class Case:
    def __init__(self, name, rs, groups, chain_field=None):
        self.name, self.rs, self.groups, self.chain_field = name, rs, groups, chain_field
        self.T = rs.truth(groups)
        self.ver = verified(groups)
        self.gate = gates(groups)
        self.want, self.counts, self.M, self.route = reference(rs, self.T, self.ver, self.gate)

    @functools.cached_property
    def batch(self):
        return self.rs.make_batch(self.groups)

    @functools.lru_cache(maxsize=None)
    def models(self, flags=0):
        cap = self.rs.program(flags).verdict_shape()["capacity"]
        return [GroupModel(self.rs, flags, g, cap) for g in self.groups]


def last_pass_field(rs):
    """the token field whose atoms lie in the LAST scan pass (its chains come when the other passes' entries are appended)"""
    _, tabs = rs.tables(0)
    cols = column_of_atoms(rs, 0)
    last = max(range(4), key=lambda f: max(cols[f * N_TOK:(f + 1) * N_TOK]))
    return last


@functools.lru_cache(maxsize=None)
def case(name):
    rs = rule_set(name)
    if isinstance(rs, PassSet):
        return Case(name, rs, pass_groups(rs))
    if isinstance(rs, LazySet):
        return Case(name, rs, lazy_groups(rs))
    e_caps = {rs.program(flags).verdict_shape()["capacity"] for flags in (0, GLOBAL, HITS, TINY, TINY | GLOBAL)}
    cf = last_pass_field(rs) if name == "C" else None
    return Case(name, rs, base_groups(rs, e_caps, cf), cf)


def targets(c, flags):
    """{target: bool} for the case under the program with `flags` (the capacity is the shape hook's)"""
    if isinstance(c.rs, LazySet):
        return lazy_targets(c, flags)
    ms = c.models(flags)
    cap = ms[0].e_cap
    t = {}
    if isinstance(c.rs, PassSet):
        sh = c.rs.program(flags).verdict_shape()
        n_p, k_pre = c.rs.n_passes, globals()["k_pre"](c.rs.n_passes)
        t[f"{n_p} passes select the instantiation with {1 if n_p <= 64 else 4} bitmap registers"] = (sh["n_passes"], sh["bit_regs"]) == (n_p, 1 if n_p <= 64 else 4)
        for k in (0, 1, k_pre, k_pre + 1, n_p) + ((13,) if n_p > 64 else ()):
            t[f"{k} non-empty passes in a group"] = any(len(m.passes) == k for m in ms)
        t["more non-empty passes than are requested a group ahead: the rest loop"] = any(len(m.passes) > k_pre for m in ms)
        for p in (0, n_p - 1) + ((63, 64) if n_p > 64 else ()):
            t[f"a hit in pass {p}"] = any(p in [q[0] for q in m.passes] for m in ms)
        t["a spilled group under 8 slots"] = flags & TINY == 0 or any(m.spilled for m in ms)
        t["candidate lists of 0 and of 1"] = {0, 1} <= {m.n_cand for m in ms}
        if n_p > 64:
            t["candidate lists of exactly 64, 65 and 129"] = {64, 65, 129} <= {m.n_cand for m in ms}
            pos, last = deciding_positions(c, flags)
            t["the deciding candidate at list positions 0, 63, 64 and last"] = {0, 63, 64} <= pos and last > 0
        return t
    for d in (-1, 0, 1):
        t[f"entries cap{d:+d} by append_batch of the batch registers"] = any(m.n_entries == cap + d and m.last_site == 1 for m in ms)
        if cap > 140:
            t[f"entries cap{d:+d} by the pairs beyond 64"] = any(m.n_entries == cap + d and m.last_site == 3 for m in ms)
        if c.chain_field is not None:
            t[f"entries cap{d:+d} by merge_or_append behind a chain"] = any(m.n_entries == cap + d and m.last_site == 2 and m.last_chained for m in ms)
    t["one append_batch straddles the capacity"] = any(m.straddle for m in ms)
    t["a group of one entry"] = any(m.n_entries == 1 for m in ms)
    t["a group of two entries"] = any(m.n_entries == 2 for m in ms)
    for p in (0, 1, 63, 64, 65, 128, 129):
        t[f"n_pairs {p} without scan entries"] = any(m.n_pairs == p and not m.passes for m in ms)
        t[f"n_pairs {p} with scan entries"] = any(m.n_pairs == p and m.passes for m in ms)
    t["a pass carries the batch registers through 64"] = any("pass" in m.bn_through_64_by for m in ms)
    for k in (0, 1, K_PRE):
        t[f"{k} non-empty passes"] = any(len(m.passes) == k for m in ms)
    t["spilled, full and clean groups"] = {m.state for m in ms} == {"spilled", "full", "clean"}
    t["a candidate list within one chunk of 64"] = any(m.n_cand <= 64 for m in ms)
    t["a candidate list of two chunks"] = any(64 < m.n_cand <= 128 for m in ms)
    t["a candidate list of more than two chunks"] = any(m.n_cand > 128 for m in ms)
    pos, last = deciding_positions(c, flags)
    for p in (0, 63, 64):
        t[f"the deciding candidate at list position {p}"] = p in pos
    if c.name == "H":
        plan, _ = c.rs.tables(flags)
        plain, _ = c.rs.tables(flags & ~HITS)
        observe = [k for k, (_, _, acts) in enumerate(c.rs.rules) if not acts]
        kept = set(plan.rules["public_idx"].tolist())
        t["the rule-hits program keeps the rules without actions as device rules, the others drop them"] = (
            len(observe) == N_OBSERVE and (all(k in kept for k in observe) if flags & HITS else not any(k in kept for k in observe))
            and len(plan.rules) - len(plain.rules) == (N_OBSERVE if flags & HITS else 0))
        t["every rule without actions matches somebody and decides nobody"] = all(c.M[k].any() for k in observe) and not np.isin(c.want["rule_idx"], observe).any()
        t["a rule without actions matches a request that no rule decides otherwise than it would"] = any((c.M[k] & (c.want["rule_idx"] > k)).any() for k in observe)
    if c.name != "C":  # (set C has no rule behind its negation-only rules)
        t["the deciding candidate last in the list"] = last > 0
    if c.name == "W":
        plan, _ = c.rs.tables(flags)
        always = set(np.nonzero(np.unpackbits(plan.always.view(np.uint8), bitorder="little"))[0].tolist())
        n_dev = len(plan.rules)
        t["more than 2048 device rules"] = n_dev > 2048 + 32
        t["negation-only rules at device indices 2047 and 2048 and in the last bitmap word"] = {2047, 2048} <= always and any(r // 32 == (n_dev - 1) // 32 for r in always)
        decided = {int(plan_dev(plan, r)) for r in set(c.want["rule_idx"].tolist()) if r < 0xFFFFFFF0}
        t["deciding rules at device indices 2047, 2048, 2049 and three in the last word"] = {2047, 2048, 2049} <= decided and sum(1 for r in decided if r // 32 == (n_dev - 1) // 32) >= 3
        t["a candidate list that reaches the second round of the compaction"] = any(m.cand[-1] >= 2048 for m in ms)
        t["a match-all rule filed under column 0"] = int(plan.trig_off[1]) > int(plan.trig_off[0]) and n_dev - 1 in [int(r) for r in plan.trig_rules[int(plan.trig_off[0]):int(plan.trig_off[1])]]
    if c.chain_field is not None:
        t["a chain atom merged into an LDS entry"] = any(("lds" in [w for _, w in m.merges]) for m in ms)
        t["a chain atom merged into a spilled entry"] = any(("spill" in [w for _, w in m.merges]) for m in ms)
        t["a chain appends the entry that spills"] = any(m.spill_by_chain for m in ms)
        # A chain is a stack (csrc/hitrec.h: record_atom, csrc/confirm.hip: merge_atom push at the head): a lane that walks its field alone leaves its atoms in
        # the reverse of their order in the field. Two lanes with the same tokens in the same order then name every atom at the same step; two
        # lanes of equal length whose tokens are shifted name a common atom at different steps — in field order or its reverse alike. (Behind
        # the confirm tier several chunk lanes push one request's atoms and the order is the device's: the no-prefilter leg walks alone.)
        chained = [tuple(l) for g in c.groups for l in g.tok[c.chain_field] if len(l) >= 3]
        t["two chained lanes name the same atoms at the same steps"] = any(chained.count(l) >= 2 for l in chained)
        t["two chained lanes name an atom at different steps"] = any(len(x) == len(y) and any(a in y and y.index(a) != i for i, a in enumerate(x)) for x in chained for y in chained)
        t["a chained lane beside plain lanes"] = any(any(n_ch and plain & chain for _, plain, chain, n_ch in m.passes) for m in ms)
    return t


def lazy_targets(c, flags):
    """set Z has no group model: its targets are read from the plan (what is lazy, the residual words) and from the reference (which
    request a rule with a lazy comparison decides, by lane)"""
    plan, _ = c.rs.tables(flags)
    n_cmp = len(c.rs.CMP)
    t = {}
    lazy = [int(x) for x in plan.dev_lits if x & LIT_LAZY]
    t["both lazy slots in use: a length and the port"] = sorted(plan.lazy_vars) == [2, 5] and {(x >> 17) & 1 for x in lazy} == {0, 1}
    t["every comparison of the rules is lazy"] = plan.n_lazy == n_cmp  # (the eager comparison atoms left are the UA gate's)
    t["lazy == and <="] = {(x >> 16) & 1 for x in lazy} == {0, 1}
    t["a negated lazy literal"] = any(x & LIT_NEG for x in lazy) or any((x >> 18) & 1 for x in lazy)
    t["three residual result words"] = plan.n_residual == c.rs.N_RES > 64
    rule, lane, grp = c.want["rule_idx"], np.concatenate([np.arange(g.lanes) for g in c.groups]), np.concatenate([np.full(g.lanes, k) for k, g in enumerate(c.groups)])
    by_lazy = rule < n_cmp
    t["a lazy rule decides lane 0 of group 0"] = bool((by_lazy & (lane == 0) & (grp == 0)).any())
    t["a lazy length rule decides lane 0 of a later group"] = bool((np.isin(rule, (0, 1, 4)) & (lane == 0) & (grp > 0)).any())
    t["a lazy rule decides lane 63"] = bool((by_lazy & (lane == 63)).any())
    t["a lazy rule decides the last lane of the partial last group"] = bool(by_lazy[-1]) and c.groups[-1].lanes < 64
    for k in range(n_cmp):
        t[f"rule z{k} decides a request and misses its near neighbour"] = bool((rule == k).any()) and bool((c.M[k] != c.T[k]).any())
    t["residual rules of all three result words decide"] = all(bool(((rule >= n_cmp + 32 * w) & (rule < min(n_cmp + 32 * w + 32, n_cmp + c.rs.N_RES))).any()) for w in range(3))
    ms = c.models(flags)
    t["the residual entries carry the batch registers through 64"] = any("residual" in m.bn_through_64_by for m in ms)
    t["groups with scan entries and residual entries, with residual entries alone, with neither"] = (
        any(m.passes and m.n_residual for m in ms) and any(not m.passes and m.n_residual for m in ms) and any(m.n_entries == 1 for m in ms))
    t["a group of 64 residual entries"] = any(m.n_residual == 64 for m in ms)
    if flags & TINY:
        t["the residual entry that spills"] = any(m.spilled and m.n_residual and len(m.columns) - m.n_residual < m.e_cap <= len(m.columns) for m in ms)
    return t


def plan_dev(plan, public):
    return np.nonzero(plan.rules["public_idx"] == public)[0][0]


def deciding_positions(c, flags):
    """-> (the positions in their group's candidate list of the rules that decide a request, how many requests the list's last rule decides)"""
    plan, _ = c.rs.tables(flags)
    dev = {int(p): d for d, p in enumerate(plan.rules["public_idx"])}
    pos, last, at = set(), 0, 0
    for g, m in zip(c.groups, c.models(flags)):
        for r in c.want["rule_idx"][at:at + g.lanes].tolist():
            if r < 0xFFFFFFF0:
                p = m.cand.index(dev[r])
                pos.add(p)
                last += p == m.n_cand - 1
        at += g.lanes
    return pos, last


def assert_targets(c, flags):
    missing = [k for k, ok in targets(c, flags).items() if not ok]
    assert not missing, f"set {c.name}, flags {flags}: targets not reached: {missing}"


# ---------------------------------------------------------------------------------------------------------
# turns: the base batch tiled past the persistent grid's stride
# ---------------------------------------------------------------------------------------------------------
STATES = ("clean", "full", "spilled")


def pair_ok(a, b, ca, cb):
    """what a wave's consecutive groups must share: spilled -> clean reads a column the spilled group appended (which entries of a spilled
    group lie beyond the capacity is the kernel's order: any common column), spilled -> spilled over different column sets, clean -> clean
    over column sets that are not empty and have nothing in common"""
    if a == "spilled" and b == "clean":
        return bool(ca & cb)
    if a == "spilled" and b == "spilled":
        return ca != cb
    if a == "clean" and b == "clean":
        return bool(ca) and bool(cb) and not (ca & cb)
    return True


def turn_sequence(states, columns):
    """the base groups in the order a wave meets them: group g of the tiled batch is seq[(g % stride + g // stride) % len(seq)], so the
    wave that starts at group w takes seq[w], seq[w + 1], seq[w + 2], ... whatever the stride. Every ordered pair of states stands
    somewhere in the sequence as neighbours; every base group is in it."""
    seq = []
    for a in STATES:
        for b in STATES:
            found = [(i, j) for i in range(len(states)) for j in range(len(states)) if i != j and states[i] == a and states[j] == b and pair_ok(a, b, columns[i], columns[j])]
            assert found, f"no two base groups make the turn pair {a} -> {b}"
            seq += list(found[0])
    return seq + [i for i in range(len(states)) if i not in seq]


def turn_groups(seq, stride, turns=2, extra=96):
    """-> base group of every group of the tiled batch: `turns` whole turns of the persistent grid and a remainder (some waves take one
    more group). The stride must let every neighbour pair of the sequence fall on some wave."""
    assert stride > len(seq), (stride, len(seq))
    g = np.arange(turns * stride + min(extra, stride))
    return np.asarray(seq)[(g % stride + g // stride) % len(seq)]


def turn_pairs(kinds, stride):
    """the (earlier, later) base groups of every wave's consecutive turns"""
    return set(zip(kinds[:-stride].tolist(), kinds[stride:].tolist()))


def turn_indices(kinds):
    return (np.asarray(kinds)[:, None] * 64 + np.arange(64)[None, :]).reshape(-1)
