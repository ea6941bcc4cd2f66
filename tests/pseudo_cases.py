"""Cases for the two pseudo passes behind the scan passes (docs/pseudo_edges.md): field against field (fcmp_kernel) and the residual rules
(residual_kernel, interpreted, hit records; rvm_jit_kernel, specialized, one result word per request and 32 rules).

Every atom stands alone in a rule, so the hit matrix of a PWAF_OPT_RULE_HITS engine is one bit per (atom, request). The expected matrix is
the MODEL: plain Python on the requests' own strings for the field predicates (an absent header is the empty string, length() counts the
encoded bytes), numpy shifts and masks on the requests' integers for the residual bit rules, `word in url` for the scan rules of set M. The
model never reads a program dump; tests/test_pseudo_edges_cpu.py pins it to the oracle on every bit of every base batch and asserts every
target below, tests/test_gpu_pseudo_edges.py imports the same cases.

A base batch is a list of named groups of 64 requests (the last one partial), so that a target can name a group."""
import functools
import random

import numpy as np

import helpers as H
from pingoo_amd import Request, RequestBatch, _abi

B, CAP = H.B, H.CAP
HITS = _abi.OPT_RULE_HITS
NO_GATES = _abi.OPT_NO_UA_GATE | _abi.OPT_NO_CAPTCHA_BYPASS
OBSERVE = HITS | NO_GATES
TINY, GLOBAL, SPARSE, DENSE, NO_JIT = (_abi.OPT_TINY_VERDICT_SLOTS, _abi.OPT_GLOBAL_VERDICT_TABLES, _abi.OPT_SPARSE_VERDICT, _abi.OPT_DENSE_VERDICT,
                                       _abi.OPT_NO_RESIDUAL_JIT)
COLUMN_FILE_LEGS = {"sparse": SPARSE, "dense": DENSE, "sparse, tiny slots": SPARSE | TINY, "dense, tiny slots": DENSE | TINY}
ACTIONS = ([B], [CAP], [CAP, B])
SIZES = (1, 63, 64, 65, 129, 255, 256, 257)
ERR_SIZES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)
ERR_ONLY_LAST = (1, 65, 127, 256)  # one size of each residue class modulo 64 (and the batch of one)
ROUND = 1 << 20  # the lanes of launch_fcmp's (4096 x 256) and launch_residual's (8192 x 128) capped grids
POOL_MIN = 1 << 20  # the overflow pool holds max(2^20, 8 n) entries (pipeline.cpp)

# ---------------------------------------------------------------------------------------------------------
# field against field
# ---------------------------------------------------------------------------------------------------------
EXPR = {"host": "http_request.host", "url": "http_request.url", "path": "http_request.path", "method": "http_request.method", "ua": "http_request.user_agent",
        "h0": 'http_request.headers["x-a"]', "h1": 'http_request.headers["x-b"]', "h2": 'http_request.headers["x-c"]', "h3": 'http_request.headers["x-d"]'}
HEADER = {"h0": "x-a", "h1": "x-b", "h2": "x-c", "h3": "x-d"}
PAIRS = [("url", "path"), ("url", "host"), ("ua", "method"), ("h0", "h1"), ("h2", "host")]
OPS = ("eq", "co", "st", "en", "llt", "lle")


def expr(op, a, b):
    a, b = EXPR[a], EXPR[b]
    return {"eq": f"{a} == {b}", "co": f"{a}.contains({b})", "st": f"{a}.starts_with({b})", "en": f"{a}.ends_with({b})",
            "leq": f"{a}.length() == {b}.length()", "llt": f"{a}.length() < {b}.length()", "lle": f"{a}.length() <= {b}.length()"}[op]


def f32_atoms():
    """the 32 field atoms over 8 fields. `user_agent.length() < method.length()` stands first and `... <=` last: a request with a shorter
    user agent and nothing else satisfies exactly atoms 0 and 31, the two 15-bit fields of an inline record"""
    atoms = [(op, a, b) for a, b in PAIRS for op in OPS] + [("leq", "url", "path"), ("co", "path", "url")]
    first, last = ("llt", "ua", "method"), ("lle", "ua", "method")
    return [first] + [t for t in atoms if t not in (first, last)] + [last]


F32 = f32_atoms()
F33 = F32 + [("en", "path", "url")]  # the 33rd predicate: a residual rule
F9 = F32[:31] + [("eq", "h3", "h0")]  # the 9th field: a residual rule
assert len(F32) == 32 and len({x for _, a, b in F32 for x in (a, b)}) == 8 and (F32[0], F32[31]) == (("llt", "ua", "method"), ("lle", "ua", "method"))


def fget(f, key):
    v = f.get(key)
    return "" if v is None else v


def holds(op, x, y):
    """the model of one field predicate, on the request's own strings; length() is the number of encoded bytes"""
    if op == "eq":
        return x == y
    if op == "co":
        return y in x
    if op == "st":
        return x.startswith(y)
    if op == "en":
        return x.endswith(y)
    lx, ly = len(x.encode()), len(y.encode())
    return {"leq": lx == ly, "llt": lx < ly, "lle": lx <= ly}[op]


def field_matrix(atoms, fields):
    return np.array([[holds(op, fget(f, a), fget(f, b)) for f in fields] for op, a, b in atoms], dtype=bool)


def field_request(f, **kw):
    hdrs = {HEADER[k]: f[k] for k in HEADER if f.get(k) is not None}
    return Request(host=f["host"], url=f["url"], path=f["path"], method=f["method"], user_agent=f["ua"], headers=hdrs or None, **kw)


# no atom of F32, F33 or F9 holds: every haystack is longer than its needle and does not contain it
ZERO = dict(host="h0", url="/zzzzzz", path="/qq", method="GET", ua="Mozilla", h0="vvv", h1="w", h2="kkk", h3=None)
ALL = dict(host="ab", url="ab", path="ab", method="ab", ua="ab", h0="ab", h1="ab", h2="ab", h3="ab")  # every satisfiable atom holds
ONE = dict(ZERO, ua="PUT")  # atom 31 alone (lengths equal, nothing else)
TWO = dict(ZERO, ua="GE")  # atoms 0 and 31
THREE = dict(TWO, h0="vvv", h1="www")
FOUR = dict(THREE, h2="kk")
SHORT = ["", "a", "ab", "b", "/a", "/ab", "/a/ab", "ab/a", "xyz", "qqqq", "/q", "GET", "curl GET"]
LONG = {n: "q" * (n - 2) + "ab" for n in (255, 256, 4097)}
# (label, haystack, needle)
EDGES = [("both empty", "", ""), ("needle empty", "abc", ""), ("haystack empty", "", "abc"), ("equal", "abc", "abc"), ("needle one byte longer", "abc", "abcd"),
         ("only at offset 0", "abxcd", "ab"), ("only at the last offset", "cdxab", "ab"), ("only in the middle", "cabd", "ab"),
         ("last byte mismatches at the last offset", "xxxabd", "abc"), ("lengths equal", "abc", "xyz"), ("one byte longer", "abcd", "xyz"),
         ("one byte shorter", "ab", "xyz"), ("haystack of 1", "b", "b"), ("haystack of 2", "ab", "b"), ("haystack of 255", LONG[255], "ab"),
         ("haystack of 256", LONG[256], "ab"), ("haystack of 4097", LONG[4097], "ab"), ("haystack of 256, one byte short", "q" * 254 + "aa", "ab"),
         ("equal haystacks of 4097", LONG[4097], LONG[4097]), ("more bytes, as many characters", "aé", "ab"), ("fewer bytes, as many characters", "ab", "aé"),
         ("two bytes against one character", "é", "a"), ("multi-byte needle at the end", "ab€", "€")]


def edge_targets(fields, a, b):
    """what the requests hold for the pair (haystack a, needle b), from their bytes"""
    t = dict.fromkeys(["both empty", "needle empty", "haystack empty", "equal", "needle one byte longer", "only at offset 0", "only at the last offset",
                       "only in the middle", "last byte mismatches at the last offset", "lengths equal", "one byte longer", "one byte shorter",
                       "as many characters, other byte counts"] + [f"haystack of {n}" for n in (1, 2, 255, 256, 4097)], False)
    if a in HEADER or b in HEADER:
        t.update({"header absent": False, "header present and empty": False, "header present and equal": False})
    for f in fields:
        xs, ys = fget(f, a), fget(f, b)
        x, y = xs.encode(), ys.encode()
        t["both empty"] |= not x and not y
        t["needle empty"] |= bool(x) and not y
        t["haystack empty"] |= not x and bool(y)
        t["equal"] |= bool(x) and x == y
        t["needle one byte longer"] |= len(y) == len(x) + 1 and y.startswith(x) and bool(x)
        at, last = x.find(y), len(x) - len(y)
        once = bool(y) and last > 0 and at >= 0 and at == x.rfind(y)
        t["only at offset 0"] |= once and at == 0
        t["only at the last offset"] |= once and at == last
        t["only in the middle"] |= once and 0 < at < last
        t["last byte mismatches at the last offset"] |= len(y) >= 2 and last > 0 and y not in x and x[last:-1] == y[:-1] and x[-1] != y[-1]
        t["lengths equal"] |= len(x) == len(y) and x != y
        t["one byte longer"] |= len(x) == len(y) + 1
        t["one byte shorter"] |= len(x) + 1 == len(y)
        t["as many characters, other byte counts"] |= len(xs) == len(ys) and len(x) != len(y)
        if len(x) in (1, 2, 255, 256, 4097) and y and x.endswith(y):
            t[f"haystack of {len(x)}"] = True
        for k in (a, b):
            if k in HEADER:
                t["header absent"] |= f.get(k) is None
                t["header present and empty"] |= f.get(k) == ""
                t["header present and equal"] |= bool(x) and x == y
    return t


def isolate(a, b, x, y):
    """a request that holds (x, y) for the pair and, as far as the shared fields allow, nothing for the other pairs"""
    f = dict(ZERO)
    f[a], f[b] = x, y
    x, y = x or "", y or ""
    if (a, b) == ("h2", "host") or (a, b) == ("url", "host"):
        # host is the needle of two pairs: keep the other pair's haystack longer than it and free of it
        other = "h2" if a == "url" else "url"
        f[other] = ("/" if other == "url" else "") + "z" * (len(y.encode()) + 3)
    if (a, b) == ("url", "host") and len(x.encode()) <= len(f["path"]):
        f["path"] = "Q" * (len(x.encode()) - 1)  # (shorter than the url and not in it; for a url of at most one byte the empty path cannot be avoided)
    return f


def chained(count):
    return count >= 3


def field_groups():
    """-> [(kind, [field dict, ...])]: whole groups of 64, the last one partial"""
    rng = random.Random(0xFC)
    draw = lambda: {k: rng.choice(SHORT) for k in ("host", "url", "path", "method", "ua", "h0", "h1", "h2")} | {"h3": rng.choice([None, "", "ab", "a"])}  # noqa: E731
    sparse = lambda: rng.choice([ZERO, ZERO, ONE, TWO])  # noqa: E731
    groups = []
    # the edges of every pair, each request twice (of two neighbours at most one is captcha-verified)
    edge = [dict(ALL)]  # request 0: every comparison runs against offset 0 of its arena
    for a, b in PAIRS:
        for _, x, y in EDGES:
            edge += [isolate(a, b, x, y)] * 2
        # an empty haystack between a request that ends in the needle and one that begins with it; the same for an empty needle
        edge += [isolate(a, b, "zzab", "q"), isolate(a, b, "", "ab"), isolate(a, b, "abzz", "q")]
        edge += [isolate(a, b, "q", "zzab"), isolate(a, b, "ab", ""), isolate(a, b, "q", "abzz")]
        if a in HEADER:
            for ha, hb in ((None, None), ("", None), (None, ""), ("", ""), ("v", None), (None, "v"), ("v", "v"), ("v", "")):
                edge += [isolate(a, b, ha, hb if b in HEADER else hb or "")] * 2
    edge += [dict(ZERO, h3="vvv"), dict(ZERO, h3="vvv"), dict(ZERO, h3=""), dict(ZERO, path="/zzzzzz", url="zz"), dict(ZERO, path="/zzzzzz", url="zz")]
    while len(edge) % 64:
        edge.append(draw())
    groups += [(f"edges {k // 64}", edge[k:k + 64]) for k in range(0, len(edge), 64)]
    groups.append(("counts", [ZERO, ONE, TWO, THREE, FOUR, ALL] * 2 + [sparse() for _ in range(52)]))
    groups.append(("none chained", [sparse() for _ in range(64)]))
    groups.append(("lane 0 chained", [FOUR] + [sparse() for _ in range(63)]))
    groups.append(("lane 63 chained", [sparse() for _ in range(63)] + [THREE]))
    groups.append(("every lane chained", [rng.choice([THREE, FOUR, ALL]) for _ in range(64)]))
    groups.append(("chain and inline name the same atoms", [rng.choice([TWO, THREE, FOUR, ONE]) for _ in range(60)] + [TWO, FOUR, TWO, THREE]))
    for k in range(6):
        groups.append((f"random {k}", [draw() for _ in range(64)]))
    # the partial last group: its last request's haystacks end in their needles, at the last byte of every arena
    groups.append(("partial", [draw() for _ in range(35)] + [dict(ZERO), dict(host="ab", url="cd/ab", path="ab", method="ab", ua="xab", h0="yab", h1="ab", h2="zab", h3="yab")]))
    return groups


# ---------------------------------------------------------------------------------------------------------
# residual rules
# ---------------------------------------------------------------------------------------------------------
SOURCES = [("client.remote_port", "port", 16), ("client.asn", "asn", 31), ("http_request.path.length()", "plen", 10), ("http_request.url.length()", "ulen", 10),
           ("http_request.host.length()", "hlen", 6)]
BITS = [(e, key, j) for e, key, nb in SOURCES for j in range(nb)]
assert len(BITS) == 73


def bit_rule(e, j):
    return f"{e} / {1 << j} % 2 == 1"


def err_rule(k, modulus):
    """errs (a division by zero) for exactly the requests with asn % 3 == 1, whatever the port"""
    return f"{k} / (client.asn % 3 - 1) >= 0 && client.remote_port % {modulus} == 1"


# (kind, ...) per rule: ("bit", key, j) or ("err", constant, modulus)
R74 = [("bit", key, j) for _, key, j in BITS] + [("err", 7, 2)]
R8 = R74[:8]
RE_AT = (31, 32, 63, 64, 77)
RE_ERR = [("err", 7, 2), ("err", 8, 3), ("err", 9, 5), ("err", 10, 7), ("err", 11, 11)]


def re_rules():
    rules, bits, errs = [], list(R74[:73]), list(RE_ERR)
    for k in range(78):
        rules.append(errs.pop(0) if k in RE_AT else bits.pop(0))
    return rules


RE = re_rules()
assert [k for k, r in enumerate(RE) if r[0] == "err"] == list(RE_AT)
KEY_EXPR = {key: e for e, key, _ in SOURCES}


def residual_expr(r):
    return bit_rule(KEY_EXPR[r[1]], r[2]) if r[0] == "bit" else err_rule(r[1], r[2])


def residual_model(rules, v):
    """v: dict of int64 arrays port, asn, plen, ulen, hlen -> (M bool[n_rules, n], errors per rule)"""
    n = len(v["port"])
    m, errs = np.zeros((len(rules), n), dtype=bool), []
    for k, r in enumerate(rules):
        if r[0] == "bit":
            m[k] = (v[r[1]] >> r[2]) & 1 == 1
            errs.append(0)
        else:
            m[k] = (v["asn"] % 3 == 2) & (v["port"] % r[2] == 1)
            errs.append(int((v["asn"] % 3 == 1).sum()))
    return m, errs


def ints(port=0, asn=0, plen=0, ulen=0, hlen=0):
    return dict(port=port, asn=asn, plen=plen, ulen=ulen, hlen=hlen)


def int_request(d, **kw):
    return Request(host="h" * d["hlen"], url=("/" + "u" * (d["ulen"] - 1))[:d["ulen"]], path=("/" + "p" * (d["plen"] - 1))[:d["plen"]], method="GET", user_agent="ua",
                   remote_port=d["port"], asn=d["asn"], country="FR", **kw)


def int_columns(rows):
    return {k: np.array([d[k] for d in rows], dtype=np.int64) for k in ("port", "asn", "plen", "ulen", "hlen")}


ALL_BITS = ints(65535, (1 << 31) - 1, 1023, 1023, 63)  # all 73 bit rules (asn % 3 == 1: the erring rules err)
WORD2_FULL = ints(1, 2, 0, 896, 63)  # rules 64 ... 73 of R74: every bit of the last result word


def single(rules, k):
    """a request for which rule k of `rules` holds and as little else as the rule allows"""
    r = rules[k]
    if r[0] == "bit":
        return ints(**{r[1]: 1 << r[2]})
    others = [q[2] for q in rules if q[0] == "err" and q is not r]
    port = next(p for p in range(1, 65536) if p % r[2] == 1 and all(p % o != 1 for o in others))
    return ints(port=port, asn=2)


def residual_groups(rules):
    rng = random.Random(0x2E5 + len(rules))
    r16, r31, r10, r6 = (lambda: rng.choice([0, 65535, rng.randrange(65536)])), (lambda: rng.choice([0, (1 << 31) - 1, rng.randrange(1 << 31)])), \
        (lambda: rng.randrange(1024)), (lambda: rng.randrange(64))
    draw = lambda: ints(r16(), r31(), r10(), r10(), r6())  # noqa: E731
    zero, one, two, three, four = ints(), ints(port=1, asn=0), ints(port=3), ints(port=7), ints(port=15)
    sparse = lambda: rng.choice([zero, zero, one, two, ints(port=2), ints(asn=3 << 20)])  # noqa: E731
    groups = []
    edge = []
    for k in range(len(rules)):
        edge += [single(rules, k)] * 2
    while len(edge) % 64:
        edge.append(draw())
    groups += [(f"single rules {k // 64}", edge[k:k + 64]) for k in range(0, len(edge), 64)]
    groups.append(("counts", [zero, one, two, three, four, ALL_BITS, WORD2_FULL] * 2 + [sparse() for _ in range(50)]))
    groups.append(("none chained", [sparse() for _ in range(64)]))
    groups.append(("lane 0 chained", [four] + [sparse() for _ in range(63)]))
    groups.append(("lane 63 chained", [sparse() for _ in range(63)] + [three]))
    groups.append(("every lane chained", [rng.choice([three, four, ALL_BITS, ints(port=7, asn=7, ulen=7)]) for _ in range(64)]))
    groups.append(("chain and inline name the same atoms", [rng.choice([one, two, three, four]) for _ in range(60)] + [two, four, two, three]))
    # word 0 (the ports and asn bits 0 ... 15, prefetched a group ahead) zero for every lane and the last word not, and the reverse
    groups.append(("word 0 zero, last word not", [ints(asn=rng.choice([0, 3, 6]) << 16, plen=rng.randrange(1024), ulen=128 * rng.randrange(1, 8), hlen=rng.randrange(1, 64)) for _ in range(64)]))
    groups.append(("last word zero, word 0 not", [ints(port=2 * rng.randrange(1, 32768), asn=3 * rng.randrange(1, 21845), plen=rng.randrange(512), ulen=rng.randrange(8)) for _ in range(64)]))
    for k in range(4):
        groups.append((f"random {k}", [draw() for _ in range(64)]))
    groups.append(("partial", [draw() for _ in range(36)] + [single(rules, len(rules) - 1)]))
    return groups


# ---------------------------------------------------------------------------------------------------------
# set M: scan passes and both pseudo passes in one program
# ---------------------------------------------------------------------------------------------------------
M_RES = R74[:16] + R74[16:19] + [("err", 7, 2)]  # the port's bits, asn bits 0 ... 2, the erring rule: nothing that reads a length
M_WORDS = H.pass_words(0xED6E, 12)


def m_rules():
    """-> [(kind, payload)] in rule order: 8 x (4 field atoms, a word, 2 residual rules, ...)"""
    f, r, w, out = list(F32), list(M_RES), list(M_WORDS), []
    while f or r or w:
        for src, kind, take in ((f, "field", 3), (w, "word", 1), (r, "res", 2), (f, "field", 1), (w, "word", 1), (r, "res", 1)):
            for _ in range(take):
                if src:
                    out.append((kind, src.pop(0)))
    return out


M_RULES = m_rules()
assert len(M_RULES) == 64 and [k for k, _ in M_RULES].count("field") == 32


def m_request(f, d, **kw):
    hdrs = {HEADER[k]: f[k] for k in HEADER if f.get(k) is not None}
    return Request(host=f["host"], url=f["url"], path=f["path"], method=f["method"], user_agent=f["ua"], headers=hdrs or None, remote_port=d["port"], asn=d["asn"], country="FR", **kw)


def m_groups():
    rng = random.Random(0x3E)
    rows = []

    def one(scan, fch, rch):
        f = dict(FOUR if fch else rng.choice([ZERO, ONE, TWO]))
        if scan:
            f["url"] = f["url"] + "-".join(rng.sample(M_WORDS, rng.randint(1, 4)))
        return f, ints(port=rng.choice([7, 15, 65535]) if rch else rng.choice([0, 1, 2]), asn=rng.choice([2, 5]) if rch else 0)

    groups = []
    for scan in (0, 1):
        for fch in (0, 1):
            for rch in (0, 1):
                rows = [one(0, 0, 0) for _ in range(64)]
                for lane in rng.sample(range(64), 9):
                    rows[lane] = one(scan, fch, rch)
                groups.append((f"scan {scan}, field chain {fch}, residual chain {rch}", rows))
    groups.append(("all three in every lane", [one(1, 1, 1) for _ in range(64)]))
    for k in range(4):
        rows = []
        for _ in range(64):
            f = {k2: rng.choice(SHORT) for k2 in ("host", "url", "path", "method", "ua", "h0", "h1", "h2")} | {"h3": None}
            if rng.random() < 0.5:
                f["url"] += rng.choice(M_WORDS) + rng.choice(["", M_WORDS[0][:5], rng.choice(M_WORDS)])
            rows.append((f, ints(port=rng.randrange(65536), asn=rng.randrange(8))))
        groups.append((f"random {k}", rows))
    # every rule alone, twice (the deciding form: a rule that holds alone decides)
    alone = []
    for kind, p in M_RULES:
        if kind == "word":
            alone += [(dict(ZERO, url=ZERO["url"] + p), ints())] * 2
        elif kind == "res":
            alone += [(dict(ZERO), single(M_RES, M_RES.index(p)))] * 2
    for a, b in PAIRS:
        for _, x, y in EDGES:
            alone += [(isolate(a, b, x, y), ints())] * 2
    alone = alone[:64 * (len(alone) // 64) + 37]
    groups += [(f"alone {k // 64}", alone[k:k + 64]) for k in range(0, len(alone), 64)]
    return groups


def m_model(rows):
    fields, v = [f for f, _ in rows], int_columns([dict(ints(), **d) for _, d in rows])
    fm = field_matrix(F32, fields)
    rm, _ = residual_model(M_RES, v)
    m = np.zeros((len(M_RULES), len(rows)), dtype=bool)
    kinds = np.empty(len(M_RULES), dtype=object)
    for k, (kind, p) in enumerate(M_RULES):
        kinds[k] = kind
        m[k] = fm[F32.index(p)] if kind == "field" else rm[M_RES.index(p)] if kind == "res" else [p in f["url"] for f in fields]
    return m, kinds, int((v["asn"] % 3 == 1).sum())


# ---------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------
class Case:
    """name, exprs (one per rule), groups [(kind, rows)], batch, M (the model's matrix), errors (per rule, the base batch), verified"""

    def __init__(self, name, exprs, groups, requests, m, errors):
        self.name, self.exprs, self.groups, self.M, self.errors = name, exprs, groups, m, errors
        self.batch = RequestBatch.from_requests(requests)
        self.n = self.batch.n
        self.verified = (self.batch.flags & _abi.FLAG_CAPTCHA_VERIFIED) != 0
        assert self.n < 2000 and m.shape == (len(exprs), self.n)
        assert len(groups[-1][1]) < 64 and all(len(rows) == 64 for _, rows in groups[:-1])
        assert m.any(axis=1).all() and not m.all(axis=1).any(), ("an atom holds for nobody or for everybody", np.nonzero(~m.any(axis=1))[0], np.nonzero(m.all(axis=1))[0])

    def group_of(self, kind):
        k = [g for g, _ in self.groups].index(kind)
        return slice(64 * k, min(64 * k + 64, self.n))

    def observe(self):
        return [(f"r{k}", e, []) for k, e in enumerate(self.exprs)]

    def deciding(self, reverse=False):
        rules = [(f"r{k}", e, ACTIONS[k % 3]) for k, e in enumerate(self.exprs)]
        return rules[::-1] if reverse else rules

    def expect(self, reverse=False, cols=slice(None)):
        """the deciding form's verdicts and counters, from the model's matrix"""
        from test_gpu_rule_hits import deciding_rule

        rules, m = self.deciding(reverse), (self.M[::-1] if reverse else self.M)[:, cols]
        first, action = deciding_rule(m, rules, self.verified[cols])
        want = np.zeros(m.shape[1], dtype=np.dtype([("action", np.uint8), ("rule_idx", np.uint32)]))
        want["action"], want["rule_idx"] = action, np.where(first < len(rules), first, _abi.RULE_NONE)
        return want

    def assert_every_rule_decides(self):
        n_rules = len(self.exprs)
        fwd, rev = self.expect(False)["rule_idx"], self.expect(True)["rule_idx"]
        decided = set(fwd[fwd < n_rules].tolist()) | {n_rules - 1 - int(k) for k in rev[rev < n_rules]}
        assert decided == set(range(n_rules)), (self.name, "rules that decide nobody in either order", sorted(set(range(n_rules)) - decided))
        assert 0.25 < self.verified.mean() < 0.4 and not self.verified[-1]


def _requests(groups, make):
    rows = [r for _, g in groups for r in g]
    return rows, [make(r, captcha_verified=(i % 3 == 1 and i != len(rows) - 1)) for i, r in enumerate(rows)]


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("F32", "F33", "F9"):
        atoms, groups = {"F32": F32, "F33": F33, "F9": F9}[name], field_groups()
        rows, reqs = _requests(groups, field_request)
        c = Case(name, [expr(*t) for t in atoms], groups, reqs, field_matrix(atoms, rows), [0] * len(atoms))
        c.atoms, c.fields = atoms, rows
    elif name in ("R74", "RE"):
        rules = R74 if name == "R74" else RE
        groups = residual_groups(rules)
        rows, reqs = _requests(groups, int_request)
        m, errors = residual_model(rules, int_columns(rows))
        c = Case(name, [residual_expr(r) for r in rules], groups, reqs, m, errors)
        c.res_rules, c.ints = rules, rows
    elif name == "M":
        groups = m_groups()
        rows, reqs = _requests(groups, lambda r, **kw: m_request(r[0], r[1], **kw))
        m, kinds, n_err = m_model(rows)
        exprs = [expr(*p) if kind == "field" else residual_expr(p) if kind == "res" else f'http_request.url.contains("{p}")' for kind, p in M_RULES]
        c = Case(name, exprs, groups, reqs, m, [n_err if (kind, p) == ("res", ("err", 7, 2)) else 0 for kind, p in M_RULES])
        c.kinds = kinds
    else:
        raise KeyError(name)
    return c


# ---------------------------------------------------------------------------------------------------------
# targets (asserted on the model by the CPU suite, and again by the device suite before anything is sent)
# ---------------------------------------------------------------------------------------------------------
def record_targets(c, m, what):
    """the hit records of a dense pass over the rows `m` of the matrix (one pass's atoms)"""
    cnt = m.sum(axis=0)
    for k in (0, 1, 2, 3, 4):
        assert (cnt == k).any(), f"{c.name}: no request with exactly {k} {what}"
    assert (cnt == cnt.max()).any() and cnt.max() >= 20
    lanes = {kind: chained(cnt[c.group_of(kind)]) for kind in ("none chained", "lane 0 chained", "lane 63 chained", "every lane chained", "chain and inline name the same atoms")}
    assert not lanes["none chained"].any() and lanes["every lane chained"].all()
    assert np.nonzero(lanes["lane 0 chained"])[0].tolist() == [0] and np.nonzero(lanes["lane 63 chained"])[0].tolist() == [63]
    g = c.group_of("chain and inline name the same atoms")
    mg, ch = m[:, g], lanes["chain and inline name the same atoms"]
    two = cnt[g] == 2
    assert ch.any() and two.any() and (mg[:, ch].any(axis=1) & mg[:, two].any(axis=1)).any(), "no atom named by a chain and by an inline record"
    return cnt


def assert_field_targets(c):
    assert c.atoms[:31] == F32[:31]
    for a, b in PAIRS:
        t = edge_targets(c.fields, a, b)
        assert all(t.values()), (c.name, a, b, [k for k, v in t.items() if not v])
    if c.name != "F9":  # (F9's pass holds 31 atoms: the record targets are F32's and F33's)
        m32 = c.M[:32]
        cnt = record_targets(c, m32, "field atoms")
        assert cnt.max() == 27 and (cnt[[0]] == 27).all()  # eq, contains, starts, ends and <= of every pair, == of the lengths, path.contains(url)
        inline = (cnt == 2) & m32[0] & m32[31]
        assert inline.any(), "no inline record of atoms 0 and 31"
        assert ((cnt == 1) & m32[31]).any()
    # arena position: the first request's comparisons start at offset 0 of every arena, the last one's end at the arena's last byte
    first, last = c.fields[0], c.fields[-1]
    for a, b in PAIRS:
        assert fget(first, a) and fget(first, a) == fget(first, b)
        assert fget(last, a).endswith(fget(last, b)) and fget(last, b)
    # an empty field between a neighbour that ends in the other field's bytes and one that begins with them
    for a, b in PAIRS:
        for hay, needle in ((a, b), (b, a)):
            assert any(fget(f, hay) == "" and fget(f, needle) and fget(p, hay).endswith(fget(f, needle)) and fget(q, hay).startswith(fget(f, needle))
                       for p, f, q in zip(c.fields, c.fields[1:], c.fields[2:])), (a, b, hay)
    c.assert_every_rule_decides()


def assert_residual_targets(c):
    rules, n_rules = c.res_rules, len(c.res_rules)
    words = (n_rules + 31) // 32
    bit_rows = np.array([r[0] == "bit" for r in rules])
    cnt = record_targets(c, c.M, "residual rules")
    assert (c.M[bit_rows].sum(axis=0) == 73).any(), "no request with all 73 bit rules"
    w = np.zeros((words, c.n), dtype=np.uint64)
    for k in range(n_rules):
        w[k // 32] |= c.M[k].astype(np.uint64) << np.uint64(k % 32)
    last_bits = n_rules - 32 * (words - 1)
    for k in (0, 31, 32, 63, 64):
        if rules[k][0] == "bit":
            assert ((cnt == 1) & c.M[k]).any(), f"rule {k} holds alone for nobody"
    # (the last rule needs an odd port and a nonzero asn: alone in its WORD is what can be built)
    assert (w[words - 1] == np.uint64(1 << (last_bits - 1))).any(), "the last rule is alone in the last word for nobody"
    assert (w[words - 1] == np.uint64((1 << last_bits) - 1)).any() or c.name == "RE", "no request with every bit of the last word"
    full = np.uint64(0xFFFFFFFF)
    err_bits = [sum(1 << (k % 32) for k in range(32 * j, min(32 * j + 32, n_rules)) if rules[k][0] == "err") for j in range(words)]
    assert ((w[0] == full ^ np.uint64(err_bits[0])) & (w[1] == full ^ np.uint64(err_bits[1]))).any(), "no request with every bit of words 0 and 1"
    g = c.group_of("word 0 zero, last word not")
    assert (w[0, g] == 0).all() and (w[words - 1, g] != 0).all()
    g = c.group_of("last word zero, word 0 not")
    assert (w[words - 1, g] == 0).all() and (w[0, g] != 0).all()
    g = c.group_of("partial")
    assert c.M[n_rules - 1, c.n - 1] and not c.verified[-1] and g.stop - g.start < 64
    assert all(e == c.errors[RE_AT[0] if c.name == "RE" else 73] and e > 100 for e, r in zip(c.errors, rules) if r[0] == "err")
    c.assert_every_rule_decides()


def assert_m_targets(c):
    field, res, word = (c.kinds == k for k in ("field", "res", "word"))
    fc, rc, wc = c.M[field].sum(axis=0), c.M[res].sum(axis=0), c.M[word].sum(axis=0)
    assert ((fc > 0) & (rc > 0) & (wc > 0)).any()
    seen = set()
    for k, (kind, _) in enumerate(c.groups):
        g = slice(64 * k, min(64 * k + 64, c.n))
        seen.add((bool((wc[g] > 0).any()), bool((fc[g] >= 3).any()), bool((rc[g] >= 3).any())))
    assert len(seen) == 8, seen
    c.assert_every_rule_decides()


def assert_targets(c):
    {"F32": assert_field_targets, "F33": assert_field_targets, "F9": assert_field_targets, "R74": assert_residual_targets, "RE": assert_residual_targets,
     "M": assert_m_targets}[c.name](c)


# ---------------------------------------------------------------------------------------------------------
# error counts: batches of the sizes at which the last wave is partial, whole, or one lane
# ---------------------------------------------------------------------------------------------------------
def error_batch(n):
    """-> (batch of n requests, the model's matrix, errors per rule of RE). For the sizes of ERR_ONLY_LAST the only request that errs is the
    last one of the batch."""
    rows = [dict(d) for d in case("RE").ints[:n]]
    if n in ERR_ONLY_LAST:
        for d in rows[:-1]:
            if d["asn"] % 3 == 1:
                d["asn"] -= 1
        rows[-1]["asn"] = 4
    m, errors = residual_model(RE, int_columns(rows))
    assert (n not in ERR_ONLY_LAST or all(e == 1 for e, r in zip(errors, RE) if r[0] == "err")) and [k for k, e in enumerate(errors) if e] in ([], list(RE_AT))
    return RequestBatch.from_requests([int_request(d) for d in rows]), m, errors


# ---------------------------------------------------------------------------------------------------------
# the second round of the grid-stride loops, and the pool exhausted by a pseudo pass
# ---------------------------------------------------------------------------------------------------------
BIG_BASE, BIG_N = 4099, ROUND + 257


@functools.lru_cache(maxsize=None)
def second_round(name):
    """-> (exprs, base batch of 4 099 requests with fields of at most 8 bytes, its matrix, the indices of the gathered batch). The
    requests from 1 048 576 on are base requests 3 331 ... 3 587; the ones 1 048 576 places before them are base requests 0 ... 256."""
    rng = random.Random(0xB16)
    idx = np.arange(BIG_N, dtype=np.int64) % BIG_BASE
    shift = ROUND % BIG_BASE
    if name == "F32":
        rows = [{k: rng.choice(SHORT) for k in ("host", "url", "path", "method", "ua", "h0", "h1", "h2")} | {"h3": None} for _ in range(BIG_BASE)]
        states = [ZERO, ONE, TWO, THREE, FOUR, ALL]
        for t, f in enumerate(states):  # the second round's requests hold every record state; the same lanes of the first round another one
            rows[shift + t], rows[t] = dict(f), dict(states[(t + 3) % 6])
        assert all(len(fget(f, k).encode()) <= 8 for f in rows for k in EXPR)
        m = field_matrix(F32, rows)
        batch = RequestBatch.from_requests([field_request(f) for f in rows])
        exprs = [expr(*t) for t in F32]
        # (no two requests differ in EVERY field atom: `<` implies `<=`, `==` implies `contains`; the records differ in every state instead)
        differs = [(m[:, t] != m[:, shift + t]).sum() for t in range(257)]
        assert max(differs) >= 27
    else:
        rows = [ints(port=rng.randrange(65536), asn=rng.randrange(1 << 20)) for _ in range(BIG_BASE)]
        states = [ints(port=p) for p in (0, 1, 3, 7, 15, 255)]
        for t, d in enumerate(states):
            rows[shift + t], rows[t] = dict(d), dict(states[(t + 3) % 6])
        rows[shift + 8], rows[8] = ints(port=0xFF00 | 0xA5), ints(port=0x5A)
        m, _ = residual_model(R8, int_columns(rows))
        assert (m[:, 8] != m[:, shift + 8]).all(), "no request that differs in every rule from the one 1 048 576 places before it"
        batch = RequestBatch.from_requests([int_request(d) for d in rows])
        exprs = [residual_expr(r) for r in R8]
    cnt = m.sum(axis=0)
    late = cnt[idx[ROUND:]]
    assert idx[ROUND] == shift and {0, 1, 2, 3}.issubset(set(np.minimum(late, 3).tolist())) and (late >= 4).any() and BIG_BASE % 64 != 0
    assert (chained(cnt[idx[ROUND:ROUND + 6]]) != chained(cnt[idx[:6]])).any()
    assert m.any(axis=1).all() and not m.all(axis=1).any()
    return exprs, batch, m, idx


def pool_case(name):
    """-> (exprs, the one request, its column of the matrix, n, errors per rule): n copies whose chains need more entries than the pool holds"""
    if name == "F32":
        exprs, req, col, n, errors = [expr(*t) for t in F32], field_request(ALL), field_matrix(F32, [ALL])[:, 0], 60_000, [0] * 32
    else:
        m, errors = residual_model(RE, int_columns([ALL_BITS]))
        exprs, req, col, n = [residual_expr(r) for r in RE], int_request(ALL_BITS), m[:, 0], 16_000
        errors = [e * n for e in errors]
    t = int(col.sum())
    assert t >= 20 and n * t > max(POOL_MIN, 8 * n), (n, t)
    return exprs, req, col, n, errors


def packed(m):
    """bool[n_rules, n] -> uint64[n_rules, groups]: the masks a hit list must hold"""
    n_rules, n = m.shape
    pad = np.zeros((n_rules, (n + 63) // 64 * 64), dtype=bool)
    pad[:, :n] = m
    return np.packbits(pad, axis=1, bitorder="little").view("<u8")


def assert_hits_packed(label, hits, rule_hits, want_masks, want_counts):
    """helpers.assert_hits for a batch too large for a bool matrix per hit entry: the same statements on 64-bit masks"""
    assert (hits["mask"] != 0).all(), f"{label}: an entry with an empty mask"
    assert (hits["rule_idx"] < want_masks.shape[0]).all() and (hits["group"] < want_masks.shape[1]).all(), f"{label}: a hit names a rule or a group beyond the batch"
    got = np.zeros_like(want_masks)
    seen = np.zeros(want_masks.shape, dtype=np.uint32)
    np.add.at(seen, (hits["rule_idx"].astype(np.int64), hits["group"].astype(np.int64)), 1)
    assert seen.max(initial=0) <= 1, f"{label}: a (rule, group) pair appears twice"
    got[hits["rule_idx"].astype(np.int64), hits["group"].astype(np.int64)] = hits["mask"]
    diff = got ^ want_masks
    bad = np.argwhere(diff != 0)
    n_bits = int(np.unpackbits(diff.view(np.uint8)).sum())
    assert n_bits == 0, f"{label}: {n_bits} (rule, request) bits differ; first: rule {bad[0][0]}, group {bad[0][1]}: got {int(got[tuple(bad[0])]):#x} want {int(want_masks[tuple(bad[0])]):#x}"
    assert rule_hits.tolist() == list(want_counts), f"{label}: rule_hits"
