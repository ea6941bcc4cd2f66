"""Cases for attr_kernel's comparison and short-literal atoms (docs/attr_edges.md): the two atom loops behind the membership rows of
csrc/attr.hip, and the host code that feeds them (csrc/tableplan.cpp: canonical_comparisons, choose_polarity, encode_comparisons,
record_row; csrc/scanplan.cpp: the short-literal pass).

Every atom stands alone in a rule, so the hit matrix of a PWAF_OPT_RULE_HITS engine is one bit per (atom, request). The expected matrix
is the MODEL: plain Python on the requests' own integers and encoded bytes — `len(value) <op> c` on Python integers (no width, no sign),
`value == literal`, `value.startswith(literal)`, `port in set`, and for the engine-resolved asn a longest-prefix lookup written here. The
model never reads a dump; tests/test_attr_edges_cpu.py pins it to the oracle on every bit of every base batch and asserts from the two
plan dumps that every set lands where it is aimed, tests/test_gpu_attr_edges.py imports the same cases.

A base batch is a list of named groups of 64 requests (the last one partial, 37 requests), so that a target can name a group."""
import functools
import ipaddress
import random

import numpy as np

import pseudo_cases as PC
from pingoo_amd import Request, RequestBatch, _abi, geoip_entries

FIELDS = _abi.FIELD_NAMES
OPS = ("==", "!=", "<", "<=", ">", ">=")
U32 = (1 << 32) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
CONSTS = (0, 1, 255, 256, 65535, 65536, (1 << 31) - 1, 1 << 31, U32, U32 + 1, -1, I64_MIN, I64_MAX)
LEN_CONSTS = CONSTS + (2, 3, 4096, 4097)  # (2 and 3: the multi-byte values; 4097: the longest value of the other suites)
OBSERVE, NO_GATES, ACTIONS = PC.OBSERVE, PC.NO_GATES, PC.ACTIONS
EAGER, NO_PREFILTER = _abi.OPT_EAGER_CMP, _abi.OPT_NO_PREFILTER
SIZES = (1, 63, 64, 65, 129, 257)
V_PORT, V_ASN = 5, 6  # (the plan's variable indices: 0 ... 4 the field lengths, then these, then 7 + k the k-th header length)
PORT_MAX = 65535
LEN_REACH, URL_REACH = 4098, 65537  # the longest value a set builds for a length (url.length() alone goes to both sides of 65536)
PARTIAL = 37
# kernels.h / attr.hip: what the kernel keeps where
CMP_REGS, CMP_STAGED, SHORT_REGS, SHORT_STAGED = 64, 192, 64, 64


# ---------------------------------------------------------------------------------------------------------
# atoms: ("cmp", var, op, c) | ("lit", field, form, bytes) | ("pset", (ports)) | ("and", token, atom)
# ---------------------------------------------------------------------------------------------------------
def var_expr(var):
    if isinstance(var, str):
        return f'http_request.headers["{var}"].length()'
    return f"http_request.{FIELDS[var]}.length()" if var < 5 else ("client.remote_port", "client.asn")[var - 5]


def expr(atom):
    kind = atom[0]
    if kind == "cmp":
        return f"{var_expr(atom[1])} {atom[2]} {atom[3]}"
    if kind == "lit":
        e, t = f"http_request.{FIELDS[atom[1]]}", atom[3].decode()
        return {"eq": f'{e} == "{t}"', "sw": f'{e}.starts_with("{t}")', "re_eq": f'{e}.matches("^{t}$")', "re_sw": f'{e}.matches("^{t}")'}[atom[2]]
    if kind == "pset":
        return "[" + ", ".join(str(p) for p in atom[1]) + "].contains(client.remote_port)"
    return f'http_request.host.contains("{atom[1]}") && {expr(atom[2])}'


NEUTRAL = dict(f=(b"h.example", b"/index.html", b"/index", b"GET", b"agent/1.0"), port=30000, asn=64500, ip="10.9.0.1", hdr={})
NEUTRAL_COVER = ("10.9.0.0/16", 64500, "FR")  # the record the neutral address reads when the engine resolves the asn


def bytes_of_len(n):
    """a value of n BYTES; an even n of two or more is n / 2 two-byte characters, so that a count of characters is another number"""
    return "é".encode() * (n // 2) if n >= 2 and n % 2 == 0 else b"x" * n


def put(row, var, v):
    """a copy of the row with the variable's value set to v"""
    r = dict(row, f=tuple(row["f"]), hdr=dict(row["hdr"]))
    if isinstance(var, str):
        r["hdr"].pop(var, None)
        if v:
            r["hdr"][var] = bytes_of_len(v)  # (length 0: the header is absent)
    elif var < 5:
        r["f"] = tuple(bytes_of_len(v) if k == var else x for k, x in enumerate(row["f"]))
    elif var == V_PORT:
        r["port"] = v
    else:
        r["asn"], r["ip"] = v, None  # (an engine-resolved case gives every asn an address and a record of its own: Case.resolve)
    return r


def value(r, var):
    if isinstance(var, str):
        return len(r["hdr"].get(var, b""))
    return len(r["f"][var]) if var < 5 else r["port"] if var == V_PORT else r["asn"]


def holds(atom, r):
    """the model of one atom: Python integers and bytes"""
    kind = atom[0]
    if kind == "cmp":
        v, c = value(r, atom[1]), atom[3]
        return {"==": v == c, "!=": v != c, "<": v < c, "<=": v <= c, ">": v > c, ">=": v >= c}[atom[2]]
    if kind == "lit":
        v = r["f"][atom[1]]
        return v == atom[3] if atom[2] in ("eq", "re_eq") else v.startswith(atom[3])
    if kind == "pset":
        return r["port"] in atom[1]
    return atom[1].encode() in r["f"][0] and holds(atom[2], r)


def constant_over(atom, hi):
    """True / False when the comparison has one answer for every value in [0, hi], else None. With hi = the variable's whole range this
    is what the model calls folded: `port <= 65536`, `asn < 2^32`, `length() >= 0` always; `asn == 2^32`, `port > 65535`, anything `< 0` never."""
    _, _, op, c = atom
    at = lambda v: {"==": v == c, "!=": v != c, "<": v < c, "<=": v <= c, ">": v > c, ">=": v >= c}[op]  # noqa: E731
    if op in ("==", "!="):
        return None if 0 <= c <= hi else at(0)
    return at(0) if at(0) == at(hi) else None


def var_range(var):
    return PORT_MAX if var == V_PORT else U32


def canon(op, c):
    """the device form of a source comparison (csrc/tableplan.cpp: canonical_comparisons): (operator 0 `==` / 1 `<=`, 32-bit constant,
    negated), or None when no value of 32 bits satisfies the atom — its column stays zero and a negation of it holds for everybody"""
    neg = op in ("!=", ">", ">=")
    base = {"==": "==", "!=": "==", "<": "<", ">=": "<", "<=": "<=", ">": "<="}[op]
    if base == "==":
        return (0, c, neg) if 0 <= c <= U32 else None
    if base == "<":
        c -= 1
    return (1, min(c, U32), neg) if c >= 0 else None


def geo_lookup(ip, records):
    """the reference's GeoipDB::lookup for the asn: loopback and multicast addresses are not looked up, the longest prefix of the
    address's own family wins, no record is the default record {0, "XX"}"""
    a = ipaddress.ip_address(ip)
    excluded = ("127.0.0.0/8", "224.0.0.0/4") if a.version == 4 else ("::1/128", "ff00::/8")
    if any(a in ipaddress.ip_network(x) for x in excluded):
        return 0
    best = None
    for net, asn in records:
        if net.version == a.version and a in net and (best is None or net.prefixlen > best[0]):
            best = (net.prefixlen, asn)
    return best[1] if best else 0


# ---------------------------------------------------------------------------------------------------------
# a case: atoms, named groups of rows, the model's matrix
# ---------------------------------------------------------------------------------------------------------
class Case:
    """name, atoms, exprs (one per rule), groups [(kind, rows)], rows, batch, M (the model's matrix), verified, geo (GeoIP rows when the
    engine resolves the asn, else None: the batch carries the column), flags (beyond the form's own), reach {variable: largest value}"""

    def __init__(self, name, atoms, groups, geo=False, flags=0, reach=None):
        assert len(groups[-1][1]) == PARTIAL and all(len(rows) == 64 for _, rows in groups[:-1]), [(k, len(r)) for k, r in groups]
        self.name, self.atoms, self.groups, self.flags, self.reach = name, list(atoms), groups, flags, dict(reach or {})
        self.exprs = [expr(a) for a in self.atoms]
        self.rows = [r for _, g in groups for r in g]
        self.geo = self.resolve() if geo else None
        self.n = len(self.rows)
        self.M = np.array([[holds(a, r) for r in self.rows] for a in self.atoms], dtype=bool)
        self.batch = RequestBatch.from_requests(self.request(r, captcha_verified=(i % 3 == 1 and i != self.n - 1)) for i, r in enumerate(self.rows))
        self.verified = (self.batch.flags & _abi.FLAG_CAPTCHA_VERIFIED) != 0
        assert (self.batch.asn is None) == bool(geo) and max(SIZES) < self.n < 2600, self.n
        # every comparison with two answers within the values a request can carry gives both; the others are named by the model
        self.constant = {}
        for k, a in enumerate(self.atoms):
            const = constant_over(a, self.reach.get(a[1], var_range(a[1]))) if a[0] == "cmp" else None
            if const is None:
                assert self.M[k].any() and not self.M[k].all(), (name, "an atom holds for nobody or for everybody", k, self.exprs[k])
            else:
                assert (self.M[k] == const).all(), (name, k, self.exprs[k])
                self.constant[k] = const

    def resolve(self):
        """engine-resolved asn: every asn a row asks for gets an address and a /32 record of its own (boundary asns are records), the
        neutral address reads a /16; the MODEL's asn of a row is then looked up from the address again"""
        want = sorted({r["asn"] for r in self.rows if r["ip"] is None})
        addr = {v: f"10.{1 + (j >> 16)}.{(j >> 8) & 255}.{j & 255}" for j, v in enumerate(want)}
        table = [NEUTRAL_COVER] + [(addr[v] + "/32", v, "FR") for v in want]
        records = [(ipaddress.ip_network(net), asn) for net, asn, _ in table]
        for r in self.rows:
            asked = r["asn"]
            if r["ip"] is None:
                r["ip"] = addr[asked]
            r["asn"] = geo_lookup(r["ip"], records)
            assert r.get("default") or r["asn"] == asked, (r["ip"], asked, r["asn"])
            assert not r.get("default") or r["asn"] == 0
        return table

    def request(self, r, **kw):
        f = r["f"]
        geo = {} if self.geo is not None else dict(asn=r["asn"], country="XX")
        return Request(host=f[0], url=f[1], path=f[2], method=f[3], user_agent=f[4], ip=r["ip"] or NEUTRAL["ip"], remote_port=r["port"], headers=r["hdr"] or None, **geo, **kw)

    def geoip(self):
        return geoip_entries(self.geo) if self.geo is not None else None

    def group_of(self, kind):
        k = [g for g, _ in self.groups].index(kind)
        return slice(64 * k, min(64 * k + 64, self.n))

    def observe(self):
        return [(f"r{k}", e, []) for k, e in enumerate(self.exprs)]

    def deciding(self):
        return [(f"r{k}", e, ACTIONS[k % 3]) for k, e in enumerate(self.exprs)]

    def expect(self, cols=slice(None), m=None, verified=None):
        """the deciding form's verdicts, from the model's matrix (the four counters are the histogram of its actions)"""
        from test_gpu_rule_hits import deciding_rule

        rules, m = self.deciding(), (self.M if m is None else m)[:, cols]
        first, action = deciding_rule(m, rules, (self.verified if verified is None else verified)[cols])
        want = np.zeros(m.shape[1], dtype=np.dtype([("action", np.uint8), ("rule_idx", np.uint32)]))
        want["action"], want["rule_idx"] = action, np.where(first < len(rules), first, _abi.RULE_NONE)
        return want


def whole_groups(tag, rows, pad):
    rows = list(rows)
    while len(rows) % 64:
        rows.append(pad)
    return [(f"{tag} {k // 64}", rows[k:k + 64]) for k in range(0, len(rows), 64)]


def lane_groups(zero, one):
    """no atom holds; exactly one atom holds, in lane 0, 31, 32 or 63 alone (both halves of the parked mask); it holds in all 64 lanes"""
    out = [("none", [zero] * 64)]
    for lane in (0, 31, 32, 63):
        out.append((f"lane {lane}", [one if k == lane else zero for k in range(64)]))
    return out + [("all lanes", [one] * 64)]


def random_groups(rows, seed, count=4):
    """whole groups drawn at random from the set's own rows: the same values in other lanes, beside other neighbours"""
    rng = random.Random(seed)
    rows = list(rows)
    return [(f"random {k}", [rng.choice(rows) for _ in range(64)]) for k in range(count)]


def combined_groups(values, seed, count=4):
    """whole groups of requests that carry an edge value of EVERY variable of the set at once"""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        rows = []
        for _ in range(64):
            r = NEUTRAL
            for var, vs in values.items():
                r = put(r, var, rng.choice(vs))
            rows.append(r)
        out.append((f"combined {k}", rows))
    return out


def partial(rows, last):
    rows = list(rows)
    return ("partial", [rows[k % len(rows)] for k in range(PARTIAL - 1)] + [last])


def neighbours(atoms, reach):
    """per comparison atom the values c - 1, c, c + 1 that a request can carry: all the c - 1 first, then the c, then the c + 1 (so that the
    captcha-verified third of the batch is spread over all three)"""
    out = []
    for d in (-1, 0, 1):
        for a in atoms:
            if a[0] == "cmp" and 0 <= a[3] + d <= reach.get(a[1], var_range(a[1])):
                out.append((a[1], a[3] + d))
    return out


def reach_of(atoms, url_far=False):
    return {a[1]: (PORT_MAX if a[1] == V_PORT else U32 if a[1] == V_ASN else URL_REACH if url_far and a[1] == 1 else LEN_REACH) for a in atoms if a[0] == "cmp"}


# ---------------------------------------------------------------------------------------------------------
# comparison sets: operators, neighbours, variables, constants
# ---------------------------------------------------------------------------------------------------------
DEFAULT_IPS = ("9.9.9.9", "127.0.0.1", "224.0.0.5", "::1", "2001:db8::1", "ff02::1")  # no record; loopback; multicast; an IPv6 client against IPv4 prefixes
DEFAULT_ATOMS = [("cmp", V_ASN, "<", 5), ("cmp", V_ASN, "<=", 0), ("cmp", V_ASN, "==", 0), ("cmp", V_ASN, "!=", 0)]


def default_rows():
    return [dict(NEUTRAL, ip=ip, asn=0, default=True) for ip in DEFAULT_IPS]


def cmp_set(name, variables, consts, geo=False, extra_atoms=(), extra_rows=(), flags=0):
    """all six operators on every variable and constant; every value c - 1, c, c + 1 twice (of two neighbours at most one is
    captcha-verified)"""
    atoms = [("cmp", v, op, c) for v in variables for c in consts for op in OPS] + list(extra_atoms)
    reach = reach_of(atoms, url_far=(list(variables) == [1]))
    seen, rows, values = set(), [], {}
    for var, v in neighbours(atoms, reach):
        if (var, v) not in seen:
            seen.add((var, v))
            rows += [put(NEUTRAL, var, v)] * 2
            if v <= LEN_REACH or var in (V_PORT, V_ASN):
                values.setdefault(var, []).append(v)
    rows = [dict(r) for r in rows + list(extra_rows)]
    groups = whole_groups("edges", rows, dict(NEUTRAL)) + combined_groups(values, len(atoms)) + random_groups(rows, len(atoms), 1)
    groups.append(partial([dict(r) for r in rows], dict(NEUTRAL)))
    return Case(name, atoms, groups, geo=geo, reach=reach, flags=flags)


def header_rows(names):
    """absent, present and empty, one byte, a multi-byte value"""
    out = []
    for h in names:
        out += [dict(NEUTRAL, hdr={}), dict(NEUTRAL, hdr={h: b""}), dict(NEUTRAL, hdr={h: b"v"}), dict(NEUTRAL, hdr={h: "aé".encode()})]
    return out


H8 = [f"x-h{k}" for k in range(9)]  # eight header lengths are variables 7 ... 14; the ninth is lowered to a residual rule


# ---------------------------------------------------------------------------------------------------------
# polarity: `>`, `>=` and `!=` alone in a rule are planned complemented; request 0 satisfies every such atom
# ---------------------------------------------------------------------------------------------------------
def polarity_case():
    atoms = []
    for v in (0, 1, 2, 3, 4, V_PORT):
        c = 300 + 7 * v
        atoms += [("cmp", v, ">", c), ("cmp", v, ">=", c + 3), ("cmp", v, "!=", c + 5), ("cmp", v, "==", c + 9), ("cmp", v, "<", c - 3)]
    reach = reach_of(atoms)
    big = dict(NEUTRAL, f=tuple(b"y" * 1000 for _ in range(5)), port=60000)  # every complemented atom holds, nothing else
    rows = [put(big, var, v) for var, v in neighbours(atoms, reach)]
    groups = [("first", [big] + rows[:63])] + whole_groups("edges", rows[63:], big) + random_groups(rows + [big], 0x901) + [partial(rows, big)]
    c = Case("POL", atoms, groups, reach=reach)
    c.complemented = [k for k, a in enumerate(atoms) if a[2] in (">", ">=", "!=")]
    assert c.M[c.complemented, 0].all() and not c.M[[k for k in range(len(atoms)) if k not in c.complemented], 0].any()
    return c


# ---------------------------------------------------------------------------------------------------------
# chunks: exactly N eager comparison atoms, in the plan's own order (variable, operator, rule), so that rule k is PCMP entry k
# ---------------------------------------------------------------------------------------------------------
CHUNK_SIZES = (1, 64, 65, 256, 257, 300)
ZERO = dict(NEUTRAL, f=(b"h.example", b"/index.html", b"/index123", b"GET", b"agent/1.0"), port=65000, asn=99999)  # no atom of a chunk or short-chunk set holds
FILLER = [("pset", (40000 + k, 50000 + k)) for k in range(33)]  # 33 port sets: a second word of the port-set row, the wide instantiation


def filler_group():
    return ("filler", [dict(ZERO, port=40000 + k) for k in range(33)] + [dict(ZERO)] * 31)


def chunk_atoms(n):
    if n == 1:
        return [("cmp", V_PORT, "==", 1000)]
    n_asn = 6
    n_port = n - 4 - n_asn
    return ([("cmp", 2, "==", 30), ("cmp", 2, "<=", 5)] + [("cmp", V_PORT, "==", 1000 + 3 * k) for k in range(n_port)] + [("cmp", V_PORT, "<=", 100)]
            + [("cmp", V_ASN, "==", v) for v in (0, 7, (1 << 31) - 1, 1 << 31, U32 - 1, U32)] + [("cmp", V_ASN, "<=", 4)])


def chunk_case(n, wide):
    atoms = chunk_atoms(n)
    reach = reach_of(atoms)
    rows = [put(ZERO, var, v) for var, v in neighbours(atoms, reach)]
    probes = sorted({0, 63, 64, 255, 256, n - 1} & set(range(n)))
    one_at = next((k for k in (64, 63, 256, 255) if k < n and atoms[k][2] == "=="), 0)  # (an atom beyond the registers where the set has one)
    one = put(ZERO, atoms[one_at][1], atoms[one_at][3])
    groups = whole_groups("edges", rows, ZERO) + lane_groups(ZERO, one) + random_groups(rows + [ZERO], n, 2) + [filler_group(), partial(rows, one)]
    c = Case(f"C{n}" + ("w" if wide else ""), atoms + (FILLER if wide else []), groups, reach=reach)
    c.n_cmp, c.probes, c.one_at, c.wide = n, probes, one_at, wide
    assert not c.M[:, c.group_of("none")].any() and c.M[:n].sum(axis=0)[c.group_of("all lanes")].tolist() == [1] * 64 and c.M[one_at, c.group_of("all lanes")].all()
    for lane in (0, 31, 32, 63):
        assert np.nonzero(c.M[one_at, c.group_of(f"lane {lane}")])[0].tolist() == [lane]
    return c


# ---------------------------------------------------------------------------------------------------------
# engine-resolved asn: n distinct comparisons are n bits of the class row (one word, a second word, the limit)
# ---------------------------------------------------------------------------------------------------------
GEO_SIZES = (32, 33, 128)


def geo_atoms(n):
    """`==` first, then `<=`: the plan's order, so that rule k is class-row bit k (the rule `!= 0` shares bit 0 and stands last)"""
    le = [("cmp", V_ASN, "<", 5), ("cmp", V_ASN, "<=", 0), ("cmp", V_ASN, "<=", (1 << 31) - 1), ("cmp", V_ASN, "<", (1 << 31) + 1), ("cmp", V_ASN, "<=", U32 - 1)]
    eq = [("cmp", V_ASN, "==", v) for v in (0, 1, (1 << 31) - 1, 1 << 31, U32 - 1, U32)]
    eq += [("cmp", V_ASN, "==", 1000 + 3 * k) for k in range(n - len(eq) - len(le))]
    return eq + le + [("cmp", V_ASN, "!=", 0)]


def geo_case(n):
    atoms = geo_atoms(n)
    reach = reach_of(atoms)
    rows = [put(NEUTRAL, var, v) for var, v in neighbours(atoms, reach)]
    rows = rows[:40] + default_rows() + rows[40:]
    c = Case(f"G{n}", atoms, whole_groups("edges", rows, dict(NEUTRAL)) + random_groups(rows, n) + [partial([dict(r) for r in rows], dict(NEUTRAL))], geo=True, reach=reach)
    c.n_acmp = n
    return c


# ---------------------------------------------------------------------------------------------------------
# lazy atoms: three variables beside a rare token; two become lazy, the third stays eager without being a trigger
# ---------------------------------------------------------------------------------------------------------
LAZY_TOKENS = ("zqxjkv", "wvkqzx", "jxqzvk")


def lazy_case():
    atoms = []
    for tok, v in zip(LAZY_TOKENS, (2, 4, V_PORT)):
        atoms += [("and", tok, ("cmp", v, "<=", 40)), ("and", tok, ("cmp", v, "==", 44)), ("and", tok, ("cmp", v, ">", 50))]
    rows = []
    for tok, v in zip(LAZY_TOKENS, (2, 4, V_PORT)):
        for x in (39, 40, 41, 43, 44, 45, 50, 51):
            for host in (b"a." + tok.encode() + b".example", b"h.example"):
                rows.append(dict(put(NEUTRAL, v, x), f=(host,) + put(NEUTRAL, v, x)["f"][1:]))
    groups = whole_groups("edges", rows, dict(NEUTRAL)) + random_groups(rows, 0x2A) + [partial(rows, dict(NEUTRAL))]
    return Case("Z", atoms, groups)


# ---------------------------------------------------------------------------------------------------------
# short literals
# ---------------------------------------------------------------------------------------------------------
ALPHA = b"ABCDEFGH"
UTF8_LIT = "aé".encode()


def short_atoms(field):
    """lengths 0 ... 8 as `==` and `starts_with` (`starts_with("")` is the constant true to the compiler: no atom), a literal with a two-byte
    character, and the two regex spellings"""
    atoms = [("lit", field, "eq", b"")]
    for k in range(1, 9):
        atoms += [("lit", field, "eq", ALPHA[:k]), ("lit", field, "sw", ALPHA[:k])]
    return atoms + [("lit", field, "eq", UTF8_LIT), ("lit", field, "sw", UTF8_LIT), ("lit", field, "re_eq", b"xy"), ("lit", field, "re_sw", b"xz")]


def literal_values(lit):
    """the values around one literal. Where the value is one byte short, the NEXT value supplies the byte that would complete it."""
    k, out = len(lit), []
    if k:
        out += [lit[:-1], lit[-1:] + b"tail"]  # both forms miss the first; its 8-byte read runs into the second
    out += [lit, lit + b"Z"]
    if k == 8:
        out += [lit + b"I", lit + b"IJKLMNOP", lit + b"\x00"]  # nine and more bytes equal in the first eight; they differ in byte 8 alone
    for at in (0, 3, 4, 7):
        if at < k:
            out.append(lit[:at] + bytes([lit[at] ^ 0x20]) + lit[at + 1:])  # differs in this byte alone
    if k < 8:
        out += [lit + b"\x00", lit + b"\xff", lit + b"\x00" * (8 - k)]  # a NUL and a 0xFF byte where the literal's zero padding lies
    return out


def short_rows(field, atoms):
    vals = []
    for lit in dict.fromkeys(a[3] for a in atoms if a[0] == "lit" and a[1] == field):
        vals += literal_values(lit)
    # an empty value between a neighbour that ends in a literal and one that begins with it
    vals += [b"xx" + ALPHA[:4], b"", ALPHA[:4] + b"xx", b"xx" + ALPHA, b"", ALPHA + b"xx"]
    return [dict(NEUTRAL, f=tuple(v if k == field else x for k, x in enumerate(NEUTRAL["f"]))) for v in vals]


def with_field(row, field, v):
    return dict(row, f=tuple(v if k == field else x for k, x in enumerate(row["f"])))


def short_case(field, flags=0, both=False):
    """the short field is `field`; request 0 is the 8-byte literal at arena offset 0, request 1 is empty (the batch without request 0
    begins with an empty value), the last request is empty (its 8-byte read lies in the arena's pad) and the one before it is the
    8-byte literal (the batch without its last request ends at the arena's last byte)"""
    atoms = short_atoms(field) + (short_atoms(3 if field != 3 else 0) if both else [])
    rows = short_rows(field, atoms)
    if both:
        rows += short_rows(atoms[-1][1], atoms)
    rows = [with_field(NEUTRAL, field, ALPHA), with_field(NEUTRAL, field, b"")] + rows
    tail = [with_field(NEUTRAL, field, ALPHA[:5]), with_field(NEUTRAL, field, ALPHA)]
    groups = whole_groups("edges", rows, dict(NEUTRAL)) + random_groups(rows, 0x50 + field)
    groups.append(("partial", [rows[k % len(rows)] for k in range(PARTIAL - 3)] + tail + [with_field(NEUTRAL, field, b"")]))
    c = Case(f"S{field}" + ("+" if both else "") + ("n" if flags else ""), atoms, groups, flags=flags)
    c.field, c.both = field, both
    f = lambda i: c.rows[i]["f"][field]  # noqa: E731
    assert f(0) == ALPHA and f(1) == b"" and f(c.n - 1) == b"" and f(c.n - 2) == ALPHA
    assert any(f(i - 1).endswith(ALPHA) and f(i) == b"" and f(i + 1).startswith(ALPHA) for i in range(1, c.n - 1))
    return c


SHORT_CHUNKS = (1, 64, 65, 128, 129)


def short_chunk_atoms(n):
    """n literals on the method: 8-byte edge literals (exact at the even places, prefix at the odd ones) at atoms 0, 63, 64, 127, 128 and
    the last, exact literals of 4 to 7 bytes everywhere else"""
    edges = {0, 63, 64, 127, 128, n - 1} & set(range(n))
    return [("lit", 3, "sw" if k % 2 else "eq", b"Q%07d" % k) if k in edges else ("lit", 3, "eq", b"M%03d" % k + b"x" * (k % 4)) for k in range(n)], sorted(edges)


def short_chunk_case(n, wide):
    atoms, edges = short_chunk_atoms(n)
    vals = []
    for k, a in enumerate(atoms):
        vals += literal_values(a[3]) if k in edges else [a[3], a[3] + b"y"]
    rows = [with_field(ZERO, 3, v) for v in vals]
    one = with_field(ZERO, 3, atoms[edges[-1]][3])
    groups = whole_groups("edges", rows, ZERO) + lane_groups(ZERO, one) + random_groups(rows + [ZERO], n, 2) + [filler_group(), partial(rows, one)]
    c = Case(f"SC{n}" + ("w" if wide else ""), atoms + (FILLER if wide else []), groups)
    c.n_short, c.edges, c.wide = n, edges, wide
    assert not c.M[:, c.group_of("none")].any() and c.M[:, c.group_of("all lanes")].sum(axis=0).tolist() == [1] * 64
    return c


# ---------------------------------------------------------------------------------------------------------
# the pair list: memberships, comparisons and short literals together; groups in which every atom holds for somebody
# ---------------------------------------------------------------------------------------------------------
def mixed_case(wide):
    g = 40 if wide else 20  # (40 port sets: a second word of the port-set row)
    atoms = []
    for k in range(g):
        atoms += [("pset", (2000 + k, 9000 + k)), ("cmp", V_PORT, "==", 2000 + k), ("cmp", 2, "==", 10 + k), ("lit", 3, "eq", b"M%03d" % k + b"x" * (k % 4))]
    hit = lambda k: with_field(dict(ZERO, port=2000 + k, f=put(ZERO, 2, 10 + k)["f"]), 3, atoms[4 * k + 3][3])  # noqa: E731
    zero = put(ZERO, 2, 9)
    full_a, full_b = [hit(k % g) for k in range(64)], [hit((63 - k) % g) for k in range(64)]
    some = [hit(k) if k % 3 == 0 else dict(zero, port=9000 + k) if k % 3 == 1 else zero for k in range(g)]
    groups = [("full A", full_a), ("full B", full_b), ("empty", [zero] * 64)] + lane_groups(zero, hit(g - 1)) + whole_groups("some", some, zero) + [("full C", full_b[::-1]), partial(some, hit(0))]
    c = Case("X" + ("w" if wide else ""), atoms, groups)
    c.per_kind, c.wide = g, wide
    for kind in ("full A", "full B", "full C"):
        assert c.M[:, c.group_of(kind)].any(axis=1).all(), "an atom holds for nobody in a full group"
    assert not c.M[:, c.group_of("empty")].any() and not c.M[:, c.group_of("none")].any()
    return c


# ---------------------------------------------------------------------------------------------------------
# turns of the persistent grid: consecutive groups of a wave differ in every input the kernel prefetches
# ---------------------------------------------------------------------------------------------------------
TURN_K = 7
ATTR_GROUPS_PER_CU = 24  # launch_attr: at most 6 workgroups per compute unit, 4 groups per workgroup and turn


def turn_row(j, lane):
    f = tuple(b"v" * (2 + 2 * j + (lane & 1)) if k != 3 else b"T%d" % j + b"x" * j for k in range(5))
    return dict(NEUTRAL, f=f, port=1000 * (j + 1) + lane, asn=100 * (j + 1) + lane)


def turn_inputs(r):
    """what attr_kernel prefetches of a request: the five lengths, the port, the asn, the short value's length and its first 8 bytes"""
    return [len(x) for x in r["f"]] + [r["port"], r["asn"], r["f"][3][:8]]


@functools.lru_cache(maxsize=None)
def turn_base():
    """K whole groups; 48 atoms: per input a threshold between every two neighbouring groups, and the short value of six groups"""
    atoms = []
    for t in range(TURN_K - 1):
        atoms += [("cmp", f, "<=", 3 + 2 * t) for f in (0, 1, 2, 4)] + [("cmp", 3, "<=", 2 + t), ("cmp", V_PORT, "<=", 1000 * (t + 1) + 500), ("cmp", V_ASN, "<=", 100 * (t + 1) + 80),
                                                                         ("lit", 3, "eq", b"T%d" % t + b"x" * t)]
    groups = [(f"turn {j}", [turn_row(j, lane) for lane in range(64)]) for j in range(TURN_K)]
    c = Case("T", atoms, groups + [partial(groups[0][1], turn_row(0, 0))])
    assert len(atoms) == 48
    for j in range(TURN_K):  # any two different groups differ, lane by lane, in every prefetched input
        for i in range(TURN_K):
            if i != j:
                assert all(a != b for lane in range(64) for a, b in zip(turn_inputs(turn_row(i, lane)), turn_inputs(turn_row(j, lane))))
    return c


def turn_kinds(stride):
    """the base group of every group of the turn batch: two strides and 96 groups, group g = base group (g mod stride + g div stride) mod K
    — the wave that starts at group w meets base groups w, w + 1, w + 2 (mod K) in its consecutive turns"""
    g = np.arange(2 * stride + 96)
    return (g % stride + g // stride) % TURN_K


def turn_indices(kinds):
    return (np.asarray(kinds, dtype=np.int64)[:, None] * 64 + np.arange(64)[None, :]).reshape(-1)


# ---------------------------------------------------------------------------------------------------------
# the cases by name
# ---------------------------------------------------------------------------------------------------------
CMP_SETS = [f"LEN{f}" for f in range(5)] + ["LENALL", "PORT", "ASNCOL", "ASNGEO", "H1", "H8"]
CHUNK_SETS = [f"C{n}{w}" for n in CHUNK_SIZES for w in ("", "w")]
GEO_SETS = [f"G{n}" for n in GEO_SIZES]
SHORT_SETS = [f"S{f}" for f in range(5)] + ["S0+", "S0+n"]
SHORT_CHUNK_SETS = [f"SC{n}{w}" for n in SHORT_CHUNKS for w in ("", "w")]
ALL_SETS = CMP_SETS + ["POL"] + CHUNK_SETS + GEO_SETS + ["Z"] + SHORT_SETS + SHORT_CHUNK_SETS + ["X", "Xw", "T"]


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("LEN") and name != "LENALL":
        return cmp_set(name, [int(name[3:])], LEN_CONSTS)
    if name == "LENALL":
        return cmp_set(name, [0, 1, 2, 3, 4], (0, 1, 255, 256))
    if name == "PORT":
        return cmp_set(name, [V_PORT], CONSTS + (65534,))
    if name == "ASNCOL":
        return cmp_set(name, [V_ASN], CONSTS + (U32 - 1,))
    if name == "ASNGEO":
        return cmp_set(name, [V_ASN], CONSTS + (U32 - 1,), geo=True, extra_atoms=[DEFAULT_ATOMS[0]], extra_rows=default_rows())
    if name == "H1":
        return cmp_set(name, [H8[0]], (0, 1, 3, 255, 256, 4097), extra_rows=header_rows(H8[:1]))
    if name == "H8":
        return cmp_set(name, H8[:8], (0, 2), extra_atoms=[("cmp", H8[8], "<=", 2)], extra_rows=header_rows(H8))
    if name == "POL":
        return polarity_case()
    if name == "Z":
        return lazy_case()
    if name == "T":
        return turn_base()
    if name in ("X", "Xw"):
        return mixed_case(name == "Xw")
    wide = name.endswith("w")
    if name.startswith("SC"):
        return short_chunk_case(int(name[2:].rstrip("w")), wide)
    if name.startswith("C"):
        return chunk_case(int(name[1:].rstrip("w")), wide)
    if name.startswith("G"):
        return geo_case(int(name[1:]))
    if name.startswith("S"):
        return short_case(int(name[1]), flags=NO_PREFILTER if name.endswith("n") else 0, both="+" in name)
    raise KeyError(name)
