"""The oracle of pwaf_parse_pow_bodies / pwaf_parse_pow_body_one: decisions D-B1 to D-B10 of DESIGN.md §5.1.8 restated byte by byte with
bytes methods and one regular expression. A helper, not a test file; written from the decisions, not from csrc/powbody.h: it cuts the
body from the left with lstrip / find / slicing instead of walking a position, and decodes the hash with bytes.fromhex. It also builds
the corpora the tests share: genuine bodies (both member orders, whitespace variants, mixed-case hex), per decision the bodies that make
its MALFORMED and its UNDECIDED event at the first, a middle and the last possible position, and a seeded mutator."""
import functools
import hashlib
import random
import re

NONE, OK, MALFORMED, UNDECIDED = 0, 1, 2, 3
MAX_BYTES = 4096  # PWAF_POW_BODY_MAX_BYTES
WS = b" \t\n\r"
ZERO = bytes(32)
HEX64 = re.compile(rb"[0-9a-fA-F]{64}")


class _Decided(Exception):
    def __init__(self, status):
        self.status = status


def _string(rest):
    """D-B4: `rest` begins behind an opening '"' -> (the text, what follows the closing '"')"""
    q = rest.find(b'"')
    if q < 0:
        raise _Decided(MALFORMED)
    text = rest[:q]
    if any(b < 0x20 for b in text):
        raise _Decided(MALFORMED)
    if b"\\" in text:
        raise _Decided(UNDECIDED)
    return text, rest[q + 1:]


def _after_ws(rest):
    """ws*, and the body must go on (D-B2, D-B3: its end anywhere up to the closing brace is MALFORMED)"""
    rest = rest.lstrip(WS)
    if not rest:
        raise _Decided(MALFORMED)
    return rest


def _members(body):
    if len(body) > MAX_BYTES:  # D-B1
        raise _Decided(UNDECIDED)
    rest = _after_ws(body)  # D-B2
    if rest[:1] == b"[":
        raise _Decided(UNDECIDED)
    if rest[:1] != b"{":
        raise _Decided(MALFORMED)
    rest = rest[1:]
    found = {}
    while True:
        rest = _after_ws(rest)  # D-B3
        if rest[:1] != b'"':
            raise _Decided(MALFORMED)
        key, rest = _string(rest[1:])
        if any(b >= 0x80 for b in key) or key not in (b"hash", b"nonce"):  # D-B5
            raise _Decided(UNDECIDED)
        if key in found:
            raise _Decided(MALFORMED)
        rest = _after_ws(rest)
        if rest[:1] != b":":
            raise _Decided(MALFORMED)
        rest = _after_ws(rest[1:])
        if rest[:1] != b'"':  # D-B6
            raise _Decided(MALFORMED)
        text, rest = _string(rest[1:])
        if key == b"hash":  # D-B7
            if not HEX64.fullmatch(text):
                raise _Decided(MALFORMED)
            found[key] = bytes.fromhex(text.decode("ascii"))
        else:  # D-B8
            if any(b >= 0x80 for b in text):
                raise _Decided(UNDECIDED)
            found[key] = text
        rest = _after_ws(rest)
        if rest[:1] == b"}":
            break
        if rest[:1] != b",":
            raise _Decided(MALFORMED)
        rest = rest[1:]
    if len(found) != 2 or rest[1:].strip(WS):  # D-B9
        raise _Decided(MALFORMED)
    return found


@functools.lru_cache(maxsize=None)
def decide(body):
    """body: bytes -> (status, the hash's 32 bytes, the nonce's bytes); 32 zero bytes and b"" unless the status is OK"""
    try:
        found = _members(body)
    except _Decided as d:
        return d.status, ZERO, b""
    return OK, found[b"hash"], found[b"nonce"]  # D-B10


# ---- genuine bodies ------------------------------------------------------------------------------------------------------------------------
def digest_of(k):
    return hashlib.sha256(b"powbody %d" % k).digest()


def genuine(nonce=b"4711", digest=None, order="nh", ws=None, case="lower"):
    """JSON.stringify({nonce, hash}) as captcha/src/index.tsx sends it; order "hn": the members swapped; ws: 9 byte strings placed in
    front of '{', the first key, ':', the first value, ',', the second key, ':', the second value and '}', plus (a tenth) behind '}';
    case: "lower" | "upper" | "mixed" hex"""
    digest = digest_of(len(nonce)) if digest is None else digest
    text = digest.hex()
    if case == "upper":
        text = text.upper()
    elif case == "mixed":
        text = "".join(c.upper() if k % 3 == 0 else c for k, c in enumerate(text))
    members = {"n": (b'"nonce"', b'"' + nonce + b'"'), "h": (b'"hash"', b'"' + text.encode() + b'"')}
    (k1, v1), (k2, v2) = members[order[0]], members[order[1]]
    w = list(ws or [b""] * 10)
    w += [b""] * (10 - len(w))
    return w[0] + b"{" + w[1] + k1 + w[2] + b":" + w[3] + v1 + w[4] + b"," + w[5] + k2 + w[6] + b":" + w[7] + v2 + w[8] + b"}" + w[9]


def genuine_cases():
    """[(label, body)] that are all OK: both orders, every whitespace byte at every place, mixed-case hex, nonces of many lengths"""
    out = []
    for order in ("nh", "hn"):
        for case in ("lower", "upper", "mixed"):
            out.append((f"genuine {order} {case}", genuine(order=order, case=case)))
        for place in range(10):
            for fill in (b" ", b"\t", b"\n", b"\r", b" \t\r\n "):
                ws = [b""] * 10
                ws[place] = fill
                out.append((f"genuine {order} ws {fill!r} at {place}", genuine(order=order, ws=ws)))
        out.append((f"genuine {order} ws everywhere", genuine(order=order, ws=[b" \n"] * 10)))
        for length in (0, 1, 2, 15, 16, 17, 20, 300):
            out.append((f"genuine {order} nonce of {length}", genuine(nonce=b"9" * length, order=order)))
    out.append(("genuine nonce of every printable byte", genuine(nonce=bytes(b for b in range(0x20, 0x7F) if b not in b'"\\'))))
    out.append(("genuine nonce 0x7F", genuine(nonce=b"\x7f")))
    return out


def _places(lo, hi):
    """the first, a middle and the last position of [lo, hi)"""
    return sorted({lo, (lo + hi - 1) // 2, hi - 1})


def _put(body, at, byte):
    return body[:at] + byte + body[at + 1:]


def decision_cases():
    """[(label beginning with its decision, body, the status the decision gives)], written out by hand from D-B1 to D-B10"""
    g = genuine()
    n_key, n_val, h_key, h_val = g.index(b'nonce'), g.index(b'4711'), g.index(b'hash'), g.index(b'"', g.index(b'hash') + 6) + 1
    out = []
    add = lambda label, body, status: out.append((label, body, status))  # noqa: E731
    # D-B1
    add("D-B1 a body of exactly the limit", g + b" " * (MAX_BYTES - len(g)), OK)
    add("D-B1 a body one byte above the limit", g + b" " * (MAX_BYTES + 1 - len(g)), UNDECIDED)
    add("D-B1 a long body that would be MALFORMED", b"x" * (MAX_BYTES + 1), UNDECIDED)
    add("D-B1 a nonce that fills the limit", genuine(nonce=b"7" * (MAX_BYTES - len(g) + 4)), OK)
    # D-B2
    add("D-B2 the empty body", b"", MALFORMED)
    for fill in (b" ", b"\t\n\r ", b" " * 33):
        add(f"D-B2 only ws {fill[:4]!r} x {len(fill)}", fill, MALFORMED)
    add("D-B2 an array", b"[]", UNDECIDED)
    add("D-B2 an array behind ws", b" \n[" + g, UNDECIDED)
    add("D-B2 an unclosed array", b"[", UNDECIDED)
    for first in (b"x", b'"', b"}", b"n", b"1", b"\x00", b"\x0b", b"\x0c", b"\xc3", b"\\", b","):
        add(f"D-B2 first byte {first!r}", first + g, MALFORMED)
        add(f"D-B2 first byte {first!r} behind ws", b"\r\n" + first + g[1:], MALFORMED)
    # D-B3
    for k in range(1, len(g)):
        add(f"D-B3 the body ends behind {k} bytes", g[:k], MALFORMED)
    add("D-B3 the body ends in ws inside the object", g[:-1] + b"  ", MALFORMED)
    for label, body in (("a bare key", b'{nonce:"1"}'), ("a key in single quotes", b"{'nonce':\"1\"}"), ("a number as the key", b'{1:"1"}'),
                        ("a closing brace right behind a comma", g[:-1] + b",}"), ("two commas", g.replace(b",", b",,")),
                        ("a comma first", b"{," + g[1:]), ("an unknown bare key behind a known member", g[:-1] + b",x:1}")):
        add(f"D-B3 {label}", body, MALFORMED)
    for label, body in (("'=' for ':'", g.replace(b":", b"=", 1)), ("no ':' at all", g.replace(b'":"', b'""', 1)), ("the second ':' missing", g[::-1].replace(b":", b" ", 1)[::-1]),
                        ("a closing brace for ':'", b'{"nonce"}')):
        add(f"D-B3 {label}", body, MALFORMED)
    for label, body in (("';' between the members", g.replace(b",", b";")), ("nothing between the members", g.replace(b",", b" ")), ("']' for the closing brace", g[:-1] + b"]"),
                        ("a second value", g[:-1] + b'"x"}'), ("a 0x0B behind a value", g[:-1] + b"\x0b}"), ("a colon behind a value", g[:-1] + b":}")):
        add(f"D-B3 {label}", body, MALFORMED)
    # D-B4
    for name, lo, hi in (("the first key", n_key, n_key + 5), ("the nonce", n_val, n_val + 4), ("the second key", h_key, h_key + 4), ("the hash", h_val, h_val + 64)):
        for at in _places(lo, hi):
            for ctl in (b"\x00", b"\x01", b"\x1f", b"\n"):
                add(f"D-B4 {ctl!r} in {name} at {at - lo}", _put(g, at, ctl), MALFORMED)
            add(f"D-B4 an escape in {name} at {at - lo}", _put(g, at, b"\\"), UNDECIDED)
            add(f"D-B4 an escape inserted in {name} at {at - lo}", g[:at] + b"\\u0031" + g[at:], UNDECIDED)
        add(f"D-B4 an escape then a control byte in {name}", _put(_put(g, lo, b"\\"), hi - 1, b"\x01"), MALFORMED)
        add(f"D-B4 a control byte then an escape in {name}", _put(_put(g, lo, b"\x01"), hi - 1, b"\\"), MALFORMED)
    add("D-B4 an escaped quote ends the string where it stands", b'{"nonce":"a\\"b","hash":"' + b"0" * 64 + b'"}', UNDECIDED)
    add("D-B4 an escape in a string that never closes", b'{"nonce":"a\\', MALFORMED)
    add("D-B4 an escape in the last string, which never closes", g[:h_val] + b"\\" + g[h_val:-2], MALFORMED)
    add("D-B4 a control byte behind the closing quote's place", b'{"nonce":"1"\x01,"hash":"' + b"0" * 64 + b'"}', MALFORMED)
    # D-B5
    for at in _places(n_key, n_key + 5):
        add(f"D-B5 0xC3 in the first key at {at - n_key}", _put(g, at, b"\xc3"), UNDECIDED)
    for at in _places(h_key, h_key + 4):
        add(f"D-B5 0xC3 in the second key at {at - h_key}", _put(g, at, b"\xc3"), UNDECIDED)
    for key in (b"", b"h", b"has", b"hashh", b"Hash", b"HASH", b"nonc", b"nonce ", b" nonce", b"nonces", b"hash\x7f", b"noncehash", b"x" * 40, b"nonce\xc3\xa9"):
        add(f"D-B5 the key {key!r} first", b'{"' + key + b'":"1",' + g[1:], UNDECIDED)
        add(f"D-B5 the key {key!r} last", g[:-1] + b',"' + key + b'":[{"a":"}"}]}', UNDECIDED)
    add("D-B5 an unknown key in front of a body that ends early", b'{"x":', UNDECIDED)
    add("D-B5 an unknown key in front of a missing colon", b'{"x"}', UNDECIDED)
    add("D-B5 nonce twice", b'{"nonce":"1","nonce":"1","hash":"' + b"0" * 64 + b'"}', MALFORMED)
    add("D-B5 hash twice", g[:-1] + b',"hash":"' + b"0" * 64 + b'"}', MALFORMED)
    add("D-B5 nonce twice, the second value a number", b'{"nonce":"1","nonce":5}', MALFORMED)
    add("D-B5 nonce twice, the second value with an escape", b'{"nonce":"1","nonce":"\\n"}', MALFORMED)
    add("D-B5 nonce twice, nothing behind the second key", b'{"nonce":"1","nonce"', MALFORMED)
    add("D-B5 hash twice in front of an unknown key", b'{"hash":"' + b"0" * 64 + b'","hash":"' + b"0" * 64 + b'","x":1}', MALFORMED)
    # D-B6
    for value in (b"1", b"4711", b"null", b"true", b"[]", b"{}", b"-", b"x", b"'1'", b"\x01", b"\xc3", b"\\"):
        add(f"D-B6 the nonce is {value!r}", b'{"nonce":' + value + b',"hash":"' + b"0" * 64 + b'"}', MALFORMED)
        add(f"D-B6 the hash is {value!r}", b'{"nonce":"1","hash":' + value + b"}", MALFORMED)
    add("D-B6 a number in front of an unknown key", b'{"nonce":5,"x":1}', MALFORMED)
    # D-B7
    for length in (0, 1, 2, 32, 62, 63, 65, 66, 128):
        add(f"D-B7 a hash text of {length}", b'{"nonce":"1","hash":"' + b"a" * length + b'"}', MALFORMED)
    for at in _places(h_val, h_val + 64):
        for byte in (b"g", b"G", b"/", b":", b"@", b"`", b" ", b"x", b"\x7f", b"\x80", b"\xc3", b"\xff"):
            add(f"D-B7 {byte!r} in the hash at {at - h_val}", _put(g, at, byte), MALFORMED)
    add("D-B7 0x prefix", b'{"nonce":"1","hash":"0x' + b"a" * 62 + b'"}', MALFORMED)
    add("D-B7 every hexadecimal digit of both cases", b'{"nonce":"1","hash":"0123456789abcdefABCDEF' + b"5" * 42 + b'"}', OK)
    add("D-B7 an escape in a hash text of the wrong length", b'{"nonce":"1","hash":"\\u0061"}', UNDECIDED)
    add("D-B7 a wrong hash in front of an unknown key", b'{"hash":"zz","x":1}', MALFORMED)
    # D-B8
    for at in _places(n_val, n_val + 4):
        for byte in (b"\x80", b"\xc3", b"\xff"):
            add(f"D-B8 {byte!r} in the nonce at {at - n_val}", _put(g, at, byte), UNDECIDED)
    add("D-B8 a well-formed two-byte character in the nonce", genuine(nonce=b"caf\xc3\xa9"), UNDECIDED)
    add("D-B8 a high byte in the nonce in front of a wrong hash", b'{"nonce":"\xc3","hash":"zz"}', UNDECIDED)
    add("D-B8 a high byte in the nonce behind a wrong hash", b'{"hash":"zz","nonce":"\xc3"}', MALFORMED)
    add("D-B8 the empty nonce", genuine(nonce=b""), OK)
    add("D-B8 a nonce that is no number", genuine(nonce=b"{not: a [number]} 'at' all,:"), OK)
    # D-B9
    add("D-B9 the empty object", b"{}", MALFORMED)
    add("D-B9 the empty object with ws", b" { } ", MALFORMED)
    add("D-B9 the nonce alone", b'{"nonce":"1"}', MALFORMED)
    add("D-B9 the hash alone", b'{"hash":"' + b"0" * 64 + b'"}', MALFORMED)
    for tail in (b"x", b"}", b"{}", b",", b"\x00", b"\x0b", b"\xc3", b" x", b"\n\n\\", b"[", b" " * 40 + b"0"):
        add(f"D-B9 {tail[-4:]!r} behind the object", g + tail, MALFORMED)
    add("D-B9 ws of every kind behind the object", g + b" \t\n\r" * 9, OK)
    # D-B10
    add("D-B10 the genuine body", g, OK)
    add("D-B10 the members swapped", genuine(order="hn"), OK)
    return out


@functools.lru_cache(maxsize=None)
def fixed_corpus():
    """[(label, body, the status written by hand or None)]: the genuine cases and every decision's"""
    return tuple([(label, body, OK) for label, body in genuine_cases()] + decision_cases())


# ---- the mutator ---------------------------------------------------------------------------------------------------------------------------
SPLICES = (b"\\", b'"', b",", b"}", b"\x01", b"\xc3")


def mutate(rng, body):
    """one mutation: a byte flip, an insertion, a deletion, a truncation, or a splice of one of SPLICES"""
    kind = rng.randrange(6)
    at = rng.randrange(len(body) + 1) if body else 0
    if kind == 0 and body:
        at = min(at, len(body) - 1)
        return _put(body, at, bytes([body[at] ^ (1 << rng.randrange(8))]))
    if kind == 1:
        return body[:at] + bytes([rng.randrange(256)]) + body[at:]
    if kind == 2 and body:
        at = min(at, len(body) - 1)
        return body[:at] + body[at + 1:]
    if kind == 3:
        return body[:at]
    if kind == 4 and body:
        at = min(at, len(body) - 1)
        return _put(body, at, bytes([rng.choice(b"0123456789abcdefABCDEF \t")]))
    return body[:at] + rng.choice(SPLICES) + body[at:]


@functools.lru_cache(maxsize=None)
def mutated_corpus(count=20000, seed=20260):
    """`count` bodies: a genuine body (random nonce length, order, whitespace, hex case) behind 0, 1, 2 or 3 mutations. One body in four is
    left as it is and most mutations are decided, so that well over half of the corpus is decided and a tenth is OK (the tests assert it)."""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        nonce = bytes(rng.choice(b"0123456789") for _ in range(rng.choice((0, 1, 3, 5, 8, 12, 16, 19, 40))))
        ws = [rng.choice((b"", b"", b"", b" ", b"\n", b"\t ")) for _ in range(10)] if rng.randrange(4) == 0 else None
        body = genuine(nonce, digest_of(k), order=rng.choice(("nh", "nh", "hn")), ws=ws, case=rng.choice(("lower", "lower", "upper", "mixed")))
        for _ in range(rng.choice((0, 1, 1, 2))):
            body = mutate(rng, body)
        out.append(body)
    return tuple(out)


def column(bodies, lead=0):
    """a string column: bodies back to back behind `lead` bytes of 0xAA, PWAF_ARENA_PAD zero bytes behind -> (data bytes, [offsets])"""
    off, at = [lead], lead
    for b in bodies:
        at += len(b)
        off.append(at)
    return b"\xaa" * lead + b"".join(bodies) + bytes(16), off


def expect_batch(bodies, idx=None, m=None):
    """what a call over `bodies` answers -> (status list per entry, hash rows per request or None where unwritten, nonce per request, stats)"""
    n = len(bodies)
    entries = list(range(n)) if idx is None else list(idx)[:len(idx) if m is None else min(m, len(idx))]
    status, rows, nonces = [], [None] * n, [b""] * n
    for i in entries:
        if not 0 <= i < n:
            status.append(NONE)
            continue
        st, h, nonce = decide(bodies[i])
        status.append(st)
        rows[i], nonces[i] = h, nonce
    stats = {"nonce_bytes": sum(len(x) for x in nonces), "n": len(entries), "n_ok": status.count(OK), "n_malformed": status.count(MALFORMED),
             "n_undecided": status.count(UNDECIDED)}
    return status, rows, nonces, stats
