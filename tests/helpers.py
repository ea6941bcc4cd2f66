"""Shared test helpers: golden-vector loading, a random expression / request fuzzer, verdict comparison."""
from __future__ import annotations

import ctypes as C
import json
import os
import random

import numpy as np

from oracle import pyoracle
from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.batch import hits_to_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA


def load_kat():
    with open(os.path.join(HERE, "golden", "kat.json")) as f:
        return json.load(f)


def kat_case_inputs(c):
    rules = [(r[0], r[1], r[2]) for r in c["rules"]]
    lists = {k: (v[0], v[1]) for k, v in c.get("lists", {}).items()}
    batch = RequestBatch.from_requests([Request(**r) for r in c["requests"]])
    expect = np.array([(a, r) for a, r in c["expect"]], dtype=np.int64)
    return rules, lists, batch, expect


def assert_verdicts_equal(got, want, batch=None, what=""):
    bad = np.nonzero((got["action"] != want["action"]) | (got["rule_idx"] != want["rule_idx"]))[0]
    if len(bad):
        i = int(bad[0])
        ctx = ""
        if batch is not None:
            ctx = " fields=" + repr([batch.field_bytes(f, i) for f in range(5)]) + f" ip={bytes(batch.ip[i]).hex()} v6={batch.ip_is_v6[i]} port={batch.port[i]} flags={batch.flags[i]}"
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} verdicts differ; first at {i}: got ({got[i]['action']}, {got[i]['rule_idx']}) "
                             f"want ({want[i]['action']}, {want[i]['rule_idx']}){ctx}")


# ---------------------------------------------------------------------------------------------------------
# fuzzer: small alphabets so that predicates actually fire
# ---------------------------------------------------------------------------------------------------------
ALPHA = "ab/."
# url / path / host values with UTF-8 in them (http 1.3.1 admits it in path and query, the regex crate matches scalar values): two- and
# three-byte sequences next to the ASCII alphabet, members of \w (e-acute), of \s (U+00A0), of neither (the euro sign), and the two
# code points whose simple case folding reaches ASCII (U+017F ~ s, U+212A ~ k)
UALPHA = "ab/.sk\u00e9\u20ac\u00a0\u017f\u212a"
FIELDS = ["host", "url", "path", "method", "user_agent"]
COUNTRIES = ["XX", "FR", "US", "CN", "DE", "AA", "ZZ"]


def rstr(rng: random.Random, lo=0, hi=6, alpha=ALPHA):
    return "".join(rng.choice(alpha) for _ in range(rng.randint(lo, hi)))


def q(s: str) -> str:
    return '"' + s.replace("\\", "\\\\").replace('"', '\\"') + '"'


def rregex(rng: random.Random, depth=0) -> str:
    """Random pattern over the syntax both the oracle and the device compiler support."""
    k = rng.randint(0, 13 if depth < 3 else 4)
    if k <= 1:
        return rng.choice(["a", "b", "/", "\\.", "ab", "ba", "a/b", ".", "\u00e9", "a\u20ac", "s"])
    if k == 2:
        if rng.random() < 0.2:  # Unicode general categories
            return rng.choice(["\\p{L}", "\\pL", "\\P{L}", "\\p{Lu}", "\\p{Ll}", "\\p{N}", "\\p{Nd}", "\\P{N}", "\\p{P}", "\\p{^P}", "[\\p{L}/]", "[^\\p{N}a]", "\\p{S}", "\\p{Zs}", "[\\P{Lu}b]",
                               "[^\u00e9]", "[\u00e0-\u00ff]", "(?-u:\\w)", "(?-u:\\b)"])
        return rng.choice(["[ab]", "[^a]", "[a-b/]", "\\w", "\\W", "\\d", "\\s", "[[:alpha:]]", "[^/.]", "\\S"])
    if k == 3:
        return rng.choice(["^", "$", "\\b", "\\B", "\\A", "\\z"]) if rng.random() < 0.5 else "a"
    if k == 4:
        return rregex(rng, depth + 1) + rregex(rng, depth + 1)
    if k == 5:
        return "(" + rregex(rng, depth + 1) + "|" + rregex(rng, depth + 1) + ")"
    if k == 6:
        return "(?:" + rregex(rng, depth + 1) + ")" + rng.choice(["*", "+", "?", "{2}", "{1,3}", "{2,}", "*?", "+?"])
    if k == 7:
        return rregex(rng, depth + 1) + rng.choice(["a*", "b+", "/?", ".*", ".+", "[ab]{0,2}"])
    if k == 8:
        return "^" + rregex(rng, depth + 1)
    if k == 9:
        return rregex(rng, depth + 1) + "$"
    if k == 10:
        return "(?i)" + rng.choice(["A", "aB", "[A-B]/", "S", "Ks", "\u00c9", "[r-t]"]) + rregex(rng, depth + 1)
    if k == 11:
        return "(" + rregex(rng, depth + 1) + ")" + rregex(rng, depth + 1)
    if k == 12:
        return rng.choice(["(?m)^a", "(?m)b$", "(?s)a.b", "a|", "|b", "(a|)", "()", "(?i:a)b"])
    return rregex(rng, depth + 1) + "|" + rregex(rng, depth + 1)


def rpred(rng: random.Random, lists) -> str:
    """One atomic predicate (mostly well-typed, sometimes deliberately not)."""
    k = rng.randint(0, 30)
    f = "http_request." + rng.choice(FIELDS)
    if k <= 4:
        return f"{f}.{rng.choice(['contains', 'starts_with', 'ends_with'])}({q(rstr(rng, 0, 3))})"
    if k <= 6:
        return f"{f} {rng.choice(['==', '!='])} {q(rstr(rng, 0, 3))}"
    if k <= 9:
        return f"{f}.matches({q(rregex(rng))})"
    if k == 10:
        return f"{f}.length() {rng.choice(['==', '!=', '<', '<=', '>', '>='])} {rng.randint(-1, 6)}"
    if k == 11:
        return f"client.remote_port {rng.choice(['==', '!=', '<', '<=', '>', '>='])} {rng.choice([0, 1, 2, 3, 80, 443, 65535, 70000, -5, 2.5, 3.0])}"
    if k == 12:
        return f"client.asn {rng.choice(['==', '<', '>='])} {rng.choice([0, 1, 2, 3, 4294967295, 64512])}"
    if k == 13:
        items = ", ".join(q(rstr(rng, 0, 3)) for _ in range(rng.randint(0, 4)))
        return f"[{items}].contains({f})"
    if k == 14:
        items = ", ".join(str(rng.randint(0, 5)) for _ in range(rng.randint(0, 4)))
        v = rng.choice(["client.asn", "client.remote_port", f + ".length()"])
        return rng.choice([f"[{items}].contains({v})", f"{v} in [{items}]"])
    if k == 15:
        return f"client.country {rng.choice(['==', '!='])} {q(rng.choice(COUNTRIES))}"
    if k == 16:
        items = ", ".join(q(rng.choice(COUNTRIES)) for _ in range(rng.randint(1, 3)))
        return f"[{items}].contains(client.country)"
    if k == 17:
        return f"client.country.{rng.choice(['starts_with', 'ends_with', 'contains'])}({q(rng.choice(['X', 'F', 'R', 'XX', '', 'U']))})"
    if k == 18 and lists:
        ip_lists = [n for n, (t, _) in lists.items() if t == _abi.LIST_IP]
        if ip_lists:
            n = rng.choice(ip_lists)
            return rng.choice([f"lists[{q(n)}].contains(client.ip)", f"client.ip in lists.{n}"])
    if k == 19 and lists:
        s_lists = [n for n, (t, _) in lists.items() if t == _abi.LIST_STRING]
        if s_lists:
            return f"lists[{q(rng.choice(s_lists))}].contains({f})"
    if k == 20 and lists:
        i_lists = [n for n, (t, _) in lists.items() if t == _abi.LIST_INT]
        if i_lists:
            return f"lists[{q(rng.choice(i_lists))}].contains(client.asn)"
    if k == 21:
        return rng.choice(["true", "false", "1 == 1", '"a" < "b"', "1 + 1 == 2", "[1, 2].contains(2)", '"abc".contains("b")', "2 > 3.5", "1 / 0 == 1", '"x".length() == 1'])
    if k == 22:  # statically erroring or ill-typed
        return rng.choice(["http_request.nope == 1", "client.nope", 'lists["missing"].contains(client.ip)', f"{f} && true", "!client.remote_port", "undefined_fn(1)",
                           f'{f}.contains(1)', f"{f}.bogus()", 'client.ip == "1.2.3.4"', "client.remote_port == \"80\"", "1 < \"a\"", f'{f}.matches("(")', "null == null"])
    if k == 23:
        return f"{q(rstr(rng, 1, 5))}.{rng.choice(['contains', 'starts_with', 'ends_with'])}({f})"
    if k == 24:
        return f"{f}.length() {rng.choice(['<', '>='])} {rng.randint(0, 5)}.5"
    if k == 25:
        return f"{f} in [{q(rstr(rng, 0, 2))}, {q(rstr(rng, 0, 3))}]"
    if k == 26:
        return f'http_request["{rng.choice(FIELDS)}"] == {q(rstr(rng, 0, 2))}'
    if k == 27:
        return f'"path" in http_request && {f}.contains({q(rstr(rng, 1, 2))})'
    return f"{f}.contains({q(rstr(rng, 1, 2))})"


def rexpr(rng: random.Random, lists, depth=0) -> str:
    k = rng.randint(0, 9 if depth < 3 else 2)
    if k <= 2:
        return rpred(rng, lists)
    if k == 3:
        return "!" + ("(" + rexpr(rng, lists, depth + 1) + ")")
    if k in (4, 5):
        return "(" + rexpr(rng, lists, depth + 1) + rng.choice([" && ", " || "]) + rexpr(rng, lists, depth + 1) + ")"
    if k == 6:
        return rexpr(rng, lists, depth + 1) + rng.choice([" && ", " || "]) + rexpr(rng, lists, depth + 1)
    if k == 7:
        return "(" + rexpr(rng, lists, depth + 1) + " ? " + rexpr(rng, lists, depth + 1) + " : " + rexpr(rng, lists, depth + 1) + ")"
    if k == 8:
        return "(" + rexpr(rng, lists, depth + 1) + rng.choice([" == ", " != "]) + rexpr(rng, lists, depth + 1) + ")"
    return rpred(rng, lists)


def wide_v4(rng: random.Random) -> str:
    """an IPv4 address from a space wide enough for every third octet (every 32-/24 group of a /16, every summary block) and small
    enough in its first two octets that prefixes and clients still meet"""
    return f"{rng.choice([0, 1, 2, 3, 3, 127, 200, 224, 255])}.{rng.choice([0, 1, 2, 3, 255])}.{rng.randint(0, 255)}.{rng.randint(0, 255)}"


def wide_v6(rng: random.Random) -> str:
    import ipaddress

    if rng.random() < 0.2:
        return rng.choice(["::", "::1", "ff02::1", "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "2001:db8::"])
    v = (0x20010DB8 << 96) | (rng.randint(0, 3) << 80)  # 2001:db8:0-3::/48, then a few bytes anywhere below
    for _ in range(rng.randint(0, 3)):
        v |= rng.randint(0, 255) << (8 * rng.randint(0, 9))
    return str(ipaddress.IPv6Address(v))


def wide_nets(rng: random.Random, n: int, v6_share: float = 0.25):
    return [f"{wide_v6(rng)}/{rng.randint(0, 128)}" if rng.random() < v6_share else f"{wide_v4(rng)}/{rng.randint(0, 32)}" for _ in range(n)]


def address_edges(lists, geo):
    """first / last address of every prefix of the ip lists and the GeoIP entries, and the addresses just outside"""
    import ipaddress

    nets = [ipaddress.ip_network(s.strip(), strict=False) for t, items in (lists or {}).values() if t == _abi.LIST_IP for s in items]
    for e in (geo if geo is not None else []):
        raw = bytes(e["addr"])
        nets.append(ipaddress.ip_network((raw if e["is_v6"] else raw[:4], int(e["prefix_len"])), strict=False))
    out = []
    for net in nets:
        lo, hi, top = int(net.network_address), int(net.broadcast_address), (1 << net.max_prefixlen) - 1
        cls = ipaddress.IPv6Address if net.version == 6 else ipaddress.IPv4Address
        out += [str(cls(a)) for a in (lo, hi, max(lo - 1, 0), min(hi + 1, top))]
    return out


def fuzz_lists(rng: random.Random, wide: bool = False):
    """wide: addresses with every third octet, prefix lengths 0...32 / 0...128 (the committed seeds keep the narrow draw)"""
    if wide:
        return {
            "nets": (_abi.LIST_IP, wide_nets(rng, rng.randint(1, 12))),
            "nets2": (_abi.LIST_IP, wide_nets(rng, rng.randint(0, 5), 0.1) + ["1.1.1.1", " 2.2.2.2 "]),
            "words": (_abi.LIST_STRING, [rstr(rng, 0, 3) for _ in range(rng.randint(0, 6))]),
            "asns": (_abi.LIST_INT, [str(rng.randint(0, 5)) for _ in range(rng.randint(0, 5))] + [" 64512 "]),
        }
    nets = []
    for _ in range(rng.randint(1, 12)):
        if rng.random() < 0.75:
            ln = rng.choice([8, 16, 24, 30, 32, 0, 12, 31])
            nets.append(f"{rng.randint(1, 3)}.{rng.randint(0, 3)}.{rng.randint(0, 3)}.{rng.randint(0, 255)}/{ln}")
        else:
            nets.append(f"2001:db8:{rng.randint(0, 3):x}::{rng.randint(0, 3):x}/{rng.choice([32, 48, 64, 128, 127, 0, 3])}")
    nets2 = [f"{rng.randint(1, 3)}.{rng.randint(0, 3)}.0.0/{rng.choice([14, 15, 16, 23])}" for _ in range(rng.randint(0, 5))] + ["1.1.1.1", " 2.2.2.2 "]
    return {
        "nets": (_abi.LIST_IP, nets),
        "nets2": (_abi.LIST_IP, nets2),
        "words": (_abi.LIST_STRING, [rstr(rng, 0, 3) for _ in range(rng.randint(0, 6))]),
        "asns": (_abi.LIST_INT, [str(rng.randint(0, 5)) for _ in range(rng.randint(0, 5))] + [" 64512 "]),
    }


def fuzz_requests(rng: random.Random, n: int, with_geo: bool, wide: bool = False, edges=()):
    """wide: client addresses from the wide space, half of them from `edges` (address_edges of the lists and the GeoIP table)"""
    reqs = []
    for _ in range(n):
        alpha = UALPHA if rng.random() < 0.3 else ALPHA
        path = rstr(rng, 0, 8, alpha)
        if rng.random() < 0.1:
            path = "/__pingoo/captcha" + path
        ua = rstr(rng, 0, 8, "abM/ ") if rng.random() < 0.9 else rng.choice(["", "x" * 255, "x" * 256, "x" * 290])
        if wide:
            ip = rng.choice(edges) if edges and rng.random() < 0.5 else wide_v6(rng) if rng.random() < 0.25 else wide_v4(rng)
        elif rng.random() < 0.75:
            ip = f"{rng.randint(1, 3)}.{rng.randint(0, 3)}.{rng.randint(0, 3)}.{rng.randint(0, 255)}"
        else:
            ip = rng.choice([f"2001:db8:{rng.randint(0, 3):x}::{rng.randint(0, 3):x}", "::1", "ff02::1", "127.0.0.1", "224.1.2.3", "1.1.1.1", "2.2.2.2"])
        kw = {}
        if with_geo:
            kw = dict(asn=rng.choice([0, 1, 2, 3, 64512, 4294967295]), country=rng.choice(COUNTRIES))
        reqs.append(Request(host=rstr(rng, 0, 6, alpha), url=path + rstr(rng, 0, 4, alpha), path=path, method=rng.choice(["GET", "POST", "a", ""]), user_agent=ua, ip=ip,
                            remote_port=rng.choice([0, 1, 2, 3, 80, 443, 65535, rng.randint(0, 65535)]), captcha_verified=rng.random() < 0.3, **kw))
    return reqs


def fuzz_geoip(rng: random.Random, wide: bool = False):
    from pingoo_amd import geoip_entries

    if wide:
        rows = [(net, rng.choice([0, 1, 2, 3, 64512]), rng.choice(COUNTRIES + ["xx", "F1"])) for net in wide_nets(rng, rng.randint(1, 14))]
        return geoip_entries(rows + [("127.0.0.0/8", 3, "US")])
    rows = []
    for _ in range(rng.randint(1, 10)):
        if rng.random() < 0.7:
            rows.append((f"{rng.randint(1, 3)}.{rng.randint(0, 3)}.0.0/{rng.choice([8, 14, 16, 24])}", rng.choice([0, 1, 2, 3, 64512]), rng.choice(COUNTRIES + ["xx", "F1"])))
        else:
            rows.append((f"2001:db8:{rng.randint(0, 3):x}::/{rng.choice([32, 48, 64])}", rng.choice([1, 2, 3]), rng.choice(COUNTRIES)))
    rows.append(("127.0.0.0/8", 3, "US"))  # must be ignored: loopback is never looked up (geoip.rs:74-76)
    rows.append(("::/0", 2, "DE"))
    return geoip_entries(rows)


def fuzz_actions(rng: random.Random):
    return rng.choice([[B], [CAP], [CAP, B], [B, CAP], [], [CAP, CAP]])


# ---------------------------------------------------------------------------------------------------------
# literal-heavy rule sets: every pattern has a literal factor of two or more bytes, so the compiler puts the passes behind
# the bigram prefilter; requests are built from the same tokens (whole, truncated, case-flipped, glued across
# field boundaries) so that both matches and near misses are frequent
# ---------------------------------------------------------------------------------------------------------
TOKENS = ["/.env", "../", "<script", "union select", "/wp-admin", "cmd.exe", "ab", "Mozilla/", "curl/", "bot", "x9k2", "/api/v1", "=%27", "admin", "select", "q7",
          ".php", "passwd", "etc", "AbCd", "zz", "/a/b", "hello-world", "0x41", "id=", "__", "a.b"]


def lit_token(rng: random.Random) -> str:
    t = rng.choice(TOKENS)
    k = rng.random()
    if k < 0.15 and len(t) > 3:
        t = t[:rng.randint(2, len(t) - 1)]
    elif k < 0.25:
        t = t + rng.choice(TOKENS)
    return t


HEADER_NAMES = ["x-a", "cookie", "x-b"]


def lit_pred(rng: random.Random) -> str:
    f = "http_request." + rng.choice(["host", "url", "path", "user_agent", "url", "path", 'headers["x-a"]', 'headers["cookie"]', "headers.referer"])
    t = lit_token(rng)
    k = rng.randint(0, 13)
    if k == 12:
        return f"{f}.length() {rng.choice(['>', '<=', '=='])} {rng.randint(0, 12)}"
    if k == 13:
        return rng.choice(['"x-a" in http_request.headers', 'http_request.headers.contains("cookie")', '"headers" in http_request', f'{f} == ""'])
    if k <= 2:
        return f"{f}.contains({q(t)})"
    if k == 3:
        return f"{f}.starts_with({q(t)})"
    if k == 4:
        return f"{f}.ends_with({q(t)})"
    if k == 5:
        return f"{f} == {q(t)}"
    esc = "".join("\\" + c if c in ".^$*+?()[]{}|\\/" else c for c in t)
    if k == 6:
        return f"{f}.matches({q('(?i)' + esc)})"
    if k == 7:
        return f"{f}.matches({q(esc + '[0-9]+' + ''.join(chr(92) + c if c in '.^$*+?()[]{}|/' else c for c in lit_token(rng)))})"
    if k == 8:
        return f"{f}.matches({q(esc + '.*' + ''.join(chr(92) + c if c in '.^$*+?()[]{}|/' else c for c in lit_token(rng)))})"
    if k == 9:
        return f"{f}.matches({q('^' + esc + '(x|y|' + esc + ')$')})"
    if k == 10:
        return f"{f}.matches({q('(' + esc + '|' + ''.join(chr(92) + c if c in '.^$*+?()[]{}|/' else c for c in lit_token(rng)) + ')' + chr(92) + 's?=')})"
    return f"!{f}.starts_with({q(t)})"


def lit_rules(rng: random.Random, n: int):
    rules = []
    for k in range(n):
        e = lit_pred(rng)
        s = rng.randint(0, 5)
        if s == 0:
            e = e + " && " + lit_pred(rng)
        elif s == 1:
            e = e + " || " + lit_pred(rng)
        elif s == 2:
            e = "(" + e + " || " + lit_pred(rng) + ") && " + lit_pred(rng)
        rules.append((f"r{k}", e, fuzz_actions(rng)))
    return rules


def lit_field(rng: random.Random, lo=0, hi=6) -> str:
    parts = []
    for _ in range(rng.randint(lo, hi)):
        k = rng.random()
        if k < 0.45:
            parts.append(lit_token(rng))
        elif k < 0.55:
            t = rng.choice(TOKENS)
            parts.append(t.swapcase())
        elif k < 0.7:
            parts.append(str(rng.randint(0, 99999)))
        else:
            parts.append(rstr(rng, 1, 9, "abcdefxyz/.=-_ %"))
    return "".join(parts)


def lit_requests(rng: random.Random, n: int):
    reqs = []
    for _ in range(n):
        path = lit_field(rng, 0, 5)
        ua = lit_field(rng, 1, 4) if rng.random() < 0.95 else ""
        hdrs = {h: lit_field(rng, 0, 3) for h in ["x-a", "cookie", "referer", "x-unused"] if rng.random() < 0.6}
        reqs.append(Request(host=lit_field(rng, 0, 2), url=path + ("?" + lit_field(rng, 0, 4) if rng.random() < 0.6 else ""), path=path,
                            method=rng.choice(["GET", "POST"]), user_agent=ua[:255], ip=f"{rng.randint(1, 3)}.{rng.randint(0, 3)}.0.{rng.randint(0, 255)}",
                            remote_port=rng.randint(0, 65535), captcha_verified=rng.random() < 0.3, headers=hdrs or None))
    return reqs


REWRITTEN = {"rules": 0, "unsupported": 0}  # how often the fuzzers meet a rule the engine does not evaluate (the gap must be measured, not masked)


def as_the_engine_sees(rules, prog, allow=0):
    """The rule list with every rule the engine reports as unsupported (pwaf_program_rule_status; only possible with
    PWAF_OPT_LENIENT) replaced by one that never matches — the engine's documented behaviour for such a rule — so that the oracle can
    check everything else in the set. Since round 3 rules outside the column compiler's reach run in the residual interpreter, so
    the fuzz grammars produce NO such rule: `allow` is how many a test tolerates (default none)."""
    bad = set(prog.unsupported_rules(len(rules)))
    REWRITTEN["rules"] += len(rules)
    REWRITTEN["unsupported"] += len(bad)
    assert len(bad) <= allow, [(i, prog.rule_status(i)[1]) for i in sorted(bad)]
    return [(n, "false" if i in bad else e, a) for i, (n, e, a) in enumerate(rules)], bad


# ---------------------------------------------------------------------------------------------------------
# rule sets pinned to an exact number of scan passes (the engine's capacity limits: 250 passes, 256 list-scan descriptors per launch,
# the verdict kernels' 64-pass bitmap, 32 gated gap passes). The pass count is not monotone in the rule count, so the search walks rule
# counts one compile at a time, and word seeds when it circles, until the count is exact.
# ---------------------------------------------------------------------------------------------------------
CONSONANTS = "bcdfghjklmnpqrstvwxz"
PASS_KINDS = ("confirm_walk", "confirm_literal", "gap", "identity")
_PASS_RATE = {"confirm_walk": 0.66, "confirm_literal": 0.33, "gap": 0.5, "identity": 1.0}  # passes per rule, measured (the search's first guess)
_PASS_OPTS = {"confirm_walk": dict(max_table_bytes=1024), "confirm_literal": dict(max_table_bytes=1024), "gap": {}, "identity": dict(max_table_bytes=1024)}
GAP_MAX = 30


def pass_words(seed: int, n: int):
    """n distinct six-consonant words (no vowel: no English word, no token of the other generators)"""
    rng = random.Random(0x5EED00 + seed)
    seen, out = set(), []
    while len(out) < n:
        w = "".join(rng.choice(CONSONANTS) for _ in range(6))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def kind_rules(kind: str, n: int, seed: int = 0, prefix: str = ""):
    """n rules of one kind and, per rule, the field it reads and the values that make its literals occur:
    confirm_walk    url.matches("<w1>[0-9]+<w2>"): a literal factor and a non-literal middle (a confirm tier that walks)
    confirm_literal url.contains("<w>"): the confirm tier decides the literal (no walk)
    gap             url.matches("<w1>.{0,30}<w2>"): a counted gap (a gated gap pass fed by the literal passes' factors)
    identity        method.matches("<C>[A-Z]{5}$"): no literal factor of two bytes (a method pass walks every request)"""
    B_ = [B, CAP, [CAP, B]]
    rules, tokens = [], []
    if kind == "identity":
        if n > 26 * 3:
            raise ValueError("at most 78 identity rules")
        for k in range(n):
            c, m = chr(ord("A") + k % 26), 5 + k // 26
            rules.append((f"{prefix}i{k}", f'http_request.method.matches("{c}[A-Z]{{{m}}}$")', [B]))
            tokens.append(("method", [c + "QZX" * 3, "x" + c + "Q" * m, c + "Q" * (m - 1), (c + "Z" * m)[:-1] + "0"]))
        return rules, tokens
    w = pass_words(seed * 7 + PASS_KINDS.index(kind), 2 * n)
    for k in range(n):
        a, b = w[2 * k], w[2 * k + 1]
        acts = B_[k % 3] if isinstance(B_[k % 3], list) else [B_[k % 3]]
        if kind == "confirm_walk":
            rules.append((f"{prefix}c{k}", f'http_request.url.matches("{a}[0-9]+{b}")', acts))
            tokens.append(("url", [f"{a}{k % 97}{b}", f"{a}{b}", f"{a[:-1]}7{b}", f"{a}12x{b}", f"{'_' * (k % 16)}{a}0{b}"]))
        elif kind == "confirm_literal":
            rules.append((f"{prefix}l{k}", f'http_request.url.contains("{a}")', acts))
            tokens.append(("url", [a, a[:-1], a[1:], f"{'_' * (k % 16)}{a}", a[:3] + "/" + a[3:]]))
        elif kind == "gap":
            rules.append((f"{prefix}g{k}", f'http_request.url.matches("{a}.{{0,{GAP_MAX}}}{b}")', acts))
            tokens.append(("url", [a + b, a + "x" * (GAP_MAX - 1) + b, a + "y" * GAP_MAX + b, a + "z" * (GAP_MAX + 1) + b, f"{'_' * (k % 16)}{a}-{b}", a[:-1] + "-" + b]))
        else:
            raise ValueError(kind)
    return rules, tokens


class PinnedSet:
    """A rule set and what it compiles to: n_passes (scan passes), n_gated (gated gap passes), n_filtered, n_confirm (passes with a
    confirm tier), n_walk (those of them that walk), opts (the compile options it was pinned with), tokens (per rule: its field and
    the values that make its literals occur — whole, truncated, padded so that they straddle 16-byte chunks)."""

    def __init__(self, rules, tokens, opts, program):
        from table_walker import Tables

        self.rules, self.tokens, self.opts, self.program = rules, tokens, opts, program
        s = program.stats()
        self.n_passes, self.n_gated, self.n_filtered = s["n_dfa_groups"], s["n_gated_groups"], s["n_filtered_groups"]
        groups = Tables(program.dump()).groups
        self.n_confirm = sum(1 for g in groups if g.get("confirm"))
        self.n_walk = sum(1 for g in groups if g.get("confirm") and g.get("confirm_walk"))

    def pass_of_input(self, value: bytes, first: int = 0):
        """the filtered passes from `first` on that the value flags (pwaf_program_confirm_field: the device's own prefilter code)"""
        from pingoo_amd.engine import PwafError

        out = []
        for g in range(first, self.n_passes):
            try:
                if self.program.confirm_field(g, value)[1]:
                    out.append(g)
            except PwafError:
                pass  # (a pass without a prefilter)
        return out


_PINNED = {}


def pinned_passes(kind: str, n: int, seed: int = 0, extra=(), max_seeds: int = 4, max_tries: int = 14) -> PinnedSet:
    """A deterministic rule set of `kind` (PASS_KINDS) that compiles, together with the fixed rules `extra` (e.g. kind_rules of another
    kind), to exactly n scan passes — n GATED gap passes for kind "gap". Fails naming the nearest counts found when n is unreachable."""
    from pingoo_amd.engine import CompiledProgram, UnsupportedExpression

    key = (kind, n, seed, repr(list(extra)))
    if key in _PINNED:
        return _PINNED[key]
    opts = dict(_PASS_OPTS[kind])
    seen = {}
    for s in range(seed, seed + max_seeds):
        r, tried = max(1, round(n / _PASS_RATE[kind])), set()
        for _ in range(max_tries):
            if r in tried or r < 1:
                break  # (circling: next word seed)
            tried.add(r)
            rules, tokens = kind_rules(kind, r, s)
            try:
                prog = CompiledProgram(list(extra) + rules, **opts)
            except UnsupportedExpression:
                seen[(s, r)] = 251  # (refused: more than 250 passes)
                r -= max(1, round(r * 0.02))
                continue
            st = prog.stats()
            c = st["n_gated_groups"] if kind == "gap" else st["n_dfa_groups"]
            seen[(s, r)] = c
            if c == n:
                ps = PinnedSet(list(extra) + rules, [("", [])] * len(extra) + tokens, opts, prog)
                _PINNED[key] = ps
                return ps
            step = round((n - c) / _PASS_RATE[kind] / 2)  # (half the estimate: near the count, one rule at a time)
            r += max(-16, min(16, step if step else (1 if n > c else -1)))
    near = sorted(set(seen.values()), key=lambda c: (abs(c - n), c))[:4]
    raise AssertionError(f"no {kind} rule set compiles to exactly {n} passes (seeds {seed}..{seed + max_seeds - 1}); nearest counts found: {near}")


def pinned_requests(rng: random.Random, ps: PinnedSet, n: int, hit: float = 0.3, rules=None):
    """Requests whose url / method carry the tokens of the set's rules (of `rules`, indices, when given) next to benign filler."""
    idx = [k for k in (rules if rules is not None else range(len(ps.tokens))) if ps.tokens[k][1]]
    reqs = []
    for _ in range(n):
        url, method = [], "GET"
        for _ in range(rng.randint(0, 4)):
            if idx and rng.random() < hit:
                f, vals = ps.tokens[rng.choice(idx)]
                v = rng.choice(vals)
                if f == "method":
                    method = v
                else:
                    url.append(v)
            else:
                url.append(rstr(rng, 1, 12, "abcdefxyz/.=-_0123456789"))
        u = "/" + rng.choice(["", "?", "/", "&"]).join(url)
        reqs.append(Request(host="h.example", url=u, path=u.split("?")[0], method=method, user_agent="ua/" + rstr(rng, 0, 6),
                            ip=f"{rng.randint(1, 3)}.{rng.randint(0, 3)}.0.{rng.randint(0, 255)}", remote_port=rng.randint(0, 65535),
                            captcha_verified=rng.random() < 0.3))
    return reqs


# ---------------------------------------------------------------------------------------------------------
# the hit matrix of PWAF_OPT_RULE_HITS against the oracle's own
# ---------------------------------------------------------------------------------------------------------
def oracle_matrix(oracle, batch, only=None):
    """-> (M, the oracle's verdicts): M[k, i] = rule k evaluates to Bool(true) for request i (or has no expression), cleared where the
    request's verdict is a gate's. `only`: the requests (columns) to fill; the others stay False."""
    st = batch.as_struct(oracle.header_names)
    fn, h, ref = pyoracle.lib().pwaf_oracle_execute_rule, oracle._h, C.byref(st)
    m = np.zeros((oracle.n_rules, batch.n), dtype=bool)
    cols = range(batch.n) if only is None else list(only)
    for k in range(oracle.n_rules):
        for i in cols:
            m[k, i] = fn(h, k, ref, i) == 1
    want = oracle.evaluate(batch)
    m[:, np.isin(want["rule_idx"], (_abi.RULE_UA_GATE, _abi.RULE_CAPTCHA_ENDPOINT))] = False
    return m, want


def assert_hits(label, hits, rule_hits, m):
    n_rules, n = m.shape
    assert (hits["mask"] != 0).all(), f"{label}: an entry with an empty mask"
    pairs = hits["rule_idx"].astype(np.uint64) << np.uint64(32) | hits["group"].astype(np.uint64)
    assert len(np.unique(pairs)) == len(hits), f"{label}: a (rule, group) pair appears twice"
    got = hits_to_matrix(hits, n, n_rules)
    bad = np.argwhere(got != m)
    assert len(bad) == 0, f"{label}: {len(bad)} of {m.size} (rule, request) bits differ; first: rule {bad[0][0]}, request {bad[0][1]}: got {got[tuple(bad[0])]}"
    assert rule_hits.tolist() == m.sum(axis=1).tolist(), f"{label}: rule_hits"
