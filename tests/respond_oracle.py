"""TEST-ONLY: which response the reference's listener gives a request, restated in Python from pingoo/listeners/http_listener.rs:196-272
and pingoo/captcha.rs:158-174 (serve_captcha_request), independently of csrc/respond.h. The inputs are what the batch services answer:
the verdict (how the evaluation reports gates A and B and the rule loop), the verified-cookie status, the route and the path. Shared by
tests/test_respond_cpu.py and tests/test_gpu_respond.py, with the case builders both use."""
from __future__ import annotations

import itertools

import numpy as np

# include/pwaf.h, restated (tests/test_respond_cpu.py compares them with the header's through a C compiler)
FORWARD, NOT_FOUND, BLOCKED, CAPTCHA_PAGE, CAPTCHA_ASSET, CAPTCHA_INIT, CAPTCHA_VERIFY, CAPTCHA_NOT_FOUND, HOST_DECIDES = range(9)
KINDS, MAX_LISTS = 9, 4
ALLOW, BLOCK, CAPTCHA, BYPASS = 0, 1, 2, 3
RULE_NONE, RULE_UA_GATE, RULE_CAPTCHA_ENDPOINT, RULE_COOKIE = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
ABSENT, VERIFIED, INVALID, UNDECIDED = 0, 1, 2, 3
ROUTE_NONE = 0xFFFFFFFF
ARENA_PAD = 16

PREFIX = b"/__pingoo/captcha"
ASSETS, INIT, VERIFY = PREFIX + b"/assets", PREFIX + b"/api/init", PREFIX + b"/api/verify"


def decide(verdict, status, route, path):
    """verdict: (action, rule_idx) as the evaluation answers it; status: the cookie's (None: no column, ABSENT); route: None (no route
    column), an index, or ROUTE_NONE; path: bytes (get_path's value) -> (kind, arg)"""
    action, rule = int(verdict[0]), int(verdict[1])
    status = ABSENT if status is None else int(status)
    # http_listener.rs:196-198: an empty or over-long User-Agent, which the evaluation reports as rule_idx UA_GATE
    if rule == RULE_UA_GATE:
        return BLOCKED, RULE_UA_GATE
    # :200-204: path.starts_with("/__pingoo/captcha") -> serve_captcha_request, which the evaluation reports as BYPASS
    if action == BYPASS:
        # captcha.rs:164-173
        if path.startswith(ASSETS):
            return CAPTCHA_ASSET, RULE_CAPTCHA_ENDPOINT
        elif path == INIT:
            return CAPTCHA_INIT, RULE_CAPTCHA_ENDPOINT
        elif path == VERIFY:
            return CAPTCHA_VERIFY, RULE_CAPTCHA_ENDPOINT
        return CAPTCHA_NOT_FOUND, RULE_CAPTCHA_ENDPOINT
    # :222-236: a cookie that is there and does not validate -> serve_captcha()
    if status == INVALID:
        return CAPTCHA_PAGE, RULE_COOKIE
    # (no reference line: the batch service could not parse a token that a key of the set signed; the host validates it itself)
    if status == UNDECIDED:
        return HOST_DECIDES, rule
    # :251-264: the rule loop's outcome
    if action == BLOCK:
        return BLOCKED, rule
    if action == CAPTCHA:
        return CAPTCHA_PAGE, rule
    # :266-272: the first service whose route matches, else 404
    if route is None:
        return FORWARD, ROUTE_NONE
    route = int(route) & 0xFFFFFFFF
    return (NOT_FOUND, ROUTE_NONE) if route == ROUTE_NONE else (FORWARD, route)


def mask_of(kinds) -> int:
    m = 0
    for k in kinds:
        m |= 1 << k
    return m


def expect_batch(verdicts, statuses, routes, paths, lists=(), caps=None):
    """verdicts: [(action, rule_idx)]; statuses, routes: a sequence or None (no column); paths: [bytes]; lists: [tuple of kinds]; caps: per
    list (None: n) -> (responses [(kind, arg)], counts [KINDS], [(the first min(count, cap) members ascending, count)])"""
    n = len(verdicts)
    resp = [decide(verdicts[i], None if statuses is None else statuses[i], None if routes is None else routes[i], paths[i]) for i in range(n)]
    counts = [0] * KINDS
    for k, _ in resp:
        counts[k] += 1
    caps = [n] * len(lists) if caps is None else list(caps)
    out = []
    for kinds, cap in zip(lists, caps):
        members = [i for i, (k, _) in enumerate(resp) if k in kinds]
        out.append((members[:cap], len(members)))
    return resp, counts, out


# ---- case builders -----------------------------------------------------------------------------------------------------------------------
def path_cases():
    """[(label, path)]: the three literals, each less its last byte and plus one byte, the prefix alone and with another byte, the empty
    path, one outside the prefix, and the lengths 0, 15, 16, 17, 23..29, 32 and 300 both under the prefix's head and as an exact literal's head"""
    cases = []
    for name, lit in (("assets", ASSETS), ("init", INIT), ("verify", VERIFY)):
        cases += [(name, lit), (name + " less its last byte", lit[:-1]), (name + " + x", lit + b"x"), (name + " + /", lit + b"/"), (name + " + 300", lit + b"/" + b"a" * 300)]
    cases += [("the prefix alone", PREFIX), ("the prefix + X", PREFIX + b"X"), ("the prefix + /", PREFIX + b"/"), ("empty", b""), ("outside the prefix", b"/index.html"),
              ("outside, as long as verify", b"/" + b"z" * 27), ("assets with its first byte wrong", b"x" + ASSETS[1:]), ("assets with byte 16 wrong", ASSETS[:16] + b"b" + ASSETS[17:]),
              ("init with its last byte wrong", INIT[:-1] + b"u"), ("verify with byte 24 wrong", VERIFY[:24] + b"x" + VERIFY[25:]), ("init in upper case", INIT.upper())]
    for length in (0, 15, 16, 17, 23, 24, 25, 26, 27, 28, 29, 32, 300):
        for name, base in (("assets", ASSETS), ("init", INIT), ("verify", VERIFY)):
            p = (base + b"/" + b"q" * 300)[:length]
            cases.append((f"{name} cut or filled to {length}", p))
    return cases


ACTIONS = (ALLOW, BLOCK, CAPTCHA, BYPASS)
RULES = (3, RULE_UA_GATE, RULE_CAPTCHA_ENDPOINT, RULE_NONE)
STATUS_COLUMNS = (None, ABSENT, VERIFIED, INVALID, UNDECIDED)  # None: the call gets no column
ROUTE_COLUMNS = (None, 5, ROUTE_NONE)
PATH_CLASSES = (ASSETS + b"/app.js", INIT, VERIFY, PREFIX + b"/nothing", b"/index.html", b"")


def cross_product():
    """every (action, rule_idx, status column, route column, path class): [(verdict, status, route, path)]"""
    return [((a, r), s, t, p) for a, r, s, t, p in itertools.product(ACTIONS, RULES, STATUS_COLUMNS, ROUTE_COLUMNS, PATH_CLASSES)]


def path_column(paths, lead=0, pad=ARENA_PAD):
    """[bytes] -> (data uint8 with `pad` zero bytes behind the last path, offsets uint32), the first path `lead` bytes into the arena"""
    off = np.zeros(len(paths) + 1, dtype=np.uint32)
    if paths:
        off[1:] = np.cumsum([len(p) for p in paths], dtype=np.uint64).astype(np.uint32)
    off += np.uint32(lead)
    return np.frombuffer(b"\xA5" * lead + b"".join(paths) + b"\0" * pad, dtype=np.uint8).copy(), off


def mixed_batch(n, seed=1):
    """n requests over every row of the table: (verdicts, statuses, routes, paths), deterministic"""
    rng = np.random.RandomState(seed)
    pool = cross_product()
    pick = rng.randint(0, len(pool), size=n)
    paths = [p for _, p in path_cases()]
    verdicts, statuses, routes, out_paths = [], [], [], []
    for i, k in enumerate(pick):
        v, s, t, p = pool[k]
        verdicts.append(v)
        statuses.append(ABSENT if s is None else s)
        routes.append(ROUTE_NONE if t is None else (t + i % 3 if t != ROUTE_NONE else t))
        out_paths.append(paths[(i * 7 + k) % len(paths)] if v[0] == BYPASS and i % 2 else p)
    return verdicts, statuses, routes, out_paths
