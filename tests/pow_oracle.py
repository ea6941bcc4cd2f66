"""The oracle of pwaf_verify_pow / pwaf_verify_pow_one: the check CaptchaManager::api_verify runs on a proof-of-work submission
(pingoo/captcha.rs:241-333; jwt/jwt.rs:198-327) restated with hashlib, json and re. A helper, not a test file; written from DESIGN.md
§5.1.7, not from csrc/pow.h: the cookie split with bytes methods, the flat subset plus the one escape as ONE regular expression over the
decoded text, the claims through json.loads (which decodes \\u0000 itself), the leading zeroes counted on the hex form as the reference
counts them, the proof of work with hashlib.sha256 over the decoded challenge and the nonce. Ed25519 and base64url come from
tests/cookie_oracle.py. It also mints challenge tokens (the reference's Header and CaptchaCookieJwtClaims serialised in declaration
order, compactly) and searches a nonce for a given number of leading zero nibbles."""
import hashlib
import json
import re

from cookie_oracle import DROP, b64d, b64e, client_id, header_json, is_int, mint, sign, verify  # noqa: F401 (re-exported for the tests)

ABSENT, PASSED, FAILED, UNDECIDED = 0, 1, 2, 3
COOKIE = b"__pingoo_captcha"
MAX_SIGNED = 8192  # PWAF_COOKIE_MAX_SIGNED_BYTES
NUL = "\0"


# ---- what the reference puts into a token (captcha.rs:589-602: 32 bytes as 43 characters followed by one 0x00 byte) -----------------
def heapless44(raw32):
    """encode_to_base64_heapless::<44, _>: URL_SAFE_NO_PAD into a zeroed 44-byte buffer, all 44 bytes pushed into the string"""
    assert len(raw32) == 32
    return b64e(raw32).decode() + NUL


def client_sub(ip_packed, ua, host):
    """the reference's client id string: the 43 characters and the NUL (the 44 bytes of pwaf_client_id.text)"""
    return client_id(ip_packed, ua, host) + NUL


def claims_json(sub, now, challenge, difficulty, jti="0190b5a2-7c1e-7d43-9f6a-3b2c1d0e4f55", **change):
    """CaptchaCookieJwtClaims in declaration order: challenge, difficulty, then the flattened RegisteredClaims (captcha.rs:61-67;
    jwt.rs:89-124). json.dumps writes a NUL as \\u0000, as serde_json does. change: name=value replaces a member, name=DROP removes it."""
    d = {"challenge": None, "difficulty": None, "iss": "pingoo", "sub": None, "aud": "pingoo", "exp": now + 300, "nbf": now, "iat": now, "jti": None}
    for k, v in [("challenge", challenge), ("difficulty", difficulty), ("sub", sub), ("jti", jti)] + list(change.items()):
        if v is DROP:
            d.pop(k, None)
        else:
            d[k] = v
    return json.dumps(d, separators=(",", ":")).encode()


def zero_nibbles(digest):
    """captcha.rs:311-314: the leading '0' characters of the hex form"""
    text = digest.hex()
    return len(text) - len(text.lstrip("0"))


def search_nonce(challenge, want, exactly=True, start=0, prefix=""):
    """the first decimal counter n >= start for which SHA-256(challenge || prefix || str(n)) has `want` leading zero nibbles (exactly, or
    at least) -> (nonce bytes, digest). `challenge` is the decoded string's bytes."""
    n = start
    while True:
        nonce = (prefix + str(n)).encode()
        digest = hashlib.sha256(challenge + nonce).digest()
        z = zero_nibbles(digest)
        if z == want or (not exactly and z >= want):
            return nonce, digest
        n += 1


# ---- the cookie header (cookie 0.18 Cookie::split_parse behind HeaderValue::to_str): D-C1..D-C3 with this call's name ----------------
def find_cookie(value, name=COOKIE):
    if any(b != 9 and not 0x20 <= b <= 0x7E for b in value):
        return None
    for seg in value.split(b";"):
        seg = seg.strip(b" \t")
        if b"=" not in seg:
            continue
        key, val = seg.split(b"=", 1)
        key, val = key.strip(b" \t"), val.strip(b" \t")
        if not key:
            continue
        if key == name:
            return val[1:-1] if len(val) >= 2 and val[:1] == b'"' and val[-1:] == b'"' else val
    return None


# ---- the flat subset, without and with the escape ------------------------------------------------------------------------------------
_PLAIN = r"[\x20\x21\x23-\x5B\x5D-\x7E]"
_NAME = rf'"{_PLAIN}*"'
_W = r"[ \t\n\r]*"


def _flat_re(string):
    value = rf"(?:{string}|-?(?:0|[1-9][0-9]*)(?![.eE0-9])|true|false|null)"
    pair = rf"{_NAME}{_W}:{_W}{value}{_W}"
    return re.compile(rf"{_W}\{{{_W}(?:{pair}(?:,{_W}{pair})*)?\}}{_W}\Z")


FLAT_RE = {False: _flat_re(_NAME), True: _flat_re(rf'"(?:{_PLAIN}|\\u0000)*"')}
HEADER_NAMES = ("typ", "alg", "kid", "cty", "jku", "x5u", "x5t", "x5t#S256", "x5c")
CLAIM_NAMES = ("challenge", "difficulty", "iss", "sub", "aud", "exp", "nbf", "iat", "jti")


def flat(raw, names, escape):
    """the object as a dict (null members dropped), or None: outside the subset, or a name of `names` twice"""
    if raw is None:
        return None
    try:
        text = raw.decode("ascii")
    except UnicodeDecodeError:
        return None
    if not FLAT_RE[escape].match(text):
        return None
    if re.search(r"[:][ \t\n\r]*-0(?![0-9])", re.sub(r'"[^"]*"', '""', text)):  # "-0": serde_json reads a float (no string holds a '"' here)
        return None
    pairs = json.loads(text, object_pairs_hook=list)
    keys = [k for k, _ in pairs]
    if any(keys.count(k) > 1 for k in names):
        return None
    if any(is_int(v) and not -2**63 <= v < 2**63 for _, v in pairs):
        return None
    return {k: v for k, v in pairs if v is not None}


# ---- the decision -------------------------------------------------------------------------------------------------------------------------
def decide(keys, cookie_header, digest, nonce, now, ip_packed, ua, host):
    """keys: [(kid str, x bytes)]; cookie_header: the first Cookie header's value (bytes) or None; digest: the body's 32 hash bytes;
    nonce: the body's nonce (bytes) -> (status, handed): handed is True when the signature stage was asked (rules 3, 4 and 6)"""
    token = None if cookie_header is None else find_cookie(cookie_header)
    if token is None:
        return ABSENT, False
    parts = token.split(b".")
    if len(parts) != 3:
        return FAILED, False
    sig = b64d(parts[2])
    if sig is None or len(sig) != 64:
        return FAILED, False
    msg = parts[0] + b"." + parts[1]
    header = flat(b64d(parts[0]), HEADER_NAMES, False) if len(msg) <= MAX_SIGNED else None
    if header is not None:
        if any(not isinstance(header.get(k, ""), str) for k in ("cty", "jku", "x5u", "x5t", "x5t#S256")) or "x5c" in header:
            header = None
    if header is None:
        return (UNDECIDED if any(verify(x, msg, sig) for _, x in keys) else FAILED), True
    key = next((x for kid, x in keys if kid == header.get("kid")), None)
    if key is None or header.get("alg") != "EdDSA" or header.get("typ") != "JWT":
        return FAILED, False
    claims = flat(b64d(parts[1]), CLAIM_NAMES, True)
    if claims is None or not is_int(claims.get("iat", 0)) or not isinstance(claims.get("jti", ""), str):
        return (UNDECIDED if verify(key, msg, sig) else FAILED), True
    exp, nbf, difficulty, challenge = claims.get("exp"), claims.get("nbf"), claims.get("difficulty"), claims.get("challenge")
    ok = is_int(exp) and exp >= now - 5 and is_int(nbf) and nbf <= now + 5
    ok = ok and claims.get("aud") == "pingoo" and claims.get("iss") == "pingoo"
    ok = ok and claims.get("sub") == client_sub(ip_packed, ua, host)
    ok = ok and isinstance(challenge, str) and is_int(difficulty) and 0 <= difficulty <= 255
    ok = ok and zero_nibbles(digest) >= difficulty
    ok = ok and hashlib.sha256(challenge.encode("latin-1") + nonce).digest() == digest
    if not ok:
        return FAILED, False
    return (PASSED if verify(key, msg, sig) else FAILED), True
