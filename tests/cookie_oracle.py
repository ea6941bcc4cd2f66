"""The oracle of pwaf_verify_cookies / pwaf_verify_cookie_one: gate C of the reference (http_listener.rs:169-181, :222-236;
pingoo/captcha.rs:125-156; jwt/jwt.rs:198-327) restated with Python's own integers, hashlib, base64, json and re. A helper, not a test
file; written from DESIGN.md §5.1.6 and RFC 8032, not from csrc/cookie.h: Ed25519 on Python integers as RFC 8032 §6 writes it, the
cookie split with str methods, the flat subset as ONE regular expression over the decoded text, the claims through json.loads.
It also mints tokens: the reference's Header and CaptchaVerifiedCookieJwtClaims serialised in declaration order, compactly (what
serde_json::to_string writes), signed with a seed."""
import base64
import hashlib
import json
import re

ABSENT, VERIFIED, INVALID, UNDECIDED = 0, 1, 2, 3
COOKIE = "__pingoo_captcha_verified"
MAX_SIGNED = 8192  # PWAF_COOKIE_MAX_SIGNED_BYTES

# ---- Ed25519 (RFC 8032 §5.1, §6) on Python integers -------------------------------------------------------------------
P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)


def point_add(a, b):
    """RFC 8032 §6: extended homogeneous coordinates (X, Y, Z, T), x = X/Z, y = Y/Z, x y = T/Z"""
    A, B = (a[1] - a[0]) * (b[1] - b[0]) % P, (a[1] + a[0]) * (b[1] + b[0]) % P
    C, Dd = 2 * a[3] * b[3] * D % P, 2 * a[2] * b[2] % P
    E, F, G, H = B - A, Dd - C, Dd + C, B + A
    return (E * F % P, G * H % P, F * G % P, E * H % P)


def point_mul(s, pt):
    q = (0, 1, 1, 0)
    while s:
        if s & 1:
            q = point_add(q, pt)
        pt = point_add(pt, pt)
        s >>= 1
    return q


def recover_x(y, sign):
    if y >= P:
        return None
    x2 = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
    if x2 == 0:
        return None if sign else 0
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * SQRT_M1 % P
    if (x * x - x2) % P:
        return None
    return P - x if (x & 1) != sign else x


BASE_Y = 4 * pow(5, P - 2, P) % P
BASE_X = recover_x(BASE_Y, 0)
BASE = (BASE_X, BASE_Y, 1, BASE_X * BASE_Y % P)


def encode_point(pt):
    zi = pow(pt[2], P - 2, P)
    x, y = pt[0] * zi % P, pt[1] * zi % P
    return (y | (x & 1) << 255).to_bytes(32, "little")


def decode_point(b):
    """None: not the canonical encoding of a point on the curve"""
    y = int.from_bytes(b, "little")
    sign, y = y >> 255, y & (2**255 - 1)
    x = recover_x(y, sign)
    return None if x is None else (x, y, 1, x * y % P)


def secret_expand(seed):
    h = hashlib.sha512(seed).digest()
    a = int.from_bytes(h[:32], "little")
    a &= (1 << 254) - 8
    a |= 1 << 254
    return a, h[32:]


def public_key(seed):
    return encode_point(point_mul(secret_expand(seed)[0], BASE))


def sign(seed, msg):
    a, prefix = secret_expand(seed)
    pub = encode_point(point_mul(a, BASE))
    r = int.from_bytes(hashlib.sha512(prefix + msg).digest(), "little") % L
    rs = encode_point(point_mul(r, BASE))
    h = int.from_bytes(hashlib.sha512(rs + pub + msg).digest(), "little") % L
    return rs + ((r + h * a) % L).to_bytes(32, "little")


def verify(pub, msg, sig):
    """aws-lc's ED25519_verify: S < L, R' = [S]B - [k]A encoded and compared with R byte for byte; R is not decompressed"""
    if len(sig) != 64:
        return False
    a = decode_point(pub)
    s = int.from_bytes(sig[32:], "little")
    if a is None or s >= L:
        return False
    k = int.from_bytes(hashlib.sha512(sig[:32] + pub + msg).digest(), "little") % L
    neg_a = ((P - a[0]) % P, a[1], 1, (P - a[3]) % P)
    return encode_point(point_add(point_mul(s, BASE), point_mul(k, neg_a))) == sig[:32]


def self_check():
    """RFC 8032 §7.1 TEST 1"""
    seed = bytes.fromhex("9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60")
    pub = bytes.fromhex("d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a")
    sig = bytes.fromhex("e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b")
    assert public_key(seed) == pub and sign(seed, b"") == sig and verify(pub, b"", sig)
    assert not verify(pub, b"x", sig)


self_check()


# ---- base64url without padding ----------------------------------------------------------------------------------------------
B64_RE = re.compile(rb"[A-Za-z0-9_-]*\Z")


def b64e(b):
    return base64.urlsafe_b64encode(b).rstrip(b"=")


def b64d(t):
    """None: a foreign byte, a '=', a length of 1 mod 4 or non-zero trailing bits"""
    if not B64_RE.match(t) or len(t) % 4 == 1:
        return None
    raw = base64.urlsafe_b64decode(t + b"=" * (-len(t) % 4))
    return raw if b64e(raw) == t else None


# ---- the client id (captcha.rs:409-421) -----------------------------------------------------------------------------------------
def client_id(ip_packed, ua, host):
    return b64e(hashlib.sha256(ip_packed + ua + host).digest()).decode()


# ---- minting ----------------------------------------------------------------------------------------------------------------
def header_json(kid, alg="EdDSA", typ="JWT"):
    """jwt::Header in declaration order, None members skipped (jwt.rs:36-85)"""
    d = {"typ": typ, "alg": alg}
    if kid is not None:
        d["kid"] = kid
    return json.dumps(d, separators=(",", ":")).encode()


def claims_json(sub, now, jti="0190b5a2-7c1e-7d43-9f6a-3b2c1d0e4f55", **change):
    """CaptchaVerifiedCookieJwtClaims in declaration order (captcha.rs:70-75, :478-489; jwt.rs:89-124). change: name=value replaces a
    member, name=DROP removes it."""
    d = {"challenge_passed": True, "iss": "pingoo", "sub": sub, "aud": "pingoo", "exp": now + 86400, "nbf": now, "iat": now, "jti": jti}
    for k, v in [("sub", sub), ("jti", jti)] + list(change.items()):
        if v is DROP:
            d.pop(k, None)
        else:
            d[k] = v
    return json.dumps(d, separators=(",", ":")).encode()


DROP = object()


def mint(seed, header, claims):
    """header and claims are the JSON texts (bytes) -> the token (bytes)"""
    msg = b64e(header) + b"." + b64e(claims)
    return msg + b"." + b64e(sign(seed, msg))


# ---- the cookie header (cookie 0.18 Cookie::split_parse behind HeaderValue::to_str) ---------------------------------------------------
def find_cookie(value):
    """the first cookie named COOKIE -> its value (bytes), or None"""
    if any(b != 9 and not 0x20 <= b <= 0x7E for b in value):
        return None
    for seg in value.split(b";"):
        seg = seg.strip(b" \t")
        if not seg or b"=" not in seg:
            continue
        name, val = seg.split(b"=", 1)
        name, val = name.strip(b" \t"), val.strip(b" \t")
        if not name:
            continue
        if len(val) >= 2 and val[:1] == b'"' and val[-1:] == b'"':
            val = val[1:-1]
        if name == COOKIE.encode():
            return val
    return None


# ---- the flat subset ----------------------------------------------------------------------------------------------------------
_S = r'"[\x20\x21\x23-\x5B\x5D-\x7E]*"'
_V = rf"(?:{_S}|-?(?:0|[1-9][0-9]*)(?![.eE0-9])|true|false|null)"
_W = r"[ \t\n\r]*"
FLAT_RE = re.compile(rf"{_W}\{{{_W}(?:{_S}{_W}:{_W}{_V}{_W}(?:,{_W}{_S}{_W}:{_W}{_V}{_W})*)?\}}{_W}\Z")
HEADER_NAMES = ("typ", "alg", "kid", "cty", "jku", "x5u", "x5t", "x5t#S256", "x5c")
CLAIM_NAMES = ("challenge_passed", "iss", "sub", "aud", "exp", "nbf", "iat", "jti")


def is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def flat(raw, names):
    """the object as a dict (null members dropped), or None: outside the subset, or a name of `names` twice"""
    if raw is None:
        return None
    try:
        text = raw.decode("ascii")
    except UnicodeDecodeError:
        return None
    if not FLAT_RE.match(text) or re.search(r'[:,{][ \t\n\r]*-0(?![0-9])', re.sub(_S, '""', text)):
        return None
    pairs = json.loads(text, object_pairs_hook=list)
    keys = [k for k, _ in pairs]
    if any(keys.count(k) > 1 for k in names):
        return None
    if any(is_int(v) and not -2**63 <= v < 2**63 for _, v in pairs):
        return None
    return {k: v for k, v in pairs if v is not None}


def decide(keys, cookie_header, now, ip_packed, ua, host):
    """keys: [(kid str, x bytes)]; cookie_header: the first Cookie header's value (bytes) or None -> the status"""
    token = None if cookie_header is None else find_cookie(cookie_header)
    if token is None:
        return ABSENT
    parts = token.split(b".")
    if len(parts) != 3:
        return INVALID
    sig = b64d(parts[2])
    if sig is None or len(sig) != 64:
        return INVALID
    msg = parts[0] + b"." + parts[1]
    header = flat(b64d(parts[0]), HEADER_NAMES) if len(msg) <= MAX_SIGNED else None
    if header is not None:
        if any(not isinstance(header.get(k, ""), str) for k in ("cty", "jku", "x5u", "x5t", "x5t#S256")) or "x5c" in header:
            header = None
    if header is None:
        return UNDECIDED if any(verify(x, msg, sig) for _, x in keys) else INVALID
    key = next((x for kid, x in keys if kid == header.get("kid")), None)
    if key is None or header.get("alg") != "EdDSA" or header.get("typ") != "JWT":
        return INVALID
    if not verify(key, msg, sig):
        return INVALID
    claims = flat(b64d(parts[1]), CLAIM_NAMES)
    if claims is None or not is_int(claims.get("iat", 0)) or not isinstance(claims.get("jti", ""), str):
        return UNDECIDED
    exp, nbf = claims.get("exp"), claims.get("nbf")
    ok = is_int(exp) and exp >= now - 5 and is_int(nbf) and nbf <= now + 5
    ok = ok and claims.get("aud") == "pingoo" and claims.get("iss") == "pingoo" and claims.get("challenge_passed") is True
    ok = ok and claims.get("sub") == client_id(ip_packed, ua, host)
    return VERIFIED if ok else INVALID
