"""pwaf_verify_cookies in HOST mode and pwaf_verify_cookie_one (no GPU, no HIP call): gate C of the reference (http_listener.rs:169-181,
:222-236; captcha.rs:125-156; jwt.rs:198-327) against the independent oracle of tests/cookie_oracle.py, status for status, over a corpus
of labelled cases — the valid token, every single-claim defect, the time edges, the key choice, the signature edges (each of the 512 bits,
S + L, S = L, the top bits of S, every SHA-512 padding edge), the base64 edges, the cookie-header edges, the flat subset's edges behind a
good signature — then list shapes against a canary, every refusal, key-set creation, load_captcha_jwks, and csrc/cookie.h alone under
AddressSanitizer + UBSan as a stand-alone program (tests/cookie_host.cpp) over exact-size heap blocks. Each corpus case also carries the
status it is there to show, so the oracle itself is pinned."""
import ctypes as C
import functools
import ipaddress
import json
import os
import random
import subprocess

import numpy as np
import pytest

import cookie_oracle as O
from pingoo_amd import KeySet, Request, RequestBatch, _abi, verify_cookie, verify_cookies
from pingoo_amd.config import ConfigError, load_captcha_jwks
from pingoo_amd.engine import PwafError, RuleEngine, cookie_column, lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "cookie_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "pingoo_amd", "csrc", "cookie.h"), os.path.join(ROOT, "pingoo_amd", "csrc", "clientid.h"), os.path.join(ROOT, "pingoo_amd", "csrc", "service.h"), os.path.join(ROOT, "include", "pwaf.h")]
A, V, I, U = O.ABSENT, O.VERIFIED, O.INVALID, O.UNDECIDED
NOW = 1_800_000_000
NAME = b"__pingoo_captcha_verified"
ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"
ZERO = b"\0"

SEEDS = [bytes([7 * k + 1] * 32) for k in range(3)]
KIDS = ["k1", "captcha-2", "0190b5a2-7c1e-7d43-9f6a-3b2c1d0e4f-k3"]  # 2, 9 and 37 bytes: the header's length in all three residues mod 3
KEYS = [(kid, O.public_key(seed)) for kid, seed in zip(KIDS, SEEDS)]
OTHER_SEED = bytes([0xC3] * 32)  # a key that is not in the set

IP4, IP6, UA, HOST = "203.0.113.7", "2001:db8:0:7::9", b"Mozilla/5.0 (X11; Linux x86_64) Gecko/20100101 Firefox/128.0", b"shop.example.com"


def packed(ip):
    return ipaddress.ip_address(ip).packed


def cid(ip=IP4, ua=UA, host=HOST):
    return O.client_id(packed(ip), ua, host)


def token(key=0, header=None, claims=None, seed=None, **change):
    """a token of client (IP4, UA, HOST) under key `key`; header / claims: the JSON text instead of the reference's; change: claims_json's"""
    header = O.header_json(KIDS[key]) if header is None else header
    claims = O.claims_json(change.pop("sub", cid()), NOW, **change) if claims is None else claims
    return O.mint(SEEDS[key] if seed is None else seed, header, claims)


def with_signature(tok, fn):
    """the token with its 64 signature bytes replaced by fn(bytes)"""
    h, c, s = tok.split(b".")
    return h + b"." + c + b"." + O.b64e(fn(O.b64d(s)))


def scalar(sig, fn):
    return sig[:32] + (fn(int.from_bytes(sig[32:], "little")) % 2**256).to_bytes(32, "little")


class Case:
    def __init__(self, label, expect, cookie, ip=IP4, ua=UA, host=HOST, now=NOW):
        self.label, self.expect, self.cookie, self.ip, self.ua, self.host, self.now = label, expect, cookie, ip, ua, host, now

    def oracle(self):
        return O.decide(KEYS, self.cookie, self.now, packed(self.ip), self.ua, self.host)

    def request(self):
        return Request(host=self.host, url=b"/u", path=b"/p", method=b"GET", user_agent=self.ua, ip=self.ip)


def padding_edge_tokens():
    """valid tokens whose hashed length 64 + len(message) is each of 367, 368, 383, 384, 385 (111, 112, 127, 0, 1 mod 128: the 0x80 byte and the
    length word on both sides of a block edge) and 495, 496 (one block more), found by varying the key (its kid's length) and the jti"""
    found = {}
    for total in (367, 368, 383, 384, 385, 495, 496):
        for key in range(3):
            for jti_len in range(0, 220):
                tok = None
                h, c = O.b64e(O.header_json(KIDS[key])), O.b64e(O.claims_json(cid(), NOW, jti="j" * jti_len))
                if 64 + len(h) + 1 + len(c) == total:
                    tok = token(key, jti="j" * jti_len)
                    break
            if tok:
                found[total] = tok
                break
    return found


@functools.lru_cache(maxsize=None)
def corpus():
    """every labelled case but the 512 bit flips (bit_flip_cases) -> [Case]"""
    good = token()
    ck = lambda t: NAME + b"=" + t  # noqa: E731
    cs = [Case("the valid token", V, ck(good)), Case("the valid token, IPv6 client", V, ck(token(sub=cid(IP6))), ip=IP6)]
    # single-claim defects
    for name in ("challenge_passed", "iss", "sub", "aud", "exp", "nbf"):
        cs.append(Case(f"claim {name} missing", I, ck(token(**{name: O.DROP}))))
        cs.append(Case(f"claim {name} null", I, ck(token(**{name: None}))))
    for name in ("iat", "jti"):
        cs.append(Case(f"optional claim {name} missing", V, ck(token(**{name: O.DROP}))))
        cs.append(Case(f"optional claim {name} null", V, ck(token(**{name: None}))))
    for name, wrong in (("exp", str(NOW + 9)), ("nbf", str(NOW)), ("aud", 5), ("iss", 5), ("challenge_passed", "true"), ("challenge_passed", 1), ("sub", 5), ("exp", True)):
        cs.append(Case(f"claim {name} of the wrong type ({wrong!r})", I, ck(token(**{name: wrong}))))
    for name, wrong in (("aud", "pingo"), ("aud", "pingoo2"), ("iss", "Pingoo"), ("iss", ""), ("challenge_passed", False), ("sub", cid()[:42]), ("sub", cid() + "A"),
                        ("sub", cid()[:-1] + ("A" if cid()[-1] != "A" else "B"))):
        cs.append(Case(f"claim {name} with the wrong value ({wrong!r})", I, ck(token(**{name: wrong}))))
    for what, kw in (("ip", dict(ip="203.0.113.8")), ("User-Agent", dict(ua=UA + b"x")), ("host", dict(host=b"shop.example.org")), ("address family", dict(ip=IP6))):
        cs.append(Case(f"sub of another {what}", I, ck(good), **kw))
    for what, kw in (("ip", dict(ip="2001:db8:0:7::a")), ("User-Agent", dict(ua=b"")), ("host", dict(host=b"")), ("address family", dict(ip=IP4))):
        cs.append(Case(f"IPv6 client: sub of another {what}", I, ck(token(sub=cid(IP6))), **{"ip": IP6, **kw}))
    # the time edges: exp >= now - 5, nbf <= now + 5
    for d, want in ((-6, I), (-5, V), (-4, V)):
        cs.append(Case(f"exp = now{d:+d}", want, ck(token(exp=NOW + d))))
    for d, want in ((4, V), (5, V), (6, I)):
        cs.append(Case(f"nbf = now{d:+d}", want, ck(token(nbf=NOW + d))))
    cs.append(Case("negative exp", I, ck(token(exp=-5))))
    # key choice
    cs.append(Case("an unknown kid", I, ck(token(header=O.header_json("nobody")))))
    cs.append(Case("a key outside the set under a kid of the set", I, ck(token(seed=OTHER_SEED))))
    cs.append(Case("the token under the second key", V, ck(token(1))))
    cs.append(Case("the token under the third key", V, ck(token(2))))
    cs.append(Case("the second key's kid, the first key's signature", I, ck(token(0, header=O.header_json(KIDS[1])))))
    cs.append(Case("alg ES256", I, ck(token(header=O.header_json(KIDS[0], alg="ES256")))))
    cs.append(Case("alg none", I, ck(token(header=O.header_json(KIDS[0], alg="none")))))
    cs.append(Case("typ JWS", I, ck(token(header=O.header_json(KIDS[0], typ="JWS")))))
    cs.append(Case("no kid", I, ck(token(header=O.header_json(None)))))
    cs.append(Case("kid null", I, ck(token(header=b'{"typ":"JWT","alg":"EdDSA","kid":null}'))))
    cs.append(Case("no typ", I, ck(token(header=b'{"alg":"EdDSA","kid":"k1"}'))))
    cs.append(Case("header members in another order, with blanks", V, ck(token(header=b' { "kid" : "k1" ,\t"alg":"EdDSA",\r\n"typ":"JWT","zip":null, "extra":7 } '))))
    nested = b'{"typ":"JWT","alg":"EdDSA","kid":"k1","jwk":{"kty":"OKP"}}'
    cs.append(Case("a header outside the subset, good signature", U, ck(token(header=nested))))
    cs.append(Case("a header outside the subset, good signature of the third key", U, ck(token(2, header=nested))))
    cs.append(Case("a header outside the subset, a key outside the set", I, ck(token(header=nested, seed=OTHER_SEED))))
    cs.append(Case("a header outside the subset, bad signature", I, ck(with_signature(token(header=nested), lambda s: s[:5] + bytes([s[5] ^ 1]) + s[6:]))))
    cs.append(Case("a header with x5c, good signature", U, ck(token(header=b'{"typ":"JWT","alg":"EdDSA","kid":"k1","x5c":"a"}'))))
    cs.append(Case("a header with cty of the wrong type, good signature", U, ck(token(header=b'{"typ":"JWT","alg":"EdDSA","kid":"k1","cty":5}'))))
    cs.append(Case("a header with typ twice, good signature", U, ck(token(header=b'{"typ":"JWT","alg":"EdDSA","kid":"k1","typ":"JWT"}'))))
    # signature edges
    cs.append(Case("S + L", I, ck(with_signature(good, lambda s: scalar(s, lambda x: x + O.L)))))
    cs.append(Case("S = L", I, ck(with_signature(good, lambda s: scalar(s, lambda x: O.L)))))
    cs.append(Case("S = 0", I, ck(with_signature(good, lambda s: scalar(s, lambda x: 0)))))
    for bit in (255, 254, 253):
        cs.append(Case(f"S with bit {bit} set", I, ck(with_signature(good, lambda s, bit=bit: scalar(s, lambda x: x | 1 << bit)))))
    h, c, s = good.split(b".")
    for part, text in (("header", h), ("claims", c)):
        other = bytes([text[3] ^ 1]) if chr(text[3] ^ 1).isalnum() else b"A"
        changed = text[:3] + other + text[4:]
        cs.append(Case(f"one byte of the {part} changed", I, ck((changed if part == "header" else h) + b"." + (changed if part == "claims" else c) + b"." + s)))
    edges = padding_edge_tokens()
    assert sorted(edges) == [367, 368, 383, 384, 385, 495, 496], sorted(edges)
    for total, tok in edges.items():
        cs.append(Case(f"valid, {total} hashed bytes", V, ck(tok)))
        cs.append(Case(f"bad, {total} hashed bytes", I, ck(with_signature(tok, lambda s: s[:40] + bytes([s[40] ^ 0x10]) + s[41:]))))
    shapes = {(len(O.header_json(KIDS[k])) % 3, len(O.claims_json(cid(), NOW, jti="j" * j)) % 3) for k in range(3) for j in range(3)}
    assert len(shapes) == 9
    for k in range(3):
        for j in range(3):
            cs.append(Case(f"valid, key {k}, jti of {j} bytes", V, ck(token(k, jti="j" * j))))
    # base64 edges
    cs.append(Case("a '=' behind the signature", I, ck(good + b"=")))
    cs.append(Case("a '=' inside the signature", I, ck(h + b"." + c + b"." + s[:40] + b"=" + s[41:])))
    cs.append(Case("a signature part of 85 characters", I, ck(h + b"." + c + b"." + s[:85])))
    cs.append(Case("non-zero trailing bits in the signature part", I, ck(h + b"." + c + b"." + s[:85] + bytes([ALPHABET[ALPHABET.index(s[85]) | 1]]))))
    cs.append(Case("a signature of 63 bytes", I, ck(with_signature(good, lambda b: b[:63]))))
    cs.append(Case("a signature of 65 bytes", I, ck(with_signature(good, lambda b: b + b"\0"))))
    cs.append(Case("a signature with a foreign byte", I, ck(h + b"." + c + b"." + s[:10] + b"+" + s[11:])))
    cs.append(Case("two parts", I, ck(h + b"." + c)))
    cs.append(Case("four parts", I, ck(good + b".AAAA")))
    cs.append(Case("one part", I, ck(h)))
    cs.append(Case("an empty value", I, NAME + b"="))
    cs.append(Case("a header part that is not base64, signed", U, ck(sign_raw(b"!!!!", c))))
    cs.append(Case("a header part of 1 mod 4 characters, signed", U, ck(sign_raw(h + b"A", c))))
    cs.append(Case("a header part with trailing bits, signed", U, ck(sign_raw(O.b64e(O.header_json("k1"))[:-1] + b"_", c))))
    cs.append(Case("a claims part that is not base64, signed", U, ck(sign_raw(h, b"%%%"))))
    cs.append(Case("an empty header part, signed", U, ck(sign_raw(b"", c))))
    cs.append(Case("an empty claims part, signed", U, ck(sign_raw(h, b""))))
    cs.append(Case("a header part that is not base64, not signed", I, ck(b"!!!!." + c + b"." + s)))
    # cookie header edges
    cs.append(Case("no Cookie header", A, None))
    cs.append(Case("an empty Cookie header", A, b""))
    cs.append(Case("a byte 0x80 in the value", A, ck(good) + b"; a=\x80"))
    cs.append(Case("a byte 0x7F in the value", A, b"a=\x7f; " + ck(good)))
    cs.append(Case("a NUL in the value", A, ck(good) + b"\0"))
    cs.append(Case("other cookies only", A, b"session=abc; theme=dark"))
    cs.append(Case("the cookie first", V, ck(good) + b"; a=b; c=d"))
    cs.append(Case("the cookie in the middle", V, b"a=b; " + ck(good) + b"; c=d"))
    cs.append(Case("the cookie last", V, b"a=b; c=d; " + ck(good)))
    cs.append(Case("the same name twice, the first valid", V, ck(good) + b"; " + ck(b"junk")))
    cs.append(Case("the same name twice, the first invalid", I, ck(b"junk") + b"; " + ck(good)))
    cs.append(Case("the name in another case", A, b"__Pingoo_captcha_verified=" + good))
    cs.append(Case("a name that ends with the real one", A, b"x" + ck(good)))
    cs.append(Case("a name that begins with the real one", A, NAME + b"2=" + good))
    cs.append(Case("a name with a blank inside", A, b"__pingoo_captcha _verified=" + good))
    cs.append(Case("blanks and tabs around name and value", V, b"a=b;\t " + NAME + b" \t=\t  " + good + b" \t ; c=d"))
    cs.append(Case("a quoted value", V, NAME + b'="' + good + b'"'))
    cs.append(Case("a quoted value with blanks around it", V, b"a=b; " + NAME + b'= "' + good + b'" '))
    cs.append(Case("a value with only an opening quote", I, NAME + b'="' + good))
    cs.append(Case("a value that is one quote", I, NAME + b'="'))
    cs.append(Case("empty segments", V, b";; ;\t;" + ck(good) + b";;"))
    cs.append(Case("a segment without '='", V, b"flag; " + ck(good)))
    cs.append(Case("the name without '='", A, NAME + b"; a=b"))
    cs.append(Case("a segment with an empty name", V, b"=x; " + ck(good)))
    cs.append(Case("the name as another cookie's value", A, b"a=" + ck(good)))
    cs.append(Case("'=' inside the value", I, ck(good + b"=x")))
    # the flat subset behind a good signature
    base = O.claims_json(cid(), NOW)
    for what, claims, want in (
        ("an escape in a string", base.replace(b'"jti":"0190', b'"jti":"\\u0030190'), U),
        ("an escaped quote in a string", base.replace(b'"jti":"0190', b'"jti":"\\"0190'), U),
        ("iat 1.0", base.replace(b'"iat":%d' % NOW, b'"iat":1.0'), U),
        ("exp 1e3", base.replace(b'"exp":%d' % (NOW + 86400), b'"exp":1e3'), U),
        ("exp as a fraction", base.replace(b'"exp":%d' % (NOW + 86400), b'"exp":%d.5' % (NOW + 86400)), U),
        ("a nested object", base[:-1] + b',"ctx":{"a":1}}', U),
        ("a nested array", base[:-1] + b',"ctx":[1]}', U),
        ("a duplicate key", base[:-1] + b',"exp":1}', U),
        ("a duplicate of an unknown key", base[:-1] + b',"x":1,"x":2}', V),
        ("an integer beyond int64", base.replace(b'"iat":%d' % NOW, b'"iat":9223372036854775808'), U),
        ("int64's largest", base.replace(b'"exp":%d' % (NOW + 86400), b'"exp":9223372036854775807'), V),
        ("int64's smallest", base.replace(b'"nbf":%d' % NOW, b'"nbf":-9223372036854775808'), V),
        ("below int64", base.replace(b'"nbf":%d' % NOW, b'"nbf":-9223372036854775809'), U),
        ("minus zero", base.replace(b'"iat":%d' % NOW, b'"iat":-0'), U),
        ("a leading zero", base.replace(b'"iat":%d' % NOW, b'"iat":01'), U),
        ("a byte above 0x7E in a string", base.replace(b'"jti":"0190', b'"jti":"\xc3\xa9190'), U),
        ("iat of the wrong type", base.replace(b'"iat":%d' % NOW, b'"iat":"x"'), U),
        ("jti of the wrong type", base.replace(b'"jti":"', b'"jti":7,"j":"'), U),
        ("not an object", b"[1]", U),
        ("an empty object", b"{}", I),
        ("nothing", b"", U),
        ("text behind the object", base + b"x", U),
        ("a trailing comma", base[:-1] + b",}", U),
        ("blanks between the tokens", base.replace(b",", b" ,\n\t").replace(b":", b" : ").replace(b"{", b" { ") + b"\r\n", V),
        ("unknown keys", base[:-1] + b',"n":null,"t":true,"f":false,"i":-12,"s":"x"}', V),
        ("true misspelt", base.replace(b"true", b"True"), U),
    ):
        cs.append(Case(f"claims: {what}", want, ck(token(claims=claims))))
    long_jti = "j" * 6200  # header '.' claims beyond PWAF_COOKIE_MAX_SIGNED_BYTES
    assert len(token(jti=long_jti)) - 87 > O.MAX_SIGNED == _abi.COOKIE_MAX_SIGNED_BYTES
    cs.append(Case("a signed part beyond the cap, good signature", U, ck(token(jti=long_jti))))
    cs.append(Case("a signed part beyond the cap, bad signature", I, ck(with_signature(token(jti=long_jti), lambda s: bytes([s[0] ^ 2]) + s[1:]))))
    signed_len = lambda k, j: len(O.b64e(O.header_json(KIDS[k]))) + 1 + len(O.b64e(O.claims_json(cid(), NOW, jti="j" * j)))  # noqa: E731
    k, just = next((k, j) for j in range(5800, 6200) for k in range(3) if signed_len(k, j) == O.MAX_SIGNED)
    cs.append(Case("a signed part of exactly the cap", V, ck(token(k, jti="j" * just))))
    return cs


def sign_raw(header_part, claims_part):
    """a token over the given PARTS (their text as it stands), signed by the first key"""
    msg = header_part + b"." + claims_part
    return msg + b"." + O.b64e(O.sign(SEEDS[0], msg))


@functools.lru_cache(maxsize=None)
def bit_flip_cases():
    good = token()
    return [Case(f"signature bit {bit} flipped", I, NAME + b"=" + with_signature(good, lambda s, bit=bit: s[:bit // 8] + bytes([s[bit // 8] ^ 1 << bit % 8]) + s[bit // 8 + 1:]))
            for bit in range(512)]


def batch_of(cases):
    """-> (RequestBatch, cookies list)"""
    return RequestBatch.from_requests([c.request() for c in cases]), [c.cookie for c in cases]


@functools.lru_cache(maxsize=None)
def keyset():
    return KeySet(KEYS)


@functools.lru_cache(maxsize=None)
def corpus_oracle():
    return [c.oracle() for c in corpus()]


# ---- layout -----------------------------------------------------------------------------------------------------------
def test_key_layout_and_constants_against_c_compiler(tmp_path):
    prog = tmp_path / "sizes.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pwaf.h"\nint main(void){printf("%zu %zu %u %u %u %u %u %u %u %u\\n",sizeof(pwaf_ed25519_key),'
                    "offsetof(pwaf_ed25519_key,x),PWAF_COOKIE_ABSENT,PWAF_COOKIE_VERIFIED,PWAF_COOKIE_INVALID,PWAF_COOKIE_UNDECIDED,PWAF_KEYSET_MAX_KEYS,"
                    "PWAF_KEYSET_MAX_KID,PWAF_COOKIE_MAX_SIGNED_BYTES,PWAF_ABI_VERSION);return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_abi.Ed25519Key), _abi.Ed25519Key.x.offset, _abi.COOKIE_ABSENT, _abi.COOKIE_VERIFIED, _abi.COOKIE_INVALID, _abi.COOKIE_UNDECIDED,
                   _abi.KEYSET_MAX_KEYS, _abi.KEYSET_MAX_KID, _abi.COOKIE_MAX_SIGNED_BYTES, 4]
    assert (A, V, I, U) == (_abi.COOKIE_ABSENT, _abi.COOKIE_VERIFIED, _abi.COOKIE_INVALID, _abi.COOKIE_UNDECIDED)
    assert lib().pwaf_abi_version() == 4


# ---- the corpus -----------------------------------------------------------------------------------------------------------
def test_the_oracle_gives_every_case_the_status_it_is_there_to_show():
    got = corpus_oracle()
    wrong = [(c.label, c.expect, g) for c, g in zip(corpus(), got) if g != c.expect]
    assert not wrong, wrong
    assert {c.expect for c in corpus()} == {A, V, I, U}


def test_one_request_at_a_time_equals_the_oracle_on_every_case():
    ks = keyset()
    wrong = [(c.label, want, got) for c, want in zip(corpus(), corpus_oracle()) if (got := verify_cookie(ks, c.request(), c.cookie, c.now)) != want]
    assert not wrong, wrong
    c = corpus()[0]
    assert RuleEngine.verify_cookie(None, ks, c.request(), c.cookie, c.now) == V  # the method needs nothing of the engine


def test_the_host_mode_equals_the_oracle_on_every_case_as_one_batch():
    cases = corpus()
    assert len({c.now for c in cases}) == 1
    batch, cookies = batch_of(cases)
    got = verify_cookies(keyset(), batch, cookies, NOW)
    wrong = [(c.label, want, int(g)) for c, want, g in zip(cases, corpus_oracle(), got) if g != want]
    assert not wrong, wrong
    assert (RuleEngine.verify_cookies(None, keyset(), batch, cookie_column(cookies), NOW) == got).all()


def test_each_of_the_512_signature_bits_flipped_is_invalid():
    cases = bit_flip_cases()
    batch, cookies = batch_of(cases)
    got = verify_cookies(keyset(), batch, cookies, NOW)
    assert (got == I).all(), np.nonzero(got != I)[0]
    rng = random.Random(512)
    for c in rng.sample(cases, 24) + [cases[0], cases[255], cases[256], cases[511]]:  # the oracle on a sample: every one runs a full verification there
        assert c.oracle() == I, c.label


def test_now_moves_the_time_edges():
    tok = NAME + b"=" + token(exp=NOW + 100, nbf=NOW - 100)
    ks, req = keyset(), corpus()[0].request()
    for now, want in ((NOW + 105, V), (NOW + 106, I), (NOW - 105, V), (NOW - 106, I), (-2**63, I), (2**63 - 1, I)):
        assert verify_cookie(ks, req, tok, now) == want == O.decide(KEYS, tok, now, packed(IP4), UA, HOST), now


# ---- lists, flags ---------------------------------------------------------------------------------------------------------
def raw_call(ks, st, col, idx=None, n_idx=None, idx_cap=None, room=None, status="own", idx_ptr="own", n_ptr="own", flags_out=None, cookies_ptr="own"):
    """pwaf_verify_cookies as it is, into `room` entries pre-filled with 0x5A -> (rc, status array); every argument can be bent"""
    if idx is not None:
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
    idx_cap = (0 if idx is None else len(idx)) if idx_cap is None else idx_cap
    n_ref = None if n_idx is None else np.array([n_idx], dtype=np.uint32)
    room = (idx_cap if idx is not None else (st.n if st is not None else 0)) + 2 if room is None else room
    buf = np.full(room, 0x5A, dtype=np.uint8)
    rc = lib().pwaf_verify_cookies(ks, C.byref(st) if st is not None else None, (C.byref(col) if col is not None else None) if cookies_ptr == "own" else cookies_ptr, NOW,
                                   (None if idx is None else idx.ctypes.data) if idx_ptr == "own" else idx_ptr, idx_cap,
                                   (None if n_ref is None else n_ref.ctypes.data) if n_ptr == "own" else n_ptr, buf.ctypes.data if status == "own" else status,
                                   flags_out, None, 0, None)
    return rc, buf


@functools.lru_cache(maxsize=None)
def small():
    """40 cases of the corpus with every status among them -> (batch, cookie column, statuses, keep-alive)"""
    cases = [c for k, c in enumerate(corpus()) if k % 5 == 0][:40]
    want = [c.oracle() for c in cases]
    assert {A, V, I, U} <= set(want)
    batch, cookies = batch_of(cases)
    data, off = cookie_column(cookies)
    col = _abi.StrCol()
    col.data, col.offsets = data.ctypes.data, off.ctypes.data
    return batch, col, want, (data, off)


def test_lists_with_duplicates_out_of_range_entries_and_the_length_word_against_a_canary():
    batch, col, want, _ = small()
    n, ks, st = batch.n, keyset()._h, batch.as_struct()
    idx = np.array([5, 5, n - 1, n, 0, 0xFFFFFFFF, 7, 5, n + 1, 20], dtype=np.uint32)
    for n_idx in (None, 0, 1, len(idx), len(idx) + 5):
        m = len(idx) if n_idx is None else min(n_idx, len(idx))
        rc, out = raw_call(ks, st, col, idx, n_idx=n_idx, room=len(idx) + 3)
        assert rc == 0
        assert list(out[:m]) == [want[i] if i < n else A for i in idx[:m]], n_idx
        assert (out[m:] == 0x5A).all(), f"n_idx {n_idx}: written at or beyond status + m"
        assert list(verify_cookies(keyset(), batch, (small()[3]), NOW, idx=idx, n_idx=n_idx)) == [want[i] if i < n else A for i in idx[:m]]
    rc, out = raw_call(ks, st, col, room=n + 3)  # idx == NULL: every request, and the canary behind status + n
    assert rc == 0 and list(out[:n]) == want and (out[n:] == 0x5A).all()
    rc, out = raw_call(ks, st, col, idx, idx_cap=0, room=4)  # a list without room for an entry
    assert rc == 0 and (out == 0x5A).all()
    assert len(verify_cookies(keyset(), batch, small()[3], NOW, idx=np.zeros(0, dtype=np.uint32))) == 0
    empty = RequestBatch.from_requests([])
    assert len(verify_cookies(keyset(), empty, [], NOW)) == 0 and list(verify_cookies(keyset(), empty, [], NOW, idx=[0, 1])) == [A, A]


def test_flags_out_sets_the_bit_for_verified_requests_only_and_may_alias_the_flags():
    batch, col, want, column = small()
    n = batch.n
    flags = (np.arange(n) * 37 % 256).astype(np.uint8)  # the bit set and clear on requests of every status, other bits to keep
    expect = np.where(np.array(want) == V, flags | 1, flags & 0xFE).astype(np.uint8)
    own = RequestBatch(batch.data, batch.offsets, batch.ip, batch.ip_is_v6, batch.port, flags.copy())
    out = np.full(n + 2, 0x5A, dtype=np.uint8)
    got = verify_cookies(keyset(), own, column, NOW, flags_out=out[:n])
    assert list(got) == want and (out[:n] == expect).all() and (out[n:] == 0x5A).all() and (own.flags == flags).all()
    got = verify_cookies(keyset(), own, column, NOW, flags_out=own.flags)  # in place
    assert list(got) == want and (own.flags == expect).all()
    st = own.as_struct()
    st.flags = None  # no flags column: the bit alone
    rc, _ = raw_call(keyset()._h, st, col, flags_out=out.ctypes.data)
    assert rc == 0 and (out[:n] == (np.array(want) == V)).all() and (out[n:] == 0x5A).all()
    before = out.copy()
    rc, _ = raw_call(keyset()._h, st, col, idx=[0, 1, 2], flags_out=out.ctypes.data)  # with a list flags_out is not written
    assert rc == 0 and (out == before).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_every_invalid_argument_is_refused_before_anything_is_written():
    batch, col, _, _ = small()
    ks = keyset()._h
    idx = np.arange(10, dtype=np.uint32)
    one = np.array([3], dtype=np.uint32)
    good = batch.as_struct
    UAF, HOSTF = 4, 0

    def bent(**kw):
        st = good()
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def no_column(f, part):
        st = good()
        setattr(st.field[f], part, None)
        return st

    def no_cookies(part):
        c = _abi.StrCol()
        c.data, c.offsets = col.data, col.offsets
        setattr(c, part, None)
        return c

    cases = [
        ("NULL key set", dict(ks=None, st=good(), idx=idx)),
        ("NULL in", dict(st=None, idx=idx)),
        ("NULL cookies", dict(st=good(), idx=idx, cookies_ptr=None)),
        ("NULL status", dict(st=good(), idx=idx, status=None)),
        ("struct_size", dict(st=bent(struct_size=C.sizeof(_abi.Batch) - 8), idx=idx)),
        ("memory", dict(st=bent(memory=2), idx=idx)),
        ("NULL idx with idx_cap != 0", dict(st=good(), idx=idx, idx_ptr=None)),
        ("NULL idx with n_idx", dict(st=good(), idx=None, n_ptr=one.ctypes.data)),
        ("NULL ip", dict(st=bent(ip=None), idx=idx)),
        ("NULL ip_is_v6", dict(st=bent(ip_is_v6=None), idx=idx)),
        ("NULL User-Agent data", dict(st=no_column(UAF, "data"), idx=idx)),
        ("NULL User-Agent offsets", dict(st=no_column(UAF, "offsets"), idx=idx)),
        ("NULL host data", dict(st=no_column(HOSTF, "data"), idx=idx)),
        ("NULL host offsets", dict(st=no_column(HOSTF, "offsets"), idx=idx)),
        ("NULL cookies data", dict(st=good(), idx=idx, col=no_cookies("data"))),
        ("NULL cookies offsets", dict(st=good(), idx=idx, col=no_cookies("offsets"))),
    ]
    for what, kw in cases:
        rc, out = raw_call(kw.pop("ks", ks), kw.pop("st"), kw.pop("col", col), kw.pop("idx"), room=batch.n + 2, **kw)
        assert rc == _abi.E_INVALID_ARG, what
        assert lib().pwaf_last_error(), what
        assert (out == 0x5A).all(), what
    st = batch.as_struct()
    st.memory = _abi.MEM_DEVICE  # a host-only key set has nothing on a device
    rc, out = raw_call(ks, st, col)
    assert rc == _abi.E_DEVICE and (out == 0x5A).all()
    # with n == 0 the columns are not looked at
    st = RequestBatch.from_requests([]).as_struct()
    st.ip = st.ip_is_v6 = None
    st.field[UAF].data = st.field[HOSTF].offsets = None
    rc, out = raw_call(ks, st, no_cookies("data"), [0], room=3)
    assert rc == 0 and out[0] == A and (out[1:] == 0x5A).all()
    # pwaf_verify_cookie_one
    req = _abi.Request()
    status = C.c_uint8(0x5A)
    for args in ((None, C.byref(req), b"a=b", 3, NOW, C.byref(status)), (ks, None, b"a=b", 3, NOW, C.byref(status)), (ks, C.byref(req), b"a=b", 3, NOW, None),
                 (ks, C.byref(req), None, 3, NOW, C.byref(status))):
        assert lib().pwaf_verify_cookie_one(*args) == _abi.E_INVALID_ARG and status.value == 0x5A
    assert lib().pwaf_verify_cookie_one(ks, C.byref(req), None, 0, NOW, C.byref(status)) == 0 and status.value == A


def test_decreasing_offsets_of_a_selected_request_refuse_the_call_with_the_status_untouched():
    batch, col, want, (data, off) = small()
    ks = keyset()._h
    for which in ("cookies", 4, 0):
        st = batch.as_struct()
        c = _abi.StrCol()
        c.data, c.offsets = col.data, col.offsets
        src = off if which == "cookies" else batch.offsets[which]
        o = src.copy()
        o[21] = o[20] - 1  # request 20's value ends before it begins
        if which == "cookies":
            c.offsets = o.ctypes.data
        else:
            st.field[which].offsets = o.ctypes.data
        rc, out = raw_call(ks, st, c, [3, 4, 20, 5])
        assert rc == _abi.E_BATCH and b"entry 2" in lib().pwaf_last_error(), which
        assert (out == 0x5A).all(), "nothing is written for a refused call"
        rc, out = raw_call(ks, st, c)
        assert rc == _abi.E_BATCH and b"entry 20" in lib().pwaf_last_error() and (out == 0x5A).all()
        rc, out = raw_call(ks, st, c, [3, 4, 19, 22])  # requests that are not selected are not looked at
        assert rc == 0 and list(out[:4]) == [want[3], want[4], want[19], want[22]]
    broken = off.copy()
    broken[21] = broken[20] - 1
    with pytest.raises(PwafError):
        verify_cookies(keyset(), batch, (data, broken), NOW)


def test_the_other_columns_of_the_batch_may_be_null():
    batch, col, want, _ = small()
    st = batch.as_struct()
    for f in (1, 2, 3):  # url, path, method
        st.field[f].data = st.field[f].offsets = None
    st.port = st.flags = st.asn = st.country = None
    rc, out = raw_call(keyset()._h, st, col)
    assert rc == 0 and list(out[:batch.n]) == want


# ---- key sets ---------------------------------------------------------------------------------------------------------------
def off_curve_y():
    return next(y for y in range(2, 50) if O.recover_x(y, 0) is None)


def test_key_set_creation_refuses_what_is_not_a_key():
    x = KEYS[0][1]
    refused = [
        ("y = p + 1: not canonical", [("k", (O.P + 1).to_bytes(32, "little"))]),
        ("x = 0 with the sign bit: not canonical", [("k", (1 | 1 << 255).to_bytes(32, "little"))]),
        ("y off the curve", [("k", off_curve_y().to_bytes(32, "little"))]),
        ("y off the curve with the sign bit", [("k", (off_curve_y() | 1 << 255).to_bytes(32, "little"))]),
        ("an empty kid", [("", x)]),
        ("a kid of 65 bytes", [("k" * 65, x)]),
        ("nine keys", [(f"k{i}", x) for i in range(9)]),
        ("no key", []),
        ("one kid twice", [("k", x), ("k", KEYS[1][1])]),
        ("a bad key behind a good one", [("a", x), ("b", (O.P + 1).to_bytes(32, "little"))]),
    ]
    for what, keys in refused:
        with pytest.raises(PwafError) as err:
            KeySet(keys)
        assert err.value.code == _abi.E_INVALID_ARG, what
    with pytest.raises(ValueError):
        KeySet([("k", x[:31])])
    h = C.c_void_p(0x5A)
    assert lib().pwaf_keyset_create(None, 1, -1, C.byref(h)) == _abi.E_INVALID_ARG and not h.value
    arr = (_abi.Ed25519Key * 1)()
    assert lib().pwaf_keyset_create(arr, 1, -1, None) == _abi.E_INVALID_ARG
    assert lib().pwaf_keyset_create(arr, 1, -1, C.byref(h)) == _abi.E_INVALID_ARG  # a NULL kid
    lib().pwaf_keyset_destroy(None)
    # accepted: eight keys, a kid of 64 bytes, the neutral element's and the base point's encodings
    ks = KeySet([(f"k{i}", O.public_key(bytes([i] * 32))) for i in range(7)] + [("k" * 64, x)])
    tok = O.mint(SEEDS[0], O.header_json("k" * 64), O.claims_json(cid(), NOW))
    assert verify_cookie(ks, corpus()[0].request(), NAME + b"=" + tok, NOW) == V
    ks.close()
    ks.close()
    KeySet([("one", (1).to_bytes(32, "little")), ("base", O.encode_point(O.BASE))]).close()


def test_load_captcha_jwks_reads_the_reference_s_file(tmp_path):
    jwk = lambda kid, seed, **kw: {"kid": kid, "use": "sig", "alg": "EdDSA", "kty": "OKP", "crv": "Ed25519", "x": O.b64e(O.public_key(seed)).decode(),  # noqa: E731
                                   "d": O.b64e(seed).decode(), **kw}
    doc = {"keys": [jwk(KIDS[0], SEEDS[0]), jwk(KIDS[1], SEEDS[1])]}
    path = tmp_path / "captcha_jwks.json"
    path.write_text(json.dumps(doc))
    keys = load_captcha_jwks(str(path))
    assert keys == KEYS[:2] == load_captcha_jwks(json.dumps(doc).encode())
    assert all(SEEDS[k] not in repr(keys).encode() and O.b64e(SEEDS[k]).decode() not in repr(keys) for k in range(2)), "d is never kept"
    ks = KeySet(keys)
    assert verify_cookie(ks, corpus()[0].request(), NAME + b"=" + token(1), NOW) == V
    ks.close()

    def refused(keys, needle):
        with pytest.raises(ConfigError) as err:
            load_captcha_jwks(json.dumps({"keys": keys}).encode())
        assert needle in str(err.value), (needle, str(err.value))

    refused([], "captcha JWKS file is empty")
    refused([jwk(" ", SEEDS[0])], "JWK key ID is empty")
    refused([jwk("h", SEEDS[0], alg="HS512", kty="oct", key="AAAA")], "JWT algorithm HS512 not suported for key h. Only EdDSA is currently supported.")
    refused([jwk("e", SEEDS[0], alg="ES256", kty="EC", crv="P-256", y="AAAA")], "JWT algorithm ES256 not suported for key e")
    no_d = jwk("n", SEEDS[0])
    del no_d["d"]
    refused([no_d], "Private key is missing for key n")
    refused([jwk("n", SEEDS[0], d=None)], "Private key is missing for key n")
    refused([jwk("p", SEEDS[0], x=O.b64e(O.public_key(SEEDS[0])).decode() + "=")], "x")
    refused([jwk("s", SEEDS[0], x=O.b64e(b"short").decode())], "32 bytes")
    refused([jwk("c", SEEDS[0], crv="Ed448")], "Ed25519")
    with pytest.raises(ConfigError, match="error parsing captcha JWKS file"):
        load_captcha_jwks(b"{not json")
    with pytest.raises(ConfigError, match="error reading captcha JWKS file"):
        load_captcha_jwks(str(tmp_path / "missing.json"))


# ---- the shared header under the sanitizers -------------------------------------------------------------------------------------
def test_the_shared_header_under_asan_and_ubsan_reads_no_byte_outside_a_value():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "cookie_host")
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                        os.path.join(ROOT, "include"), SRC, "-o", exe], check=True)
    hexed = lambda b: b.hex() or "-"  # noqa: E731
    lines = [f"K {kid.encode().hex()} {x.hex()}" for kid, x in KEYS]
    # key encodings: accepted and refused
    xs = [KEYS[0][1], (O.P + 1).to_bytes(32, "little"), (1 | 1 << 255).to_bytes(32, "little"), off_curve_y().to_bytes(32, "little"), (1).to_bytes(32, "little"),
          O.encode_point(O.BASE), (O.P - 1).to_bytes(32, "little"), bytes([0xFF] * 32)]
    lines += [f"X {x.hex()}" for x in xs]
    # scalars mod L: the edges of every fold, and random ones
    rng = random.Random(252)
    big = [0, 1, O.L - 1, O.L, O.L + 1, 2 * O.L, 2**252 - 1, 2**252, 2**253, 2**256 - 1, 2**256, 2**384 - 1, 2**385, 2**512 - 1, 2**512 - O.L, (2**260 - 1) << 252,
           O.L * (2**259), O.L * (2**259) - 1, 2**511 + 2**32 - 1] + [rng.getrandbits(512) for _ in range(200)] + [rng.getrandbits(k) << s for k, s in ((40, 470), (33, 250), (64, 224))]
    lines += [f"R {x.to_bytes(64, 'little').hex()}" for x in big]
    cases = corpus() + bit_flip_cases()[::37]
    lines.append(f"N {NOW}")
    for c in cases:
        ip = packed(c.ip)
        lines.append(f"Q {int(len(ip) == 16)} {ip.ljust(16, ZERO).hex()} {hexed(c.ua)} {hexed(c.host)} {'~' if c.cookie is None else hexed(c.cookie)}")
    lines.append(f"N {NOW + 86400 + 6}")  # a second batch at a later `now`: the valid token has expired
    c = corpus()[0]
    lines.append(f"Q 0 {packed(c.ip).ljust(16, ZERO).hex()} {hexed(c.ua)} {hexed(c.host)} {hexed(c.cookie)}")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    out = r.stdout.split("\n")
    assert [ln for ln in out if ln.startswith("X")] == [f"X {int(O.decode_point(x) is not None)}" for x in xs]
    assert [ln for ln in out if ln.startswith("X")][:4] == ["X 1", "X 0", "X 0", "X 0"]
    assert [ln for ln in out if ln.startswith("R")] == [f"R {(x % O.L).to_bytes(32, 'little').hex()}" for x in big]
    want = corpus_oracle() + [I] * len(bit_flip_cases()[::37]) + [I]
    assert [int(ln.split()[1]) for ln in out if ln.startswith("Q")] == want
