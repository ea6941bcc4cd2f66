"""pwaf_verify_pow in HOST mode and pwaf_verify_pow_one (no GPU, no HIP call): the check CaptchaManager::api_verify runs on a
proof-of-work submission (captcha.rs:241-333; jwt.rs:198-327) against the independent oracle of tests/pow_oracle.py, status for status,
over a corpus of labelled cases — the valid submission, every single-claim defect, the time edges, the client id with and without its NUL,
the difficulty's range and the leading zero nibbles around it, each of the 256 bits of the hash, every SHA-256 padding edge of the
message, the one escape and every other backslash form, the cookie-header edges, the signature edges behind an otherwise passing
submission, the subset's and the cap's edges — then list shapes against a canary, every refusal, a regression guard on
pwaf_verify_cookies, and csrc/pow.h alone under AddressSanitizer + UBSan as a stand-alone program (tests/pow_host.cpp) over exact-size heap
blocks. Each corpus case also carries the status it is there to show, so the oracle itself is pinned."""
import ctypes as C
import functools
import hashlib
import ipaddress
import os
import subprocess

import numpy as np
import pytest

import cookie_oracle as CO
import pow_oracle as O
from pingoo_amd import KeySet, Request, RequestBatch, _abi, verify_cookies, verify_pow, verify_pow_one
from pingoo_amd.engine import PwafError, RuleEngine, cookie_column, lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "pow_host.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "pingoo_amd", "csrc", h) for h in ("pow.h", "cookie.h", "clientid.h")] + [os.path.join(ROOT, "pingoo_amd", "csrc", "service.h"), os.path.join(ROOT, "include", "pwaf.h")]
A, P, F, U = O.ABSENT, O.PASSED, O.FAILED, O.UNDECIDED
NOW = 1_800_000_000
NAME = b"__pingoo_captcha"
VERIFIED_NAME = b"__pingoo_captcha_verified"
ZERO = b"\0"
NUL = O.NUL

SEEDS = [bytes([11 * k + 3] * 32) for k in range(3)]
KIDS = ["k1", "captcha-2", "0190b5a2-7c1e-7d43-9f6a-3b2c1d0e4f-k3"]  # 2, 9 and 37 bytes
KEYS = [(kid, CO.public_key(seed)) for kid, seed in zip(KIDS, SEEDS)]
OTHER_SEED = bytes([0xC3] * 32)  # a key that is not in the set

IP4, IP6, UA, HOST = "203.0.113.7", "2001:db8:0:7::9", b"Mozilla/5.0 (X11; Linux x86_64) Gecko/20100101 Firefox/128.0", b"shop.example.com"
CHALLENGE = O.heapless44(hashlib.sha256(b"a challenge").digest())  # genuine-shaped: 43 characters and the NUL


def packed(ip):
    return ipaddress.ip_address(ip).packed


def sub_of(ip=IP4, ua=UA, host=HOST):
    return O.client_sub(packed(ip), ua, host)


def raw(challenge):
    return challenge.encode("latin-1")


@functools.lru_cache(maxsize=None)
def work(challenge=CHALLENGE, zeros=3, exactly=False, start=0):
    """(nonce, digest) with `zeros` leading zero nibbles (at least, or exactly)"""
    return O.search_nonce(raw(challenge), zeros, exactly=exactly, start=start)


def token(key=0, header=None, claims=None, seed=None, challenge=CHALLENGE, difficulty=1, **change):
    """a challenge token of client (IP4, UA, HOST) under key `key`; header / claims: the JSON text instead of the reference's"""
    header = O.header_json(KIDS[key]) if header is None else header
    claims = O.claims_json(change.pop("sub", sub_of()), NOW, challenge, difficulty, **change) if claims is None else claims
    return O.mint(SEEDS[key] if seed is None else seed, header, claims)


def with_signature(tok, fn):
    h, c, s = tok.split(b".")
    return h + b"." + c + b"." + O.b64e(fn(O.b64d(s)))


def flip(b, bit):
    return b[:bit // 8] + bytes([b[bit // 8] ^ 1 << bit % 8]) + b[bit // 8 + 1:]


class Case:
    def __init__(self, label, expect, cookie, digest=None, nonce=None, ip=IP4, ua=UA, host=HOST, now=NOW):
        if digest is None:
            nonce, digest = work()
        self.label, self.expect, self.cookie, self.digest, self.nonce, self.ip, self.ua, self.host, self.now = label, expect, cookie, digest, nonce, ip, ua, host, now

    def oracle(self):
        return O.decide(KEYS, self.cookie, self.digest, self.nonce, self.now, packed(self.ip), self.ua, self.host)

    def request(self):
        return Request(host=self.host, url=b"/__pingoo/captcha/api/verify", path=b"/__pingoo/captcha/api/verify", method=b"POST", user_agent=self.ua, ip=self.ip)


def signed_len(key, jti_len):
    return len(O.b64e(O.header_json(KIDS[key]))) + 1 + len(O.b64e(O.claims_json(sub_of(), NOW, CHALLENGE, 1, jti="j" * jti_len)))


@functools.lru_cache(maxsize=None)
def corpus():
    """every labelled case but the bit flips (hash_flip_cases, signature_flip_cases) -> [Case]"""
    ck = lambda t: NAME + b"=" + t  # noqa: E731
    good = token()
    cs = [Case("the valid submission", P, ck(good)), Case("the valid submission, IPv6 client", P, ck(token(sub=sub_of(IP6))), ip=IP6)]
    assert b"\\u0000" in O.claims_json(sub_of(), NOW, CHALLENGE, 1) and len(CHALLENGE) == 44, "genuine-shaped: 43 characters and \\u0000"
    # single-claim defects
    for name in ("challenge", "difficulty", "iss", "sub", "aud", "exp", "nbf"):
        cs.append(Case(f"claim {name} missing", F, ck(token(**{name: O.DROP}))))
        cs.append(Case(f"claim {name} null", F, ck(token(**{name: None}))))
    for name in ("iat", "jti"):
        cs.append(Case(f"optional claim {name} missing", P, ck(token(**{name: O.DROP}))))
        cs.append(Case(f"optional claim {name} null", P, ck(token(**{name: None}))))
    for name, wrong in (("challenge", 5), ("challenge", True), ("iss", 5), ("sub", 5), ("aud", 5), ("exp", str(NOW + 9)), ("nbf", str(NOW)), ("exp", True), ("difficulty", True)):
        cs.append(Case(f"claim {name} of the wrong type ({wrong!r})", F, ck(token(**{name: wrong}))))
    for name, wrong in (("aud", "pingo"), ("aud", "pingoo" + NUL), ("iss", "Pingoo"), ("iss", "")):
        cs.append(Case(f"claim {name} with the wrong value ({wrong!r})", F, ck(token(**{name: wrong}))))
    cs.append(Case("iat of the wrong type, good signature", U, ck(token(iat="x"))))
    cs.append(Case("jti of the wrong type, good signature", U, ck(token(jti=7))))
    cs.append(Case("jti of the wrong type, bad signature", F, ck(with_signature(token(jti=7), lambda s: flip(s, 9)))))
    cs.append(Case("an escape in jti", P, ck(token(jti="a" + NUL + "b"))))
    # the time edges: exp >= now - 5, nbf <= now + 5
    for d, want in ((-6, F), (-5, P), (-4, P)):
        cs.append(Case(f"exp = now{d:+d}", want, ck(token(exp=NOW + d))))
    for d, want in ((4, P), (5, P), (6, F)):
        cs.append(Case(f"nbf = now{d:+d}", want, ck(token(nbf=NOW + d))))
    # the client id: 43 characters AND the NUL
    for what, kw in (("ip", dict(ip="203.0.113.8")), ("User-Agent", dict(ua=UA + b"x")), ("host", dict(host=b"shop.example.org")), ("address family", dict(ip=IP6))):
        cs.append(Case(f"sub of another {what}", F, ck(good), **kw))
    plain = sub_of()[:43]
    for what, sub in (("the 43 characters without the NUL", plain), ("44 characters, no NUL", plain + "A"), ("two NULs", plain + NUL + NUL), ("the NUL first", NUL + plain),
                      ("42 characters and the NUL", plain[:42] + NUL), ("the last character changed", plain[:42] + ("A" if plain[42] != "A" else "B") + NUL), ("empty", "")):
        cs.append(Case(f"sub: {what}", F, ck(token(sub=sub))))
    # the difficulty (a u8) against a hash with three leading zero nibbles
    nonce3, digest3 = work(zeros=3, exactly=True)
    for d, want in ((0, P), (1, P), (2, P), (3, P), (4, F), (64, F), (65, F), (255, F), (256, F), (-1, F), ("1", F), (2**63 - 1, F), (-2**63, F)):
        cs.append(Case(f"difficulty {d!r}, three zero nibbles", want, ck(token(difficulty=d)), digest3, nonce3))
    claims_f = O.claims_json(sub_of(), NOW, CHALLENGE, 1).replace(b'"difficulty":1,', b'"difficulty":1.0,')
    cs.append(Case("difficulty 1.0 (outside the subset), good signature", U, ck(token(claims=claims_f)), digest3, nonce3))
    cs.append(Case("difficulty 1.0 (outside the subset), bad signature", F, ck(with_signature(token(claims=claims_f), lambda s: flip(s, 300))), digest3, nonce3))
    cs.append(Case("difficulty 64 and a hash of 32 zero bytes", F, ck(token(difficulty=64)), bytes(32), nonce3))
    cs.append(Case("difficulty 65 and a hash of 32 zero bytes", F, ck(token(difficulty=65)), bytes(32), nonce3))
    for d in (1, 2, 3):
        for z in (d - 1, d, d + 1):
            nonce, digest = work(zeros=z, exactly=True)
            assert O.zero_nibbles(digest) == z
            cs.append(Case(f"difficulty {d}, exactly {z} leading zero nibbles", P if z >= d else F, ck(token(difficulty=d)), digest, nonce))
    other_nonce, other_digest = work(zeros=3, exactly=False, start=int(nonce3) + 1)
    assert other_nonce != nonce3
    cs.append(Case("a wrong answer that still has the required zeros (another nonce's hash)", F, ck(token(difficulty=3)), other_digest, nonce3))
    cs.append(Case("a wrong answer that still has the required zeros (another nonce)", F, ck(token(difficulty=3)), digest3, other_nonce))
    cs.append(Case("the nonce with a byte appended", F, ck(good), digest3, nonce3 + b"0"))
    cs.append(Case("the nonce one byte short", F, ck(good), digest3, nonce3[:-1]))
    # the SHA-256 padding edges of the message challenge || nonce
    for total in (0, 55, 56, 63, 64, 65, 119, 120):
        for what, challenge in (("plain", "C" * (total // 2)), ("with the escape", ("C" * (total // 2 - 1) + NUL) if total else "")):
            nonce = b"7" * (total - len(challenge))
            digest = hashlib.sha256(raw(challenge) + nonce).digest()
            cs.append(Case(f"a message of {total} bytes, challenge {what}", P, ck(token(challenge=challenge, difficulty=0)), digest, nonce))
            if total:
                cs.append(Case(f"a message of {total} bytes, challenge {what}, last nonce byte changed", F, ck(token(challenge=challenge, difficulty=0)), digest, nonce[:-1] + b"8"))
    for what, challenge, nonce in (("an empty nonce", CHALLENGE, b""), ("an empty challenge", "", b"12345"), ("a nonce of 200 bytes", CHALLENGE, b"n" * 200),
                                   ("a challenge of 300 bytes", "c" * 299 + NUL, b"1")):
        cs.append(Case(what, P, ck(token(challenge=challenge, difficulty=0)), hashlib.sha256(raw(challenge) + nonce).digest(), nonce))
    # the escape: first, in the middle, twice, adjacent, none
    for what, challenge in (("first", NUL + "abcdef"), ("in the middle", "abc" + NUL + "def"), ("twice", "ab" + NUL + "cd" + NUL), ("twice in a row", "ab" + NUL + NUL + "cd"), ("none", "abcdef"),
                            ("alone", NUL), ("the text u0000 without a backslash", "au0000")):
        nonce = b"42"
        cs.append(Case(f"challenge with the escape {what}", P, ck(token(challenge=challenge, difficulty=0)), hashlib.sha256(raw(challenge) + nonce).digest(), nonce))
    cs.append(Case("the decoded challenge differs from the text as it stands", F, ck(token(challenge="ab" + NUL, difficulty=0)), hashlib.sha256(b"ab\\u0000" + b"42").digest(), b"42"))
    # every other backslash form: outside the subset
    base = O.claims_json(sub_of(), NOW, "abcXdef", 0)
    nonce_x = b"42"
    for what, text in (("\\u0001", b"\\u0001"), ("\\n", b"\\n"), ("a truncated \\u000", b"\\u000"), ("\\U0000", b"\\U0000"), ("\\\\", b"\\\\"), ('\\"', b'\\"'), ("\\u00000 cut to \\u000g", b"\\u000g"),
                       ("\\u0020", b"\\u0020"), ("\\/", b"\\/")):
        claims = base.replace(b"abcXdef", b"abc" + text + b"def")
        digest = hashlib.sha256(b"abc\0def" + nonce_x).digest()
        cs.append(Case(f"claims: {what} in the challenge, good signature", U, ck(token(claims=claims)), digest, nonce_x))
        cs.append(Case(f"claims: {what} in the challenge, bad signature", F, ck(with_signature(token(claims=claims), lambda s: flip(s, 77))), digest, nonce_x))
    at_end = base.replace(b'"abcXdef"', b'"abc\\u000"')
    cs.append(Case("claims: a truncated escape at the end of the string, good signature", U, ck(token(claims=at_end)), hashlib.sha256(b"abc" + nonce_x).digest(), nonce_x))
    in_name = base.replace(b'"challenge"', b'"chal\\u0000lenge"')
    cs.append(Case("claims: the escape in a name, good signature", U, ck(token(claims=in_name)), hashlib.sha256(b"abcXdef" + nonce_x).digest(), nonce_x))
    dup = base[:-1] + b',"difficulty":0}'
    cs.append(Case("claims: a known name twice, good signature", U, ck(token(claims=dup)), hashlib.sha256(b"abcXdef" + nonce_x).digest(), nonce_x))
    cs.append(Case("claims: a known name twice, bad signature", F, ck(with_signature(token(claims=dup), lambda s: flip(s, 1))), hashlib.sha256(b"abcXdef" + nonce_x).digest(), nonce_x))
    cs.append(Case("claims: a nested object, good signature", U, ck(token(claims=base[:-1] + b',"ctx":{"a":1}}')), hashlib.sha256(b"abcXdef" + nonce_x).digest(), nonce_x))
    cs.append(Case("claims: blanks between the tokens and unknown names", P, ck(token(claims=base.replace(b",", b" ,\n\t").replace(b'":', b'" : ')[:-1] + b',"n":null,"t":true,"i":-12 } ')),
                   hashlib.sha256(b"abcXdef" + nonce_x).digest(), nonce_x))
    cs.append(Case("claims: not base64, signed", U, ck(sign_raw(O.b64e(O.header_json(KIDS[0])), b"%%%"))))
    # the cookie header
    verified = VERIFIED_NAME + b"=" + CO.mint(SEEDS[0], CO.header_json(KIDS[0]), CO.claims_json(sub_of()[:43], NOW))
    cs.append(Case("no Cookie header", A, None))
    cs.append(Case("an empty Cookie header", A, b""))
    cs.append(Case("other cookies only", A, b"session=abc; theme=dark"))
    cs.append(Case("both captcha cookies, the verified one first", P, verified + b"; " + ck(good)))
    cs.append(Case("both captcha cookies, the verified one last", P, ck(good) + b"; " + verified))
    cs.append(Case("the verified cookie alone", A, verified))
    cs.append(Case("the verified cookie's name with the challenge token", A, VERIFIED_NAME + b"=" + good))
    cs.append(Case("the name in another case", A, b"__Pingoo_captcha=" + good))
    cs.append(Case("a name that ends with the real one", A, b"x" + ck(good)))
    cs.append(Case("a quoted value", P, NAME + b'="' + good + b'"'))
    cs.append(Case("a value with only an opening quote", F, NAME + b'="' + good))
    cs.append(Case("blanks and tabs around name and value", P, b"a=b;\t " + NAME + b" \t=\t  " + good + b" \t ; c=d"))
    cs.append(Case("the same name twice, the first valid", P, ck(good) + b"; " + ck(b"junk")))
    cs.append(Case("the same name twice, the first invalid", F, ck(b"junk") + b"; " + ck(good)))
    cs.append(Case("a byte 0x80 in the value (D-C1)", A, ck(good) + b"; a=\x80"))
    cs.append(Case("a NUL in the value (D-C1)", A, ck(good) + b"\0"))
    cs.append(Case("two parts", F, ck(good.rsplit(b".", 1)[0])))
    cs.append(Case("a signature part of 85 characters", F, ck(good[:-1])))
    cs.append(Case("an empty value", F, NAME + b"="))
    # the signature, behind a submission that passes every cheap check
    cs.append(Case("S + L", F, ck(with_signature(good, lambda s: s[:32] + (int.from_bytes(s[32:], "little") + CO.L).to_bytes(32, "little")))))
    cs.append(Case("a kid outside the set", F, ck(token(header=O.header_json("nobody")))))
    cs.append(Case("a token signed by a key outside the set", F, ck(token(seed=OTHER_SEED))))
    cs.append(Case("the second key's kid, the first key's signature", F, ck(token(0, header=O.header_json(KIDS[1])))))
    cs.append(Case("the token under the second key", P, ck(token(1))))
    cs.append(Case("the token under the third key", P, ck(token(2))))
    cs.append(Case("alg ES256", F, ck(token(header=O.header_json(KIDS[0], alg="ES256")))))
    cs.append(Case("typ JWS", F, ck(token(header=O.header_json(KIDS[0], typ="JWS")))))
    # the header outside the subset; the cap
    nested = b'{"typ":"JWT","alg":"EdDSA","kid":"k1","jwk":{"kty":"OKP"}}'
    cs.append(Case("a header outside the subset, good signature", U, ck(token(header=nested))))
    cs.append(Case("a header outside the subset, good signature of the third key", U, ck(token(2, header=nested))))
    cs.append(Case("a header outside the subset, bad signature", F, ck(with_signature(token(header=nested), lambda s: flip(s, 40)))))
    cs.append(Case("a header outside the subset, a key outside the set", F, ck(token(header=nested, seed=OTHER_SEED))))
    cs.append(Case("a header with the escape, good signature", U, ck(token(header=b'{"typ":"JWT","alg":"EdDSA","kid":"k1","cty":"a\\u0000"}'))))
    cs.append(Case("a header outside the subset over a wrong hash: still the signature's answer", U, ck(token(header=nested)), flip(work()[1], 255), work()[0]))
    for want_len, want in ((O.MAX_SIGNED, P), (O.MAX_SIGNED + 1, U)):
        key, jti_len = next((k, j) for j in range(5700, 6300) for k in range(3) if signed_len(k, j) == want_len)
        tok = token(key, jti="j" * jti_len)
        assert len(tok) - 87 == want_len
        cs.append(Case(f"a signed part of {want_len} characters", want, ck(tok)))
        if want == U:
            cs.append(Case(f"a signed part of {want_len} characters, bad signature", F, ck(with_signature(tok, lambda s: flip(s, 3)))))
    return cs


def sign_raw(header_part, claims_part):
    """a token over the given PARTS (their text as it stands), signed by the first key"""
    msg = header_part + b"." + claims_part
    return msg + b"." + O.b64e(O.sign(SEEDS[0], msg))


@functools.lru_cache(maxsize=None)
def hash_flip_cases():
    nonce, digest = work()
    cookie = NAME + b"=" + token()
    return [Case(f"hash bit {bit} flipped", F, cookie, flip(digest, bit), nonce) for bit in range(256)]


@functools.lru_cache(maxsize=None)
def signature_flip_cases():
    good = token()
    return [Case(f"signature bit {bit} flipped", F, NAME + b"=" + with_signature(good, lambda s, bit=bit: flip(s, bit))) for bit in range(0, 512, 8)]


def batch_of(cases):
    """-> (RequestBatch, cookies list, (n, 32) hashes, nonces list)"""
    hashes = np.frombuffer(b"".join(c.digest for c in cases), dtype=np.uint8).reshape(-1, 32).copy() if cases else np.zeros((0, 32), dtype=np.uint8)
    return RequestBatch.from_requests([c.request() for c in cases]), [c.cookie for c in cases], hashes, [c.nonce for c in cases]


@functools.lru_cache(maxsize=None)
def keyset():
    return KeySet(KEYS)


@functools.lru_cache(maxsize=None)
def corpus_oracle():
    """[(status, handed to the signature stage)]"""
    return [c.oracle() for c in corpus()]


def corpus_status():
    return [s for s, _ in corpus_oracle()]


# ---- layout -----------------------------------------------------------------------------------------------------------
def test_constants_against_c_compiler(tmp_path):
    prog = tmp_path / "pow.c"
    prog.write_text('#include <stdio.h>\n#include "pwaf.h"\nint main(void){printf("%u %u %u %u %u\\n",PWAF_POW_ABSENT,PWAF_POW_PASSED,PWAF_POW_FAILED,PWAF_POW_UNDECIDED,'
                    "PWAF_ABI_VERSION);return 0;}\n")
    exe = tmp_path / "pow"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [_abi.POW_ABSENT, _abi.POW_PASSED, _abi.POW_FAILED, _abi.POW_UNDECIDED, 4] == [A, P, F, U, 4]
    assert lib().pwaf_abi_version() == 4
    assert lib().pwaf_verify_pow_scratch_bytes(0) == 16 and lib().pwaf_verify_pow_scratch_bytes(10) == 16 + 24 * 10


# ---- the corpus -----------------------------------------------------------------------------------------------------------
def test_the_oracle_gives_every_case_the_status_it_is_there_to_show():
    wrong = [(c.label, c.expect, g) for c, g in zip(corpus(), corpus_status()) if g != c.expect]
    assert not wrong, wrong
    assert {c.expect for c in corpus()} == {A, P, F, U}
    # the signature stage is asked exactly for PASSED, UNDECIDED and the failures that only a signature decides
    assert all(h for (s, h) in corpus_oracle() if s in (P, U)) and not any(h for (s, h), c in zip(corpus_oracle(), corpus()) if c.label.startswith("difficulty 4,"))


def test_one_request_at_a_time_equals_the_oracle_on_every_case():
    ks = keyset()
    wrong = [(c.label, want, got) for c, want in zip(corpus(), corpus_status()) if (got := verify_pow_one(ks, c.request(), c.cookie, c.digest, c.nonce, c.now)) != want]
    assert not wrong, wrong
    c = corpus()[0]
    assert RuleEngine.verify_pow_one(None, ks, c.request(), c.cookie, c.digest, c.nonce, c.now) == P  # the method needs nothing of the engine
    assert verify_pow_one(ks, c.request(), c.cookie.decode(), c.digest, c.nonce.decode(), c.now) == P
    with pytest.raises(ValueError):
        verify_pow_one(ks, c.request(), c.cookie, c.digest[:31], c.nonce, c.now)


def test_the_host_mode_equals_the_oracle_on_every_case_as_one_batch():
    cases = corpus()
    assert len({c.now for c in cases}) == 1
    batch, cookies, hashes, nonces = batch_of(cases)
    got = verify_pow(keyset(), batch, cookies, hashes, nonces, NOW)
    wrong = [(c.label, want, int(g)) for c, want, g in zip(cases, corpus_status(), got) if g != want]
    assert not wrong, wrong
    again = RuleEngine.verify_pow(None, keyset(), batch, cookie_column(cookies), [c.digest for c in cases], cookie_column(nonces), NOW)
    assert (again == got).all()


def test_each_of_the_256_hash_bits_flipped_fails_without_the_signature_stage():
    cases = hash_flip_cases()
    batch, cookies, hashes, nonces = batch_of(cases)
    got = verify_pow(keyset(), batch, cookies, hashes, nonces, NOW)
    assert (got == F).all(), np.nonzero(got != F)[0]
    assert all(c.oracle() == (F, False) for c in cases)


def test_every_eighth_signature_bit_flipped_on_a_passing_submission_fails():
    cases = signature_flip_cases()
    batch, cookies, hashes, nonces = batch_of(cases)
    got = verify_pow(keyset(), batch, cookies, hashes, nonces, NOW)
    assert (got == F).all(), np.nonzero(got != F)[0]
    for c in cases[::9] + [cases[-1]]:  # the oracle on a sample: every one runs a full verification there
        assert c.oracle() == (F, True), c.label


def test_now_moves_the_time_edges():
    tok = NAME + b"=" + token(exp=NOW + 100, nbf=NOW - 100)
    ks, req = keyset(), corpus()[0].request()
    nonce, digest = work()
    for now, want in ((NOW + 105, P), (NOW + 106, F), (NOW - 105, P), (NOW - 106, F), (-2**63, F), (2**63 - 1, F)):
        assert verify_pow_one(ks, req, tok, digest, nonce, now) == want == O.decide(KEYS, tok, digest, nonce, now, packed(IP4), UA, HOST)[0], now


# ---- lists ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small():
    """40 cases of the corpus with every status among them -> (batch, cookie column struct, nonce column struct, hashes, statuses, keep-alive)"""
    cases = [c for k, c in enumerate(corpus()) if k % 5 == 0][:40]
    want = [c.oracle()[0] for c in cases]
    assert {A, P, F, U} <= set(want)
    batch, cookies, hashes, nonces = batch_of(cases)
    columns = cookie_column(cookies), cookie_column(nonces)
    col, ncol = _abi.StrCol(), _abi.StrCol()
    col.data, col.offsets = columns[0][0].ctypes.data, columns[0][1].ctypes.data
    ncol.data, ncol.offsets = columns[1][0].ctypes.data, columns[1][1].ctypes.data
    return batch, col, ncol, hashes, want, columns


def raw_call(ks, st, col, ncol, hashes, idx=None, n_idx=None, idx_cap=None, room=None, status="own", idx_ptr="own", n_ptr="own", cookies_ptr="own", nonce_ptr="own", hash_ptr="own"):
    """pwaf_verify_pow as it is, into `room` entries pre-filled with 0x5A -> (rc, status array); every argument can be bent"""
    if idx is not None:
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
    idx_cap = (0 if idx is None else len(idx)) if idx_cap is None else idx_cap
    n_ref = None if n_idx is None else np.array([n_idx], dtype=np.uint32)
    room = (idx_cap if idx is not None else (st.n if st is not None else 0)) + 2 if room is None else room
    buf = np.full(room, 0x5A, dtype=np.uint8)
    by_ref = lambda c: None if c is None else C.byref(c)  # noqa: E731
    rc = lib().pwaf_verify_pow(ks, by_ref(st), by_ref(col) if cookies_ptr == "own" else cookies_ptr, hashes.ctypes.data if hash_ptr == "own" else hash_ptr,
                               by_ref(ncol) if nonce_ptr == "own" else nonce_ptr, NOW, (None if idx is None else idx.ctypes.data) if idx_ptr == "own" else idx_ptr, idx_cap,
                               (None if n_ref is None else n_ref.ctypes.data) if n_ptr == "own" else n_ptr, buf.ctypes.data if status == "own" else status, None, 0, None)
    return rc, buf


def test_lists_with_duplicates_out_of_range_entries_and_the_length_word_against_a_canary():
    batch, col, ncol, hashes, want, columns = small()
    n, ks, st = batch.n, keyset()._h, batch.as_struct()
    idx = np.array([5, 5, n - 1, n, 0, 0xFFFFFFFF, 7, 5, n + 1, 20], dtype=np.uint32)
    for n_idx in (None, 0, 1, len(idx) - 1, len(idx), len(idx) + 5):
        m = len(idx) if n_idx is None else min(n_idx, len(idx))
        rc, out = raw_call(ks, st, col, ncol, hashes, idx, n_idx=n_idx, room=len(idx) + 3)
        assert rc == 0
        assert list(out[:m]) == [want[i] if i < n else A for i in idx[:m]], n_idx
        assert (out[m:] == 0x5A).all(), f"n_idx {n_idx}: written at or beyond status + m"
        assert list(verify_pow(keyset(), batch, columns[0], hashes, columns[1], NOW, idx=idx, n_idx=n_idx)) == [want[i] if i < n else A for i in idx[:m]]
    rc, out = raw_call(ks, st, col, ncol, hashes, room=n + 3)  # idx == NULL: every request, and the canary behind status + n
    assert rc == 0 and list(out[:n]) == want and (out[n:] == 0x5A).all()
    rc, out = raw_call(ks, st, col, ncol, hashes, idx, idx_cap=0, room=4)  # a list without room for an entry
    assert rc == 0 and (out == 0x5A).all()
    assert len(verify_pow(keyset(), batch, columns[0], hashes, columns[1], NOW, idx=np.zeros(0, dtype=np.uint32))) == 0
    empty = RequestBatch.from_requests([])
    assert len(verify_pow(keyset(), empty, [], [], [], NOW)) == 0 and list(verify_pow(keyset(), empty, [], [], [], NOW, idx=[0, 1])) == [A, A]


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_every_invalid_argument_is_refused_before_anything_is_written():
    batch, col, ncol, hashes, _, _ = small()
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

    def without(c, part):
        d = _abi.StrCol()
        d.data, d.offsets = c.data, c.offsets
        setattr(d, part, None)
        return d

    cases = [
        ("NULL key set", dict(ks=None, st=good(), idx=idx)),
        ("NULL in", dict(st=None, idx=idx)),
        ("NULL cookies", dict(st=good(), idx=idx, cookies_ptr=None)),
        ("NULL status", dict(st=good(), idx=idx, status=None)),
        ("NULL hash", dict(st=good(), idx=idx, hash_ptr=None)),
        ("NULL nonce", dict(st=good(), idx=idx, nonce_ptr=None)),
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
        ("NULL cookies data", dict(st=good(), idx=idx, col=without(col, "data"))),
        ("NULL cookies offsets", dict(st=good(), idx=idx, col=without(col, "offsets"))),
        ("NULL nonce data", dict(st=good(), idx=idx, ncol=without(ncol, "data"))),
        ("NULL nonce offsets", dict(st=good(), idx=idx, ncol=without(ncol, "offsets"))),
    ]
    for what, kw in cases:
        rc, out = raw_call(kw.pop("ks", ks), kw.pop("st"), kw.pop("col", col), kw.pop("ncol", ncol), hashes, kw.pop("idx"), room=batch.n + 2, **kw)
        assert rc == _abi.E_INVALID_ARG, what
        assert lib().pwaf_last_error(), what
        assert (out == 0x5A).all(), what
    st = batch.as_struct()
    st.memory = _abi.MEM_DEVICE  # a host-only key set has nothing on a device
    rc, out = raw_call(ks, st, col, ncol, hashes)
    assert rc == _abi.E_DEVICE and (out == 0x5A).all()
    # with n == 0 the columns are not looked at (the nonce column's members neither), but hash and nonce themselves are
    st = RequestBatch.from_requests([]).as_struct()
    st.ip = st.ip_is_v6 = None
    st.field[UAF].data = st.field[HOSTF].offsets = None
    rc, out = raw_call(ks, st, without(col, "data"), without(ncol, "offsets"), hashes, [0], room=3)
    assert rc == 0 and out[0] == A and (out[1:] == 0x5A).all()
    rc, out = raw_call(ks, st, col, ncol, hashes, [0], room=3, hash_ptr=None)
    assert rc == _abi.E_INVALID_ARG and (out == 0x5A).all()
    # pwaf_verify_pow_one
    req = _abi.Request()
    status = C.c_uint8(0x5A)
    h = bytes(32)
    for args in ((None, C.byref(req), b"a=b", 3, h, b"1", 1, NOW, C.byref(status)), (ks, None, b"a=b", 3, h, b"1", 1, NOW, C.byref(status)),
                 (ks, C.byref(req), b"a=b", 3, h, b"1", 1, NOW, None), (ks, C.byref(req), None, 3, h, b"1", 1, NOW, C.byref(status)),
                 (ks, C.byref(req), b"a=b", 3, None, b"1", 1, NOW, C.byref(status)), (ks, C.byref(req), b"a=b", 3, h, None, 1, NOW, C.byref(status))):
        assert lib().pwaf_verify_pow_one(*args) == _abi.E_INVALID_ARG and status.value == 0x5A
    assert lib().pwaf_verify_pow_one(ks, C.byref(req), None, 0, h, None, 0, NOW, C.byref(status)) == 0 and status.value == A


def test_decreasing_offsets_of_a_selected_request_refuse_the_call_with_the_status_untouched():
    batch, col, ncol, hashes, want, columns = small()
    ks = keyset()._h
    for which in ("cookies", "nonce", 4, 0):
        st = batch.as_struct()
        c, nc = _abi.StrCol(), _abi.StrCol()
        c.data, c.offsets, nc.data, nc.offsets = col.data, col.offsets, ncol.data, ncol.offsets
        src = columns[0][1] if which == "cookies" else columns[1][1] if which == "nonce" else batch.offsets[which]
        o = src.copy()
        o[21] = o[20] - 1  # request 20's value ends before it begins
        if which == "cookies":
            c.offsets = o.ctypes.data
        elif which == "nonce":
            nc.offsets = o.ctypes.data
        else:
            st.field[which].offsets = o.ctypes.data
        rc, out = raw_call(ks, st, c, nc, hashes, [3, 4, 20, 5])
        assert rc == _abi.E_BATCH and b"entry 2" in lib().pwaf_last_error(), which
        assert (out == 0x5A).all(), "nothing is written for a refused call"
        rc, out = raw_call(ks, st, c, nc, hashes)
        assert rc == _abi.E_BATCH and b"entry 20" in lib().pwaf_last_error() and (out == 0x5A).all()
        rc, out = raw_call(ks, st, c, nc, hashes, [3, 4, 19, 22])  # requests that are not selected are not looked at
        assert rc == 0 and list(out[:4]) == [want[3], want[4], want[19], want[22]]
    broken = columns[1][1].copy()
    broken[21] = broken[20] - 1
    with pytest.raises(PwafError):
        verify_pow(keyset(), batch, columns[0], hashes, (columns[1][0], broken), NOW)


# ---- pwaf_verify_cookies answers what it answered before ----------------------------------------------------------------------
def test_verify_cookies_still_answers_its_own_cases_as_before():
    """the name parameter of the cookie scan and the escape-aware reader leave gate C alone: 43 bytes of sub, no escape, its own cookie"""
    import test_verify_cookies_cpu as T

    labels = ["the valid token", "the valid token, IPv6 client", "claim sub missing", "exp = now-6", "claims: an escape in a string", "claims: an escaped quote in a string",
              "a header outside the subset, good signature", "the name in another case", "a name that begins with the real one", "a quoted value", "S + L", "no Cookie header"]
    cases = [c for c in T.corpus() if c.label in labels]
    assert len(cases) == len(labels)
    batch, cookies = T.batch_of(cases)
    ks = KeySet(T.KEYS)
    got = verify_cookies(ks, batch, cookies, T.NOW)
    assert [int(g) for g in got] == [c.expect for c in cases]
    # what §5.1.7 changes for the OTHER call stays out of this one: a sub with the NUL, and \u0000 anywhere, are not VERIFIED here
    cid = T.cid()
    with_nul = T.NAME + b"=" + T.token(sub=cid + NUL)
    escaped_jti = T.NAME + b"=" + T.token(jti="a" + NUL)
    req = cases[0].request()
    from pingoo_amd import verify_cookie

    assert verify_cookie(ks, req, with_nul, T.NOW) == CO.UNDECIDED and verify_cookie(ks, req, escaped_jti, T.NOW) == CO.UNDECIDED
    assert verify_cookie(ks, req, NAME + b"=" + T.token(), T.NOW) == CO.ABSENT  # the challenge cookie's name is not gate C's
    ks.close()


# ---- the shared header under the sanitizers -------------------------------------------------------------------------------------
def test_the_shared_header_under_asan_and_ubsan_reads_no_byte_outside_a_value():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "pow_host")
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                        os.path.join(ROOT, "include"), SRC, "-o", exe], check=True)
    hexed = lambda b: b.hex() or "-"  # noqa: E731
    lines = [f"K {kid.encode().hex()} {x.hex()}" for kid, x in KEYS]
    cases = corpus() + hash_flip_cases()[::17] + signature_flip_cases()[::7]
    lines.append(f"N {NOW}")
    for c in cases:
        ip = packed(c.ip)
        lines.append(f"Q {int(len(ip) == 16)} {ip.ljust(16, ZERO).hex()} {hexed(c.ua)} {hexed(c.host)} {'~' if c.cookie is None else hexed(c.cookie)} {c.digest.hex()} {hexed(c.nonce)}")
    lines.append(f"N {NOW + 300 + 6}")  # a second batch at a later `now`: the valid token has expired
    c = corpus()[0]
    lines.append(f"Q 0 {packed(c.ip).ljust(16, ZERO).hex()} {hexed(c.ua)} {hexed(c.host)} {hexed(c.cookie)} {c.digest.hex()} {hexed(c.nonce)}")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    out = [ln.split() for ln in r.stdout.split("\n") if ln.startswith("Q")]
    want = corpus_oracle() + [(F, False)] * len(hash_flip_cases()[::17]) + [(F, True)] * len(signature_flip_cases()[::7]) + [(F, False)]
    assert [(int(a), bool(int(b))) for _, a, b in out] == want
