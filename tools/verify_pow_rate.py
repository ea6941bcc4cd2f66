#!/usr/bin/env python3
"""What pwaf_verify_pow costs on one GPU (pow_check_kernel + pow_verify_kernel) and on one CPU thread; writes
profiles/verify_pow_rate.json.

A pool of --clients clients, each with its own address, User-Agent and host, a challenge token of its own (minted by tests/pow_oracle.py:
the reference's header and claims with the 43 characters and \\u0000 of challenge and sub) and a nonce that solves it at difficulty 1,
repeated to --requests submissions, device-resident. Three legs: (a) every submission passes; (b) every submission carries a wrong hash
under its valid token (one bit of the hash flipped: the flood an attacker can send); (c) every submission carries a validly signed token
whose claims lie outside the flat subset (a nested member): UNDECIDED. Next to (a), in the same run, pwaf_verify_cookies over as many
valid verified cookies of the same clients: the same curve work per entry. Each case: WARMUP warm-up and LAUNCHES timed calls, each
between two HIP events on the launch stream; median, min and max; the statuses of the last call are checked and scratch word 0 (the
entries handed to the signature stage) is recorded. Then the HOST mode of the same three legs on one thread over the first
--host-requests submissions (wall clock, median of three). Refuses to run without a GPU.

usage: python tools/verify_pow_rate.py [--requests 65536] [--clients 512] [--host-requests 2048] [--launches 10] [--warmup 3] [--commit ID] [--out FILE]"""
import argparse
import ctypes as C
import hashlib
import ipaddress
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=65536)
    ap.add_argument("--clients", type=int, default=512)
    ap.add_argument("--host-requests", type=int, default=2048)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_pow_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("verify_pow_rate.py measures the device call: no GPU is visible, nothing was measured")

    import cookie_oracle as CO
    import pow_oracle as O
    from pingoo_amd import KeySet, Request, RequestBatch, _abi
    from pingoo_amd.engine import DeviceBatch, cookie_column, lib

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    now = 1_800_000_000
    seeds = [bytes([k + 1] * 32) for k in range(2)]
    kids = ["0190b5a2-7c1e-7d43-9f6a-3b2c1d0e4f55", "0190b5a2-7c1e-7d43-9f6a-3b2c1d0e4f56"]  # Uuid::new_v7().to_string() (captcha.rs:111)
    keys = [(kid, CO.public_key(seed)) for kid, seed in zip(kids, seeds)]
    ks, ks_host = KeySet(keys, device=0), KeySet(keys)
    pool = []
    for k in range(args.clients):
        ip = f"10.{k >> 16 & 255}.{k >> 8 & 255}.{k & 255}" if k % 4 else f"2001:db8::{k + 1:x}"
        ua = b"Mozilla/5.0 (X11; Linux x86_64; rv:128.0) Gecko/20100101 Firefox/128.%d" % k
        host = b"shop%d.example.com" % (k % 50)
        ipb = ipaddress.ip_address(ip).packed
        challenge = O.heapless44(hashlib.sha256(b"challenge %d" % k).digest())
        nonce, digest = O.search_nonce(challenge.encode("latin-1"), 1, exactly=False)
        jti = "0190b5a2-7c1e-7d43-9f6a-%012x" % k
        claims = O.claims_json(O.client_sub(ipb, ua, host), now, challenge, 1, jti=jti)
        tok = O.mint(seeds[k % 2], O.header_json(kids[k % 2]), claims)
        odd = O.mint(seeds[k % 2], O.header_json(kids[k % 2]), claims[:-1] + b',"ctx":{"v":1}}')
        verified = CO.mint(seeds[k % 2], CO.header_json(kids[k % 2]), CO.claims_json(CO.client_id(ipb, ua, host), now, jti=jti))
        wrap = lambda name, t: b"session=8f2c1d0e4f55; " + name + b"=" + t + b"; theme=dark"  # noqa: E731
        pool.append(dict(req=Request(host=host, url=b"/__pingoo/captcha/api/verify", path=b"/__pingoo/captcha/api/verify", method=b"POST", user_agent=ua, ip=ip),
                         cookie=wrap(b"__pingoo_captcha", tok), odd=wrap(b"__pingoo_captcha", odd), verified=wrap(b"__pingoo_captcha_verified", verified), nonce=nonce, digest=digest,
                         wrong=digest[:31] + bytes([digest[31] ^ 1]), signed=len(tok) - 87))
    n = args.requests
    pick = lambda name: [pool[i % len(pool)][name] for i in range(n)]  # noqa: E731
    batch = RequestBatch.from_requests(pick("req"))
    db = DeviceBatch(batch, dev)
    st = db.as_struct()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches)]
        for a, b in ev:
            a.record(stream)
            fn()
            b.record(stream)
        torch.cuda.synchronize(dev)
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        return {"launches": len(ms), "median_ms": round(statistics.median(ms), 5), "min_ms": round(ms[0], 5), "max_ms": round(ms[-1], 5)}

    def column(values):
        data, off = cookie_column(values)
        d_data, d_off = torch.from_numpy(data).to(dev), torch.from_numpy(off.view(np.int32)).to(dev)
        col = _abi.StrCol()
        col.data, col.offsets = d_data.data_ptr(), d_off.data_ptr()
        hcol = _abi.StrCol()
        hcol.data, hcol.offsets = data.ctypes.data, off.ctypes.data
        return col, hcol, (d_data, d_off, data, off)

    ncol, h_ncol, keep_nonce = column(pick("nonce"))
    legs = {"passing": ("cookie", "digest", _abi.POW_PASSED), "wrong_hash": ("cookie", "wrong", _abi.POW_FAILED), "outside_subset": ("odd", "digest", _abi.POW_UNDECIDED)}
    host_inputs = {}

    def device_leg(cookie_name, hash_name, want):
        col, h_col, keep = column(pick(cookie_name))
        hashes = np.frombuffer(b"".join(pick(hash_name)), dtype=np.uint8).reshape(n, 32).copy()
        d_hashes = torch.from_numpy(hashes).to(dev)
        need = int(lib().pwaf_verify_pow_scratch_bytes(n))
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.zeros(n, dtype=torch.uint8, device=dev)

        def call():
            rc = lib().pwaf_verify_pow(ks._h, C.byref(st), C.byref(col), d_hashes.data_ptr(), C.byref(ncol), now, None, 0, None, out.data_ptr(), scratch.data_ptr(), need,
                                       C.c_void_p(stream.cuda_stream))
            assert rc == 0, lib().pwaf_last_error()

        t = timed(call)
        got = out.cpu().numpy()
        t.update(submissions=n, submissions_per_s=round(n / (t["median_ms"] / 1e3)), statuses_differing=int((got != want).sum()),
                 handed_to_signature_stage=int(scratch[:4].cpu().numpy().view(np.uint32)[0]))
        return t, (h_col, hashes, keep)

    result = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup, "clients": len(pool),
              "mean_signed_bytes": round(sum(p["signed"] for p in pool) / len(pool), 1)}
    for leg, (cookie_name, hash_name, want) in legs.items():
        result["device_" + leg], host_inputs[leg] = device_leg(cookie_name, hash_name, want)
    result["wrong_hash_over_passing"] = round(result["device_wrong_hash"]["median_ms"] / result["device_passing"]["median_ms"], 4)

    # ---- pwaf_verify_cookies over as many valid verified cookies, in the same run ----
    vcol, _, keep_verified = column(pick("verified"))
    need = int(lib().pwaf_verify_cookies_scratch_bytes(n))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.zeros(n, dtype=torch.uint8, device=dev)

    def cookies_call():
        rc = lib().pwaf_verify_cookies(ks._h, C.byref(st), C.byref(vcol), now, None, 0, None, out.data_ptr(), None, scratch.data_ptr(), need, C.c_void_p(stream.cuda_stream))
        assert rc == 0, lib().pwaf_last_error()

    t = timed(cookies_call)
    t.update(tokens=n, tokens_per_s=round(n / (t["median_ms"] / 1e3)), statuses_differing=int((out.cpu().numpy() != _abi.COOKIE_VERIFIED).sum()))
    result["device_verify_cookies_same_clients"] = t
    result["passing_over_verify_cookies"] = round(result["device_passing"]["median_ms"] / t["median_ms"], 4)

    # ---- the HOST mode of the same legs, one thread ----
    h = min(args.host_requests, n)
    hst = batch.view(0, h).as_struct()
    for leg, (_, _, want) in legs.items():
        h_col, hashes, _ = host_inputs[leg]
        out = np.zeros(h, dtype=np.uint8)
        secs = []
        for _ in range(3):
            t0 = time.perf_counter()
            rc = lib().pwaf_verify_pow(ks_host._h, C.byref(hst), C.byref(h_col), hashes.ctypes.data, C.byref(h_ncol), now, None, 0, None, out.ctypes.data, None, 0, None)
            secs.append(time.perf_counter() - t0)
            assert rc == 0
        med = statistics.median(secs)
        result["host_" + leg] = {"runs": 3, "median_ms": round(med * 1e3, 3), "min_ms": round(min(secs) * 1e3, 3), "max_ms": round(max(secs) * 1e3, 3), "submissions": h,
                                 "submissions_per_s": round(h / med), "statuses_differing": int((out != want).sum())}
        result["device_over_host_" + leg] = round(result["device_" + leg]["submissions_per_s"] / result["host_" + leg]["submissions_per_s"], 1)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    del keep_nonce, keep_verified


if __name__ == "__main__":
    main()
