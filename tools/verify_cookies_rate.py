#!/usr/bin/env python3
"""What pwaf_verify_cookies costs on one GPU (cookie_locate_kernel + cookie_verify_kernel) and on one CPU thread; writes
profiles/verify_cookies_rate.json.

A pool of --clients clients, each with its own address, User-Agent and host and a valid token of its own (minted by tests/cookie_oracle.py:
the reference's header and claims, about 330 signed bytes), repeated to --requests requests, device-resident. (a) every request carries
its token; (b) one request in 16 does, the others carry an ordinary Cookie header without it. Each case: WARMUP warm-up and LAUNCHES timed
calls, each between two HIP events on the launch stream; median, min and max; the statuses of the last call are checked (VERIFIED exactly
where a token is). (c) In the same run, the HOST mode of the same call on one thread over the first --host-requests requests of (a) (wall
clock, median of three). Rates are tokens verified per second. Refuses to run without a GPU.

usage: python tools/verify_cookies_rate.py [--requests 65536] [--clients 512] [--host-requests 2048] [--launches 10] [--warmup 3] [--commit ID] [--out FILE]"""
import argparse
import ctypes as C
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_cookies_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("verify_cookies_rate.py measures the device call: no GPU is visible, nothing was measured")

    import cookie_oracle as O
    from pingoo_amd import KeySet, Request, RequestBatch, _abi
    from pingoo_amd.engine import DeviceBatch, cookie_column, lib

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    now = 1_800_000_000
    seeds = [bytes([k + 1] * 32) for k in range(2)]
    kids = ["0190b5a2-7c1e-7d43-9f6a-3b2c1d0e4f55", "0190b5a2-7c1e-7d43-9f6a-3b2c1d0e4f56"]  # Uuid::new_v7().to_string() (captcha.rs:111)
    keys = [(kid, O.public_key(seed)) for kid, seed in zip(kids, seeds)]
    ks, ks_host = KeySet(keys, device=0), KeySet(keys)
    pool = []
    for k in range(args.clients):
        ip = f"10.{k >> 16 & 255}.{k >> 8 & 255}.{k & 255}" if k % 4 else f"2001:db8::{k + 1:x}"
        ua = b"Mozilla/5.0 (X11; Linux x86_64; rv:128.0) Gecko/20100101 Firefox/128.%d" % k
        host = b"shop%d.example.com" % (k % 50)
        sub = O.client_id(ipaddress.ip_address(ip).packed, ua, host)
        tok = O.mint(seeds[k % 2], O.header_json(kids[k % 2]), O.claims_json(sub, now, jti="0190b5a2-7c1e-7d43-9f6a-%012x" % k))
        pool.append((Request(host=host, url=b"/cart", path=b"/cart", method=b"GET", user_agent=ua, ip=ip), b"session=8f2c1d0e4f55; __pingoo_captcha_verified=" + tok + b"; theme=dark", len(tok) - 87))
    n = args.requests
    batch = RequestBatch.from_requests([pool[i % len(pool)][0] for i in range(n)])
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

    def device_case(every):
        cookies = [pool[i % len(pool)][1] if i % every == 0 else b"session=8f2c1d0e4f55; theme=dark" for i in range(n)]
        data, off = cookie_column(cookies)
        d_data, d_off = torch.from_numpy(data).to(dev), torch.from_numpy(off.view(np.int32)).to(dev)
        col = _abi.StrCol()
        col.data, col.offsets = d_data.data_ptr(), d_off.data_ptr()
        need = int(lib().pwaf_verify_cookies_scratch_bytes(n))
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.zeros(n, dtype=torch.uint8, device=dev)

        def call():
            rc = lib().pwaf_verify_cookies(ks._h, C.byref(st), C.byref(col), now, None, 0, None, out.data_ptr(), None, scratch.data_ptr(), need, C.c_void_p(stream.cuda_stream))
            assert rc == 0, lib().pwaf_last_error()

        t = timed(call)
        tokens = len(range(0, n, every))
        got = out.cpu().numpy()
        want = np.where(np.arange(n) % every == 0, _abi.COOKIE_VERIFIED, _abi.COOKIE_ABSENT)
        t.update(requests=n, tokens=tokens, tokens_per_s=round(tokens / (t["median_ms"] / 1e3)), requests_per_s=round(n / (t["median_ms"] / 1e3)), statuses_differing=int((got != want).sum()))
        return t, (data, off)

    result = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup, "clients": len(pool),
              "mean_signed_bytes": round(sum(p[2] for p in pool) / len(pool), 1)}
    result["device_every_request"], column = device_case(1)
    result["device_one_request_in_16"], _ = device_case(16)

    # ---- the HOST mode of the same call, one thread ----
    h = min(args.host_requests, n)
    view = batch.view(0, h)
    hst = view.as_struct()
    col = _abi.StrCol()
    col.data, col.offsets = column[0].ctypes.data, column[1].ctypes.data
    out = np.zeros(h, dtype=np.uint8)
    secs = []
    for _ in range(3):
        t0 = time.perf_counter()
        rc = lib().pwaf_verify_cookies(ks_host._h, C.byref(hst), C.byref(col), now, None, 0, None, out.ctypes.data, None, None, 0, None)
        secs.append(time.perf_counter() - t0)
        assert rc == 0
    med = statistics.median(secs)
    result["host_mode_one_thread"] = {"runs": 3, "median_ms": round(med * 1e3, 3), "min_ms": round(min(secs) * 1e3, 3), "max_ms": round(max(secs) * 1e3, 3), "tokens": h,
                                      "tokens_per_s": round(h / med), "statuses_differing": int((out != _abi.COOKIE_VERIFIED).sum())}
    result["device_over_host_one_thread"] = round(result["device_every_request"]["tokens_per_s"] / result["host_mode_one_thread"]["tokens_per_s"], 1)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
