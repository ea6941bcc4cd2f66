#!/usr/bin/env python3
"""What pwaf_parse_pow_bodies costs on one GPU (powbody_parse_kernel + powbody_base_kernel + powbody_copy_kernel) and on one CPU thread;
writes profiles/parse_pow_rate.json.

The client pool of tools/verify_pow_rate.py (each client its own address, User-Agent, host, challenge token and a nonce that solves it at
difficulty 1), repeated to --requests submissions whose bodies lie in device memory. Three legs: (a) the genuine body
{"nonce":"<decimal>","hash":"<64 hex>"}; (b) bodies that are MALFORMED at their first byte; (c) bodies UNDECIDED by an unknown member
behind a genuine prefix. Each leg: WARMUP warm-up and LAUNCHES timed calls, each between two HIP events on the launch stream; median, min
and max; every status, hash row and nonce of the last call is checked against tests/powbody_oracle.py. Next to each leg, in the same
run: a device-to-device hipMemcpyAsync of the same body bytes (the yardstick for a kernel that should read each body once);
pwaf_verify_pow over the same submissions, fed with the columns the parse wrote (what share of the chain the parse adds); the same call
through a list that names every request (the form the chain uses: the memset and the base launch's own tile sums); and the HOST mode on
one thread over the first --host-requests bodies (wall clock, median of three). Refuses to run without a GPU.

usage: python tools/parse_pow_rate.py [--requests 65536] [--clients 512] [--host-requests 2048] [--launches 10] [--warmup 3] [--commit ID] [--out FILE]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parse_pow_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("parse_pow_rate.py measures the device call: no GPU is visible, nothing was measured")

    import cookie_oracle as CO
    import pow_oracle as PO
    import powbody_oracle as O
    from pingoo_amd import KeySet, Request, RequestBatch, _abi
    from pingoo_amd.engine import DeviceBatch, body_column, body_stats, cookie_column, lib

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    now = 1_800_000_000
    seeds = [bytes([k + 1] * 32) for k in range(2)]
    kids = ["0190b5a2-7c1e-7d43-9f6a-3b2c1d0e4f55", "0190b5a2-7c1e-7d43-9f6a-3b2c1d0e4f56"]
    ks = KeySet([(kid, CO.public_key(seed)) for kid, seed in zip(kids, seeds)], device=0)
    pool = []
    for k in range(args.clients):
        ip = f"10.{k >> 16 & 255}.{k >> 8 & 255}.{k & 255}" if k % 4 else f"2001:db8::{k + 1:x}"
        ua = b"Mozilla/5.0 (X11; Linux x86_64; rv:128.0) Gecko/20100101 Firefox/128.%d" % k
        host = b"shop%d.example.com" % (k % 50)
        ipb = ipaddress.ip_address(ip).packed
        challenge = PO.heapless44(hashlib.sha256(b"challenge %d" % k).digest())
        nonce, digest = PO.search_nonce(challenge.encode("latin-1"), 1, exactly=False)
        claims = PO.claims_json(PO.client_sub(ipb, ua, host), now, challenge, 1, jti="0190b5a2-7c1e-7d43-9f6a-%012x" % k)
        tok = PO.mint(seeds[k % 2], PO.header_json(kids[k % 2]), claims)
        body = O.genuine(nonce, digest)
        pool.append(dict(req=Request(host=host, url=b"/__pingoo/captcha/api/verify", path=b"/__pingoo/captcha/api/verify", method=b"POST", user_agent=ua, ip=ip),
                         cookie=b"session=8f2c1d0e4f55; __pingoo_captcha=" + tok + b"; theme=dark", genuine=body, malformed_first_byte=b"x" + body[1:],
                         unknown_member=body[:-1] + b',"x":1}'))
    n = args.requests
    pick = lambda name: [pool[i % len(pool)][name] for i in range(n)]  # noqa: E731
    batch = RequestBatch.from_requests(pick("req"))
    db = DeviceBatch(batch, dev)
    st = db.as_struct()
    c_data, c_off = cookie_column(pick("cookie"))
    d_cookies = (torch.from_numpy(c_data).to(dev), torch.from_numpy(c_off.view(np.int32)).to(dev))
    ccol = _abi.StrCol()
    ccol.data, ccol.offsets = d_cookies[0].data_ptr(), d_cookies[1].data_ptr()

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

    result = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup, "clients": len(pool), "bodies": n}
    want_pow = {"genuine": _abi.POW_PASSED, "malformed_first_byte": _abi.POW_FAILED, "unknown_member": _abi.POW_FAILED}
    for leg in ("genuine", "malformed_first_byte", "unknown_member"):
        bodies = pick(leg)
        data, off = body_column(bodies)
        d_data, d_off = torch.from_numpy(data).to(dev), torch.from_numpy(off.view(np.int32)).to(dev)
        col = _abi.StrCol()
        col.data, col.offsets = d_data.data_ptr(), d_off.data_ptr()
        cap = len(data) + _abi.ARENA_PAD
        status, hashes = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        ndata, noff = torch.zeros(cap, dtype=torch.uint8, device=dev), torch.zeros(n + 1, dtype=torch.int32, device=dev)
        stats = torch.zeros(32, dtype=torch.uint8, device=dev)
        need = int(lib().pwaf_parse_pow_bodies_scratch_bytes(n))
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        every = torch.arange(n, dtype=torch.int32, device=dev)
        ncol = _abi.DerivedCol()
        ncol.data, ncol.offsets, ncol.cap = ndata.data_ptr(), noff.data_ptr(), cap

        def parse(idx=None):
            rc = lib().pwaf_parse_pow_bodies(C.byref(col), n, _abi.MEM_DEVICE, None if idx is None else idx.data_ptr(), 0 if idx is None else n, None, status.data_ptr(), hashes.data_ptr(),
                                             C.byref(ncol), stats.data_ptr(), scratch.data_ptr(), need, C.c_void_p(stream.cuda_stream))
            assert rc == 0, lib().pwaf_last_error()

        def check():
            want = [O.decide(b) for b in bodies]
            got_status, got_rows, got_off, got_data = status.cpu().numpy(), hashes.cpu().numpy(), noff.cpu().numpy().view(np.uint32), ndata.cpu().numpy()
            ends = np.cumsum([0] + [len(w[2]) for w in want])
            differing = int((got_status != np.array([w[0] for w in want], dtype=np.uint8)).sum())
            differing += int((got_rows != np.frombuffer(b"".join(w[1] for w in want), dtype=np.uint8).reshape(n, 32)).any(axis=1).sum())
            differing += int((got_off != ends).sum()) + int(bytes(got_data[:ends[-1]]) != b"".join(w[2] for w in want))
            return differing, body_stats(stats)

        t = timed(parse)
        differing, bstats = check()
        t.update(bodies=n, body_bytes=int(off[-1]), bodies_per_s=round(n / (t["median_ms"] / 1e3)), gb_per_s=round(int(off[-1]) / (t["median_ms"] / 1e3) / 1e9, 2),
                 answers_differing_from_the_oracle=differing, stats=bstats)
        result["device_" + leg] = t
        tl = timed(lambda: parse(every))
        differing, _ = check()
        tl.update(answers_differing_from_the_oracle=differing)
        result["device_" + leg + "_through_a_list"] = tl

        # the yardstick: a device-to-device copy of the same body bytes
        src, dst = d_data[:int(off[-1])], torch.empty(int(off[-1]), dtype=torch.uint8, device=dev)
        tc = timed(lambda: dst.copy_(src, non_blocking=True))
        result["device_copy_" + leg] = tc
        result["parse_over_copy_" + leg] = round(t["median_ms"] / tc["median_ms"], 2)

        # pwaf_verify_pow over the same submissions, fed with what the parse wrote
        vneed = int(lib().pwaf_verify_pow_scratch_bytes(n))
        vscratch, vout = torch.empty(vneed, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
        vncol = _abi.StrCol()
        vncol.data, vncol.offsets = ndata.data_ptr(), noff.data_ptr()

        def verify():
            rc = lib().pwaf_verify_pow(ks._h, C.byref(st), C.byref(ccol), hashes.data_ptr(), C.byref(vncol), now, None, 0, None, vout.data_ptr(), vscratch.data_ptr(), vneed,
                                       C.c_void_p(stream.cuda_stream))
            assert rc == 0, lib().pwaf_last_error()

        parse()
        tv = timed(verify)
        tv.update(statuses_differing=int((vout.cpu().numpy() != want_pow[leg]).sum()))
        result["device_verify_pow_" + leg] = tv
        result["parse_share_of_the_chain_" + leg] = round(t["median_ms"] / (t["median_ms"] + tv["median_ms"]), 4)

        # the HOST mode, one thread
        h = min(args.host_requests, n)
        hcol, hncol = _abi.StrCol(), _abi.DerivedCol()
        hcol.data, hcol.offsets = data.ctypes.data, off.ctypes.data
        hstatus, hrows, hoff, hstats = np.zeros(h, dtype=np.uint8), np.zeros((h, 32), dtype=np.uint8), np.zeros(h + 1, dtype=np.uint32), np.zeros(4, dtype=np.uint64)
        raw = np.zeros(int(off[h]) + 32, dtype=np.uint8)
        hdata = raw[-raw.ctypes.data % 16:]
        hncol.data, hncol.offsets, hncol.cap = hdata.ctypes.data, hoff.ctypes.data, int(off[h]) + 16
        secs = []
        for _ in range(3):
            t0 = time.perf_counter()
            rc = lib().pwaf_parse_pow_bodies(C.byref(hcol), h, _abi.MEM_HOST, None, 0, None, hstatus.ctypes.data, hrows.ctypes.data, C.byref(hncol), hstats.ctypes.data, None, 0, None)
            secs.append(time.perf_counter() - t0)
            assert rc == 0
        med = statistics.median(secs)
        result["host_" + leg] = {"runs": 3, "median_ms": round(med * 1e3, 3), "min_ms": round(min(secs) * 1e3, 3), "max_ms": round(max(secs) * 1e3, 3), "bodies": h,
                                 "bodies_per_s": round(h / med), "statuses_differing": int((hstatus != np.array([O.decide(b)[0] for b in bodies[:h]], dtype=np.uint8)).sum())}
        result["device_over_host_" + leg] = round(t["bodies_per_s"] / result["host_" + leg]["bodies_per_s"], 1)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
