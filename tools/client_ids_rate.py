#!/usr/bin/env python3
"""What pwaf_client_ids costs on one GPU (client_id_kernel) and on one CPU thread; writes profiles/client_ids_rate.json.

A seeded batch of the benchmark's workload (synth/, BASELINE.json configs[2]: its User-Agent and host lengths), device-resident:
(a) every request (idx NULL), (b) a match list of every tenth request, read on the device. Each case: WARMUP warm-up and LAUNCHES timed
calls, each between two HIP events on the launch stream; median, min and max. (c) In the same run, the HOST mode of the same call on one
thread over the first --host-requests requests (wall clock, median of three). Rates are requests per second and hashed SHA-256 blocks per
second (a request's blocks: (ip octets + User-Agent + host + 9 + 63) / 64). A sample of the device's ids is checked against hashlib.
Refuses to run without a GPU.

usage: python tools/client_ids_rate.py [--requests 1000000] [--host-requests 100000] [--launches 20] [--warmup 5] [--commit ID] [--out FILE]"""
import argparse
import base64
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=1_000_000)
    ap.add_argument("--host-requests", type=int, default=100_000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "client_ids_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("client_ids_rate.py measures the device call: no GPU is visible, nothing was measured")

    from pingoo_amd.engine import DeviceBatch, lib
    from synth import pysynth

    dev = torch.device("cuda", 0)
    threads = min(16, os.cpu_count() or 1)
    wl = pysynth.Workload(3)
    n = args.requests
    batch = wl.batch(0, n, threads=threads)
    db = DeviceBatch(batch, dev)
    stream = torch.cuda.current_stream(dev)
    UA, HOST = 4, 0
    ua_len = np.diff(batch.offsets[UA].astype(np.int64))
    host_len = np.diff(batch.offsets[HOST].astype(np.int64))
    blocks = (np.where(batch.ip_is_v6 != 0, 16, 4) + ua_len + host_len + 9 + 63) // 64

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

    def rates(t, requests, n_blocks):
        s = t["median_ms"] / 1e3
        t.update(requests=int(requests), blocks=int(n_blocks), requests_per_s=round(requests / s), blocks_per_s=round(n_blocks / s))
        return t

    def oracle(i):
        ip = batch.ip[i].tobytes()[:16 if batch.ip_is_v6[i] else 4]
        uo, ho = batch.offsets[UA], batch.offsets[HOST]
        return base64.urlsafe_b64encode(hashlib.sha256(ip + batch.data[UA][int(uo[i]):int(uo[i + 1])].tobytes() + batch.data[HOST][int(ho[i]):int(ho[i + 1])].tobytes()).digest()).rstrip(b"=")

    def device_case(idx):
        m = n if idx is None else len(idx)
        d_idx = None if idx is None else torch.from_numpy(idx.view(np.int32).copy()).to(dev)
        d_n = None if idx is None else torch.tensor([m], dtype=torch.int32, device=dev)
        d_out = torch.zeros((m, 44), dtype=torch.uint8, device=dev)
        st = db.as_struct()

        def call():
            rc = lib().pwaf_client_ids(C.byref(st), None if d_idx is None else d_idx.data_ptr(), 0 if idx is None else m, None if d_n is None else d_n.data_ptr(),
                                       d_out.data_ptr(), C.c_void_p(stream.cuda_stream))
            assert rc == 0, lib().pwaf_last_error()

        t = timed(call)
        which = np.arange(n) if idx is None else idx.astype(np.int64)
        rates(t, m, blocks[which].sum())
        out = d_out.cpu().numpy()
        pick = np.random.default_rng(1).choice(m, min(2000, m), replace=False)
        t["ids_checked_against_hashlib"] = int(len(pick))
        t["ids_differing"] = int(sum(out[j].tobytes()[:43] != oracle(int(which[j])) or out[j, 43] != 0 for j in pick))
        return t

    result = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup, "workload": "synth Workload(3)",
              "mean_user_agent_bytes": round(float(ua_len.mean()), 1), "mean_host_bytes": round(float(host_len.mean()), 1), "mean_blocks_per_request": round(float(blocks.mean()), 3),
              "max_blocks_of_a_request": int(blocks.max())}
    result["device_every_request"] = device_case(None)
    result["device_every_tenth_request"] = device_case(np.arange(0, n, 10, dtype=np.uint32))

    # ---- the HOST mode of the same call, one thread ----
    h = min(args.host_requests, n)
    view = batch.view(0, h)
    st = view.as_struct()
    out = np.zeros((h, 44), dtype=np.uint8)
    secs = []
    for _ in range(3):
        t0 = time.perf_counter()
        rc = lib().pwaf_client_ids(C.byref(st), None, 0, None, out.ctypes.data, None)
        secs.append(time.perf_counter() - t0)
        assert rc == 0
    host = rates({"runs": 3, "median_ms": round(statistics.median(secs) * 1e3, 3), "min_ms": round(min(secs) * 1e3, 3), "max_ms": round(max(secs) * 1e3, 3)}, h, blocks[:h].sum())
    host["ids_differing"] = int(sum(out[j].tobytes()[:43] != oracle(int(j)) for j in range(0, h, max(1, h // 2000))))
    result["host_mode_one_thread"] = host
    dev_rate = result["device_every_request"]["requests_per_s"]
    result["device_over_host_one_thread"] = round(dev_rate / host["requests_per_s"], 1)
    result["device_over_16_host_threads_worth"] = round(dev_rate / (16 * host["requests_per_s"]), 2)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
