#!/usr/bin/env python3
"""What pwaf_export_records costs on one GPU (pack_records_kernel); writes profiles/export_records.json.

(a) The headline workload of bench.py (BASELINE.json configs[2]: 10M device-resident requests, tuned engine): one evaluation leaves the
    non-Allow requests in match_idx / n_matches; the export is timed straight from those device buffers.
(b) The dense case: every request of a 1M-request batch, in request order.
Each case: a size query, then WARMUP warm-up and LAUNCHES timed calls, each between two HIP events on the launch stream (the 16-byte memset of
the statistics is inside the window: it is part of the call). Beside each, in the same process: a device-to-device hipMemcpyAsync of the
same byte count, timed the same way — the reference the kernel is judged against — and for (a) the copy of the whole batch's arenas, what a
caller without this function would have to move. GB/s are bytes WRITTEN per second (the kernel also reads as many).
The exported records are checked: those of (b), and a sample of (a), against the HOST mode of the same call.

usage: python tools/export_bench.py [--requests 10000000] [--dense 1000000] [--launches 20] [--warmup 5] [--commit ID]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=10_000_000)
    ap.add_argument("--dense", type=int, default=1_000_000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export_records.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from pingoo_amd import _abi
    from pingoo_amd.engine import DeviceBatch, RuleEngine, export_records, export_stats
    from synth import pysynth

    dev = torch.device("cuda", 0)
    threads = min(16, os.cpu_count() or 1)
    wl = pysynth.Workload(3)
    stream = torch.cuda.current_stream(dev)

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

    def copy_of(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        t = timed(lambda: dst.copy_(src, non_blocking=True))  # (device to device: hipMemcpyAsync on the current stream)
        t["bytes"] = nbytes
        t["gbs"] = round(nbytes / (t["median_ms"] / 1e3) / 1e9, 1)
        return t

    def case(db, batch, d_idx, d_n, check_entries):
        _, _, d_stats = export_records(db, d_idx, n_idx=d_n, cap=0)  # the size query
        torch.cuda.synchronize(dev)
        q = export_stats(d_stats)
        need = q["bytes_needed"]
        last = {}

        def call():
            last["r"] = export_records(db, d_idx, n_idx=d_n, cap=need)

        t = timed(call)
        d_buf, d_off, d_stats = last["r"]
        s = export_stats(d_stats)
        assert s == {"bytes_needed": need, "n_selected": q["n_selected"], "n_written": q["n_selected"]}, s
        t.update(records=s["n_written"], bytes_written=need, gbs_written=round(need / (t["median_ms"] / 1e3) / 1e9, 1), bytes_per_record=round(need / max(1, s["n_written"]), 1))
        t["memcpy_same_bytes"] = copy_of(need)
        t["kernel_over_memcpy"] = round(t["median_ms"] / t["memcpy_same_bytes"]["median_ms"], 3)
        # the records themselves, against the HOST mode of the same call
        idx = d_idx.cpu().numpy().view(np.uint32)[:s["n_selected"]]
        off = d_off.cpu().numpy().view(np.uint32)[:s["n_selected"]]
        pick = np.arange(len(idx)) if check_entries is None else np.random.default_rng(1).choice(len(idx), min(check_entries, len(idx)), replace=False)
        hbuf, hoff, _ = export_records(batch, idx[pick])
        buf = d_buf.cpu().numpy()
        bad = 0
        for j, o in zip(pick, hoff):
            size = int(hbuf[int(o):int(o) + 4].view(np.uint32)[0])
            bad += buf[int(off[j]):int(off[j]) + size].tobytes() != hbuf[int(o):int(o) + size].tobytes()
        t["records_checked_against_host_mode"] = int(len(pick))
        t["records_differing"] = int(bad)
        return t

    result = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "launches": args.launches, "warmup": args.warmup}

    # ---- (a) the headline workload's non-Allow requests, straight from match_idx ----
    n = args.requests
    batch = wl.batch(0, n, threads=threads)
    eng = RuleEngine(wl.rules, wl.lists, wl.geoip)
    eng.tune(wl.batch(n, 65536, threads=threads))  # (bench.py tunes on a sample disjoint from the timed batch)
    db = DeviceBatch(batch, dev)
    d_idx = torch.zeros(n, dtype=torch.int32, device=dev)
    d_nm = torch.zeros(1, dtype=torch.int32, device=dev)
    eng.evaluate_device(db, match_idx=d_idx, n_matches=d_nm)
    torch.cuda.synchronize(dev)
    eng.device_status()
    a = case(db, batch, d_idx, d_nm, 20000)
    arena = sum(db.arena_bytes)
    a.update(requests=n, non_allow=int(d_nm.item()), list="match_idx / n_matches of pwaf_evaluate_device, read on the device (idx_cap = requests)",
             whole_batch_arena_bytes=arena, memcpy_whole_batch_arenas=copy_of(arena))
    a["kernel_over_whole_batch_copy"] = round(a["median_ms"] / a["memcpy_whole_batch_arenas"]["median_ms"], 3)
    result["headline_non_allow"] = a
    eng.close()
    del db, batch, d_idx

    # ---- (b) every request of a 1M-request batch ----
    m = args.dense
    batch = wl.batch(0, m, threads=threads)
    db = DeviceBatch(batch, dev)
    b = case(db, batch, torch.arange(m, dtype=torch.int32, device=dev), None, 50000)
    b.update(requests=m, list="0 .. n - 1, n_idx NULL")
    result["dense_every_request"] = b

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
