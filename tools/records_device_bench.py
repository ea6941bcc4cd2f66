#!/usr/bin/env python3
"""What pwaf_evaluate_records_device costs on one GPU; writes profiles/records_device.json.

For the rule sets of BASELINE.json configs[2] (1024 rules, 5 string fields) and configs[4] (4096 rules, 5 + 64 string fields), tuned, on
--requests synthetic requests whose records pwaf_export_records wrote on the device (every request, in request order):
(a) pwaf_evaluate_records_device on those records where they lie: one call and the wait for its stream, wall clock;
(b) the only route the records had before: device -> host copy of the records and offsets into page-locked memory, then
    pwaf_evaluate_records from there, wall clock;
(c) the three scan launches and unpack_records_kernel of (a), each from pwaf_engine_kernel_times (HIP events; separate profiled calls);
(d) a plain pwaf_evaluate_device on the struct-of-arrays batch the records were exported from, and the wait, wall clock.
Every figure is the median of --calls calls after --warmup warm-up calls, in one process. The verdicts of (a), (b) and (d) are compared.

usage: python tools/records_device_bench.py [--requests 1000000] [--calls 9] [--warmup 3] [--commit ID]"""
import argparse
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
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "records_device.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from pingoo_amd.engine import DeviceBatch, RuleEngine, export_stats
    from synth import pysynth

    dev = torch.device("cuda", 0)
    threads = min(16, os.cpu_count() or 1)
    n = args.requests

    def wall(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        return {"calls": len(ms), "median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}

    result = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "requests": n, "calls": args.calls, "warmup": args.warmup, "configs": {}}
    for cfg in (int(c) for c in args.configs.split(",")):
        wl = pysynth.Workload(cfg)
        eng = RuleEngine(wl.rules, wl.lists, wl.geoip)
        eng.tune(wl.batch(n, 65536, threads=threads))
        batch = wl.batch(0, n, threads=threads)
        db = DeviceBatch(batch, dev)
        d_buf, d_off, d_stats = eng.export_records(db, torch.arange(n, dtype=torch.int32, device=dev))
        torch.cuda.synchronize(dev)
        st = export_stats(d_stats)
        assert st["n_written"] == n, st
        d_buf = d_buf[:st["bytes_needed"]].clone()  # exactly the records' bytes: no pad behind them
        out_a = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        out_d = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        h_buf = torch.empty(st["bytes_needed"], dtype=torch.uint8, pin_memory=True)
        h_off = torch.empty(n, dtype=torch.int32, pin_memory=True)
        host = {}

        def route_b():
            h_buf.copy_(d_buf)
            h_off.copy_(d_off)
            torch.cuda.synchronize(dev)
            host["out"] = eng.evaluate_records(h_buf.numpy(), h_off.numpy().view(np.uint32))

        r = {"rules": len(wl.rules), "header_fields": len(eng.header_names), "record_bytes": st["bytes_needed"], "bytes_per_record": round(st["bytes_needed"] / n, 1)}
        r["a_evaluate_records_device"] = wall(lambda: eng.evaluate_records_device(d_buf, d_off, out=out_a))
        r["b_copy_to_host_then_evaluate_records"] = wall(route_b)
        r["d_evaluate_device_on_the_batch"] = wall(lambda: eng.evaluate_device(db, out=out_d))
        eng.device_status()
        a, d = out_a.cpu().numpy(), out_d.cpu().numpy()
        r["verdicts_differing_a_vs_d"] = int((a != d).any(axis=1).sum())
        r["verdicts_differing_b_vs_d"] = int((host["out"].view(np.int32).reshape(-1, 2) != d).any(axis=1).sum())
        # (c) per launch, from profiled calls of their own
        per = {}
        for k in range(args.warmup + args.calls):
            eng.set_profiling(1)
            eng.evaluate_records_device(d_buf, d_off, out=out_a)
            torch.cuda.synchronize(dev)
            times = eng.kernel_times()[:4]
            eng.set_profiling(0)
            if k >= args.warmup:
                for name, ms, _ in times:
                    per.setdefault(name, []).append(ms)
        r["c_kernels_median_ms"] = {name: round(statistics.median(v), 4) for name, v in per.items()}
        scan = sum(v for name, v in r["c_kernels_median_ms"].items() if name != "unpack_records_kernel")
        r["c_scan_launches_ms"] = round(scan, 4)
        r["c_scan_over_unpack"] = round(scan / r["c_kernels_median_ms"]["unpack_records_kernel"], 3)
        r["a_minus_d_ms"] = round(r["a_evaluate_records_device"]["median_ms"] - r["d_evaluate_device_on_the_batch"]["median_ms"], 4)
        r["a_over_b"] = round(r["a_evaluate_records_device"]["median_ms"] / r["b_copy_to_host_then_evaluate_records"]["median_ms"], 3)
        result["configs"][f"configs[{cfg - 1}]"] = r
        eng.close()
        del db, batch, d_buf, d_off, out_a, out_d, h_buf, h_off
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
