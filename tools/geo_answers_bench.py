#!/usr/bin/env python3
"""What the GeoIP answers (PWAF_OPT_GEO_ANSWERS) cost, measured on one GPU; writes profiles/geo_answers.json.

1. The kernel alone: pwaf_geoip_lookup on the device-resident addresses of the headline batch (BASELINE.json configs[2], 10M requests),
   HIP events around every launch (pwaf_engine_set_profiling), LAUNCHES launches after warmup. Beside it, in the same process:
   ipres_kernel on the same addresses — (a) alone: an engine over the same lists and GeoIP table whose rules are the workload's rules
   that read nothing but the client (no scans run, so nothing runs beside it); (b) inside the full pipeline of the headline engine.
   The kernel's floor is its compulsory traffic, 25 bytes per request (16 address + 1 family in, 8 out), at the HBM peak.
2. What the answers cost a batch: two engines in one process, flag off and flag on with a device `geo` output, alternated REPEATS
   times, STEPS timed steps each after WARMUP warmup steps; the step-time difference and the spread of the flag-off repeats.

usage: python tools/geo_answers_bench.py [--requests N] [--launches 50] [--steps 20] [--warmup 5] [--repeats 3] [--commit ID]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
FLOOR_BYTES = 25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geo_answers.json"))
    args = ap.parse_args()

    import torch

    from pingoo_amd import _abi
    from pingoo_amd.engine import DeviceBatch, RuleEngine, lib
    from synth import pysynth

    dev = torch.device("cuda", 0)
    n = args.requests
    threads = min(16, os.cpu_count() or 1)
    wl = pysynth.Workload(3)
    batch = wl.batch(0, n, threads=threads)
    sample = wl.batch(n, 65536, threads=threads)  # (bench.py tunes on a sample disjoint from the timed batch)
    engines = {}
    for name, flags in (("off", 0), ("on", _abi.OPT_GEO_ANSWERS)):
        t0 = time.time()
        engines[name] = RuleEngine(wl.rules, wl.lists, wl.geoip, flags=flags)
        create_s = time.time() - t0
        engines[name].tune(sample)
        print(f"[geo_answers_bench] engine {name}: created in {create_s:.2f} s", file=sys.stderr)
        engines[name + "_create_s"] = create_s
    on, off = engines["on"], engines["off"]
    db = DeviceBatch(batch, dev)
    stream = torch.cuda.current_stream(dev)
    result = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "requests": n, "workload": "BASELINE.json configs[2]: synthetic 1k-rule WAF, device-resident batch",
              "geo_answer_tables": on.geo_answer_tables(), "address_tables": on.address_tables(), "engine_create_s": {"flag_off": round(engines["off_create_s"], 3), "flag_on": round(engines["on_create_s"], 3)}}

    # ---- 1. the kernel alone ----
    geo = torch.zeros((n, 2), dtype=torch.int32, device=dev)

    def lookups(k):
        for _ in range(k):
            rc = lib().pwaf_geoip_lookup(on._h, db.ip.data_ptr(), db.ip_is_v6.data_ptr(), n, _abi.MEM_DEVICE, geo.data_ptr(), C.c_void_p(stream.cuda_stream))
            assert rc == 0, lib().pwaf_last_error()
        torch.cuda.synchronize(dev)

    lookups(10)
    on.set_profiling(1)
    lookups(args.launches)
    ms = [t[1] for t in on.kernel_times() if t[0] == "georec"]
    on.set_profiling(0)
    assert len(ms) == args.launches

    def summary(xs):
        xs = sorted(xs)
        return {"launches": len(xs), "median_ms": round(statistics.median(xs), 5), "min_ms": round(xs[0], 5), "max_ms": round(xs[-1], 5), "mean_ms": round(statistics.fmean(xs), 5)}

    floor_ms = n * FLOOR_BYTES / (HBM_PEAK_GBS * 1e9) * 1e3
    k = summary(ms)
    k["floor_ms_25B_per_request_at_8TBs"] = round(floor_ms, 5)
    k["share_of_floor_bound"] = round(floor_ms / k["median_ms"], 4)
    k["achieved_gbs_of_compulsory_traffic"] = round(n * FLOOR_BYTES / (k["median_ms"] / 1e3) / 1e9, 1)
    result["georec_kernel_alone"] = k

    # ipres_kernel on the same addresses: (a) alone, (b) inside the headline pipeline
    out = torch.empty((n, 2), dtype=torch.int32, device=dev)

    def ipres_times(eng, launches):
        for _ in range(5):
            eng.evaluate_device(db, out=out)
        torch.cuda.synchronize(dev)
        eng.set_profiling(1)
        for _ in range(launches):
            eng.evaluate_device(db, out=out)
        torch.cuda.synchronize(dev)
        kt = eng.kernel_times()
        eng.set_profiling(0)
        return [t[1] for t in kt if t[0] == "ipres"], sorted({t[0] for t in kt})

    client_rules = [r for r in wl.rules if r[1] is not None and "http_request" not in r[1]]
    if client_rules:
        alone = RuleEngine(client_rules, wl.lists, wl.geoip)
        ims, names = ipres_times(alone, args.launches)
        result["ipres_kernel_alone"] = dict(summary(ims), rules=len(client_rules), kernels_of_the_batch=names, address_tables=alone.address_tables(),
                                            note="an engine over the same lists and GeoIP table with the workload's client-only rules: no scan runs beside the lookup")
        alone.close()
    else:
        result["ipres_kernel_alone"] = "not measured: the workload has no rule that reads the client alone"
    ims, _ = ipres_times(off, args.launches)
    result["ipres_kernel_in_the_headline_pipeline"] = dict(summary(ims), note="the headline engine's own launch, on the side stream beside the batch's other kernels")
    if isinstance(result["ipres_kernel_alone"], dict):
        result["georec_over_ipres_alone"] = round(k["median_ms"] / result["ipres_kernel_alone"]["median_ms"], 4)

    # ---- 2. what the answers cost a batch ----
    cnt = torch.zeros(4, dtype=torch.int64, device=dev)

    def steps_ms(eng, with_geo):
        eng.set_profiling(2)  # (as bench.py's timed steps: events around the streaming launch only)
        for _ in range(args.warmup):
            eng.evaluate_device(db, out=out, counts=cnt, geo=geo if with_geo else None)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            eng.evaluate_device(db, out=out, counts=cnt, geo=geo if with_geo else None)
        torch.cuda.synchronize(dev)
        el = time.perf_counter() - t0
        eng.kernel_times()
        eng.set_profiling(0)
        return 1e3 * el / args.steps

    t_off, t_on = [], []
    for _ in range(args.repeats):
        t_off.append(steps_ms(off, False))
        t_on.append(steps_ms(on, True))
    result["batch_cost"] = {"steps": args.steps, "warmup": args.warmup, "flag_off_ms_per_step": [round(x, 4) for x in t_off], "flag_on_with_geo_ms_per_step": [round(x, 4) for x in t_on],
                            "delta_ms": round(statistics.fmean(t_on) - statistics.fmean(t_off), 4), "flag_off_spread_ms": round(max(t_off) - min(t_off), 4)}
    # the answers themselves: the evaluate path's records are the lookup's
    chk = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    assert lib().pwaf_geoip_lookup(on._h, db.ip.data_ptr(), db.ip_is_v6.data_ptr(), n, _abi.MEM_DEVICE, chk.data_ptr(), C.c_void_p(stream.cuda_stream)) == 0
    torch.cuda.synchronize(dev)
    result["evaluate_records_equal_lookup"] = bool(torch.equal(chk, geo))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
