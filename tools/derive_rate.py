#!/usr/bin/env python3
"""What pwaf_derive_batch costs on one GPU (derive_span_kernel, derive_base_kernel, derive_copy_kernel); writes profiles/derive_rate.json.

A seeded batch of synth/'s benign shape (the benchmark's workload), device-resident, taken as the raw batch: its host, path and user_agent
columns stand for the Host header, uri.path() and the User-Agent header (no URI hosts, every request has both headers). WARMUP warm-up and
LAUNCHES timed calls of pwaf_derive_batch, each between two HIP events on the launch stream: median, min and max of the three launches
together. The yardstick, in the same process on the same device: a device-to-device copy of as many bytes as the call's string traffic (the
raw bytes of the three columns read + the derived bytes written), timed the same way. A sample of the derived values is checked against
get_host / get_path / get_user_agent. Refuses to run without a GPU.

usage: python tools/derive_rate.py [--requests 1000000] [--launches 20] [--warmup 5] [--commit ID] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=1_000_000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derive_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("derive_rate.py measures the device call: no GPU is visible, nothing was measured")

    from pingoo_amd import _abi
    from pingoo_amd.engine import DERIVED_FIELDS, DeviceBatch, derive_stats, get_host, get_path, get_user_agent, lib
    from synth import pysynth

    dev = torch.device("cuda", 0)
    n = args.requests
    batch = pysynth.Workload(3).batch(0, n, threads=min(16, os.cpu_count() or 1))
    db = DeviceBatch(batch, dev)
    stream = torch.cuda.current_stream(dev)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(max(20, args.launches))]
        for a, b in ev:
            a.record(stream)
            fn()
            b.record(stream)
        torch.cuda.synchronize(dev)
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        return {"launches": len(ms), "median_ms": round(statistics.median(ms), 5), "min_ms": round(ms[0], 5), "max_ms": round(ms[-1], 5)}

    # the call as a host in C makes it: outputs and scratch allocated once (room: the raw column's bytes + 16)
    raw_bytes = [db.field_bytes[f] for f in DERIVED_FIELDS]
    data = [torch.empty(b + _abi.ARENA_PAD, dtype=torch.uint8, device=dev) for b in raw_bytes]
    offs = [torch.empty(n + 1, dtype=torch.int32, device=dev) for _ in raw_bytes]
    d_stats = torch.empty(32, dtype=torch.uint8, device=dev)
    need = int(lib().pwaf_derive_scratch_bytes(n))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    cols = (_abi.DerivedCol * 3)()
    for c in range(3):
        cols[c].data, cols[c].offsets, cols[c].cap = data[c].data_ptr(), offs[c].data_ptr(), data[c].numel()
    st = db.as_struct()

    def call():
        rc = lib().pwaf_derive_batch(C.byref(st), None, cols, d_stats.data_ptr(), scratch.data_ptr(), need, C.c_void_p(stream.cuda_stream))
        assert rc == 0, lib().pwaf_last_error()

    t = timed(call)
    derived = DeviceBatch.adopt(db, {f: (data[c], offs[c]) for c, f in enumerate(DERIVED_FIELDS)})
    stats = derive_stats(d_stats)
    traffic = sum(raw_bytes) + sum(stats["bytes"])
    t.update(requests=n, requests_per_s=round(n / (t["median_ms"] / 1e3)), raw_bytes=raw_bytes, derived_bytes=stats["bytes"], overflow=stats["overflow"],
             string_bytes_moved=traffic, gb_per_s=round(traffic / (t["median_ms"] / 1e3) / 1e9, 1))
    # a sample against the per-request functions
    pick = np.random.default_rng(1).choice(n, min(2000, n), replace=False)
    differing = 0
    for c, f in enumerate(DERIVED_FIELDS):
        o = derived.offsets[f].cpu().numpy().view(np.uint32)
        blob = derived.data[f].cpu().numpy()
        fn = (lambda v: get_host(None, v), get_path, get_user_agent)[c]
        differing += sum(blob[o[i]:o[i + 1]].tobytes() != fn(batch.field_bytes(f, int(i))) for i in pick)
    t["values_checked"], t["values_differing"] = 3 * len(pick), int(differing)

    src = torch.empty(traffic, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    copy = timed(lambda: dst.copy_(src))
    copy.update(bytes=traffic, gb_per_s_copied=round(traffic / (copy["median_ms"] / 1e3) / 1e9, 1))

    props = torch.cuda.get_device_properties(0)  # (the marketing name is often generic: the architecture, CU count and memory identify the part)
    device = f"{props.name}, {getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, {props.total_memory / 2**30:.0f} GiB"
    result = {"commit": args.commit, "device": device, "warmup": args.warmup, "workload": "synth Workload(3), benign, taken as the raw batch",
              "derive_three_launches": t, "device_to_device_copy_of_the_same_bytes": copy, "derive_over_copy": round(t["median_ms"] / copy["median_ms"], 2)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
