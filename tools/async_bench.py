"""Throughput and latency of the non-blocking queue (pwaf_async_*) next to the blocking micro-batcher (pwaf_batcher_*), both driven by
native threads, on one synthetic workload (pysynth.Workload id; 3 = BASELINE.json configs[2], the 1024-rule set):
`python tools/async_bench.py [--config 3] [--threads 4] [--in-flight 2048] [--out FILE]`.
Prints (and writes with --out) one JSON object: {"async": ..., "blocking": ...}."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--in-flight", type=int, default=2048)
    ap.add_argument("--per-thread", type=int, default=250_000)
    ap.add_argument("--max-batch", type=int, default=8192)
    ap.add_argument("--deadline-us", type=int, default=200)
    ap.add_argument("--blocking-threads", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    from pingoo_amd.engine import RuleEngine, native_async_throughput, native_batcher_latency
    from synth import pysynth

    w = pysynth.Workload(a.config)
    eng = RuleEngine(w.rules, w.lists, w.geoip)
    batch = w.batch(0, 4096)
    res = {"config": a.config, "rules": len(w.rules)}
    res["async"] = native_async_throughput(eng, batch, threads=a.threads, in_flight=a.in_flight, per_thread=a.per_thread, max_batch=a.max_batch, max_delay_us=a.deadline_us)
    res["blocking"] = native_batcher_latency(eng, batch, threads=a.blocking_threads, per_thread=150)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
