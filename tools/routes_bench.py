#!/usr/bin/env python3
"""What answering each request's service route in the verdict's pass costs, measured on one GPU; writes profiles/routes.json.

The headline workload of bench.py (BASELINE.json configs[2]: 10M device-resident requests, 1024 rules) with 16 routes — host prefixes,
path prefixes, one regex and a catch-all, their literals drawn from a sample of the stream. Four configurations in one process,
alternated ROUNDS times, STEPS timed device-resident steps each after WARMUP warm-up steps:
  (a) the engine without routes;
  (b) the routed engine, no route output asked for (the plain kernels over rules + routes);
  (c) the routed engine with the route output (verdict2_kernel's ROUTES variant; 4 more bytes written per request);
  (d) (a) followed by a separate ServiceRouter engine over the same routes, the same batch: what the feature replaces.
Beside the step times: the verdict kernel's own time from HIP events around every launch, taken in the warm-up steps (profiling level 1
there, level 2 — as bench.py — in the timed steps).

usage: python tools/routes_bench.py [--requests N] [--steps 20] [--warmup 5] [--rounds 3] [--commit ID]"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pick_routes(sample, n_host=7, n_path=7):
    """16 routes over what the stream carries: the first bytes of its most frequent hosts, its most frequent first path segments, one
    regex, a catch-all"""
    hosts = collections.Counter(sample.field_bytes(0, i)[:5] for i in range(sample.n))
    segs = collections.Counter(b"/".join(sample.field_bytes(2, i).split(b"/")[:2]) + b"/" for i in range(sample.n))

    def text(b):
        return '"' + b.decode("latin-1").replace("\\", "\\\\").replace('"', '\\"') + '"'

    printable = lambda b: len(b) >= 3 and all(0x20 <= c < 0x7F for c in b)
    routes = [(f"host{k}", f"http_request.host.starts_with({text(h)})") for k, (h, _) in enumerate([x for x in hosts.most_common(40) if printable(x[0])][3:3 + n_host])]
    routes += [(f"path{k}", f"http_request.path.starts_with({text(s)})") for k, (s, _) in enumerate([x for x in segs.most_common(40) if printable(x[0])][:n_path])]
    routes.append(("versioned", 'http_request.url.matches("^/v[0-9]+/[a-z]+")'))
    routes.append(("default", None))
    return routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "routes.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from pingoo_amd.engine import DeviceBatch, RuleEngine, ServiceRouter
    from synth import pysynth

    dev = torch.device("cuda", 0)
    n = args.requests
    threads = min(16, os.cpu_count() or 1)
    wl = pysynth.Workload(3)
    batch = wl.batch(0, n, threads=threads)
    sample = wl.batch(n, 65536, threads=threads)  # (bench.py tunes on a sample disjoint from the timed batch)
    routes = pick_routes(sample.slice(0, 4096))
    assert len(routes) == 16, routes
    engines, create_s = {}, {}
    for name, make in (("plain", lambda: RuleEngine(wl.rules, wl.lists, wl.geoip)), ("routed", lambda: RuleEngine(wl.rules, wl.lists, wl.geoip, routes=routes)),
                       ("router", lambda: ServiceRouter(routes, wl.lists, wl.geoip)._engine)):
        t0 = time.time()
        engines[name] = make()
        create_s[name] = round(time.time() - t0, 3)
        engines[name].tune(sample)
        print(f"[routes_bench] engine {name}: created in {create_s[name]:.2f} s", file=sys.stderr)
    plain, routed, router = engines["plain"], engines["routed"], engines["router"]
    db = DeviceBatch(batch, dev)
    out = torch.empty((n, 2), dtype=torch.int32, device=dev)
    out2 = torch.empty((n, 2), dtype=torch.int32, device=dev)
    route = torch.full((n,), -2, dtype=torch.int32, device=dev)
    cnt = torch.zeros(4, dtype=torch.int64, device=dev)

    def step(config):
        if config == "a":
            plain.evaluate_device(db, out=out, counts=cnt)
        elif config == "b":
            routed.evaluate_device(db, out=out, counts=cnt)
        elif config == "c":
            routed.evaluate_device(db, out=out, counts=cnt, route=route)
        else:
            plain.evaluate_device(db, out=out, counts=cnt)
            router.evaluate_device(db, out=out2)

    def measure(config):
        used = {"a": [plain], "b": [routed], "c": [routed], "d": [plain, router]}[config]
        for e in used:
            e.set_profiling(1)
        for _ in range(args.warmup):
            step(config)
        torch.cuda.synchronize(dev)
        kernels = collections.defaultdict(list)
        for e in used:
            for name, ms, _ in e.kernel_times():
                kernels[name].append(ms)
            e.set_profiling(2)  # (as bench.py's timed steps: events around the streaming launch only)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(config)
        torch.cuda.synchronize(dev)
        el = time.perf_counter() - t0
        for e in used:
            e.kernel_times()
            e.set_profiling(0)
        per_step = {k: round(sum(v) / args.warmup, 4) for k, v in kernels.items()}  # (d: the two engines' launches of one name added up)
        return 1e3 * el / args.steps, per_step

    labels = {"a": "engine without routes", "b": "routed engine, no route output", "c": "routed engine, route output", "d": "engine without routes + ServiceRouter engine"}
    steps = {k: [] for k in labels}
    kern = {k: [] for k in labels}
    for _ in range(args.rounds):
        for config in labels:
            ms, per_step = measure(config)
            steps[config].append(round(ms, 4))
            kern[config].append(per_step)
    # the answers: the routed engine's routes are the ServiceRouter's, its verdicts the plain engine's
    step("c")
    torch.cuda.synchronize(dev)
    got_routes, got_out = route.cpu().numpy(), out.cpu().numpy().copy()
    step("d")
    torch.cuda.synchronize(dev)
    v = out2.cpu().numpy()
    action, rule = v[:, 0] & 0xFF, v[:, 1].astype(np.int64) & 0xFFFFFFFF
    want_routes = np.where(action == 1, rule, -1).astype(np.int32)
    mean = {k: statistics.fmean(x) for k, x in steps.items()}
    result = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "requests": n, "workload": "BASELINE.json configs[2]: synthetic 1k-rule WAF, device-resident batch, 16 routes",
              "routes": [[nm, e] for nm, e in routes], "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "engine_create_s": create_s,
              "device_rules": {"plain": plain.stats()["n_rules"], "routed": routed.stats()["n_rules"]}, "scan_passes": {"plain": plain.stats()["n_dfa_groups"], "routed": routed.stats()["n_dfa_groups"]},
              "ms_per_step": {k: {"what": labels[k], "rounds": steps[k], "mean": round(mean[k], 4)} for k in labels},
              "verdict_kernel_ms_warmup_mean": {k: [r.get("verdict") for r in kern[k]] for k in labels},
              "filter_kernel_ms_warmup_mean": {k: [r.get("filter") for r in kern[k]] for k in labels},
              "kernels_ms_warmup_mean_last_round": {k: kern[k][-1] for k in labels},
              "extra_bytes_written_per_step": 4 * n,
              "claims": {"c_less_than_d": bool(mean["c"] < mean["d"]), "c_over_d": round(mean["c"] / mean["d"], 4), "b_over_a": round(mean["b"] / mean["a"], 4), "c_over_a": round(mean["c"] / mean["a"], 4),
                         "a_spread_ms": round(max(steps["a"]) - min(steps["a"]), 4)},
              "routes_equal_service_router": bool((got_routes == want_routes).all()), "verdicts_equal_plain_engine": bool((got_out == out.cpu().numpy()).all()),
              "route_histogram": {str(k): int(c) for k, c in zip(*np.unique(got_routes, return_counts=True))}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
