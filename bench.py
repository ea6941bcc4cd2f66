#!/usr/bin/env python3
"""bench.py — requests/s matched by the MI355X WAF batch matcher on BASELINE.json's workload.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

With N > 1 as a plain command it re-executes itself under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
--master-addr 127.0.0.1` (one rank per GPU); launched by torch.distributed.run it reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*.

A "step" is one pass of the hot path (filter / scan kernels, list scans, attribute and verdict kernels) over one batch of
synthetic requests that is already resident in HBM. Default workload: BASELINE.json configs[2] — 10M requests x 1024 rules
(600 literal + 200 regex + 124 CIDR lists + 100 GeoIP/ASN rules, 600k-prefix GeoIP table) — the configuration the metric
("1k-rule WAF") is quoted on; it fits one GPU. With N GPUs every rank evaluates its own slab of the same seeded stream (weak
scaling); the only collective is the RCCL all-reduce of the four action counters (`rccl_ranks` = the world size that all-reduce saw).
`--config 5` is BASELINE.json configs[4]: 4096 rules over 5 + 64 string fields (header-field extension), 1M-request batches,
with per-batch latency percentiles; the `--full` run carries a short leg of it as `config5`.

A plain run does only what the headline figure needs: generate, compile, tune, upload, W warmup + K timed steps, the result line.
Prints ONE JSON line on rank 0 (contract in the task statement) including
  roofline       HBM roofline of the dominant kernel (filter_kernel: the launch that streams the request bytes), from HIP events
                 recorded on the launch stream during the timed steps; algorithmic bytes per SURVEY.md §8(d) / DESIGN.md §6
`--full` adds the side measurements and checks, each a run of its own after the headline's timed steps:
  traffic_modes  the same engine UNTUNED (no traffic sample) and on the ADVERSARIAL variant of the stream (near misses of the rule
                 literals, maximum-length fields), next to the headline (tuned on a benign sample disjoint from the timed batch)
  config5        BASELINE.json configs[4] on this GPU: requests/s, per-batch latency p50 / p99, adversarial, untuned
  cpu_baseline   the CPU oracle ("port": a restatement of the reference's interpreter loop, NOT the Rust binary) timed on this
                 box's host cores over a bounded sample of the same request stream (rank 0, N=1 only)
  and the measured copy bandwidth, PCIe-inclusive host batches, the native micro-batcher, the residual-rule leg, the RCCL check.

`--dump-outputs DIR` writes what the timed path handed its caller in the last timed step (rank 0's slab): the four action counters
(`action_counts.npy`, float64) and each request's verdict (`verdict_action.npy`, `verdict_rule_idx.npy`, float32; rule_idx
sentinels as signed values, e.g. -1 = no rule). A batch of more than DUMP_MAX_REQUESTS requests is sampled: the sorted indices
np.random.default_rng(DUMP_SEED).choice(n, DUMP_MAX_REQUESTS, replace=False). Same arguments, same inputs: the stream is seeded.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~5.4-6.3 TB/s is the measured copy ceiling
DEFAULT_N = {1: 10_000, 2: 1_000_000, 3: 10_000_000, 5: 1_000_000}
TUNE_N = 32768
DUMP_MAX_REQUESTS = 4_000_000  # two float32 verdict columns: 32 MB
DUMP_SEED = 0


def effective_cpus():
    """CPUs this process can really use: the scheduler affinity mask, capped by the cgroup CPU quota (a container on a 256-thread host
    is usually granted a handful; `os.cpu_count()` reports the host's). Returns (count, how it was derived)."""
    try:
        n = len(os.sched_getaffinity(0))
        how = f"sched_getaffinity {n}"
    except AttributeError:
        n = os.cpu_count() or 1
        how = f"cpu_count {n}"
    quota = None
    try:  # cgroup v2
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = int(q) / int(per)
    except (OSError, ValueError):
        try:  # cgroup v1
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0 and per > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    if quota is not None:
        how += f", cgroup quota {quota:.2f}"
        n = max(1, min(n, int(quota + 0.999)))
    return n, how + f", os.cpu_count {os.cpu_count()}"


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(p / 100.0 * (len(xs) - 1))))]


class stdout_to_stderr:
    """RCCL prints a version banner on the C library's stdout when a communicator is created; the bench's stdout carries ONE JSON line.
    While this is active file descriptor 1 is stderr (C stdio flushed on the way out)."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        import ctypes

        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        return False


def self_launch(args_list, n):
    """`python bench.py --gpus N` as a plain command: become N ranks (one per GPU) under torch.distributed.run."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + args_list
    os.execv(sys.executable, cmd)


class Runner:
    """One engine + one HBM-resident batch: timed steps, per-kernel summaries."""

    def __init__(self, eng, n, dev, world, inflight):
        import torch

        self.torch, self.eng, self.n, self.dev, self.world = torch, eng, n, dev, world
        self.inflight = inflight
        n_streams = max(inflight, 2)
        self.outs = [torch.empty((n, 2), dtype=torch.int32, device=dev) for _ in range(n_streams)]
        self.cnts = [torch.zeros(4, dtype=torch.int64, device=dev) for _ in range(n_streams)]
        # one batch in flight: torch's current stream; several: streams of their own (the current stream is HIP's NULL stream, which
        # synchronises with every other blocking stream — no two batches would overlap)
        self.own_streams = [torch.cuda.Stream(dev) for _ in range(n_streams)]
        self.issue_ms = 0.0

    def barrier(self):
        if self.world > 1:
            self.torch.distributed.barrier()
        self.torch.cuda.synchronize(self.dev)

    def timed_run(self, db, steps, warmup, inflight=None, events=True):
        """W untimed + K timed steps over the resident batch `db`; returns (seconds, kernel times, action counters)."""
        from pingoo_amd import shard

        torch = self.torch
        inflight = inflight or self.inflight
        streams = [torch.cuda.current_stream(self.dev)] if inflight == 1 else self.own_streams

        # every step accumulates into a counter row of its own, zeroed before the run (a caller that hands each batch fresh counters): a
        # `zero_()` per step was one more 6 us launch in front of every batch of the timed region
        ring = torch.zeros((warmup + steps, 4), dtype=torch.int64, device=self.dev)
        self.barrier()

        def step(i, row):
            k = i % inflight
            with torch.cuda.stream(streams[k]):
                self.eng.evaluate_device(db, out=self.outs[k], counts=ring[row], stream=streams[k].cuda_stream)
                shard.allreduce_counts(ring[row])  # the path's only exchange: 4 counters over RCCL/xGMI

        # The WARMUP steps carry HIP events around EVERY kernel (the per-kernel table, `kernels_ms_per_step`); the TIMED steps only around the launch
        # that streams the request bytes — the dominant kernel the roofline is quoted on, measured live in the timed region as the contract asks.
        # (An event between two kernels keeps the second from starting while the first drains: ~20 us per step with a dozen launches, which
        # rounds 1-5 charged to the headline.) PWAF_BENCH_ALL_EVENTS=1 restores events around every kernel in the timed steps.
        want_events = events and not os.environ.get("PWAF_BENCH_NO_EVENTS")
        self.eng.set_profiling(1 if want_events else 0)
        for i in range(warmup):
            step(i, i)
        self.barrier()
        self.warm_kt, self.warm_steps = (self.eng.kernel_times(), warmup) if want_events and warmup else ([], 0)
        self.eng.set_profiling((1 if os.environ.get("PWAF_BENCH_ALL_EVENTS") else 2) if want_events else 0)
        self.barrier()
        t0 = time.perf_counter()
        for i in range(steps):
            step(i, warmup + i)
        self.issue_ms = 1e3 * (time.perf_counter() - t0) / steps  # host time to enqueue one step (the device runs behind it)
        self.barrier()
        elapsed = time.perf_counter() - t0
        if self.world > 1:
            t = torch.tensor([elapsed], dtype=torch.float64, device=self.dev)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            elapsed = float(t.item())
        kt = self.eng.kernel_times()
        self.eng.set_profiling(False)
        return elapsed, kt, ring[warmup + steps - 1].cpu().tolist()

    @staticmethod
    def stream_kernels(kt):
        """Launches that stream request bytes: filter_kernel (passes behind a bigram prefilter: arenas as flat byte streams) and
        scan_kernel (a DFA over every request). The engine reports each launch's algorithmic bytes — every byte of a streamed
        arena ONCE + its n+1 offsets. Returns {kernel: [ms, launches, bytes]} and the other kernels' ms."""
        kinds = {"filter_kernel<stride 1>": [0.0, 0, 0], "filter_kernel<stride 2>": [0.0, 0, 0], "filter_kernel<strides 1+2>": [0.0, 0, 0], "scan_kernel": [0.0, 0, 0]}
        other = {}
        for name, ms, tag in kt:
            # (ONE filter launch per batch; the engine's mark says which sampling strides its passes use)
            key = {"filter_s1": "filter_kernel<stride 1>", "filter_s2": "filter_kernel<stride 2>", "filter_mix": "filter_kernel<strides 1+2>"}.get(name, "scan_kernel" if name.startswith("scan_") else None)
            if key:
                kinds[key][0] += ms
                kinds[key][1] += 1
                kinds[key][2] += tag
            else:
                k2 = name.split("_x")[0]
                other[k2] = other.get(k2, 0.0) + ms
        return kinds, other

    def mode_summary(self, elapsed, kt, steps):
        kinds, _ = self.stream_kernels(kt)
        dom = max(kinds, key=lambda kk: kinds[kk][0])
        ms, _, nbytes = kinds[dom]
        ach = nbytes / (ms / 1e3) / 1e9 if ms > 0 else 0.0
        # per-kernel durations: from the warmup steps of the same run (events around every kernel there), the streaming launch from the timed steps
        per = {}
        if getattr(self, "warm_kt", None) and len(kt) < len(self.warm_kt) * steps // max(1, self.warm_steps):
            by_name = {}
            for name, kms, _ in self.warm_kt:
                by_name.setdefault(name, []).append(kms)
            for name, vals in by_name.items():  # (the MEDIAN launch x launches per step: a kernel's first launch carries its code object's load — 3.7 ms once for the hiprtc-built residual program)
                vals.sort()
                per[name] = vals[len(vals) // 2] * len(vals) / self.warm_steps
            for name in {n for n, _, _ in kt}:
                per[name] = 0.0
        for name, kms, _ in kt:
            per[name] = per.get(name, 0.0) + kms / steps
        return {"requests_per_s": self.n * self.world * steps / elapsed, "ms_per_step": 1e3 * elapsed / steps, "kernel": dom, "achieved_gbs": ach, "frac": ach / HBM_PEAK_GBS,
                "kernels_ms_per_step": {k: round(v, 4) for k, v in per.items()},
                "kernels_ms_source": "streaming launch: HIP events in the timed steps; the other kernels: HIP events in the warmup steps of the same run (median launch)"}

    def batch_latency(self, db, calls=40):
        """Per-batch latency: one synchronised device-resident call per batch."""
        torch = self.torch
        lat = []
        for _ in range(calls):
            torch.cuda.synchronize(self.dev)
            t0 = time.perf_counter()
            self.eng.evaluate_device(db, out=self.outs[0])
            torch.cuda.synchronize(self.dev)
            lat.append(1e3 * (time.perf_counter() - t0))
        return {"p50": pct(lat, 50), "p99": pct(lat, 99), "max": max(lat)}


def native_batcher_bench(eng, hb):
    """tools/batcher_bench (C++, 64 pthreads over pwaf_batcher_evaluate): what a native per-request host sees. None when the
    harness has not been built."""
    try:
        from pingoo_amd.engine import native_batcher_latency
    except ImportError:
        return None
    try:
        return native_batcher_latency(eng, hb)
    except Exception as exc:  # informational only
        print(f"native batcher benchmark failed: {exc}", file=sys.stderr)
        return None


def oracle_check(wl, host_prefix, gpu_out, cores):
    """The CPU oracle on a prefix of a timed batch against the verdicts the GPU wrote for it (the checker, never the thing measured)."""
    import numpy as np

    from oracle import pyoracle

    t0 = time.perf_counter()
    cpu_v = pyoracle.Oracle(wl.rules, wl.lists, wl.geoip).evaluate(host_prefix, threads=cores)
    dt = time.perf_counter() - t0
    gpu_v = gpu_out[: host_prefix.n].cpu().numpy().view(np.uint32)
    same = bool((gpu_v[:, 0] == cpu_v["action"]).all() and (gpu_v[:, 1] == cpu_v["rule_idx"]).all())
    return {"verdicts_match_gpu": same, "oracle_sample": f"first {host_prefix.n} requests of the timed batch, {cores} threads, {dt:.1f} s",
            "oracle_non_allow_in_sample": int(np.count_nonzero(cpu_v["action"]))}


def config5_leg(dev, threads, steps, verbose, check_adversarial=True):
    """BASELINE.json configs[4] on one GPU, short: 4096 rules over 5 + 64 string fields, 1M-request batches (the per-GPU batch of the
    50M-request / 8-GPU configuration is 6.25M: `--config 5 --requests 6250000` times that). Tuned on a benign sample."""
    import torch

    from pingoo_amd.engine import DeviceBatch, RuleEngine
    from synth import pysynth

    n = DEFAULT_N[5]
    t0 = time.time()
    wl = pysynth.Workload(5)
    eng = RuleEngine(wl.rules, wl.lists, wl.geoip)
    db = DeviceBatch(wl.batch(0, n, threads=threads), dev)
    r = Runner(eng, n, dev, 1, 1)
    out = {"workload": f"BASELINE.json configs[4] per GPU: {n} requests x {len(wl.rules)} rules, {len(eng.header_names)} header fields, benign stream; device-resident"}
    el, kt, _ = r.timed_run(db, max(2, steps // 2), 1)
    out["untuned"] = {k: v for k, v in r.mode_summary(el, kt, max(2, steps // 2)).items() if k in ("requests_per_s", "ms_per_step", "frac")}
    eng.tune(wl.batch(n, TUNE_N, threads=threads))
    el, kt, cnt = r.timed_run(db, steps, 2)
    head = r.mode_summary(el, kt, steps)
    out.update({"requests_per_s": head["requests_per_s"], "ms_per_step": head["ms_per_step"], "kernel": head["kernel"], "frac": head["frac"],
                "kernels_ms_per_step": head["kernels_ms_per_step"], "action_counts_allow_block_captcha_bypass": cnt})
    out["latency_ms"] = dict(r.batch_latency(db, 40), batch=n, calls=40)
    adv_host = wl.batch(0, n, threads=threads, adversarial=True)
    adv = DeviceBatch(adv_host, dev)
    el, kt, acnt = r.timed_run(adv, max(2, steps // 2), 1)
    a = r.mode_summary(el, kt, max(2, steps // 2))
    out["adversarial"] = {"requests_per_s": a["requests_per_s"], "ms_per_step": a["ms_per_step"], "frac": a["frac"], "kernels_ms_per_step": a["kernels_ms_per_step"],
                          "action_counts_allow_block_captcha_bypass": acnt}
    if check_adversarial:  # (before the latency calls: they write the same output buffer — with the same verdicts)
        out["adversarial"].update(oracle_check(wl, adv_host.slice(0, min(n, 12_000)), r.outs[0], effective_cpus()[0]))
    out["adversarial"]["latency_ms"] = r.batch_latency(adv, 20)
    del adv_host
    out["adversarial_over_benign"] = a["ms_per_step"] / head["ms_per_step"]
    out["setup_s"] = round(time.time() - t0, 1)
    del adv, db
    eng.close()
    torch.cuda.empty_cache()
    if verbose:
        print(f"[bench] config5 leg: {json.dumps(out)}", file=sys.stderr)
    return out


def slab_of(scaling, n_arg, rank, world):
    """(requests of this rank, requests of the whole job, index of this rank's first request in the global seeded stream).
    strong: BASELINE configs[3] as written — ONE batch of n_arg requests, rank r takes its 64-aligned slab (pingoo_amd/shard.py =
    pwaf_node_shard_bounds); weak: n_arg requests per GPU."""
    if scaling == "strong":
        from pingoo_amd import shard

        first, last = shard.shard_bounds(n_arg, rank, world)
        return last - first, n_arg, first
    return n_arg, n_arg * world, rank * n_arg


def dump_outputs(path, out, counts):
    """--dump-outputs: the verdicts of the last timed step (`out`, (n, 2) int32 on the device: action, rule_idx) — a fixed seeded
    sample of DUMP_MAX_REQUESTS of them when the batch is larger — and its four action counters, as .npy files under `path`."""
    import numpy as np
    import torch

    n = out.shape[0]
    if n > DUMP_MAX_REQUESTS:
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n, DUMP_MAX_REQUESTS, replace=False))
        v = out[torch.from_numpy(idx).to(out.device)].cpu().numpy()
    else:
        v = out.cpu().numpy()
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "verdict_action.npy"), v[:, 0].astype(np.float32))
    np.save(os.path.join(path, "verdict_rule_idx.npy"), v[:, 1].astype(np.float32))  # (sentinels 0xFFFFFFFx as int32: -1, -2, -3)
    np.save(os.path.join(path, "action_counts.npy"), np.asarray(counts, dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", type=int, default=3, help="synthetic config id (BASELINE.json configs[id-1]); default 3")
    ap.add_argument("--requests", type=int, default=0, help="requests per batch (default: the config's batch size): per GPU with --scaling weak, of the ONE batch all GPUs share with --scaling strong")
    ap.add_argument("--scaling", choices=["weak", "strong"], default=None,
                    help="strong (default when --gpus > 1): BASELINE configs[3] as written — ONE batch of --requests requests, split over the GPUs by shard_bounds "
                         "(64-aligned contiguous slabs); weak (default at one GPU): --requests requests PER GPU")
    ap.add_argument("--lds-budget", type=int, default=0)
    ap.add_argument("--engine-flags", type=lambda x: int(x, 0), default=0, help="extra pwaf_options.flags for A/B runs (e.g. 2048 = PWAF_OPT_DENSE_VERDICT: the round-4 column file); same verdicts")
    ap.add_argument("--adversarial", action="store_true", help="time the adversarial variant of the stream as the HEADLINE batch (the tuning sample stays benign)")
    ap.add_argument("--no-extra-modes", action="store_true", help="skip the untuned and adversarial side runs (traffic_modes)")
    ap.add_argument("--no-config5", action="store_true", help="skip the short BASELINE configs[4] leg of the --full run")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pcie", action="store_true", help="skip the host-batch (PCIe-inclusive) and micro-batcher measurements")
    ap.add_argument("--full", action="store_true", help="after the headline: the untuned / adversarial / saturated / two-in-flight runs, the config 5 leg, "
                                                        "the residual-rule leg, the copy-bandwidth probe, PCIe-inclusive and micro-batcher calls, the CPU baseline "
                                                        "and oracle checks, the RCCL single-rank check (a plain run times the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the verdicts and action counters of the last timed step as .npy files under DIR")
    ap.add_argument("--verbose", action="store_true", help="per-kernel timings on stderr")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--residual", type=int, default=None, help="also time the same workload with K extra rules outside the column compiler's subset (arithmetic on lengths / ports, "
                                                            "concatenation, lists of request values, orderings between fields), evaluated by their specialized device program "
                                                            "(DESIGN.md 3.5): `residual` object. Default: 8 with --full, none with --no-extra-modes or without --full; 0 skips the leg")
    ap.add_argument("--inflight", type=int, default=1, help="batches in flight: step i is issued on stream i mod INFLIGHT (pwaf_evaluate_device is re-entrant: every call takes "
                                                            "its own scratch context), so one batch's small latency-bound kernels run under the next batch's streaming kernels")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.gpus > 1 and "RANK" not in os.environ:
        self_launch(sys.argv[1:], args.gpus)  # does not return

    import numpy as np
    import torch

    from pingoo_amd import shard
    from pingoo_amd.engine import DeviceBatch, RuleEngine
    from synth import pysynth

    rank, world, local = shard.env_rank()
    args.gpus = world
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    if local >= torch.cuda.device_count():
        raise SystemExit(f"rank {rank}: local rank {local} has no GPU ({torch.cuda.device_count()} visible): --gpus {world} needs {world} GPUs on this node")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    with stdout_to_stderr():
        shard.init_process_group()
    # the world size the counters' all-reduce runs over: under torch.distributed.run a process group exists at every world size (1
    # included) and every step ends in one RCCL all-reduce; started plainly at N = 1 there is none during the timed steps (0 here) and
    # ONE all-reduce of the final counters runs after them (`rccl_single_rank_check` below)
    ones = torch.ones(1, dtype=torch.int64, device=dev)
    with stdout_to_stderr():  # (the first collective creates the communicator)
        shard.allreduce_counts(ones)
        torch.cuda.synchronize(dev)
    rccl_ranks = int(ones.item()) if shard.collective_world() else 0

    scaling = args.scaling or ("strong" if world > 1 else "weak")
    n_arg = args.requests or DEFAULT_N.get(args.config, 100_000)
    n, total, first = slab_of(scaling, n_arg, rank, world)
    if n == 0:
        raise SystemExit(f"rank {rank}: an empty slab ({total} requests over {world} GPUs)")
    threads = max(1, effective_cpus()[0] // world)
    extras = args.full and world == 1 and not args.no_extra_modes and not os.environ.get("PWAF_BENCH_NO_TUNE")

    def phase(msg):
        if args.verbose and rank == 0:
            print(f"[bench] {msg}", file=sys.stderr, flush=True)

    t0 = time.time()
    wl = pysynth.Workload(args.config)
    batch = wl.batch(first, n, threads=threads, adversarial=args.adversarial)  # this rank's slab of the global seeded request stream
    t_gen = time.time() - t0
    t0 = time.time()
    opts = {"lds_table_budget": args.lds_budget} if args.lds_budget else {}
    if args.engine_flags:
        opts["flags"] = args.engine_flags
    eng = RuleEngine(wl.rules, wl.lists, wl.geoip, **opts)
    t_compile = time.time() - t0
    stats = eng.stats()
    dbatch = DeviceBatch(batch, dev)
    inflight = max(1, min(args.inflight, 3))
    R = Runner(eng, n, dev, world, inflight)

    traffic_modes = {}
    tune_n = 0 if os.environ.get("PWAF_BENCH_NO_TUNE") else TUNE_N
    if extras:
        # the engine as created: default filter tables and BFS-order LDS rows, no traffic sample
        phase("untuned run")
        el, kt, _ = R.timed_run(dbatch, max(2, args.steps // 2), 1)
        traffic_modes["untuned_benign"] = R.mode_summary(el, kt, max(2, args.steps // 2))
    if tune_n:
        # profile-guided tables from a traffic sample DISJOINT from the timed batch (a deployment would sample live traffic): bigram
        # statistics and heads of the prefilters, LDS-resident DFA rows; verdicts do not depend on it. The sample is always BENIGN.
        phase("tune")
        t0 = time.time()
        # (PWAF_BENCH_TUNE_ADVERSARIAL: timing experiment — what tables fitted to the hostile stream would buy; never the reported mode)
        eng.tune(wl.batch(total + rank * tune_n, tune_n, threads=threads, adversarial=bool(os.environ.get("PWAF_BENCH_TUNE_ADVERSARIAL"))))
        t_compile += time.time() - t0
        if os.environ.get("PWAF_BENCH_RETUNE_ROWS_ADV"):
            # timing experiment (profiling build): which rows are LDS-resident re-ranked from a HOSTILE sample, prefilters untouched —
            # what an engine that adapted its table residency to the traffic it sees would reach; never the reported mode
            os.environ["PWAF_TUNE_ROWS_ONLY"] = "1"
            eng.tune(wl.batch(total + world * tune_n + rank * tune_n, tune_n, threads=threads, adversarial=True))
            del os.environ["PWAF_TUNE_ROWS_ONLY"]

    phase("headline run")
    elapsed, ktimes, final_counts = R.timed_run(dbatch, args.steps, args.warmup)
    value = total * args.steps / elapsed
    head = R.mode_summary(elapsed, ktimes, args.steps)
    head["host_enqueue_ms_per_step"] = round(R.issue_ms, 3)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, R.outs[(args.steps - 1) % inflight], final_counts)
    if args.full:
        headline_out = R.outs[0][: min(n, 1_000_000)].clone()  # verdicts of the headline batch (the side runs below overwrite the buffer)

    if extras and inflight == 1:
        # the same batch with TWO batches in flight (step i on stream i mod 2; pwaf_evaluate_device is re-entrant: every call takes its
        # own scratch context): one batch's small latency-bound kernels run under the next batch's streaming kernels. Throughput only —
        # per-kernel durations (and anything derived from them, like the roofline object) are quoted for one batch at a time.
        phase("two batches in flight")
        k2 = max(4, args.steps)
        el, kt, _ = R.timed_run(dbatch, k2, 2, inflight=2)
        traffic_modes["tuned_benign_two_batches_in_flight"] = {"requests_per_s": total * k2 / el, "ms_per_step": 1e3 * el / k2, "host_enqueue_ms_per_step": round(R.issue_ms, 3)}
    if extras and not args.adversarial:
        phase("adversarial run")
        adv_host = wl.batch(first, n, threads=threads, adversarial=True)
        adv = DeviceBatch(adv_host, dev)
        ka = max(2, args.steps // 2)
        el, kt, adv_counts = R.timed_run(adv, ka, 1)
        traffic_modes["adversarial_tuned_on_benign"] = dict(R.mode_summary(el, kt, ka), action_counts_allow_block_captcha_bypass=adv_counts)
        if rank == 0 and not args.no_cpu_baseline:
            # the hostile batch's verdicts against the CPU oracle too (only the benign headline was): a bounded prefix
            phase("adversarial oracle check")
            traffic_modes["adversarial_tuned_on_benign"].update(oracle_check(wl, adv_host.slice(0, min(n, 60_000)), R.outs[0], effective_cpus()[0]))
        del adv, adv_host
        if args.config == 3 and rank == 0:
            # SATURATED: url / path / User-Agent filled to their caps with tokens that complete a window of the pass's own
            # (tuned) filter tables without being a rule literal — nearly every 16-byte chunk goes to the confirm tier: its worst case
            phase("saturated run")
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            from pingoo_amd.engine import CompiledProgram
            from saturated import saturated_batch

            model = CompiledProgram(wl.rules, wl.lists, wl.geoip)
            model.tune(wl.batch(total + rank * tune_n, tune_n, threads=threads))  # (the same sample the engine was tuned on: the same tables)
            n_sat = min(n, 4_000_000)  # (a 500-byte url per request: the arena's 32-bit offsets hold 4M of them)
            sat_host, sat_info = saturated_batch(wl, model, n_sat)
            sat = DeviceBatch(sat_host, dev)
            Rs = Runner(eng, sat_host.n, dev, world, 1)
            ks = max(2, args.steps // 2)
            el, kt, sat_counts = Rs.timed_run(sat, ks, 1)
            traffic_modes["saturated"] = dict(Rs.mode_summary(el, kt, ks), requests=sat_host.n, bytes_per_request=round(sat_host.algorithmic_bytes() / sat_host.n, 1),
                                              flagged_chunks_model=sat_info, action_counts_allow_block_captcha_bypass=sat_counts)
            if not args.no_cpu_baseline:
                traffic_modes["saturated"].update(oracle_check(wl, sat_host.slice(0, min(sat_host.n, 20_000)), Rs.outs[0], effective_cpus()[0]))
            del sat, sat_host, Rs, model
    traffic_modes["tuned_benign" if not args.adversarial else "adversarial_tuned_on_benign (headline)"] = head

    rules_desc = {3: "1k-rule WAF", 5: "4096-rule bot-protection set, 64 header fields (extension)"}.get(args.config, f"{len(wl.rules)}-rule set")
    result = {
        "metric": f"requests/sec matched (whole node), {rules_desc}",
        "value": value,
        "unit": "requests/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1000.0 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": scaling,
        "requests_total": total,
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic",
        "rccl_ranks": rccl_ranks,
        "config": {
            "workload": f"BASELINE.json configs[{args.config - 1 if world == 1 or args.config != 3 else 3}]: "
                        + (f"{n} requests/GPU" if scaling == "weak" else f"ONE batch of {total} requests split over {world} GPU(s) ({n} on rank 0)") + f" x {len(wl.rules)} rules "
                        f"({stats['n_scan_atoms']} string/regex predicates in {stats['n_dfa_groups']} DFA passes, {stats['n_filtered_groups']} of them behind a bigram prefilter, "
                        f"{stats['n_ip_lists']} CIDR lists, {0 if wl.geoip is None else len(wl.geoip)} GeoIP prefixes, {len(eng.header_names)} header fields), "
                        f"seed 0x50494E47^{args.config}, {'adversarial' if args.adversarial else 'benign'} stream",
            "requests_per_gpu": n,
            "rules": len(wl.rules),
            "tuning": (f"tuned on {tune_n} {'ADVERSARIAL (experiment)' if os.environ.get('PWAF_BENCH_TUNE_ADVERSARIAL') else 'benign'} sample requests disjoint from the timed batch") if tune_n else "none (untuned)",
            "parallelism": f"requests sharded over {world} GPU(s), tables replicated, RCCL all-reduce of 4 counters",
            "batches_in_flight": inflight,
            "action_counts_allow_block_captcha_bypass": final_counts,
            "parity_note": "verdicts of the timed batch are checked against the CPU oracle on the cpu_baseline sample (a prefix of the batch), not on all of it: "
                           "the oracle evaluates ~14k requests/s",
        },
    }
    if not args.full:
        result["config"]["parity_note"] = "not oracle-checked in a plain run: --full checks a prefix of the timed batch against the CPU oracle"

    if rank == 0:
        kinds, _ = R.stream_kernels(ktimes)
        # the kernels that do not stream request bytes: per-step durations from the warmup steps' events (mode_summary), here as totals over the timed steps
        streaming_names = {name for name, _, _ in ktimes}
        other_ms = {}
        for name, ms_step in head["kernels_ms_per_step"].items():
            if name not in streaming_names and not name.startswith(("filter_", "scan_")):
                k2 = name.split("_x")[0]
                other_ms[k2] = other_ms.get(k2, 0.0) + ms_step * args.steps
        verdict_ms = other_ms.pop("verdict", 0.0)
        attr_ms = other_ms.pop("attr", 0.0) + other_ms.pop("ipres", 0.0)  # side stream: address lookups, then rows / transposes / comparisons
        dom = head["kernel"]
        scan_ms, n_scan_launches, scan_alg = kinds[dom]
        stream_ms = sum(v[0] for v in kinds.values())
        if args.verbose:
            per = {}
            for name, ms, tag in ktimes:
                per.setdefault(name, []).append(ms)
            for name, v in per.items():
                print(f"  {name:<24} avg {sum(v) / len(v):8.3f} ms  x{len(v)}", file=sys.stderr)
            print("  " + json.dumps(stats), file=sys.stderr)
        achieved = head["achieved_gbs"]
        pipeline_alg = dbatch.algorithmic_bytes * args.steps
        # HBM traffic cannot be counted from inside this process: it comes from the separate rocprofv3 --pmc passes over this very
        # command (tools/profile_round.sh), committed under profiles/ and only quoted for the workload they were measured on
        traffic, traffic_src = None, None
        for tname in ("r6_traffic.json", "r5_traffic.json", "r4_traffic.json", "r3_traffic.json"):
            tpath = os.path.join(ROOT, "profiles", tname)
            if traffic is not None or not (args.config == 3 and n == 10_000_000 and not args.adversarial and os.path.exists(tpath)):
                continue
            try:
                tj = json.load(open(tpath))
                want = ("::scan_kernel<", "") if dom == "scan_kernel" else ("::filter_kernel<", "")
                sk = [v for k, v in tj["kernels"].items() if want[0] in k and want[1] in k]  # one entry per template instantiation
                if not sk:
                    raise KeyError(dom)  # the committed passes predate this kernel: no figure rather than a wrong one
                traffic = sum(sum(v["fetch_bytes"]) + sum(v["write_bytes"]) for v in sk) // max(1, sum(v["launches"] for v in sk))
                traffic_src = f"profiles/{tname} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes; FETCH_SIZE factor {sk[0].get('fetch_factor', 2) if sk else '?'} for this kernel, see tools/pmc_traffic.py; taken at commit {tj.get('commit', '?')})"
            except Exception:  # a malformed profile file must not break the bench line
                traffic, traffic_src = None, None
        kernel_s = (stream_ms + verdict_ms + sum(other_ms.values())) / 1000.0  # (the attribute kernel runs beside these on a side stream)
        result["roofline"] = {
            "bound": "hbm",
            "kernel": dom,
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "frac_untuned": traffic_modes.get("untuned_benign", {}).get("frac"),
            "frac_adversarial": traffic_modes.get("adversarial_tuned_on_benign", {}).get("frac"),
            "traffic": traffic,  # HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (profiles/), or null
            "traffic_source": traffic_src,
            "alg_bytes_per_launch": scan_alg // max(1, n_scan_launches),
            "launches_per_step": n_scan_launches // max(1, args.steps),
            "avg_launch_ms": scan_ms / max(1, n_scan_launches),
            "alg_bytes_per_step": scan_alg // args.steps,
            "pipeline": {
                "alg_bytes_per_request": dbatch.algorithmic_bytes / n,
                "achieved": pipeline_alg / kernel_s / 1e9 if kernel_s > 0 else 0.0,
                "frac": (pipeline_alg / kernel_s / 1e9 / HBM_PEAK_GBS) if kernel_s > 0 else 0.0,
                "frac_of_step_wall_time": dbatch.algorithmic_bytes / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS,
                "streaming_launches": {k: {"ms_per_step": v[0] / args.steps, "alg_bytes_per_step": v[2] // args.steps,
                                           "achieved": (v[2] / (v[0] / 1e3) / 1e9) if v[0] > 0 else 0.0, "frac": (v[2] / (v[0] / 1e3) / 1e9 / HBM_PEAK_GBS) if v[0] > 0 else 0.0}
                                       for k, v in kinds.items() if v[1]},
                "streaming_frac": (sum(v[2] for v in kinds.values()) / (stream_ms / 1e3) / 1e9 / HBM_PEAK_GBS) if stream_ms > 0 else 0.0,
                "verdict_ms_per_step": verdict_ms / args.steps,
                "attr_ms_per_step_side_stream": attr_ms / args.steps,
                "other_ms_per_step": {k: v / args.steps for k, v in other_ms.items()},
            },
        }
        result["traffic_modes"] = traffic_modes
        # ---- SURVEY §8(d) extras: the part's measured copy bandwidth, bytes per clock and CU ----
        if args.full:
            try:
                src = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                dst.copy_(src)
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(8):
                    dst.copy_(src)
                e1.record()
                torch.cuda.synchronize(dev)
                copy_gbs = 8 * 2 * src.numel() / (e0.elapsed_time(e1) / 1e3) / 1e9  # read + write traffic of a device-to-device copy
                del src, dst
                props = torch.cuda.get_device_properties(dev)
                result["roofline"]["peak_measured_copy_gbs"] = copy_gbs
                result["roofline"]["frac_of_measured_copy"] = achieved / copy_gbs
                # (2.4 GHz: the MI355X peak engine clock of MI355X_MICROARCH.md; torch does not expose the running clock)
                result["roofline"]["bytes_per_clk_per_cu_at_2p4ghz"] = achieved * 1e9 / (props.multi_processor_count * 2.4e9)
            except Exception as exc:  # informational only
                result["roofline"]["peak_measured_copy_gbs"] = None
                print(f"copy-bandwidth probe failed: {exc}", file=sys.stderr)

        if world == 1 and args.full and args.config == 5:
            # per-batch latency (BASELINE.json configs[4]): one synchronised call per batch, device-resident
            phase("latency calls")
            result["latency_ms"] = {"batch": n, "calls": 40, "device_resident": R.batch_latency(dbatch, 40)}
        if world == 1 and args.full and not args.no_pcie:
            # host batch in, verdicts out through pwaf_evaluate_batch: H2D + kernels + D2H, on a bounded slice of the same batch
            phase("host-batch (PCIe-inclusive) calls")
            m = min(n, 1_000_000)
            hb = batch.slice(0, m) if m < n else batch
            eng.evaluate_batch(hb)
            lat = []
            hv = None
            for _ in range(6 if args.config != 5 else 12):
                t0 = time.perf_counter()
                hv = eng.evaluate_batch(hb)
                lat.append(time.perf_counter() - t0)
            gv = headline_out[:m].cpu().numpy().view(np.uint32)
            result["pcie_inclusive"] = {"value": m / pct(lat, 50), "unit": "requests/s",
                                        "sample": f"{m} requests from host memory, synchronous pwaf_evaluate_batch (H2D of ~{hb.algorithmic_bytes() / m:.0f} B/request, kernels, D2H of 8 B/request), median of {len(lat)} calls",
                                        "latency_ms": {"p50": 1e3 * pct(lat, 50), "p99": 1e3 * pct(lat, 99)},
                                        "verdicts_match_device_resident_run": bool((hv["action"] == gv[:, 0]).all() and (hv["rule_idx"] == gv[:, 1]).all())}
            if "latency_ms" in result:
                result["latency_ms"]["host_batch_pcie_inclusive"] = result["pcie_inclusive"]["latency_ms"]
            # the same host batches from several caller threads at once: the engine's per-call contexts (scratch, staging buffers,
            # stream each) let one batch's copies run under another's kernels
            import threading

            n_thr, per_thr = 3, 4

            def host_caller():
                for _ in range(per_thr):
                    eng.evaluate_batch(hb)
            th = [threading.Thread(target=host_caller) for _ in range(n_thr)]
            t0 = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join()
            dt = time.perf_counter() - t0
            result["pcie_inclusive"]["pipelined"] = {"value": n_thr * per_thr * m / dt, "unit": "requests/s", "sample": f"{n_thr} caller threads x {per_thr} synchronous calls of {m} requests each"}
            # deadline micro-batcher (the evaluate(Request) -> Action façade) driven by NATIVE caller threads (tools/batcher_bench.cpp:
            # 64 pthreads, 200 us deadline): per-request latency as a compiled host would see it
            phase("micro-batcher (native callers)")
            nb = native_batcher_bench(eng, hb)
            if nb is not None:
                result["batcher"] = nb
            # (last of the host-side legs: registering and unregistering 300 MB of the process's memory perturbs what runs after it)
            # the same call on PAGE-LOCKED columns and result array (pwaf_host_register / pwaf_host_alloc: what a listener that parses
            # requests into such arenas hands over): the copy engine reads the caller's bytes directly, validation runs under the copies
            from pingoo_amd.engine import PinnedVerdicts
            pv = PinnedVerdicts(m)
            hb.pin()
            eng.evaluate_batch(hb, out=pv.array)
            lat_p = []
            for _ in range(6 if args.config != 5 else 12):
                t0 = time.perf_counter()
                eng.evaluate_batch(hb, out=pv.array)
                lat_p.append(time.perf_counter() - t0)
            result["pcie_inclusive"]["page_locked"] = {"value": m / pct(lat_p, 50), "unit": "requests/s", "latency_ms": {"p50": 1e3 * pct(lat_p, 50), "p99": 1e3 * pct(lat_p, 99)},
                                                       "gb_per_s_in": hb.algorithmic_bytes() / pct(lat_p, 50) / 1e9,
                                                       "verdicts_match_device_resident_run": bool((pv.array["action"] == gv[:, 0]).all() and (pv.array["rule_idx"] == gv[:, 1]).all())}
            hb.unpin()
            pv.free()
        if args.residual is None:
            args.residual = 8 if (extras and args.config == 3) else 0
        if world == 1 and args.residual > 0:
            # the residual path: K rules no column form exists for, appended to the rule set — what a9's "any expression"
            # costs per batch on top of the column pipeline (it had never been timed)
            phase("residual rules")
            kinds = ["http_request.path.length() + 1 > http_request.url.length() && client.remote_port % 2 == 0",
                     '(http_request.host + ":" + http_request.method).matches("^[a-z]+:(GET|POST)$") && http_request.path + "x" == "/qx"',
                     '[http_request.host, "zz"].contains(http_request.path)',
                     'http_request.host < http_request.path && http_request.path < "c"',
                     "client.remote_port * 2 == 4242 && http_request.url.length() - http_request.path.length() > 300",
                     '(http_request.path.starts_with("/a") ? http_request.host : http_request.url).ends_with("!")',
                     "client.remote_port % 7 == 3 && client.remote_port / 7 == 1234",
                     '{"k": http_request.method}.k == "TRACE"']
            extra = [(f"residual_{k}", kinds[k % len(kinds)] + (f" && client.remote_port != {k}" if k >= len(kinds) else ""), [1]) for k in range(args.residual)]
            eng_r = RuleEngine(list(wl.rules) + extra, wl.lists, wl.geoip, **opts)
            n_res = sum("residual interpreter" in w for w in eng_r.program.warnings())
            if tune_n:
                eng_r.tune(wl.batch(total + rank * tune_n, tune_n, threads=threads))
            Rr = Runner(eng_r, n, dev, world, 1)
            el, kt, cnt_r = Rr.timed_run(dbatch, args.steps, 1)
            sm = Rr.mode_summary(el, kt, args.steps)
            result["residual"] = {"extra_rules": args.residual, "rules_on_the_interpreter": n_res, "ms_per_step": sm["ms_per_step"], "requests_per_s": sm["requests_per_s"],
                                  "mode": {0: "none", 1: "interpreted", 2: "specialized (hiprtc)"}[eng_r.residual_mode],
                                  "residual_kernel_ms_per_step": sum(v for k, v in sm["kernels_ms_per_step"].items() if k.startswith("residual")), "delta_ms_vs_headline": sm["ms_per_step"] - 1000.0 * elapsed / args.steps,
                                  "kernels_ms_per_step": sm["kernels_ms_per_step"], "action_counts_allow_block_captcha_bypass": cnt_r}
            eng_r.close()
            del Rr
        if world == 1 and args.config == 3 and not args.no_config5 and extras:
            phase("config 5 leg")
            # (the 10M-request batch and its scratch stay resident: config 5 adds ~6 GB)
            try:
                result["config5"] = config5_leg(dev, threads, max(4, args.steps), args.verbose, check_adversarial=not args.no_cpu_baseline)
            except Exception as exc:  # the headline line must survive a failure of the side leg
                result["config5"] = {"error": repr(exc)}
        # ---- CPU baseline: the oracle (port of the reference's per-request interpreter loop) on host cores ----
        if world == 1 and args.full and not args.no_cpu_baseline:
            from oracle import pyoracle

            phase("cpu baseline")
            cores, cores_how = effective_cpus()
            orc = pyoracle.Oracle(wl.rules, wl.lists, wl.geoip)
            # ONE thread first (single thread + all cores, core count stated): ~3 s of the same stream
            probe = batch.slice(0, min(n, 1000))
            t0 = time.perf_counter()
            orc.evaluate(probe, threads=1)
            rate1 = probe.n / max(1e-6, time.perf_counter() - t0)
            s1 = batch.slice(0, int(min(n, max(1000, rate1 * 3.0))))
            t0 = time.perf_counter()
            orc.evaluate(s1, threads=1)
            single = s1.n / max(1e-6, time.perf_counter() - t0)
            # ... then every CPU the process really has (threads_used = cores): a prefix of the timed batch sized for --cpu-seconds
            sample_n = int(min(n, len(headline_out), max(2000, single * cores * args.cpu_seconds)))
            sample = batch.slice(0, sample_n) if sample_n < n else batch
            t0 = time.perf_counter()
            cpu_v = orc.evaluate(sample, threads=cores)
            cpu_t = time.perf_counter() - t0
            gpu_v = headline_out[:sample_n].cpu().numpy().view(np.uint32)
            same = bool((gpu_v[:, 0] == cpu_v["action"]).all() and (gpu_v[:, 1] == cpu_v["rule_idx"]).all())
            allc = sample_n / cpu_t
            result["cpu_baseline"] = {
                "value": allc,
                "unit": "requests/s",
                "cores": cores,
                "threads_used": cores,
                "cores_source": cores_how,
                "single_thread_value": single,
                "per_core_value": allc / cores,
                "parallel_efficiency": allc / (cores * single),
                "measured_parallelism": allc / single,  # how many single-thread rates the all-thread run delivered: what the box really grants
                "kind": "port",
                "sample": f"first {sample_n} requests of the same batch, same rules; CPU restatement of the reference's interpreter loop "
                          f"(oracle/), {cores} threads on {cores} effective CPUs (single thread: {s1.n} requests); verdicts {'identical to' if same else 'DIFFERENT from'} the GPU's",
                "verdicts_match_gpu": same,
                # (what the figure is and is not: a like-for-like restatement — tree-walking evaluator, Pike-VM regex, linear CIDR
                # scans — not a tuned CPU engine; the reference's Rust interpreter with the lazy-DFA regex crate is faster per core)
                "note": "like-for-like port of the reference's per-request rule loop, not a tuned CPU engine: a reported baseline, not the target",
            }
            if allc < 0.7 * cores * single:
                result["cpu_baseline"]["scaling_note"] = (f"all-core rate is {allc / (cores * single):.2f} of cores x single-thread: the slabs are split statically "
                                                          "(the slowest thread ends the call) and the affinity mask / quota may count SMT siblings or CPUs shared with other containers")
            result["config"]["oracle_checked_fraction"] = sample_n / n
            result["config"]["parity_note"] = (f"{100.0 * sample_n / n:.2f} % of the timed batch ({sample_n} requests, a prefix) oracle-checked in this line; "
                                               "a 20k random sample of the same batch in tests/test_gpu_prefilter.py")
        result["timing_notes"] = {"generate_s": round(t_gen, 2), "compile_upload_tune_s": round(t_compile, 2)}
        if world == 1 and args.full and shard.collective_world() == 0:
            # a plain single process: the RCCL wiring exercised once, outside the timed region — a process group of one rank, the final
            # counters all-reduced (the sum over one rank is the counters themselves)
            try:
                with stdout_to_stderr():
                    shard.init_process_group(always=True)
                    t = torch.tensor(final_counts, dtype=torch.int64, device=dev)
                    shard.allreduce_counts(t)
                    torch.cuda.synchronize(dev)
                    result["rccl_single_rank_check"] = {"world": shard.collective_world(), "counters_unchanged": t.cpu().tolist() == final_counts}
                    torch.distributed.destroy_process_group()
            except Exception as exc:  # informational: the headline line must survive
                result["rccl_single_rank_check"] = {"error": repr(exc)}
        print(json.dumps(result))
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
