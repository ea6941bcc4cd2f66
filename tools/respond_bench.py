#!/usr/bin/env python3
"""What pwaf_respond costs on one GPU (the memset, respond_classify_kernel, respond_base_kernel, respond_scatter_kernel); writes
profiles/respond.json. A figure, not a check: nothing asserts it.

--requests requests (default 1 Mi) of a listener's mix — most allowed and routed, some blocked, some sent to the captcha page, a few on
the captcha endpoints, a few with an invalid or undecided cookie — whose verdicts, statuses, routes and paths lie in device memory, and
three lists (VERIFY, INIT | VERIFY, BLOCKED), as the chain of INTEGRATION.md takes them. WARMUP warm-up calls, then WINDOWS windows of
CALLS calls each between two HIP events on the launch stream; per call: median, min and max over the windows. Beside it, in the same run
and the same way: a device-to-device copy of the bytes the call reads (verdicts, statuses, routes: 13 bytes per request). Every response,
count and list entry of the last call is compared with tests/respond_oracle.py. Refuses to run without a GPU.

usage: python tools/respond_bench.py [--requests 1048576] [--calls 50] [--windows 10] [--warmup 5] [--commit ID] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "respond.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("respond_bench.py measures the device call: no GPU is visible, nothing was measured")

    import respond_cases as RC
    import respond_oracle as O

    n = args.requests
    rng = np.random.RandomState(9)
    # (verdict, status, route, path) by weight
    mix = [(((O.ALLOW, O.RULE_NONE), O.ABSENT, 2, b"/index.html"), 700), (((O.ALLOW, O.RULE_NONE), O.VERIFIED, 0, b"/api/v1/items"), 150), (((O.ALLOW, O.RULE_NONE), O.ABSENT, O.ROUTE_NONE, b"/nowhere"), 20),
           (((O.BLOCK, 3), O.ABSENT, 2, b"/.env"), 50), (((O.BLOCK, O.RULE_UA_GATE), O.ABSENT, 2, b"/"), 20), (((O.CAPTCHA, 5), O.ABSENT, 1, b"/login"), 20),
           ((((O.BYPASS, O.RULE_CAPTCHA_ENDPOINT)), O.ABSENT, 2, O.VERIFY), 10), (((O.BYPASS, O.RULE_CAPTCHA_ENDPOINT), O.ABSENT, 2, O.INIT), 10),
           (((O.BYPASS, O.RULE_CAPTCHA_ENDPOINT), O.ABSENT, 2, O.ASSETS + b"/index.js"), 8), (((O.BYPASS, O.RULE_CAPTCHA_ENDPOINT), O.INVALID, 2, O.PREFIX + b"/x"), 2),
           (((O.ALLOW, O.RULE_NONE), O.INVALID, 2, b"/index.html"), 7), (((O.BLOCK, 3), O.UNDECIDED, 2, b"/.git/config"), 3)]
    weights = np.array([w for _, w in mix], dtype=np.float64)
    pick = rng.choice(len(mix), size=n, p=weights / weights.sum())
    verdicts, statuses, routes, paths = ([mix[k][0][j] for k in pick] for j in range(4))
    lists = [(O.CAPTCHA_VERIFY,), (O.CAPTCHA_INIT, O.CAPTCHA_VERIFY), (O.BLOCKED,)]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    call = RC.Call(RC.DeviceMem(dev), verdicts, statuses, routes, paths, lists)
    torch.cuda.synchronize(dev)

    def respond():
        rc = call.run(stream=stream.cuda_stream)
        assert rc == 0, rc

    src = torch.empty(13 * n, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.windows)]
        for a, b in ev:
            a.record(stream)
            for _ in range(args.calls):
                fn()
            b.record(stream)
        torch.cuda.synchronize(dev)
        ms = sorted(a.elapsed_time(b) / args.calls for a, b in ev)
        return {"windows": len(ms), "calls_per_window": args.calls, "median_ms": round(statistics.median(ms), 5), "min_ms": round(ms[0], 5), "max_ms": round(ms[-1], 5)}

    result = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "requests": n, "lists": len(lists), "warmup": args.warmup}
    t = timed(respond)
    got, want = call.results("respond_bench"), O.expect_batch(verdicts, statuses, routes, paths, lists)
    differing = sum(1 for g, w in zip(got[0], want[0]) if g != w) + sum(1 for g, w in zip(got[1], want[1]) if g != w) + sum(1 for g, w in zip(got[2], want[2]) if g != w)
    read_bytes, written_bytes = 13 * n + sum(len(p) for v, p in zip(verdicts, paths) if v[0] == O.BYPASS), 8 * n + 4 * sum(m for _, m in want[2])
    t.update(requests_per_s=round(n / (t["median_ms"] / 1e3)), bytes_read=read_bytes, bytes_written=written_bytes,
             gb_per_s=round((read_bytes + written_bytes) / (t["median_ms"] / 1e3) / 1e9, 1), counts=want[1], list_members=[m for _, m in want[2]],
             answers_differing_from_the_oracle=differing)
    result["respond"] = t
    tc = timed(lambda: dst.copy_(src, non_blocking=True))
    tc.update(bytes_copied=13 * n)
    result["device_copy_of_the_input_bytes"] = tc
    result["respond_over_copy"] = round(t["median_ms"] / tc["median_ms"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
