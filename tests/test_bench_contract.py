"""The bench line's contract (the driver parses ONE JSON line; the judge recomputes the roofline from it) checked on the line committed
with the round's profiles — no GPU, no bench run: the keys the driver and the review rely on are there, the derived figures follow from
the raw ones, and the traffic the line quotes is the committed PMC file's."""
import glob
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def latest_line():
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_c3_10M_bench.json")))
    assert paths, "no committed bench line under profiles/"
    return paths[-1], json.loads(open(paths[-1]).read().strip().splitlines()[-1])


def test_committed_bench_line_keeps_the_contract():
    path, d = latest_line()
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, (path, k)
    assert d["unit"] == "requests/s" and d["higher_is_better"] is True and d["n_gpus"] == 1 and d["dtype"] == "u8" and d["data"] == "synthetic"
    assert d["vs_baseline"] is None  # BASELINE.md holds no published number for this metric
    assert "workload" in d["config"] and "configs[2]" in d["config"]["workload"] and "model" not in d["config"]
    n = d["config"]["requests_per_gpu"]
    assert abs(d["value"] - n / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6  # value = requests of the step / time of the step
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    # achieved = algorithmic bytes per launch / the launch's average duration (HIP events inside the timed region)
    assert abs(r["achieved"] - r["alg_bytes_per_launch"] / (r["avg_launch_ms"] / 1e3) / 1e9) / r["achieved"] < 1e-6
    assert r["avg_launch_ms"] * r["launches_per_step"] < d["ms_per_step"]  # the dominant kernel fits inside the step
    assert r["alg_bytes_per_step"] / (d["ms_per_step"] / 1e3) / 1e9 < r["peak"]
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "requests/s" and c["cores"] >= 1 and c["value"] > 0 and c["verdicts_match_gpu"] is True and "sample" in c


def test_quoted_traffic_is_the_committed_pmc_file():
    _, d = latest_line()
    r = d["roofline"]
    if r["traffic"] is None:
        return
    name = r["traffic_source"].split(" ")[0]
    tj = json.load(open(os.path.join(ROOT, name)))
    sk = [v for k, v in tj["kernels"].items() if "::filter_kernel<" in k]
    now = sum(sum(v["fetch_bytes"]) + sum(v["write_bytes"]) for v in sk) // max(1, sum(v["launches"] for v in sk))
    # (the line was written BEFORE the PMC passes of its own closing run replaced the file: the figure it quotes is the previous passes',
    # of the same kernel — the two agree to a fraction of a percent)
    assert sk and abs(r["traffic"] - now) / now < 0.01, (r["traffic"], now)
    assert 0.95 < r["traffic"] / r["alg_bytes_per_launch"] < 1.10  # no wasted re-reads in the streaming kernel (and it cannot read less than it must)


def test_dump_outputs_writes_the_verdicts_and_counters_as_float_arrays(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the last step's verdicts (a fixed seeded sample above DUMP_MAX_REQUESTS) and its four action counters,
    float32 / float64, exact for the rule_idx sentinels; the same sample on every call."""
    import numpy as np
    import torch

    import bench

    out = torch.arange(2 * 5000, dtype=torch.int32).reshape(5000, 2)
    out[:, 0] %= 4
    out[7, 1] = -1  # PWAF_RULE_NONE as the device writes it
    bench.dump_outputs(str(tmp_path / "all"), out[:10], [6, 2, 1, 1])
    assert (np.load(tmp_path / "all" / "verdict_action.npy") == out[:10, 0].numpy()).all()
    r = np.load(tmp_path / "all" / "verdict_rule_idx.npy")
    assert r.dtype == np.float32 and r[7] == -1 and (r == out[:10, 1].numpy()).all()
    c = np.load(tmp_path / "all" / "action_counts.npy")
    assert c.dtype == np.float64 and c.tolist() == [6, 2, 1, 1]
    monkeypatch.setattr(bench, "DUMP_MAX_REQUESTS", 1000)
    bench.dump_outputs(str(tmp_path / "a"), out, [0, 0, 0, 0])
    bench.dump_outputs(str(tmp_path / "b"), out, [0, 0, 0, 0])
    a, b = np.load(tmp_path / "a" / "verdict_rule_idx.npy"), np.load(tmp_path / "b" / "verdict_rule_idx.npy")
    assert a.shape == (1000,) and (a == b).all() and (np.diff(a) > 0).all()  # sorted indices, odd values 2k+1 unique per request


def test_bench_options_full_and_dump_outputs():
    """A plain run times the headline only; the side legs are behind --full. --steps is validated."""
    import subprocess
    import sys

    bench_py = os.path.join(ROOT, "bench.py")
    h = subprocess.run([sys.executable, bench_py, "--help"], capture_output=True, text=True, check=True).stdout
    assert "--full" in h and "--dump-outputs" in h
    r = subprocess.run([sys.executable, bench_py, "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--steps" in r.stderr
