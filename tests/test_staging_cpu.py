"""The staging layouts of the evaluate entry points on the CPU (csrc/staging.h: where pwaf_evaluate_batch packs a small host batch, where
pwaf_evaluate_records* put the unpacked columns and their bookkeeping, what the host checks of a HOST batch's columns):
tests/staging_host.cpp runs them as a plain g++ program and a second time under AddressSanitizer + UBSan. Every case runs in both builds."""
import functools
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "staging_host.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "pingoo_amd", "csrc", h) for h in ("staging.h", "records.h")] + [os.path.join(ROOT, "pingoo_amd", "csrc", "service.h"), os.path.join(ROOT, "include", "pwaf.h")]
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
PACK_MAX = 1 << 20  # csrc/staging.h: kPackMax
E_BATCH = -6        # include/pwaf.h: PWAF_E_BATCH
# the texts as pwaf_evaluate_batch has always set them
NOT_MONOTONE = "field offsets are not monotone"
BAD_COUNTRY = "country is not two letters A-Z (pingoo/geoip.rs:128-142)"


@functools.lru_cache(maxsize=None)
def tool(build):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "staging_host_" + build)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *FLAGS[build], "-I", os.path.join(ROOT, "include"), SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(params=["plain", "sanitized"])
def build(request):
    return request.param


def run(build, *args):
    r = subprocess.run([tool(build), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return [json.loads(line) for line in r.stdout.strip().splitlines()]


def test_every_plan_keeps_its_parts_aligned_disjoint_and_large_enough(build):
    (r,) = run(build, "invariants", 11, 6000)
    assert r["cases"] == 6000 and r["failures"] == 0, r
    assert 1000 < r["packable"] < 5000, "the random batches must fall on both sides of the packed block's limit"


def test_record_columns_lie_where_the_host_path_s_take_loop_put_them(build):
    (r,) = run(build, "record_cols", 12, 5000)
    assert r["cases"] == 5000 and r["failures"] == 0, r


def test_the_packed_block_s_three_limits(build):
    res = run(build, "packed_edges")
    assert len(res) == 8 * 5 and {(r["asn"], r["geo"], r["route"]) for r in res} == {(a, g, t) for a in (0, 1) for g in (0, 1) for t in (0, 1)}
    for r in res:
        assert r["packable"] == r["expected"], r
        want_need, want, placed = {"exact": (PACK_MAX, True, 7), "above": (PACK_MAX + 256, False, 7), "below": (PACK_MAX - 256, True, 7), "running": (None, False, 3),
                                   "slab": (None, False, 4)}[r["name"]]
        assert r["packable"] == want and r["placed"] == placed, r
        if want_need is not None:
            assert r["need"] == r["own_need"] == want_need, r
        elif r["name"] == "slab":
            assert r["need"] < PACK_MAX // 8, "the slab view is refused for its first offset alone"


def test_host_column_checks_keep_their_codes_and_texts(build):
    res = {r["name"]: (r["code"], r["text"]) for r in run(build, "host_columns")}
    ok, mono, cc = (0, ""), (E_BATCH, NOT_MONOTONE), (E_BATCH, BAD_COUNTRY)
    want = {"ends: ordered": ok, "full: ordered": ok, "full: ordered, no country": ok}
    for f in (0, 7):  # the first and the last present column
        want.update({f"full: column {f} pair {i}": mono for i in (0, 4, 8)})
        want.update({f"ends: column {f}": mono, f"full: column {f} end before begin": mono})
    for at in (0, 8):
        want.update({f"country {v} at {at}": code for v, code in (("@A", cc), ("A[", cc), ("AA", ok), ("ZZ", ok), ("fr", cc), ("Fr", cc), ("fR", cc))})
    assert res == want
