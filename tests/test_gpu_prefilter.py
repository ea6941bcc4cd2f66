"""The bigram prefilter on the device: filter_kernel + compact_kernel + list-driven DFA passes, through the C ABI, against the CPU
oracle. The filter may only change WHICH requests a pass walks, never a verdict."""
import os
import random

import numpy as np
import pytest

import helpers as H
from oracle import pyoracle
from pingoo_amd import Request, RequestBatch, _abi
from pingoo_amd.engine import RuleEngine

pytestmark = pytest.mark.gpu
B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA


@pytest.mark.parametrize("seed", range(24))
def test_literal_heavy_fuzz_filtered_matches_oracle(seed):
    rng = random.Random(9100 + seed)
    rules = H.lit_rules(rng, rng.randint(3, 60))
    eng = RuleEngine(rules, {}, lds_table_budget=rng.choice([0, 0, 2048]))
    assert eng.stats()["n_filtered_groups"] >= 1
    n = rng.choice([1, 64, 65, 500, 2047, 2048, 2049, 5000])
    batch = RequestBatch.from_requests(H.lit_requests(rng, n))
    want = pyoracle.Oracle(rules, {}).evaluate(batch)
    got, counts = eng.evaluate_batch(batch, with_counts=True)
    H.assert_verdicts_equal(got, want, batch, f"seed {seed}")
    assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist()
    # the same rules with every pass walking every request
    plain = RuleEngine(rules, {}, flags=_abi.OPT_NO_PREFILTER)
    H.assert_verdicts_equal(plain.evaluate_batch(batch), want, batch, f"seed {seed}, no prefilter")
    # filters rebuilt from a traffic sample (heads, window choice, bucketing change): same verdicts
    eng.tune(RequestBatch.from_requests(H.lit_requests(rng, 400)))
    H.assert_verdicts_equal(eng.evaluate_batch(batch), want, batch, f"seed {seed}, tuned")
    eng.close()
    plain.close()


def test_heads_and_candidates_at_slab_and_chunk_boundaries():
    """Requests of every length around the 16/32-byte chunking, factors placed at the very start / end of a field and straddling
    chunk boundaries, head literals present / absent / truncated, across more than one slab (128 KiB of arena: csrc/kernels.h, kStreamSlab)."""
    rules = [("ua", '!http_request.user_agent.starts_with("Mozilla/") && http_request.path.contains("/.env")', [B]),
             ("exact", 'http_request.user_agent == "curl/8.5.0"', [CAP]),
             ("tail", 'http_request.url.ends_with("x9k2")', [B]),
             ("head", 'http_request.url.starts_with("/wp-admin")', [CAP]),
             ("mid", 'http_request.url.matches("(?i)union\\\\s+select")', [B])]
    reqs = []
    for k in range(0, 70):
        pad = "q" * k
        reqs += [Request(url=pad + "x9k2", path="/.env", user_agent="Mozilla/5.0", host="h"), Request(url=pad + "x9k", path=pad + "/.env", user_agent="Mozill", host="h"),
                 Request(url="/wp-admin" + pad, path="/" + pad, user_agent="curl/8.5.0", host="h"), Request(url="/wp-admi" + pad, path=pad, user_agent="curl/8.5.01", host="h"),
                 Request(url=pad + "UNION  SELECT" + pad, path="/a", user_agent="Mozilla/", host="h"), Request(url=pad + "union select", path="/.en" + pad + "v", user_agent="x", host="h")]
    reqs = reqs * 12  # > 2 slabs
    batch = RequestBatch.from_requests(reqs)
    eng = RuleEngine(rules)
    assert eng.stats()["n_filtered_groups"] >= 3
    want = pyoracle.Oracle(rules).evaluate(batch)
    H.assert_verdicts_equal(eng.evaluate_batch(batch), want, batch, "boundaries")
    assert len(set(want["action"].tolist())) == 3
    eng.close()


@pytest.mark.parametrize("parts", ["1", "4"])
def test_resolve_with_one_wave_and_four_waves_per_slab(parts, monkeypatch):
    """resolve_kernel<PARTS>: a slab's flagged chunks resolved by one wave or by four (each its quarter of the slab's chunks; the launch picks by
    the batch's slab count, PWAF_RESOLVE_PARTS forces it, read per launch). Same pairs, same verdicts: requests of every length around the
    chunking, requests that straddle quarter and slab boundaries (2 KiB - 40 KiB fields), a batch of several slabs."""
    monkeypatch.setenv("PWAF_RESOLVE_PARTS", parts)
    rng = random.Random(4400)
    rules = [("env", 'http_request.path.contains("/.env")', [B]), ("tail", 'http_request.url.ends_with("x9k2")', [CAP]),
             ("mid", 'http_request.url.matches("(?i)union\\\\s+select")', [B]), ("ua", 'http_request.user_agent.contains("sqlmap")', [B])]
    reqs = []
    for k in range(3000):
        pad = "q" * rng.choice([0, 1, 15, 16, 17, 31, 33, 200, 2047, 2048, 2049, 8191, 8192, 8193, 32767, 32768, 40000] if k % 50 == 0 else [0, 3, 16, 40, 90])
        kind = rng.randrange(6)
        url = [pad + "x9k2", pad + "x9k", "union select" + pad, pad + "UNION  SELECT", pad + "/index", "x9k2" + pad][kind]
        reqs.append(Request(url=url, path=["/.env", "/a" + pad[:300] + "/.env", "/.en", pad[:500]][rng.randrange(4)], user_agent=["Mozilla/5.0", "sqlmap/1.7", pad[:100] + "sqlmap"][rng.randrange(3)], host="h"))
    batch = RequestBatch.from_requests(reqs)
    eng = RuleEngine(rules)
    assert eng.stats()["n_filtered_groups"] >= 2
    want = pyoracle.Oracle(rules).evaluate(batch)
    H.assert_verdicts_equal(eng.evaluate_batch(batch), want, batch, f"parts {parts}")
    assert len(set(want["action"].tolist())) == 3
    eng.close()


def test_every_request_a_candidate_and_none():
    rules = [("a", 'http_request.path.contains("/.env")', [B]), ("b", 'http_request.url.contains("zz9")', [CAP])]
    eng = RuleEngine(rules)
    orc = pyoracle.Oracle(rules)
    for reqs in ([Request(path="/.env", url="/.env?zz9", host="h")] * 5000, [Request(path="/index.html", url="/index.html?a=1", host="h")] * 5000):
        batch = RequestBatch.from_requests(reqs)
        H.assert_verdicts_equal(eng.evaluate_batch(batch), orc.evaluate(batch), batch, "uniform batch")
    eng.close()


def test_synthetic_config3_tuned_and_untuned_at_100k():
    """Size-independent property at a size the oracle cannot check in seconds: the filtered engine, the tuned filtered engine and the
    engine without prefilters agree on every verdict of 100k requests; a 4000-request prefix is checked against the oracle."""
    from synth import pysynth

    w = pysynth.Workload(3)
    batch = w.batch(5_000_000, 100_000)
    eng = RuleEngine(w.rules, w.lists, w.geoip)
    plain = RuleEngine(w.rules, w.lists, w.geoip, flags=_abi.OPT_NO_PREFILTER)
    a = eng.evaluate_batch(batch)
    b = plain.evaluate_batch(batch)
    H.assert_verdicts_equal(a, b, batch, "filtered vs plain")
    eng.tune(w.batch(9_000_000, 8192))
    H.assert_verdicts_equal(eng.evaluate_batch(batch), b, batch, "tuned filtered vs plain")
    head = batch.slice(0, 4000)
    want = pyoracle.Oracle(w.rules, w.lists, w.geoip).evaluate(head, threads=8)
    H.assert_verdicts_equal(a[:4000], want, head, "oracle prefix")
    eng.close()
    plain.close()


def test_rule_set_without_string_predicates_at_one_million_requests():
    """No scan pass at all and both gates off (what ServiceRouter configures): the verdict kernel must not read hit records."""
    rules = [("port", "client.remote_port < 1024", [B]), ("cc", 'client.country == "XX"', [CAP])]
    eng = RuleEngine(rules, flags=_abi.OPT_NO_UA_GATE | _abi.OPT_NO_CAPTCHA_BYPASS)
    rng = np.random.default_rng(3)
    n = 1_000_000
    reqs = RequestBatch.from_requests([Request(host="h", remote_port=1)])
    big = reqs.tile(n) if hasattr(reqs, "tile") else None
    if big is None:
        pytest.skip("RequestBatch.tile not available")
    big.port[:] = rng.integers(0, 65536, n).astype(np.uint16)
    got = eng.evaluate_batch(big)
    assert (got["action"] == np.where(big.port < 1024, 1, 2)).all()
    eng.close()


def test_header_fields_extension_on_the_device():
    """EXTENSION (BASELINE.json configs[4]): http_request.headers["name"] columns — scan predicates, lengths, membership in the map,
    absent headers (= ""), a batch that carries none of the columns, and evaluate(Request)."""
    rules = [("k", 'http_request.headers["x-api-key"].contains("bad") || http_request.headers["x-api-key"].starts_with("tok_")', [B]),
             ("len", 'http_request.headers.accept.length() > 5 && "accept" in http_request.headers', [CAP]),
             ("empty", 'http_request.path.starts_with("/a") && http_request.headers["x-api-key"] == ""', [B]),
             ("re", 'http_request.headers["cookie"].matches("(?i)sid=[0-9a-f]{8};")', [CAP])]
    eng = RuleEngine(rules)
    assert sorted(eng.header_names) == ["accept", "cookie", "x-api-key"]
    orc = pyoracle.Oracle(rules)
    rng = random.Random(11)
    reqs = []
    for _ in range(3000):
        h = {}
        if rng.random() < 0.7:
            h["x-api-key"] = rng.choice(["", "tok_123", "verybadkey", "ok", "TOK_", "bad"])
        if rng.random() < 0.7:
            h["accept"] = rng.choice(["*/*", "text/html", "a", ""])
        if rng.random() < 0.5:
            h["cookie"] = rng.choice(["sid=0123abcd;x=1", "SID=DEADBEEF;", "sid=12345;", "theme=dark"])
        if rng.random() < 0.3:
            h["x-other"] = "ignored"
        reqs.append(Request(path=rng.choice(["/a", "/b", "/ab/c"]), host="h", headers=h or None))
    batch = RequestBatch.from_requests(reqs)
    want = orc.evaluate(batch)
    H.assert_verdicts_equal(eng.evaluate_batch(batch), want, batch, "headers")
    assert len(set(want["action"].tolist())) == 3
    # a batch without any header column: every header reads as ""
    bare = RequestBatch.from_requests([Request(path="/a", host="h"), Request(path="/b", host="h")])
    H.assert_verdicts_equal(eng.evaluate_batch(bare), orc.evaluate(bare), bare, "no header columns")
    assert int(eng.evaluate(Request(path="/a", host="h")).decision) == 1
    eng.close()


def test_config5_4096_rules_64_header_fields_benign_and_adversarial():
    """BASELINE.json configs[4] at a size the oracle finishes in seconds: 4096 rules over 5 + 64 string fields; the engine is tuned on
    benign traffic and evaluated on the adversarial stream (near misses of the rule literals, maximum-length fields)."""
    from synth import pysynth

    w = pysynth.Workload(5)
    eng = RuleEngine(w.rules, w.lists, w.geoip)
    assert len(eng.header_names) == 64 and eng.stats()["n_filtered_groups"] >= 60
    orc = pyoracle.Oracle(w.rules, w.lists, w.geoip)
    benign = w.batch(0, 6000)
    hostile = w.batch(100_000, 20000, adversarial=True)
    want_b = orc.evaluate(benign, threads=16)
    H.assert_verdicts_equal(eng.evaluate_batch(benign), want_b, benign, "config 5 benign")
    eng.tune(w.batch(1_000_000, 4096))
    want_h = orc.evaluate(hostile, threads=16)
    got_h, counts = eng.evaluate_batch(hostile, with_counts=True)
    H.assert_verdicts_equal(got_h, want_h, hostile, "config 5 adversarial, tuned on benign")
    assert counts.tolist() == np.bincount(want_h["action"], minlength=4).tolist()
    assert np.count_nonzero(want_h["action"]) > 0
    eng.close()


@pytest.mark.parametrize("seed", range(8))
def test_stride_two_filters_on_the_device(seed):
    """filter_kernel<., 2> (bigrams at the even bytes of the arena stream; fields start at either parity): forced through
    PWAF_OPT_FILTER_STRIDE2, then chosen per pass by tune; verdicts against the oracle, boundaries included."""
    rng = random.Random(9900 + seed)
    rules = H.lit_rules(rng, rng.randint(3, 60))
    eng = RuleEngine(rules, {}, flags=_abi.OPT_FILTER_STRIDE2)
    n = rng.choice([65, 500, 2049, 6000])
    reqs = H.lit_requests(rng, n)
    for k in range(0, 40):  # factors at every offset around the 16 / 64-byte chunking
        reqs.append(Request(url="q" * k + reqs[k % n].url, path="/" + "p" * k + reqs[(k + 1) % n].path, user_agent="u" * k + reqs[(k + 2) % n].user_agent, host=reqs[k % n].host))
    batch = RequestBatch.from_requests(reqs)
    want = pyoracle.Oracle(rules, {}).evaluate(batch)
    H.assert_verdicts_equal(eng.evaluate_batch(batch), want, batch, f"seed {seed}, stride 2")
    eng.tune(RequestBatch.from_requests(H.lit_requests(rng, 400)))
    H.assert_verdicts_equal(eng.evaluate_batch(batch), want, batch, f"seed {seed}, stride 2, tuned")
    eng.close()


def test_hot_prefix_factor_of_gated_gap_passes_after_tuning():
    """`^/api/.*foo.*bar` rules isolated into gated gap passes whose factor `\\A/api/` is hot in the tuning sample.
    A factor promoted to a filter head would only land in the hit record — requests outside the bigram candidates would never reach
    the gap passes and their rules would silently never match. Checked before and after tuning, against the oracle."""
    import test_prefilter as TP

    rules = TP._gated_head_rules()
    rng = random.Random(11)

    def reqs(n):
        out = []
        for _ in range(n):
            mid = "".join(rng.choice("abcxyz/") for _ in range(rng.randint(0, 12)))
            a, b = rng.choice([("foo", "bar"), ("select", "from"), ("aa", "bb"), ("cmd", "exe"), ("nope", "never")])
            pre = rng.choice(["/api/", "/api/", "/api/", "/ap/", "/x/api/"])
            out.append(Request(path=pre + mid + a + mid + (b if rng.random() < 0.7 else ""), url="/", host="h"))
        return out

    eng = RuleEngine(rules, {}, max_dfa_states=600)
    assert eng.stats()["n_gated_groups"] >= 1
    batch = RequestBatch.from_requests(reqs(6000))
    want = pyoracle.Oracle(rules, {}).evaluate(batch)
    assert len(set(want["action"].tolist())) >= 2
    H.assert_verdicts_equal(eng.evaluate_batch(batch), want, batch, "gated gap passes, untuned")
    eng.tune(RequestBatch.from_requests(reqs(2000)))
    H.assert_verdicts_equal(eng.evaluate_batch(batch), want, batch, "gated gap passes, tuned on traffic where the factor is hot")
    eng.close()


def test_config5_per_gpu_share_properties_at_6_25M():
    """BASELINE.json configs[4] at the size one GPU gets of it (50M requests over 8 GPUs = 6.25M per batch; 4096 rules over 5 + 64 string
    columns): too big for the oracle to check in seconds, so the size-independent properties of test_full_size_config2_properties:
    (1) a 3000-request slab checked bit-exactly against the oracle, (2) counters == histogram of the verdict array, (3) evaluating
    slabs separately (cut at non-aligned points) equals evaluating the whole, (4) tuning changes no verdict."""
    import torch
    from pingoo_amd.engine import DeviceBatch
    from synth import pysynth

    w = pysynth.Workload(5)
    eng = RuleEngine(w.rules, w.lists, w.geoip)
    n = 6_250_000
    batch = w.batch(0, n, threads=64)
    db = DeviceBatch(batch)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    out = eng.evaluate_device(db, counts=counts)
    eng.device_status()
    got = out.cpu().numpy().view(np.uint32)
    assert counts.cpu().tolist() == np.bincount(got[:, 0], minlength=4).tolist() and int(counts.sum()) == n
    frac = counts.cpu().numpy() / n
    assert 0.85 < frac[0] < 0.99 and frac[1] > 0.01, frac
    rng = np.random.default_rng(11)
    lo = int(rng.integers(0, n - 3000))
    sub = batch.slice(lo, lo + 3000)
    want = pyoracle.Oracle(w.rules, w.lists, w.geoip).evaluate(sub, threads=16)
    assert (got[lo:lo + 3000, 0] == want["action"]).all() and (got[lo:lo + 3000, 1] == want["rule_idx"]).all()
    cuts = [0, 2_000_001, 2_000_001 + 64 * 5000 + 13, n]
    for a, b in zip(cuts, cuts[1:]):
        part = eng.evaluate_device(DeviceBatch(batch.slice(a, b)))
        eng.device_status()
        p = part.cpu().numpy().view(np.uint32)
        assert (p == got[a:b]).all(), (a, b)
    eng.tune(w.batch(n, 32768, threads=64))
    out2 = eng.evaluate_device(db)
    eng.device_status()
    assert (out2.cpu().numpy().view(np.uint32) == got).all()
    eng.close()


@pytest.mark.parametrize("seed", range(10))
def test_confirm_tier_on_long_fields_on_the_device(seed):
    """confirm_kernel + the R-tier walk on long fields with rule tokens (whole, cut short, case-swapped) at their start, middle and
    end — several flagged chunks per candidate, chunk-bitmap words straddled — against the oracle, tuned or not, at both strides;
    and the engine without a confirm tier (PWAF_OPT_NO_CONFIRM: every candidate through the full DFA) returns the same."""
    from test_prefilter import _long_requests

    rng = random.Random(9300 + seed)
    rules = H.lit_rules(rng, rng.randint(3, 50))
    flags = _abi.OPT_FILTER_STRIDE2 if seed % 3 == 2 else 0
    eng = RuleEngine(rules, {}, flags=flags)
    n = rng.choice([64, 700, 3000, 9000])
    batch = RequestBatch.from_requests(_long_requests(rng, n))
    want = pyoracle.Oracle(rules, {}).evaluate(batch)
    H.assert_verdicts_equal(eng.evaluate_batch(batch), want, batch, f"seed {seed}")
    eng.tune(RequestBatch.from_requests(_long_requests(rng, 300)))
    H.assert_verdicts_equal(eng.evaluate_batch(batch), want, batch, f"seed {seed}, tuned")
    plain = RuleEngine(rules, {}, flags=flags | _abi.OPT_NO_CONFIRM)
    H.assert_verdicts_equal(plain.evaluate_batch(batch), want, batch, f"seed {seed}, no confirm tier")
    assert plain.stats()["n_confirm_literals"] == 0
    eng.close()
    plain.close()


def test_confirm_tier_on_the_synthetic_streams_against_the_full_dfa_walk():
    """The 1k-rule set at 200k requests, benign and hostile stream: the engine with the confirm tier returns what the engine that walks
    every candidate through the full DFA returns (both are compared with the oracle at smaller sizes by the other tests)."""
    from synth.pysynth import Workload

    wl = Workload(3)
    conf = RuleEngine(wl.rules, wl.lists, wl.geoip)
    plain = RuleEngine(wl.rules, wl.lists, wl.geoip, flags=_abi.OPT_NO_CONFIRM)
    assert conf.stats()["n_confirm_literals"] >= 400 and plain.stats()["n_confirm_literals"] == 0
    sample = wl.batch(5_000_000, 20000)
    conf.tune(sample)
    plain.tune(sample)
    for adversarial in (False, True):
        batch = wl.batch(0, 200_000, adversarial=adversarial)
        a, b = plain.evaluate_batch(batch), conf.evaluate_batch(batch)
        assert np.array_equal(a["action"], b["action"]) and np.array_equal(a["rule_idx"], b["rule_idx"]), adversarial
        assert len(set(a["action"].tolist())) >= 2
    plain.close()
    conf.close()


def test_every_request_a_candidate_at_one_million():
    """The hostile extreme at size: one million requests, every one a candidate of both filtered passes (near misses and hits mixed,
    long fields) — the lists are the whole batch, walked by lscan_async. Checked against the engine without prefilters (the
    streaming scan of every request) on all of it and against the oracle on a prefix."""
    rng = random.Random(424242)
    rules = [("a", 'http_request.path.contains("/.env")', [B]), ("b", 'http_request.url.contains("zz9=1") || http_request.url.matches("(?i)union\\\\s+select")', [CAP]),
             ("c", 'http_request.user_agent.contains("sqlmap")', [B])]
    pool = []
    for _ in range(32768):
        pad = H.rstr(rng, 5, 120, "abcdefxyz/.=-_%0123456789")
        path = "/" + pad + rng.choice(["/.env", "/.en", "/.envx", "/.e"]) + (H.rstr(rng, 0, 40, "abc/") if rng.random() < 0.5 else "")
        url = path + "?" + pad + rng.choice(["zz9=1", "zz9=", "zz9", "union select", "UNION  SELECT", "union+select", "unionselect"]) + H.rstr(rng, 0, 60, "abc&=")
        pool.append(Request(path=path[:250], url=url[:500], host="h", user_agent=rng.choice(["sqlmap/1.7", "sqlma", "Mozilla/5.0 sqlmap", "curl/8"]) + pad[:40]))
    reqs = [pool[i % 32768] for i in range(1_000_000)]
    batch = RequestBatch.from_requests(reqs)
    eng = RuleEngine(rules)
    plain = RuleEngine(rules, flags=_abi.OPT_NO_PREFILTER)
    a, counts = eng.evaluate_batch(batch, with_counts=True)
    b = plain.evaluate_batch(batch)
    assert np.array_equal(a["action"], b["action"]) and np.array_equal(a["rule_idx"], b["rule_idx"])
    assert counts.tolist() == np.bincount(a["action"], minlength=4).tolist() and len(set(a["action"].tolist())) >= 3
    # the oracle on 20 000 requests drawn from the WHOLE batch (the first 4 096 are one pass through the pool; positions deep
    # in the lists, at other arena alignments, are what lscan_async's later work items see)
    pick = np.sort(np.random.default_rng(7).choice(len(reqs), 20000, replace=False))
    sample = RequestBatch.from_requests([reqs[int(i)] for i in pick])
    want = pyoracle.Oracle(rules).evaluate(sample, threads=8)
    H.assert_verdicts_equal(a[pick], want, sample, "oracle on a random 20k sample")
    eng.close()
    plain.close()


def test_config3_adversarial_stream_tuned_on_benign_vs_oracle():
    """BASELINE.json configs[2] rule set (1024 rules, 200 regex, CIDR lists, GeoIP) on its HOSTILE stream (near misses of the rule
    literals, maximum-length fields): the engine is tuned on benign traffic — the attacker picks the traffic, not the tuning sample —
    and its verdicts on 100 000 hostile requests are the oracle's (mirror of the config-5 test above; VERDICT r3 weak #1b, r4 weak #1b)."""
    from synth import pysynth

    w = pysynth.Workload(3)
    eng = RuleEngine(w.rules, w.lists, w.geoip)
    orc = pyoracle.Oracle(w.rules, w.lists, w.geoip)
    hostile = w.batch(250_000, 100_000, adversarial=True)
    want = orc.evaluate(hostile, threads=os.cpu_count() or 16)
    got, counts = eng.evaluate_batch(hostile, with_counts=True)
    H.assert_verdicts_equal(got, want, hostile, "config 3 adversarial, untuned")
    eng.tune(w.batch(5_000_000, 32768))
    got, counts = eng.evaluate_batch(hostile, with_counts=True)
    H.assert_verdicts_equal(got, want, hostile, "config 3 adversarial, tuned on benign")
    assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist()
    assert np.count_nonzero(want["action"]) > 100
    eng.close()


def test_random_sample_of_the_10M_headline_batch_vs_oracle():
    """VERDICT r4 weak #1b: the headline workload itself — BASELINE.json configs[2], the 10M-request benign batch bench.py times, tuned
    as bench.py tunes — evaluated whole on the device, and 20 000 requests drawn at random from ALL of it (every arena position, every
    slab, lists deep into the batch) compared with the oracle; the action counters against the verdict array."""
    from synth import pysynth

    n = 10_000_000
    w = pysynth.Workload(3)
    batch = w.batch(0, n, threads=os.cpu_count() or 16)
    eng = RuleEngine(w.rules, w.lists, w.geoip)
    eng.tune(w.batch(n, 32768))
    got, counts = eng.evaluate_batch(batch, with_counts=True)
    assert counts.tolist() == np.bincount(got["action"], minlength=4).tolist() and counts.sum() == n
    pick = np.sort(np.random.default_rng(2025).choice(n, 20_000, replace=False))
    sample = batch.take(pick)
    want = pyoracle.Oracle(w.rules, w.lists, w.geoip).evaluate(sample, threads=os.cpu_count() or 16)
    H.assert_verdicts_equal(got[pick], want, sample, "random 20k sample of the 10M batch")
    assert np.count_nonzero(want["action"]) > 200
    eng.close()


def test_slab_view_whose_first_bytes_complete_a_window():
    """a batch that is a SLAB VIEW of a larger arena (offsets[0] != 0: a rank's share in pwaf_node_evaluate_batch, a
    caller splitting one parsed buffer). The 16-byte chunk that holds offsets[0] begins BEFORE the view's first request; resolve_kernel
    gave it no owner, so a literal completing inside the view's first < 16 bytes was never confirmed (fail-open), and chunks flagged in
    the bytes before offsets[0] left unwritten slots in the pair list. Every view start 1..40 (all residues mod 16) with the literal at
    every offset 0..14 of the first request, bytes BEFORE the view that would flag on their own, through pwaf_evaluate_batch and through
    a two-replica node whose second share starts off 16-byte alignment."""
    from pingoo_amd.engine import NodeEngine

    rules = [("env", 'http_request.path.contains("/.env")', [B]), ("tail", 'http_request.url.ends_with("x9k2")', [CAP]),
             ("sqli", 'http_request.url.matches("(?i)union\\\\s+select")', [B]), ("wp", 'http_request.path.starts_with("/wp-admin")', [CAP])]
    eng = RuleEngine(rules)
    orc = pyoracle.Oracle(rules)
    assert eng.stats()["n_filtered_groups"] >= 2
    for lead in range(1, 41):
        for at in (0, 1, 5, 9, 14):
            reqs = [Request(path="/.env" + "p" * (lead - 5) if lead >= 5 else "/" * lead, url="union select x9k2"[: max(lead, 1)].ljust(lead, "u"), host="h")]  # the bytes before the view
            reqs += [Request(path="q" * at + "/.env", url="z" * at + "UNION  select" + "x9k2", host="h"), Request(path="", url="", host="h"),
                     Request(path="/wp-admin/x", url="/wp-admin/x?a=1", host="h"), Request(path="/index.html", url="/index.html?x9k2", host="h")]
            reqs += [Request(path="/a/b" * (k % 7), url="/a/b?c=" + "d" * k, host="h") for k in range(60)]
            batch = RequestBatch.from_requests(reqs)
            assert int(batch.offsets[2][1]) == lead
            view = batch.view(1, batch.n)
            want = orc.evaluate(batch.slice(1, batch.n))
            assert want["action"][0] == B and want["rule_idx"][0] == 0
            H.assert_verdicts_equal(eng.evaluate_batch(view), want, batch.slice(1, batch.n), f"view at byte {lead}, literal at {at}")
    # the node's shares: 64-aligned request counts, arbitrary byte positions; the second share begins with the literal
    reqs = [Request(path="/x" * (k % 5) + "/i", url="/x?k=%d" % k, host="h") for k in range(64)]
    reqs += [Request(path="/.env", url="/.env", host="h")] + [Request(path="/y/%d" % k, url="/y?union+select", host="h") for k in range(63)]
    batch = RequestBatch.from_requests(reqs)
    assert int(batch.offsets[2][64]) % 16 != 0
    node = NodeEngine(rules, devices=[0, 0])
    want = orc.evaluate(batch)
    assert want["action"][64] == B
    H.assert_verdicts_equal(node.evaluate_batch(batch), want, batch, "node, second share off alignment")
    node.close()
    eng.close()


def test_saturated_stream_vs_oracle():
    """url / path / User-Agent filled to their caps with tokens that complete a window of the pass's own (tuned) filter
    tables without being a rule literal (tools/saturated.py: chosen with the numpy model of filter_kernel over the engine's tables) —
    nearly every 16-byte chunk is flagged and goes through the confirm tier (~55 pairs per request instead of 0.04): its worst case.
    Engine vs oracle, vs the engine without a confirm tier, and a mixed batch (saturated and benign requests interleaved by slabs)."""
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from pingoo_amd.engine import CompiledProgram
    from saturated import saturated_batch
    from synth import pysynth

    w = pysynth.Workload(3)
    sample = w.batch(5_000_000, 32768)
    model = CompiledProgram(w.rules, w.lists, w.geoip)
    model.tune(sample)
    sat, info = saturated_batch(w, model, 40_000, block=40_000)
    assert info["url"]["flagged_chunk_fraction_model"] > 0.9
    eng = RuleEngine(w.rules, w.lists, w.geoip)
    eng.tune(sample)
    orc = pyoracle.Oracle(w.rules, w.lists, w.geoip)
    want = orc.evaluate(sat, threads=os.cpu_count() or 16)
    H.assert_verdicts_equal(eng.evaluate_batch(sat), want, sat, "saturated, tuned")  # (round 6: the flagged passes are walked WHOLE — the flag-density switch)
    chunkwise = RuleEngine(w.rules, w.lists, w.geoip, flags=_abi.OPT_NO_DENSE_SWITCH)  # ... and confirmed chunk by chunk, as in round 5
    chunkwise.tune(sample)
    H.assert_verdicts_equal(chunkwise.evaluate_batch(sat), want, sat, "saturated, tuned, no dense switch")
    chunkwise.close()
    plain = RuleEngine(w.rules, w.lists, w.geoip, flags=_abi.OPT_NO_CONFIRM)
    H.assert_verdicts_equal(plain.evaluate_batch(sat), want, sat, "saturated, no confirm tier")
    plain.close()
    # an untuned engine (other tables: the tokens flag less, some passes stay sparse) and a batch that is half benign
    raw = RuleEngine(w.rules, w.lists, w.geoip)
    H.assert_verdicts_equal(raw.evaluate_batch(sat), want, sat, "saturated, untuned engine")
    raw.close()
    benign = w.batch(100_000, 40_000)
    mixed = RequestBatch.from_requests([])  # (built column by column below)
    both = [sat.slice(0, 20_000), benign.slice(0, 20_000), sat.slice(20_000, 40_000), benign.slice(20_000, 40_000)]
    data, offs = [], []
    for f in range(5):
        arena = np.concatenate([b.data[f][: int(b.offsets[f][-1])] for b in both] + [np.zeros(_abi.ARENA_PAD, np.uint8)])
        o, base = [np.zeros(1, np.uint32)], 0
        for b in both:
            o.append((b.offsets[f][1:].astype(np.int64) + base).astype(np.uint32))
            base += int(b.offsets[f][-1])
        data.append(arena)
        offs.append(np.concatenate(o))
    mixed = RequestBatch(data, offs, np.concatenate([b.ip for b in both]), np.concatenate([b.ip_is_v6 for b in both]), np.concatenate([b.port for b in both]),
                         np.concatenate([b.flags for b in both]))
    want_mixed = orc.evaluate(mixed, threads=os.cpu_count() or 16)
    H.assert_verdicts_equal(eng.evaluate_batch(mixed), want_mixed, mixed, "saturated and benign slabs mixed")
    # the switch is per pass and per batch: benign batches before and after a saturated one take the confirm tier again (same engine, same scratch)
    H.assert_verdicts_equal(eng.evaluate_batch(benign), orc.evaluate(benign, threads=os.cpu_count() or 16), benign, "benign after saturated")
    H.assert_verdicts_equal(eng.evaluate_batch(sat), want, sat, "saturated after benign")
    # a batch in which only ONE field is saturated (the other passes keep their confirm tier in the same launch)
    half = RequestBatch([sat.data[0], sat.data[1], benign.data[2], sat.data[3], benign.data[4]], [sat.offsets[0], sat.offsets[1], benign.offsets[2], sat.offsets[3], benign.offsets[4]],
                        sat.ip, sat.ip_is_v6, sat.port, sat.flags)
    H.assert_verdicts_equal(eng.evaluate_batch(half), orc.evaluate(half, threads=os.cpu_count() or 16), half, "url saturated, path and user-agent benign")
    eng.close()


def test_short_factors_at_stride_two_on_the_device():
    """Round 5: stride-2 windows of factors with fewer than four sampled bigrams reach one bigram beyond the factor on either side
    (csrc/filter.cpp, Model::best_window): the bigram behind a factor that ENDS its field pairs the field's last byte with the next
    request's first byte (or the arena's slack), the one in front of a factor that STARTS its field with the previous request's last
    byte. Literals of 3 to 7 bytes as contains / starts_with / ends_with / ==, fields that ARE the literal or hold it at their start /
    middle / end, packed back to back at every arena alignment (filler requests of 0..17 bytes in between), the first and the last
    request of the batch included — against the oracle, and against the engine without the confirm tier."""
    rng = random.Random(55)
    lits = ["../", "%00x", "/.env", "passwd", "<script"]
    rules = []
    for k, lit in enumerate(lits):
        rules += [(f"c{k}", f"http_request.path.contains({H.q(lit)})", [B]), (f"s{k}", f"http_request.url.starts_with({H.q(lit)})", [CAP]),
                  (f"e{k}", f"http_request.user_agent.ends_with({H.q(lit)})", [B]), (f"q{k}", f"http_request.host == {H.q(lit)}", [CAP])]
    reqs = []
    for lit in lits:
        for v in [lit, lit + "a", "a" + lit, "ab" + lit, lit + "ab", "a" + lit + "b", "abcdefghijklmnop" + lit, lit + "abcdefghijklmnopq", "xyz" + lit[:-1], lit[1:] + "xyz",
                  "abcdefghijklm" + lit + "nopqrstuvwxyz", lit[:-1] + "~", "~" + lit[1:]]:
            for pad in range(18):
                reqs.append(Request(host=v, url=v, path=v, method="GET", user_agent=v))
                if pad:
                    f = H.rstr(rng, pad, pad, "abcxyz0189")
                    reqs.append(Request(host=f, url=f, path=f, method="GET", user_agent=f))
    reqs = [Request(host=lits[0], url=lits[0], path=lits[0], method="GET", user_agent=lits[0])] + reqs + [Request(host=lits[1], url=lits[1], path=lits[1], method="GET", user_agent=lits[1])]
    batch = RequestBatch.from_requests(reqs)
    want = pyoracle.Oracle(rules, {}, flags=_abi.OPT_NO_UA_GATE).evaluate(batch)
    assert np.count_nonzero(want["action"]) > 500
    for extra in (0, _abi.OPT_NO_CONFIRM):
        eng = RuleEngine(rules, {}, flags=_abi.OPT_FILTER_STRIDE2 | _abi.OPT_NO_UA_GATE | extra)
        assert eng.stats()["n_filtered_groups"] == 4
        H.assert_verdicts_equal(eng.evaluate_batch(batch), want, batch, f"stride 2, flags {extra}")
        eng.close()
