"""The two pseudo passes at their edges on the device (docs/pseudo_edges.md): fcmp_kernel (one request field against another, hit records),
residual_kernel (residual rules interpreted, hit records) and rvm_jit_kernel (the same rules specialized, one result word per request and
32 rules, transposed by the verdict kernels' step 2b). The cases are built by tests/pseudo_cases.py; tests/test_pseudo_edges_cpu.py
asserts their targets and pins the model to the oracle without a device.

Hit legs: every atom stands alone in a rule without actions on a PWAF_OPT_RULE_HITS engine, so the hit list is one bit per (atom, request)
and helpers.assert_hits compares all of them with the model's matrix — as built, with 8 entry slots, with the program tables in global
memory, and device-resident. Deciding legs: the same expressions with actions, forward and in reversed rule order (so that the late rules
decide somebody), on the column-file verdict kernels, which cannot report hits: verdicts and the four counters against the first rule of
the model's matrix that takes effect. Every leg runs the base batch, its prefixes of 1, 63, 64, 65, 129, 255, 256 and 257 requests, and the
base batch again. Residual sets run interpreted and specialized; the mode the engine reports is asserted.

Beyond one engine and one base batch: the per-rule error counters at the sizes where the last wave is partial and the erring rules stand
at result-word boundaries; 1 048 576 + 257 requests, which need the second round of the record-writing kernels' grid-stride loops; copies
of an all-true request whose chains outgrow the overflow pool (the synchronous call grows it and runs the batch again)."""
import numpy as np
import pytest

import helpers as H
import pseudo_cases as PC
from pingoo_amd import RequestBatch, _abi
from pingoo_amd.batch import RULE_HIT_DTYPE
from pingoo_amd.engine import DeviceBatch, RuleEngine
from test_gpu_residual import check_mode

pytestmark = pytest.mark.gpu
HIT_LEGS = {"as built": 0, "tiny slots": PC.TINY, "global tables": PC.GLOBAL}
MODES = {"specialized": 0, "interpreted": PC.NO_JIT}
FIELD_SETS, RESIDUAL_SETS = ("F32", "F33", "F9"), ("R74", "RE")
# (set, residual mode): the field sets' one lowered rule runs in both modes as well
SET_MODES = [("F32", "specialized")] + [(s, m) for s in ("F33", "F9", "R74", "RE", "M") for m in MODES]
PASS_KERNEL = {"specialized": "residual_jit", "interpreted": "residual"}


def cap_for(n_rules, n):
    """room for every (rule, group) pair: the wrapper never fetches a list again, so every batch is evaluated once"""
    return n_rules * ((n + 63) // 64) + 8


def kernels_of(name, mode):
    return (["fcmp"] if name in FIELD_SETS + ("M",) else []) + ([PASS_KERNEL[mode]] if name != "F32" else [])


def check_observe(what, eng, batch, m, kernels=()):
    """the hit list against the model's matrix, bit for bit; rules without actions decide nothing"""
    eng.set_profiling(1)
    got, hits, rule_hits, counts = eng.evaluate_batch_hits(batch, with_counts=True, cap=cap_for(m.shape[0], batch.n))
    names = [k[0] for k in eng.kernel_times()]
    eng.set_profiling(0)
    for k in kernels:
        assert names.count(k) == 1, (what, k, names)
    H.assert_hits(what, hits, rule_hits, m)
    assert (got["action"] == 0).all() and (got["rule_idx"] == _abi.RULE_NONE).all() and counts.tolist() == [batch.n, 0, 0, 0], what


def check_deciding(what, eng, batch, want):
    got, counts = eng.evaluate_batch(batch, with_counts=True)
    H.assert_verdicts_equal(got, want, batch, what)
    assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist(), what


@pytest.mark.parametrize("leg", list(HIT_LEGS))
@pytest.mark.parametrize("name,mode", SET_MODES)
def test_hits_of_every_atom(name, mode, leg):
    c = PC.case(name)
    PC.assert_targets(c)
    eng = RuleEngine(c.observe(), flags=PC.OBSERVE | HIT_LEGS[leg] | MODES[mode])
    try:
        check_mode(eng, mode)
        what = f"set {name}, {mode}, {leg}"
        check_observe(what, eng, c.batch, c.M, kernels_of(name, mode))
        for n in PC.SIZES:
            check_observe(f"{what}, batch of {n}", eng, c.batch.slice(0, n), c.M[:, :n])
        check_observe(f"{what}, again", eng, c.batch, c.M)
    finally:
        eng.close()


@pytest.mark.parametrize("leg", list(PC.COLUMN_FILE_LEGS))
@pytest.mark.parametrize("name,mode", SET_MODES)
def test_deciding_form_on_the_column_file_kernels(name, mode, leg):
    c = PC.case(name)
    c.assert_every_rule_decides()
    for reverse in (False, True):
        eng = RuleEngine(c.deciding(reverse), flags=PC.NO_GATES | PC.COLUMN_FILE_LEGS[leg] | MODES[mode])
        try:
            check_mode(eng, mode)
            what = f"set {name}, {mode}, {leg}, {'reversed' if reverse else 'forward'}"
            check_deciding(what, eng, c.batch, c.expect(reverse))
            for n in PC.SIZES:
                check_deciding(f"{what}, batch of {n}", eng, c.batch.slice(0, n), c.expect(reverse, slice(0, n)))
            check_deciding(f"{what}, again", eng, c.batch, c.expect(reverse))
        finally:
            eng.close()


@pytest.mark.parametrize("name,mode", [("F32", "specialized"), ("R74", "specialized"), ("R74", "interpreted")])
def test_device_resident_batch(name, mode):
    import torch

    c = PC.case(name)
    n_rules = len(c.exprs)
    eng = RuleEngine(c.observe(), flags=PC.OBSERVE | MODES[mode])
    try:
        db = DeviceBatch(c.batch)
        cap = cap_for(n_rules, c.n)
        d_hits = torch.zeros((cap, 16), dtype=torch.uint8, device="cuda:0")
        d_n, d_rule = torch.zeros(1, dtype=torch.int32, device="cuda:0"), torch.zeros(n_rules, dtype=torch.int64, device="cuda:0")
        out = eng.evaluate_device(db, hits=d_hits, n_hits=d_n, rule_hits=d_rule, hits_cap=cap)
        torch.cuda.synchronize()
        eng.device_status()
        k = int(d_n.item())
        assert k <= cap
        H.assert_hits(f"set {name}, {mode}, device-resident", d_hits.cpu().numpy().reshape(-1).view(RULE_HIT_DTYPE)[:k], d_rule.cpu().numpy(), c.M)
        got = out.cpu().numpy().view(np.uint32).reshape(-1, 2)
        assert (got[:, 0] & 0xFF == 0).all() and (got[:, 1] == _abi.RULE_NONE).all()
    finally:
        eng.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_error_counts_at_wave_and_word_edges(mode):
    """rule_errors counts, per rule, the requests whose evaluation ended in an execution error: a ballot inside the kernels' loops. The erring
    rules stand at residual indices 31, 32, 63, 64 and last; for one size of each residue class modulo 64 the only erring request is the
    batch's last one. After one evaluation and after two of the same batch."""
    n_rules = len(PC.RE)
    eng = RuleEngine(PC.case("RE").observe(), flags=PC.OBSERVE | MODES[mode])
    try:
        check_mode(eng, mode)
        total = np.zeros(n_rules, dtype=np.int64)
        assert eng.rule_errors(n_rules) == total.tolist()
        for n in PC.ERR_SIZES:
            batch, m, errors = PC.error_batch(n)
            for turn in (1, 2):
                check_observe(f"RE, {mode}, error batch of {n}, evaluation {turn}", eng, batch, m)
                total += np.array(errors)
                got = eng.rule_errors(n_rules)
                print(f"RE, {mode}, n {n}, evaluation {turn}: errors at {PC.RE_AT} = {[got[k] for k in PC.RE_AT]}, want {[int(total[k]) for k in PC.RE_AT]}")
                assert got == total.tolist(), (mode, n, turn, [(k, g, int(w)) for k, (g, w) in enumerate(zip(got, total)) if g != w])
        c = PC.case("RE")
        check_observe(f"RE, {mode}, the base batch", eng, c.batch, c.M)
        total += np.array(c.errors)
        assert eng.rule_errors(n_rules) == total.tolist()
    finally:
        eng.close()


@pytest.mark.parametrize("name,mode", [("F32", "specialized"), ("R8", "interpreted"), ("R8", "specialized")])
def test_second_round_of_the_grid_stride_loops(name, mode):
    """1 048 576 + 257 requests: launch_fcmp caps its grid at 4096 x 256 lanes and launch_residual at 8192 x 128, so the requests from
    1 048 576 on are evaluated by lanes that have stored a record before. Expected: the base batch's matrix, gathered."""
    exprs, base, m, idx = PC.second_round(name)
    rules = [(f"r{k}", e, []) for k, e in enumerate(exprs)]
    batch = base.take(idx)
    want = PC.packed(m[:, idx])
    counts = m[:, idx].sum(axis=1)
    eng = RuleEngine(rules, flags=PC.OBSERVE | MODES[mode])
    try:
        check_mode(eng, mode)
        eng.set_profiling(1)
        got, hits, rule_hits = eng.evaluate_batch_hits(batch, cap=cap_for(len(rules), batch.n))
        names = [k[0] for k in eng.kernel_times()]
        eng.set_profiling(0)
        # (twice where the chains of so many requests outgrow the pool of 8 n entries and the batch is run again)
        launches = names.count("fcmp" if name == "F32" else PASS_KERNEL[mode])
        print(f"{name}, {mode}: {batch.n} requests, {len(hits)} hit entries, the pass ran {launches} x")
        assert launches in (1, 2), names
        PC.assert_hits_packed(f"{name}, {mode}, {batch.n} requests", hits, rule_hits, want, counts)
        assert (got["action"] == 0).all()
    finally:
        eng.close()


@pytest.mark.parametrize("name,mode", [("F32", "specialized"), ("RE", "interpreted"), ("RE", "specialized")])
def test_pool_exhausted_by_a_pseudo_pass(name, mode):
    """copies of one request whose true atoms, one pool entry each, outgrow the overflow pool of max(2^20, 8 n) entries: the synchronous
    call grows the pool and runs the batch again; the matrix is the model's and every erring request is counted once. The specialized
    residual program writes result words and needs no pool (the engine exposes no pool figure: the arithmetic of pseudo_cases.pool_case
    stands in)."""
    exprs, req, col, n, errors = PC.pool_case(name)
    rules = [(f"r{k}", e, []) for k, e in enumerate(exprs)]
    batch = RequestBatch.from_requests([req]).take(np.zeros(n, dtype=np.int64))
    m = np.repeat(col[:, None], n, axis=1)
    eng = RuleEngine(rules, flags=PC.OBSERVE | MODES[mode])
    try:
        check_mode(eng, mode)
        eng.set_profiling(1)
        got, hits, rule_hits = eng.evaluate_batch_hits(batch, cap=cap_for(len(rules), n))
        names = [k[0] for k in eng.kernel_times()]
        eng.set_profiling(0)
        print(f"{name}, {mode}: {n} requests x {int(col.sum())} true atoms, launches {names.count('verdict')} x verdict")
        # the launch list is what the engine shows of the pool: a batch that exhausted it runs twice, result words need none
        assert names.count("verdict") == (1 if (name, mode) == ("RE", "specialized") else 2), names
        PC.assert_hits_packed(f"{name}, {mode}, {n} copies", hits, rule_hits, PC.packed(m), m.sum(axis=1))
        assert eng.rule_errors(len(rules)) == errors
        # and once more on the grown pool
        got, hits, rule_hits = eng.evaluate_batch_hits(batch, cap=cap_for(len(rules), n))
        PC.assert_hits_packed(f"{name}, {mode}, {n} copies, again", hits, rule_hits, PC.packed(m), m.sum(axis=1))
        assert eng.rule_errors(len(rules)) == [2 * e for e in errors]
    finally:
        eng.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_lowered_field_rules_beside_the_field_pass(mode):
    """F33 (the 33rd predicate) and F9 (the 9th field): the lowered rule's bits are the model's in both residual modes and the field atoms
    beside it are F32's, bit for bit, from the same batch"""
    base = PC.case("F32")
    for name, kept in (("F33", 32), ("F9", 31)):
        c = PC.case(name)
        assert (c.M[:kept] == base.M[:kept]).all() and c.M[-1].any() and not c.M[-1].all()
        eng = RuleEngine(c.observe(), flags=PC.OBSERVE | MODES[mode])
        try:
            check_mode(eng, mode)
            assert sum("residual interpreter" in w for w in eng.program.warnings()) == 1
            check_observe(f"set {name}, {mode}", eng, c.batch, c.M, ["fcmp", PASS_KERNEL[mode]])
        finally:
            eng.close()
