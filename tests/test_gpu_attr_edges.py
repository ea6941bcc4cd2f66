"""attr_kernel's comparison and short-literal atoms at their edges on the device (docs/attr_edges.md): the comparison loop (atoms in
registers, staged in LDS, re-read from global memory; the per-variable ballots; unsigned compares; the complement bit under the valid
mask), the short-literal loop (the unaligned 8-byte read, the length masks, exact against prefix), the class-row bits that answer
client.asn for engine-resolved records, the pair list filled to its stride, and the prefetch rotation over the turns of the persistent
grid. The cases are built by tests/attr_cases.py; tests/test_attr_edges_cpu.py asserts from the plan dumps that they land where they are
aimed and pins the model to the oracle without a device.

Hit legs: every atom stands alone in a rule without actions on a PWAF_OPT_RULE_HITS engine, so the hit list is one bit per (atom, request)
and helpers.assert_hits compares all of them with the model's matrix. Deciding legs: the same expressions with actions through the plain
call: verdicts and the four counters against the first rule of the model's matrix that takes effect. Every leg runs the base batch, its
prefixes of 1, 63, 64, 65, 129 and 257 requests, and the base batch again on the same engine. Every comparison is exact."""
import numpy as np
import pytest

import attr_cases as AC
import helpers as H
import pseudo_cases as PC
from pingoo_amd import _abi
from pingoo_amd.engine import RuleEngine

pytestmark = pytest.mark.gpu
POLARITY_LEGS = {"as built": 0, "eager": AC.EAGER}


def cap_for(n_rules, n):
    """room for every (rule, group) pair: the wrapper never fetches a list again, so every batch is evaluated once"""
    return n_rules * ((n + 63) // 64) + 8


def engine(c, rules, flags):
    eng = RuleEngine(rules, None, c.geoip(), flags=flags | c.flags)
    assert eng.address_tables()["packed"] == 1
    return eng


def check_observe(what, eng, batch, m, profiled=False):
    """the hit list against the model's matrix, bit for bit; rules without actions decide nothing"""
    if profiled:
        eng.set_profiling(1)
    got, hits, rule_hits, counts = eng.evaluate_batch_hits(batch, with_counts=True, cap=cap_for(m.shape[0], batch.n))
    if profiled:
        names = [k[0] for k in eng.kernel_times()]
        eng.set_profiling(0)
        assert names.count("attr") == 1, (what, names)
    H.assert_hits(what, hits, rule_hits, m)
    assert (got["action"] == 0).all() and (got["rule_idx"] == _abi.RULE_NONE).all() and counts.tolist() == [batch.n, 0, 0, 0], what


def check_deciding(what, eng, batch, want):
    got, counts = eng.evaluate_batch(batch, with_counts=True)
    H.assert_verdicts_equal(got, want, batch, what)
    assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist(), (what, counts.tolist())


def run_observe(c, flags=0, what=None):
    what = what or f"set {c.name}"
    eng = engine(c, c.observe(), AC.OBSERVE | flags)
    try:
        check_observe(what, eng, c.batch, c.M, profiled=True)
        for n in AC.SIZES:
            check_observe(f"{what}, batch of {n}", eng, c.batch.slice(0, n), c.M[:, :n])
        check_observe(f"{what}, again", eng, c.batch, c.M)
    finally:
        eng.close()


def run_deciding(c, flags=0, what=None):
    what = what or f"set {c.name}, deciding"
    eng = engine(c, c.deciding(), AC.NO_GATES | flags)
    try:
        check_deciding(what, eng, c.batch, c.expect())
        for n in AC.SIZES:
            check_deciding(f"{what}, batch of {n}", eng, c.batch.slice(0, n), c.expect(slice(0, n)))
        check_deciding(f"{what}, again", eng, c.batch, c.expect())
    finally:
        eng.close()


@pytest.mark.parametrize("name", AC.CMP_SETS)
def test_operators_neighbours_and_constants(name):
    """all six operators against 0, 1, 255, 256, 65535, 65536, 2^31 - 1, 2^31, 2^32 - 1, 2^32, -1 and the 64-bit extremes, the values
    c - 1, c and c + 1 around each: one length alone (the other four length columns are not loaded), all five, the port, the asn from the
    batch's column and from the engine's own records (class-row bits), one header's length, eight headers' and a ninth"""
    c = AC.case(name)
    run_observe(c)
    run_deciding(c)


@pytest.mark.parametrize("leg", list(POLARITY_LEGS))
def test_complemented_atoms_under_the_valid_mask(leg):
    """`>`, `>=` and `!=` alone in a rule are evaluated complemented (as built) or not (PWAF_OPT_EAGER_CMP): the same matrix. Request 0
    satisfies every complemented atom and the lanes beyond a batch's end reload request 0: at 1, 63, 65 and 129 requests a complement
    that is not masked sets bits beyond the batch and counts requests that are not there."""
    c = AC.case("POL")
    assert c.M[c.complemented, 0].all()
    run_observe(c, POLARITY_LEGS[leg], f"set POL, {leg}")
    run_deciding(c, POLARITY_LEGS[leg], f"set POL, {leg}, deciding")


@pytest.mark.parametrize("name", AC.CHUNK_SETS)
def test_comparison_chunks_in_registers_lds_and_global_memory(name):
    """exactly 1, 64, 65, 256, 257 and 300 eager atoms, rule k = atom k, every atom with its neighbours: atoms 0 ... 63 in registers,
    64 ... 255 staged in LDS (at another offset in the wide instantiation), 256 and up re-read per group; groups in which no atom holds, one
    holds in lane 0, 31, 32 or 63 alone, and in all 64 lanes"""
    c = AC.case(name)
    run_observe(c)
    run_deciding(c)


@pytest.mark.parametrize("name", AC.GEO_SETS)
def test_engine_resolved_asn_comparisons_are_class_row_bits(name):
    """32 comparisons (one word, SMALL), 33 (a second word, wide) and 128 (the limit) of client.asn against records at 0, 1, 2^31 - 1, 2^31,
    2^32 - 2 and 2^32 - 1; an address without a record, 127.0.0.1, a multicast address, ::1 and IPv6 clients against a table of IPv4
    prefixes read the default record {0, "XX"}, for which `asn < 5`, `<= 0` and `== 0` hold"""
    c = AC.case(name)
    run_observe(c)
    run_deciding(c)


def test_an_eager_atom_that_is_no_trigger_beside_two_lazy_variables():
    c = AC.case("Z")
    run_observe(c)
    run_observe(c, AC.EAGER, "set Z, eager")
    run_deciding(c)


@pytest.mark.parametrize("name", AC.SHORT_SETS)
def test_short_literals_of_every_length_on_every_field(name):
    """literals of 0 ... 8 bytes as `==`, `starts_with` and the two regex spellings on each field in turn; values one byte short (the next
    value supplies the byte), exact, one byte longer, nine and more bytes, differing in byte 0, 3, 4, 7 or 8 alone, with a NUL or 0xFF
    byte where the literal's padding lies. Request 0 at arena offset 0 is non-empty, and empty in the batch without it; the last request
    is empty (its 8-byte read lies in the pad), and the batch without it ends at the arena's last byte. S0+: two fields qualify, only
    the first is the short field; S0+n: PWAF_OPT_NO_PREFILTER, no short atoms, the same matrix."""
    c = AC.case(name)
    if name == "S0+n":
        assert (c.M == AC.case("S0+").M).all()
    run_observe(c)
    eng = engine(c, c.observe(), AC.OBSERVE)
    try:
        check_observe(f"set {name}, without request 0", eng, c.batch.slice(1, c.n), c.M[:, 1:])
        check_observe(f"set {name}, without the last request", eng, c.batch.slice(0, c.n - 1), c.M[:, :-1])
        check_observe(f"set {name}, requests 1 and 2", eng, c.batch.slice(1, 3), c.M[:, 1:3])
    finally:
        eng.close()
    run_deciding(c)


@pytest.mark.parametrize("name", AC.SHORT_CHUNK_SETS)
def test_short_literal_chunks_in_registers_lds_and_global_memory(name):
    """n_short of exactly 1, 64, 65, 128 and 129 with 8-byte edge literals at atoms 0, 63, 64, 127, 128 and the last"""
    c = AC.case(name)
    run_observe(c)
    run_deciding(c)


@pytest.mark.parametrize("name", ["X", "Xw"])
def test_pair_list_filled_to_its_stride(name):
    """memberships, comparisons and short literals together: in a full group every atom holds for somebody, so the group's slice of the
    pair list is exactly pair_stride long; another such group follows it, then an empty one"""
    c = AC.case(name)
    run_observe(c)
    run_deciding(c)


def test_turns_of_the_persistent_grid():
    """two strides and 96 groups: every wave meets, in consecutive turns, groups that differ lane by lane in every input the kernel
    prefetches — the lengths, the port, the asn, the short value's length and its first 8 bytes"""
    c = AC.case("T")
    eng = engine(c, c.observe(), AC.OBSERVE)
    try:
        stride = eng.compute_units() * AC.ATTR_GROUPS_PER_CU
        kinds = AC.turn_kinds(stride)
        assert (kinds[:-stride] != kinds[stride:]).all()
        idx = AC.turn_indices(kinds)
        batch, m = c.batch.take(idx), c.M[:, idx]
        got, hits, rule_hits = eng.evaluate_batch_hits(batch, cap=cap_for(len(c.atoms), batch.n))
        print(f"turns: {eng.compute_units()} compute units, stride {stride} groups, {batch.n} requests, {len(hits)} hit entries")
        PC.assert_hits_packed(f"set T, {batch.n} requests", hits, rule_hits, PC.packed(m), m.sum(axis=1))
        assert (got["action"] == 0).all()
        check_observe("set T, the base batch", eng, c.batch, c.M)
    finally:
        eng.close()
    eng = engine(c, c.deciding(), AC.NO_GATES)
    try:
        check_deciding("set T, turns, deciding", eng, batch, c.expect(m=m, verified=(batch.flags & _abi.FLAG_CAPTCHA_VERIFIED) != 0))
    finally:
        eng.close()
