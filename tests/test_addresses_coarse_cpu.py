"""The coarse level of the IPv4 lookup table on the CPU (no device): csrc/dirtable.h — the header pwaf_engine_create calls — builds it
from a flat table; tests/dirtable_coarse_host.cpp checks every coarse bit against the table, walks ALL 2^24 /24s through a scalar
restatement of ipres_kernel<.., COARSE>'s three levels and says where each lookup ends. The tables come from the brute-force reference
(tests/lpm_reference.py) over the shapes of tests/coarse_cases.py and tests/address_cases.py; every shape asserts the count of lookups
that end at each level, worked out here from the table alone, so a shape that does not produce its path fails."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import address_cases as AC
import coarse_cases as CC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
SRC = os.path.join(HERE, "dirtable_coarse_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "pingoo_amd", "csrc", "dirtable.h")]
KIB = 1024
_FLAT = {}


def flat(name):
    """the tables, computed once and left unchanged"""
    if name not in _FLAT:
        if name == "sparse":
            f = CC.flat_from_prefixes(CC.sparse_geo_prefixes(), CC.sparse_lists())
        elif name == "dense":
            f = CC.flat_from_prefixes(CC.dense_geo_prefixes())
        elif name == "quarters":
            f = CC.flat_from_prefixes(CC.quarters_geo_prefixes())
        elif name == "common":
            g, l = CC.common_not_zero()
            f = CC.flat_from_prefixes(g, l)
        else:
            f = AC.summary_flat(int(name[1:]))
        f.setflags(write=False)
        _FLAT[name] = f
    return _FLAT[name]


def tool():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "dirtable_coarse_host")
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", SRC, "-o", out], check=True)
    return out


def run(tmp_path, table, budget=None, no_summary=False, queries=()):
    """-> (stats, coarse words, [(entry, level)] per query); budget None = compress()'s default argument"""
    fin, fout = str(tmp_path / "c.in"), str(tmp_path / "c.out")
    q = np.asarray(queries, dtype="<u4")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4I", 0x43524944, (1 if no_summary else 0) | (2 if budget is None else 0), budget or 0, len(q)))
        f.write(np.ascontiguousarray(table, dtype="<u4").tobytes())
        f.write(q.tobytes())
    r = subprocess.run([tool(), fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    stats = json.loads(r.stdout)
    out = np.fromfile(fout, dtype="<u4")
    os.remove(fin)
    os.remove(fout)
    n_c = stats["coarse_bytes"] // 4
    assert stats["out_of_range"] == 0 and stats["lookup_mismatch"] == 0 and stats["bit_mismatch"] == 0, stats
    return stats, out[:n_c], out[n_c:].reshape(-1, 2)


def expected_ends(table, common, shift, coarse_shift):
    """lookups (one per /24) that end at the coarse bit, at the summary bit, in the table — from the table alone"""
    other = table != np.uint32(common)
    in_sum = other.reshape(-1, 1 << shift).any(axis=1).repeat(1 << shift)
    if coarse_shift is None:
        return 0, int((~in_sum).sum()), int(in_sum.sum())
    in_coarse = other.reshape(-1, 1 << coarse_shift).any(axis=1).repeat(1 << coarse_shift)
    return int((~in_coarse).sum()), int((in_coarse & ~in_sum).sum()), int(in_sum.sum())


@pytest.mark.parametrize("budget,cs", [(None, 5), (64 * KIB, 5), (32 * KIB, 6), (64 * KIB - 1, 6), (16 * KIB, 7)])
def test_sparse_table_every_bit_every_24_and_the_block_edges(tmp_path, budget, cs):
    t = flat("sparse")
    q = CC.edge_24s(cs)
    stats, coarse, res = run(tmp_path, t, budget, queries=q)
    assert stats["has_summary"] == 1 and stats["common"] == 0 and stats["shift"] == 4, stats
    assert stats["has_coarse"] == 1 and stats["coarse_shift"] == cs and stats["coarse_bytes"] == (1 << 21) >> cs, stats
    # the bitmap against numpy's own pass over the table (the harness made the same pass in C++: bit_mismatch)
    want_bits = (t != 0).reshape(-1, 1 << cs).any(axis=1)
    got_bits = ((coarse[np.arange(len(want_bits)) >> 5] >> (np.arange(len(want_bits)) & 31).astype(np.uint32)) & 1).astype(bool)
    assert (got_bits == want_bits).all() and stats["coarse_set"] == int(want_bits.sum())
    assert stats["coarse_set"] * 2 <= len(want_bits)
    # the named blocks are what their names say
    blk = lambda x: x >> cs
    assert not want_bits[blk(CC.CLEAR_24)] and want_bits[blk(CC.SET_24)] and want_bits[0] and want_bits[-1]
    assert want_bits[blk(CC.ISOLATED_24)] and not want_bits[blk(CC.ISOLATED_24) - 1] and not want_bits[blk(CC.ISOLATED_24) + 1]
    assert want_bits[blk(CC.LOOPBACK_SET_24)] and not want_bits[blk(CC.LOOPBACK_CLEAR_24)] and want_bits[blk(CC.MULTICAST_SET_24)] and not want_bits[blk(CC.MULTICAST_CLEAR_24)]
    # first and last /24 of those blocks: the entry, and the level the lookup ends at
    assert (res[:, 0] == t[q]).all()
    sum_bits = (t != 0).reshape(-1, 16).any(axis=1)
    want_level = [0 if not want_bits[x >> cs] else 1 if not sum_bits[x >> 4] else 2 for x in q]
    assert res[:, 1].tolist() == want_level and set(want_level) == {0, 1, 2}
    ends = expected_ends(t, 0, 4, cs)
    assert (stats["ends_coarse"], stats["ends_summary"], stats["ends_table"]) == ends and all(e > 0 for e in ends), (stats, ends)
    assert stats["ends_coarse"] > 0.9 * (1 << 24)


def test_no_level_without_a_budget(tmp_path):
    t = flat("sparse")
    stats, coarse, _ = run(tmp_path, t, 0)
    assert stats["has_summary"] == 1 and stats["has_coarse"] == 0 and stats["coarse_shift"] == 0 and len(coarse) == 0
    assert (stats["ends_coarse"], stats["ends_summary"], stats["ends_table"]) == expected_ends(t, 0, 4, None)
    stats, _, _ = run(tmp_path, t, 100)  # smaller than the bitmap of the coarsest shift
    assert stats["has_summary"] == 1 and stats["has_coarse"] == 0


def test_level_absent_when_more_than_half_of_the_coarse_blocks_are_set(tmp_path):
    t = flat("dense")
    for budget in (None, 32 * KIB):
        stats, _, _ = run(tmp_path, t, budget)
        assert stats["has_summary"] == 1 and stats["shift"] == 2 and stats["has_coarse"] == 0 and stats["coarse_shift"] == 0, stats
        assert (stats["ends_coarse"], stats["ends_summary"], stats["ends_table"]) == expected_ends(t, 0, 2, None)
    assert int((t != 0).reshape(-1, 32).any(axis=1).sum()) * 2 > 1 << 19
    # the summary shapes of tests/address_cases.py: blocks of 2^s /24s alternate over 60 % of the space, so 60 % of the /19s are set
    for s in (0, 4):
        t = flat(f"s{s}")
        stats, _, _ = run(tmp_path, t, None)
        assert stats["has_summary"] == 1 and stats["shift"] == s and stats["has_coarse"] == 0, stats


def test_level_absent_when_no_summary_was_chosen_or_none_is_asked_for(tmp_path):
    stats, _, _ = run(tmp_path, flat("quarters"), None)
    assert stats["has_summary"] == 0 and stats["has_coarse"] == 0 and stats["ends_table"] == 1 << 24, stats
    stats, _, _ = run(tmp_path, flat("sparse"), None, no_summary=True)
    assert stats["has_summary"] == 0 and stats["has_coarse"] == 0 and stats["ends_table"] == 1 << 24, stats


@pytest.mark.parametrize("budget,cs", [(None, 5), (32 * KIB, 6)])
def test_level_present_with_a_common_entry_that_is_not_zero(tmp_path, budget, cs):
    t = flat("common")
    common = int(t[0])
    assert common & 0xFFFF == 1 and common >> 16 == 1
    q = [0, (1 << 23) - 1, 1 << 23, (1 << 24) - 1, CC.X(10, 1, 0), CC.X(10, 1, 16), CC.X(200, 1, 2)]  # (10.1.16.0: the other /20 of 10.1.0.0/19)
    stats, _, res = run(tmp_path, t, budget, queries=q)
    assert stats["has_summary"] == 1 and stats["common"] == common and stats["has_coarse"] == 1 and stats["coarse_shift"] == cs, stats
    assert (res[:, 0] == t[q]).all() and res[:, 1].tolist() == [0, 0, 2, 0, 2, 1, 2]
    ends = expected_ends(t, common, stats["shift"], cs)
    assert (stats["ends_coarse"], stats["ends_summary"], stats["ends_table"]) == ends and all(e > 0 for e in ends), (stats, ends)
