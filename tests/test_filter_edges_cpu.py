"""The filter edge cases (tests/filter_cases.py) on the host: every case is BUILT here and its shape assertions made with the numpy model
of filter_kernel, by the same functions the device suite calls, so a shape that cannot be reached fails without a GPU; the model's
one extension, the byte behind the stream (filter_cases.byte_behind), changes nothing where the arena does not end on a chunk
boundary, and its three cases are exercised against hand-built eight-chunk arenas. docs/filter_edges.md records the figures
(`pytest -s` prints them)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import confirm_cases as CC
import filter_cases as FC
from oracle import pyoracle
from pingoo_amd import _abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_hook_is_declared_as_the_wrapper_reads_it_and_refuses_null():
    src = open(os.path.join(ROOT, "include", "pwaf.h")).read()
    assert int(re.search(r"#define PWAF_FILTER_SLAB_ROWS (\d+)", src).group(1)) == _abi.FILTER_SLAB_ROWS == FC.SLAB // FC.ROW
    assert len(_abi.FILTER_FLAGS_FIELDS) == 8
    L = engine.lib()
    assert L.pwaf_engine_filter_flags(None, 0, (C.c_uint32 * 8)(), None, 0, None, None, 0) == _abi.E_INVALID_ARG
    assert b"pwaf_engine_filter_flags" in L.pwaf_last_error()


def test_set_f_has_the_passes_the_cases_are_written_for():
    rs = FC.set_f()  # (asserts strides, tiers, heads, fillers and where each literal completes)
    for flags in (0, FC.NO_CONFIRM):
        print({f: (gi, g["f_stride"], g.get("confirm", 0)) for f, (gi, g) in FC.passes(rs, flags).items()})
    g = FC.passes(rs)["url"][1]
    for p in range(64, 96):
        assert FC.completes_at(g, "kw#7x", p) == p + 3 and FC.completes_at(g, "zq", p) == p  # (the bigram's second byte: p + 4, p + 1)
    for f in ("host", "path", "user_agent"):
        for lit in FC.F_LITS[f]:
            assert {FC.completes_at(FC.passes(rs)[f][1], lit, p) % 2 for p in range(64, 96)} == {0}


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_every_case_reaches_its_shape(name):
    case = FC.CASES[name]()
    print(name, case.measured)
    assert case.sent and all(FC.passes(rs, flags) for rs, flags in case.legs)
    # the legs stream the same arenas with the same tables: the pass without a pair list flags what the pass with one flags
    (rs, f0), (_, f1) = case.legs
    for s in case.sent[:: max(1, len(case.sent) // 4)]:
        a, b = FC.expected(rs, f0, s.batch), FC.expected(rs, f1, s.batch)
        assert all(a[f][2] == b[f][2] and (a[f][3] == b[f][3]).all() for f in a)
    if any(s.verdicts for s in case.sent):  # the oracle's verdicts are not all alike: the plants are found
        oracle = pyoracle.Oracle(rs.rules(0), {})
        assert any(len(set(oracle.evaluate(s.batch)["action"].tolist())) >= 2 for s in case.sent[-8:]), name


@pytest.mark.parametrize("which", FC.D_LEGS, ids=lambda w: f"{w[0]}-{w[1]}-{w[2]}")
def test_every_random_arena_flags_enough_and_not_too_much(which):
    case = FC.case_d(which)
    print(case.name, case.measured)


def test_the_byte_behind_the_stream_changes_nothing_unless_the_arena_ends_on_a_chunk_boundary():
    """every arena of the cases, cut at many ends: where total % 16 != 0 the extended model is the model as it stood"""
    rs = FC.set_f()
    pool = [(rs, 0, FC.case_c().sent[0].batch), (rs, 0, FC.case_b().sent[7].batch), (FC.set_sb(), 0, FC.d_arena("all 256 values")), (CC.set_a(), 0, FC.d_arena("lowercase"))]
    seen = set()
    for rset, flags, batch in pool:
        for f, (gi, g) in FC.passes(rset, flags).items():
            data, whole = batch.data[FC.FID[f]], int(batch.offsets[FC.FID[f]][-1])
            for total in sorted({t for t in list(range(1, 80)) + [1023, 1025, 4095, 4097, 8191, whole - 1, whole] if 0 < t <= whole}):
                case, b = FC.byte_behind(data, total)
                seen.add(case)
                if total % 16:
                    d = data[:total + 16].copy()
                    d[total:] = 0  # (the slack behind a batch's arena is zero)
                    assert (FC.device_chunks(g, d, total) == FC.device_chunks(g, d, total, extended=False)).all(), (rset.name, f, total, case)
    assert seen == {FC.BEHIND_AFTER, FC.BEHIND_BYTE0, FC.BEHIND_BYTE0_SLACK}


def test_the_three_cases_of_the_byte_behind_the_stream_on_eight_chunk_arenas():
    """set F's url pass, `contains("zq")`: one bigram is a window. Arenas of eight chunks (and of eight chunks of the LAST row of an
    iteration) that begin with 'q' and end with 'z'."""
    g = FC.passes(FC.set_f())["url"][1]
    assert g["f_stride"] == 1

    def arena(total, first=b"q", last=b"z"):
        return np.frombuffer(first + b"-" * (total - 2) + last + b"\0" * 16, dtype=np.uint8)

    # total % 16 == 0, not the end of an iteration: the last byte is paired with arena byte 0 -- "zq" by the extended model alone
    a = arena(128)
    assert FC.byte_behind(a, 128) == (FC.BEHIND_BYTE0, ord("q"))
    assert np.nonzero(FC.device_chunks(g, a, 128))[0].tolist() == [7] and not FC.device_chunks(g, a, 128, extended=False).any()
    assert not FC.device_chunks(g, arena(128, first=b"x"), 128).any()  # (another byte 0: no window)
    assert CC.window_positions(g, a, 128, behind=ord("q"))[127] and not CC.window_positions(g, a, 128)[127]
    # the arena ends with an iteration: `after`, the constant 0, whatever byte 0 is
    a = arena(4096)
    assert FC.byte_behind(a, 4096) == (FC.BEHIND_AFTER, 0) and FC.byte_behind(arena(4090), 4090) == (FC.BEHIND_AFTER, 0)
    assert not FC.device_chunks(g, a, 4096)[-8:].any() and not FC.device_chunks(g, a, 4096).any()
    # total % 16 != 0: the last byte is paired with the slack behind it; byte 0 stands behind the chunk's last SLACK byte
    a = arena(125)
    assert FC.byte_behind(a, 125) == (FC.BEHIND_BYTE0_SLACK, ord("q"))
    assert not FC.device_chunks(g, a, 125).any() and not FC.device_chunks(g, a, 125, extended=False).any()
    # ... and a real "zq" across the last lane seam is found by both
    a = np.frombuffer(b"-" * 111 + b"zq" + b"-" * 12 + b"\0" * 16, dtype=np.uint8)
    assert np.nonzero(FC.device_chunks(g, a, 125))[0].tolist() == np.nonzero(FC.device_chunks(g, a, 125, extended=False))[0].tolist() == [6]
    # stride 2 never looks across a dword: no byte behind the stream
    g2 = FC.passes(FC.set_f())["host"][1]
    a = arena(128)
    assert (CC.window_positions(g2, a, 128, behind=ord("q")) == CC.window_positions(g2, a, 128)).all()
