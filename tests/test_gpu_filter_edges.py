"""filter_kernel's chunk flags bit for bit at every edge of the stream (csrc/filter.hip, filter_rows). Everything behind the filter works
from the chunk bitmap it writes, and verdicts are blind to two kinds of mistake in it: a chunk flagged that should not be only costs a
comparison, and a chunk missed at a seam is a verdict only where a test happens to place a literal there. Here the bitmap itself is
read back (RuleEngine.filter_flags, the hook pwaf_engine_filter_flags) and compared with the numpy restatement of the shift-or
automaton over the whole arena (confirm_cases.window_positions, extended by filter_cases.byte_behind). The cases are built by
tests/filter_cases.py, which proves each one's shape with the model first (tests/test_filter_edges_cpu.py: the same without a device):

  A  the pass's literal across a lane, row, iteration, slab and workgroup seam, at every displacement, both strides and both phases
  B  arenas that end at 1 .. 4 x 131072 + 1 bytes, a window completing in their last bytes, behind a batch of six slabs that flagged
     every row (stale bitmap words); the byte behind the stream made visible
  C  the fused stride-1 / stride-2 launch with unequal classes, empty classes included; no two slabs of a batch alike
  D  random arenas -- lowercase, printable, all 256 byte values -- against 4 000 literals at both strides and against set S
  E  a slab view that begins inside slab 2: absolute positions, a warm-up from bytes that are no request's

Every batch, on the pass with a pair list and (A, B, C, E) on the same pass under PWAF_OPT_NO_CONFIRM: the chunk bits of every
streamed slab, the per-slab counts, the pair list's length and the slabs' places in it; A, B, C and E also verdicts and action counters
against pyoracle. docs/filter_edges.md records what each case measured and which tests fail when filter_rows is made subtly wrong."""
import numpy as np
import pytest

import filter_cases as FC
import helpers as H
from oracle import pyoracle
from pingoo_amd import _abi
from pingoo_amd.engine import PwafError, RuleEngine

pytestmark = pytest.mark.gpu

_engines, _oracles, _wants = {}, {}, {}


@pytest.fixture(scope="module")
def engine_of():
    """one engine per (rule set, flags), created when first asked for and kept for the module"""
    def get(rs, flags):
        if (rs.name, flags) not in _engines:
            _engines[rs.name, flags] = RuleEngine(rs.rules(flags), {}, flags=flags)
        return _engines[rs.name, flags]

    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()
    _wants.clear()


def oracle_verdicts(rs, batch):
    if rs.name not in _oracles:
        _oracles[rs.name] = pyoracle.Oracle(rs.rules(0), {})
    if id(batch) not in _wants:
        _wants[id(batch)] = (batch, _oracles[rs.name].evaluate(batch))
    return _wants[id(batch)][1]


def check_flags(what, eng, rs, flags, batch):
    """every filtered pass of the engine's latest batch against the model"""
    for field, (gi, g, slab0, want) in FC.expected(rs, flags, batch).items():
        fid = FC.FID[field]
        got = eng.filter_flags(gi)
        where = f"{what}: pass {gi} ({field}, stride {g['f_stride']})"
        print(where, "slab0", got["slab0"], "slabs", got["slabs"], "flagged", int(got["chunks"].sum()), "model", int(want.sum()), "pairs", got["pair_count"])
        assert (got["slab0"], got["slabs"], got["stride"]) == (slab0, len(want) // FC.SLAB_CHUNKS, g["f_stride"]), where
        assert len(got["chunks"]) == len(want), where
        bad = np.nonzero(got["chunks"] != want)[0]
        if len(bad):
            c = int(bad[0])
            at = (slab0 * FC.SLAB_CHUNKS + c) * FC.CHUNK
            raise AssertionError(f"{where}: {len(bad)} chunk bits differ from the model; first at (slab, iteration, row, lane) = {FC.describe_chunk(c, slab0)}, arena byte {at}: "
                                 f"device {int(got['chunks'][c])}, model {int(want[c])}; bytes {max(0, at - 4)}..: {batch.data[fid][max(0, at - 4):at + 20].tobytes()!r}, "
                                 f"the arena ends at {int(batch.offsets[fid][-1])}")
        pop = want.reshape(-1, FC.SLAB_CHUNKS).sum(axis=1)
        assert got["per_slab"].tolist() == pop.tolist(), where
        if g.get("confirm"):
            assert got["pair_count"] == int(pop.sum()), (where, got["pair_count"], int(pop.sum()))
            # the slabs' parts of the pair list, in whatever order their waves ended, tile [0, pair_count)
            parts = sorted((int(b), int(b) + int(n)) for b, n in zip(got["pair_base"], pop) if n)
            assert [a for a, _ in parts] == [0, *(b for _, b in parts)][:len(parts)] and (parts[-1][1] if parts else 0) == got["pair_count"], (where, parts)
        else:
            assert got["pair_base"] is None and got["pair_count"] is None, where


def send(case, engine_of, sent):
    for rs, flags in case.legs:
        eng = engine_of(rs, flags)
        for s in sent:
            what = f"case {case.name}: {s.label}, {'no pair list' if flags & FC.NO_CONFIRM else 'flags ' + str(flags)}"
            if s.before is not None:
                eng.evaluate_batch(s.before)
            got, counts = eng.evaluate_batch(s.batch, with_counts=True)
            check_flags(what, eng, rs, flags, s.batch)
            if s.verdicts:
                want = oracle_verdicts(rs, s.batch)
                H.assert_verdicts_equal(got, want, None, what)
                assert counts.tolist() == np.bincount(want["action"], minlength=4).tolist(), what


def test_the_hook_refuses_what_it_cannot_answer():
    rs = FC.set_f()
    eng = RuleEngine(rs.rules(0), {})
    plain = RuleEngine(rs.rules(0), {}, flags=_abi.OPT_NO_PREFILTER)
    try:
        with pytest.raises(PwafError, match="evaluated nothing"):
            eng.filter_flags(FC.passes(rs)["url"][0])
        batch = FC.case_c().sent[3].batch  # slabs (0, 5, 0, 0)
        eng.evaluate_batch(batch)
        plain.evaluate_batch(batch)
        with pytest.raises(PwafError, match="no prefilter"):
            eng.filter_flags(99)
        with pytest.raises(PwafError, match="no prefilter"):
            plain.filter_flags(0)
        got = eng.filter_flags(FC.passes(rs)["host"][0])  # every host field empty: no slab
        assert (got["slabs"], got["slab0"], len(got["chunks"]), got["pair_count"], got["stride"]) == (0, 0, 0, 0, 2)
        assert eng.filter_flags(FC.passes(rs)["url"][0])["slabs"] == 5
    finally:
        eng.close()
        plain.close()


def test_the_dirty_batch_flags_every_row_of_six_slabs(engine_of):
    """what case B sends in front of every batch: the device's bitmap has a bit in every row word, as the model's"""
    rs = FC.set_f()
    eng = engine_of(rs, 0)
    eng.evaluate_batch(FC.dirty_batch())
    check_flags("the dirty batch", eng, rs, 0, FC.dirty_batch())
    for field, (gi, g) in FC.passes(rs).items():
        got = eng.filter_flags(gi)
        assert got["slabs"] == FC.B_DIRTY_SLABS and got["chunks"].reshape(-1, 64).any(axis=1).all(), field


@pytest.mark.parametrize("j", range(FC.A_BATCHES))
def test_a_splits(engine_of, j):
    case = FC.case_a()
    send(case, engine_of, [case.sent[j]])


@pytest.mark.parametrize("total", FC.B_TOTALS)
def test_b_ends(engine_of, total):
    case = FC.case_b()
    sent = [s for s in case.sent if s.label.startswith(f"B total {total},")]
    assert len(sent) == 2
    send(case, engine_of, sent)


def test_b_the_byte_behind_the_stream(engine_of):
    """the pinned choice: the arena's last byte 'z' is paired with arena byte 0, 'q', when the arena ends on a chunk boundary that is
    not an iteration's end, and the chunk is flagged for `contains("zq")`; no verdict changes"""
    case = FC.case_b()
    sent = [s for s in case.sent if s.label.startswith("B byte behind")]
    assert len(sent) == 3
    send(case, engine_of, sent)
    eng = engine_of(*case.legs[0])
    eng.evaluate_batch(sent[0].batch)
    got = eng.filter_flags(FC.passes(case.legs[0][0])["url"][0])
    assert np.nonzero(got["chunks"])[0].tolist() == case.measured["visible"][FC.BEHIND_BYTE0] == [64]


@pytest.mark.parametrize("i", range(len(FC.C_SLABS)), ids=lambda i: "-".join(map(str, FC.C_SLABS[i])))
def test_c_mix(engine_of, i):
    case = FC.case_c()
    send(case, engine_of, [case.sent[i]])


@pytest.mark.parametrize("which", FC.D_LEGS, ids=lambda w: f"{w[0]}-{w[1]}-{w[2]}")
def test_d_bytes(engine_of, which):
    case = FC.case_d(which)
    send(case, engine_of, case.sent)


def test_e_view(engine_of):
    case = FC.case_e()
    send(case, engine_of, case.sent)
    rs, flags = case.legs[0]
    for field in ("url", "path"):
        assert engine_of(rs, flags).filter_flags(FC.passes(rs)[field][0])["slab0"] == 2
