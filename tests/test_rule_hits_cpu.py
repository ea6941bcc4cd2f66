"""Rule hits (PWAF_OPT_RULE_HITS), the part that needs no device: the compiler keeps an observe-only rule (a rule whose actions can never
take effect) only with the flag and is otherwise unchanged by it; the flag is refused beside the verdict kernels that cannot report
hits; struct layout; the entry points' argument checks; the host-side list -> matrix helper."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pingoo_amd import _abi
from pingoo_amd.batch import RULE_HIT_DTYPE, hits_to_matrix
from pingoo_amd.engine import CompiledProgram, PwafError, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, CAP = _abi.RULE_ACTION_BLOCK, _abi.RULE_ACTION_CAPTCHA
HITS = _abi.OPT_RULE_HITS
DECIDING = [("env", 'http_request.path.starts_with("/.env")', [B]), ("bot", 'http_request.user_agent.contains("bot") && client.remote_port < 1024', [CAP]),
            ("all", None, [CAP, B]), ("len", "http_request.url.length() - http_request.path.length() > 9", [B])]
OBSERVE = ("watch", 'http_request.path.contains("admin")', [])
FLAGS_AT = 8 + 16 + 7 * 4  # "PWAFPRG1", the HEAD section's header, seven words: the program's flags (csrc/compile.cpp: dump_program)


def with_observer(at):
    return DECIDING[:at] + [OBSERVE] + DECIDING[at:]


def clear_flag(dump: bytes) -> bytes:
    flags = int.from_bytes(dump[FLAGS_AT:FLAGS_AT + 4], "little")
    assert flags & HITS
    return dump[:FLAGS_AT] + (flags & ~HITS).to_bytes(4, "little") + dump[FLAGS_AT + 4:]


@pytest.mark.parametrize("at", [0, 2, 4])
def test_an_observe_only_rule_is_kept_with_the_flag_only(at):
    rules = with_observer(at)
    off, on = CompiledProgram(rules), CompiledProgram(rules, flags=HITS)
    assert on.stats()["n_rules"] == off.stats()["n_rules"] + 1
    # without the flag the rule is dropped as before: nothing but the caller's indices of the later rules tells the two sets apart
    assert off.stats()["n_rules"] == CompiledProgram(DECIDING).stats()["n_rules"]
    assert on.stats()["n_atoms"] == off.stats()["n_atoms"] + 1  # ("admin": no other rule reads it)
    # a rule that can never match stays dropped, whatever its actions
    never = rules + [("never", "false", []), ("never2", "1 == 2", [B])]
    assert CompiledProgram(never, flags=HITS).stats()["n_rules"] == on.stats()["n_rules"]


@pytest.mark.parametrize("extra", [0, _abi.OPT_TINY_VERDICT_SLOTS, _abi.OPT_GLOBAL_VERDICT_TABLES, _abi.OPT_NO_UA_GATE | _abi.OPT_EAGER_CMP])
def test_the_flag_alone_changes_nothing_but_the_flag_word(extra):
    off, on = CompiledProgram(DECIDING, flags=extra).dump(), CompiledProgram(DECIDING, flags=extra | HITS).dump()
    assert int.from_bytes(off[FLAGS_AT:FLAGS_AT + 4], "little") == extra
    assert clear_flag(on) == off
    # ... and a set with an observe-only rule, compiled without the flag, is the set without it but for the rule indices
    assert len(CompiledProgram(with_observer(4), flags=extra).dump()) == len(off)
    assert CompiledProgram(with_observer(4), flags=extra).dump() == off  # (the observer comes last: no index moves)


@pytest.mark.parametrize("variant", [_abi.OPT_SPARSE_VERDICT, _abi.OPT_DENSE_VERDICT, _abi.OPT_SPARSE_VERDICT | _abi.OPT_TINY_VERDICT_SLOTS])
def test_the_flag_is_refused_beside_the_column_file_verdict_kernels(variant):
    with pytest.raises(PwafError, match="PWAF_OPT_RULE_HITS") as ei:
        CompiledProgram(DECIDING, flags=HITS | variant)
    assert ei.value.code == _abi.E_INVALID_ARG
    CompiledProgram(DECIDING, flags=variant)
    CompiledProgram(DECIDING, flags=HITS | _abi.OPT_TINY_VERDICT_SLOTS | _abi.OPT_GLOBAL_VERDICT_TABLES)


def test_struct_size_and_null_engine():
    assert C.sizeof(_abi.RuleHit) == 16 and RULE_HIT_DTYPE.itemsize == 16
    assert [RULE_HIT_DTYPE.fields[k][1] for k in ("rule_idx", "group", "mask")] == [_abi.RuleHit.rule_idx.offset, _abi.RuleHit.group.offset, _abi.RuleHit.mask.offset] == [0, 4, 8]
    out, n = (C.c_uint64 * 4)(), C.c_uint32(7)
    st = _abi.Batch()
    assert lib().pwaf_evaluate_batch_hits(None, C.byref(st), out, None, None, 0, None, None) == _abi.E_INVALID_ARG
    assert lib().pwaf_evaluate_device_hits(None, C.byref(st), out, None, None, None, out, 1, C.addressof(n), None, None) == _abi.E_INVALID_ARG
    assert n.value == 7
    assert lib().pwaf_abi_version() == 4


def test_struct_size_against_c_compiler(tmp_path):
    prog = tmp_path / "sizes.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pwaf.h"\nint main(void){printf("%zu %zu %zu %zu %u\\n",sizeof(pwaf_rule_hit),offsetof(pwaf_rule_hit,rule_idx),'
                    'offsetof(pwaf_rule_hit,group),offsetof(pwaf_rule_hit,mask),PWAF_OPT_RULE_HITS);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [16, 0, 4, 8, HITS] and HITS == 131072


def test_hits_to_matrix():
    hits = np.array([(2, 0, 1 | (1 << 63)), (0, 1, 0b110), (2, 2, 1)], dtype=RULE_HIT_DTYPE)
    m = hits_to_matrix(hits, 129, 3)
    assert m.shape == (3, 129) and m.dtype == bool and m.sum() == 5
    assert m[2, 0] and m[2, 63] and m[0, 65] and m[0, 66] and m[2, 128] and not m[1].any()
    assert hits_to_matrix(hits[:0], 5, 3).sum() == 0
    with pytest.raises(AssertionError):
        hits_to_matrix(hits, 128, 3)
