"""Host-side mirror of the reference's rule interface, over the C ABI of libpwaf.so.

Names follow the reference so call sites read the same:

    rules::Action {Block, Captcha}        rules/rules.rs:30-35      -> Action
    rules::compile_expression             rules/rules.rs:45-53      -> compile_expression
    rules::validate_expression            rules/rules.rs:55-77      -> validate_expression
    pingoo::rules::Rule {name, expression: Option<_>, actions}      -> Rule
    Rule::match_request / the rule loop   http_listener.rs:251-264  -> RuleEngine.evaluate(...)
    Error::ExpressionIsNotValid           rules/rules.rs:41-42      -> ExpressionIsNotValid

Every evaluation runs on the GPU through libpwaf.so; there is no Python or CPU evaluation path.
If the library (or a HIP device) is missing the calls raise — loudly.
"""
from __future__ import annotations

import ctypes as C
import enum
import ipaddress
import os
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from .batch import GEO_DTYPE, RESPONSE_DTYPE, RULE_HIT_DTYPE, VERDICT_DTYPE, Request, RequestBatch

_LIB = None
# PWAF_LIB_VARIANT=prof loads libpwaf_prof.so, the -DPWAF_PROFILING build with the timing-experiment switches (tools/ only: results may
# be wrong when a switch is set). Nothing else is ever loaded: there is no fallback of any kind.
_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), f"libpwaf_{os.environ['PWAF_LIB_VARIANT']}.so" if os.environ.get("PWAF_LIB_VARIANT") else "libpwaf.so")


class PwafError(RuntimeError):
    def __init__(self, code: int, message: str, rule_index: Optional[int] = None):
        super().__init__(f"[{code}] {message}")
        self.code = code
        self.message = message
        self.rule_index = rule_index


class ExpressionIsNotValid(PwafError):
    """rules::Error::ExpressionIsNotValid (rules/rules.rs:41-42)."""


class UnsupportedExpression(PwafError):
    """A valid expression outside the device-compilable subset."""


class DeviceError(PwafError):
    """No usable HIP device / a HIP call failed. The caller decides whether to fail open."""


def lib():
    """Loads libpwaf.so. Raises if it has not been built — the product path never falls back."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_LIB_PATH):
        raise ImportError(f"{_LIB_PATH} is missing: build it with `python -m pingoo_amd.build` (hipcc, gfx950). "
                          "pingoo_amd has no CPU fallback.")
    # ONE HIP runtime per process. libpwaf.so needs "libamdhip64.so.7"; PyTorch-ROCm bundles its own copy with that
    # very soname (plus its own libhsa-runtime64). Whichever is mapped first serves both users — two HSA runtimes in
    # one process do not work (the second sees no GPU). bench.py and the tests use torch for device buffers, streams
    # and torch.distributed, so when torch is installed its runtime is mapped first and libpwaf.so binds to it.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(_LIB_PATH)
    vp = C.c_void_p
    L.pwaf_abi_version.restype = C.c_uint32
    L.pwaf_last_error.restype = C.c_char_p
    L.pwaf_compile_expression.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.pwaf_validate_expression.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    create_args = [C.POINTER(_abi.RuleDesc), C.c_size_t, C.POINTER(_abi.ListDesc), C.c_size_t, C.POINTER(_abi.GeoipTable), C.POINTER(_abi.Options)]
    L.pwaf_program_compile.argtypes = create_args + [C.POINTER(vp), C.POINTER(_abi.CompileError)]
    L.pwaf_program_destroy.argtypes = [vp]
    L.pwaf_program_destroy.restype = None
    L.pwaf_program_dump.argtypes = [vp, vp, C.c_size_t]
    L.pwaf_program_dump.restype = C.c_size_t
    L.pwaf_program_warning_count.argtypes = [vp]
    L.pwaf_program_warning_count.restype = C.c_size_t
    L.pwaf_program_warning.argtypes = [vp, C.c_size_t]
    L.pwaf_program_warning.restype = C.c_char_p
    L.pwaf_program_stats.argtypes = [vp, C.POINTER(_abi.Stats)]
    L.pwaf_program_rule_status.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_size_t]
    L.pwaf_program_confirm_field.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint16), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pwaf_program_confirm_shape.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32)]
    L.pwaf_program_flat_image.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_size_t]
    L.pwaf_program_flat_image.restype = C.c_size_t
    L.pwaf_program_list_scans.argtypes = [vp, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]
    L.pwaf_program_verdict_shape.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.pwaf_engine_compute_units.argtypes = [vp]
    L.pwaf_engine_compute_units.restype = C.c_uint32
    L.pwaf_engine_rule_errors.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t]
    L.pwaf_engine_residual_mode.argtypes = [vp]
    L.pwaf_engine_address_tables.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.pwaf_engine_residual_fallback.argtypes = [vp]
    L.pwaf_engine_residual_fallback.restype = C.c_char_p
    L.pwaf_program_residual_source.argtypes = [vp, C.c_int, C.c_char_p, C.c_size_t]
    L.pwaf_program_residual_source.restype = C.c_size_t
    L.pwaf_program_residual_compile.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_size_t]
    L.pwaf_program_residual_compile.restype = C.c_long
    L.pwaf_engine_create.argtypes = create_args + [C.POINTER(vp), C.POINTER(_abi.CompileError)]
    L.pwaf_engine_destroy.argtypes = [vp]
    L.pwaf_engine_destroy.restype = None
    L.pwaf_engine_program.argtypes = [vp]
    L.pwaf_engine_program.restype = vp
    L.pwaf_engine_stats.argtypes = [vp, C.POINTER(_abi.Stats)]
    for fn_name in ("pwaf_engine_header_count", "pwaf_program_header_count"):
        getattr(L, fn_name).argtypes = [vp]
        getattr(L, fn_name).restype = C.c_uint32
    for fn_name in ("pwaf_engine_header_name", "pwaf_program_header_name"):
        getattr(L, fn_name).argtypes = [vp, C.c_uint32]
        getattr(L, fn_name).restype = C.c_char_p
    L.pwaf_engine_stream.argtypes = [vp]
    L.pwaf_engine_stream.restype = vp
    L.pwaf_evaluate_batch.argtypes = [vp, C.POINTER(_abi.Batch), vp, vp]
    L.pwaf_evaluate_device.argtypes = [vp, C.POINTER(_abi.Batch), vp, vp, vp, vp, vp]
    L.pwaf_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.pwaf_host_free.argtypes = [vp]
    L.pwaf_host_free.restype = None
    L.pwaf_host_register.argtypes = [vp, C.c_size_t]
    L.pwaf_host_unregister.argtypes = [vp]
    L.pwaf_evaluate_one.argtypes = [vp, C.POINTER(_abi.Request), C.POINTER(_abi.Verdict)]
    L.pwaf_engine_device_status.argtypes = [vp]
    L.pwaf_engine_set_profiling.argtypes = [vp, C.c_int]
    L.pwaf_engine_tune.argtypes = [vp, C.POINTER(_abi.Batch)]
    L.pwaf_program_tune.argtypes = [vp, C.POINTER(_abi.Batch)]
    L.pwaf_node_create.argtypes = create_args + [C.POINTER(C.c_int), C.c_size_t, C.POINTER(vp), C.POINTER(_abi.CompileError)]
    L.pwaf_node_destroy.argtypes = [vp]
    L.pwaf_node_destroy.restype = None
    L.pwaf_node_device_count.argtypes = [vp]
    L.pwaf_node_device_count.restype = C.c_size_t
    L.pwaf_node_engine.argtypes = [vp, C.c_size_t]
    L.pwaf_node_engine.restype = vp
    L.pwaf_node_tune.argtypes = [vp, C.POINTER(_abi.Batch)]
    L.pwaf_node_evaluate_batch.argtypes = [vp, C.POINTER(_abi.Batch), vp, vp]
    L.pwaf_node_evaluate_device.argtypes = [vp, C.POINTER(C.POINTER(_abi.Batch)), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.pwaf_node_synchronize.argtypes = [vp]
    L.pwaf_node_allreduce_counts.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.pwaf_node_shard_bounds.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.pwaf_node_shard_bounds.restype = None
    L.pwaf_batcher_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.pwaf_batcher_evaluate.argtypes = [vp, C.POINTER(_abi.Request), C.POINTER(_abi.Verdict)]
    L.pwaf_batcher_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.pwaf_batcher_destroy.argtypes = [vp]
    L.pwaf_batcher_destroy.restype = None
    L.pwaf_evaluate_records.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, vp, vp]
    L.pwaf_export_records.argtypes = [C.POINTER(_abi.Batch), vp, C.c_uint32, vp, vp, C.c_size_t, vp, vp, vp]
    L.pwaf_evaluate_records_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, vp, vp, vp, vp, vp, vp]
    L.pwaf_records_scan_shape.argtypes = [C.POINTER(C.c_uint32)]
    L.pwaf_client_ids.argtypes = [C.POINTER(_abi.Batch), vp, C.c_uint32, vp, vp, vp]
    L.pwaf_client_id_one.argtypes = [C.POINTER(_abi.Request), vp]
    L.pwaf_keyset_create.argtypes = [C.POINTER(_abi.Ed25519Key), C.c_uint32, C.c_int, C.POINTER(vp)]
    L.pwaf_keyset_destroy.argtypes = [vp]
    L.pwaf_keyset_destroy.restype = None
    L.pwaf_verify_cookies_scratch_bytes.argtypes = [C.c_uint32]
    L.pwaf_verify_cookies_scratch_bytes.restype = C.c_size_t
    L.pwaf_verify_cookies.argtypes = [vp, C.POINTER(_abi.Batch), C.POINTER(_abi.StrCol), C.c_int64, vp, C.c_uint32, vp, vp, vp, vp, C.c_size_t, vp]
    L.pwaf_verify_cookie_one.argtypes = [vp, C.POINTER(_abi.Request), vp, C.c_uint32, C.c_int64, C.POINTER(C.c_uint8)]
    L.pwaf_verify_pow_scratch_bytes.argtypes = [C.c_uint32]
    L.pwaf_verify_pow_scratch_bytes.restype = C.c_size_t
    L.pwaf_verify_pow.argtypes = [vp, C.POINTER(_abi.Batch), C.POINTER(_abi.StrCol), vp, C.POINTER(_abi.StrCol), C.c_int64, vp, C.c_uint32, vp, vp, vp, C.c_size_t, vp]
    L.pwaf_verify_pow_one.argtypes = [vp, C.POINTER(_abi.Request), vp, C.c_uint32, vp, vp, C.c_uint32, C.c_int64, C.POINTER(C.c_uint8)]
    L.pwaf_parse_pow_bodies_scratch_bytes.argtypes = [C.c_uint32]
    L.pwaf_parse_pow_bodies_scratch_bytes.restype = C.c_size_t
    L.pwaf_parse_pow_bodies.argtypes = [C.POINTER(_abi.StrCol), C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.POINTER(_abi.DerivedCol), vp, vp, C.c_size_t, vp]
    L.pwaf_parse_pow_body_one.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint8), vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.pwaf_parse_pow_scan_shape.argtypes = [C.POINTER(C.c_uint32)]
    L.pwaf_respond_scratch_bytes.argtypes = [C.c_uint32]
    L.pwaf_respond_scratch_bytes.restype = C.c_size_t
    L.pwaf_respond.argtypes = [C.POINTER(_abi.Batch), vp, vp, vp, vp, vp, C.POINTER(_abi.RespList), C.c_uint32, vp, C.c_size_t, vp]
    L.pwaf_respond_one.argtypes = [C.POINTER(_abi.Verdict), C.c_uint8, C.c_int, C.c_uint32, vp, C.c_uint32, C.POINTER(_abi.Response)]
    L.pwaf_respond_scan_shape.argtypes = [C.POINTER(C.c_uint32)]
    L.pwaf_derive_scratch_bytes.argtypes = [C.c_uint32]
    L.pwaf_derive_scratch_bytes.restype = C.c_size_t
    L.pwaf_derive_batch.argtypes = [C.POINTER(_abi.Batch), C.POINTER(_abi.RawColumns), C.POINTER(_abi.DerivedCol), vp, vp, C.c_size_t, vp]
    L.pwaf_derive_scan_shape.argtypes = [C.POINTER(C.c_uint32)]
    L.pwaf_async_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.pwaf_async_submit.argtypes = [vp, C.POINTER(_abi.Request), C.c_uint64]
    L.pwaf_async_poll.argtypes = [vp, C.POINTER(_abi.Completion), C.c_size_t]
    L.pwaf_async_poll.restype = C.c_size_t
    L.pwaf_async_fd.argtypes = [vp]
    L.pwaf_async_flush.argtypes = [vp]
    L.pwaf_async_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.pwaf_async_destroy.argtypes = [vp]
    L.pwaf_async_destroy.restype = None
    # GeoIP answers (engines created with OPT_GEO_ANSWERS)
    L.pwaf_geoip_lookup.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp]
    L.pwaf_evaluate_batch_geo.argtypes = [vp, C.POINTER(_abi.Batch), vp, vp, vp]
    L.pwaf_evaluate_device_geo.argtypes = [vp, C.POINTER(_abi.Batch), vp, vp, vp, vp, vp, vp]
    L.pwaf_evaluate_batch_hits.argtypes = [vp, C.POINTER(_abi.Batch), vp, vp, vp, C.c_uint32, vp, vp]
    L.pwaf_evaluate_device_hits.argtypes = [vp, C.POINTER(_abi.Batch), vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp]
    # routes (engines created with routes beside their rules)
    routed_args = create_args[:2] + [C.POINTER(_abi.RouteDesc), C.c_size_t] + create_args[2:]
    L.pwaf_program_compile_routed.argtypes = routed_args + [C.POINTER(vp), C.POINTER(_abi.CompileError)]
    L.pwaf_engine_create_routed.argtypes = routed_args + [C.POINTER(vp), C.POINTER(_abi.CompileError)]
    for fn_name in ("pwaf_engine_route_count", "pwaf_program_route_count"):
        getattr(L, fn_name).argtypes = [vp]
        getattr(L, fn_name).restype = C.c_uint32
    L.pwaf_evaluate_batch_routes.argtypes = [vp, C.POINTER(_abi.Batch), vp, vp, vp]
    L.pwaf_evaluate_device_routes.argtypes = [vp, C.POINTER(_abi.Batch), vp, vp, vp, vp, vp, vp]
    L.pwaf_evaluate_one_route.argtypes = [vp, C.POINTER(_abi.Request), C.POINTER(_abi.Verdict), C.POINTER(C.c_uint32)]
    L.pwaf_evaluate_records_geo.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, vp, vp, vp]
    L.pwaf_evaluate_one_geo.argtypes = [vp, C.POINTER(_abi.Request), C.POINTER(_abi.Verdict), C.POINTER(_abi.Geo)]
    L.pwaf_async_create_geo.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.pwaf_async_poll_geo.argtypes = [vp, C.POINTER(_abi.Completion), C.POINTER(_abi.Geo), C.c_size_t]
    L.pwaf_async_poll_geo.restype = C.c_size_t
    L.pwaf_engine_geo_answer_tables.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.pwaf_engine_coarse_tables.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.pwaf_engine_filter_flags.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32), vp, C.c_size_t, vp, vp, C.c_size_t]
    L.pwaf_geoip_from_mmdb.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(_abi.GeoipEntry)), C.POINTER(C.c_size_t)]
    L.pwaf_geoip_from_file_image.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(_abi.GeoipEntry)), C.POINTER(C.c_size_t)]
    L.pwaf_zstd_decompress.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.pwaf_buffer_free.argtypes = [C.c_void_p]
    L.pwaf_buffer_free.restype = None
    L.pwaf_geoip_free.argtypes = [C.POINTER(_abi.GeoipEntry)]
    L.pwaf_geoip_free.restype = None
    L.pwaf_list_parse_csv.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.c_size_t)]
    L.pwaf_list_free.argtypes = [C.POINTER(C.c_char_p), C.c_size_t]
    L.pwaf_list_free.restype = None
    L.pwaf_engine_kernel_times.argtypes = [vp, C.POINTER(_abi.KernelTime), C.c_int]
    L.pwaf_derive_path.argtypes = [C.c_char_p, C.c_size_t]
    L.pwaf_derive_path.restype = C.c_size_t
    L.pwaf_derive_user_agent.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.pwaf_derive_user_agent.restype = None
    L.pwaf_derive_host.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.pwaf_derive_host.restype = None
    if L.pwaf_abi_version() != _abi.ABI_VERSION:
        raise ImportError("libpwaf.so ABI version mismatch: rebuild with `python -m pingoo_amd.build --force`")
    _LIB = L
    return L


def _raise(code: int, message: str, rule_index: Optional[int] = None):
    cls = {_abi.E_SYNTAX: ExpressionIsNotValid, _abi.E_UNSUPPORTED: UnsupportedExpression, _abi.E_DEVICE: DeviceError}.get(code, PwafError)
    raise cls(code, message, rule_index)


def _check(rc: int, message: str = "", rule_index: Optional[int] = None) -> None:
    """The status of a C ABI call: 0, or the error to raise with `message` or else what the library recorded for it."""
    if rc != 0:
        _raise(rc, message or lib().pwaf_last_error().decode(errors="replace"), rule_index)


class Action(enum.IntEnum):
    """rules::Action (rules/rules.rs:30-35). Values are the PWAF_RULE_ACTION_* codes."""

    Block = _abi.RULE_ACTION_BLOCK
    Captcha = _abi.RULE_ACTION_CAPTCHA


class Decision(enum.IntEnum):
    """What the listener does with the request (http_listener.rs:196-264)."""

    Allow = _abi.ACTION_ALLOW
    Block = _abi.ACTION_BLOCK
    Captcha = _abi.ACTION_CAPTCHA
    Bypass = _abi.ACTION_BYPASS  # /__pingoo/captcha endpoints: rules are skipped


@dataclass
class Rule:
    """pingoo::rules::Rule (pingoo/rules.rs:9-14). expression None == match all."""

    name: str
    expression: Optional[str]
    actions: Sequence[Action] = field(default_factory=list)

    def as_tuple(self) -> Tuple[str, Optional[str], List[int]]:
        return (self.name, self.expression, [int(a) for a in self.actions])


@dataclass
class Verdict:
    decision: Decision
    rule_idx: Optional[int]  # index of the deciding rule; None for Allow / the built-in gates
    gate: Optional[str] = None  # "user_agent" | "captcha_endpoint" when a built-in gate decided


def compile_expression(expression: str) -> None:
    """rules::compile_expression: raises ExpressionIsNotValid on a syntax error."""
    buf = C.create_string_buffer(512)
    rc = lib().pwaf_compile_expression(expression.encode(), buf, 512)
    if rc != 0:
        _raise(rc, buf.value.decode(errors="replace"))


def validate_expression(expression: str) -> None:
    """rules::validate_expression: additionally rejects "" and the `in` operator."""
    buf = C.create_string_buffer(512)
    rc = lib().pwaf_validate_expression(expression.encode(), buf, 512)
    if rc != 0:
        _raise(rc, buf.value.decode(errors="replace"))


def get_path(uri_path: bytes) -> bytes:
    """get_path (http_utils.rs:114-116)."""
    return uri_path[: lib().pwaf_derive_path(uri_path, len(uri_path))]


def get_user_agent(header: Optional[bytes]) -> bytes:
    """The User-Agent derivation of http_listener.rs:159-165."""
    s, l = C.c_size_t(), C.c_size_t()
    h = header or b""
    lib().pwaf_derive_user_agent(h, len(h), int(header is not None), C.byref(s), C.byref(l))
    return h[s.value:s.value + l.value]


def get_host(uri_host: Optional[bytes], host_header: Optional[bytes]) -> bytes:
    """get_host (http_listener.rs:284-296)."""
    s, l, fh = C.c_size_t(), C.c_size_t(), C.c_int()
    a, b = uri_host or b"", host_header or b""
    lib().pwaf_derive_host(a, len(a), int(uri_host is not None), b, len(b), int(host_header is not None), C.byref(fh), C.byref(s), C.byref(l))
    src = b if fh.value else a
    return src[s.value:s.value + l.value]


def generate_captcha_client_id(ip, user_agent, host) -> str:
    """captcha::generate_captcha_client_id (pingoo/captcha.rs:409-421; called at http_listener.rs:167) through pwaf_client_id_one:
    base64url_nopad(SHA-256(ip octets || user_agent || host)), 43 characters. ip: a str or an ipaddress object; user_agent and host:
    str or bytes, as get_user_agent / get_host derive them. Runs on the host."""
    from .batch import ip_to_bytes16

    ua, h = (x.encode() if isinstance(x, str) else bytes(x) for x in (user_agent, host))
    st = _abi.Request()
    st.user_agent, st.user_agent_len, st.host, st.host_len = ua, len(ua), h, len(h)
    raw, v6 = ip_to_bytes16(str(ip))
    C.memmove(st.ip, raw, 16)
    st.ip_is_v6 = int(v6)
    out = _abi.ClientId()
    _check(lib().pwaf_client_id_one(C.byref(st), C.addressof(out)))
    return out.text.decode("ascii")


def _options(flags=0, device=-1, lds_table_budget=0, max_dfa_states=0, max_table_bytes=0) -> _abi.Options:
    o = _abi.Options()
    o.struct_size = C.sizeof(_abi.Options)
    o.flags = flags
    o.device = device
    o.lds_table_budget = lds_table_budget
    o.max_dfa_states = max_dfa_states
    o.max_table_bytes = max_table_bytes
    return o


def _norm_rules(rules) -> List[Tuple[str, Optional[str], List[int]]]:
    return [r.as_tuple() if isinstance(r, Rule) else (r[0], r[1], [int(a) for a in r[2]]) for r in rules]


class CompiledProgram:
    """Host-side compilation only (no GPU): stats, warnings and the table dump used by the tests."""

    def __init__(self, rules, lists: Optional[Dict[str, Tuple[int, Sequence[str]]]] = None, geoip: Optional[np.ndarray] = None, routes=None, **opts):
        """routes: ordered [(name, expression | None)] compiled beside the rules (pwaf_program_compile_routed); None: pwaf_program_compile."""
        L = lib()
        m = _abi.Marshalled()
        r, nr = _abi.marshal_rules(_norm_rules(rules), m)
        l, nl = _abi.marshal_lists(lists, m)
        g = _abi.marshal_geoip(geoip, m)
        o = _options(**opts)
        h = C.c_void_p()
        err = _abi.CompileError()
        if routes is None:
            rc = L.pwaf_program_compile(r, nr, l, nl, g, C.byref(o), C.byref(h), C.byref(err))
        else:
            rt, nrt = _abi.marshal_routes(routes, m)
            rc = L.pwaf_program_compile_routed(r, nr, rt, nrt, l, nl, g, C.byref(o), C.byref(h), C.byref(err))
        if rc < 0:
            _raise(rc, err.message.decode(errors="replace"), None if err.rule_index == 0xFFFFFFFF else err.rule_index)
        self.partial = rc == _abi.W_PARTIAL  # PWAF_OPT_LENIENT: some rule is not evaluated (rule_status / warnings say which)
        self._h = h
        self._owned = True

    @property
    def header_names(self) -> List[str]:
        """EXTENSION: the header names the rule set mentions = the header columns a batch must carry, in this order."""
        return [lib().pwaf_program_header_name(self._h, i).decode() for i in range(lib().pwaf_program_header_count(self._h))]

    @classmethod
    def _borrow(cls, handle) -> "CompiledProgram":
        self = cls.__new__(cls)
        self._h = C.c_void_p(handle)
        self._owned = False
        return self

    def __del__(self):
        if getattr(self, "_owned", False) and self._h:
            lib().pwaf_program_destroy(self._h)
            self._h = None

    def dump(self) -> bytes:
        n = lib().pwaf_program_dump(self._h, None, 0)
        buf = C.create_string_buffer(n)
        lib().pwaf_program_dump(self._h, buf, n)
        return buf.raw

    def confirm_field(self, group: int, data: bytes, arena_offset: int = 0):
        """TEST HOOK (pwaf_program_confirm_field): prefilter + confirm tier of pass `group` over one field value, run by the very code the
        device compiles (csrc/confirm.h). Returns (local atoms of the confirmed literal predicates, flagged, walk)."""
        atoms = (C.c_uint16 * 4096)()
        n, fl, wk = C.c_size_t(), C.c_int(), C.c_int()
        _check(lib().pwaf_program_confirm_field(self._h, group, data, len(data), arena_offset, atoms, 4096, C.byref(n), C.byref(fl), C.byref(wk)))
        return sorted(set(atoms[k] for k in range(n.value))), bool(fl.value), bool(wk.value)

    def confirm_shape(self, group: int) -> dict:
        """TEST HOOK (pwaf_program_confirm_shape): the shape of pass `group`'s confirm tier, by the names of _abi.CONFIRM_SHAPE_FIELDS —
        entries, pool bytes, class words, in_lds (confirm_kernel compares from its LDS copy), longest factor, highest class position,
        largest bin, has_walk. Raises for a pass without a confirm tier."""
        out = (C.c_uint32 * len(_abi.CONFIRM_SHAPE_FIELDS))()
        _check(lib().pwaf_program_confirm_shape(self._h, group, out))
        return dict(zip(_abi.CONFIRM_SHAPE_FIELDS, (int(x) for x in out)))

    def flat_image(self, group: int, tier: int = 0) -> bytes:
        """TEST HOOK (pwaf_program_flat_image): the list scan's flat table of pass `group` exactly as an engine uploads it (tier 0: of every
        atom, 1: the R tier), as sections of the dump's format — "FSHP" (_abi.FLAT_SHAPE_FIELDS), cells, delta records, class image, emit
        and end lists. After tune() the table rebuilt for the sample. Raises for a pass without that tier."""
        n = lib().pwaf_program_flat_image(self._h, group, tier, None, 0)
        if n == 0:
            _check(_abi.E_INVALID_ARG)
        buf = C.create_string_buffer(n)
        lib().pwaf_program_flat_image(self._h, group, tier, buf, n)
        return buf.raw

    def list_scans(self) -> List[dict]:
        """TEST HOOK (pwaf_program_list_scans): the list-scan descriptors of every batch of an engine created from this program, in launch
        order, by the names of _abi.LIST_SCAN_FIELDS (share_owner -1: the pass walks a list of its own)."""
        W = len(_abi.LIST_SCAN_FIELDS)
        n = C.c_size_t()
        rc = lib().pwaf_program_list_scans(self._h, None, 0, C.byref(n))
        if rc == 0 and n.value:
            out = (C.c_uint32 * (W * n.value))()
            rc = lib().pwaf_program_list_scans(self._h, out, n.value, C.byref(n))
        _check(rc)
        res = [dict(zip(_abi.LIST_SCAN_FIELDS, (int(x) for x in out[k * W:(k + 1) * W]))) for k in range(n.value)]
        for d in res:
            d["share_owner"] = -1 if d["share_owner"] == 0xFFFFFFFF else d["share_owner"]
        return res

    def verdict_shape(self) -> dict:
        """TEST HOOK (pwaf_program_verdict_shape): the verdict kernel's launch shape in every batch of an engine created from this program,
        by the names of _abi.VERDICT_SHAPE_FIELDS — mode, capacity per wave, waves per workgroup (0: engine creation refuses the program),
        workgroups per CU, tables in LDS, LDS bytes, the pass count it was computed for and the bitmap registers that count selects."""
        out = (C.c_uint32 * len(_abi.VERDICT_SHAPE_FIELDS))()
        _check(lib().pwaf_program_verdict_shape(self._h, out))
        return dict(zip(_abi.VERDICT_SHAPE_FIELDS, (int(x) for x in out)))

    def residual_source(self, kind: int = 1) -> str:
        """Inspection hook: the specialized form of the residual rules (csrc/residual_jit.cpp). kind 0 = the rule functions alone,
        1 = the whole device program as handed to hiprtc at engine creation. "" when the rule set has no residual rules."""
        n = lib().pwaf_program_residual_source(self._h, kind, None, 0)
        if n == 0:
            return ""
        buf = C.create_string_buffer(n + 1)
        lib().pwaf_program_residual_source(self._h, kind, buf, n + 1)
        return buf.value.decode()

    def residual_compile(self, arch: str = "gfx950") -> int:
        """Inspection hook: compiles that program with hiprtc for `arch` (no device needed); the code object's size (0: no residual rules)."""
        err = C.create_string_buffer(4000)
        rc = lib().pwaf_program_residual_compile(self._h, arch.encode(), err, 4000)
        if rc < 0:
            _raise(int(rc), err.value.decode(errors="replace"))
        return int(rc)

    def rule_status(self, i: int) -> Tuple[int, str]:
        """(PWAF_OK, "") or (PWAF_E_UNSUPPORTED, reason): a rule the device compiler cannot take never matches and says so here."""
        buf = C.create_string_buffer(300)
        rc = lib().pwaf_program_rule_status(self._h, i, buf, 300)
        return rc, buf.value.decode(errors="replace")

    def unsupported_rules(self, n_rules: int) -> List[int]:
        return [i for i in range(n_rules) if self.rule_status(i)[0] != 0]

    def tune(self, sample: RequestBatch) -> None:
        """The host half of RuleEngine.tune on this program alone (no device): the prefilters in the dump become the tuned ones."""
        st = sample.as_struct(self.header_names)
        _check(lib().pwaf_program_tune(self._h, C.byref(st)))

    def warnings(self) -> List[str]:
        return [lib().pwaf_program_warning(self._h, i).decode(errors="replace") for i in range(lib().pwaf_program_warning_count(self._h))]

    def stats(self) -> dict:
        s = _abi.Stats()
        lib().pwaf_program_stats(self._h, C.byref(s))
        res = {k: getattr(s, k) for k, _ in _abi.Stats._fields_ if k != "reserved"}
        res["n_routes"] = int(lib().pwaf_program_route_count(self._h))  # (pwaf_stats has no room: a getter of its own)
        return res


class RuleEngine:
    """The engine handle that replaces `(Arc<Vec<Rule>>, lists, geoip)` (pingoo/server.rs:40-47,76).

    rules: ordered [Rule | (name, expression|None, [actions])]
    lists: {name: (LIST_STRING|LIST_INT|LIST_IP, [csv column-0 strings])}
    geoip: GEOIP_DTYPE array (see pingoo_amd.batch.geoip_entries) or None
    routes: ordered [(name, expression|None)] — the services' `route:` expressions; the engine then also answers each request's first
            matching route in the same pass (evaluate_batch_routes, evaluate_routed, evaluate_device(route=...)). None: no routes.
    """

    def __init__(self, rules, lists: Optional[Dict[str, Tuple[int, Sequence[str]]]] = None, geoip: Optional[np.ndarray] = None, routes=None, **opts):
        L = lib()
        m = _abi.Marshalled()
        self.rules = _norm_rules(rules)
        self.routes = [(n, x) for n, x in routes] if routes is not None else []
        r, nr = _abi.marshal_rules(self.rules, m)
        l, nl = _abi.marshal_lists(lists, m)
        g = _abi.marshal_geoip(geoip, m)
        o = _options(**opts)
        h = C.c_void_p()
        err = _abi.CompileError()
        if routes is None:
            rc = L.pwaf_engine_create(r, nr, l, nl, g, C.byref(o), C.byref(h), C.byref(err))
        else:
            rt, nrt = _abi.marshal_routes(self.routes, m)
            rc = L.pwaf_engine_create_routed(r, nr, rt, nrt, l, nl, g, C.byref(o), C.byref(h), C.byref(err))
        if rc < 0:
            _raise(rc, err.message.decode(errors="replace"), None if err.rule_index == 0xFFFFFFFF else err.rule_index)
        self.partial = rc == _abi.W_PARTIAL  # PWAF_OPT_LENIENT: some rule is not evaluated (program.rule_status / warnings say which)
        self._h = h
        self.header_names = [L.pwaf_engine_header_name(h, i).decode() for i in range(L.pwaf_engine_header_count(h))]

    def close(self):
        if getattr(self, "_h", None):
            lib().pwaf_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def program(self) -> CompiledProgram:
        return CompiledProgram._borrow(lib().pwaf_engine_program(self._h))

    @property
    def residual_mode(self) -> int:
        """0: no residual rules; 1: interpreted per request (residual_kernel); 2: specialized — compiled for this device by hiprtc when
        the engine was created (csrc/residual_jit.cpp). With 1 and no OPT_NO_RESIDUAL_JIT, `residual_fallback` says why."""
        return int(lib().pwaf_engine_residual_mode(self._h))

    @property
    def residual_fallback(self) -> str:
        return (lib().pwaf_engine_residual_fallback(self._h) or b"").decode(errors="replace")

    def compute_units(self) -> int:
        """TEST HOOK (pwaf_engine_compute_units): the compute units the engine sizes its persistent grids with."""
        return int(lib().pwaf_engine_compute_units(self._h))

    def address_tables(self) -> dict:
        """TEST HOOK (pwaf_engine_address_tables): the shape of this engine's IPv4 lookup structures, by the names of
        _abi.ADDRESS_TABLE_FIELDS — escapes, run-table length, summary present / granularity / common entry, packed, classes, sets."""
        out = (C.c_uint32 * len(_abi.ADDRESS_TABLE_FIELDS))()
        _check(lib().pwaf_engine_address_tables(self._h, out))
        return dict(zip(_abi.ADDRESS_TABLE_FIELDS, (int(x) for x in out)))

    def coarse_tables(self) -> dict:
        """TEST HOOK (pwaf_engine_coarse_tables): the coarse bitmap in front of the summary — present, shift, bytes, blocks set, the
        summary's blocks set, the lookup kernel's launch shape — by the names of _abi.COARSE_TABLE_FIELDS."""
        out = (C.c_uint32 * len(_abi.COARSE_TABLE_FIELDS))()
        _check(lib().pwaf_engine_coarse_tables(self._h, out))
        return dict(zip(_abi.COARSE_TABLE_FIELDS, (int(x) for x in out)))

    def filter_flags(self, group: int) -> dict:
        """TEST HOOK (pwaf_engine_filter_flags): what filter_kernel left for scan pass `group` in the engine's most recent batch (a host
        batch, or a device batch on the default stream) -> slab0, slabs, stride (ints), chunks (bool per 16-byte chunk of the streamed
        slabs, chunk c at arena byte slab0 * 131072 + 16 c; every row word of every slab), per_slab (the waves' own counts), pair_base
        (where each slab's pairs begin) and pair_count (both None for a pass without a pair list)."""
        L = lib()
        info = (C.c_uint32 * len(_abi.FILTER_FLAGS_FIELDS))()
        _check(L.pwaf_engine_filter_flags(self._h, group, info, None, 0, None, None, 0))
        d = dict(zip(_abi.FILTER_FLAGS_FIELDS, (int(x) for x in info)))
        assert d["slab_rows"] == _abi.FILTER_SLAB_ROWS
        slabs = d["slabs"]
        rows = np.zeros(slabs * _abi.FILTER_SLAB_ROWS, dtype="<u8")
        per_slab, pair_base = np.zeros(slabs, dtype=np.uint32), np.zeros(slabs, dtype=np.uint32)
        if slabs:
            _check(L.pwaf_engine_filter_flags(self._h, group, info, rows.ctypes.data, len(rows), per_slab.ctypes.data, pair_base.ctypes.data, slabs))
        has_pairs = bool(d["has_pairs"])
        return dict(slab0=d["slab0"], slabs=slabs, stride=d["stride"], chunks=np.unpackbits(rows.view(np.uint8), bitorder="little").astype(bool), per_slab=per_slab,
                    pair_base=pair_base if has_pairs else None, pair_count=d["pair_count"] if has_pairs else None)

    def geo_answer_tables(self) -> dict:
        """TEST HOOK (pwaf_engine_geo_answer_tables; OPT_GEO_ANSWERS engines): the shape of the record tables, by the names of
        _abi.GEO_ANSWER_TABLE_FIELDS."""
        out = (C.c_uint32 * len(_abi.GEO_ANSWER_TABLE_FIELDS))()
        _check(lib().pwaf_engine_geo_answer_tables(self._h, out))
        return dict(zip(_abi.GEO_ANSWER_TABLE_FIELDS, (int(x) for x in out)))

    def lookup_geoip(self, ip16, v6) -> np.ndarray:
        """GeoipDB::lookup for a batch of addresses (pwaf_geoip_lookup; OPT_GEO_ANSWERS engines): ip16 = n x 16 address bytes (IPv4 in
        bytes 0..3), v6 = n family flags -> GEO_DTYPE array, the default record {0, "XX"} where the reference finds none."""
        ip16 = np.ascontiguousarray(ip16, dtype=np.uint8).reshape(-1, 16)
        v6 = np.ascontiguousarray(v6, dtype=np.uint8).reshape(-1)
        assert len(ip16) == len(v6)
        out = np.zeros(len(v6), dtype=GEO_DTYPE)
        _check(lib().pwaf_geoip_lookup(self._h, ip16.ctypes.data, v6.ctypes.data, len(v6), _abi.MEM_HOST, out.ctypes.data, None))
        return out

    def rule_errors(self, n_rules: int) -> List[int]:
        """Per caller rule: requests (over every batch so far) for which the rule's evaluation ended in an execution error — what the
        reference logs per occurrence (pingoo/rules.rs:41-45). Static errors are creation-time warnings instead."""
        arr = (C.c_uint64 * n_rules)()
        _check(lib().pwaf_engine_rule_errors(self._h, arr, n_rules))
        return list(arr)

    def stats(self) -> dict:
        s = _abi.Stats()
        lib().pwaf_engine_stats(self._h, C.byref(s))
        return {k: getattr(s, k) for k, _ in _abi.Stats._fields_ if k != "reserved"}

    # ---- evaluation -------------------------------------------------------------------------------
    def evaluate_batch(self, batch: RequestBatch, with_counts: bool = False, out: Optional[np.ndarray] = None, with_geo: bool = False):
        """Host batch in, numpy VERDICT_DTYPE array out (and the 4 action counters when asked). `out`: a caller-owned result array
        (e.g. page-locked: PinnedVerdicts(n).array) instead of a fresh one per call. with_geo (OPT_GEO_ANSWERS engines): the GEO_DTYPE
        array of the requests' GeoIP records is appended to what is returned."""
        if out is None:
            out = np.zeros(batch.n, dtype=VERDICT_DTYPE)
        assert out.dtype == VERDICT_DTYPE and len(out) >= batch.n and out.flags["C_CONTIGUOUS"]
        counts = _abi.Counts()
        st = batch.as_struct(self.header_names)
        geo = np.zeros(batch.n, dtype=GEO_DTYPE) if with_geo else None
        if with_geo:
            rc = lib().pwaf_evaluate_batch_geo(self._h, C.byref(st), out.ctypes.data, C.addressof(counts), geo.ctypes.data)
        else:
            rc = lib().pwaf_evaluate_batch(self._h, C.byref(st), out.ctypes.data, C.addressof(counts))
        _check(rc)
        res = (out, np.array(list(counts.by_action), dtype=np.uint64)) if with_counts else (out,)
        res += (geo,) if with_geo else ()
        return res if len(res) > 1 else res[0]

    def evaluate_batch_routes(self, batch: RequestBatch, with_counts: bool = False):
        """Verdicts and service routes in one pass (engines created with routes=; pwaf_evaluate_batch_routes) -> (verdicts, routes[, counts]).
        routes: int32, the index of the first route whose expression is true for the request, -1 where none is (ServiceRouter's
        convention). It is answered for every request whatever its verdict; the reference routes only what it lets through."""
        out = np.zeros(batch.n, dtype=VERDICT_DTYPE)
        route = np.full(max(1, batch.n), _abi.ROUTE_NONE, dtype=np.uint32)
        counts = _abi.Counts()
        st = batch.as_struct(self.header_names)
        _check(lib().pwaf_evaluate_batch_routes(self._h, C.byref(st), out.ctypes.data, C.addressof(counts), route.ctypes.data))
        res = (out, route[:batch.n].view(np.int32))
        return res + (np.array(list(counts.by_action), dtype=np.uint64),) if with_counts else res

    def evaluate_routed(self, request: Request) -> Tuple[Verdict, int]:
        """One request -> (Verdict, route index or -1) (pwaf_evaluate_one_route; engines created with routes=)."""
        st, _keep = _request_struct(request, self.header_names)
        out = _abi.Verdict()
        route = C.c_uint32(_abi.ROUTE_NONE)
        _check(lib().pwaf_evaluate_one_route(self._h, C.byref(st), C.byref(out), C.byref(route)))
        return verdict_from_record({"action": out.action, "rule_idx": out.rule_idx}), (-1 if route.value == _abi.ROUTE_NONE else int(route.value))

    def evaluate_batch_hits_into(self, batch: RequestBatch, hits: Optional[np.ndarray], cap: int = 0, with_rule_hits: bool = True):
        """pwaf_evaluate_batch_hits as it is (OPT_RULE_HITS engines): `hits` = a caller-owned RULE_HIT_DTYPE array of which at most `cap`
        entries are written (None: no list) -> (verdicts, counts, n_hits or None, rule_hits or None). n_hits > cap: the list is incomplete."""
        out = np.zeros(batch.n, dtype=VERDICT_DTYPE)
        counts = _abi.Counts()
        n_hits = C.c_uint32(0)
        if hits is not None:
            assert hits.dtype == RULE_HIT_DTYPE and hits.flags["C_CONTIGUOUS"] and len(hits) >= cap
        rule_hits = np.zeros(max(1, len(self.rules)), dtype=np.uint64) if with_rule_hits else None
        st = batch.as_struct(self.header_names)
        rc = lib().pwaf_evaluate_batch_hits(self._h, C.byref(st), out.ctypes.data, C.addressof(counts), None if hits is None else max(hits.ctypes.data, 1), cap,
                                            None if hits is None else C.addressof(n_hits), None if rule_hits is None else rule_hits.ctypes.data)
        _check(rc)
        return (out, np.array(list(counts.by_action), dtype=np.uint64), None if hits is None else int(n_hits.value),
                None if rule_hits is None else rule_hits[:len(self.rules)])

    def evaluate_batch_hits(self, batch: RequestBatch, with_counts: bool = False, cap: Optional[int] = None):
        """Every rule that matches, not only the deciding one (OPT_RULE_HITS engines): -> (verdicts, hits, rule_hits[, counts]). hits = the
        RULE_HIT_DTYPE list, one entry per (rule, group of 64 requests) with a non-zero match word, in no particular order
        (batch.hits_to_matrix turns it into bool[n_rules, n]); rule_hits[k] = the requests rule k matches. Gated requests match nothing.
        cap: entries to make room for at first; a list that did not fit is fetched again, once, with the size the engine reported."""
        if cap is None:
            cap = max(1024, 8 * ((batch.n + 63) // 64))
        for _ in range(2):
            hits = np.zeros(max(1, cap), dtype=RULE_HIT_DTYPE)
            out, counts, n_hits, rule_hits = self.evaluate_batch_hits_into(batch, hits, cap)
            if n_hits <= cap:
                break
            cap = n_hits
        assert n_hits <= cap
        res = (out, hits[:n_hits], rule_hits)
        return res + (counts,) if with_counts else res

    def evaluate_records(self, buf: np.ndarray, rec_off: np.ndarray, with_counts: bool = False, with_geo: bool = False):
        """Request records (RequestBatch.to_records, include/pwaf.h pwaf_record_head) in, VERDICT_DTYPE array out: verdict i belongs to the
        record at buf[rec_off[i]] (pwaf_evaluate_records). `buf` may be page-locked (pwaf_host_alloc / _register) or not."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint32)
        out = np.zeros(len(rec_off), dtype=VERDICT_DTYPE)
        counts = _abi.Counts()
        geo = np.zeros(len(rec_off), dtype=GEO_DTYPE) if with_geo else None
        if with_geo:  # (OPT_GEO_ANSWERS engines: the records' GeoIP answers, appended to what is returned)
            rc = lib().pwaf_evaluate_records_geo(self._h, buf.ctypes.data, buf.nbytes, rec_off.ctypes.data, len(rec_off), out.ctypes.data, C.addressof(counts), geo.ctypes.data)
        else:
            rc = lib().pwaf_evaluate_records(self._h, buf.ctypes.data, buf.nbytes, rec_off.ctypes.data, len(rec_off), out.ctypes.data, C.addressof(counts))
        _check(rc)
        res = (out, np.array(list(counts.by_action), dtype=np.uint64)) if with_counts else (out,)
        res += (geo,) if with_geo else ()
        return res if len(res) > 1 else res[0]

    def export_records(self, batch, idx, n_idx=None, cap=None, stream=None):
        """export_records (below) with this engine's header columns: the records are what evaluate_records of this engine takes."""
        return export_records(batch, idx, n_idx=n_idx, cap=cap, stream=stream, header_names=self.header_names)

    def evaluate_records_device(self, buf, rec_off, n_rec=None, out=None, counts=None, match_idx=None, n_matches=None, stream=None):
        """Request records that lie in device memory (pwaf_evaluate_records_device): `buf` a uint8 device tensor of exactly the records'
        bytes (16-byte aligned, no pad), `rec_off` a 32-bit device tensor — request i is the record at buf[rec_off[i]] —, `n_rec` a
        one-element 32-bit device tensor or None: min(n_rec, len(rec_off)) records are evaluated (export_records' stats tensor viewed as
        int32 holds n_written at [3:4]). Validation runs on the device; a malformed call raises PwafError with pwaf_evaluate_records' text
        and leaves every output untouched. The call waits for the stream once (for the column sizes), enqueues the rest on torch's current
        stream (or `stream`) and returns `out` ((n, 2) int32; rows past the evaluated records are not written). counts / n_matches
        ACCUMULATE: zero them first."""
        import torch

        assert buf.is_contiguous() and buf.element_size() == 1 and rec_off.is_contiguous() and rec_off.element_size() == 4
        assert n_rec is None or (n_rec.element_size() == 4 and n_rec.numel() >= 1)
        n = rec_off.numel()
        if out is None:
            out = torch.empty((n, 2), dtype=torch.int32, device=buf.device)
        if stream is None:
            stream = torch.cuda.current_stream(buf.device).cuda_stream
        rc = lib().pwaf_evaluate_records_device(self._h, buf.data_ptr() if buf.numel() else None, buf.numel(), rec_off.data_ptr() if n else None, n,
                                                None if n_rec is None else n_rec.data_ptr(), out.data_ptr(), None if counts is None else counts.data_ptr(),
                                                None if match_idx is None else match_idx.data_ptr(), None if n_matches is None else n_matches.data_ptr(),
                                                C.c_void_p(stream))
        _check(rc)
        return out

    def client_ids(self, batch, idx=None, n_idx=None, stream=None):
        """client_ids (below): the captcha client ids of the requests of `batch` that `idx` names; needs nothing of the engine."""
        return client_ids(batch, idx=idx, n_idx=n_idx, stream=stream)

    def verify_cookies(self, keyset, batch, cookies, now, idx=None, n_idx=None, flags_out=None, stream=None):
        """verify_cookies (below): gate C for the requests of `batch`; needs nothing of the engine."""
        return verify_cookies(keyset, batch, cookies, now, idx=idx, n_idx=n_idx, flags_out=flags_out, stream=stream)

    def verify_cookie(self, keyset, request, cookie, now):
        """verify_cookie (below): gate C for one request, on the host; needs nothing of the engine."""
        return verify_cookie(keyset, request, cookie, now)

    def verify_pow(self, keyset, batch, cookies, hashes, nonces, now, idx=None, n_idx=None, stream=None):
        """verify_pow (below): the proof-of-work check for the requests of `batch`; needs nothing of the engine."""
        return verify_pow(keyset, batch, cookies, hashes, nonces, now, idx=idx, n_idx=n_idx, stream=stream)

    def verify_pow_one(self, keyset, request, cookie, hash, nonce, now):
        """verify_pow_one (below): the proof-of-work check for one request, on the host; needs nothing of the engine."""
        return verify_pow_one(keyset, request, cookie, hash, nonce, now)

    def parse_pow_bodies(self, bodies, n=None, idx=None, n_idx=None, stream=None, cap=None):
        """parse_pow_bodies (below): hash and nonce out of proof-of-work request bodies, as verify_pow takes them; needs nothing of the engine."""
        return parse_pow_bodies(bodies, n=n, idx=idx, n_idx=n_idx, stream=stream, cap=cap)

    def parse_pow_body_one(self, body):
        """parse_pow_body_one (below): one proof-of-work request body, on the host; needs nothing of the engine."""
        return parse_pow_body_one(body)

    def respond(self, batch, verdicts, cookie_status=None, route=None, lists=(), caps=None, stream=None):
        """respond (below): which response each request of a batch gets, and the lists the follow-up calls take; needs nothing of the engine."""
        return respond(batch, verdicts, cookie_status=cookie_status, route=route, lists=lists, caps=caps, stream=stream)

    def derive_batch(self, batch, uri_host=None, present=None, stream=None):
        """derive_batch (below): the derived host, path and user_agent columns of a raw batch; needs nothing of the engine."""
        return derive_batch(batch, uri_host=uri_host, present=present, stream=stream)

    def evaluate(self, request: Request, with_geo: bool = False):
        """RuleEngine::evaluate(Request) -> Action (pwaf_evaluate_one): a batch of one through the same device path. with_geo
        (OPT_GEO_ANSWERS engines): -> (Verdict, (asn, country)) — the reference's (Action, GeoipRecord)."""
        st, _keep = _request_struct(request, self.header_names)
        out = _abi.Verdict()
        geo = _abi.Geo()
        if with_geo:
            rc = lib().pwaf_evaluate_one_geo(self._h, C.byref(st), C.byref(out), C.byref(geo))
        else:
            rc = lib().pwaf_evaluate_one(self._h, C.byref(st), C.byref(out))
        _check(rc)
        v = verdict_from_record({"action": out.action, "rule_idx": out.rule_idx})
        return (v, (int(geo.asn), bytes(geo.country).decode("latin-1"))) if with_geo else v

    def evaluate_device(self, dbatch: "DeviceBatch", out=None, counts=None, match_idx=None, n_matches=None, stream=None, geo=None, hits=None, n_hits=None,
                        rule_hits=None, hits_cap=None, route=None):
        """Device-resident evaluation on torch's current stream (or `stream`). Tensors stay on the GPU. geo (OPT_GEO_ANSWERS engines): a
        device tensor of n x 8 bytes that receives the requests' GeoIP records (pwaf_geo). hits / n_hits / rule_hits (OPT_RULE_HITS engines;
        not together with geo): device tensors for the rule-hit list (16 bytes per entry, RULE_HIT_DTYPE; hits_cap entries, default: all
        the tensor holds), its 32-bit entry counter and the n_rules 64-bit per-rule counters — the counters ACCUMULATE: zero them first.
        route (engines created with routes=; not together with geo or the hit outputs): a device tensor of n 32-bit words that receives
        each request's first matching route (as int32: -1 where none matches)."""
        import torch

        if out is None:
            out = torch.empty((dbatch.n, 2), dtype=torch.int32, device=dbatch.device)
        if stream is None:
            stream = torch.cuda.current_stream(dbatch.device).cuda_stream
        st = dbatch.as_struct(self.header_names)
        args = (self._h, C.byref(st), out.data_ptr(), counts.data_ptr() if counts is not None else None,
                match_idx.data_ptr() if match_idx is not None else None, n_matches.data_ptr() if n_matches is not None else None)
        if route is not None:
            assert geo is None and hits is None and n_hits is None and rule_hits is None, "the _routes, _geo and _hits entry points are separate calls"
            assert route.is_contiguous() and route.numel() * route.element_size() >= 4 * dbatch.n
            rc = lib().pwaf_evaluate_device_routes(*args, route.data_ptr(), C.c_void_p(stream))
        elif hits is not None or n_hits is not None or rule_hits is not None:
            assert geo is None, "the _geo and _hits entry points are separate calls"
            room = 0 if hits is None else hits.numel() * hits.element_size() // RULE_HIT_DTYPE.itemsize
            cap = room if hits_cap is None else int(hits_cap)
            assert hits is None or (hits.is_contiguous() and cap <= room)
            assert rule_hits is None or (rule_hits.is_contiguous() and rule_hits.numel() * rule_hits.element_size() >= 8 * len(self.rules))
            # (a list of no entries still needs a non-NULL pointer beside n_hits: a count-only query)
            rc = lib().pwaf_evaluate_device_hits(*args, None if hits is None else max(hits.data_ptr(), 1), cap, None if n_hits is None else n_hits.data_ptr(),
                                                 None if rule_hits is None else rule_hits.data_ptr(), C.c_void_p(stream))
        elif geo is not None:
            assert geo.is_contiguous() and geo.numel() * geo.element_size() >= dbatch.n * GEO_DTYPE.itemsize
            rc = lib().pwaf_evaluate_device_geo(*args, geo.data_ptr(), C.c_void_p(stream))
        else:
            rc = lib().pwaf_evaluate_device(*args, C.c_void_p(stream))
        _check(rc)
        return out

    def device_status(self) -> None:
        """Synchronises and raises if the last device-resident batch ran out of scan scratch."""
        _check(lib().pwaf_engine_device_status(self._h))

    def tune(self, sample: RequestBatch) -> None:
        """Re-selects the LDS-resident DFA rows from a host traffic sample (speed only; verdicts never change)."""
        st = sample.as_struct(self.header_names)
        _check(lib().pwaf_engine_tune(self._h, C.byref(st)))

    def set_profiling(self, on):
        """False / 0: off; True / 1: HIP events around every kernel; 2: only around the launches that stream the request bytes."""
        lib().pwaf_engine_set_profiling(self._h, int(on))

    def kernel_times(self) -> List[Tuple[str, float, int]]:
        arr = (_abi.KernelTime * 8192)()
        n = lib().pwaf_engine_kernel_times(self._h, arr, 8192)
        if n < 0:
            _check(n)
        return [(arr[i].name.decode(), float(arr[i].ms), int(arr[i].alg_bytes)) for i in range(n)]


class NodeEngine:
    """One process driving several GPUs (pwaf_node_*): an engine replica per device, host batches cut into 64-aligned slabs, one host
    thread and stream per device, action counters summed on the host. The single-process counterpart of bench.py's rank-per-GPU mode."""

    def __init__(self, rules, lists=None, geoip=None, devices: Sequence[int] = (0,), **opts):
        L = lib()
        m = _abi.Marshalled()
        r, nr = _abi.marshal_rules(_norm_rules(rules), m)
        l, nl = _abi.marshal_lists(lists, m)
        g = _abi.marshal_geoip(geoip, m)
        o = _options(**opts)
        h = C.c_void_p()
        err = _abi.CompileError()
        devs = (C.c_int * len(devices))(*devices)
        rc = L.pwaf_node_create(r, nr, l, nl, g, C.byref(o), devs, len(devices), C.byref(h), C.byref(err))
        if rc < 0:
            _check(rc, err.message.decode(errors="replace"), None if err.rule_index == 0xFFFFFFFF else err.rule_index)
        self.partial = rc == _abi.W_PARTIAL  # PWAF_OPT_LENIENT dropped a rule (see the program's rule status / warnings)
        self._h = h
        e0 = L.pwaf_node_engine(h, 0)
        self.header_names = [L.pwaf_engine_header_name(e0, i).decode() for i in range(L.pwaf_engine_header_count(e0))]
        self.n_devices = L.pwaf_node_device_count(h)

    def evaluate_batch(self, batch: RequestBatch, with_counts: bool = False):
        out = np.zeros(batch.n, dtype=VERDICT_DTYPE)
        counts = _abi.Counts()
        st = batch.as_struct(self.header_names)
        _check(lib().pwaf_node_evaluate_batch(self._h, C.byref(st), out.ctypes.data, C.addressof(counts)))
        return (out, np.array(list(counts.by_action), dtype=np.uint64)) if with_counts else out

    def evaluate_device(self, dbatches, outs, counts=None, streams=None) -> None:
        """pwaf_node_evaluate_device: one DEVICE-resident slab per device of the node (DeviceBatch list), verdict tensors `outs`
        ((n_r, 2) int32 on device r), optional per-device int64[4] counter tensors (accumulated into). Asynchronous: call
        synchronize() before reading."""
        k = len(dbatches)
        structs = [b.as_struct(self.header_names) for b in dbatches]
        arr = (C.POINTER(_abi.Batch) * k)(*[C.pointer(s) for s in structs])
        o = (C.c_void_p * k)(*[t.data_ptr() for t in outs])
        c = (C.c_void_p * k)(*[t.data_ptr() for t in counts]) if counts is not None else None
        st = (C.c_void_p * k)(*[int(x) for x in streams]) if streams is not None else None
        _check(lib().pwaf_node_evaluate_device(self._h, arr, o, c, st))

    def allreduce_counts(self, comms, counts, streams=None) -> None:
        """pwaf_node_allreduce_counts: the per-device int64[4] counter tensors summed in place over RCCL; `comms` = one ncclComm_t
        (integer handle) per device, e.g. from ncclCommInitAll."""
        k = len(counts)
        cm = (C.c_void_p * k)(*[int(x) for x in comms])
        c = (C.c_void_p * k)(*[t.data_ptr() for t in counts])
        st = (C.c_void_p * k)(*[int(x) for x in streams]) if streams is not None else None
        _check(lib().pwaf_node_allreduce_counts(self._h, cm, c, st))

    def synchronize(self) -> None:
        _check(lib().pwaf_node_synchronize(self._h))

    def tune(self, sample: RequestBatch) -> None:
        st = sample.as_struct(self.header_names)
        _check(lib().pwaf_node_tune(self._h, C.byref(st)))

    def close(self):
        if getattr(self, "_h", None):
            lib().pwaf_node_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class PinnedVerdicts:
    """A page-locked verdict array (pwaf_host_alloc) for RuleEngine.evaluate_batch(out=...): the device-to-host copy of the results
    lands in it directly. `.array` is the numpy view; free() releases the memory (the view must not be used afterwards)."""

    def __init__(self, n: int):
        p = C.c_void_p()
        nbytes = max(1, n) * VERDICT_DTYPE.itemsize
        _check(lib().pwaf_host_alloc(nbytes, C.byref(p)))
        self._p = p
        self.array = np.frombuffer((C.c_uint8 * nbytes).from_address(p.value), dtype=VERDICT_DTYPE, count=n)

    def free(self) -> None:
        if self._p:
            self.array = None
            lib().pwaf_host_free(self._p)
            self._p = None


def node_shard_bounds(n: int, rank: int, world: int) -> Tuple[int, int]:
    lo, hi = C.c_uint32(), C.c_uint32()
    lib().pwaf_node_shard_bounds(n, rank, world, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


class ServiceRouter:
    """Service selection on the same engine: the reference walks `services` in order and hands the request to the
    first one whose `route:` expression is true — or has none (http_listener.rs:266-271, http_proxy_service.rs:84-95: same language,
    same context, error / non-bool = no match). That is first-match-wins over one expression per service, i.e. a rule set whose rule
    k 'blocks' with rule index k: no new device code, just an engine without the two request gates.
    `route_batch` -> int32 array: index of the selected service, -1 = none (the reference answers 404).
    For route-only callers. A host that wants the verdict AND the service creates ONE engine with both —
    RuleEngine(rules, lists, geoip, routes=[...]).evaluate_batch_routes(batch) -> (verdicts, routes) — which answers the same routes in
    the verdict's own pass: no second pipeline, no second set of tables."""

    def __init__(self, routes: Sequence[Tuple[str, Optional[str]]], lists=None, geoip=None, **opts):
        rules = [(name, expr, [_abi.RULE_ACTION_BLOCK]) for name, expr in routes]
        self._engine = RuleEngine(rules, lists or {}, geoip, flags=_abi.OPT_NO_UA_GATE | _abi.OPT_NO_CAPTCHA_BYPASS, **opts)

    def route_batch(self, batch: RequestBatch) -> np.ndarray:
        v = self._engine.evaluate_batch(batch)
        return np.where(v["action"] == _abi.ACTION_BLOCK, v["rule_idx"].astype(np.int64), -1).astype(np.int32)

    def close(self):
        self._engine.close()


def _request_struct(r: Request, header_names: Sequence[str] = ()):
    """pwaf_request for one Request; returns (struct, keepalive) — the byte strings must outlive the call. header_names = the engine's
    header columns: the request's values are handed over in that order (an absent header reads as "")."""
    from .batch import ip_to_bytes16

    fields = [x.encode() if isinstance(x, str) else bytes(x) for x in (r.host, r.url, r.path, r.method, r.user_agent)]
    st = _abi.Request()
    for name, b in zip(("host", "url", "path", "method", "user_agent"), fields):
        setattr(st, name, b)
        setattr(st, name + "_len", len(b))
    ip, v6 = ip_to_bytes16(r.ip)
    C.memmove(st.ip, ip, 16)
    st.ip_is_v6 = int(v6)
    st.flags = _abi.FLAG_CAPTCHA_VERIFIED if r.captcha_verified else 0
    st.port = r.remote_port
    if r.asn is not None and r.country is not None:
        st.has_geoip = 1
        cc = r.country.encode() if isinstance(r.country, str) else bytes(r.country)
        st.country[0], st.country[1] = cc[0], cc[1]
        st.asn = r.asn
    keep = [fields]
    if header_names:
        spans = (_abi.Span * len(header_names))()
        vals = []
        for k, name in enumerate(header_names):
            v = (r.headers or {}).get(name)
            if v is None:
                continue
            v = v.encode() if isinstance(v, str) else bytes(v)
            vals.append(v)
            spans[k].data = v
            spans[k].len = len(v)
        st.n_headers = len(header_names)
        st.headers = C.cast(spans, C.c_void_p)
        keep += [spans, vals]
    return st, keep


class MicroBatcher:
    """Deadline micro-batcher over a RuleEngine (pwaf_batcher_*): `evaluate(Request)` blocks until the request's batch — closed at
    `max_batch` requests or after `max_delay_us` — has been evaluated on the GPU. Safe to call from many threads (ctypes drops the GIL)."""

    def __init__(self, engine: "RuleEngine", max_batch: int = 4096, max_delay_us: int = 200):
        self._engine = engine  # keeps the engine alive
        h = C.c_void_p()
        _check(lib().pwaf_batcher_create(engine._h, max_batch, max_delay_us, C.byref(h)))
        self._h = h

    def evaluate(self, request: Request) -> Verdict:
        st, _keep = _request_struct(request, self._engine.header_names)
        out = _abi.Verdict()
        _check(lib().pwaf_batcher_evaluate(self._h, C.byref(st), C.byref(out)))
        return verdict_from_record({"action": out.action, "rule_idx": out.rule_idx})

    def stats(self) -> Tuple[int, int]:
        nb, nr = C.c_uint64(0), C.c_uint64(0)
        lib().pwaf_batcher_stats(self._h, C.byref(nb), C.byref(nr))
        return nb.value, nr.value

    def close(self):
        if self._h:
            lib().pwaf_batcher_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def native_batcher_latency(engine: "RuleEngine", batch: RequestBatch, threads: int = 64, per_thread: int = 150, max_batch: int = 4096, max_delay_us: int = 200, pool: int = 256) -> dict:
    """Per-request latency through the deadline micro-batcher as a NATIVE host sees it: tools/libbatcher_bench.so (C++, `threads`
    std::threads calling pwaf_batcher_evaluate back to back over the first `pool` requests of `batch`). Measurement only."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "libbatcher_bench.so")
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing (built by __graft_entry__.build())")
    bb = C.CDLL(path)
    bb.bb_run.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.Request), C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_double)]
    pool = min(pool, batch.n)
    reqs = (_abi.Request * pool)()
    keep = []
    names = engine.header_names
    for i in range(pool):
        hdrs = {h: batch.header_bytes(h, i) for h in names} if names else None
        r = Request(host=batch.field_bytes(0, i), url=batch.field_bytes(1, i), path=batch.field_bytes(2, i), method=batch.field_bytes(3, i), user_agent=batch.field_bytes(4, i),
                    ip="203.0.113.%d" % (i % 250 + 1), remote_port=int(batch.port[i]), headers=hdrs)
        st, k = _request_struct(r, names)
        reqs[i] = st
        keep.append(k)
    mb = MicroBatcher(engine, max_batch=max_batch, max_delay_us=max_delay_us)
    n = threads * per_thread
    lat = (C.c_double * n)()
    secs = C.c_double(0)
    fn = C.cast(lib().pwaf_batcher_evaluate, C.c_void_p)
    failed = bb.bb_run(fn, mb._h, reqs, pool, threads, per_thread, lat, None, C.byref(secs))
    nb, nr = mb.stats()
    mb.close()
    xs = sorted(lat)
    pct = lambda p: xs[min(n - 1, int(round(p / 100.0 * (n - 1))))]  # noqa: E731
    return {"caller_threads": threads, "callers": "native (std::thread, tools/batcher_bench.cpp)", "requests": n, "failed": failed, "max_batch": max_batch, "deadline_us": max_delay_us,
            "batches": nb, "requests_per_s": n / secs.value if secs.value > 0 else 0.0, "latency_ms": {"p50": pct(50), "p99": pct(99), "max": xs[-1]}}


class AsyncBatcher:
    """Non-blocking request queue over a RuleEngine (pwaf_async_*): `submit(request, tag)` queues a request and returns at once (False:
    the queue is full — pwaf_async_submit's PWAF_E_BUSY — nothing was queued); `poll(cap)` hands out finished requests as (tag, Verdict,
    status) tuples. Wait for `fileno()` to be readable (select / an event loop), read it (`drain_fd()`), then poll until it returns [].
    Safe from many threads (ctypes drops the GIL)."""

    def __init__(self, engine: "RuleEngine", max_batch: int = 4096, max_delay_us: int = 200, max_in_flight: int = 65536, geo: bool = False):
        self._engine = engine  # keeps the engine alive
        self._geo = geo  # pwaf_async_create_geo (OPT_GEO_ANSWERS engines): completions carry the request's GeoIP record
        h = C.c_void_p()
        _check((lib().pwaf_async_create_geo if geo else lib().pwaf_async_create)(engine._h, max_batch, max_delay_us, max_in_flight, C.byref(h)))
        self._h = h

    def submit(self, request: Request, tag: int) -> bool:
        st, _keep = _request_struct(request, self._engine.header_names)
        rc = lib().pwaf_async_submit(self._h, C.byref(st), tag)
        if rc == _abi.E_BUSY:
            return False
        _check(rc)
        return True

    def poll(self, cap: int = 4096, with_geo: bool = False):
        """-> [(tag, Verdict, status)]; with_geo (a queue made with geo=True): [(tag, Verdict, status, (asn, country))]"""
        arr = (_abi.Completion * cap)()
        if with_geo:
            garr = (_abi.Geo * cap)()
            k = lib().pwaf_async_poll_geo(self._h, arr, garr, cap)
            if k == 0 and not self._geo:
                _check(_abi.E_UNSUPPORTED)
            return [(arr[i].tag, verdict_from_record({"action": arr[i].verdict.action, "rule_idx": arr[i].verdict.rule_idx}), arr[i].status,
                     (int(garr[i].asn), bytes(garr[i].country).decode("latin-1"))) for i in range(k)]
        k = lib().pwaf_async_poll(self._h, arr, cap)
        return [(arr[i].tag, verdict_from_record({"action": arr[i].verdict.action, "rule_idx": arr[i].verdict.rule_idx}), arr[i].status) for i in range(k)]

    def fileno(self) -> int:
        return lib().pwaf_async_fd(self._h)

    def drain_fd(self) -> None:
        """Reads the eventfd (resets its counter); a no-op when nothing was signalled."""
        try:
            os.read(self.fileno(), 8)
        except BlockingIOError:
            pass

    def flush(self) -> None:
        lib().pwaf_async_flush(self._h)

    def stats(self) -> Tuple[int, int, int]:
        """(batches evaluated, requests evaluated, requests submitted and not yet polled)."""
        nb, nr, fl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        lib().pwaf_async_stats(self._h, C.byref(nb), C.byref(nr), C.byref(fl))
        return nb.value, nr.value, fl.value

    def close(self):
        """Refuses new submits, evaluates every accepted request and frees the queue (completions nobody polled are dropped)."""
        if self._h:
            lib().pwaf_async_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _native_requests(engine: "RuleEngine", batch: RequestBatch, pool: int):
    """The first `pool` requests of `batch` as pwaf_request structs (with the engine's header values) + what keeps their bytes alive."""
    pool = min(pool, batch.n)
    reqs = (_abi.Request * pool)()
    keep = []
    names = engine.header_names
    for i in range(pool):
        hdrs = {h: batch.header_bytes(h, i) for h in names} if names else None
        geo = {} if batch.asn is None else {"asn": int(batch.asn[i]), "country": int(batch.country[i]).to_bytes(2, "little").decode("latin-1")}
        ipb = bytes(batch.ip[i])
        ip = str(ipaddress.ip_address(ipb if batch.ip_is_v6[i] else ipb[:4]))
        r = Request(host=batch.field_bytes(0, i), url=batch.field_bytes(1, i), path=batch.field_bytes(2, i), method=batch.field_bytes(3, i), user_agent=batch.field_bytes(4, i),
                    ip=ip, remote_port=int(batch.port[i]), captcha_verified=bool(batch.flags[i] & _abi.FLAG_CAPTCHA_VERIFIED), headers=hdrs, **geo)
        st, k = _request_struct(r, names)
        reqs[i] = st
        keep.append(k)
    return reqs, keep


def native_async_throughput(engine: "RuleEngine", batch: RequestBatch, threads: int = 4, in_flight: int = 2048, per_thread: int = 200_000, max_batch: int = 8192,
                            max_delay_us: int = 200, pool: int = 4096) -> dict:
    """Requests/s and submit->completion latency through the non-blocking queue as a NATIVE host sees it: tools/libasync_bench.so (C++,
    built on first use: `threads` submitter threads keeping `in_flight` requests each in flight over the first `pool` requests of `batch`,
    one poller on the eventfd). Every verdict is checked against pwaf_evaluate_batch on the same requests. Measurement only."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, path = os.path.join(root, "tools", "async_bench.cpp"), os.path.join(root, "tools", "libasync_bench.so")
    if not os.path.exists(path) or os.path.getmtime(src) > os.path.getmtime(path):
        import subprocess

        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-I", os.path.join(root, "include"), src, "-o", path], check=True)
    ab = C.CDLL(path)
    ab.ab_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_abi.Request), C.c_size_t, C.POINTER(_abi.Verdict), C.c_int, C.c_int, C.c_uint64,
                          C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]
    reqs, _keep = _native_requests(engine, batch, pool)
    n = len(reqs)
    sub = batch.slice(0, n)
    want = engine.evaluate_batch(sub)
    wv = (_abi.Verdict * n)()
    C.memmove(wv, want.ctypes.data, n * C.sizeof(_abi.Verdict))
    out = C.create_string_buffer(4096)
    L = lib()
    fns = (C.c_void_p * 7)(*[C.cast(getattr(L, f), C.c_void_p).value for f in ("pwaf_async_create", "pwaf_async_submit", "pwaf_async_poll", "pwaf_async_fd",
                                                                                 "pwaf_async_flush", "pwaf_async_stats", "pwaf_async_destroy")])
    # a short unmeasured run first: the engine's per-call contexts grow their device and page-locked buffers to the batch sizes the queue makes
    ab.ab_run(fns, engine._h, None, reqs, n, wv, threads, in_flight, min(per_thread, 20_000), max_batch, max_delay_us, out, len(out))
    rc = ab.ab_run(fns, engine._h, None, reqs, n, wv, threads, in_flight, per_thread, max_batch, max_delay_us, out, len(out))
    import json

    res = json.loads(out.value.decode())
    res["rc"] = rc
    return res


def geoip_from_mmdb(content: bytes, path: str = "geoip.mmdb") -> np.ndarray:
    """MaxMind DB file content -> GEOIP_DTYPE prefix table for RuleEngine(..., geoip=...) (pingoo/geoip.rs:43-91). A `path` ending in
    ".zst" means the content is ZSTD-compressed (geoip.rs:49-55)."""
    from .batch import GEOIP_DTYPE

    ptr, n = C.POINTER(_abi.GeoipEntry)(), C.c_size_t(0)
    _check(lib().pwaf_geoip_from_file_image(path.encode(), content, len(content), C.byref(ptr), C.byref(n)))
    try:
        out = np.zeros(n.value, dtype=GEOIP_DTYPE)
        if n.value:
            C.memmove(out.ctypes.data, ptr, n.value * GEOIP_DTYPE.itemsize)
    finally:
        lib().pwaf_geoip_free(ptr)
    return out


def zstd_decompress(data: bytes) -> bytes:
    out, n = C.c_void_p(), C.c_size_t(0)
    _check(lib().pwaf_zstd_decompress(data, len(data), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value)
    finally:
        lib().pwaf_buffer_free(out)


def parse_list_csv(text) -> List[str]:
    """List file content -> items (pingoo/lists.rs:62-117: CSV, no header, 1-2 columns, first column trimmed)."""
    raw = text.encode() if isinstance(text, str) else bytes(text)
    items, n = C.POINTER(C.c_char_p)(), C.c_size_t(0)
    _check(lib().pwaf_list_parse_csv(raw, len(raw), C.byref(items), C.byref(n)))
    try:
        return [items[k].decode(errors="surrogateescape") for k in range(n.value)]
    finally:
        lib().pwaf_list_free(items, n.value)


def export_stats(stats) -> dict:
    """The 16 bytes of a pwaf_export_stats (a device tensor once its stream is synchronised, a numpy array or bytes) -> {bytes_needed, n_selected, n_written}."""
    raw = stats.cpu().numpy().tobytes() if hasattr(stats, "cpu") else bytes(stats)
    s = _abi.ExportStats.from_buffer_copy(raw[:C.sizeof(_abi.ExportStats)])
    return {"bytes_needed": int(s.bytes_needed), "n_selected": int(s.n_selected), "n_written": int(s.n_written)}


def _aligned_bytes(nbytes: int) -> np.ndarray:
    """A zeroed uint8 array of nbytes at a 16-byte aligned address."""
    raw = np.zeros(nbytes + 16, dtype=np.uint8)
    at = -raw.ctypes.data % 16
    return raw[at:at + nbytes]


def _host_list(n: int, idx, n_idx):
    """The list arguments of a HOST-mode call over n requests -> (idx_ptr, idx_len, n_idx_ptr, m, keep). idx None: every request, a NULL
    idx and m = n. Else idx_len entries, of which m = min(idx_len, n_idx) count (n_idx clamps m here only: the library reads it itself);
    an empty list is not NULL, which would mean every request. `keep` owns what the pointers point at."""
    if idx is None:
        assert n_idx is None
        return None, 0, None, n, ()
    idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
    n_ref = None if n_idx is None else np.array([int(np.asarray(n_idx).reshape(-1)[0])], dtype=np.uint32)
    keep = idx if len(idx) else np.zeros(1, dtype=np.uint32)
    return keep.ctypes.data, len(idx), None if n_ref is None else n_ref.ctypes.data, len(idx) if n_ref is None else min(len(idx), int(n_ref[0])), (keep, n_ref)


def _device_list(n: int, idx, n_idx):
    """_host_list for device tensors: idx and n_idx (one element) are 32 bits wide and stay on the device, so m = idx_len."""
    if idx is None:
        assert n_idx is None
        return None, 0, None, n, ()
    import torch

    assert idx.is_contiguous() and idx.element_size() == 4 and (n_idx is None or n_idx.element_size() == 4)
    m = idx.numel()
    keep = idx if m else torch.zeros(1, dtype=torch.int32, device=idx.device)
    return keep.data_ptr(), m, None if n_idx is None else n_idx.data_ptr(), m, (keep, n_idx)


def _strcol(values, device=None):
    """A list of bytes | str | None, or a (data, offsets) pair -> (an _abi.StrCol, the (data, offsets) it points at) in host memory, or on
    `device` (a list is uploaded)."""
    col = _abi.StrCol()
    data, off = values if isinstance(values, tuple) else cookie_column(values)
    if device is None:
        data, off = np.ascontiguousarray(data, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint32)
        col.data, col.offsets = data.ctypes.data, off.ctypes.data
        return col, (data, off)
    import torch

    if not torch.is_tensor(off):
        data, off = torch.from_numpy(data).to(device), torch.from_numpy(off.view(np.int32)).to(device)
    assert data.is_contiguous() and off.is_contiguous() and off.element_size() == 4
    col.data, col.offsets = data.data_ptr(), off.data_ptr()
    return col, (data, off)


def _scan_shape(fn, fields) -> dict:
    out = (C.c_uint32 * 4)()
    _check(fn(out))
    return dict(zip(fields, (int(x) for x in out)))


def export_records(batch, idx, n_idx=None, cap=None, stream=None, header_names: Optional[Sequence[str]] = None):
    """The requests of `batch` that the list `idx` names, as request records (pwaf_export_records; include/pwaf.h) -> (buf, rec_off, stats):
    the record of request idx[j] starts at buf[rec_off[j]], or rec_off[j] == _abi.RECORD_NONE when it has none (it did not fit `cap`
    bytes, or idx[j] is not a request of the batch). Takes no engine; header_names = the header columns a record carries, in order
    (default: the batch's own; RuleEngine.export_records passes the engine's, so that its evaluate_records takes the records).
    RequestBatch: idx (and n_idx: how many entries of idx count, default all) are numpy arrays / ints, the call is synchronous and runs
    on the CPU; cap=None asks for the size first and exports everything. -> (uint8 array of bytes_needed bytes, uint32 array, dict).
    DeviceBatch: idx and n_idx (a one-element 32-bit tensor, or None) are device tensors — e.g. evaluate_device's match_idx / n_matches,
    in which case the call follows the evaluation on `stream` (default: torch's current stream) without a synchronisation in between. The
    work is enqueued and the call returns: -> (uint8 tensor of cap bytes, int32 tensor, a 16-byte tensor for export_stats()) to be read
    after the stream is synchronised. cap=None makes room for every request of the batch once, which a list without duplicates cannot
    exceed (at most 0xFFFFFFF0 bytes)."""
    names = list(batch.headers) if header_names is None else list(header_names)
    st = batch.as_struct(names)
    if isinstance(batch, RequestBatch):
        idx_ptr, n_list, n_ptr, _, keep = _host_list(batch.n, np.asarray(idx), n_idx)
        rec_off = np.full(max(1, n_list), _abi.RECORD_NONE, dtype=np.uint32)
        stats = _abi.ExportStats()

        def call(buf, nbytes):
            _check(lib().pwaf_export_records(C.byref(st), idx_ptr, n_list, n_ptr, None if buf is None else buf.ctypes.data, nbytes, rec_off.ctypes.data, C.addressof(stats), None))

        if cap is None:
            call(None, 0)
            cap = int(stats.bytes_needed)
        buf = _aligned_bytes(int(cap))
        call(buf, int(cap))
        res = {"bytes_needed": int(stats.bytes_needed), "n_selected": int(stats.n_selected), "n_written": int(stats.n_written)}
        del keep
        return buf[:min(int(cap), res["bytes_needed"])], rec_off[:n_list], res
    import torch

    assert idx.is_contiguous() and idx.element_size() == 4 and (n_idx is None or n_idx.element_size() == 4)
    n_list = idx.numel()
    if cap is None:
        per_record = (C.sizeof(_abi.RecordHead) + 4 * (_abi.N_FIELDS + len(names)) + 15 & ~15) + 15
        cap = sum(batch.field_bytes) + sum(batch.headers[nm][2] for nm in names if nm in batch.headers) + min(n_list, batch.n) * per_record
        cap = min(cap + 15 & ~15, 0xFFFFFFF0)
    if stream is None:
        stream = torch.cuda.current_stream(batch.device).cuda_stream
    buf = torch.empty(max(16, int(cap)), dtype=torch.uint8, device=batch.device)
    rec_off = torch.empty(max(1, n_list), dtype=torch.int32, device=batch.device)
    stats = torch.empty(16, dtype=torch.uint8, device=batch.device)
    rc = lib().pwaf_export_records(C.byref(st), idx.data_ptr() if n_list else None, n_list, None if n_idx is None else n_idx.data_ptr(), buf.data_ptr(), int(cap),
                                   rec_off.data_ptr(), stats.data_ptr(), C.c_void_p(stream))
    _check(rc)
    return buf[:int(cap)], rec_off[:n_list], stats


def client_ids(batch, idx=None, n_idx=None, stream=None):
    """The captcha client ids (generate_captcha_client_id, above) of requests of `batch` (pwaf_client_ids; include/pwaf.h): of every request
    when idx is None (entry i belongs to request i), else of the requests the list `idx` names (entry j belongs to request idx[j]; n_idx:
    how many entries of idx count, default all; an entry that names no request of the batch reads as ""). Takes no engine.
    RequestBatch: idx / n_idx are numpy arrays / ints, the call is synchronous and runs on the CPU -> a list of str.
    DeviceBatch: idx and n_idx (a one-element 32-bit tensor, or None) are device tensors — e.g. evaluate_device's match_idx / n_matches, in
    which case the call follows the evaluation on `stream` (default: torch's current stream) without a synchronisation in between. One
    launch is enqueued and the call returns: -> a (m, 44) uint8 tensor (43 characters and a NUL per entry; m = the entries of idx, or the
    batch's requests) to be read after the stream is synchronised; rows at or past n_idx are not written."""
    st = batch.as_struct()
    if isinstance(batch, RequestBatch):
        idx_ptr, n_list, n_ptr, m, keep = _host_list(batch.n, idx, n_idx)
        if idx is not None and not n_list:
            return []
        out = np.zeros((max(1, m), 44), dtype=np.uint8)
        _check(lib().pwaf_client_ids(C.byref(st), idx_ptr, n_list, n_ptr, out.ctypes.data, None))
        del keep
        return [row.tobytes().split(b"\0", 1)[0].decode("ascii") for row in out[:m]]
    import torch

    idx_ptr, n_list, n_ptr, m, _ = _device_list(batch.n, idx, n_idx)
    if stream is None:
        stream = torch.cuda.current_stream(batch.device).cuda_stream
    out = torch.empty((max(1, m), 44), dtype=torch.uint8, device=batch.device)
    if idx is not None and not m:
        return out[:0]
    _check(lib().pwaf_client_ids(C.byref(st), idx_ptr, n_list, n_ptr, out.data_ptr(), C.c_void_p(stream)))
    return out[:m]


class KeySet:
    """The captcha verifying keys (pwaf_keyset; the reference's CaptchaManager::verifying_keys, captcha.rs:77-123): `keys` is a sequence of
    (kid, x) with x the 32 bytes of an Ed25519 public key, e.g. config.load_captcha_jwks()'s. Creation decompresses each key, precomputes
    the multiples the verifier adds and, with a device, uploads them. device: None = host only (verify_cookies then takes RequestBatches
    and verify_cookie single requests); an ordinal, "cuda:N" or a torch.device = that GPU as well. Read-only afterwards: any number of
    calls on any streams may share it. close() (or the garbage collector) frees it, after the last call that uses it has run."""

    def __init__(self, keys, device=None):
        keys = [(kid.encode() if isinstance(kid, str) else bytes(kid), bytes(x)) for kid, x in keys]
        if device is None:
            ordinal = -1
        elif isinstance(device, int):
            ordinal = device
        else:
            import torch

            d = torch.device(device)
            ordinal = torch.cuda.current_device() if d.index is None else d.index
        arr = (_abi.Ed25519Key * max(1, len(keys)))()
        for k, (kid, x) in enumerate(keys):
            if len(x) != 32:
                raise ValueError(f"KeySet: key {k}: x has {len(x)} bytes, an Ed25519 public key has 32")
            if b"\0" in kid:
                raise ValueError(f"KeySet: key {k}: the kid contains a NUL byte")
            arr[k].kid = kid
            C.memmove(arr[k].x, x, 32)
        h = C.c_void_p()
        _check(lib().pwaf_keyset_create(arr, len(keys), ordinal, C.byref(h)))
        self._h, self.device, self.kids = h, ordinal, [kid.decode(errors="replace") for kid, _ in keys]

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().pwaf_keyset_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter shutdown: the library may be gone)
            pass


def cookie_column(cookies):
    """[bytes | str | None per request] (None: no Cookie header) -> (data with PWAF_ARENA_PAD zero bytes behind it, offsets) numpy arrays"""
    vals = [b"" if v is None else (v.encode() if isinstance(v, str) else bytes(v)) for v in cookies]
    off = np.zeros(len(vals) + 1, dtype=np.uint32)
    if vals:
        off[1:] = np.cumsum([len(v) for v in vals], dtype=np.uint64).astype(np.uint32)
    return np.frombuffer(b"".join(vals) + b"\0" * _abi.ARENA_PAD, dtype=np.uint8).copy(), off


def verify_cookies(keyset, batch, cookies, now, idx=None, n_idx=None, flags_out=None, stream=None):
    """Gate C of the reference (http_listener.rs:169-181, :222-236; captcha.rs:125-156; jwt.rs:198-327) for requests of `batch`
    (pwaf_verify_cookies; include/pwaf.h): one _abi.COOKIE_* status per request — of every request when idx is None (entry i belongs to
    request i), else of the requests the list `idx` names (n_idx: how many entries count; an entry that names no request reads ABSENT).
    cookies: each request's FIRST Cookie header value — a (data, offsets) pair where the batch lives, or a list of bytes | str | None.
    now: Unix seconds. flags_out (only with idx None): n bytes that receive the batch's flags with FLAG_CAPTCHA_VERIFIED set exactly for
    the VERIFIED requests; it may be the batch's own flags. Takes no engine.
    RequestBatch: numpy arguments, synchronous, on the CPU -> a numpy uint8 array.
    DeviceBatch: device tensors (a list of cookies is uploaded); a memset and two launches are enqueued on `stream` (default: torch's
    current stream, which must be the stream torch allocates on when the call is made: the scratch comes from its caching allocator) and
    the call returns -> a uint8 tensor to be read after the stream is synchronised; entries at or past n_idx are not written. With
    flags_out = batch.flags an evaluate_device on the same stream follows without a synchronisation by the caller."""
    st = batch.as_struct()
    if isinstance(batch, RequestBatch):
        col, cmem = _strcol(cookies)  # (cmem, like keep below, owns what the call reads)
        assert len(cmem[1]) == batch.n + 1
        idx_ptr, n_list, n_ptr, m, keep = _host_list(batch.n, idx, n_idx)
        if idx is not None and not n_list:
            return np.zeros(0, dtype=np.uint8)
        if flags_out is not None:
            assert isinstance(flags_out, np.ndarray) and flags_out.dtype == np.uint8 and flags_out.flags.c_contiguous and flags_out.size == batch.n
        out = np.zeros(max(1, m), dtype=np.uint8)
        _check(lib().pwaf_verify_cookies(keyset._h, C.byref(st), C.byref(col), int(now), idx_ptr, n_list, n_ptr, out.ctypes.data,
                                         None if flags_out is None else flags_out.ctypes.data, None, 0, None))
        del keep, cmem
        return out[:m]
    import torch

    col, cmem = _strcol(cookies, batch.device)
    assert len(cmem[1]) == batch.n + 1
    idx_ptr, n_list, n_ptr, m, _ = _device_list(batch.n, idx, n_idx)
    if flags_out is not None:
        assert flags_out.is_contiguous() and flags_out.element_size() == 1 and flags_out.numel() == batch.n
    if stream is None:
        stream = torch.cuda.current_stream(batch.device).cuda_stream
    out = torch.empty(max(1, m), dtype=torch.uint8, device=batch.device)
    if not m:
        return out[:0]
    need = int(lib().pwaf_verify_cookies_scratch_bytes(m))
    scratch = torch.empty(need, dtype=torch.uint8, device=batch.device)
    _check(lib().pwaf_verify_cookies(keyset._h, C.byref(st), C.byref(col), int(now), idx_ptr, n_list, n_ptr, out.data_ptr(), None if flags_out is None else flags_out.data_ptr(),
                                     scratch.data_ptr(), need, C.c_void_p(stream)))
    return out[:m]


def verify_cookie(keyset, request, cookie, now) -> int:
    """Gate C for one request on the host (pwaf_verify_cookie_one): `cookie` is the first Cookie header's value (bytes | str | None: no
    header) -> _abi.COOKIE_ABSENT / _VERIFIED / _INVALID / _UNDECIDED. What a per-request closure calls at http_listener.rs:222-236."""
    st, keep = _request_struct(request)
    c = None if cookie is None else (cookie.encode() if isinstance(cookie, str) else bytes(cookie))
    out = C.c_uint8(0xEE)
    rc = lib().pwaf_verify_cookie_one(keyset._h, C.byref(st), c, 0 if c is None else len(c), int(now), C.byref(out))
    del keep
    _check(rc)
    return int(out.value)


def pow_handed(status) -> int:
    """The diagnostic of a verify_pow call on a DeviceBatch: the number of entries that were handed to the signature stage (word 0 of the
    call's scratch, which the returned tensor keeps reachable as `status.pow_scratch`). Call it after the stream is synchronised."""
    scratch = getattr(status, "pow_scratch", None)
    return 0 if scratch is None else int(scratch[:4].cpu().numpy().view(np.uint32)[0])


def _hash_rows(hashes, n):
    """[32 bytes per request] | an (n, 32) uint8 array -> a C-contiguous (n, 32) numpy array"""
    if isinstance(hashes, np.ndarray):
        arr = np.ascontiguousarray(hashes, dtype=np.uint8).reshape(-1, 32)
    else:
        rows = [bytes(h) for h in hashes]
        assert all(len(h) == 32 for h in rows), "a proof-of-work hash has 32 bytes"
        arr = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 32).copy()
    assert len(arr) == n
    return arr


def verify_pow(keyset, batch, cookies, hashes, nonces, now, idx=None, n_idx=None, stream=None):
    """The check of CaptchaManager::api_verify (captcha.rs:241-333; jwt.rs:198-327) for proof-of-work submissions among the requests of
    `batch` (pwaf_verify_pow; include/pwaf.h): one _abi.POW_* status per request — of every request when idx is None, else of the requests
    the list `idx` names (n_idx: how many entries count; an entry that names no request reads ABSENT), e.g. the match_idx / n_matches of
    an evaluation, which lists the requests on /__pingoo/captcha/api/verify. cookies: as for verify_cookies. hashes: 32 bytes per request
    (a list of bytes or an (n, 32) uint8 array / tensor); nonces: a (data, offsets) column where the batch lives, or a list of
    bytes | str: CaptchaVerifyRequestBody after the host has parsed it. now: Unix seconds. PASSED means the host issues the verified
    cookie; that, and parsing the body, stay on the host. Takes no engine.
    RequestBatch: numpy arguments, synchronous, on the CPU -> a numpy uint8 array.
    DeviceBatch: device tensors (lists are uploaded); a memset and two launches are enqueued on `stream` (default: torch's current
    stream, from whose allocator the scratch comes) and the call returns -> a uint8 tensor to be read after the stream is
    synchronised (entries at or past n_idx are not written); it keeps the call's scratch reachable as `.pow_scratch`, whose word 0
    pow_handed(status) reads: the diagnostic."""
    st = batch.as_struct()
    if isinstance(batch, RequestBatch):
        (col, cmem), (ncol, nmem) = _strcol(cookies), _strcol(nonces)
        assert len(cmem[1]) == batch.n + 1 and len(nmem[1]) == batch.n + 1
        rows = _hash_rows(hashes, batch.n)
        hbuf = rows if batch.n else np.zeros((1, 32), dtype=np.uint8)
        idx_ptr, n_list, n_ptr, m, keep = _host_list(batch.n, idx, n_idx)
        if idx is not None and not n_list:
            return np.zeros(0, dtype=np.uint8)
        out = np.zeros(max(1, m), dtype=np.uint8)
        _check(lib().pwaf_verify_pow(keyset._h, C.byref(st), C.byref(col), hbuf.ctypes.data, C.byref(ncol), int(now), idx_ptr, n_list, n_ptr, out.ctypes.data, None, 0, None))
        del keep, cmem, nmem
        return out[:m]
    import torch

    (col, cmem), (ncol, nmem) = _strcol(cookies, batch.device), _strcol(nonces, batch.device)
    assert len(cmem[1]) == batch.n + 1 and len(nmem[1]) == batch.n + 1
    if not torch.is_tensor(hashes):
        hashes = torch.from_numpy(_hash_rows(hashes, batch.n)).to(batch.device)
    assert hashes.is_contiguous() and hashes.element_size() == 1 and hashes.numel() == 32 * batch.n
    idx_ptr, n_list, n_ptr, m, _ = _device_list(batch.n, idx, n_idx)
    if stream is None:
        stream = torch.cuda.current_stream(batch.device).cuda_stream
    out = torch.empty(max(1, m), dtype=torch.uint8, device=batch.device)
    if not m:
        return out[:0]
    need = int(lib().pwaf_verify_pow_scratch_bytes(m))
    scratch = torch.empty(need, dtype=torch.uint8, device=batch.device)
    _check(lib().pwaf_verify_pow(keyset._h, C.byref(st), C.byref(col), hashes.data_ptr(), C.byref(ncol), int(now), idx_ptr, n_list, n_ptr, out.data_ptr(), scratch.data_ptr(), need,
                                 C.c_void_p(stream)))
    status = out[:m]
    status.pow_scratch = scratch
    return status


def verify_pow_one(keyset, request, cookie, hash, nonce, now) -> int:
    """The proof-of-work check for one request on the host (pwaf_verify_pow_one): `cookie` is the first Cookie header's value (bytes | str |
    None: no header), `hash` the body's 32 bytes, `nonce` its string -> _abi.POW_ABSENT / _PASSED / _FAILED / _UNDECIDED."""
    st, keep = _request_struct(request)
    c = None if cookie is None else (cookie.encode() if isinstance(cookie, str) else bytes(cookie))
    nv = nonce.encode() if isinstance(nonce, str) else bytes(nonce)
    h = bytes(hash)
    if len(h) != 32:
        raise ValueError(f"verify_pow_one: the hash has {len(h)} bytes, a SHA-256 digest has 32")
    out = C.c_uint8(0xEE)
    rc = lib().pwaf_verify_pow_one(keyset._h, C.byref(st), c, 0 if c is None else len(c), h, nv, len(nv), int(now), C.byref(out))
    del keep
    _check(rc)
    return int(out.value)


def body_column(bodies):
    """[bytes | str | None per request] (None: no body) -> (data with PWAF_ARENA_PAD zero bytes behind it, offsets) numpy arrays, as cookie_column"""
    return cookie_column(bodies)


def body_stats(stats) -> dict:
    """The 32 bytes of a pwaf_body_stats (a device tensor once its stream is synchronised, a numpy array or bytes) -> {nonce_bytes, n, n_ok,
    n_malformed, n_undecided, overflow}."""
    raw = stats.cpu().numpy().tobytes() if hasattr(stats, "cpu") else bytes(stats)
    s = _abi.BodyStats.from_buffer_copy(raw[:C.sizeof(_abi.BodyStats)])
    return {"nonce_bytes": int(s.nonce_bytes), "n": int(s.n), "n_ok": int(s.n_ok), "n_malformed": int(s.n_malformed), "n_undecided": int(s.n_undecided),
            "overflow": int(s.overflow)}


def parse_pow_scan_shape() -> dict:
    """TEST HOOK (pwaf_parse_pow_scan_shape): the shape of parse_pow_bodies' scan, by the names of _abi.PARSE_POW_SCAN_SHAPE_FIELDS."""
    return _scan_shape(lib().pwaf_parse_pow_scan_shape, _abi.PARSE_POW_SCAN_SHAPE_FIELDS)


def parse_pow_bodies(bodies, n=None, idx=None, n_idx=None, stream=None, cap=None):
    """What serde_json makes CaptchaVerifyRequestBody of (captcha.rs:50-57, :291), for the proof-of-work request bodies of a batch
    (pwaf_parse_pow_bodies; include/pwaf.h) -> (status, hashes, nonce_col, stats): one _abi.BODY_* status per entry — of every request
    when idx is None, else of the requests the list `idx` names (n_idx: how many entries count; an entry that names no request reads
    BODY_NONE), e.g. the match_idx / n_matches of an evaluation; hashes (n, 32) and nonce_col = (data, offsets) indexed BY REQUEST, which
    verify_pow(..., hashes, nonce_col, ...) takes as they stand; stats: 32 bytes for body_stats(). The caller reads verify_pow's status
    only where the body status is BODY_OK; MALFORMED is the reference's error response, UNDECIDED a body the host parses with its own
    library. bodies: a list of bytes | str | None (host memory, as body_column makes it a column), or a (data, offsets) pair of numpy
    arrays (HOST mode) or of device tensors (DEVICE mode); n defaults to the offsets' length - 1. cap: the nonce column's room in bytes
    (default: the bodies' bytes + 16, in which no batch overflows). Takes no engine.
    HOST mode: synchronous, on the CPU -> numpy arrays. DEVICE mode: at most a memset and three launches are enqueued on `stream`
    (default: torch's current stream, which must be the stream torch allocates on when the call is made: outputs and scratch come from
    its caching allocator) and the call returns -> tensors to be read after the stream is synchronised; status entries at or past n_idx
    and hash rows of unselected requests are not written. The scratch stays reachable as `status.body_scratch`."""
    if not isinstance(bodies, tuple):
        bodies = body_column(bodies)
    data, off = bodies
    host_mode = isinstance(off, np.ndarray)
    col, (data, off) = _strcol(bodies, None if host_mode else off.device)
    ncol = _abi.DerivedCol()
    if n is None:
        n = len(off) - 1
    assert len(off) >= n + 1
    if host_mode:
        idx_ptr, n_list, n_ptr, m, keep = _host_list(n, idx, n_idx)
        if cap is None:
            cap = (int(off[n]) - int(off[0]) if n else 0) + _abi.ARENA_PAD
        status = np.zeros(max(1, m), dtype=np.uint8)
        hashes = np.zeros((max(1, n), 32), dtype=np.uint8)
        ndata, noff = _aligned_bytes(cap), np.zeros(n + 1, dtype=np.uint32)
        stats = np.zeros(C.sizeof(_abi.BodyStats) // 8, dtype=np.uint64)
        ncol.data, ncol.offsets, ncol.cap = ndata.ctypes.data, noff.ctypes.data, cap
        _check(lib().pwaf_parse_pow_bodies(C.byref(col), n, _abi.MEM_HOST, idx_ptr, n_list, n_ptr, status.ctypes.data, hashes.ctypes.data, C.byref(ncol), stats.ctypes.data, None, 0, None))
        del keep
        return status[:m], hashes[:n], (ndata, noff), stats.view(np.uint8)
    import torch

    device = off.device
    idx_ptr, n_list, n_ptr, m, keep = _device_list(n, idx, n_idx)
    if stream is None:
        stream = torch.cuda.current_stream(device).cuda_stream
    if cap is None:
        cap = data.numel() + _abi.ARENA_PAD  # (an upper bound without a synchronisation: the arena with its pad)
    status = torch.empty(max(1, m), dtype=torch.uint8, device=device)
    hashes = torch.empty((max(1, n), 32), dtype=torch.uint8, device=device)
    ndata = torch.empty(max(16, cap), dtype=torch.uint8, device=device)
    noff = torch.empty(n + 1, dtype=torch.int32, device=device)
    stats = torch.empty(C.sizeof(_abi.BodyStats), dtype=torch.uint8, device=device)
    need = int(lib().pwaf_parse_pow_bodies_scratch_bytes(n))
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    ncol.data, ncol.offsets, ncol.cap = ndata.data_ptr(), noff.data_ptr(), cap
    _check(lib().pwaf_parse_pow_bodies(C.byref(col), n, _abi.MEM_DEVICE, idx_ptr, n_list, n_ptr, status.data_ptr(), hashes.data_ptr(), C.byref(ncol), stats.data_ptr(), scratch.data_ptr(), need,
                                       C.c_void_p(stream)))
    status = status[:m]
    status.body_scratch = (scratch, keep, bodies)
    return status, hashes[:n], (ndata, noff), stats


def parse_pow_body_one(body):
    """One proof-of-work request body on the host (pwaf_parse_pow_body_one) -> (status, hash, nonce): an _abi.BODY_* status, the 32 bytes
    and the nonce's bytes (32 zero bytes and b"" unless the status is BODY_OK): what a per-request closure hands verify_pow_one."""
    b = body.encode() if isinstance(body, str) else bytes(body)
    buf = (C.c_uint8 * max(1, len(b))).from_buffer_copy(b or b"\0")
    st, h, at, ln = C.c_uint8(0xEE), (C.c_uint8 * 32)(), C.c_uint32(0), C.c_uint32(0)
    _check(lib().pwaf_parse_pow_body_one(C.addressof(buf), len(b), C.byref(st), C.addressof(h), C.byref(at), C.byref(ln)))
    return int(st.value), bytes(h), b[at.value:at.value + ln.value]


def respond_scan_shape() -> dict:
    """TEST HOOK (pwaf_respond_scan_shape): the shape of respond's scan, by the names of _abi.RESPOND_SCAN_SHAPE_FIELDS."""
    return _scan_shape(lib().pwaf_respond_scan_shape, _abi.RESPOND_SCAN_SHAPE_FIELDS)


def _resp_mask(kinds) -> int:
    """A tuple of _abi.RESP_* kinds (or a mask as an int) -> the mask of a pwaf_resp_list"""
    if isinstance(kinds, (int, np.integer)):
        return int(kinds)
    mask = 0
    for k in kinds:
        mask |= 1 << int(k)
    return mask


def respond(batch, verdicts, cookie_status=None, route=None, lists=(), caps=None, stream=None):
    """Which response each request of `batch` gets (pwaf_respond; include/pwaf.h): the reference's order of precedence
    (http_listener.rs:196-272: gate A, gate B with serve_captcha_request's dispatch, gate C, the rules, the routes, 404) over what the
    earlier calls wrote — verdicts (evaluate_*), cookie_status (verify_cookies; None: every request ABSENT) and route (evaluate_*_routes;
    None: no route column) — and the batch's path column. -> (responses, counts, [(idx, n), ...]): one response per request (kind: an
    _abi.RESP_*, arg: the rule, the route or a sentinel), the RESP_KINDS counters, and per entry of `lists` (each a tuple of RESP_* kinds;
    at most RESP_MAX_LISTS) the ASCENDING indices of the requests whose kind is among them with their number n — what client_ids,
    verify_cookies, verify_pow, parse_pow_bodies and export_records take as idx / n_idx. caps: the room of each list (default: the batch's
    n, which no list exceeds; 0: count only); n may exceed it, the first min(n, cap) entries are written. Takes no engine.
    RequestBatch: verdicts a VERDICT_DTYPE array, cookie_status uint8, route 32 bits wide (-1 / ROUTE_NONE: none); synchronous, on the CPU
    -> a RESPONSE_DTYPE array, a uint64 array, [(uint32 array of min(n, cap) entries, int)].
    DeviceBatch: device tensors (verdicts as evaluate_device returns them); one small memset and at most three launches are enqueued on
    `stream` (default: torch's current stream, which must be the stream torch allocates on when the call is made: outputs and scratch come
    from its caching allocator) and the call returns -> an (n, 2) int32 tensor (word 0: the kind, word 1: the arg), an int64 tensor of
    RESP_KINDS counters, [(int32 tensor of cap entries, one-element int32 tensor)] to be read after the stream is synchronised; a
    consumer on the same stream takes (idx, n) as they are. The scratch stays reachable as `responses.respond_scratch`."""
    lists = [_resp_mask(k) for k in lists]
    n = batch.n
    caps = [n] * len(lists) if caps is None else [int(c) for c in caps]
    assert len(caps) == len(lists)
    st = batch.as_struct()
    arr = (_abi.RespList * max(1, len(lists)))()
    if isinstance(batch, RequestBatch):
        verdicts = np.ascontiguousarray(verdicts, dtype=VERDICT_DTYPE)
        assert len(verdicts) >= n
        status = None if cookie_status is None else np.ascontiguousarray(cookie_status, dtype=np.uint8)
        rt = None if route is None else np.ascontiguousarray(np.asarray(route).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)
        assert (status is None or len(status) >= n) and (rt is None or len(rt) >= n)
        out = np.zeros(max(1, n), dtype=RESPONSE_DTYPE)
        counts = np.zeros(_abi.RESP_KINDS, dtype=np.uint64)
        res = []
        for l, (mask, cap) in enumerate(zip(lists, caps)):
            idx, cnt = np.zeros(max(1, cap), dtype=np.uint32), np.zeros(1, dtype=np.uint32)
            arr[l].kinds, arr[l].cap, arr[l].idx, arr[l].n = mask, cap, idx.ctypes.data if cap else None, cnt.ctypes.data
            res.append((idx, cnt))
        _check(lib().pwaf_respond(C.byref(st), verdicts.ctypes.data, None if status is None else status.ctypes.data, None if rt is None else rt.ctypes.data, out.ctypes.data,
                                  counts.ctypes.data, arr, len(lists), None, 0, None))
        return out[:n], counts, [(idx[:min(int(cnt[0]), cap)], int(cnt[0])) for (idx, cnt), cap in zip(res, caps)]
    import torch

    device = batch.device
    for t, width in ((verdicts, 8), (cookie_status, 1), (route, 4)):
        assert t is None or (t.is_contiguous() and t.numel() * t.element_size() >= width * n)
    if stream is None:
        stream = torch.cuda.current_stream(device).cuda_stream
    out = torch.empty((max(1, n), 2), dtype=torch.int32, device=device)
    counts = torch.empty(_abi.RESP_KINDS, dtype=torch.int64, device=device)
    res = []
    for l, (mask, cap) in enumerate(zip(lists, caps)):
        idx, cnt = torch.empty(max(1, cap), dtype=torch.int32, device=device), torch.empty(1, dtype=torch.int32, device=device)
        arr[l].kinds, arr[l].cap, arr[l].idx, arr[l].n = mask, cap, idx.data_ptr() if cap else None, cnt.data_ptr()
        res.append((idx[:cap], cnt))
    need = int(lib().pwaf_respond_scratch_bytes(n))
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    _check(lib().pwaf_respond(C.byref(st), verdicts.data_ptr(), None if cookie_status is None else cookie_status.data_ptr(), None if route is None else route.data_ptr(),
                              out.data_ptr(), counts.data_ptr(), arr, len(lists), scratch.data_ptr(), need, C.c_void_p(stream)))
    out = out[:n]
    out.respond_scratch = scratch
    return out, counts, res


def respond_one(verdict, cookie_status=0, route=None, path=b""):
    """The same decision for one request on the host (pwaf_respond_one) -> (kind, arg): verdict an (action, rule_idx) pair or a record of
    VERDICT_DTYPE, cookie_status an _abi.COOKIE_*, route None (no route column), an index, or -1 / ROUTE_NONE (no route matches), path the
    request's derived path. What a per-request closure calls behind verify_cookie and evaluate_routed."""
    v = _abi.Verdict()
    if isinstance(verdict, (tuple, list)):
        v.action, v.rule_idx = int(verdict[0]), int(verdict[1]) & 0xFFFFFFFF
    else:
        v.action, v.rule_idx = int(verdict["action"]), int(verdict["rule_idx"])
    p = path.encode() if isinstance(path, str) else bytes(path)
    buf = (C.c_uint8 * max(1, len(p))).from_buffer_copy(p or b"\0")
    out = _abi.Response()
    _check(lib().pwaf_respond_one(C.byref(v), int(cookie_status), 0 if route is None else 1, 0 if route is None else int(route) & 0xFFFFFFFF, C.addressof(buf), len(p), C.byref(out)))
    return int(out.kind), int(out.arg)


DERIVED_FIELDS = (0, 2, 4)  # PWAF_FIELD_HOST, _PATH, _USER_AGENT: pwaf_derive_batch's out[0..2]


def derive_stats(stats) -> dict:
    """The 32 bytes of a pwaf_derive_stats (a device tensor once its stream is synchronised, a numpy array or bytes) -> {bytes: [host, path,
    user_agent], n, overflow}."""
    raw = stats.cpu().numpy().tobytes() if hasattr(stats, "cpu") else bytes(stats)
    s = _abi.DeriveStats.from_buffer_copy(raw[:C.sizeof(_abi.DeriveStats)])
    return {"bytes": [int(b) for b in s.bytes], "n": int(s.n), "overflow": int(s.overflow)}


def derive_scan_shape() -> dict:
    """TEST HOOK (pwaf_derive_scan_shape): the shape of derive_batch's scan, by the names of _abi.DERIVE_SCAN_SHAPE_FIELDS."""
    return _scan_shape(lib().pwaf_derive_scan_shape, _abi.DERIVE_SCAN_SHAPE_FIELDS)


def derive_batch(batch, uri_host=None, present=None, stream=None):
    """The reference's own derivation of host, path and User-Agent (get_host / get_path / get_user_agent above) for a whole batch
    (pwaf_derive_batch; include/pwaf.h). `batch`'s host, path and user_agent columns hold the RAW values: the Host header's value,
    uri.path() and the User-Agent header's value. uri_host: uri.host() per request; present: n bytes of _abi.RAW_HAS_* saying which of
    the three sources a request has (default: a Host header and a User-Agent, no URI host). Takes no engine.
    RequestBatch: uri_host is a (data, offsets) numpy pair (needs `present`) or a list of bytes | None, whose entries set RAW_HAS_URI_HOST
    themselves; the call is synchronous and runs on the CPU -> a new RequestBatch with the three columns replaced and every other shared.
    DeviceBatch: uri_host is a (data, offsets) pair of device tensors and present a device tensor; at most three launches are enqueued on
    `stream` (default: torch's current stream) and the call returns -> (DeviceBatch, stats): the new DeviceBatch shares the untouched
    tensors, owns the derived columns (room: the raw column's bytes + 16; host: the Host headers' + the URI hosts' bytes + 16, so no
    column can overflow) and reports field_bytes 0 for them, so evaluate_device on the same stream follows without a synchronisation by the
    caller; stats is a 32-byte tensor for derive_stats() once the stream is synchronised. `stream` must be the stream torch allocates on
    when the call is made (its current stream, e.g. inside `with torch.cuda.stream(s)`): the outputs and the scratch come from torch's
    caching allocator, which may hand their memory to other work of ITS stream once they are dropped. A DeviceBatch that derive_batch
    returned is not a raw batch and is refused."""
    n = batch.n
    host_mode = isinstance(batch, RequestBatch)
    keep = []
    extra = None
    uri_bytes = 0
    if host_mode:
        if present is not None:
            present = np.ascontiguousarray(present, dtype=np.uint8).reshape(-1)
            assert len(present) == n
        if isinstance(uri_host, (list, tuple)) and not (len(uri_host) == 2 and isinstance(uri_host[0], np.ndarray)):
            assert len(uri_host) == n
            has = np.array([_abi.RAW_HAS_URI_HOST if v is not None else 0 for v in uri_host], dtype=np.uint8).reshape(-1)
            rest = np.full(n, _abi.RAW_HAS_HOST_HEADER | _abi.RAW_HAS_USER_AGENT, dtype=np.uint8) if present is None else present & ~np.uint8(_abi.RAW_HAS_URI_HOST)
            present = (rest | has).astype(np.uint8)
            uri_host = cookie_column(uri_host)
        elif uri_host is not None:
            if present is None:
                raise ValueError("derive_batch: a uri_host column needs `present` to say which requests have a URI host")
            uri_host = (np.ascontiguousarray(uri_host[0], dtype=np.uint8), np.ascontiguousarray(uri_host[1], dtype=np.uint32))
            assert len(uri_host[1]) == n + 1
        if uri_host is not None:
            uri_bytes = int(uri_host[1][-1]) - int(uri_host[1][0])
        ptr = lambda a: a.ctypes.data  # noqa: E731
        raw_bytes = [int(batch.offsets[f][-1]) - int(batch.offsets[f][0]) for f in DERIVED_FIELDS]
    else:
        import torch

        if uri_host is not None:
            assert present is not None, "derive_batch: a uri_host column needs `present` to say which requests have a URI host"
            assert uri_host[0].is_contiguous() and uri_host[1].is_contiguous() and uri_host[1].element_size() == 4 and uri_host[1].numel() == n + 1
            uri_bytes = uri_host[0].numel()  # (an upper bound: the arena with its pad)
        if present is not None:
            assert present.is_contiguous() and present.element_size() == 1 and present.numel() == n
        ptr = lambda t: t.data_ptr()  # noqa: E731
        raw_bytes = [batch.field_bytes[f] for f in DERIVED_FIELDS]
        if any(b is None for b in raw_bytes):
            raise ValueError("derive_batch: this DeviceBatch holds derived columns (their sizes are not known on the host): it is not a raw batch")
        if stream is None:
            stream = torch.cuda.current_stream(batch.device).cuda_stream
    if uri_host is not None or present is not None:
        extra = _abi.RawColumns()
        extra.struct_size = C.sizeof(_abi.RawColumns)
        if uri_host is not None:
            extra.uri_host.data, extra.uri_host.offsets = ptr(uri_host[0]), ptr(uri_host[1])
        if present is not None:
            extra.present = ptr(present)
        keep += [uri_host, present]
    # room in which no column can overflow: a request takes its host from the Host header or from the URI, so a batch may keep both columns' bytes
    caps = [raw_bytes[0] + uri_bytes + _abi.ARENA_PAD, raw_bytes[1] + _abi.ARENA_PAD, raw_bytes[2] + _abi.ARENA_PAD]
    st = batch.as_struct()
    out = (_abi.DerivedCol * 3)()
    if host_mode:
        data = [_aligned_bytes(c) for c in caps]
        offs = [np.zeros(n + 1, dtype=np.uint32) for _ in caps]
        stats = np.zeros(C.sizeof(_abi.DeriveStats) // 8, dtype=np.uint64)
        scratch, scratch_bytes = None, 0
    else:
        data = [torch.empty(c, dtype=torch.uint8, device=batch.device) for c in caps]
        offs = [torch.empty(n + 1, dtype=torch.int32, device=batch.device) for _ in caps]
        stats = torch.empty(C.sizeof(_abi.DeriveStats), dtype=torch.uint8, device=batch.device)
        scratch_bytes = int(lib().pwaf_derive_scratch_bytes(n))
        scratch = torch.empty(max(16, scratch_bytes), dtype=torch.uint8, device=batch.device)
    for c in range(3):
        out[c].data, out[c].offsets, out[c].cap = ptr(data[c]), ptr(offs[c]), caps[c]
    rc = lib().pwaf_derive_batch(C.byref(st), None if extra is None else C.byref(extra), out, ptr(stats), None if scratch is None else ptr(scratch), scratch_bytes,
                                 None if host_mode else C.c_void_p(stream))
    _check(rc)
    if host_mode:
        if derive_stats(stats)["overflow"]:  # (cannot happen with the caps above: a column's bytes would be incomplete)
            raise PwafError(_abi.E_BATCH, f"derive_batch: a derived column did not fit its room: {derive_stats(stats)}")
        new_data, new_offs = list(batch.data), list(batch.offsets)
        for c, f in enumerate(DERIVED_FIELDS):
            new_data[f], new_offs[f] = data[c], offs[c]
        return RequestBatch(new_data, new_offs, batch.ip, batch.ip_is_v6, batch.port, batch.flags, batch.asn, batch.country, dict(batch.headers))
    derived = DeviceBatch.adopt(batch, {f: (data[c], offs[c]) for c, f in enumerate(DERIVED_FIELDS)})
    derived._derive_scratch = (scratch, keep)  # (the launches' own until they have run)
    return derived, stats


def records_scan_shape() -> dict:
    """TEST HOOK (pwaf_records_scan_shape): the shape of evaluate_records_device's scan, by the names of _abi.RECORDS_SCAN_SHAPE_FIELDS."""
    return _scan_shape(lib().pwaf_records_scan_shape, _abi.RECORDS_SCAN_SHAPE_FIELDS)


def verdict_from_record(v) -> Verdict:
    ridx = int(v["rule_idx"])
    gate = {_abi.RULE_UA_GATE: "user_agent", _abi.RULE_CAPTCHA_ENDPOINT: "captcha_endpoint"}.get(ridx)
    return Verdict(Decision(int(v["action"])), None if ridx >= _abi.RULE_CAPTCHA_ENDPOINT else ridx, gate)


class DeviceBatch:
    """A RequestBatch uploaded to HBM as torch tensors (PyTorch is only the allocator/stream owner here)."""

    def __init__(self, batch: RequestBatch, device="cuda:0"):
        import torch

        self.device = torch.device(device)
        self.n = batch.n
        self.algorithmic_bytes = batch.algorithmic_bytes()
        self.field_bytes = [int(o[-1]) - int(o[0]) for o in batch.offsets]
        self.arena_bytes = [int(o[-1]) for o in batch.offsets]  # offsets[n]: what pwaf_batch.field_bytes carries
        t = lambda a: torch.from_numpy(a).to(self.device, non_blocking=False)  # noqa: E731
        self.data = [t(d) for d in batch.data]
        self.offsets = [t(o.view(np.int32)) for o in batch.offsets]
        self.ip = t(batch.ip)
        self.ip_is_v6 = t(batch.ip_is_v6)
        self.port = t(batch.port.view(np.int16))
        self.flags = t(batch.flags)
        self.asn = None if batch.asn is None else t(batch.asn.view(np.int32))
        self.country = None if batch.country is None else t(batch.country.view(np.int16))
        self.headers = {name: (t(d), t(o.view(np.int32)), int(o[-1])) for name, (d, o) in batch.headers.items()}
        self._empty = None

    @classmethod
    def adopt(cls, other: "DeviceBatch", columns: dict) -> "DeviceBatch":
        """A DeviceBatch that shares every tensor of `other` except the fields `columns` names: {field id: (data, offsets)} device tensors
        that already hold a valid arena (derive_batch's outputs). Their sizes are not known on the host: as_struct() reports field_bytes 0
        for them and the engine asks for offsets[n] on its stream."""
        b = cls.__new__(cls)
        b.device, b.n, b.algorithmic_bytes = other.device, other.n, other.algorithmic_bytes
        b.field_bytes, b.arena_bytes = list(other.field_bytes), list(other.arena_bytes)
        b.data, b.offsets = list(other.data), list(other.offsets)
        for f, (d, o) in columns.items():
            b.data[f], b.offsets[f] = d, o
            b.field_bytes[f], b.arena_bytes[f] = None, 0  # (None: not known on the host)
        b.ip, b.ip_is_v6, b.port, b.flags, b.asn, b.country = other.ip, other.ip_is_v6, other.port, other.flags, other.asn, other.country
        b.headers = dict(other.headers)
        b._empty = None
        return b

    def as_struct(self, header_names: Sequence[str] = ()) -> _abi.Batch:
        import torch

        b = _abi.Batch()
        b.struct_size = C.sizeof(_abi.Batch)
        b.n = self.n
        b.memory = _abi.MEM_DEVICE
        if header_names:
            cols = (_abi.StrCol * len(header_names))()
            hb = (C.c_uint32 * len(header_names))()
            for k, name in enumerate(header_names):
                if name in self.headers:
                    d, o, nbytes = self.headers[name]
                    cols[k].data, cols[k].offsets, hb[k] = d.data_ptr(), o.data_ptr(), nbytes
                # (a missing name stays NULL: the engine reads it as the empty string for every request)
            b.n_headers = len(header_names)
            b.headers = cols
            b.header_bytes = hb
            b._keep = [cols, hb]
        for f in range(_abi.N_FIELDS):
            b.field[f].data = self.data[f].data_ptr()
            b.field[f].offsets = self.offsets[f].data_ptr()
            b.field_bytes[f] = self.arena_bytes[f]
        b.ip = self.ip.data_ptr()
        b.ip_is_v6 = self.ip_is_v6.data_ptr()
        b.port = self.port.data_ptr()
        b.flags = self.flags.data_ptr()
        b.asn = None if self.asn is None else self.asn.data_ptr()
        b.country = None if self.country is None else self.country.data_ptr()
        return b
