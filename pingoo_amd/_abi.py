"""ctypes mirror of include/pwaf.h (struct layouts and constants only — no behaviour).

Kept in one place so the product wrapper (pingoo_amd.engine) and the test-side oracle wrapper
(oracle/pyoracle.py) marshal the *same* bytes across their respective C ABIs.
"""
import ctypes as C

ABI_VERSION = 4

OK = 0
E_INVALID_ARG = -1
E_SYNTAX = -2
E_UNSUPPORTED = -3
E_LIST = -4
E_DEVICE = -5
E_BATCH = -6
E_NOMEM = -7
E_BUSY = -8

ACTION_ALLOW, ACTION_BLOCK, ACTION_CAPTCHA, ACTION_BYPASS = 0, 1, 2, 3
RULE_NONE = 0xFFFFFFFF
RULE_UA_GATE = 0xFFFFFFFE
RULE_CAPTCHA_ENDPOINT = 0xFFFFFFFD
RULE_ACTION_BLOCK, RULE_ACTION_CAPTCHA = 1, 2

LIST_STRING, LIST_INT, LIST_IP = 0, 1, 2
OPT_NO_UA_GATE, OPT_NO_CAPTCHA_BYPASS, OPT_NO_PREFILTER, OPT_STRICT, OPT_FILTER_STRIDE2, OPT_LENIENT, OPT_NO_RESIDUAL, OPT_GLOBAL_VERDICT_TABLES, OPT_NO_CONFIRM, OPT_NO_RESIDUAL_JIT = 1, 2, 4, 8, 16, 32, 64, 128, 512, 1024
OPT_DENSE_VERDICT, OPT_TINY_VERDICT_SLOTS, OPT_NO_DIR_SUMMARY, OPT_SPARSE_VERDICT, OPT_EAGER_CMP, OPT_NO_DENSE_SWITCH = 2048, 4096, 8192, 16384, 32768, 65536
OPT_GEO_ANSWERS = 256  # the engine also answers each request's GeoIP record (pwaf_geoip_lookup, pwaf_evaluate_*_geo)
OPT_RULE_HITS = 131072  # the engine can report every rule that matches a request (pwaf_evaluate_*_hits); keeps observe-only rules
W_PARTIAL = 1
MEM_HOST, MEM_DEVICE = 0, 1
FLAG_CAPTCHA_VERIFIED = 1
ROUTE_NONE = 0xFFFFFFFF  # PWAF_ROUTE_NONE: no route matches the request (pwaf_evaluate_*_routes)
RECORD_NONE = 0xFFFFFFFF  # PWAF_RECORD_NONE: the list entry has no record in the buffer (pwaf_export_records)
# pwaf_verify_cookies / pwaf_verify_cookie_one: one status per request (gate C, http_listener.rs:222-236)
COOKIE_ABSENT, COOKIE_VERIFIED, COOKIE_INVALID, COOKIE_UNDECIDED = 0, 1, 2, 3
KEYSET_MAX_KEYS, KEYSET_MAX_KID, COOKIE_MAX_SIGNED_BYTES = 8, 64, 8192
# pwaf_verify_pow / pwaf_verify_pow_one: one status per proof-of-work submission (CaptchaManager::api_verify, captcha.rs:241-333)
POW_ABSENT, POW_PASSED, POW_FAILED, POW_UNDECIDED = 0, 1, 2, 3
# pwaf_parse_pow_bodies / pwaf_parse_pow_body_one: one status per proof-of-work request body (CaptchaVerifyRequestBody, captcha.rs:50-57, :291)
BODY_NONE, BODY_OK, BODY_MALFORMED, BODY_UNDECIDED = 0, 1, 2, 3
POW_BODY_MAX_BYTES = 4096
# pwaf_respond / pwaf_respond_one: which response a request gets (http_listener.rs:196-272; serve_captcha_request, captcha.rs:158-174)
RESP_FORWARD, RESP_NOT_FOUND, RESP_BLOCKED, RESP_CAPTCHA_PAGE, RESP_CAPTCHA_ASSET, RESP_CAPTCHA_INIT, RESP_CAPTCHA_VERIFY, RESP_CAPTCHA_NOT_FOUND, RESP_HOST_DECIDES = range(9)
RESP_KINDS, RESP_MAX_LISTS = 9, 4
RESP_KIND_NAMES = ("forward", "not_found", "blocked", "captcha_page", "captcha_asset", "captcha_init", "captcha_verify", "captcha_not_found", "host_decides")
RULE_COOKIE = 0xFFFFFFFC  # PWAF_RULE_COOKIE: gate C, a present but invalid verified cookie (pwaf_response.arg)
N_FIELDS = 5
FIELD_NAMES = ("host", "url", "path", "method", "user_agent")
ARENA_PAD = 16
# pwaf_engine_address_tables (test hook): the meaning of out[0..7]
ADDRESS_TABLE_FIELDS = ("escapes", "n_vals", "has_summary", "shift", "common", "packed", "classes", "sets")
# pwaf_program_confirm_shape (test hook): the meaning of out[0..7]
CONFIRM_SHAPE_FIELDS = ("entries", "bytes", "class_words", "in_lds", "longest", "top_class_pos", "widest_bin", "has_walk")
# pwaf_records_scan_shape (test hook): the meaning of out[0..3] (pwaf_evaluate_records_device's scan: records per tile, tiles per phase-2 step)
RECORDS_SCAN_SHAPE_FIELDS = ("tile", "step", "zero2", "zero3")
# pwaf_derive_scan_shape (test hook): the meaning of out[0..3] (pwaf_derive_batch's scan: requests per tile, tiles per step of the base launch,
# requests per workgroup of the copy launch)
DERIVE_SCAN_SHAPE_FIELDS = ("tile", "step", "copy_group", "zero3")
# pwaf_parse_pow_scan_shape (test hook): the meaning of out[0..3] (pwaf_parse_pow_bodies' scan: entries per tile, tiles per step of the base
# launch, requests per workgroup of the copy launch, the least bound on the parse launch's workgroups with a list)
PARSE_POW_SCAN_SHAPE_FIELDS = ("tile", "step", "copy_group", "min_groups")
# pwaf_respond_scan_shape (test hook): the meaning of out[0..3] (pwaf_respond's scan: requests per tile, tiles per step of the base launch,
# PWAF_RESP_MAX_LISTS, PWAF_RESP_KINDS)
RESPOND_SCAN_SHAPE_FIELDS = ("tile", "step", "max_lists", "kinds")
# pwaf_raw_columns.present: which of its sources a raw request has (pwaf_derive_batch)
RAW_HAS_URI_HOST, RAW_HAS_HOST_HEADER, RAW_HAS_USER_AGENT = 1, 2, 4
# pwaf_program_list_scans (test hook): the meaning of a descriptor's PWAF_LIST_SCAN_WORDS words (share_owner 0xFFFFFFFF: none)
LIST_SCAN_FIELDS = ("phase", "pass", "tier", "threads", "hot_bytes", "n_hot", "n_delta", "behind_filter", "merge_rec", "dense_mode", "share_owner", "need_bit",
                    "launch", "launch_count", "wg_per_cu", "zero15")
# pwaf_program_verdict_shape (test hook): the meaning of out[0..7] (capacity: entries / value slots per wave; bit_regs: the BR of the instantiation)
VERDICT_SHAPE_FIELDS = ("mode", "capacity", "waves", "per_cu", "lds_tables", "lds_bytes", "n_passes", "bit_regs")
# pwaf_program_flat_image (test hook): the words of its "FSHP" section
FLAT_SHAPE_FIELDS = ("n_states", "n_classes", "scalar_mode", "ill_class", "n_full", "n_delta", "lds_bytes")
# pwaf_engine_coarse_tables (test hook): the meaning of out[0..15]
COARSE_TABLE_FIELDS = ("present", "shift", "bytes", "blocks_set", "summary_blocks_set", "threads", "wg_per_cu", "zero7",
                       "rec_present", "rec_shift", "rec_bytes", "rec_blocks_set", "zero12", "zero13", "zero14", "zero15")
# pwaf_engine_filter_flags (test hook): the meaning of info[0..7]; FILTER_SLAB_ROWS = PWAF_FILTER_SLAB_ROWS, the 64-bit row words per 128 KiB slab
FILTER_FLAGS_FIELDS = ("slab0", "slabs", "stride", "has_pairs", "pair_count", "slab_rows", "zero6", "zero7")
FILTER_SLAB_ROWS = 128
# pwaf_engine_geo_answer_tables (test hook): the meaning of out[0..7]
GEO_ANSWER_TABLE_FIELDS = ("has_table", "escapes", "n_vals", "has_summary", "shift", "common", "records", "zero")


class RuleDesc(C.Structure):
    _fields_ = [
        ("name", C.c_char_p),
        ("expression", C.c_char_p),
        ("actions", C.POINTER(C.c_uint8)),
        ("n_actions", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class RouteDesc(C.Structure):
    """pwaf_route_desc: one route of an engine created with routes (expression None = matches every request)."""

    _fields_ = [("name", C.c_char_p), ("expression", C.c_char_p), ("reserved", C.c_uint64)]


class ListDesc(C.Structure):
    _fields_ = [
        ("name", C.c_char_p),
        ("type", C.c_uint32),
        ("n_items", C.c_uint32),
        ("items", C.POINTER(C.c_char_p)),
    ]


class GeoipEntry(C.Structure):
    _fields_ = [
        ("addr", C.c_uint8 * 16),
        ("prefix_len", C.c_uint8),
        ("is_v6", C.c_uint8),
        ("country", C.c_uint8 * 2),
        ("asn", C.c_uint32),
    ]


class GeoipTable(C.Structure):
    _fields_ = [("entries", C.POINTER(GeoipEntry)), ("n_entries", C.c_size_t)]


class Options(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("flags", C.c_uint32),
        ("device", C.c_int32),
        ("lds_table_budget", C.c_uint32),
        ("max_dfa_states", C.c_uint32),
        ("max_table_bytes", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class CompileError(C.Structure):
    _fields_ = [("code", C.c_int32), ("rule_index", C.c_uint32), ("message", C.c_char * 248)]


class StrCol(C.Structure):
    _fields_ = [("data", C.c_void_p), ("offsets", C.c_void_p)]


class Batch(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n", C.c_uint32),
        ("memory", C.c_uint32),
        ("n_headers", C.c_uint32),
        ("field", StrCol * N_FIELDS),
        ("ip", C.c_void_p),
        ("ip_is_v6", C.c_void_p),
        ("port", C.c_void_p),
        ("flags", C.c_void_p),
        ("asn", C.c_void_p),
        ("country", C.c_void_p),
        ("field_bytes", C.c_uint32 * N_FIELDS),
        ("reserved", C.c_uint32),
        ("headers", C.POINTER(StrCol)),
        ("header_bytes", C.POINTER(C.c_uint32)),
    ]


class Verdict(C.Structure):
    _fields_ = [("action", C.c_uint8), ("pad", C.c_uint8 * 3), ("rule_idx", C.c_uint32)]


class Counts(C.Structure):
    _fields_ = [("by_action", C.c_uint64 * 4)]


class Request(C.Structure):
    _fields_ = [
        ("host", C.c_char_p), ("url", C.c_char_p), ("path", C.c_char_p), ("method", C.c_char_p), ("user_agent", C.c_char_p),
        ("host_len", C.c_uint32), ("url_len", C.c_uint32), ("path_len", C.c_uint32), ("method_len", C.c_uint32), ("user_agent_len", C.c_uint32),
        ("ip", C.c_uint8 * 16),
        ("ip_is_v6", C.c_uint8),
        ("flags", C.c_uint8),
        ("port", C.c_uint16),
        ("has_geoip", C.c_uint8),
        ("country", C.c_uint8 * 2),
        ("pad", C.c_uint8),
        ("asn", C.c_uint32),
        ("n_headers", C.c_uint32),
        ("headers", C.c_void_p),  # pwaf_span[n_headers]
    ]


class RecordHead(C.Structure):
    """pwaf_record_head (ABI 4): the fixed part of one request record; lengths and values follow (include/pwaf.h)."""

    _fields_ = [
        ("size", C.c_uint32),
        ("n_values", C.c_uint16),
        ("port", C.c_uint16),
        ("ip", C.c_uint8 * 16),
        ("asn", C.c_uint32),
        ("country", C.c_uint8 * 2),
        ("flags", C.c_uint8),
        ("ip_is_v6", C.c_uint8),
        ("has_geoip", C.c_uint8),
        ("reserved", C.c_uint8 * 3),
    ]


class ExportStats(C.Structure):
    """pwaf_export_stats: what pwaf_export_records reports — the bytes of every valid selected record, list entries looked at, records written."""

    _fields_ = [("bytes_needed", C.c_uint64), ("n_selected", C.c_uint32), ("n_written", C.c_uint32)]


class ClientId(C.Structure):
    """pwaf_client_id: a captcha client id (pwaf_client_ids / pwaf_client_id_one) — 43 characters of the URL-safe alphabet, then NUL."""

    _fields_ = [("text", C.c_char * 44)]


class Ed25519Key(C.Structure):
    """pwaf_ed25519_key: one verifying key of a pwaf_keyset — the kid (NUL-terminated) and the public key's 32-byte encoding."""

    _fields_ = [("kid", C.c_char_p), ("x", C.c_uint8 * 32)]


class RawColumns(C.Structure):
    """pwaf_raw_columns: what a raw batch carries beyond pwaf_batch (pwaf_derive_batch) — the URI hosts and the present bytes."""

    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("uri_host", StrCol), ("present", C.c_void_p)]


class DerivedCol(C.Structure):
    """pwaf_derived_col: one output column of pwaf_derive_batch — data, offsets (n + 1) and the bytes data has room for."""

    _fields_ = [("data", C.c_void_p), ("offsets", C.c_void_p), ("cap", C.c_uint64)]


class DeriveStats(C.Structure):
    """pwaf_derive_stats: offsets[n] of the derived host, path and user_agent column, the requests derived, one overflow bit per column."""

    _fields_ = [("bytes", C.c_uint64 * 3), ("n", C.c_uint32), ("overflow", C.c_uint32)]


class BodyStats(C.Structure):
    """pwaf_body_stats: offsets[n] of the nonce column pwaf_parse_pow_bodies wrote, the entries looked at and their statuses, the overflow bit."""

    _fields_ = [("nonce_bytes", C.c_uint64), ("n", C.c_uint32), ("n_ok", C.c_uint32), ("n_malformed", C.c_uint32), ("n_undecided", C.c_uint32),
                ("overflow", C.c_uint32), ("reserved", C.c_uint32)]


class Response(C.Structure):
    """pwaf_response: which response a request gets (pwaf_respond) — a RESP_* kind and its argument (a rule, a route or a RULE_* sentinel)."""

    _fields_ = [("kind", C.c_uint8), ("pad", C.c_uint8 * 3), ("arg", C.c_uint32)]


class RespList(C.Structure):
    """pwaf_resp_list: one output list of pwaf_respond — the mask of kinds that belong, the room of idx, idx and the written count."""

    _fields_ = [("kinds", C.c_uint32), ("cap", C.c_uint32), ("idx", C.c_void_p), ("n", C.c_void_p)]


class Geo(C.Structure):
    """pwaf_geo: one GeoIP answer (PWAF_OPT_GEO_ANSWERS) — the record the rules saw as client.asn / client.country."""

    _fields_ = [("asn", C.c_uint32), ("country", C.c_uint8 * 2), ("reserved", C.c_uint16)]


class RuleHit(C.Structure):
    """pwaf_rule_hit: rule `rule_idx` matches the requests 64 * group + r for every set bit r of mask (PWAF_OPT_RULE_HITS)."""

    _fields_ = [("rule_idx", C.c_uint32), ("group", C.c_uint32), ("mask", C.c_uint64)]


class Completion(C.Structure):
    _fields_ = [("tag", C.c_uint64), ("verdict", Verdict), ("status", C.c_int32), ("reserved", C.c_uint32)]


class Span(C.Structure):
    _fields_ = [("data", C.c_char_p), ("len", C.c_uint32), ("reserved", C.c_uint32)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("ms", C.c_float), ("alg_bytes", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [
        ("n_rules", C.c_uint32), ("n_atoms", C.c_uint32), ("n_scan_atoms", C.c_uint32), ("n_numeric_atoms", C.c_uint32),
        ("n_dfa_groups", C.c_uint32), ("n_dfa_states_total", C.c_uint32), ("max_dfa_states", C.c_uint32), ("dfa_table_bytes_total", C.c_uint32),
        ("n_ip_lists", C.c_uint32), ("ipset_trie_nodes", C.c_uint32), ("geo_trie_nodes", C.c_uint32), ("n_dnf_literals", C.c_uint32),
        ("n_warnings", C.c_uint32), ("n_filtered_groups", C.c_uint32), ("n_gated_groups", C.c_uint32), ("n_confirm_literals", C.c_uint32),
    ]


class Marshalled:
    """Keeps the Python objects backing a set of C descriptors alive."""

    def __init__(self):
        self.keep = []


def marshal_rules(rules, m):
    """rules: iterable of (name, expression-or-None, [action codes]) -> (RuleDesc array, n)."""
    rules = list(rules)
    arr = (RuleDesc * max(1, len(rules)))()
    for i, (name, expr, actions) in enumerate(rules):
        acts = (C.c_uint8 * max(1, len(actions)))(*actions)
        m.keep.append(acts)
        arr[i].name = name.encode() if isinstance(name, str) else name
        arr[i].expression = None if expr is None else (expr.encode() if isinstance(expr, str) else expr)
        arr[i].actions = C.cast(acts, C.POINTER(C.c_uint8))
        arr[i].n_actions = len(actions)
    m.keep.append(arr)
    return arr, len(rules)


def marshal_routes(routes, m):
    """routes: iterable of (name, expression-or-None) -> (RouteDesc array, n)."""
    routes = list(routes)
    arr = (RouteDesc * max(1, len(routes)))()
    for i, (name, expr) in enumerate(routes):
        arr[i].name = name.encode() if isinstance(name, str) else name
        arr[i].expression = None if expr is None else (expr.encode() if isinstance(expr, str) else expr)
    m.keep.append(arr)
    return arr, len(routes)


def marshal_lists(lists, m):
    """lists: dict name -> (type code, [item strings]) -> (ListDesc array, n)."""
    lists = lists or {}
    arr = (ListDesc * max(1, len(lists)))()
    for i, (name, (ltype, items)) in enumerate(lists.items()):
        enc = [(s.encode() if isinstance(s, str) else s) for s in items]
        carr = (C.c_char_p * max(1, len(enc)))(*enc)
        m.keep.append((enc, carr))
        arr[i].name = name.encode()
        arr[i].type = ltype
        arr[i].n_items = len(enc)
        arr[i].items = C.cast(carr, C.POINTER(C.c_char_p))
    m.keep.append(arr)
    return arr, len(lists)


def marshal_geoip(entries, m):
    """entries: numpy structured array (see pingoo_amd.batch.GEOIP_DTYPE) or None -> pointer or None."""
    if entries is None:
        return None
    import numpy as np

    entries = np.ascontiguousarray(entries)
    assert entries.dtype.itemsize == C.sizeof(GeoipEntry), entries.dtype
    t = GeoipTable()
    t.entries = C.cast(entries.ctypes.data, C.POINTER(GeoipEntry))
    t.n_entries = len(entries)
    m.keep.append((entries, t))
    return C.pointer(t)
