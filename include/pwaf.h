/*
 * pwaf.h — C ABI of the MI355X batched WAF rule-matching engine (libpwaf.so).
 *
 * This is the drop-in boundary for ONE hot path of pingooio/pingoo: the per-request
 * rule evaluation that the reference runs inline in its hyper request closure.
 * The reference has no FFI/plugin seam for this path, so every entry
 * point below cites the reference code it replaces. All citations are relative to
 * the reference tree.
 *
 *   reference construct                                        replaced by
 *   ---------------------------------------------------------  ---------------------------
 *   rules::compile_expression        rules/rules.rs:45-53      pwaf_compile_expression
 *   rules::validate_expression       rules/rules.rs:55-77      pwaf_validate_expression
 *   Vec<Rule> + lists + GeoipDB      pingoo/server.rs:40-47,76 pwaf_engine_create
 *   rule loop + gates                http_listener.rs:196-264  pwaf_evaluate_batch / _one
 *   Rule::match_request              pingoo/rules.rs:37-51     (inside the batch evaluation)
 *   GeoipDB::lookup                  pingoo/geoip.rs:73-91     (device trie, or caller-supplied asn/country)
 *   geoip record -> RequestContext   http_listener.rs:143-157,183-191; upstream headers http_proxy_service.rs:174-189
 *                                                              pwaf_geoip_lookup / pwaf_evaluate_*_geo (PWAF_OPT_GEO_ANSWERS)
 *   get_host / get_path / UA derive  http_listener.rs:140-165,284-296; http_utils.rs:114-116
 *                                                              pwaf_derive_host / _path / _user_agent; pwaf_derive_batch
 *   generate_captcha_client_id       http_listener.rs:167; pingoo/captcha.rs:409-421
 *                                                              pwaf_client_id_one / pwaf_client_ids
 *   cookie split + validate_captcha_verified_cookie            http_listener.rs:169-181,222-236; pingoo/captcha.rs:125-156; jwt/jwt.rs:198-327
 *                                                              pwaf_verify_cookie_one / pwaf_verify_cookies (pwaf_keyset)
 *   CaptchaManager::api_verify up to issuing the cookie      pingoo/captcha.rs:241-333; jwt/jwt.rs:198-327
 *                                                              pwaf_verify_pow_one / pwaf_verify_pow (pwaf_keyset)
 *   serde_json::from_reader -> CaptchaVerifyRequestBody      pingoo/captcha.rs:50-57,291
 *                                                              pwaf_parse_pow_body_one / pwaf_parse_pow_bodies
 *   which response a request gets    http_listener.rs:196-272; pingoo/captcha.rs:158-174
 *                                                              pwaf_respond_one / pwaf_respond
 *
 * Plain pointers and sizes only; no C++/torch types. Never aborts across the ABI:
 * every failure is an int status (<0) plus pwaf_last_error().
 */
#ifndef PWAF_H
#define PWAF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PWAF_ABI_VERSION 4u /* 2: pwaf_batch carries header columns; strict rule compilation by default (PWAF_OPT_LENIENT, PWAF_W_PARTIAL);
                            * residual rules; pwaf_request carries header values; pwaf_node_evaluate_device; pwaf_program_tune
                            * 3: page-locked host memory for batch columns (pwaf_host_alloc / _register); no struct changed
                            * 4: request records, non-blocking queue; no existing struct changed
                            *    + GeoIP answers: new symbols only */

/* ---- status codes ------------------------------------------------------------------ */
#define PWAF_OK 0
#define PWAF_E_INVALID_ARG (-1)  /* NULL pointer, bad struct_size, bad enum value            */
#define PWAF_E_SYNTAX (-2)       /* == rules::Error::ExpressionIsNotValid (rules/rules.rs:41) */
#define PWAF_E_UNSUPPORTED (-3)  /* valid expression outside the device-compilable subset     */
#define PWAF_E_LIST (-4)         /* list item does not parse (pingoo/lists.rs:93-108)         */
#define PWAF_E_DEVICE (-5)       /* HIP error / no GPU: host may fail open                    */
#define PWAF_E_BATCH (-6)        /* malformed batch (offsets not monotone, bad country, ...)  */
#define PWAF_E_NOMEM (-7)
#define PWAF_E_BUSY (-8)         /* non-blocking queue full: nothing was queued, submit again later (ABI 4)            */
#define PWAF_W_PARTIAL 1          /* (positive: a warning, the object WAS created) with PWAF_OPT_LENIENT some rule is not evaluated */

/* ---- verdict vocabulary (rules::Action, rules/rules.rs:30-35) ------------------------ */
#define PWAF_ACTION_ALLOW 0u   /* no rule fired: proceed to routing (http_listener.rs:266)   */
#define PWAF_ACTION_BLOCK 1u   /* Action::Block {}   -> 403 (http_listener.rs:255)           */
#define PWAF_ACTION_CAPTCHA 2u /* Action::Captcha {} -> captcha page (http_listener.rs:256)  */
#define PWAF_ACTION_BYPASS 3u  /* path under /__pingoo/captcha: rules skipped (:200-204)     */

#define PWAF_RULE_NONE 0xFFFFFFFFu             /* verdict not caused by a rule (Allow)       */
#define PWAF_RULE_UA_GATE 0xFFFFFFFEu          /* UA empty or >=256 B (http_listener.rs:196) */
#define PWAF_RULE_CAPTCHA_ENDPOINT 0xFFFFFFFDu /* http_listener.rs:200                        */

/* action kinds inside a rule description (serde tag "action": block | captcha) */
#define PWAF_RULE_ACTION_BLOCK 1u
#define PWAF_RULE_ACTION_CAPTCHA 2u

typedef struct pwaf_engine pwaf_engine;   /* compiled rules + device tables (immutable, thread-safe) */
typedef struct pwaf_program pwaf_program; /* host-side compiled form only (no GPU needed)            */

/* One rule == pingoo::rules::Rule {name, expression: Option<Program>, actions} (pingoo/rules.rs:9-14).
 * Array order == evaluation order (first match wins, http_listener.rs:251-264). */
typedef struct pwaf_rule_desc {
    const char *name;       /* NUL-terminated, for diagnostics                         */
    const char *expression; /* NUL-terminated; NULL == match-all (pingoo/rules.rs:48-50) */
    const uint8_t *actions; /* PWAF_RULE_ACTION_*, in order                            */
    uint32_t n_actions;
    uint32_t reserved;
} pwaf_rule_desc;

/* One list == pingoo/lists.rs:11-15. Items are the raw CSV column-0 strings; the engine trims
 * them and parses Int / IpNetwork exactly where the reference does (lists.rs:90-108). */
#define PWAF_LIST_STRING 0u
#define PWAF_LIST_INT 1u
#define PWAF_LIST_IP 2u
typedef struct pwaf_list_desc {
    const char *name;
    uint32_t type;
    uint32_t n_items;
    const char *const *items;
} pwaf_list_desc;

/* GeoIP prefix table: the decoded content of a MaxMind DB as the reference consumes it
 * (pingoo/geoip.rs:17-23: asn u32, country 2 x 'A'..'Z'). Longest prefix wins. */
typedef struct pwaf_geoip_entry {
    uint8_t addr[16];  /* v4: first 4 bytes, network order; v6: all 16 */
    uint8_t prefix_len;
    uint8_t is_v6;
    uint8_t country[2];
    uint32_t asn;
} pwaf_geoip_entry;
typedef struct pwaf_geoip_table {
    const pwaf_geoip_entry *entries;
    size_t n_entries;
} pwaf_geoip_table;

/* ---- data-file readers (the callers' data formats on either side of the path) ----------------------------- */
/* Flattens a MaxMind DB (the uncompressed content of geoip.mmdb; for .zst see pwaf_geoip_from_file_image) into the prefix table above: one entry per network of the search tree, IPv4 networks of an IPv6 database (those
 * below ::/96) emitted as IPv4 entries as well. Records are read the way the reference deserialises them (pingoo/geoip.rs:17-23,
 * serde_utils.rs:1-9): {"asn": "AS<digits>" string, "country": two upper-case letters}; a record that would make the
 * reference's lookup fail yields the default {0, "XX"} for its network (http_listener.rs:143-157). Replaces
 * maxminddb::Reader::from_source + lookup (geoip.rs:57,73-91). *entries_out is malloc'ed: release with pwaf_geoip_free. */
int pwaf_geoip_from_mmdb(const uint8_t *mmdb, size_t len, pwaf_geoip_entry **entries_out, size_t *n_out);
void pwaf_geoip_free(pwaf_geoip_entry *entries);
/* zstd::decode_all for `.zst` databases (pingoo/geoip.rs:49-55; the reference's Docker image ships geoip.mmdb.zst): libzstd is loaded
 * at run time; PWAF_E_UNSUPPORTED when it is not installed. *out is malloc'ed: release with pwaf_buffer_free. */
int pwaf_zstd_decompress(const uint8_t *src, size_t len, uint8_t **out, size_t *out_len);
void pwaf_buffer_free(uint8_t *);
/* GeoipDB::load on a file image: decompresses when `path` ends in ".zst" (geoip.rs:49-55), then pwaf_geoip_from_mmdb. */
int pwaf_geoip_from_file_image(const char *path, const uint8_t *content, size_t len, pwaf_geoip_entry **entries_out, size_t *n_out);
/* The list-file format of pingoo/lists.rs:62-117: CSV without header, 1 or 2 columns, the first column trimmed is the item.
 * Returns the items as malloc'ed NUL-terminated strings for pwaf_list_desc.items: release with pwaf_list_free. */
int pwaf_list_parse_csv(const char *text, size_t len, char ***items_out, size_t *n_out);
void pwaf_list_free(char **items, size_t n);

#define PWAF_OPT_NO_UA_GATE 1u        /* skip gate A (http_listener.rs:196-198)             */
#define PWAF_OPT_NO_CAPTCHA_BYPASS 2u /* skip gate B (http_listener.rs:200-204)             */
#define PWAF_OPT_STRICT 8u            /* (deprecated: strict is the default since ABI 2) */
#define PWAF_OPT_LENIENT 32u          /* a rule neither the column compiler nor the residual interpreter can take does NOT fail creation:
                                       * that rule alone never matches, pwaf_program_rule_status / the warnings say why, and creation
                                       * returns PWAF_W_PARTIAL instead of PWAF_OK. Default (ABI 2): creation fails with the rule's index —
                                       * the reference evaluates every valid expression (pingoo/rules.rs:37-51), a silently dropped Block
                                       * rule is a fail-open hole */
#define PWAF_OPT_GLOBAL_VERDICT_TABLES 128u /* testing: the verdict kernel variant for programs whose tables do not fit LDS (same verdicts) */
#define PWAF_OPT_SPARSE_VERDICT 16384u /* A-B / testing: the verdict kernel with the round-5 SPARSE column file (dirty bits + rank per 32 columns) instead of the entry list (same verdicts) */
#define PWAF_OPT_DENSE_VERDICT 2048u  /* A-B / testing: the verdict kernel with the round-4 DENSE column file (8 bytes per column and wave) instead of the sparse one (same verdicts) */
#define PWAF_OPT_TINY_VERDICT_SLOTS 4096u /* testing: 8 entry slots per wave (with PWAF_OPT_SPARSE_VERDICT: 8 value slots of the sparse column file), so that every group takes the spill path (same verdicts) */
#define PWAF_OPT_NO_DENSE_SWITCH 65536u /* A-B / testing: a pass whose prefilter flags most of the arena is still confirmed chunk by chunk (round 5), never walked whole (same verdicts) */
#define PWAF_OPT_EAGER_CMP 32768u      /* A-B / testing: every length / port comparison is evaluated per group by the attribute kernel (round 5), none lazily by the verdict kernel (same verdicts) */
#define PWAF_OPT_NO_DIR_SUMMARY 8192u  /* A-B / testing: IPv4 lookups always gather from the compressed DIR-24 table, without the summary bitmap in front of it (same verdicts) */
#define PWAF_OPT_GEO_ANSWERS 256u     /* the engine also keeps RECORD tables and answers each request's GeoIP record: pwaf_geoip_lookup,
                                       * pwaf_evaluate_*_geo, pwaf_async_create_geo (see "GeoIP answers" below). Without it those return
                                       * PWAF_E_UNSUPPORTED and nothing about the engine differs: memory, creation time, launches, verdicts */
#define PWAF_OPT_RULE_HITS 131072u    /* the engine can report EVERY rule that matches a request, not only the deciding one: pwaf_evaluate_batch_hits /
                                       * pwaf_evaluate_device_hits. A rule whose actions can never take effect (an empty action list: an observe-only
                                       * rule) is then kept, matched and reported, and never decides a verdict. Not with PWAF_OPT_SPARSE_VERDICT /
                                       * PWAF_OPT_DENSE_VERDICT (PWAF_E_INVALID_ARG). Without the flag nothing about the engine differs. */
#define PWAF_OPT_NO_RESIDUAL 64u      /* do not use the per-request residual interpreter (testing / benchmarking the column path alone) */
#define PWAF_OPT_NO_RESIDUAL_JIT 1024u /* residual rules are INTERPRETED per request (residual_kernel) instead of running as the specialized
                                       * device program compiled by hiprtc when the engine is created (the default): same verdicts */
#define PWAF_OPT_NO_PREFILTER 4u      /* every scan pass walks its DFA over every request (no bigram prefilter): same verdicts */
#define PWAF_OPT_FILTER_STRIDE2 16u   /* prefilters sample every second byte wherever a pass's patterns allow it (default: stride 1
                                       * until pwaf_engine_tune decides per pass from the traffic sample): same verdicts */
#define PWAF_OPT_NO_CONFIRM 512u      /* testing / A-B: no confirm tier — every prefilter candidate is walked through the pass's full DFA
                                       * (the round-3 path): same verdicts */
typedef struct pwaf_options {
    uint32_t struct_size; /* sizeof(pwaf_options) */
    uint32_t flags;
    int32_t device;            /* HIP device ordinal, -1 = current device                 */
    uint32_t lds_table_budget; /* LDS bytes for the hot rows of one DFA table; 0 = default (128 KiB) */
    uint32_t max_dfa_states;   /* per DFA group, <= 32767; 0 = default (32767)                       */
    uint32_t max_table_bytes;  /* per DFA group (L2-resident transition table); 0 = default (3 MiB)  */
    uint32_t reserved[2];
} pwaf_options;

/* Per-rule diagnostics of engine creation. */
typedef struct pwaf_compile_error {
    int32_t code;        /* PWAF_E_* */
    uint32_t rule_index; /* offending rule, or 0xFFFFFFFF */
    char message[248];
} pwaf_compile_error;

/* ---- the batch: struct-of-arrays, one request per index --------------------------------
 * String field i of request r is data[offsets[r] .. offsets[r+1]). offsets has n+1 entries and is
 * non-decreasing, so each field's bytes are contiguous in request order (field-major arena).
 * `data` must be readable for 16 bytes past offsets[n] (PWAF_ARENA_PAD) when memory == DEVICE.
 * Field meaning == RequestData / ClientData (pingoo/rules.rs:16-34) AFTER the reference's own
 * derivation (pwaf_derive_* below). */
#define PWAF_FIELD_HOST 0
#define PWAF_FIELD_URL 1
#define PWAF_FIELD_PATH 2
#define PWAF_FIELD_METHOD 3
#define PWAF_FIELD_USER_AGENT 4
#define PWAF_N_FIELDS 5
#define PWAF_ARENA_PAD 16u

#define PWAF_MEM_HOST 0u
#define PWAF_MEM_DEVICE 1u

#define PWAF_FLAG_CAPTCHA_VERIFIED 1u /* http_listener.rs:222-236 (JWT): the caller's, or pwaf_verify_cookies' flags_out */

typedef struct pwaf_strcol {
    const uint8_t *data;
    const uint32_t *offsets; /* n+1 */
} pwaf_strcol;

typedef struct pwaf_batch {
    uint32_t struct_size; /* sizeof(pwaf_batch) */
    uint32_t n;
    uint32_t memory; /* PWAF_MEM_HOST | PWAF_MEM_DEVICE: where EVERY pointer below lives */
    uint32_t n_headers; /* header columns below (extension, see `headers`); 0 = none */
    pwaf_strcol field[PWAF_N_FIELDS];
    const uint8_t *ip;       /* n x 16; IPv4 in bytes 0..3 (network order), rest ignored  */
    const uint8_t *ip_is_v6; /* n                                                        */
    const uint16_t *port;    /* n; client.remote_port                                    */
    const uint8_t *flags;    /* n; PWAF_FLAG_*                                           */
    /* Optional pre-computed GeoIP (both or neither). When NULL the engine looks the ip up in its
     * own table on the device, or uses {0,"XX"} if it has none (geoip.rs:111-118). */
    const uint32_t *asn;     /* n */
    const uint16_t *country; /* n; two bytes 'A'..'Z' in memory order */
    /* Byte size of each field arena (= offsets[n]). The bigram prefilter streams an arena as one flat byte range, so the launch
     * geometry depends on it. HOST batches: ignored (read from the offsets). DEVICE batches: the caller that built the arenas
     * knows it; 0 = unknown, the engine then reads offsets[n] back with one small synchronous copy per evaluate call. */
    uint32_t field_bytes[PWAF_N_FIELDS];
    uint32_t reserved;
    /* EXTENSION (no reference counterpart: pingoo/rules.rs:16-25 exposes no headers — BASELINE.json configs[4]):
     * one string column per header name the rule set mentions as http_request.headers["name"], in the order of
     * pwaf_engine_header_name(); a request without the header carries the empty string. */
    const pwaf_strcol *headers;    /* n_headers column descriptors (the ARRAY is in host memory; the pointers inside follow `memory`) */
    const uint32_t *header_bytes;  /* n_headers arena sizes (HOST memory, same rule as field_bytes), or NULL */
} pwaf_batch;

typedef struct pwaf_verdict {
    uint8_t action; /* PWAF_ACTION_* */
    uint8_t pad[3];
    uint32_t rule_idx; /* index into the rule array, or PWAF_RULE_* */
} pwaf_verdict;

typedef struct pwaf_counts {
    uint64_t by_action[4]; /* indexed by PWAF_ACTION_* */
} pwaf_counts;

typedef struct pwaf_span {
    const char *data; /* not NUL-terminated */
    uint32_t len;
    uint32_t reserved;
} pwaf_span;

/* One request, for the evaluate(Request)->Action convenience wrapper. */
typedef struct pwaf_request {
    const char *host, *url, *path, *method, *user_agent; /* not NUL-terminated */
    uint32_t host_len, url_len, path_len, method_len, user_agent_len;
    uint8_t ip[16];
    uint8_t ip_is_v6;
    uint8_t flags;
    uint16_t port;
    uint8_t has_geoip; /* 1: asn/country below are valid */
    uint8_t country[2];
    uint8_t pad;
    uint32_t asn;
    /* EXTENSION (ABI 2): header values for rule sets that read http_request.headers["name"]: headers[k] is the value of header name k of
     * the engine (pwaf_engine_header_name(k); an absent header = {NULL, 0}), n_headers <= pwaf_engine_header_count — the rest reads as "".
     * The reference's RequestData has no headers (pingoo/rules.rs:16-25); the call shape served is http_listener.rs:206-264. */
    uint32_t n_headers;
    const struct pwaf_span *headers;
} pwaf_request;

/* ---- expression front-end (no GPU needed) ------------------------------------------------ */
/* rules::compile_expression (rules/rules.rs:45-53): syntax only. 0 or PWAF_E_SYNTAX. */
int pwaf_compile_expression(const char *expression, char *errbuf, size_t errbuf_len);
/* rules::validate_expression (rules/rules.rs:55-77): also rejects "" and the `in` operator. */
int pwaf_validate_expression(const char *expression, char *errbuf, size_t errbuf_len);

/* ---- host-side compilation only (used by engine_create; exported for inspection/tests) ---- */
int pwaf_program_compile(const pwaf_rule_desc *rules, size_t n_rules, const pwaf_list_desc *lists,
                         size_t n_lists, const pwaf_geoip_table *geoip, const pwaf_options *opts,
                         pwaf_program **out, pwaf_compile_error *err);
void pwaf_program_destroy(pwaf_program *);
/* Serialises the compiled tables as a self-describing little-endian blob;
 * returns the byte size; copies at most `cap` bytes into `buf` (buf may be NULL to query). */
size_t pwaf_program_dump(const pwaf_program *, uint8_t *buf, size_t cap);
/* Number of per-rule warnings (statically-erroring expressions that can never match,
 * pingoo/rules.rs:41-45) and their text. */
/* Per caller rule: PWAF_OK, or PWAF_E_UNSUPPORTED with the reason in `msg` when the device compiler cannot evaluate its expression
 * (DESIGN.md §3.5). The reference evaluates any expression (pingoo/rules.rs:37-51); an unsupported rule here never matches — the
 * reference's own behaviour for a rule whose execution fails (rules.rs:41-45) — and the host can see which ones. */
int pwaf_program_rule_status(const pwaf_program *, uint32_t rule_index, char *msg, size_t msg_len);
size_t pwaf_program_warning_count(const pwaf_program *);
const char *pwaf_program_warning(const pwaf_program *, size_t i);

/* ---- engine ------------------------------------------------------------------------------ */
int pwaf_engine_create(const pwaf_rule_desc *rules, size_t n_rules, const pwaf_list_desc *lists,
                       size_t n_lists, const pwaf_geoip_table *geoip /* nullable */,
                       const pwaf_options *opts /* nullable */, pwaf_engine **out,
                       pwaf_compile_error *err /* nullable */);
void pwaf_engine_destroy(pwaf_engine *);
const pwaf_program *pwaf_engine_program(const pwaf_engine *);
/* EXTENSION (header fields): the header names the rule set mentions as http_request.headers["name"] (exact, case-sensitive
 * strings — HTTP/2 and the `http` crate present them in lower case), in the column order pwaf_batch.headers must use. */
uint32_t pwaf_engine_header_count(const pwaf_engine *);
const char *pwaf_engine_header_name(const pwaf_engine *, uint32_t i);
uint32_t pwaf_program_header_count(const pwaf_program *);
const char *pwaf_program_header_name(const pwaf_program *, uint32_t i);
void *pwaf_engine_stream(const pwaf_engine *); /* hipStream_t the synchronous entry points run on */

/* Synchronous batch evaluation. HOST batches are copied to the device, evaluated, and verdicts are
 * copied back into `out` (host, n entries). DEVICE batches are evaluated in place and `out`/`counts`
 * must be device pointers too. `counts` is nullable. Callable concurrently from several threads: an engine owns a small ring of
 * per-call contexts (scratch, staging buffers, stream), so one caller's copies overlap another's kernels. A batch that exhausts
 * the scan overflow pool (more than two distinct matches per pass for very many requests) is evaluated again with a larger pool
 * before the call returns: PWAF_E_NOMEM is only reported when that does not help. */
int pwaf_evaluate_batch(pwaf_engine *, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts);

/* Page-locked host memory for the columns of HOST batches (ABI 3). Where the reference's listener has the request's bytes when the
 * rule loop runs (http_listener.rs:206-219) is host memory; a host that parses into arenas from pwaf_host_alloc (or registers its own
 * with pwaf_host_register) lets pwaf_evaluate_batch's copies run at the link's speed: the copy engine reads such memory directly and
 * the calling thread validates the batch meanwhile. Pageable columns still work (the runtime stages them: slower). Small host batches
 * (under 1 MiB: the micro-batcher's) are packed into one page-locked block inside the engine whatever the caller's memory is. */
int pwaf_host_alloc(size_t bytes, void **out);
void pwaf_host_free(void *);
int pwaf_host_register(void *p, size_t bytes);
int pwaf_host_unregister(void *p);

/* Asynchronous device-resident evaluation on a caller-supplied HIP stream (hipStream_t as void*, passed through
 * unchanged: NULL is HIP's default stream; pwaf_engine_stream() returns the engine's own non-blocking stream). All pointers (batch columns, out, counts, match_idx, n_matches)
 * are device pointers. `match_idx`/`n_matches` (nullable) receive the compacted indices of
 * non-Allow requests (wavefront ballot + prefix-sum compaction; order unspecified).
 * `counts` and `n_matches` are ACCUMULATED into (caller zeroes them). */
int pwaf_evaluate_device(pwaf_engine *, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts,
                         uint32_t *match_idx, uint32_t *n_matches, void *stream);

/* pwaf_evaluate_device is re-entrant: calls from several threads / on several streams each take the next per-call context of the
 * engine's ring (the stream first waits, on the device, for that context's previous user), so two in-flight batches never share
 * scratch. After pwaf_evaluate_device: pwaf_engine_device_status waits for the device and returns PWAF_OK, or PWAF_E_NOMEM when
 * some device-resident batch since the last status call ran out of scan overflow scratch (its verdicts are incomplete: evaluate it
 * again — the pool has been grown to what it asked for; cannot happen below 8 overflowing hits per request on average). */
int pwaf_engine_device_status(pwaf_engine *);

/* Optional tuning from a traffic sample (HOST memory; at most the first 65536 requests are used). Each DFA pass keeps its most
 * visited states in LDS; without a profile those are the shallowest states (BFS order), with one they are the states the sample
 * actually visits. Only speed depends on this: verdicts are identical with any profile. Synchronises the device, then rebuilds
 * and re-uploads the scan tables. No reference counterpart (the reference interprets each rule per request:
 * pingoo/rules.rs:37-51); the closest analogue is warming its caches. */
int pwaf_engine_tune(pwaf_engine *, const pwaf_batch *sample);
/* The host half of the same tuning on a compiled PROGRAM (no device needed): the program's bigram prefilters are replaced by the
 * ones rebuilt for the sample, and show up in pwaf_program_dump. Lets a deployment (and the CPU tests) inspect what tuning would
 * do to the tables before any engine exists; an engine is not affected. */
int pwaf_program_tune(pwaf_program *, const pwaf_batch *sample);

/* evaluate(Request) -> Action: a batch of one (north_star's RuleEngine::evaluate façade). */
int pwaf_evaluate_one(pwaf_engine *, const pwaf_request *req, pwaf_verdict *out);

/* ---- one process, every GPU of the node ---------------------------------------------
 * The reference builds its rule state once per process and shares it with every listener (pingoo/server.rs:40-47,76,111-134);
 * a pwaf_node is that object for a multi-GPU host: one engine replica per device (tables are tens of MB), a HOST batch is cut
 * into contiguous 64-aligned slabs (pwaf_node_shard_bounds), each slab is evaluated by its device on its own host thread and
 * stream, verdicts land in `out` at the slab's position and the four action counters are summed on the host. No data-path
 * exchange between devices. (bench.py's process-per-GPU mode does the same with an RCCL all-reduce of the counters.) */
typedef struct pwaf_node pwaf_node;
int pwaf_node_create(const pwaf_rule_desc *rules, size_t n_rules, const pwaf_list_desc *lists, size_t n_lists,
                     const pwaf_geoip_table *geoip /* nullable */, const pwaf_options *opts /* nullable; .device is ignored */,
                     const int *devices, size_t n_devices, pwaf_node **out, pwaf_compile_error *err /* nullable */);
void pwaf_node_destroy(pwaf_node *);
size_t pwaf_node_device_count(const pwaf_node *);
pwaf_engine *pwaf_node_engine(const pwaf_node *, size_t i);
int pwaf_node_tune(pwaf_node *, const pwaf_batch *sample);
int pwaf_node_evaluate_batch(pwaf_node *, const pwaf_batch *in /* HOST */, pwaf_verdict *out /* n */, pwaf_counts *counts /* nullable */);
/* DEVICE-resident slabs, one per device of the node (ABI 2): batches[r] lives on device r (its slab of the request stream:
 * pwaf_node_shard_bounds), outs[r] / counts[r] (nullable, ACCUMULATED into like pwaf_evaluate_device's) are device pointers on device
 * r, streams[r] (nullable array / entries) is a HIP stream of device r. No host staging: the enqueue runs on the node's persistent
 * per-device host threads in parallel and returns without waiting for the devices. Replaces, for a single-process host, what
 * pingoo/server.rs:111-134 does when it hands the shared rule state to every listener. */
int pwaf_node_evaluate_device(pwaf_node *, const pwaf_batch *const *batches, pwaf_verdict *const *outs, pwaf_counts *const *counts, void *const *streams);
/* Waits for every device; PWAF_E_NOMEM when a device-resident slab since the last call ran out of scan scratch (see pwaf_engine_device_status). */
int pwaf_node_synchronize(pwaf_node *);
/* The path's only cross-device exchange — the sum of the four action counters — as an RCCL all-reduce over xGMI, in place on the
 * per-device counters: comms[r] = the caller's ncclComm_t for device r (librccl.so is loaded on first use). Hosts that add the 4 x 8
 * bytes per device up themselves do not need it. */
int pwaf_node_allreduce_counts(pwaf_node *, void *const *comms, pwaf_counts *const *counts, void *const *streams);
/* Slab [lo, hi) of device `rank` out of `world` for a batch of n requests. */
void pwaf_node_shard_bounds(uint32_t n, uint32_t rank, uint32_t world, uint32_t *lo, uint32_t *hi);

/* ---- deadline micro-batcher ------------------------------------------------------ */
/* The reference evaluates rules once per request on the tokio worker that owns the connection (http_listener.rs:196-264); a
 * drop-in RuleEngine::evaluate(Request) -> Action keeps that call shape. The batcher gathers concurrent callers: each call blocks
 * until its batch — closed when it holds max_batch requests, when its oldest request has waited max_delay_us, or (early close) when
 * every caller currently inside the call is already waiting in a batch and the oldest has waited max_delay_us / 8: callers block, so
 * nobody else can join before somebody is answered — has gone through pwaf_evaluate_batch. Thread-safe; two dispatcher threads per batcher (one gathers and submits the next batch while the other waits for its own on the device). Destroy it before the engine. */
typedef struct pwaf_batcher pwaf_batcher;
int pwaf_batcher_create(pwaf_engine *engine, uint32_t max_batch, uint32_t max_delay_us, pwaf_batcher **out);
int pwaf_batcher_evaluate(pwaf_batcher *, const pwaf_request *req, pwaf_verdict *out);
int pwaf_batcher_stats(pwaf_batcher *, uint64_t *n_batches, uint64_t *n_requests);
void pwaf_batcher_destroy(pwaf_batcher *);

/* ---- request records (ABI 4) ---------------------------------------------------------------------
 * A record holds ONE request, self-contained: what a host writes while it handles requests one at a time (pingoo's listener has them one
 * per hyper closure, http_listener.rs:133-274). Records live in one buffer, each at a 16-byte aligned offset:
 *   pwaf_record_head                                  (36 bytes)
 *   uint32_t len[n_values]                            value lengths
 *   zero padding up to the next 16-byte boundary of the record
 *   the values' bytes back to back                    (no padding between values)
 *   zero padding up to `size`
 * Value order: host, url, path, method, user_agent (PWAF_FIELD_*), then the engine's header columns in pwaf_engine_header_name order.
 * 5 <= n_values <= 5 + pwaf_engine_header_count; the values a record does not carry read as "" (the rule of pwaf_request.headers).
 * A buffer of records is evaluated by pwaf_evaluate_records; pwaf_async_submit writes them itself. */
typedef struct pwaf_record_head {
    uint32_t size;     /* whole record in bytes, a multiple of 16 */
    uint16_t n_values; /* value lengths that follow the head */
    uint16_t port;     /* client.remote_port */
    uint8_t ip[16];    /* IPv4 in bytes 0..3 (network order) */
    uint32_t asn;      /* with has_geoip */
    uint8_t country[2];/* with has_geoip: two letters 'A'..'Z' */
    uint8_t flags;     /* PWAF_FLAG_* */
    uint8_t ip_is_v6;
    uint8_t has_geoip; /* 0 or 1, the same for every record of one call */
    uint8_t reserved[3];
} pwaf_record_head;

/* Synchronous evaluation of n records of a HOST buffer. Verdict i (out: n entries, host memory) belongs to the record at byte offset
 * rec_off[i] of buf (any order; records may be shared or skipped). The host reads only the record heads and lengths: it validates every
 * record and refuses the whole call with PWAF_E_BATCH, naming the record's index, when an offset is not 16-byte aligned, a record runs past
 * buf_bytes, its lengths overflow its size, n_values is out of range, a country is not two letters A-Z, has_geoip differs between records
 * or a column would exceed 4 GiB; nothing is launched then. The value bytes travel to the device as they are — one copy straight from
 * page-locked memory (pwaf_host_alloc / pwaf_host_register), else staged through the engine's own page-locked block — and
 * unpack_records_kernel writes the device batch's columns. Overflow-pool retries as in pwaf_evaluate_batch. `counts` is nullable. */
int pwaf_evaluate_records(pwaf_engine *, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n, pwaf_verdict *out,
                          pwaf_counts *counts);

/* ---- record export (ABI 4, additive) -------------------------------------------------------------------
 * The inverse of the above: selected requests of a batch, as records. For a device-resident batch the engine names the requests it did
 * not allow as an index list (match_idx / n_matches of pwaf_evaluate_device); this call turns such a list into the records of those
 * requests — a block log, a quarantine file, an offline replay, a second look through another engine — without copying the batch to the
 * host: evaluate, export, copy out exactly bytes_needed bytes, feed them to anything that takes records. It takes no engine (like
 * pwaf_host_alloc): everything it needs is in the batch. Verdicts and GeoIP answers are not part of a record: index out[] / geo[] with
 * the same idx. The reference has no counterpart (it handles one request at a time, http_listener.rs:133-274).
 * Memory and streams: in->memory says where EVERY pointer lives, the batch's and idx, n_idx, buf, rec_off and stats alike.
 *   PWAF_MEM_DEVICE  the work is enqueued on `stream` (hipStream_t; NULL = HIP's default stream) of the current device and the call
 *                    returns at once: one 16-byte memset of *stats and one launch (pack_records_kernel). The kernel reads *n_idx itself,
 *                    so a call placed right behind pwaf_evaluate_device(..., match_idx, n_matches, stream) on the same stream needs no
 *                    synchronisation in between. No memory is allocated, nothing is copied. The batch is trusted as
 *                    pwaf_evaluate_device trusts it (the kernel's 16-byte loads count on PWAF_ARENA_PAD behind every arena, as the
 *                    evaluation's do), except that the kernel itself guards idx[j] >= n.
 *   PWAF_MEM_HOST    synchronous, plain C++, no HIP call: works on a machine without a GPU. A selected request whose offsets decrease
 *                    in some column refuses the whole call with PWAF_E_BATCH (naming the list entry) before anything is written.
 * Output: n_selected = min(*n_idx, idx_cap) list entries are looked at (idx_cap when n_idx == NULL). For entry j < n_selected, rec_off[j]
 * is the byte offset in buf of the record of request idx[j], or PWAF_RECORD_NONE when the record did not fit, when idx[j] >= in->n or
 * when the record would exceed 0xFFFFFFF0 bytes; entries j >= n_selected are not written. Records sit at 16-byte aligned offsets, in
 * unspecified order, without holes: the written ones occupy a prefix of buf. Nothing is written at or beyond buf + buf_cap. Duplicates in
 * idx produce one record each. *stats is overwritten, not accumulated into; bytes_needed counts every valid selected record whether or
 * not it fitted. buf_cap == 0 (buf NULL or not) is a size query. Which records are dropped when buf_cap < bytes_needed is unspecified;
 * with buf_cap >= bytes_needed none is.
 * Record content: exactly what pwaf_evaluate_records takes. Values: the five fields, then the batch's n_headers header columns, in that
 * order; n_values ends after the last non-empty header value (5 when there is none); a header column whose descriptor is NULL reads as
 * ""; has_geoip = 1 with asn / country iff the batch carries both columns, else those fields are 0; flags, port, ip, ip_is_v6 are
 * copied; reserved and all padding are 0. Offsets need not begin at 0: a slab of a larger batch is a valid input.
 * PWAF_E_INVALID_ARG, before anything runs: NULL in, rec_off or stats; NULL idx with idx_cap > 0; a bad struct_size or memory; a NULL
 * field or numeric column, or NULL headers with n_headers > 0, in a batch with n > 0; n_headers above 120; buf not 16-byte aligned;
 * buf == NULL with buf_cap != 0; buf_cap > 0xFFFFFFF0 (rec_off is 32 bits wide). */
#define PWAF_RECORD_NONE 0xFFFFFFFFu
typedef struct pwaf_export_stats {
    uint64_t bytes_needed; /* bytes of ALL selected valid records: a buf_cap >= this writes every one */
    uint32_t n_selected;   /* list entries looked at: min(*n_idx, idx_cap), or idx_cap when n_idx == NULL */
    uint32_t n_written;    /* records written to buf */
} pwaf_export_stats;       /* 16 bytes */
int pwaf_export_records(const pwaf_batch *in, const uint32_t *idx, uint32_t idx_cap, const uint32_t *n_idx /* nullable */, uint8_t *buf,
                        size_t buf_cap, uint32_t *rec_off /* idx_cap entries */, pwaf_export_stats *stats, void *stream);

/* ---- captcha client ids (ABI 4, additive) ---------------------------------------------------------------
 * generate_captcha_client_id (http_listener.rs:167, pingoo/captcha.rs:409-421): base64url_nopad(SHA-256(ip octets || user_agent || host)),
 * the id that binds the verified-cookie JWT to a client (captcha.rs:125-156), is handed to the captcha endpoints (http_listener.rs:202)
 * and is the `sub` of the challenge issued when a rule answers Captcha (captcha.rs:194-201, :437). The reference computes it for every
 * request; a host that evaluates device-resident batches needs it for the requests of the match list whose verdict is CAPTCHA (or BYPASS
 * on the captcha endpoints), and gets it here without copying their User-Agent and host bytes back. Cookie parsing, JWT verification and
 * the proof of work stay on the host. pwaf_client_ids takes no engine (like pwaf_export_records): everything it needs is in the batch.
 * Message of request i: ip[i] (its first 4 bytes when ip_is_v6[i] == 0, else all 16; bytes 4..15 of an IPv4 row are ignored), then the
 * bytes of field[PWAF_FIELD_USER_AGENT], then those of field[PWAF_FIELD_HOST] of request i — as the batch carries them, at any length
 * (derivation, pwaf_derive_*, is the caller's job, as it is for evaluation). The digest's 32 bytes are encoded with the URL-safe
 * alphabet without padding (captcha.rs:420): 43 characters, then text[43] = 0.
 * Which requests: idx == NULL (idx_cap must be 0 and n_idx NULL): every request, out[i] belongs to request i (in->n entries). Otherwise
 * m = min(*n_idx, idx_cap), or idx_cap when n_idx == NULL, and out[j] belongs to request idx[j] for j < m; entries j >= m are not
 * written; idx[j] >= in->n writes 44 zero bytes (the empty string); duplicates each get their entry. Nothing is written at or beyond
 * out + m (out + n).
 * Memory and streams: in->memory says where EVERY pointer lives, the batch's and idx, n_idx and out alike.
 *   PWAF_MEM_DEVICE  one launch (client_id_kernel) is enqueued on `stream` (hipStream_t; NULL = HIP's default stream) of the current
 *                    device and the call returns at once. The kernel reads *n_idx itself, so a call placed right behind
 *                    pwaf_evaluate_device(..., match_idx, n_matches, stream) on the same stream needs no synchronisation in between.
 *                    Nothing is allocated, nothing is copied. Loads may run past a value by fewer than 16 bytes: inside the arena or its
 *                    PWAF_ARENA_PAD, the contract pwaf_export_records relies on. The batch is trusted as pwaf_evaluate_device trusts it,
 *                    except that the kernel itself guards idx[j] >= n.
 *   PWAF_MEM_HOST    synchronous, plain C++, no HIP call: works on a machine without a GPU, and reads no byte outside a value (no pad is
 *                    assumed). A selected request whose offsets decrease in either column refuses the whole call with PWAF_E_BATCH
 *                    (naming the entry) before anything is written.
 * PWAF_E_INVALID_ARG, before anything runs: NULL in or out; a bad struct_size or memory; idx == NULL with idx_cap != 0 or n_idx != NULL;
 * out not 4-byte aligned; in a batch with n > 0 a NULL ip, ip_is_v6, or User-Agent / host column. The other columns of the batch are
 * not looked at and may be NULL.
 * pwaf_client_id_one: the same id from req->ip, ip_is_v6, user_agent and host, on the host (no GPU): what a per-request closure calls
 * where the reference calls generate_captcha_client_id. */
typedef struct pwaf_client_id {
    char text[44]; /* 43 characters of the URL-safe alphabet (A-Z a-z 0-9 - _), then NUL */
} pwaf_client_id;
int pwaf_client_ids(const pwaf_batch *in, const uint32_t *idx /* nullable */, uint32_t idx_cap, const uint32_t *n_idx /* nullable */,
                    pwaf_client_id *out, void *stream);
int pwaf_client_id_one(const pwaf_request *req, pwaf_client_id *out);

/* ---- captcha-verified cookies (ABI 4, additive) -------------------------------------------------------------
 * Gate C of the reference (http_listener.rs:169-181, :222-236): split the Cookie header, find `__pingoo_captcha_verified`, and run
 * CaptchaManager::validate_captcha_verified_cookie (pingoo/captcha.rs:125-156) on it, which is jwt::parse_header, the key looked up by
 * `kid`, and jwt::parse_and_verify (jwt/jwt.rs:198-327: an Ed25519 signature, then exp / nbf / aud / iss), then sub == client id and
 * challenge_passed. The answer is PWAF_FLAG_CAPTCHA_VERIFIED of pwaf_batch.flags, which until now had to be made on the host, request by
 * request. pwaf_verify_cookies answers it for every request of a batch, or for the requests a list names, where the batch lives, and can
 * write the flags column the evaluation reads next on the same stream. It takes no engine (like pwaf_client_ids). DESIGN.md §5.1.6
 * states the semantics rule by rule; in short:
 *   cookie  a header value with a byte that is neither TAB nor 0x20..0x7E has no cookies; split on ';', each segment trimmed and cut at
 *           its first '='; the first cookie named exactly `__pingoo_captcha_verified` is the token, a pair of '"' around it removed.
 *   token   three parts; the third is base64url without padding of exactly 64 bytes; the header names the key by `kid` (alg "EdDSA",
 *           typ "JWT"); Ed25519 as aws-lc's ED25519_verify does it; then the claims: exp >= now - 5, nbf <= now + 5, aud == iss ==
 *           "pingoo", challenge_passed == true, sub == the client id computed from ip, User-Agent and host (pwaf_client_ids' message).
 *   subset  header and claims are read in a flat subset of JSON (one object, no escapes, no nesting, integers). A token outside it, or
 *           whose signed part is longer than PWAF_COOKIE_MAX_SIGNED_BYTES, is UNDECIDED if its signature verifies under a key of the set
 *           (the holder of a signing key wrote it: the host decides with its own library) and INVALID otherwise.
 * Keys (captcha.rs:77-123, :525-548; jwt/jwk.rs): pwaf_keyset_create decompresses each x (an encoding that is not a canonical point on
 * the curve: PWAF_E_INVALID_ARG), precomputes the multiples of -A the verifier adds, and uploads them with the kids to `device`
 * (device < 0: host only; the DEVICE mode then answers PWAF_E_DEVICE). 1..PWAF_KEYSET_MAX_KEYS keys, each kid 1..PWAF_KEYSET_MAX_KID
 * bytes (captcha.rs:526 refuses an empty one); two keys with one kid are refused. The set is read-only afterwards: any number of calls
 * on any streams may share it. pwaf_keyset_destroy(NULL) is a no-op; destroy after the last call that uses the set has run.
 * pwaf_verify_cookies: `cookies` holds each request's FIRST Cookie header value ("" when there is none; the reference looks at no
 * other, http_listener.rs:169-172), `now` is Unix seconds (a parameter: nothing here reads a clock). idx / idx_cap / n_idx mean exactly
 * what they mean for pwaf_client_ids: idx == NULL (idx_cap 0, n_idx NULL): every request, status[i] belongs to request i; otherwise
 * m = min(*n_idx, idx_cap), or idx_cap when n_idx == NULL, status[j] belongs to request idx[j] for j < m, entries j >= m are not written,
 * idx[j] >= in->n gets PWAF_COOKIE_ABSENT. flags_out (nullable, in->n entries) is written only when idx == NULL:
 * (in->flags ? in->flags[i] : 0) with PWAF_FLAG_CAPTCHA_VERIFIED set for VERIFIED and cleared otherwise; it may be in->flags itself.
 * Memory and streams: in->memory says where EVERY pointer lives: the batch's, cookies', idx, n_idx, status and flags_out alike.
 *   PWAF_MEM_DEVICE  a 16-byte memset and two launches (cookie_locate_kernel, cookie_verify_kernel) are enqueued on `stream` (hipStream_t;
 *                    NULL = HIP's default stream) of the current device, which must be the key set's, and the call returns at once. The
 *                    kernels read *n_idx and the number of located tokens themselves, so the call may follow pwaf_evaluate_device on
 *                    the same stream and be followed by one without a synchronisation. scratch: pwaf_verify_cookies_scratch_bytes(k)
 *                    bytes of device memory, 16-byte aligned, k = idx_cap (in->n when idx == NULL), the call's own until the launches
 *                    have run. Loads may run past a value by fewer than 16 bytes (PWAF_ARENA_PAD, the cookies' arena too). The batch is
 *                    trusted as pwaf_evaluate_device trusts it, except that the kernels guard idx[j] >= n.
 *   PWAF_MEM_HOST    synchronous, plain C++, no HIP call; reads no byte outside a value; scratch and stream are ignored. A selected
 *                    request whose offsets decrease in the cookies, User-Agent or host column refuses the call with PWAF_E_BATCH.
 * PWAF_E_INVALID_ARG, before anything runs: NULL ks, in, cookies or status; a bad struct_size or memory; idx == NULL with idx_cap != 0
 * or n_idx != NULL; in a batch with n > 0 a NULL ip, ip_is_v6, cookies / User-Agent / host column; in DEVICE mode scratch NULL, not
 * 16-byte aligned or too small.
 * pwaf_verify_cookie_one: the same answer for one request on the host (no GPU), from req->ip, ip_is_v6, user_agent and host and the
 * first Cookie header's value (cookie == NULL: none): what a per-request closure calls where the reference runs http_listener.rs:222-236. */
#define PWAF_COOKIE_ABSENT 0u    /* no such cookie: captcha_verified = false, the rules run (http_listener.rs:222-227) */
#define PWAF_COOKIE_VERIFIED 1u  /* a valid cookie: captcha_verified = true (:232) */
#define PWAF_COOKIE_INVALID 2u   /* the reference answers serve_captcha() (:234) */
#define PWAF_COOKIE_UNDECIDED 3u /* signed by a key of the set, but not parsed here: the host decides with its own library */
#define PWAF_KEYSET_MAX_KEYS 8u
#define PWAF_KEYSET_MAX_KID 64u
#define PWAF_COOKIE_MAX_SIGNED_BYTES 8192u /* header '.' claims of a token, in base64url characters */
typedef struct pwaf_ed25519_key {
    const char *kid; /* NUL-terminated, 1..PWAF_KEYSET_MAX_KID bytes (jwt/jwk.rs:17) */
    uint8_t x[32];   /* the public key: RFC 8032 §5.1.2 encoding (the JWK's "x", jwt/jwk.rs:32-33) */
} pwaf_ed25519_key;
typedef struct pwaf_keyset pwaf_keyset;
int pwaf_keyset_create(const pwaf_ed25519_key *keys, uint32_t n, int device, pwaf_keyset **out);
void pwaf_keyset_destroy(pwaf_keyset *ks);
size_t pwaf_verify_cookies_scratch_bytes(uint32_t n); /* DEVICE mode scratch for n entries; HOST mode needs none */
int pwaf_verify_cookies(const pwaf_keyset *ks, const pwaf_batch *in, const pwaf_strcol *cookies, int64_t now, const uint32_t *idx /* nullable */,
                        uint32_t idx_cap, const uint32_t *n_idx /* nullable */, uint8_t *status, uint8_t *flags_out /* nullable */, void *scratch,
                        size_t scratch_bytes, void *stream);
int pwaf_verify_cookie_one(const pwaf_keyset *ks, const pwaf_request *req, const char *cookie /* nullable */, uint32_t cookie_len, int64_t now,
                           uint8_t *status);

/* ---- captcha proof-of-work submissions (ABI 4, additive) ----------------------------------------------------
 * A POST to /__pingoo/captcha/api/verify reaches CaptchaManager::api_verify (pingoo/captcha.rs:241-333), which finds the
 * `__pingoo_captcha` cookie, runs jwt::parse_header, looks the key up by `kid`, runs jwt::parse_and_verify into CaptchaCookieJwtClaims
 * (captcha.rs:61-67; jwt/jwt.rs:198-327), reads the body (CaptchaVerifyRequestBody: hash, nonce), and then checks sub == client id, the
 * hash's leading zeroes against the difficulty, and hash == SHA-256(challenge || nonce). The evaluation answers PWAF_ACTION_BYPASS /
 * PWAF_RULE_CAPTCHA_ENDPOINT for these requests and lists them in match_idx; pwaf_verify_pow answers the check for the requests of a
 * batch, or for those a list names, where the batch lives. pwaf_parse_pow_bodies (below) reads hash and nonce out of the bodies where they
 * lie; issuing the verified cookie to a submission that PASSED (captcha.rs:335-346: it needs the signing key) stays the host's; a request
 * without a usable body is not put into the call, or its status is not read.
 * It takes no engine. DESIGN.md §5.1.7 states the semantics rule by rule; in short:
 *   cookie  as pwaf_verify_cookies splits the header, with the name `__pingoo_captcha` exactly (`__pingoo_captcha_verified` is another
 *           cookie). None: ABSENT.
 *   token   three parts, 64 bytes of signature, header with kid / alg "EdDSA" / typ "JWT" as for pwaf_verify_cookies; else FAILED.
 *   claims  read in the flat subset PLUS one escape inside string values: the six bytes \u0000 stand for one byte 0x00 (the reference's
 *           challenge and client id are 43 characters and a NUL, which serde_json writes so). exp >= now - 5, nbf <= now + 5, aud == iss
 *           == "pingoo"; sub's decoded bytes are the 44 bytes of pwaf_client_id.text for the request; challenge a string; difficulty an
 *           integer 0..255; the leading zero nibbles of hash (high nibble of byte 0 first) number at least difficulty; SHA-256(decoded
 *           challenge || nonce) == hash. Any one failing: FAILED, whatever the signature says (every failure of api_verify is one response).
 *   order   the signature is checked LAST, and only for an entry that passed every check above: then PASSED or FAILED. A header or claims
 *           outside the subset, or a signed part above PWAF_COOKIE_MAX_SIGNED_BYTES: UNDECIDED if the signature verifies (under the
 *           header's key; under any key of the set where the header is not parsed), FAILED otherwise. A flood of wrong hashes never
 *           reaches the curve arithmetic.
 * pwaf_verify_pow: `cookies` means what it means for pwaf_verify_cookies (the FIRST Cookie header's value, "" for none); `nonce` is a
 * string column and `hash` 32 bytes per request, both indexed by request like the batch: CaptchaVerifyRequestBody after serde has read it.
 * idx / idx_cap / n_idx, PWAF_MEM_HOST / PWAF_MEM_DEVICE (in->memory says where EVERY pointer lives, hash and nonce included), `now`, the
 * key set, the trust in the batch, PWAF_ARENA_PAD (behind the nonce arena too), scratch (pwaf_verify_pow_scratch_bytes(k), 16-byte
 * aligned) and the stream rules are word for word those of pwaf_verify_cookies above; an entry with idx[j] >= in->n reads PWAF_POW_ABSENT.
 *   PWAF_MEM_DEVICE  a 16-byte memset and two launches (pow_check_kernel, pow_verify_kernel) on `stream`; nothing is allocated or copied.
 *                    Diagnostic: after the stream has run, word 0 (uint32) of scratch holds the number of entries that were handed to
 *                    the signature stage; entries decided by the cheap checks are not among them.
 *   PWAF_MEM_HOST    synchronous, plain C++, no HIP call; reads no byte outside a value. A selected request whose offsets decrease in the
 *                    cookies, nonce, User-Agent or host column refuses the call with PWAF_E_BATCH, naming the entry, nothing written.
 * PWAF_E_INVALID_ARG as for pwaf_verify_cookies, plus: a NULL hash; a NULL nonce, or with n > 0 a NULL nonce column.
 * pwaf_verify_pow_one: the same answer for one request on the host (no GPU); cookie == NULL: no Cookie header. */
#define PWAF_POW_ABSENT 0u    /* no __pingoo_captcha cookie (captcha.rs:247-253) */
#define PWAF_POW_PASSED 1u    /* every check of api_verify holds: the host issues the verified cookie (captcha.rs:335-346) */
#define PWAF_POW_FAILED 2u    /* the reference answers its error response (any of captcha.rs:256-333) */
#define PWAF_POW_UNDECIDED 3u /* signed by a key of the set, but not parsed here: the host decides with its own library */
size_t pwaf_verify_pow_scratch_bytes(uint32_t n); /* DEVICE mode scratch for n entries; HOST mode needs none */
int pwaf_verify_pow(const pwaf_keyset *ks, const pwaf_batch *in, const pwaf_strcol *cookies, const uint8_t *hash /* n x 32 */,
                    const pwaf_strcol *nonce, int64_t now, const uint32_t *idx /* nullable */, uint32_t idx_cap, const uint32_t *n_idx /* nullable */,
                    uint8_t *status, void *scratch, size_t scratch_bytes, void *stream);
int pwaf_verify_pow_one(const pwaf_keyset *ks, const pwaf_request *req, const char *cookie /* nullable */, uint32_t cookie_len,
                        const uint8_t hash[32], const char *nonce /* nullable with nonce_len 0 */, uint32_t nonce_len, int64_t now, uint8_t *status);

/* ---- derived columns of a raw batch (ABI 4, additive) -----------------------------------------------------
 * Every evaluation entry point takes the fields AFTER the reference's own derivation (http_listener.rs:140-165, :284-296;
 * http_utils.rs:114-116). pwaf_derive_host / _path / _user_agent (below) answer it per request on the host; pwaf_derive_batch answers it
 * for a whole batch whose parsed but underived bytes lie in one place — a replay file copied to the device once, a capture — and writes
 * three columns the evaluation reads as they are. It takes no engine (like pwaf_export_records and pwaf_client_ids).
 * Input: raw->field[PWAF_FIELD_HOST] holds the Host header's value bytes, field[PWAF_FIELD_PATH] uri.path(), field[PWAF_FIELD_USER_AGENT]
 * the User-Agent header's value bytes; no other member of *raw is looked at (they may be NULL). extra (nullable) carries what a raw batch
 * has beyond that: uri.host() per request and which of the three sources a request has at all. raw->memory says where EVERY pointer lives:
 * the batch's, extra's columns, out[]'s, stats and scratch. Input offsets need not begin at 0 (a slab view); output offsets do.
 * Per request i, exactly pwaf_derive_path / _user_agent / _host:
 *   path        the raw value without its trailing '/' bytes.
 *   user_agent  "" when PWAF_RAW_HAS_USER_AGENT is clear; "" when a byte of the value is neither TAB nor 0x20..0x7E; else the value
 *               trimmed of ' ' and TAB at both ends, and "" when more than 256 bytes remain (256 are kept).
 *   host        with PWAF_RAW_HAS_URI_HOST: the URI's host trimmed of 0x09..0x0D and 0x20, "" when more than 256 bytes remain; no byte
 *               check; the Host header is not consulted even when the result is "". Otherwise the Host header, taken like the
 *               User-Agent under PWAF_RAW_HAS_HOST_HEADER.
 *   The bytes of a value whose present bit is clear are ignored, and so are unknown bits of a present byte. A NULL uri_host.data or
 *   .offsets means that no request has a URI host: PWAF_RAW_HAS_URI_HOST then counts as clear.
 * Output, out[0] host, out[1] path, out[2] user_agent: offsets[0..n] are always written completely (they are sizes, offsets[0] == 0);
 * data receives the kept bytes back to back, and the PWAF_ARENA_PAD bytes behind the column's last byte are written as zero where they lie
 * below cap, which makes the column a valid PWAF_MEM_DEVICE arena. Nothing is written at or beyond data + cap, offsets + n + 1 or
 * stats + 1, and nothing between bytes[c] + 16 and cap. With bytes[c] + PWAF_ARENA_PAD <= cap the column is complete — always so when cap
 * is at least the raw column's bytes + 16; for host: the Host headers' bytes + the URI hosts' bytes + 16, because each request takes its
 * host from one of the two columns and a batch may take every byte of both — otherwise stats->overflow says so and which of that
 * column's BYTES were written is unspecified: a caller looks at overflow before it reads such a column. n == 0 writes offsets[0] = 0 (where offsets is given), the pads and stats.
 * Memory and streams:
 *   PWAF_MEM_HOST    synchronous, plain C++, no HIP call: works on a machine without a GPU and reads no byte outside a value (no pad is
 *                    assumed). scratch and stream are ignored. A request whose offsets decrease in a column it reads refuses the whole
 *                    call with PWAF_E_BATCH (naming the request and the column) before anything is written.
 *   PWAF_MEM_DEVICE  at most three launches (derive_span_kernel, derive_base_kernel, derive_copy_kernel) are enqueued on `stream`
 *                    (hipStream_t; NULL = HIP's default stream) of the current device and the call returns at once. No memset, nothing
 *                    allocated, nothing copied. scratch: pwaf_derive_scratch_bytes(n) bytes of device memory, 16-byte aligned, the
 *                    call's own until the launches have run. The batch is trusted as pwaf_evaluate_device trusts it. Loads may run
 *                    past a value's end by fewer than 16 bytes, inside the arena or its PWAF_ARENA_PAD (the URI hosts' arena too); they
 *                    never begin before the value. A caller copies its pwaf_batch, points the three fields at out[], sets their
 *                    field_bytes to 0 (the engine then asks for offsets[n] on the same stream) and calls pwaf_evaluate_device on the
 *                    same stream without a synchronisation of its own.
 * PWAF_E_INVALID_ARG, before anything runs: NULL raw, out or stats; a bad struct_size (raw's or extra's) or memory; stats not 8-byte
 * aligned; n > 0xFFFFFFF0 / 256 (a derived host or User-Agent column could pass 32 bits: the caller splits such a batch); with n > 0 a
 * NULL host, path or User-Agent column or a NULL out[c].offsets; a NULL out[c].data with cap != 0; out[c].data not 16-byte aligned or
 * offsets not 4-byte aligned; in DEVICE mode scratch NULL, not 16-byte aligned or smaller than pwaf_derive_scratch_bytes(n). */
#define PWAF_RAW_HAS_URI_HOST 1u    /* req.uri().host() is Some (HTTP/2, absolute-form) */
#define PWAF_RAW_HAS_HOST_HEADER 2u /* a Host header is present */
#define PWAF_RAW_HAS_USER_AGENT 4u  /* a User-Agent header is present */
typedef struct pwaf_raw_columns { /* what a raw batch carries beyond pwaf_batch */
    uint32_t struct_size, reserved;
    pwaf_strcol uri_host;   /* uri.host() bytes per request; data / offsets may be NULL: no request has one */
    const uint8_t *present; /* n x PWAF_RAW_HAS_*; NULL: HOST_HEADER | USER_AGENT for every request, no URI host */
} pwaf_raw_columns;
typedef struct pwaf_derived_col {
    uint8_t *data;
    uint32_t *offsets; /* n+1 */
    uint64_t cap;      /* bytes of data */
} pwaf_derived_col;
typedef struct pwaf_derive_stats { /* 32 bytes, OVERWRITTEN */
    uint64_t bytes[3]; /* offsets[n] of the derived host, path, user_agent column, whether or not it fitted */
    uint32_t n;        /* requests derived */
    uint32_t overflow; /* bit c set: bytes[c] + PWAF_ARENA_PAD > out[c].cap, that column's BYTES are incomplete */
} pwaf_derive_stats;
size_t pwaf_derive_scratch_bytes(uint32_t n); /* DEVICE mode scratch for a batch of n; HOST mode needs none */
int pwaf_derive_batch(const pwaf_batch *raw, const pwaf_raw_columns *extra /* nullable */, pwaf_derived_col out[3] /* host, path, user_agent */,
                      pwaf_derive_stats *stats, void *scratch, size_t scratch_bytes, void *stream);
/* TEST HOOK, CPU: [0] requests per tile, [1] tiles per step of the base launch, [2] requests per workgroup of the copy launch, [3] 0 */
int pwaf_derive_scan_shape(uint32_t out[4]);

/* ---- captcha proof-of-work request bodies (ABI 4, additive) --------------------------------------------------
 * The body of a POST to /__pingoo/captcha/api/verify is what serde_json::from_reader makes CaptchaVerifyRequestBody {#[serde(with = "hex")]
 * hash: [u8; 32], nonce: String} of (pingoo/captcha.rs:50-57, :291); the genuine client sends {"nonce":"<decimal>","hash":"<64 hex>"}
 * (captcha/src/index.tsx:64,145). pwaf_parse_pow_bodies reads the bodies of a batch, or of the requests a list names, where they lie, and
 * writes exactly what pwaf_verify_pow reads next on the same stream: hash[n][32] and a nonce string column, both indexed BY REQUEST, and
 * one status byte per entry (the nonce column is a pwaf_derived_col, as pwaf_derive_batch above writes them). It takes no engine and no key set. DESIGN.md §5.1.8 states the semantics decision by decision (D-B1 to
 * D-B10); in short, with ws = {0x20, 0x09, 0x0A, 0x0D}, read left to right, the FIRST deciding event wins:
 *   subset     ws* '{' members '}' ws*, a member being ws* key ws* ':' ws* value ws*, members separated by ','; key and value are strings
 *              that end at the first '"' behind their opening one; the keys are exactly `hash` and `nonce`, once each, in either order;
 *              hash's text is exactly 64 hexadecimal digits of either case (decoded high nibble first), nonce's text is any bytes below
 *              0x80 (any length, 0 included) and is the value as it stands. That is OK.
 *   MALFORMED  only where the reference's parse certainly fails: an empty or all-ws body; a first byte other than '{' or '['; a key or a
 *              known key's value that does not begin with '"'; a missing ':' ; a byte other than ',' or '}' behind a value; the body's end
 *              inside the object; a string without a closing '"' or with a byte below 0x20; a known key twice; a hash text that is not 64
 *              hexadecimal digits; `hash` or `nonce` missing at '}'; anything but ws behind '}'.
 *   UNDECIDED  everything else: a body longer than PWAF_POW_BODY_MAX_BYTES (nothing of it is read); '[' as the first byte; a '\' inside a
 *              string; a key with a byte >= 0x80 or other than `hash` / `nonce` (serde skips an unknown member's value, which may be any
 *              JSON); a nonce with a byte >= 0x80. The host parses such a body with its own library, as it did before.
 * `bodies` holds each request's body bytes ("" for a request without one); `memory` says where EVERY pointer lives: the column's, idx,
 * n_idx, status, hash, nonce's, stats and scratch. Input offsets need not begin at 0. idx / idx_cap / n_idx mean exactly what they mean
 * for pwaf_client_ids: idx == NULL (idx_cap 0, n_idx NULL): every request, status[i] belongs to request i; otherwise m = min(*n_idx,
 * idx_cap), or idx_cap when n_idx == NULL, status[j] belongs to request idx[j] for j < m, entries j >= m are not written, idx[j] >= n
 * reads PWAF_BODY_NONE, and a request named twice gets the same answer twice.
 * Output: nonce->offsets[0..n] are always written completely (offsets[0] == 0); a request that is not selected, or whose status is not OK,
 * has a nonce of length 0. The hash row of a selected request that is not OK is 32 zero bytes; rows of unselected requests are not
 * written. nonce->data receives the nonces back to back in request order, and the PWAF_ARENA_PAD bytes behind the column's last byte are
 * written as zero where they lie below cap, which makes the column a valid PWAF_MEM_DEVICE arena. Nothing is written at or beyond data +
 * cap, offsets + n + 1, status + m or stats + 1, and nothing between nonce_bytes + 16 and cap. With nonce_bytes + PWAF_ARENA_PAD <= cap
 * the column is complete — always so when cap is at least the bodies' bytes + 16 — otherwise stats->overflow says so and which of the
 * column's BYTES were written is unspecified. The caller reads pwaf_verify_pow's status only where the body status is OK; for MALFORMED
 * it sends the error response (captcha.rs:293-296); for UNDECIDED it runs serde_json as before.
 *   PWAF_MEM_DEVICE  at most one memset (with a list: it zeroes nonce->offsets) and three launches (powbody_parse_kernel,
 *                    powbody_base_kernel, powbody_copy_kernel) are enqueued on `stream` (hipStream_t; NULL = HIP's default stream) of the
 *                    current device and the call returns at once. Nothing is allocated, nothing is copied. The kernels read *n_idx
 *                    themselves, so the call may stand between pwaf_evaluate_device(..., match_idx, n_matches, stream) and
 *                    pwaf_verify_pow on one stream with no synchronisation anywhere. scratch: pwaf_parse_pow_bodies_scratch_bytes(n)
 *                    bytes of device memory, 16-byte aligned, the call's own until the launches have run. The column is trusted as
 *                    pwaf_evaluate_device trusts a batch, except that the kernels guard idx[j] >= n. Loads are 16 bytes at the body's own
 *                    alignment; they may pass a body's end by fewer than 16 bytes (the arena carries PWAF_ARENA_PAD behind its last
 *                    byte) and never begin before the body.
 *   PWAF_MEM_HOST    synchronous, plain C++, no HIP call: works on a machine without a GPU and reads no byte outside a value. scratch
 *                    and stream are ignored. A selected request whose body offsets decrease refuses the call with PWAF_E_BATCH (naming
 *                    the entry) before anything is written.
 * PWAF_E_INVALID_ARG, before anything runs: NULL bodies, status, hash, nonce or stats; a bad memory; idx == NULL with idx_cap != 0 or
 * n_idx != NULL; n > 0xFFFFFFF0 / PWAF_POW_BODY_MAX_BYTES (the nonce column could pass 32 bits: the caller splits such a batch); stats not
 * 8-byte aligned; with n > 0 a NULL bodies column or a NULL nonce->offsets; a NULL nonce->data with cap != 0; nonce->data not 16-byte
 * aligned or offsets not 4-byte aligned; in DEVICE mode scratch NULL, not 16-byte aligned or too small.
 * pwaf_parse_pow_body_one: the same answer for one body on the host (no GPU): status, the 32 bytes (zero unless OK) and the nonce as
 * body[*nonce_at, +*nonce_len) (0, 0 unless OK): what a per-request closure calls in front of pwaf_verify_pow_one. */
#define PWAF_BODY_NONE 0u       /* idx[j] >= n: not a request */
#define PWAF_BODY_OK 1u         /* hash and nonce are what serde_json hands api_verify (captcha.rs:291) */
#define PWAF_BODY_MALFORMED 2u  /* the reference's parse fails: its error response (captcha.rs:293-296) */
#define PWAF_BODY_UNDECIDED 3u  /* outside the subset parsed here: the host parses it with its own library */
#define PWAF_POW_BODY_MAX_BYTES 4096u
typedef struct pwaf_body_stats { /* 32 bytes, OVERWRITTEN */
    uint64_t nonce_bytes;        /* nonce.offsets[n], whether or not it fitted */
    uint32_t n, n_ok, n_malformed, n_undecided; /* entries looked at and their statuses */
    uint32_t overflow;           /* 1: nonce_bytes + PWAF_ARENA_PAD > nonce->cap, the column's BYTES are incomplete */
    uint32_t reserved;
} pwaf_body_stats;
size_t pwaf_parse_pow_bodies_scratch_bytes(uint32_t n); /* DEVICE mode scratch for a batch of n; HOST mode needs none */
int pwaf_parse_pow_bodies(const pwaf_strcol *bodies, uint32_t n, uint32_t memory, const uint32_t *idx /* nullable */, uint32_t idx_cap,
                          const uint32_t *n_idx /* nullable */, uint8_t *status, uint8_t *hash /* n x 32 */, pwaf_derived_col *nonce,
                          pwaf_body_stats *stats, void *scratch, size_t scratch_bytes, void *stream);
int pwaf_parse_pow_body_one(const uint8_t *body, uint32_t len, uint8_t *status, uint8_t hash[32], uint32_t *nonce_at,
                            uint32_t *nonce_len); /* the nonce is body[nonce_at, +nonce_len) */
/* TEST HOOK, CPU: [0] entries per tile, [1] tiles per step of the base launch, [2] requests per workgroup of the copy launch, [3] the
 * least bound on the parse launch's workgroups with a list */
int pwaf_parse_pow_scan_shape(uint32_t out[4]);

/* ---- the listener's response decision (ABI 4, additive) ------------------------------------------------------
 * What the reference's listener produces per request (http_listener.rs:196-272, serve_captcha_request: pingoo/captcha.rs:158-174): WHICH
 * response the request gets, from what the earlier calls wrote where they wrote it — the verdict (pwaf_evaluate_*), the verified-cookie
 * status (pwaf_verify_cookies), the route (pwaf_evaluate_*_routes) and the batch's PWAF_FIELD_PATH column (get_path's value, which both
 * http_listener.rs:141 and captcha.rs:164 use) — plus ordered lists of request indices, by kind of response, that the follow-up calls take
 * as they stand. It takes no engine and no key set. DESIGN.md §5.1.9 states it row by row; the FIRST row that applies decides:
 *   1  rule_idx == PWAF_RULE_UA_GATE      BLOCKED, arg PWAF_RULE_UA_GATE (gate A, :196-198)
 *   2  action == PWAF_ACTION_BYPASS       by the path, in captcha.rs:165-173's order: starts with /__pingoo/captcha/assets: CAPTCHA_ASSET;
 *                                         equals /__pingoo/captcha/api/init: CAPTCHA_INIT; equals /__pingoo/captcha/api/verify:
 *                                         CAPTCHA_VERIFY; anything else: CAPTCHA_NOT_FOUND. arg PWAF_RULE_CAPTCHA_ENDPOINT (gate B, :200-204)
 *   3  cookie status INVALID              CAPTCHA_PAGE, arg PWAF_RULE_COOKIE (gate C, :233-235)
 *   4  cookie status UNDECIDED            HOST_DECIDES, arg the verdict's rule_idx (the host validates the cookie with its own library and
 *                                         then takes row 3, or reads the verdict as evaluated)
 *   5  action BLOCK / CAPTCHA             BLOCKED / CAPTCHA_PAGE, arg rule_idx (:255, :258)
 *   6  otherwise (ALLOW)                  route == NULL: FORWARD, arg PWAF_ROUTE_NONE; else FORWARD, arg route[i] (:266-270), or NOT_FOUND
 *                                         when route[i] == PWAF_ROUTE_NONE (:272)
 * An invalid cookie therefore does NOT turn a request with an empty User-Agent or one on a captcha endpoint into a captcha page: :196 and
 * :200 run before :222. cookie_status == NULL: every request is ABSENT. Rows 1 and 2 follow the verdict's sentinels, so an engine created
 * with PWAF_OPT_NO_UA_GATE / PWAF_OPT_NO_CAPTCHA_BYPASS needs no special case. pwaf_respond_one, the HOST and the DEVICE mode answer the same.
 * Output: out[i] for every request; counts (nullable, PWAF_RESP_KINDS words, WRITTEN): the requests of each kind; and up to
 * PWAF_RESP_MAX_LISTS lists: list l holds, in ASCENDING request order, the indices of the requests whose kind has its bit set in
 * lists[l].kinds. *lists[l].n is WRITTEN with how many there are, which may exceed cap; only the first min(*n, cap) entries of idx are
 * written, nothing at or beyond idx + cap. Masks may overlap and may be 0 (an empty list, *n == 0); idx may be NULL with cap 0 (count
 * only). A list is exactly what pwaf_client_ids, pwaf_verify_cookies, pwaf_verify_pow, pwaf_parse_pow_bodies and pwaf_export_records take
 * as idx / idx_cap / n_idx. n == 0 writes *n = 0 for every list and zero counts.
 * Memory and streams: in->memory says where EVERY pointer lives: the path column, verdicts, cookie_status, route, out, counts and the idx
 * and n of every list (the `lists` array itself is host memory). Of the batch only n and field[PWAF_FIELD_PATH] are looked at.
 *   PWAF_MEM_DEVICE  at most one 64-byte memset and three launches (respond_classify_kernel, respond_base_kernel, respond_scatter_kernel)
 *                    are enqueued on `stream` (hipStream_t; NULL = HIP's default stream) of the current device and the call returns at
 *                    once. Nothing is allocated, nothing is copied. The call may follow pwaf_verify_cookies and
 *                    pwaf_evaluate_device_routes, and be followed by the list consumers, on one stream without a synchronisation.
 *                    scratch: pwaf_respond_scratch_bytes(n) bytes of device memory, 16-byte aligned, the call's own until the launches
 *                    have run. The inputs are trusted as pwaf_evaluate_device trusts its batch (an action or status above 3 is not
 *                    refused). Only requests whose action is BYPASS and whose path has at least 24 bytes (the shortest literal) have their
 *                    path read: two 16-byte loads at the path's own alignment; they may pass the path's end by fewer than 16 bytes
 *                    (PWAF_ARENA_PAD) and never begin before it.
 *   PWAF_MEM_HOST    synchronous, plain C++, no HIP call; reads no byte outside a path; scratch and stream are ignored. An action or a
 *                    cookie status above 3, or path offsets that decrease, refuse the call with PWAF_E_BATCH (naming the request)
 *                    before anything is written.
 * PWAF_E_INVALID_ARG, before anything runs: NULL in, verdicts or out; a bad struct_size or memory; with n > 0 a NULL path column;
 * n_lists > PWAF_RESP_MAX_LISTS; lists == NULL with n_lists != 0; a list with idx == NULL and cap != 0, or with n == NULL; a mask with a
 * bit at or above PWAF_RESP_KINDS; in DEVICE mode scratch NULL, not 16-byte aligned or smaller than pwaf_respond_scratch_bytes(n).
 * pwaf_respond_one: the same decision for one request on the host (no GPU): what a per-request closure calls behind
 * pwaf_verify_cookie_one and pwaf_evaluate_one_route. has_route == 0 stands for route == NULL. PWAF_E_INVALID_ARG for a NULL verdict or
 * out, or a NULL path with path_len != 0; PWAF_E_BATCH for an action or status above 3. */
#define PWAF_RESP_FORWARD 0u           /* a service handles it (:266-270); arg = route, or PWAF_ROUTE_NONE when no route column was given */
#define PWAF_RESP_NOT_FOUND 1u         /* a route column was given and no route matches (:272); arg = PWAF_ROUTE_NONE */
#define PWAF_RESP_BLOCKED 2u           /* new_blocked_response (:197, :255); arg = rule_idx (PWAF_RULE_UA_GATE for gate A) */
#define PWAF_RESP_CAPTCHA_PAGE 3u      /* serve_captcha (:234, :258); arg = rule_idx, or PWAF_RULE_COOKIE for an invalid cookie */
#define PWAF_RESP_CAPTCHA_ASSET 4u     /* captcha.rs:165 */
#define PWAF_RESP_CAPTCHA_INIT 5u      /* captcha.rs:167 */
#define PWAF_RESP_CAPTCHA_VERIFY 6u    /* captcha.rs:169 */
#define PWAF_RESP_CAPTCHA_NOT_FOUND 7u /* captcha.rs:173 */
#define PWAF_RESP_HOST_DECIDES 8u      /* the cookie is PWAF_COOKIE_UNDECIDED and neither gate A nor B answered; arg = rule_idx of the verdict as evaluated */
#define PWAF_RESP_KINDS 9u
#define PWAF_RESP_MAX_LISTS 4u
#define PWAF_RULE_COOKIE 0xFFFFFFFCu   /* gate C: a present but invalid verified cookie (:233-235) */
typedef struct pwaf_response {
    uint8_t kind; /* PWAF_RESP_* */
    uint8_t pad[3]; /* 0 */
    uint32_t arg;
} pwaf_response; /* 8 bytes */
typedef struct pwaf_resp_list {
    uint32_t kinds; /* bit k set: requests whose kind is k belong to the list */
    uint32_t cap;   /* entries of idx */
    uint32_t *idx;  /* nullable with cap 0: count only */
    uint32_t *n;    /* WRITTEN (not accumulated): how many requests belong, which may exceed cap */
} pwaf_resp_list;
size_t pwaf_respond_scratch_bytes(uint32_t n); /* DEVICE mode scratch for a batch of n; HOST mode needs none */
int pwaf_respond(const pwaf_batch *in, const pwaf_verdict *verdicts, const uint8_t *cookie_status /* nullable */, const uint32_t *route /* nullable */,
                 pwaf_response *out, uint64_t *counts /* PWAF_RESP_KINDS, nullable, WRITTEN */, const pwaf_resp_list *lists, uint32_t n_lists,
                 void *scratch, size_t scratch_bytes, void *stream);
int pwaf_respond_one(const pwaf_verdict *verdict, uint8_t cookie_status, int has_route, uint32_t route, const char *path, uint32_t path_len,
                     pwaf_response *out);
/* TEST HOOK, CPU: [0] requests per tile (and per workgroup of the classify and scatter launches), [1] tiles per step of the base launch,
 * [2] PWAF_RESP_MAX_LISTS, [3] PWAF_RESP_KINDS */
int pwaf_respond_scan_shape(uint32_t out[4]);

/* ---- records in device memory (ABI 4, additive) ----------------------------------------------------------
 * pwaf_evaluate_records for records that already lie in DEVICE memory — what pwaf_export_records wrote, or a replay file copied to the
 * device once: the bytes never visit the host. buf, rec_off, n_rec, out, counts, match_idx and n_matches are device pointers on the
 * engine's device; `stream` is a hipStream_t (NULL = HIP's default stream). buf is 16-byte aligned and carries NO pad: not one byte
 * outside [buf, buf + buf_bytes) is read, whatever the records say. Request i is the record at buf + rec_off[i] (any order; records may
 * be shared or skipped). The records evaluated are m = min(*n_rec, n), or n when n_rec is NULL; the device reads *n_rec, so
 * pwaf_export_stats::n_written of an export enqueued on the same stream is a valid n_rec without a synchronisation in between. out[i]
 * for i >= m is not written.
 * Format and validation are exactly pwaf_evaluate_records's, done on the device: a malformed call returns PWAF_E_BATCH with the same
 * pwaf_last_error() text as the host call gives for the same bytes (the lowest failing index, its offset, the failing check;
 * PWAF_RECORD_NONE in rec_off is a misaligned offset like any other); nothing behind the validation is launched then, and out, counts,
 * match_idx and n_matches are untouched.
 * Synchronisation: the call enqueues the validation and a segmented prefix sum of the lengths (three launches) on `stream` and waits
 * for the stream ONCE, for one small block (the failure key, m, the common has_geoip, every column's bytes), as pwaf_evaluate_device does
 * for a batch with field_bytes == 0. It then enqueues unpack_records_kernel and the ordinary pipeline and returns: out is valid once
 * `stream` has run. counts and n_matches are ACCUMULATED into (zero them first); match_idx needs room for m entries. Overflow-pool
 * exhaustion is reported by pwaf_engine_device_status, as for pwaf_evaluate_device. m == 0 launches nothing further and returns
 * PWAF_OK. Re-entrant like pwaf_evaluate_device: the unpacked columns and offsets live in the engine's context, not in caller memory, so
 * buf and rec_off may be released or rewritten once `stream` has run.
 * Out of scope: _geo / _hits / _routes variants of this call, and pwaf_node_*. The HOST pwaf_evaluate_records and the async queue keep
 * their host-side validation. */
int pwaf_evaluate_records_device(pwaf_engine *, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n,
                                 const uint32_t *n_rec /* nullable */, pwaf_verdict *out, pwaf_counts *counts /* nullable */,
                                 uint32_t *match_idx, uint32_t *n_matches /* both or neither */, void *stream);
/* TEST HOOK (CPU, no device): the shape of that call's scan, so that a test places its sizes on the real boundaries: out[0] = records
 * per tile of the check and offsets launches, out[1] = tiles one step of the tile-base launch takes, out[2] = out[3] = 0. */
int pwaf_records_scan_shape(uint32_t out[4]);

/* ---- non-blocking request queue (ABI 4) -------------------------------------------------------------
 * The call shape of an async host (the reference's rule loop runs inside an async hyper closure, http_listener.rs:133-274): submit a
 * request with a tag and go on; collect {tag, verdict, status} completions later. pwaf_async_submit copies the request ONCE, as a record,
 * into page-locked segment memory (lock-free slot reservation; it never waits for the device). A batch closes at max_batch requests, when
 * its oldest request has waited max_delay_us, or on pwaf_async_flush; requests with and without GeoIP go to separate batches. (A batch
 * whose deadline passes while an earlier batch of its GeoIP class still waits for a dispatcher keeps filling until that one is taken.) Two
 * dispatcher threads run pwaf_evaluate_records on closed segments and publish completions, in any order, then signal the eventfd.
 * Consumer pattern (race-free): wait until pwaf_async_fd is readable, read(2) it, then pwaf_async_poll until it returns 0.
 * A batch that fails completes each of its requests with that status and the verdict {ALLOW, PWAF_RULE_NONE}: the host applies its own
 * failure policy. Destroy it before the engine. */
typedef struct pwaf_async pwaf_async;
typedef struct pwaf_completion {
    uint64_t tag;         /* as given to pwaf_async_submit */
    pwaf_verdict verdict; /* {ALLOW, PWAF_RULE_NONE} when status != PWAF_OK */
    int32_t status;       /* PWAF_OK or the failing batch's PWAF_E_* */
    uint32_t reserved;
} pwaf_completion;
/* max_in_flight: requests submitted but not yet handed out by pwaf_async_poll; past it submit answers PWAF_E_BUSY. */
int pwaf_async_create(pwaf_engine *, uint32_t max_batch, uint32_t max_delay_us, uint32_t max_in_flight, pwaf_async **out);
/* PWAF_OK: exactly one completion carrying `tag` will follow. PWAF_E_BUSY: max_in_flight reached or no segment has room; nothing was
 * queued. PWAF_E_INVALID_ARG / PWAF_E_BATCH: the request itself is malformed (pwaf_batcher_evaluate's checks) or larger than a segment. */
int pwaf_async_submit(pwaf_async *, const pwaf_request *req, uint64_t tag);
/* Non-blocking: moves up to cap completions into out and returns how many. Safe from any thread; concurrent pollers get disjoint ones. */
size_t pwaf_async_poll(pwaf_async *, pwaf_completion *out, size_t cap);
/* eventfd (EFD_NONBLOCK | EFD_CLOEXEC) owned by the queue: readable after completions were published. */
int pwaf_async_fd(pwaf_async *);
/* Closes the open batches now (does not wait for them). */
int pwaf_async_flush(pwaf_async *);
int pwaf_async_stats(pwaf_async *, uint64_t *n_batches, uint64_t *n_requests, uint64_t *in_flight);
/* Refuses new submits, evaluates every accepted request, waits for threads still inside submit / poll, frees the queue. Completions
 * nobody polled are dropped. */
void pwaf_async_destroy(pwaf_async *);

/* ---- GeoIP answers (ABI 4, additive; engines created with PWAF_OPT_GEO_ANSWERS) ----------------------
 * The reference looks the client's record up once per request, before the gates (http_listener.rs:143-157), keeps asn / country in the
 * RequestContext that travels with the request (:183-191), builds the rule and routing contexts from it (:207-219, :266-270) and sends
 * it upstream as pingoo-client-country / pingoo-client-asn (services/http_proxy_service.rs:174-189). A host that lets the engine own the
 * GeoIP table gets that record back here, next to the verdict: geo[i] is the record the rules of request i saw as client.asn /
 * client.country. A batch, record or request that carries asn / country gets them echoed; otherwise it is the longest-prefix record
 * of the engine's table (later duplicates win), and the default {0, "XX"} for a miss, a loopback or multicast address (geoip.rs:73-91;
 * even below a covering prefix), a record whose country is not two letters A-Z, an engine without a table and an address family the
 * table has no prefix of. ip_is_v6 alone decides the family. Gate verdicts (UA gate, captcha endpoint) get their record too.
 * With `geo` == NULL the _geo functions are exactly the plain ones: no extra launch, no extra copy. `geo` lives where the verdicts
 * live. Out of scope: the blocking pwaf_batcher_* and pwaf_node_* (a node's engines are reachable through pwaf_node_engine). */
typedef struct pwaf_geo {
    uint32_t asn;
    uint8_t country[2];
    uint16_t reserved; /* 0 */
} pwaf_geo; /* 8 bytes == csrc/program.h: GeoRec */

/* GeoipDB::lookup for n addresses and nothing else (georec_kernel alone). `memory` says where ip, ip_is_v6 and out live. HOST: staged,
 * looked up, copied back, waited for (`stream` is ignored). DEVICE: enqueued on `stream` (hipStream_t; NULL = HIP's default); returns at once. */
int pwaf_geoip_lookup(pwaf_engine *, const uint8_t *ip /* n x 16 */, const uint8_t *ip_is_v6 /* n */, uint32_t n, uint32_t memory,
                      pwaf_geo *out /* n */, void *stream);
/* The plain entry points with one more output: pwaf_evaluate_batch / _device / _records / _one. The record kernel runs on the context's
 * side stream beside the address lookups; an overflow-pool retry runs it again. */
int pwaf_evaluate_batch_geo(pwaf_engine *, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, pwaf_geo *geo);
int pwaf_evaluate_device_geo(pwaf_engine *, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, uint32_t *match_idx,
                             uint32_t *n_matches, pwaf_geo *geo, void *stream);
int pwaf_evaluate_records_geo(pwaf_engine *, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n, pwaf_verdict *out,
                              pwaf_counts *counts, pwaf_geo *geo);
int pwaf_evaluate_one_geo(pwaf_engine *, const pwaf_request *req, pwaf_verdict *out, pwaf_geo *geo);
/* A non-blocking queue whose completions carry the record: pwaf_async_poll_geo fills geo[k] beside out[k] (geo may be NULL). A failed
 * batch completes with {0, "XX"}. pwaf_async_poll on such a queue hands out the completions and drops the records; pwaf_async_poll_geo
 * on a queue made by pwaf_async_create returns 0, consumes nothing and sets pwaf_last_error. */
int pwaf_async_create_geo(pwaf_engine *, uint32_t max_batch, uint32_t max_delay_us, uint32_t max_in_flight, pwaf_async **out);
size_t pwaf_async_poll_geo(pwaf_async *, pwaf_completion *out, pwaf_geo *geo /* cap entries, parallel to out */, size_t cap);
/* TEST HOOK (needs an engine; reads host-side fields only), like pwaf_engine_address_tables for the record tables: out[0] = 1 when an
 * IPv4 record table exists, out[1] = /24s that escape to the trie (a prefix longer than /24), out[2] = entries of the run table,
 * out[3] = 1 when a summary bitmap stands in front, out[4] = its granularity, out[5] = the table entry a clear summary bit stands for,
 * out[6] = records, out[7] = 0. */
int pwaf_engine_geo_answer_tables(const pwaf_engine *, uint32_t out[8]);

/* ---- rule hits (ABI 4, additive; engines created with PWAF_OPT_RULE_HITS) ---------------------------
 * Every rule that matches a request, as a sparse list: one entry per (rule, group of 64 requests) with a non-zero match word. Bit r of
 * `mask` is set when the request 64 * group + r is not answered by a gate (PWAF_RULE_UA_GATE, PWAF_RULE_CAPTCHA_ENDPOINT: the reference
 * evaluates no rule for those, http_listener.rs:196-204) and the rule's expression evaluates to Bool(true) or the rule has none —
 * whatever the rule's actions, PWAF_FLAG_CAPTCHA_VERIFIED and the other rules say. An execution error and a rule refused under
 * PWAF_OPT_LENIENT are no match. A (rule, group) pair appears at most once; the order of the entries is unspecified (like match_idx).
 * The list comes out of the verdict kernel: no launch and no pass over the requests is added.
 *   hits, n_hits   given together or both NULL. *n_hits receives the number of entries the batch produced whatever hits_cap is (below
 *                  2^32: groups x rules); only the first hits_cap reserved slots are written, nothing at or beyond hits + hits_cap.
 *                  *n_hits > hits_cap: the list is incomplete — no error, the verdicts are complete: call again with a larger list.
 *                  hits_cap == 0 is a count-only query.
 *   rule_hits      (nullable) n_rules counters: the requests of this call that rule k matches, exact even when the list overflowed.
 * They live where the verdicts live. pwaf_evaluate_batch_hits OVERWRITES n_hits and rule_hits (as it does counts; a batch run again for
 * its overflow pool is not counted twice); pwaf_evaluate_device_hits ACCUMULATES into them (the caller zeroes, as for counts and
 * n_matches). With hits, n_hits and rule_hits all NULL each function is exactly its plain counterpart: same launches, same copies. On an
 * engine without the flag a non-NULL hits or rule_hits returns PWAF_E_UNSUPPORTED and launches nothing.
 * Out of scope: pwaf_evaluate_records, pwaf_evaluate_one, pwaf_batcher_*, pwaf_async_*, pwaf_node_* and the _geo variants. */
typedef struct pwaf_rule_hit {
    uint32_t rule_idx; /* caller's rule index, < n_rules; the gate pseudo rules never appear */
    uint32_t group;    /* requests 64*group .. 64*group+63 */
    uint64_t mask;     /* bit r: the rule matches request 64*group + r; never 0 */
} pwaf_rule_hit;       /* 16 bytes */
int pwaf_evaluate_batch_hits(pwaf_engine *, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, pwaf_rule_hit *hits,
                             uint32_t hits_cap, uint32_t *n_hits, uint64_t *rule_hits /* n_rules, nullable */);
int pwaf_evaluate_device_hits(pwaf_engine *, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, uint32_t *match_idx,
                              uint32_t *n_matches, pwaf_rule_hit *hits, uint32_t hits_cap, uint32_t *n_hits, uint64_t *rule_hits,
                              void *stream);

/* ---- routes (ABI 4, additive; engines created with pwaf_engine_create_routed) -------------------------
 * After its rule loop the reference hands a request to the first service whose `route:` expression is true or that has none
 * (http_listener.rs:266-270, services/http_proxy_service.rs:84-95). A route is written in the rules' language over the rules' context; an
 * execution error and a result that is not a Bool are no match. An engine may be created with an ORDERED list of routes beside its rules;
 * they are compiled with the rules (shared predicates are evaluated once, a route's host or path literal joins the scan pass the rules'
 * patterns over that field already run) and answered by the verdict kernel: no launch and no pass over the requests is added.
 *   route[i] = the index of the first route whose expression is Bool(true) for request i (expression NULL: every request), or
 *              PWAF_ROUTE_NONE when there is none (the reference answers 404 then).
 * route[i] is answered for EVERY request, whatever its verdict: gates A and B, Block / Captcha actions, PWAF_FLAG_CAPTCHA_VERIFIED and the
 * PWAF_OPT_NO_*_GATE flags do not enter it. The reference routes only what it lets through, so the host reads route[i] when out[i].action
 * lets the request through (PWAF_ACTION_ALLOW) and ignores it otherwise.
 * Creation: header names (http_request.headers["x"]) are collected over the rules and then the routes, before anything is compiled. In
 * pwaf_compile_error.rule_index, pwaf_program_rule_status and pwaf_engine_rule_errors route k stands at index n_rules + k (the routes'
 * entries follow the rules'; a message about a route begins "route #k"). A route neither compiler can take fails creation
 * (PWAF_E_UNSUPPORTED); under PWAF_OPT_LENIENT it never matches and creation returns PWAF_W_PARTIAL. A route outside the column compiler's
 * subset runs as a residual program like any rule. Rules plus routes share the limit of 65519 device rules. Routes beside
 * PWAF_OPT_SPARSE_VERDICT / PWAF_OPT_DENSE_VERDICT are refused (PWAF_E_INVALID_ARG): only the entry-list verdict kernel answers them.
 * With n_routes == 0 the two functions ARE pwaf_program_compile / pwaf_engine_create: same program, same dump, same engine.
 * Evaluation: `route` (n entries) lives where `out` lives. route == NULL: each function is exactly its plain counterpart — same launches,
 * same copies — and so are the plain entry points on an engine with routes. A non-NULL route on an engine created without routes returns
 * PWAF_E_UNSUPPORTED and launches nothing. A batch the synchronous entry points run again for its overflow pool answers its routes again.
 * Out of scope: pwaf_evaluate_records, pwaf_batcher_*, pwaf_async_*, pwaf_node_* and the _geo / _hits variants (an engine may have routes
 * and those flags together: one call answers one of the reports). */
#define PWAF_ROUTE_NONE 0xFFFFFFFFu
typedef struct pwaf_route_desc {
    const char *name;       /* NUL-terminated, for diagnostics (nullable) */
    const char *expression; /* NUL-terminated; NULL = matches every request */
    uint64_t reserved;      /* 0 */
} pwaf_route_desc;          /* 24 bytes */
int pwaf_program_compile_routed(const pwaf_rule_desc *rules, size_t n_rules, const pwaf_route_desc *routes, size_t n_routes,
                                const pwaf_list_desc *lists, size_t n_lists, const pwaf_geoip_table *geoip, const pwaf_options *opts,
                                pwaf_program **out, pwaf_compile_error *err);
int pwaf_engine_create_routed(const pwaf_rule_desc *rules, size_t n_rules, const pwaf_route_desc *routes, size_t n_routes,
                              const pwaf_list_desc *lists, size_t n_lists, const pwaf_geoip_table *geoip, const pwaf_options *opts,
                              pwaf_engine **out, pwaf_compile_error *err);
uint32_t pwaf_engine_route_count(const pwaf_engine *);   /* the routes the engine was created with (0: none; also for NULL) */
uint32_t pwaf_program_route_count(const pwaf_program *);
int pwaf_evaluate_batch_routes(pwaf_engine *, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, uint32_t *route /* n, nullable */);
int pwaf_evaluate_device_routes(pwaf_engine *, const pwaf_batch *in, pwaf_verdict *out, pwaf_counts *counts, uint32_t *match_idx,
                                uint32_t *n_matches, uint32_t *route /* n, device memory, nullable */, void *stream);
int pwaf_evaluate_one_route(pwaf_engine *, const pwaf_request *req, pwaf_verdict *out, uint32_t *route /* nullable */);

/* ---- measurement ------------------------------------------------------------------------- */
typedef struct pwaf_kernel_time {
    char name[48];
    float ms;            /* HIP-event duration of the last profiled evaluate call */
    uint64_t alg_bytes;  /* algorithmic bytes this launch is credited with */
} pwaf_kernel_time;
/* on = 1: every evaluate call brackets each kernel with hipEvents on the launch stream; on = 2: only the launches that STREAM the request
 * bytes (filter_kernel, scan_kernel: what the HBM roofline is quoted on) — an event between two kernels keeps the second from starting
 * while the first drains, ~20 us per batch of a dozen launches. Calling it (any value) starts a new measurement window. */
int pwaf_engine_set_profiling(pwaf_engine *, int on);
/* Blocks until the last profiled launch finished; fills up to cap entries, one per kernel launch since the window
 * started (in launch order); returns the count. */
int pwaf_engine_kernel_times(pwaf_engine *, pwaf_kernel_time *out, int cap);

typedef struct pwaf_stats {
    uint32_t n_rules, n_atoms, n_scan_atoms, n_numeric_atoms;
    uint32_t n_dfa_groups, n_dfa_states_total, max_dfa_states, dfa_table_bytes_total;
    uint32_t n_ip_lists, ipset_trie_nodes, geo_trie_nodes, n_dnf_literals;
    uint32_t n_warnings, n_filtered_groups /* passes behind a bigram prefilter */,
        n_gated_groups /* gap passes visited only by requests whose prefix factor was found */,
        n_confirm_literals /* string predicates decided by the confirm tier of their pass's prefilter, without a DFA */;
} pwaf_stats;
int pwaf_engine_stats(const pwaf_engine *, pwaf_stats *out);
/* Execution-error visibility (the reference logs every rule whose execution errs and treats it as "no match": pingoo/rules.rs:41-45).
 * Here an error is a no-match too; errors the compiler can see — unknown names, type errors, invalid patterns: nearly all of them,
 * the context's schema being fixed — are reported ONCE at creation (pwaf_program_warning: "can never match"). What remains are
 * run-time errors of rules on the per-request interpreter (checked arithmetic: overflow, division by zero; an index computed from a
 * request value): counted on the device. counts[i] = requests, over every batch this engine has evaluated, for which caller rule i
 * ended in an execution error. Waits for the device. (An engine with routes: n_rules + n_routes counters may be asked for, the routes'
 * following the rules'; asking for n_rules gives the rules' alone.) */
int pwaf_engine_rule_errors(pwaf_engine *, uint64_t *counts, size_t n_rules);
/* How the engine evaluates the rules outside the column compiler's subset (the reference: Program::execute on every request,
 * pingoo/rules.rs:37-51): 0 = the rule set has none, 1 = interpreted per request on the device (residual_kernel),
 * 2 = SPECIALIZED — the rules' stack programs translated to straight-line device code and compiled for this device by hiprtc at
 * creation (csrc/residual_jit.cpp, rtc.cpp). When 1 was not asked for (PWAF_OPT_NO_RESIDUAL_JIT), pwaf_engine_residual_fallback
 * says why ("" otherwise; the string lives as long as the engine): no libhiprtc.so on the host, a compile error, too many rules. */
int pwaf_engine_residual_mode(const pwaf_engine *);
const char *pwaf_engine_residual_fallback(const pwaf_engine *);
/* Inspection / test hooks of the specialized form (CPU, no device). _source: kind 0 = the rule functions alone (portable C++ over
 * csrc/residual.h: the CPU suite compiles them with g++ and fuzzes them against the oracle), kind 1 = the whole device program as
 * handed to hiprtc. Returns the text's length (0: the program has no residual rules, or they cannot be specialized); copies at most
 * cap - 1 bytes + NUL. _compile: runs hiprtc for `arch` ("gfx950"); returns the code object's size, or a negative PWAF_E_* with the
 * compiler's log in err. */
size_t pwaf_program_residual_source(const pwaf_program *, int kind, char *buf, size_t cap);
long pwaf_program_residual_compile(const pwaf_program *, const char *arch, char *err, size_t err_len);
/* TEST HOOK (CPU, no device): the bigram prefilter + confirm tier of scan pass `group` over ONE field value placed `arena_offset`
 * bytes into an arena, as the device evaluates it (csrc/confirm.h is the code both run). Writes the local atom ids of the literal
 * predicates confirmed (at most cap; possibly repeated), *n_atoms, *flagged (the filter flagged the field) and *walk (a factor of a
 * non-literal predicate was confirmed: the request is walked through the pass's R-tier DFA). PWAF_E_INVALID_ARG when the pass has
 * no prefilter. The reference has no counterpart: it evaluates every predicate on every request (pingoo/rules.rs:37-51). */
int pwaf_program_confirm_field(const pwaf_program *, uint32_t group, const uint8_t *bytes, size_t len, uint32_t arena_offset,
                               uint16_t *atoms, size_t cap, size_t *n_atoms, int *flagged, int *walk);
/* TEST HOOK (CPU, no device): the shape of the confirm tier of scan pass `group`, so that a test can assert that the path it was
 * written for exists. out[0] = entries, out[1] = bytes of the value / mask / class-position pool, out[2] = class words (8 per byte
 * class), out[3] = 1 when entries * 3 + bytes / 4 + class words fit the LDS pool of confirm_kernel (the kernel's own test: the
 * comparison tables are then read from on-chip memory, otherwise from global memory), out[4] = the longest factor in bytes, out[5] =
 * the highest class position of any entry (0 without classes), out[6] = the largest entry count of one bin, out[7] = 1 when the
 * table has a walk entry (a factor of a non-literal predicate). PWAF_E_INVALID_ARG when the pass has no confirm tier. The reference
 * has no counterpart. */
int pwaf_program_confirm_shape(const pwaf_program *, uint32_t group, uint32_t out[8]);
/* TEST HOOK (CPU, no device): the flat table of scan pass `group` for the list-driven walks (lscan_kernel), exactly as an engine created
 * from this program uploads it — after pwaf_program_tune (pwaf_engine_tune, for pwaf_engine_program's handle) the table rebuilt for the
 * sample, whose states are renumbered by visits. tier 0 = the table of the pass's every atom, 1 = of its non-literal atoms (the R tier:
 * what the candidates of a confirm tier walk). The image is the dump's magic and sections of pwaf_program_dump's format, count = group:
 * "FSHP" u32 {n_states, n_classes, scalar_mode, ill_class, n_full, n_delta, LDS bytes the layout was built for}, "FFLT" u16 cells
 * (n_states rows of n_classes + 3: transitions, then the EMIT, STAY and END cell), "FDLT" u64 delta records (states n_full ..: base row
 * | class 1 << 16 | class 2 << 24 | cell 1 << 32 | cell 2 << 48), "FCLS" the class image, "FEMO" / "FEML" and "FENO" / "FENL" the emit
 * and end lists by state. Returns the image's size and copies at most cap bytes; 0 (and pwaf_last_error) for a bad argument or a pass
 * without that tier. The reference has no counterpart. */
size_t pwaf_program_flat_image(const pwaf_program *, uint32_t group, uint32_t tier, uint8_t *buf, size_t cap);
/* TEST HOOK (CPU, no device): the list-scan descriptors of every batch of an engine created from this program (with the program's
 * flags), in launch order, planned by the functions the engine plans its launches with (csrc/scanplan.h: plan_list_scans) over the
 * tables built as the engine builds them; profiling-build switches and the state of an engine are not consulted, and the answer is
 * built on the first call and kept in the program: like pwaf_program_dump, neither hook may run beside another call on the same
 * program (or, for pwaf_engine_program's handle, beside pwaf_engine_tune). PWAF_LIST_SCAN_WORDS words per descriptor: [0]
 * phase (0: the passes behind a prefilter and the identity passes, 1: the gap passes), [1] pass, [2] tier walked (0 full, 1 R), [3]
 * threads and [4] LDS bytes for hot rows of the launch's workgroups, [5] n_hot rows and [6] n_delta records staged, [7] behind_filter,
 * [8] merge_rec, [9] dense_mode, [10] the pass whose list it shares through need masks (0xFFFFFFFF: its own list) and [11] its need
 * bit, [12] the launch's index within the phase and [13] its descriptor count (the k of its `lscan_x<k>` timing entry), [14]
 * workgroups per CU, [15] 0. Writes at most cap descriptors; *n_descs = how many there are. The reference has no counterpart. */
#define PWAF_LIST_SCAN_WORDS 16
int pwaf_program_list_scans(const pwaf_program *, uint32_t *out, size_t cap, size_t *n_descs);
/* TEST HOOK (CPU, no device): the launch shape of the verdict kernel in every batch of an engine created from this program (with the
 * program's flags), computed by the function the engine computes it with (csrc/verdictplan.h: verdict_shape) over the tables planned as
 * the engine plans them and the pass count its batches hand to the kernel. out[0] = the mode (3 entry list, 4 entry list with 8 slots:
 * PWAF_OPT_TINY_VERDICT_SLOTS; 0 dense, 1 sparse column file, 2 sparse with 8 value slots), out[1] = the capacity per wave (entries of
 * the entry list, entry 0 = TRUE included — at most 254: a slot byte is 1 + entry index and 255 means spilled; value slots of the
 * sparse file; 0 for the dense one), out[2] = waves per workgroup (0: pwaf_engine_create refuses the program), out[3] = workgroups per
 * CU of the persistent grid, out[4] = 1 when the program tables are staged in LDS, out[5] = LDS bytes per workgroup, out[6] = the
 * pass count the shape was computed for (scan passes + the pseudo passes of field-against-field atoms and residual rules), out[7] =
 * the bitmap registers of the kernel instantiation that pass count selects (1: up to 64 passes, else 4). Profiling-build switches
 * are not consulted. The reference has no counterpart. */
int pwaf_program_verdict_shape(const pwaf_program *, uint32_t out[8]);
/* TEST HOOK (needs an engine; reads a host-side field): the compute units the engine sizes its persistent grids with (the list scan's
 * waves = this x workgroups per CU x threads / 64); 0 for NULL. */
uint32_t pwaf_engine_compute_units(const pwaf_engine *);
/* TEST HOOK (needs an engine, i.e. a device; reads host-side fields only): what the IPv4 lookup structures of this engine look like,
 * so that a test can assert that the path it was written for exists. out[0] = escaped /24s of the DIR-24 table (a prefix longer
 * than /24, or a class >= 65536 / membership set >= 32768), out[1] = entries of the run table behind the 16-byte records (0: the
 * engine has no DIR-24 table), out[2] = 1 when a summary bitmap stands in front of the table, out[3] = its granularity (one bit per
 * 2^out[3] /24s), out[4] = the table entry a clear summary bit stands for, out[5] = 1 when (class, set) travel packed in one word,
 * out[6] = GeoIP classes, out[7] = membership sets. The reference has no counterpart (pingoo/geoip.rs, lists.rs scan per request). */
int pwaf_engine_address_tables(const pwaf_engine *, uint32_t out[8]);
/* TEST HOOK (needs an engine; reads host-side fields only): the coarse bitmap that the address lookups read from on-chip memory
 * before the summary bitmap (one bit per 2^shift /24s, set = some /24 of the block differs from the common entry). out[0] = 1 when
 * the level is present, out[1] = its shift, out[2] = its size in bytes, out[3] = blocks set, out[4] = blocks set in the summary
 * bitmap (0 without one), out[5], out[6] = threads per workgroup and workgroups per CU of the lookup kernel's launch; out[8..11] =
 * present / shift / bytes / blocks set for the record table of a PWAF_OPT_GEO_ANSWERS engine (all 0: that table has no such level);
 * the rest 0. The reference has no counterpart. */
int pwaf_engine_coarse_tables(const pwaf_engine *, uint32_t out[16]);
/* TEST HOOK (needs an engine and a batch it has evaluated; read-only): what filter_kernel left for scan pass `group` in the scratch
 * context that served the engine's most recent batch — one of pwaf_evaluate_batch* or of pwaf_evaluate_device* on the default stream
 * (batches on other streams are not looked at). Waits for that batch, then copies from the buffers the kernels wrote; nothing is
 * launched. info[0] = slab0, the first 128 KiB slab of the arena the pass streamed (not 0: a slab view), info[1] = the slabs it
 * streamed (0: the arena had none — every field empty, or the batch never reached the prefilter), info[2] = the pass's sampling
 * stride, info[3] = 1 when the pass has a pair list (a confirm tier), info[4] = the pair list's length as filter_kernel left it (the
 * sum of the slabs' counts; 0 without a list), info[5] = PWAF_FILTER_SLAB_ROWS, info[6..7] = 0. With info[1] = S: rows = S *
 * PWAF_FILTER_SLAB_ROWS words, the pass's chunk bitmap as it lies in memory — word r of slab s: bit l = the 16-byte chunk at arena
 * byte (slab0 + s) * 131072 + 1024 r + 16 l holds a position that completed a window; EVERY word of every streamed slab, those of the
 * iterations the arena's last slab does not have included; per_slab[s] = the slab's flagged chunks as counted by its wave; pair_base[s]
 * = where the slab's pairs begin in the pair list (written as 0 for a pass without one). Each of the three arrays may be NULL (not
 * wanted); cap_rows / cap_slabs = the room of rows / of per_slab and pair_base each, PWAF_E_INVALID_ARG when it does not suffice — call
 * once with the arrays NULL for info[1]. Also PWAF_E_INVALID_ARG: a pass without a prefilter, an engine that has evaluated nothing,
 * and an engine whose latest host batch and latest default-stream device batch lie in two contexts (which came last is not recorded:
 * the hook keeps a copy of the batch's filter descriptors per context and puts nothing else on the batch path). Not to be called
 * beside another call on the same engine. The reference has no counterpart. */
#define PWAF_FILTER_SLAB_ROWS 128
int pwaf_engine_filter_flags(pwaf_engine *, uint32_t group, uint32_t info[8], uint64_t *rows, size_t cap_rows, uint32_t *per_slab, uint32_t *pair_base, size_t cap_slabs);
int pwaf_program_stats(const pwaf_program *, pwaf_stats *out);

/* ---- host-side field derivation (what the reference does before building RequestData) ------ */
/* get_path: uri.path().trim_end_matches('/') (http_utils.rs:114-116). Returns the kept length. */
size_t pwaf_derive_path(const uint8_t *uri_path, size_t len);
/* User-Agent (http_listener.rs:159-165): header bytes -> to_str() (fails -> "" unless every byte is
 * visible ASCII 0x20..0x7E or TAB) -> trim -> heapless::String<256> (len > 256 -> ""). Writes the
 * start offset and length of the kept slice. `present` = 0 when the header is absent. */
void pwaf_derive_user_agent(const uint8_t *hdr, size_t len, int present, size_t *out_start, size_t *out_len);
/* get_host (http_listener.rs:284-296): uri.host() if any (trim), else Host header to_str() (trim);
 * longer than 256 -> "". Same output convention. */
void pwaf_derive_host(const uint8_t *uri_host, size_t uri_host_len, int uri_host_present,
                      const uint8_t *host_hdr, size_t host_hdr_len, int host_hdr_present,
                      int *out_from_header, size_t *out_start, size_t *out_len);

/* Thread-local message of the last failing call on this thread. Never NULL. */
const char *pwaf_last_error(void);
uint32_t pwaf_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PWAF_H */
