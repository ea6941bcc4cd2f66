// evaluate_records.cpp — request records (ABI 4; include/pwaf.h: pwaf_evaluate_records*, csrc/records.h): records in host memory are
// validated on the host and unpacked on the device, records in device memory are validated there too (records_scan.hip); either way the
// unpacked columns are an ordinary DEVICE batch for the pipeline (pipeline.cpp). Where the parts of the two blocks go: staging.h.
#include "engine_impl.h"
#include "records.h"

using namespace pwaf;

static_assert(pwaf::records::kMaxValues == PWAF_N_FIELDS + kMaxHeaders, "records.h kMaxValues must follow program.h kMaxHeaders");

namespace pwaf {  // async.cpp: the queue takes its records-with-answers evaluator as a pointer (it links against a stub engine in the CPU suite)
using RecordsGeoFn = int (*)(pwaf_engine *, const uint8_t *, size_t, const uint32_t *, uint32_t, pwaf_verdict *, pwaf_counts *, pwaf_geo *);
int async_create_with(pwaf_engine *engine, uint32_t max_batch, uint32_t max_delay_us, uint32_t max_in_flight, RecordsGeoFn eval_geo, pwaf_async **out);
}  // namespace pwaf

namespace {

// The caller's [p, p + bytes) lies in ONE page-locked allocation (pwaf_host_alloc / pwaf_host_register): the copy engine can read it
// directly. Anything else (pageable memory, a range across two registrations) is staged.
bool page_locked(const void *p, size_t bytes) {
    hipPointerAttribute_t a{}, b{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess || hipPointerGetAttributes(&b, (const char *)p + bytes - 1) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost && b.type == hipMemoryTypeHost && a.devicePointer && b.devicePointer &&
           (const char *)b.devicePointer - (const char *)a.devicePointer == (ptrdiff_t)(bytes - 1);
}

// `geo` (nullable; host memory, n entries; PWAF_OPT_GEO_ANSWERS engines only): the GeoIP record of every request
int evaluate_records_impl(pwaf_engine *e, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n, pwaf_verdict *out, pwaf_counts *counts, pwaf_geo *geo_out) {
    namespace R = pwaf::records;
    if (e->n_fields > R::kMaxValues) return fail(PWAF_E_UNSUPPORTED, "the engine has more columns than a record can carry");
    if (n == 0) {
        if (counts) memset(counts, 0, sizeof *counts);
        return PWAF_OK;
    }
    // the host reads the heads and lengths only: validation (nothing is launched for a malformed call) and the column offsets
    const uint32_t n_cols = e->n_fields;
    std::vector<uint64_t> totals(n_cols);
    uint32_t bad = 0;
    int geo = 0;
    uint64_t lo = 0, hi = 0;
    const int chk = R::validate(buf, buf_bytes, rec_off, n, n_cols, totals.data(), &bad, &geo, &lo, &hi);
    if (chk != R::kOk) return fail(PWAF_E_BATCH, "record " + std::to_string(bad) + " (offset " + std::to_string(rec_off[bad]) + "): " + R::check_message(chk));
    HIP_TRY(hipSetDevice(e->device));
    std::unique_lock<std::mutex> lock;
    bool must_wait;
    Scratch &S = acquire_context(e, true, nullptr, lock, must_wait);
    int rc;
    if ((rc = S.ensure(true))) return rc;
    hipStream_t s = S.stream;
    if (must_wait) HIP_TRY(hipStreamWaitEvent(s, S.done, 0));
    const size_t span = (size_t)(hi - lo);
    const HostRecMeta mt = host_rec_meta(n, n_cols, geo_out != nullptr, span);
    const bool direct = page_locked(buf + lo, span);
    if ((rc = S.rec_meta.reserve(mt.need)) || (rc = S.rec_pin.reserve(direct ? mt.up_bytes : mt.need)) || (rc = S.rec_back.reserve(mt.at_rec - mt.at_counts))) return rc;
    uint8_t *const h = (uint8_t *)S.rec_pin.p;
    uint32_t *const h_recoff = (uint32_t *)(h + mt.at_recoff);
    for (uint32_t i = 0; i < n; i++) h_recoff[i] = (uint32_t)(rec_off[i] - lo);
    R::column_offsets(buf, rec_off, n, n_cols, (uint32_t *)(h + mt.at_off), mt.off_stride);
    const RecordColsPlan cp = plan_record_cols(totals.data(), n_cols, n, geo != 0);
    memcpy(h + mt.at_colat, cp.col_at, (size_t)n_cols * 8);
    if ((rc = S.rec_cols.reserve(cp.size))) return rc;
    memset(h + mt.at_counts, 0, sizeof(pwaf_counts));
    uint8_t *const d = (uint8_t *)S.rec_meta.p;
    uint8_t *const dc = (uint8_t *)S.rec_cols.p;
    HIP_TRY(hipMemcpyAsync(d, h, mt.up_bytes, hipMemcpyHostToDevice, s));
    if (direct) {
        HIP_TRY(hipMemcpyAsync(d + mt.at_rec, buf + lo, span, hipMemcpyHostToDevice, s));
    } else {
        memcpy(h + mt.at_rec, buf + lo, span);
        HIP_TRY(hipMemcpyAsync(d + mt.at_rec, h + mt.at_rec, span, hipMemcpyHostToDevice, s));
    }
    R::UnpackArgs ua{};
    fill_unpack_args(ua, cp, d + mt.at_rec, (const uint32_t *)(d + mt.at_recoff), n, n_cols, dc, (const uint64_t *)(d + mt.at_colat), (const uint32_t *)(d + mt.at_off),
                     (uint32_t)mt.off_stride);
    if (R::launch_unpack_records(ua, s)) {
        (void)hipStreamSynchronize(s);  // (the copies in flight read the caller's buffer)
        return fail(PWAF_E_DEVICE, "unpack_records_kernel launch failed");
    }
    // the device batch the kernel writes: an ordinary DEVICE batch with every column's size known on the host
    DeviceBatch dv(n, n_cols);
    for (uint32_t f = 0; f < n_cols; f++) dv.set_col(f, dc + cp.col_at[f], (const uint32_t *)(d + mt.at_off) + (size_t)f * mt.off_stride, (uint32_t)totals[f]);
    dv.set_fixed(ua.ip, ua.ip_is_v6, ua.port, ua.flags, ua.asn, ua.country);
    const std::vector<uint32_t> col_begin(n_cols, 0);
    pwaf_counts *const d_counts = (pwaf_counts *)(d + mt.at_counts);
    // (the counters arrive zeroed with the staged block; counters + verdicts come back in one copy)
    rc = run_with_retry(e, S, dv.db, (pwaf_verdict *)(d + mt.at_out), d_counts, true, &col_begin, true, [&]() -> int {
        HIP_TRY(hipMemcpyAsync(S.rec_back.p, d_counts, mt.at_rec - mt.at_counts, hipMemcpyDeviceToHost, s));
        return PWAF_OK;
    }, geo_out ? (pwaf_geo *)(d + mt.at_geo) : nullptr);
    if (rc) return rc;
    memcpy(out, (const char *)S.rec_back.p + (mt.at_out - mt.at_counts), (size_t)n * sizeof(pwaf_verdict));
    if (geo_out) memcpy(geo_out, (const char *)S.rec_back.p + (mt.at_geo - mt.at_counts), (size_t)n * sizeof(pwaf_geo));
    if (counts) memcpy(counts, S.rec_back.p, sizeof(pwaf_counts));
    return PWAF_OK;
}

// Records that already lie in DEVICE memory. What the host does above — validate every record, turn the lengths into
// column offsets — runs on the device here (records_scan.hip), on the caller's stream; the host waits for that stream ONCE, for the
// summary block (failure key, m, has_geoip, the column totals), because the arenas it reserves next and the pipeline's launch plan are
// sized from the totals. Everything behind the wait is enqueued and the call returns, like pwaf_evaluate_device.
int evaluate_records_device_impl(pwaf_engine *e, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n, const uint32_t *n_rec, pwaf_verdict *out,
                                 pwaf_counts *counts, uint32_t *match_idx, uint32_t *n_matches, hipStream_t stream) {
    namespace R = pwaf::records;
    if (e->n_fields > R::kMaxValues) return fail(PWAF_E_UNSUPPORTED, "the engine has more columns than a record can carry");
    if ((match_idx == nullptr) != (n_matches == nullptr)) return fail(PWAF_E_INVALID_ARG, "match_idx and n_matches must be given together");
    if ((uintptr_t)buf & 15u) return fail(PWAF_E_INVALID_ARG, "pwaf_evaluate_records_device: buf is not 16-byte aligned");
    if (n == 0) return PWAF_OK;
    HIP_TRY(hipSetDevice(e->device));
    std::unique_lock<std::mutex> lock;
    bool must_wait;
    Scratch &S = acquire_context(e, false, stream, lock, must_wait);
    int rc;
    if ((rc = S.ensure(false))) return rc;
    if (must_wait) HIP_TRY(hipStreamWaitEvent(stream, S.done, 0));
    const uint32_t n_cols = e->n_fields;
    const DeviceRecMeta mt = device_rec_meta(n, n_cols);
    if (mt.off_stride > 0xFFFFFFFFull) return fail(PWAF_E_UNSUPPORTED, "pwaf_evaluate_records_device: too many records for one call");
    if ((rc = S.rec_meta.reserve(mt.size)) || (rc = S.rec_pin.reserve(sizeof(R::ScanSummary)))) return rc;
    uint8_t *const d = (uint8_t *)S.rec_meta.p;
    R::ScanArgs sa{};
    sa.buf = buf, sa.buf_bytes = buf_bytes, sa.rec_off = rec_off, sa.n_rec = n_rec, sa.n = n, sa.n_cols = n_cols;
    sa.off = (uint32_t *)(d + mt.at_off), sa.off_stride = (uint32_t)mt.off_stride;
    sa.tile = (uint64_t *)(d + mt.at_tile), sa.tile_stride = (uint32_t)mt.tile_stride;
    sa.col_at = (uint64_t *)(d + mt.at_colat), sa.sum = (R::ScanSummary *)(d + mt.at_sum);
    const volatile R::ScanSummary *const sum = (const volatile R::ScanSummary *)S.rec_pin.p;
    // From the first launch on, whatever way the call leaves, the context remembers the stream (its next user waits for what was enqueued).
    auto body = [&]() -> int {
        R::UnpackArgs ua{};
        RecordColsPlan cp;
        uint64_t totals[R::kMaxValues];
        uint32_t m = 0;
        {
            KernelTimer prof(e, stream);  // (released before run_pipeline takes its own)
            HIP_TRY(hipMemsetAsync(&sa.sum->key, 0xFF, 8, stream));  // records::kNoFailure
            const uint64_t alg[3] = {(uint64_t)n * (4 + R::kHead + 4ull * n_cols), (uint64_t)mt.tile_stride * 16 * n_cols, (uint64_t)mt.off_stride * 8 * n_cols};
            for (int phase = 1; phase <= 3; phase++) {
                if ((rc = prof.begin())) return rc;
                if (R::launch_scan_records(phase, sa, stream)) return fail(PWAF_E_DEVICE, std::string(R::kScanKernelNames[phase - 1]) + " launch failed");
                if ((rc = prof.end(R::kScanKernelNames[phase - 1], alg[phase - 1]))) return rc;
            }
            // the call's one wait: the summary block
            HIP_TRY(hipMemcpyAsync(S.rec_pin.p, sa.sum, R::summary_bytes(n_cols), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            prof.commit();
            const uint64_t key = sum->key;
            if (key != R::kNoFailure)
                return fail(PWAF_E_BATCH, "record " + std::to_string(R::key_index(key)) + " (offset " + std::to_string(sum->bad_off) + "): " + R::check_message(R::key_check(key)));
            m = sum->m;
            if (m == 0) return PWAF_OK;
            for (uint32_t f = 0; f < n_cols; f++) totals[f] = sum->totals[f];
            cp = plan_record_cols(totals, n_cols, m, sum->has_geoip != 0);  // (the same places phase 3 left in sa.col_at)
            if ((rc = S.rec_cols.reserve(cp.size))) return rc;
            fill_unpack_args(ua, cp, buf, rec_off, m, n_cols, (uint8_t *)S.rec_cols.p, sa.col_at, sa.off, sa.off_stride);
            prof.last_main = -1;  // (the unpack's time begins at its own event, not in front of the wait)
            if ((rc = prof.begin())) return rc;
            if (R::launch_unpack_records(ua, stream)) return fail(PWAF_E_DEVICE, "unpack_records_kernel launch failed");
            uint64_t bytes = 0;
            for (uint32_t f = 0; f < n_cols; f++) bytes += totals[f];
            if ((rc = prof.end("unpack_records_kernel", 2 * bytes + (uint64_t)m * (R::kHead + 4ull * n_cols)))) return rc;
            prof.commit();
        }
        // an ordinary DEVICE batch with every column's size known on the host
        DeviceBatch dv(m, n_cols);
        for (uint32_t f = 0; f < n_cols; f++) dv.set_col(f, ua.arena + cp.col_at[f], sa.off + (size_t)f * mt.off_stride, (uint32_t)totals[f]);
        dv.set_fixed(ua.ip, ua.ip_is_v6, ua.port, ua.flags, ua.asn, ua.country);
        return run_pipeline(e, S, dv.db, out, counts, match_idx, n_matches, stream, true);
    };
    rc = body();
    const hipError_t he = mark_context_used(S, stream, false);
    return rc ? rc : he != hipSuccess ? device_error("hipEventRecord", he) : PWAF_OK;
}

}  // namespace

extern "C" {

int pwaf_evaluate_records(pwaf_engine *e, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n, pwaf_verdict *out, pwaf_counts *counts) {
    if (!e || (n && (!buf || !rec_off || !out))) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    return evaluate_records_impl(e, buf, buf_bytes, rec_off, n, out, counts, nullptr);
}
int pwaf_evaluate_records_geo(pwaf_engine *e, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n, pwaf_verdict *out, pwaf_counts *counts, pwaf_geo *geo) {
    if (!e || (n && (!buf || !rec_off || !out))) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    if (int rc = need_geo_answers(e, "pwaf_evaluate_records_geo")) return rc;
    return evaluate_records_impl(e, buf, buf_bytes, rec_off, n, out, counts, geo);
}
int pwaf_evaluate_records_device(pwaf_engine *e, const uint8_t *buf, size_t buf_bytes, const uint32_t *rec_off, uint32_t n, const uint32_t *n_rec, pwaf_verdict *out,
                                 pwaf_counts *counts, uint32_t *match_idx, uint32_t *n_matches, void *stream) {
    if (!e || (n && (!buf || !rec_off || !out))) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    return evaluate_records_device_impl(e, buf, buf_bytes, rec_off, n, n_rec, out, counts, match_idx, n_matches, (hipStream_t)stream);
}

int pwaf_async_create_geo(pwaf_engine *e, uint32_t max_batch, uint32_t max_delay_us, uint32_t max_in_flight, pwaf_async **out) {
    if (!e || !out) return fail(PWAF_E_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (int rc = need_geo_answers(e, "pwaf_async_create_geo")) return rc;
    return pwaf::async_create_with(e, max_batch, max_delay_us, max_in_flight, &pwaf_evaluate_records_geo, out);
}

}  // extern "C"
