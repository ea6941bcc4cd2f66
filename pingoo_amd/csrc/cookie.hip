// cookie.hip — cookie_locate_kernel and cookie_verify_kernel with their entry points pwaf_keyset_create / _destroy, pwaf_verify_cookies and
// pwaf_verify_cookie_one (include/pwaf.h): gate C of the reference, "does this request carry a valid __pingoo_captcha_verified cookie"
// (http_listener.rs:169-181, :222-236; pingoo/captcha.rs:125-156; jwt/jwt.rs:198-327), for the requests of a batch. csrc/cookie.h holds
// the computation; DESIGN.md §5.1.6 the semantics and the figures.
//
// Two launches, because most requests of a real batch carry no such cookie and the second kernel is three orders of magnitude heavier per
// request than the first:
//   cookie_locate_kernel  one request per lane, one-wave workgroups in a grid-stride loop over blocks of 64 entries. A lane scans its cookie
//                         value in 16-byte loads, splits the token and checks the signature part's base64. Where that decides (no cookie:
//                         ABSENT; not three parts, not 64 bytes of signature: INVALID) it writes the status; otherwise the lane joins
//                         the candidate list: ballot, rank by the lanes below, ONE atomicAdd per wave on the count (zeroed by the
//                         memset in front of the launch) — the idiom of the verdict kernel's match list and pack_records_kernel.
//   cookie_verify_kernel  one candidate per lane, full waves whatever the batch looked like; the count is read on the device, so the host
//                         does not sit in between. A lane parses the header, hashes R || A || message (SHA-512), reduces mod L, runs the
//                         double-scalar multiplication [S]B + [k](-A) over two 16-entry tables, encodes, compares with R, then reads the
//                         claims and computes the request's client id (clientid.h). The multiples of B are staged in LDS once per
//                         workgroup; the per-key multiples of -A stay in global memory (read-only, L2-resident: 1920 bytes per key).
// The list's order is whatever the atomics made it; a candidate carries its entry, so status[j] belongs to entry j.
#include <hip/hip_runtime.h>

#include <new>
#include <string>

#include "cookie.h"

namespace pwaf {
namespace cookie {
namespace {

__global__ __launch_bounds__(64) void cookie_locate_kernel(Args a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t m = selected(a);
    for (uint64_t e0 = blockIdx.x * 64ull; e0 < m; e0 += gridDim.x * 64ull) {
        const uint64_t e = e0 + lane;
        const bool live = e < m;
        Candidate c{0, 0, 0, 0};
        uint8_t st = PWAF_COOKIE_ABSENT;
        if (live) st = locate_entry(a, (uint32_t)e, &c);
        const bool cand = live && st == kCandidate;
        const uint64_t mask = __ballot(cand);
        uint32_t base = 0;
        if (lane == 0 && mask) base = atomicAdd(a.count, (uint32_t)__popcll(mask));
        base = __shfl(base, 0, 64);
        if (cand)
            a.cand[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = c;  // (base + rank < m: every candidate is a live entry)
        else if (live)
            a.status[e] = st;
        if (live && !a.idx && a.flags_out) a.flags_out[e] = flag_of(a, (uint32_t)e, PWAF_COOKIE_ABSENT);  // cookie_verify_kernel sets the bit
    }
}

__global__ __launch_bounds__(64) void cookie_verify_kernel(Args a) {
    __shared__ Precomp base[16];
    const uint32_t lane = threadIdx.x;
    const uint32_t cap = a.idx ? a.idx_cap : a.n;
    uint32_t count = *a.count;
    if (count > cap) count = cap;  // (it cannot be: the list has cap entries)
    if (blockIdx.x * 64ull >= count) return;
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.ks->base);
        uint32_t *dst = reinterpret_cast<uint32_t *>(base);
        for (uint32_t k = lane; k < sizeof(base) / 4; k += 64) dst[k] = src[k];
    }
    __syncthreads();
    for (uint64_t j0 = blockIdx.x * 64ull; j0 < count; j0 += gridDim.x * 64ull) {
        const uint64_t j = j0 + lane;
        if (j >= count) continue;
        const Candidate c = a.cand[j];
        const uint8_t st = judge_candidate(a, base, c);
        a.status[c.entry] = st;
        if (st == PWAF_COOKIE_VERIFIED && !a.idx && a.flags_out) a.flags_out[c.entry] |= PWAF_FLAG_CAPTCHA_VERIFIED;  // (the locate kernel wrote the rest)
    }
}

}  // namespace

int launch_verify_cookies(const Args &a, void *stream) {
    const uint32_t cap = a.idx ? a.idx_cap : a.n;
    if (cap == 0) return 0;
    if (hipMemsetAsync(a.count, 0, 16, (hipStream_t)stream) != hipSuccess) return -1;
    const uint32_t groups = (uint32_t)(((uint64_t)cap + 63u) / 64u);
    const uint32_t blocks = groups < 8192u ? groups : 8192u;
    hipLaunchKernelGGL(cookie_locate_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(cookie_verify_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cookie

}  // namespace pwaf

extern "C" int pwaf_keyset_create(const pwaf_ed25519_key *keys, uint32_t n, int device, pwaf_keyset **out) {
    namespace K = pwaf::cookie;
    using pwaf::fail;
    if (!out) return fail(PWAF_E_INVALID_ARG, "pwaf_keyset_create: NULL out");
    *out = nullptr;
    if (!keys || n == 0 || n > PWAF_KEYSET_MAX_KEYS) return fail(PWAF_E_INVALID_ARG, "pwaf_keyset_create: 1.." + std::to_string(PWAF_KEYSET_MAX_KEYS) + " keys");
    pwaf_keyset *ks = new (std::nothrow) pwaf_keyset();
    if (!ks) return fail(PWAF_E_NOMEM, "pwaf_keyset_create: out of memory");
    ks->dev = nullptr, ks->device = device;
    memset(&ks->data, 0, sizeof ks->data);
    ks->data.n_keys = n;
    int rc = PWAF_OK;
    std::string why;
    if (!K::build_base_table(ks->data.base)) rc = PWAF_E_INVALID_ARG, why = "pwaf_keyset_create: the base point does not decompress";
    for (uint32_t k = 0; k < n && rc == PWAF_OK; k++) {
        const size_t len = keys[k].kid ? strnlen(keys[k].kid, PWAF_KEYSET_MAX_KID + 1) : 0;
        if (len == 0 || len > PWAF_KEYSET_MAX_KID)
            rc = PWAF_E_INVALID_ARG, why = "pwaf_keyset_create: key " + std::to_string(k) + ": the kid is empty or longer than " + std::to_string(PWAF_KEYSET_MAX_KID) + " bytes";
        else if (!K::build_key(keys[k].x, keys[k].kid, (uint32_t)len, &ks->data.keys[k]))
            rc = PWAF_E_INVALID_ARG, why = "pwaf_keyset_create: key " + std::to_string(k) + ": x is not the canonical encoding of a point on the curve";
        for (uint32_t j = 0; j < k && rc == PWAF_OK; j++)
            if (ks->data.keys[j].kid_len == len && memcmp(ks->data.keys[j].kid, keys[k].kid, len) == 0)
                rc = PWAF_E_INVALID_ARG, why = "pwaf_keyset_create: keys " + std::to_string(j) + " and " + std::to_string(k) + " have one kid";
    }
    if (rc == PWAF_OK && device >= 0) {
        int prev = 0;
        bool ok = hipGetDevice(&prev) == hipSuccess && hipSetDevice(device) == hipSuccess;
        ok = ok && hipMalloc((void **)&ks->dev, sizeof ks->data) == hipSuccess;
        ok = ok && hipMemcpy(ks->dev, &ks->data, sizeof ks->data, hipMemcpyHostToDevice) == hipSuccess;
        (void)hipSetDevice(prev);
        if (!ok) {
            (void)hipGetLastError();
            if (ks->dev) (void)hipFree(ks->dev);
            rc = PWAF_E_DEVICE, why = "pwaf_keyset_create: the key tables could not be uploaded to device " + std::to_string(device);
        }
    }
    if (rc != PWAF_OK) {
        delete ks;
        return fail(rc, why);
    }
    *out = ks;
    return PWAF_OK;
}

extern "C" void pwaf_keyset_destroy(pwaf_keyset *ks) {
    if (!ks) return;
    if (ks->dev) (void)hipFree(ks->dev);
    delete ks;
}

extern "C" size_t pwaf_verify_cookies_scratch_bytes(uint32_t n) { return 16 + sizeof(pwaf::cookie::Candidate) * (size_t)n; }

extern "C" int pwaf_verify_cookies(const pwaf_keyset *ks, const pwaf_batch *in, const pwaf_strcol *cookies, int64_t now, const uint32_t *idx, uint32_t idx_cap,
                                   const uint32_t *n_idx, uint8_t *status, uint8_t *flags_out, void *scratch, size_t scratch_bytes, void *stream) {
    namespace K = pwaf::cookie;
    using pwaf::fail;
    if (!ks || !in || !cookies || !status) return fail(PWAF_E_INVALID_ARG, "pwaf_verify_cookies: NULL argument");
    if (int rc = pwaf::check_batch_header(in)) return rc;
    if (int rc = pwaf::check_list("pwaf_verify_cookies", idx, idx_cap, n_idx)) return rc;
    const pwaf_strcol &ua = in->field[PWAF_FIELD_USER_AGENT], &host = in->field[PWAF_FIELD_HOST];
    if (int rc = pwaf::check_client_columns(in)) return rc;
    if (in->n) {
        if (!cookies->data || !cookies->offsets) return fail(PWAF_E_INVALID_ARG, "pwaf_verify_cookies: the cookies column is NULL");
    }
    K::Args a{};
    a.cookies = *cookies, a.ua = ua, a.host = host, a.ip = in->ip, a.ip_is_v6 = in->ip_is_v6, a.flags = in->flags, a.n = in->n, a.now = now;
    a.idx = idx, a.n_idx = n_idx, a.idx_cap = idx_cap, a.status = status, a.flags_out = flags_out;
    if (in->memory == PWAF_MEM_HOST) {
        a.ks = &ks->data;
        uint32_t bad = 0;
        if (!K::verify_host(a, &bad))
            return fail(PWAF_E_BATCH, "pwaf_verify_cookies: entry " + std::to_string(bad) + " (request " + std::to_string(idx ? idx[bad] : bad) + "): offsets decrease");
        return PWAF_OK;
    }
    if (!ks->dev) return fail(PWAF_E_DEVICE, "pwaf_verify_cookies: the key set was created for the host only (device < 0)");
    const uint32_t cap = idx ? idx_cap : in->n;
    if (int rc = pwaf::check_scratch("pwaf_verify_cookies", scratch, scratch_bytes, pwaf_verify_cookies_scratch_bytes(cap), "pwaf_verify_cookies_scratch_bytes")) return rc;
    int current = -1;
    if (hipGetDevice(&current) != hipSuccess || current != ks->device) return fail(PWAF_E_DEVICE, "pwaf_verify_cookies: the current device is not the key set's");
    a.ks = ks->dev;
    a.count = static_cast<uint32_t *>(scratch);
    a.cand = reinterpret_cast<K::Candidate *>(static_cast<uint8_t *>(scratch) + 16);
    if (K::launch_verify_cookies(a, stream)) return fail(PWAF_E_DEVICE, "pwaf_verify_cookies: a launch failed");
    return PWAF_OK;
}

extern "C" int pwaf_verify_cookie_one(const pwaf_keyset *ks, const pwaf_request *req, const char *cookie, uint32_t cookie_len, int64_t now, uint8_t *status) {
    namespace K = pwaf::cookie;
    namespace C = pwaf::clientid;
    if (!ks || !req || !status) return pwaf::fail(PWAF_E_INVALID_ARG, "pwaf_verify_cookie_one: NULL argument");
    if ((req->user_agent_len && !req->user_agent) || (req->host_len && !req->host) || (cookie_len && !cookie))
        return pwaf::fail(PWAF_E_INVALID_ARG, "pwaf_verify_cookie_one: NULL value with a length");
    K::Token t{0, 0, 0};
    const uint8_t *v = reinterpret_cast<const uint8_t *>(cookie);
    uint8_t st = cookie_len ? K::locate(v, cookie_len, &t) : (uint8_t)PWAF_COOKIE_ABSENT;
    if (st == K::kCandidate) {
        uint32_t id[C::kIdWords];
        C::client_id_words(C::make_message(req->ip, req->ip_is_v6, (const uint8_t *)req->user_agent, req->user_agent_len, (const uint8_t *)req->host, req->host_len), id);
        st = K::judge(ks->data, ks->data.base, v, t, now, id);
    }
    *status = st;
    return PWAF_OK;
}
