// pow.hip — pow_check_kernel and pow_verify_kernel with their entry points pwaf_verify_pow and pwaf_verify_pow_one (include/pwaf.h): the
// check CaptchaManager::api_verify runs on a proof-of-work submission (pingoo/captcha.rs:241-333; jwt/jwt.rs:198-327), for the requests of
// a batch. csrc/pow.h holds the computation; DESIGN.md §5.1.7 the semantics and the figures.
//
// Two launches, shaped like cookie.hip's, and for a stronger reason: the one input an attacker controls freely is the hash, and a wrong
// hash must never cost the curve arithmetic.
//   pow_check_kernel   one entry per lane, one-wave workgroups in a grid-stride loop over blocks of 64 entries. A lane scans its cookie
//                      value for `__pingoo_captcha`, splits the token, reads the header and the claims (flat subset; \u0000 in the claims'
//                      strings), and runs every check that needs no curve: exp / nbf / aud / iss, the difficulty against the hash's leading
//                      zero nibbles, SHA-256(challenge || nonce) against the hash, sub against the client id computed in place. Where that
//                      decides it writes ABSENT / FAILED; otherwise the lane joins the candidate list — ballot, rank by the lanes below,
//                      ONE atomicAdd per wave on the count (scratch word 0, zeroed by the memset in front of the launch) — with the key
//                      to verify under (or "every key") and the status a good signature yields (PASSED or UNDECIDED).
//   pow_verify_kernel  one candidate per lane, full waves; the count is read on the device. signature_ok over the multiples of B staged
//                      in LDS and the key's multiples of -A in global memory, exactly as cookie_verify_kernel does it.
// The list's order is whatever the atomics made it; a candidate carries its entry, so status[j] belongs to entry j.
#include <hip/hip_runtime.h>

#include <string>

#include "pow.h"

namespace pwaf {
namespace pow {
namespace {

__global__ __launch_bounds__(64) void pow_check_kernel(Args a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t m = selected(a);
    for (uint64_t e0 = blockIdx.x * 64ull; e0 < m; e0 += gridDim.x * 64ull) {
        const uint64_t e = e0 + lane;
        const bool live = e < m;
        Candidate c{0, 0, 0, 0, 0, 0};
        uint8_t st = PWAF_POW_ABSENT;
        if (live) st = check_entry(a, (uint32_t)e, &c);
        const bool cand = live && st == kCandidate;
        const uint64_t mask = __ballot(cand);
        uint32_t base = 0;
        if (lane == 0 && mask) base = atomicAdd(a.count, (uint32_t)__popcll(mask));
        base = __shfl(base, 0, 64);
        if (cand)
            a.cand[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = c;  // (base + rank < m: every candidate is a live entry)
        else if (live)
            a.status[e] = st;
    }
}

__global__ __launch_bounds__(64) void pow_verify_kernel(Args a) {
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
        a.status[c.entry] = verify_candidate(a, base, c);
    }
}

}  // namespace

int launch_verify_pow(const Args &a, void *stream) {
    const uint32_t cap = a.idx ? a.idx_cap : a.n;
    if (cap == 0) return 0;
    if (hipMemsetAsync(a.count, 0, 16, (hipStream_t)stream) != hipSuccess) return -1;
    const uint32_t groups = (uint32_t)(((uint64_t)cap + 63u) / 64u);
    const uint32_t blocks = groups < 8192u ? groups : 8192u;
    hipLaunchKernelGGL(pow_check_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(pow_verify_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace pow

}  // namespace pwaf

extern "C" size_t pwaf_verify_pow_scratch_bytes(uint32_t n) { return 16 + sizeof(pwaf::pow::Candidate) * (size_t)n; }

extern "C" int pwaf_verify_pow(const pwaf_keyset *ks, const pwaf_batch *in, const pwaf_strcol *cookies, const uint8_t *hash, const pwaf_strcol *nonce, int64_t now,
                               const uint32_t *idx, uint32_t idx_cap, const uint32_t *n_idx, uint8_t *status, void *scratch, size_t scratch_bytes, void *stream) {
    namespace K = pwaf::pow;
    using pwaf::fail;
    if (!ks || !in || !cookies || !status || !hash || !nonce) return fail(PWAF_E_INVALID_ARG, "pwaf_verify_pow: NULL argument");
    if (int rc = pwaf::check_batch_header(in)) return rc;
    if (int rc = pwaf::check_list("pwaf_verify_pow", idx, idx_cap, n_idx)) return rc;
    const pwaf_strcol &ua = in->field[PWAF_FIELD_USER_AGENT], &host = in->field[PWAF_FIELD_HOST];
    if (int rc = pwaf::check_client_columns(in)) return rc;
    if (in->n) {
        if (!cookies->data || !cookies->offsets) return fail(PWAF_E_INVALID_ARG, "pwaf_verify_pow: the cookies column is NULL");
        if (!nonce->data || !nonce->offsets) return fail(PWAF_E_INVALID_ARG, "pwaf_verify_pow: the nonce column is NULL");
    }
    K::Args a{};
    a.cookies = *cookies, a.nonce = *nonce, a.ua = ua, a.host = host, a.ip = in->ip, a.ip_is_v6 = in->ip_is_v6, a.hash = hash, a.n = in->n, a.now = now;
    a.idx = idx, a.n_idx = n_idx, a.idx_cap = idx_cap, a.status = status;
    if (in->memory == PWAF_MEM_HOST) {
        a.ks = &ks->data;
        uint32_t bad = 0;
        if (!K::verify_host(a, &bad, nullptr))
            return fail(PWAF_E_BATCH, "pwaf_verify_pow: entry " + std::to_string(bad) + " (request " + std::to_string(idx ? idx[bad] : bad) + "): offsets decrease");
        return PWAF_OK;
    }
    if (!ks->dev) return fail(PWAF_E_DEVICE, "pwaf_verify_pow: the key set was created for the host only (device < 0)");
    const uint32_t cap = idx ? idx_cap : in->n;
    if (int rc = pwaf::check_scratch("pwaf_verify_pow", scratch, scratch_bytes, pwaf_verify_pow_scratch_bytes(cap), "pwaf_verify_pow_scratch_bytes")) return rc;
    int current = -1;
    if (hipGetDevice(&current) != hipSuccess || current != ks->device) return fail(PWAF_E_DEVICE, "pwaf_verify_pow: the current device is not the key set's");
    a.ks = ks->dev;
    a.count = static_cast<uint32_t *>(scratch);
    a.cand = reinterpret_cast<K::Candidate *>(static_cast<uint8_t *>(scratch) + 16);
    if (K::launch_verify_pow(a, stream)) return fail(PWAF_E_DEVICE, "pwaf_verify_pow: a launch failed");
    return PWAF_OK;
}

extern "C" int pwaf_verify_pow_one(const pwaf_keyset *ks, const pwaf_request *req, const char *cookie, uint32_t cookie_len, const uint8_t hash[32], const char *nonce,
                                   uint32_t nonce_len, int64_t now, uint8_t *status) {
    namespace K = pwaf::pow;
    if (!ks || !req || !status || !hash) return pwaf::fail(PWAF_E_INVALID_ARG, "pwaf_verify_pow_one: NULL argument");
    if ((req->user_agent_len && !req->user_agent) || (req->host_len && !req->host) || (cookie_len && !cookie) || (nonce_len && !nonce))
        return pwaf::fail(PWAF_E_INVALID_ARG, "pwaf_verify_pow_one: NULL value with a length");
    const K::Request r{req->ip, req->ip_is_v6, (const uint8_t *)req->user_agent, (const uint8_t *)req->host, hash, (const uint8_t *)nonce, req->user_agent_len, req->host_len, nonce_len};
    *status = K::decide(ks->data, reinterpret_cast<const uint8_t *>(cookie), cookie_len, now, r, nullptr);
    return PWAF_OK;
}
