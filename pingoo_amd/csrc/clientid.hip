// clientid.hip — client_id_kernel with its entry points pwaf_client_ids and pwaf_client_id_one (include/pwaf.h): the captcha client id,
// base64url_nopad(SHA-256(ip octets || user_agent || host)), of the requests of a batch (csrc/clientid.h holds the computation).
//
// One request per lane, one-wave workgroups in a persistent grid-stride loop over blocks of 64 entries; the list's length is read on the
// device, so the launch follows the kernel that wrote it (pwaf_evaluate_device's n_matches) without the host in between. A lane hashes its
// message block by block (clientid.h: four 16-byte chunks gathered from the three runs, 64 unrolled rounds over a 16-word window in
// registers); lanes whose message is finished are masked off while the longest of the wave goes on, so one very long User-Agent holds its
// wave for its own length (accepted: DESIGN.md §5.1.4). The 64 ids of a block then cross LDS (stride 11 words: odd, conflict-free) and
// leave as eleven coalesced 256-byte rows instead of 64 lanes x 11 words 44 bytes apart.
#include <hip/hip_runtime.h>

#include <string>

#include "clientid.h"
#include "colscan.h"

namespace pwaf {
namespace clientid {
namespace {

// (The workgroup is ONE wave: wave_sync, colscan.h, orders its lanes' LDS accesses.)
__global__ __launch_bounds__(64) void client_id_kernel(Args a) {
    __shared__ uint32_t tile[64 * kIdWords];
    const uint32_t lane = threadIdx.x;
    const uint32_t m = selected(a);
    uint32_t *const out = reinterpret_cast<uint32_t *>(a.out);
    for (uint64_t e0 = blockIdx.x * 64ull; e0 < m; e0 += gridDim.x * 64ull) {
        const uint64_t e = e0 + lane;
        uint32_t i = 0xFFFFFFFFu;  // (no request: n is at most 0xFFFFFFFF)
        if (e < m) i = a.idx ? a.idx[e] : (uint32_t)e;
        uint32_t words[kIdWords] = {0};  // an entry that names no request: the empty string
        if (i < a.n) client_id_words(message_of(a, i), words);
#pragma unroll
        for (uint32_t j = 0; j < kIdWords; j++) tile[lane * kIdWords + j] = words[j];
        wave_sync();
        // the block's ids are contiguous in out: words [11 e0, 11 min(e0 + 64, m))
        const uint64_t base = e0 * kIdWords, end = (uint64_t)m * kIdWords;
#pragma unroll
        for (uint32_t r = 0; r < kIdWords; r++) {
            const uint32_t k = r * 64u + lane;
            if (base + k < end) out[base + k] = tile[k];
        }
        wave_sync();  // (tile[] is rewritten by the next block)
    }
}

}  // namespace

int launch_client_ids(const Args &a, void *stream) {
    const uint32_t cap = a.idx ? a.idx_cap : a.n;
    if (cap == 0) return 0;
    const uint32_t groups = (uint32_t)(((uint64_t)cap + 63u) / 64u);
    const uint32_t blocks = groups < 8192u ? groups : 8192u;
    hipLaunchKernelGGL(client_id_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace clientid
}  // namespace pwaf

extern "C" int pwaf_client_ids(const pwaf_batch *in, const uint32_t *idx, uint32_t idx_cap, const uint32_t *n_idx, pwaf_client_id *out, void *stream) {
    namespace K = pwaf::clientid;
    using pwaf::fail;
    if (!in || !out) return fail(PWAF_E_INVALID_ARG, "pwaf_client_ids: NULL argument");
    if (int rc = pwaf::check_batch_header(in)) return rc;
    if (int rc = pwaf::check_list("pwaf_client_ids", idx, idx_cap, n_idx)) return rc;
    if ((uintptr_t)out & 3u) return fail(PWAF_E_INVALID_ARG, "pwaf_client_ids: out is not 4-byte aligned");
    const pwaf_strcol &ua = in->field[PWAF_FIELD_USER_AGENT], &host = in->field[PWAF_FIELD_HOST];
    if (int rc = pwaf::check_client_columns(in)) return rc;
    K::Args a{};
    a.ua = ua, a.host = host, a.ip = in->ip, a.ip_is_v6 = in->ip_is_v6, a.n = in->n;
    a.idx = idx, a.n_idx = n_idx, a.idx_cap = idx_cap, a.out = out;
    if (in->memory == PWAF_MEM_HOST) {
        uint32_t bad = 0;
        if (!K::ids_host(a, &bad))
            return fail(PWAF_E_BATCH, "pwaf_client_ids: entry " + std::to_string(bad) + " (request " + std::to_string(idx ? idx[bad] : bad) + "): offsets decrease");
        return PWAF_OK;
    }
    if (K::launch_client_ids(a, stream)) return fail(PWAF_E_DEVICE, "client_id_kernel launch failed");
    return PWAF_OK;
}

extern "C" int pwaf_client_id_one(const pwaf_request *req, pwaf_client_id *out) {
    namespace K = pwaf::clientid;
    if (!req || !out) return pwaf::fail(PWAF_E_INVALID_ARG, "pwaf_client_id_one: NULL argument");
    if ((req->user_agent_len && !req->user_agent) || (req->host_len && !req->host)) return pwaf::fail(PWAF_E_INVALID_ARG, "pwaf_client_id_one: NULL value with a length");
    uint32_t words[K::kIdWords];
    K::client_id_words(K::make_message(req->ip, req->ip_is_v6, (const uint8_t *)req->user_agent, req->user_agent_len, (const uint8_t *)req->host, req->host_len), words);
    memcpy(out->text, words, sizeof words);
    return PWAF_OK;
}
