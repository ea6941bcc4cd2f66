// verdict.hip — per 64-request group: hit records and attribute pairs become LDS column words, the trigger lists name the candidate
// rules, one lane per rule evaluates its DNF, first match wins. verdict_kernel keeps a column FILE per wave (dense or sparse),
// verdict2_kernel an ENTRY LIST (the default). Pipeline overview: kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "kernels.h"
#include "wave.h"

namespace pwaf {

// LDS per wave: the column file (one 64-request word per atom), a bitmap of non-zero columns, a bitmap of candidate rules
// and the ordered candidate list.
// (the column files' and program tables' LDS layout — verdict_wave_lds, verdict_wave_lds_sp, verdict_v_cap, verdict_wave_lds_el,
// verdict_tables — and the launch shape computed from it: verdictplan.h)

// BR = 64-pass bitmap registers (1: up to 64 passes, else kMaxPasses)
template <bool LT, int BR, bool SP>
__global__ __launch_bounds__(SP ? 768 : 1024, (SP && BR == 1) ? 6 : 1) void verdict_kernel(VerdictArgs a) {  // (sparse, up to 64 passes: 6 waves per SIMD = two 12-wave workgroups per CU)
    extern __shared__ __align__(16) unsigned char lds[];
    const uint32_t tid = threadIdx.x, wave = wave_index(), lane = tid & 63, n_waves = blockDim.x >> 6;
#ifdef PWAF_PROFILING
    const uint32_t dbg_skip = a.debug_skip;  // section switches for timing experiments (wrong results when set): -DPWAF_PROFILING builds only
#else
    constexpr uint32_t dbg_skip = 0;
#endif
    const uint32_t colw = (a.n_cols + 31) / 32, rulew = (a.n_rules + 31) / 32;
    const uint32_t v_cap = a.v_cap;  // (SP) values held in LDS; dirty columns of higher rank: the wave's spill array
    const uint32_t wave_bytes = SP ? verdict_wave_lds_sp(a.n_cols, a.n_rules, v_cap) : verdict_wave_lds(a.n_cols, a.n_rules);
    unsigned char *mine = lds + (size_t)wave * wave_bytes;
    // dense: col[n_cols] | colnz[colw]; sparse: nz[colw] = {dirty bits, dirty columns before the word} | vals[v_cap]
    unsigned long long *col = reinterpret_cast<unsigned long long *>(mine);
    uint32_t *colnz = reinterpret_cast<uint32_t *>(col + a.n_cols);
    uint32_t *nz = reinterpret_cast<uint32_t *>(mine);
    unsigned long long *vals = reinterpret_cast<unsigned long long *>(mine + (size_t)colw * 8);
    unsigned long long *spill = (SP && a.spill != nullptr) ? a.spill + (size_t)(blockIdx.x * n_waves + wave) * (a.n_cols - v_cap) : nullptr;
    uint32_t *rulebm = SP ? reinterpret_cast<uint32_t *>(vals + v_cap) : colnz + colw;
    uint16_t *cand = reinterpret_cast<uint16_t *>(rulebm + rulew);
    unsigned char *tables = lds + (size_t)n_waves * wave_bytes;
    const VerdictTables vt = verdict_tables(a.n_cols, a.n_rules, a.n_trig, a.n_lits, LT);
    uint16_t *l_trig_off = reinterpret_cast<uint16_t *>(tables + vt.trig_off);
    uint16_t *l_trig_rules = reinterpret_cast<uint16_t *>(tables + vt.trig_rules);
    uint2 *l_rules = reinterpret_cast<uint2 *>(tables + vt.rules);
    uint32_t *l_lits = reinterpret_cast<uint32_t *>(tables + vt.lits);
    uint16_t *l_pub = reinterpret_cast<uint16_t *>(tables + vt.pub);  // public rule index, 16 bits (the pseudo rules' 0xFFFFFFFx ids keep their low half)
    if (LT) {
        for (uint32_t k = tid; k <= a.n_cols; k += blockDim.x) l_trig_off[k] = (uint16_t)a.trig_off[k];
        for (uint32_t k = tid; k < a.n_trig; k += blockDim.x) l_trig_rules[k] = a.trig_rules[k];
        for (uint32_t k = tid; k < a.n_rules; k += blockDim.x) {
            const DevRule dr = a.rules[k];  // header without the public index (only read when the rule decides a request)
            l_rules[k] = make_uint2(dr.lit_off, dr.lit_cnt | ((uint32_t)dr.eff_unverified << 16) | ((uint32_t)dr.eff_verified << 24));
            l_pub[k] = (uint16_t)dr.public_idx;
        }
        for (uint32_t k = tid; k < a.n_lits; k += blockDim.x) l_lits[k] = a.lits[k];
    }
    __syncthreads();
    const unsigned long long mybit = 1ull << lane;
    const unsigned long long lt_mask = mybit - 1;
    unsigned long long cnt_block = 0, cnt_captcha = 0, cnt_bypass = 0, cnt_allow = 0;  // wave-uniform tallies

    // group-invariant, fetched once per wave: this lane's word of the always-candidate bitmap
    const uint32_t h_always = lane < rulew ? a.always_rules[lane] : 0u;

    // A group's inputs — the hit records of up to kPre passes, the captcha flag, the attribute kernel's pair count and first 64
    // pairs — are requested ONE GROUP AHEAD: with ~9 waves per CU nothing else hides the ~2 us those first-touch loads take.
    // Which passes: a list-driven (sparse) pass has a visited bitmap, and in most groups of 64 requests most such passes visited
    // nobody (a 4096-rule set over 64 header fields has ~90 passes, a handful of them non-empty per group). The group's 64 visited
    // bits of EVERY pass are requested TWO groups ahead, lane q holding pass q's word (dense passes: all ones); one group ahead a
    // ballot names the non-empty passes and only those get a record load — limited to the lanes whose bit is set.
    constexpr int kPre = kVerdictPre;
    constexpr int kBitRegs = BR;  // 64 passes per register
    struct Bits {
        unsigned long long w[kBitRegs];  // lane l of w[r]: the visited bits of pass r * 64 + l for the group's 64 requests
    };
    struct Inputs {
        uint32_t rv[kPre];    // the hit records of the group's first kPre non-empty passes ...
        uint32_t base[kPre];  // ... and their first columns (wave-uniform; kNone = slot unused)
        Bits bits;            // for the passes left over
        unsigned long long rest[kBitRegs];  // wave-uniform: non-empty passes that got no slot (fetched inside the group: rare)
        uint32_t flags, n_pairs;
        uint4 pair0;
        uint32_t res0;  // the first result word of the specialized residual program (VerdictArgs::res_match)
    };
    // group-invariant, per lane: the bitmap and first column of "my" pass in each register
    const uint32_t *my_bits[kBitRegs];
    uint32_t my_base[kBitRegs];
    bool my_live[kBitRegs];
#pragma unroll
    for (int r = 0; r < kBitRegs; r++) {
        const uint32_t ps = (uint32_t)r * 64 + lane;
        my_live[r] = ps < a.n_passes;
        my_bits[r] = nullptr;
        my_base[r] = 0;
        if (my_live[r]) {
            const PassInfo pi = a.passes[ps];
            const uint32_t kind = pi.kind_slot >> 24, slot = pi.kind_slot & 0xFFFFFFu;
            if (kind == 3) my_live[r] = false;  // a short-literal pass: its columns arrive as attribute pairs, it has no records
            my_bits[r] = kind == 1 ? a.cand_bits + (size_t)slot * a.bit_words : kind == 2 ? a.visit_bits + (size_t)slot * a.bit_words : nullptr;
            my_base[r] = pi.base;
        }
    }
    auto request_bits = [&](const uint32_t g, Bits &bt) {
        const uint32_t gg = min(g, a.n_groups - 1);
#pragma unroll
        for (int r = 0; r < kBitRegs; r++) {
            // (the bitmap of a batch whose size is not a multiple of 64 is padded to whole groups by the engine)
            bt.w[r] = !my_live[r] ? 0ull : my_bits[r] != nullptr ? *reinterpret_cast<const unsigned long long *>(my_bits[r] + 2 * (size_t)gg) : ~0ull;
        }
    };
    auto request_inputs = [&](const uint32_t g, const Bits &bt, Inputs &in) {
        const uint32_t i = g * 64 + lane;
        const bool valid = g < a.n_groups && i < a.n;
        unsigned long long nz[kBitRegs];
#pragma unroll
        for (int r = 0; r < kBitRegs; r++) nz[r] = (uint32_t)r * 64 < a.n_passes ? __ballot(bt.w[r] != 0) : 0ull;
#pragma unroll
        for (int q = 0; q < kPre; q++) {
            uint32_t ps = kNone, base = kNone;
            unsigned long long word = 0;
#pragma unroll
            for (int r = 0; r < kBitRegs; r++) {
                if (ps == kNone && nz[r] != 0) {  // wave-uniform
                    const int l = __builtin_ctzll(nz[r]);
                    nz[r] &= nz[r] - 1;
                    ps = (uint32_t)r * 64 + (uint32_t)l;
                    word = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(bt.w[r] >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bt.w[r], l);
                    base = (uint32_t)__builtin_amdgcn_readlane((int)my_base[r], l);
                }
            }
            in.base[q] = base;
            in.rv[q] = (ps != kNone && valid && ((word >> lane) & 1ull)) ? a.rec[(size_t)ps * a.n + i] : 0u;
        }
#pragma unroll
        for (int r = 0; r < kBitRegs; r++) in.rest[r] = nz[r];
        in.bits = bt;
        in.flags = valid ? (uint32_t)a.flags[i] : 0u;
        const uint32_t gg = min(g, a.n_groups - 1);
        in.n_pairs = a.ghdr[gg];
        in.pair0 = a.gpairs[(size_t)gg * a.pair_stride + lane];  // (the buffer is padded: reading past the group's count is harmless)
        in.res0 = (a.res_words && valid) ? a.res_match[i] : 0u;
    };
    if (!SP) {
        for (uint32_t k = lane; k < a.n_cols; k += 64) col[k] = 0;  // the column file starts clean; afterwards groups clean up after themselves
        for (uint32_t k = lane; k < colw; k += 64) colnz[k] = 0;
    }
    const uint32_t g_stride = gridDim.x * n_waves;
    Inputs cur;
    Bits b_nxt;
    {
        Bits b_cur;
        request_bits(blockIdx.x * n_waves + wave, b_cur);
        request_inputs(blockIdx.x * n_waves + wave, b_cur, cur);
        request_bits(blockIdx.x * n_waves + wave + g_stride, b_nxt);
    }

    for (uint32_t g = blockIdx.x * n_waves + wave; g < a.n_groups; g += g_stride) {
        const uint32_t i = g * 64 + lane;
        const bool valid = i < a.n;
        const unsigned long long valid_mask = __ballot(valid);
        Inputs nxt;
        request_inputs(g + g_stride, b_nxt, nxt);
        request_bits(g + 2 * g_stride, b_nxt);

        // 1. clear the column file and the bitmaps; column 0 is the constant TRUE; rules that can match with every column
        //    zero (a term made of negations only) are always candidates
        //    (dense: only the columns the previous group dirtied are cleared — the non-zero bitmap names them; sparse: the dirty bits)
        if (!SP) {
            for (uint32_t wv = lane; wv < colw; wv += 64) {
                uint32_t nzw = colnz[wv];
                colnz[wv] = wv == 0 ? 1u : 0u;
                while (nzw) {
                    col[wv * 32 + (uint32_t)__builtin_ctz(nzw)] = 0;
                    nzw &= nzw - 1;
                }
            }
        } else {
            for (uint32_t wv = lane; wv < colw; wv += 64) nz[2 * wv] = wv == 0 ? 1u : 0u;
        }
        for (uint32_t k = lane; k < rulew; k += 64) rulebm[k] = k < 64 ? h_always : a.always_rules[k];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (!SP && lane == 0) col[0] = ~0ull;

        const uint32_t flags = cur.flags;
        const uint4 *pairs = a.gpairs + (size_t)g * a.pair_stride;
        const uint32_t n_pairs = cur.n_pairs;
        const uint4 pair0 = cur.pair0;
        const unsigned long long verified_mask = __ballot(valid && (flags & PWAF_FLAG_CAPTCHA_VERIFIED));

        // Where column c's 64-request word lives. Dense: the column file. Sparse: at the column's rank among the group's dirty columns
        // (in LDS below v_cap, in the wave's spill array beyond) — valid once the ranks are known (phase 1).
        auto slot_of = [&](const uint32_t c) {
            const uint32_t w = c >> 5, bits = nz[2 * w], before = nz[2 * w + 1];
            return before + (uint32_t)__builtin_popcount(bits & ((1u << (c & 31u)) - 1u));
        };
        auto word_at = [&](const uint32_t slot) -> unsigned long long * { return slot < v_cap ? vals + slot : spill + (slot - v_cap); };
        // PHASE 0 (sparse only): dirty bits. PHASE 1 (sparse): values. PHASE 2: the dense file, bits and values at once.
        auto mark_all = [&](auto phase_tag) {
            constexpr int PH = decltype(phase_tag)::value;
            auto put = [&](const uint32_t c, const unsigned long long m) {  // (one lane speaks for column c)
                if (PH == 0) atomicOr(&nz[2 * (c >> 5)], 1u << (c & 31u));
                else if (PH == 1) atomicOr(word_at(slot_of(c)), m);
                else {
                    atomicOr(&col[c], m);
                    atomicOr(&colnz[c >> 5], 1u << (c & 31));
                }
            };
            // 2. scan results: each lane marks the columns its hit records name
            auto mark_hits = [&](const uint32_t rv, const uint32_t base) {
                if (__ballot(rv != 0) == 0) return;  // nobody in the group matched anything in this pass
                if (rv & REC_OVERFLOW) {
                    for (uint32_t k = rv & ~REC_OVERFLOW; k != kNone;) {
                        const PoolEntry pe = a.pool[k];
                        put(base + pe.atom, mybit);
                        k = pe.next;
                    }
                }
                // inline atoms: lanes that name the SAME atom (frequent atoms such as a browser User-Agent prefix are named by
                // most of the 64 requests) are folded into one column update instead of 64 serialised LDS atomics
#pragma unroll
                for (int half = 0; half < 2; half++) {
                    const uint32_t x = (rv & REC_OVERFLOW) ? 0u : (half == 0 ? rv & 0x7FFFu : (rv >> 15) & 0x7FFFu);
                    unsigned long long todo = __ballot(x != 0);
                    while (todo) {
                        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
                        const uint32_t xa = (uint32_t)__builtin_amdgcn_readlane((int)x, (int)__builtin_amdgcn_readfirstlane(leader));
                        const unsigned long long same = __ballot(x == xa);
                        todo &= ~same;
                        if (lane == leader) put(base + xa - 1, same);
                    }
                }
            };
            if (!(dbg_skip & 1u)) {
#pragma unroll
                for (int q = 0; q < kPre; q++) {
                    if (cur.base[q] == kNone) break;
                    mark_hits(cur.rv[q], cur.base[q]);
                }
                // more than kPre non-empty passes in this group (many dense passes, or a burst of candidates): fetched here
#pragma unroll
                for (int r = 0; r < kBitRegs; r++) {
                    unsigned long long m = cur.rest[r];
                    while (m) {
                        const int l = __builtin_ctzll(m);
                        m &= m - 1;
                        const uint32_t ps = (uint32_t)r * 64 + (uint32_t)l;
                        const unsigned long long word = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(cur.bits.w[r] >> 32), l) << 32) |
                                                        (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cur.bits.w[r], l);
                        const uint32_t base = (uint32_t)__builtin_amdgcn_readlane((int)my_base[r], l);
                        mark_hits((valid && ((word >> lane) & 1ull)) ? a.rec[(size_t)ps * a.n + i] : 0u, base);
                    }
                }
            }
            // 2b. residual rules evaluated by their specialized program: one result word per request and 32 rules, transposed here into the
            //     rules' column words (a ballot per rule that matched anybody in the group)
            for (uint32_t w = 0; w < a.res_words; w++) {
                const uint32_t mw = w == 0 ? cur.res0 : (valid ? a.res_match[(size_t)w * a.n + i] : 0u);
                if (__ballot(mw != 0u) == 0ull) continue;
                uint32_t any = mw;
                for (uint32_t d = 1; d < 64u; d <<= 1) any |= (uint32_t)__shfl_xor((int)any, (int)d, 64);
                any = (uint32_t)__builtin_amdgcn_readfirstlane((int)any);
                for (; any; any &= any - 1u) {
                    const uint32_t k = (uint32_t)__builtin_ctz(any);
                    const unsigned long long who = __ballot(((mw >> k) & 1u) != 0u);
                    if (lane == 0) put(a.res_base + 32u * w + k, who);
                }
            }
            // 3. everything that is not a string scan (memberships, comparisons) arrives from the attribute kernel as ready-made
            //    column words: one lane per pair (one pair per atom and group, and no scan pass owns these columns: a plain store)
            if (!(dbg_skip & 2u)) {
                for (uint32_t p = lane; p < n_pairs; p += 64) {
                    const uint4 pr = p < 64 ? pair0 : pairs[p];
                    const unsigned long long v = ((unsigned long long)pr.w << 32) | pr.z;
                    if (PH == 0) atomicOr(&nz[2 * (pr.x >> 5)], 1u << (pr.x & 31u));
                    else if (PH == 1) {
                        const uint32_t sl = slot_of(pr.x);
                        if (sl < v_cap) vals[sl] = v;
                        else atomicOr(spill + (sl - v_cap), v);
                    }
                    else {
                        col[pr.x] = v;
                        atomicOr(&colnz[pr.x >> 5], 1u << (pr.x & 31));
                    }
                }
            }
        };
        uint32_t n_dirty = 0;  // (sparse) dirty columns of the group
        if (SP) {
            mark_all(std::integral_constant<int, 0>{});
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            // the ranks: dirty columns before each word (the prefix sum also lists the dirty columns for step 4)
            for (uint32_t wb = 0; wb < colw; wb += 64) {
                const uint32_t bits = wb + lane < colw ? nz[2 * (wb + lane)] : 0u;
                const uint32_t pc = (uint32_t)__builtin_popcount(bits), incl = wave_scan_add(pc);
                if (wb + lane < colw) nz[2 * (wb + lane) + 1] = n_dirty + incl - pc;
                n_dirty += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            }
            // (column 0 = TRUE is dirty by construction and ranks first; a spilled word is reset with a read-modify-write, like everything
            // that touches it afterwards: performed at L2 in order — a plain store could still be on its way when the first OR arrives)
            for (uint32_t k = lane; k < n_dirty; k += 64) {
                if (k < v_cap) vals[k] = k == 0 ? ~0ull : 0ull;
                else atomicExch(spill + (k - v_cap), 0ull);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            mark_all(std::integral_constant<int, 1>{});
        } else {
            mark_all(std::integral_constant<int, 2>{});
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // the bitmap of non-zero columns (dense: colnz; sparse: the bit words of nz) and a column's word, for the steps below
        auto nz_bits = [&](const uint32_t wv) { return SP ? nz[2 * wv] : colnz[wv]; };
        auto col_word = [&](const uint32_t c) -> unsigned long long {
            if (!SP) return col[c];
            const uint32_t w = c >> 5, bits = nz[2 * w], before = nz[2 * w + 1];
            if (!((bits >> (c & 31u)) & 1u)) return 0ull;
            const uint32_t sl = before + (uint32_t)__builtin_popcount(bits & ((1u << (c & 31u)) - 1u));
            return sl < v_cap ? vals[sl] : __hip_atomic_load(spill + (sl - v_cap), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (a spilled word: from L2, where the ORs were performed)
        };

        // 4. candidate rules: a rule can only match some request of this group if one of its terms has a non-zero positive
        //    column (trigger lists, one chosen literal per term) or consists of negations only (always_rules).
        //    The non-zero columns are first LISTED (a prefix sum over the bitmap words' popcounts: the candidate array is free until
        //    the compaction below), then one lane takes one column. (Round 4 gave a lane a whole bitmap word: the ~60 attribute columns
        //    of a group sit in a handful of neighbouring words, so a few lanes walked eight to sixteen columns one after the other,
        //    each a chain of three dependent LDS reads, while the other sixty waited.)
        if (!(dbg_skip & 8u)) {
            uint32_t n_nz = 0;
            for (uint32_t wb = 0; wb < colw; wb += 64) {
                uint32_t nzv = wb + lane < colw ? nz_bits(wb + lane) : 0u;
                const uint32_t pc = (uint32_t)__builtin_popcount(nzv), incl = wave_scan_add(pc);
                uint32_t pos = n_nz + incl - pc;
                while (nzv) {
                    if (pos < a.n_rules) cand[pos] = (uint16_t)((wb + lane) * 32 + (uint32_t)__builtin_ctz(nzv));  // (n_cols < 65536: launch_verdict)
                    pos++;
                    nzv &= nzv - 1;
                }
                n_nz += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (n_nz <= a.n_rules) {
                for (uint32_t j = lane; j < n_nz; j += 64) {
                    const uint32_t c = cand[j];
                    const uint32_t kb = LT ? (uint32_t)l_trig_off[c] : a.trig_off[c], ke = LT ? (uint32_t)l_trig_off[c + 1] : a.trig_off[c + 1];
                    for (uint32_t k = kb; k < ke; k++) {
                        const uint32_t r = LT ? (uint32_t)l_trig_rules[k] : (uint32_t)a.trig_rules[k];
                        atomicOr(&rulebm[r >> 5], 1u << (r & 31));
                    }
                }
            } else {  // (more non-zero columns than the list holds: word by word)
                for (uint32_t wv = lane; wv < colw; wv += 64) {
                    uint32_t nzv = nz_bits(wv);
                    while (nzv) {
                        const uint32_t c = wv * 32 + (uint32_t)__builtin_ctz(nzv);
                        nzv &= nzv - 1;
                        const uint32_t kb = LT ? (uint32_t)l_trig_off[c] : a.trig_off[c], ke = LT ? (uint32_t)l_trig_off[c + 1] : a.trig_off[c + 1];
                        for (uint32_t k = kb; k < ke; k++) {
                            const uint32_t r = LT ? (uint32_t)l_trig_rules[k] : (uint32_t)a.trig_rules[k];
                            atomicOr(&rulebm[r >> 5], 1u << (r & 31));
                        }
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // ordered compaction of the rule bitmap into the candidate list (ascending rule index = evaluation order)
        uint32_t n_cand = 0;
        for (uint32_t wb = 0; wb < rulew && !(dbg_skip & 16u); wb += 64) {
            const uint32_t word = wb + lane < rulew ? rulebm[wb + lane] : 0u;
            const uint32_t pc = (uint32_t)__builtin_popcount(word), incl = wave_scan_add(pc);
            uint32_t pos = n_cand + incl - pc, wrd = word;
            while (wrd) {
                cand[pos++] = (uint16_t)((wb + lane) * 32 + (uint32_t)__builtin_ctz(wrd));
                wrd &= wrd - 1;
            }
            n_cand += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

        // 5. evaluate candidates: one lane per rule, 64 requests per ALU op. Each candidate's 64-request match word goes to LDS;
        //    then every REQUEST lane scans the words in rule order for its own bit (broadcast reads), so first-match-wins needs
        //    no lane-to-lane traffic
        unsigned long long pending = valid_mask;
        bool undecided = valid;
        uint32_t my_action = PWAF_ACTION_ALLOW, my_rule = PWAF_RULE_NONE;
        for (uint32_t base = 0; base < n_cand && pending != 0 && !(dbg_skip & 32u); base += 64) {
            unsigned long long fire = 0;
            if (base + lane < n_cand) {
                const uint32_t my_cand = cand[base + lane];
                uint32_t lit_off, lit_cnt, eff_u, eff_v;
                if (LT) {
                    const uint2 hdr = l_rules[my_cand];
                    lit_off = hdr.x;
                    lit_cnt = hdr.y & 0xFFFFu;
                    eff_u = (hdr.y >> 16) & 0xFFu;
                    eff_v = hdr.y >> 24;
                } else {
                    const DevRule dr = a.rules[my_cand];
                    lit_off = dr.lit_off;
                    lit_cnt = dr.lit_cnt;
                    eff_u = dr.eff_unverified;
                    eff_v = dr.eff_verified;
                }
                unsigned long long acc_or = 0, acc_and = ~0ull;
                // literals four at a time: the four literal words are requested together, then the four column words — two
                // LDS round trips per four literals instead of eight dependent ones (a padding literal is column 0 = TRUE)
                for (uint32_t k = lit_off; k < lit_off + lit_cnt; k += 4) {
                    uint32_t lit[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) lit[q] = k + q < lit_off + lit_cnt ? (LT ? l_lits[k + q] : a.lits[k + q]) : 0u;
                    unsigned long long cw[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) cw[q] = (lit[q] & LIT_LAZY) ? 0ull : col_word(lit[q] & LIT_ATOM_MASK);  // (no LAZY literal reaches this kernel — engine.cpp packs them for verdict2 only — but its low bits are no column)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        acc_and &= (lit[q] & LIT_NEG) ? ~cw[q] : cw[q];
                        if (lit[q] & LIT_TERM_END) {
                            acc_or |= acc_and;
                            acc_and = ~0ull;
                        }
                    }
                }
                // a match only decides when the rule's action list yields an effect for that client
                fire = acc_or & ((eff_u ? ~verified_mask : 0ull) | (eff_v ? verified_mask : 0ull));
            }
            if (dbg_skip & 256u) fire = 0;
            // first match wins: the candidates that fire for ANYBODY (a few per group: most candidates' terms stay false) are taken in
            // rule order, each word broadcast from its lane — a request's rule is the first word that holds its bit. (Round 4 parked
            // all 64 words in LDS and every request lane read them back, sixteen rounds of four broadcast reads per 64 candidates.)
            unsigned long long firing = (dbg_skip & 128u) ? 0ull : __ballot(fire != 0);
            uint32_t first = kNone;
            while (firing != 0 && pending != 0) {
                const int j = __builtin_ctzll(firing);
                firing &= firing - 1;
                const unsigned long long fj = (((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(fire >> 32), j) << 32) |
                                               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)fire, j)) & pending;
                if (fj & mybit) first = (uint32_t)j;
                pending &= ~fj;
            }
            if (undecided && first != kNone) {
                undecided = false;
                const uint32_t jc = cand[base + first];
                uint32_t eff_u, eff_v;
                if (LT) {
                    const uint32_t y = l_rules[jc].y;
                    eff_u = (y >> 16) & 0xFFu;
                    eff_v = y >> 24;
                    const uint32_t pi = l_pub[jc];
                    my_rule = pi >= 0xFFF0u ? 0xFFFF0000u | pi : pi;
                } else {
                    const DevRule dr = a.rules[jc];
                    eff_u = dr.eff_unverified;
                    eff_v = dr.eff_verified;
                    my_rule = dr.public_idx;
                }
                my_action = (verified_mask & mybit) ? eff_v : eff_u;
            }
        }

        if (dbg_skip & 64u) my_rule = n_cand;  // profiling aid: report the candidate count instead of the deciding rule
        // 6. outputs
        if (valid) {
            uint2 v;
            v.x = my_action;  // action in byte 0, pad bytes zero
            v.y = my_rule;
            *reinterpret_cast<uint2 *>(&a.out[i]) = v;
        }
        const unsigned long long m_block = __ballot(valid && my_action == PWAF_ACTION_BLOCK);
        const unsigned long long m_captcha = __ballot(valid && my_action == PWAF_ACTION_CAPTCHA);
        const unsigned long long m_bypass = __ballot(valid && my_action == PWAF_ACTION_BYPASS);
        cnt_block += (unsigned)__builtin_popcountll(m_block);
        cnt_captcha += (unsigned)__builtin_popcountll(m_captcha);
        cnt_bypass += (unsigned)__builtin_popcountll(m_bypass);
        cnt_allow += (unsigned)__builtin_popcountll(valid_mask & ~(m_block | m_captcha | m_bypass));
        if (a.match_idx != nullptr) {
            // compaction of non-Allow requests: wave ballot + prefix popcount, one atomic per group
            const unsigned long long hit = m_block | m_captcha | m_bypass;
            if (hit) {
                uint32_t basei = 0;
                if (lane == 0) basei = atomicAdd(a.n_matches, (uint32_t)__builtin_popcountll(hit));
                basei = __builtin_amdgcn_readfirstlane(basei);
                if (hit & mybit) a.match_idx[basei + (uint32_t)__builtin_popcountll(hit & lt_mask)] = i;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        cur = nxt;
    }
    // Action counters: one atomic per counter and WORKGROUP. (One per wave was measured at 0.25 ms of a 0.6 ms kernel: at the end of
    // every round of workgroups thousands of same-address atomics queue up at the L2.)
    __syncthreads();  // every wave is done with its column file: the start of LDS can hold the tallies
    unsigned long long *tally = reinterpret_cast<unsigned long long *>(lds);
    if (lane == 0) {
        tally[wave * 4 + PWAF_ACTION_ALLOW] = cnt_allow;
        tally[wave * 4 + PWAF_ACTION_BLOCK] = cnt_block;
        tally[wave * 4 + PWAF_ACTION_CAPTCHA] = cnt_captcha;
        tally[wave * 4 + PWAF_ACTION_BYPASS] = cnt_bypass;
    }
    __syncthreads();
    if (a.counts != nullptr && tid < 4) {
        unsigned long long sum = 0;
        for (uint32_t wv = 0; wv < n_waves; wv++) sum += tally[wv * 4 + tid];
        if (sum) atomicAdd(&a.counts[tid], sum);
    }
}

// -------------------------------------------------------------------------------------------------
// verdict, ENTRY-LIST form (round 6; the default: VerdictArgs::sparse_mode 3, 4 = its test hook with 8 entry slots)
// -------------------------------------------------------------------------------------------------
// What a group of 64 requests knows about its columns arrives as a LIST already: the attribute kernel's (column, mask) pairs, one per
// atom that holds for somebody, and per scan pass a handful of distinct atoms named by the hit records. The sparse column file above
// turns that list into {dirty bits, rank, value} in two marking passes with a prefix sum between them and a third walk over the bitmap
// to list the dirty columns again for the trigger step — 0.14 ms of marking and 0.08 ms of listing / triggers in a 0.31 ms kernel
// (profiles/r6_verdict_sections.txt). Here an entry keeps the place it is appended at:
//     slot[column]  one BYTE per column: 0 = clean, 1 + entry index, 255 = the entry lies beyond e_cap: its word is spill[column]
//     vals[e], ecol[e]  the entry's 64-request word and its column (to clean slot[] after the group: only the entries are touched)
// One pass over the inputs, a whole batch of up to 64 entries per instruction: lane k of the batch registers writes slot, value and column
// of entry n + k and walks the column's trigger list. The hit records' atoms are first gathered into the batch registers with
// v_writelane (one entry per DISTINCT atom of a pass: lanes naming the same atom are folded by a ballot). Column 0 = TRUE is entry 0
// for the life of the wave. A column's word for the DNF step is two dependent LDS reads (slot, value), like the sparse file's.
// Duplicates: a column belongs to one pass; inside a pass only an overflow chain (a request with more than two atoms) can name a column that
// another lane's record already named — a pass with such a record appends one column at a time through a lookup of slot[] (rare).
// (a wave's LDS: verdictplan.h, verdict_wave_lds_el)

// one wave-uniform (column, mask) into lane l of three registers (see park64)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void park96(uint32_t &c, uint32_t &lo, uint32_t &hi, const uint32_t col, const unsigned long long m, const uint32_t l) {
    // (scalar registers whatever the register allocator did with the wave-uniform values: under scalar-register pressure it keeps some in
    // vector registers and hands THOSE to an "s" operand)
    const uint32_t s_col = (uint32_t)__builtin_amdgcn_readfirstlane((int)col), s_l = (uint32_t)__builtin_amdgcn_readfirstlane((int)l);
    const uint32_t s_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m), s_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32));
    asm volatile("s_mov_b32 m0, %4\n\ts_nop 0\n\tv_writelane_b32 %0, %3, m0\n\tv_writelane_b32 %1, %5, m0\n\tv_writelane_b32 %2, %6, m0"
                 : "+v"(c), "+v"(lo), "+v"(hi)
                 : "s"(s_col), "s"(s_l), "s"(s_lo), "s"(s_hi)
                 : "m0");
}
#pragma clang diagnostic pop

// HITS (PWAF_OPT_RULE_HITS, only when a hit output was asked for): every candidate's match word is reported, not only the first firing one.
// The candidate loop then runs to the end of the list, a lane keeps acc_or beside fire, and per chunk of 64 candidates the non-zero words
// of caller rules are queued for a.hits (the wave's queue leaves up to 64 entries at a time: one atomic on n_hits per flush). Requests answered by a gate are
// masked out: the two gate pseudo rules are device rules 0 and 1 (compile.cpp prepends them), the candidate list ascends, so they stand
// in the FIRST chunk and a gated request is decided (both gates always take effect) before that chunk's words are appended.
// (HITS, up to 64 passes: 5 waves per SIMD. The plain kernel fills its 80 registers at 6; the queue's three more put one into scratch there.
// A CU then holds ONE 12-wave workgroup at a time; the persistent grid is unchanged, its workgroups take turns.)
// ROUTES (an engine created with routes, only when a route output was asked for; never with HITS): the caller's routes are the device rules
// [a.route_base, a.n_rules), behind every rule, with effects {ALLOW, ALLOW}: they never fire. A lane that holds one keeps its match word
// where a rule's lane keeps `fire`; the candidate list ascends, so a chunk's route lanes are its upper lanes (one wave-uniform mask). A second
// ordered pick over those lanes, against `rpending`, gives each request its first route, whatever its verdict: the loop runs until both
// the verdicts and the routes of the group are known.
template <bool LT, int BR, bool HITS, bool ROUTES>
__global__ __launch_bounds__(768, BR == 1 ? (HITS ? 5 : 6) : 1) void verdict2_kernel(VerdictArgs a) {
    static_assert(!(HITS && ROUTES), "one call answers one of the reports");
    extern __shared__ __align__(16) unsigned char lds[];
    const uint32_t tid = threadIdx.x, wave = wave_index(), lane = tid & 63, n_waves = blockDim.x >> 6;
#ifdef PWAF_PROFILING
    const uint32_t dbg_skip = a.debug_skip;
#else
    constexpr uint32_t dbg_skip = 0;
#endif
    const uint32_t rulew = (a.n_rules + 31) / 32;
    const uint32_t e_cap = a.v_cap;  // entries held in LDS (entry 0 = TRUE included); later entries: the wave's spill array, by column
    const uint32_t wave_bytes = verdict_wave_lds_el(a.n_cols, a.n_rules, e_cap);
    unsigned char *mine = lds + (size_t)wave * wave_bytes;
    unsigned long long *vals = reinterpret_cast<unsigned long long *>(mine);
    uint32_t *rulebm = reinterpret_cast<uint32_t *>(vals + e_cap);
    uint16_t *ecol = reinterpret_cast<uint16_t *>(rulebm + rulew);
    uint16_t *cand = reinterpret_cast<uint16_t *>(reinterpret_cast<unsigned char *>(ecol) + ((e_cap * 2 + 3) & ~3u));
    uint8_t *slot = reinterpret_cast<unsigned char *>(cand) + ((a.n_rules * 2 + 3) & ~3u);
    const uint32_t slot_words = ((a.n_cols + 7) & ~7u) / 4;
    unsigned long long *spill = a.spill + (size_t)(blockIdx.x * n_waves + wave) * a.n_cols;
    unsigned char *tables = lds + (size_t)n_waves * wave_bytes;
    const VerdictTables vt = verdict_tables(a.n_cols, a.n_rules, a.n_trig, a.n_lits, LT);
    uint16_t *l_trig_off = reinterpret_cast<uint16_t *>(tables + vt.trig_off);
    uint16_t *l_trig_rules = reinterpret_cast<uint16_t *>(tables + vt.trig_rules);
    uint2 *l_rules = reinterpret_cast<uint2 *>(tables + vt.rules);
    uint32_t *l_lits = reinterpret_cast<uint32_t *>(tables + vt.lits);
    uint16_t *l_pub = reinterpret_cast<uint16_t *>(tables + vt.pub);
    if (LT) {
        for (uint32_t k = tid; k <= a.n_cols; k += blockDim.x) l_trig_off[k] = (uint16_t)a.trig_off[k];
        for (uint32_t k = tid; k < a.n_trig; k += blockDim.x) l_trig_rules[k] = a.trig_rules[k];
        for (uint32_t k = tid; k < a.n_rules; k += blockDim.x) {
            const DevRule dr = a.rules[k];
            l_rules[k] = make_uint2(dr.lit_off, dr.lit_cnt | ((uint32_t)dr.eff_unverified << 16) | ((uint32_t)dr.eff_verified << 24));
            l_pub[k] = (uint16_t)dr.public_idx;
        }
        for (uint32_t k = tid; k < a.n_lits; k += blockDim.x) l_lits[k] = a.lits[k];
    }
    // the wave's slot bytes start clean; entry 0 is column 0 = TRUE
    for (uint32_t k = lane; k < slot_words; k += 64) reinterpret_cast<uint32_t *>(slot)[k] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (lane == 0) {
        slot[0] = 1;
        vals[0] = ~0ull;
        ecol[0] = 0;
    }
    __syncthreads();
    const unsigned long long mybit = 1ull << lane;
    const unsigned long long lt_mask = mybit - 1;
    unsigned long long cnt_block = 0, cnt_captcha = 0, cnt_bypass = 0, cnt_allow = 0;
    // (HITS) the wave's entries wait in three registers, lane k = entry k, and leave up to 64 at a time: ONE atomic on n_hits and one coalesced
    // store per flush. (One returning atomic per wave and chunk of candidates was measured at 1.5 ms of a 1.78 ms kernel for 10M requests x
    // 1024 rules: ~7 entries per group, a few hundred thousand same-address atomics that the L2 performs one after the other.) An entry is
    // {rule | k << 16, mask}: its group is the k-th of this wave counted from q_g0, the group of the queue's first entry.
    uint32_t q_rk = 0, q_lo = 0, q_hi = 0, q_n = 0, q_g0 = 0, q_k = 0;
    const uint32_t q_stride = gridDim.x * n_waves;
    auto q_flush = [&]() {
        if (q_n == 0) return;
        uint32_t slot0 = 0;
        if (lane == 0) slot0 = atomicAdd(a.n_hits, q_n);
        slot0 = __builtin_amdgcn_readfirstlane(slot0);
        const uint32_t at = slot0 + lane;
        if (lane < q_n && at < a.hits_cap) {  // (never at or beyond hits + hits_cap, whatever the counter held)
            pwaf_rule_hit h;
            h.rule_idx = q_rk & 0xFFFFu;
            h.group = q_g0 + (q_rk >> 16) * q_stride;
            h.mask = ((unsigned long long)q_hi << 32) | q_lo;
            a.hits[at] = h;
        }
        q_n = 0;
    };
    const uint32_t h_always = lane < rulew ? a.always_rules[lane] : 0u;
    const bool true_triggers = a.trig_off[1] != a.trig_off[0];  // rules whose chosen positive literal is the constant TRUE (`expression: None`)

    // inputs one group ahead, visited bits two groups ahead: see verdict_kernel
    // (<= 64 passes: a group of the 1k-rule set has one dense pass and two or three non-empty sparse ones; every slot costs a dozen instructions per group
    // whether it is used or not — the rest are fetched inside the group)
    constexpr int kPre = BR == 1 ? 4 : kVerdictPre;
    constexpr int kBitRegs = BR;
    struct Bits {
        unsigned long long w[kBitRegs];
    };
    struct Inputs {
        uint32_t rv[kPre];
        uint32_t base[kPre];
        Bits bits;
        unsigned long long rest[kBitRegs];
        uint32_t flags, n_pairs;
        uint4 pair0;
        uint32_t res0;
        // the lazy comparison variables (VerdictArgs::lazy_var, at most two), RAW — nothing here may wait for a load: a length as the request's END
        // offset (its start is the neighbour lane's end; lane 0's is fetched when an atom is evaluated: rare), the port as it is
        uint32_t lraw[2];
    };
    const uint32_t *my_bits[kBitRegs];
    uint32_t my_base[kBitRegs];
    bool my_live[kBitRegs];
#pragma unroll
    for (int r = 0; r < kBitRegs; r++) {
        const uint32_t ps = (uint32_t)r * 64 + lane;
        my_live[r] = ps < a.n_passes;
        my_bits[r] = nullptr;
        my_base[r] = 0;
        if (my_live[r]) {
            const PassInfo pi = a.passes[ps];
            const uint32_t kind = pi.kind_slot >> 24, sl = pi.kind_slot & 0xFFFFFFu;
            if (kind == 3) my_live[r] = false;
            my_bits[r] = kind == 1 ? a.cand_bits + (size_t)sl * a.bit_words : kind == 2 ? a.visit_bits + (size_t)sl * a.bit_words : nullptr;
            my_base[r] = pi.base;
        }
    }
    auto request_bits = [&](const uint32_t g, Bits &bt) {
        const uint32_t gg = min(g, a.n_groups - 1);
#pragma unroll
        for (int r = 0; r < kBitRegs; r++)
            bt.w[r] = !my_live[r] ? 0ull : my_bits[r] != nullptr ? *reinterpret_cast<const unsigned long long *>(my_bits[r] + 2 * (size_t)gg) : ~0ull;
    };
    auto request_inputs = [&](const uint32_t g, const Bits &bt, Inputs &in) {
        const uint32_t i = g * 64 + lane;
        const bool valid = g < a.n_groups && i < a.n;
        unsigned long long nzp[kBitRegs];
        // The visited words (the youngest loads in flight: request_bits of the previous turn) are waited for HERE, once. Every use below
        // sits under a wave-uniform condition, where the compiler waits for ALL outstanding loads again — after the first slot that
        // means for the record load just issued: one exposed round trip per prefetch slot.
#pragma unroll
        for (int r = 0; r < kBitRegs; r++) asm volatile("" ::"v"(bt.w[r]));
#pragma unroll
        for (int r = 0; r < kBitRegs; r++) nzp[r] = (uint32_t)r * 64 < a.n_passes ? __ballot(bt.w[r] != 0) : 0ull;
#pragma unroll
        for (int q = 0; q < kPre; q++) {
            uint32_t ps = kNone, base = kNone;
            unsigned long long word = 0;
#pragma unroll
            for (int r = 0; r < kBitRegs; r++) {
                if (ps == kNone && nzp[r] != 0) {
                    const int l = __builtin_ctzll(nzp[r]);
                    nzp[r] &= nzp[r] - 1;
                    ps = (uint32_t)r * 64 + (uint32_t)l;
                    word = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(bt.w[r] >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bt.w[r], l);
                    base = (uint32_t)__builtin_amdgcn_readlane((int)my_base[r], l);
                }
            }
            in.base[q] = base;
            in.rv[q] = (ps != kNone && valid && ((word >> lane) & 1ull)) ? a.rec[(size_t)ps * a.n + i] : 0u;
        }
#pragma unroll
        for (int r = 0; r < kBitRegs; r++) in.rest[r] = nzp[r];
        in.bits = bt;
        in.flags = valid ? (uint32_t)a.flags[i] : 0u;
        const uint32_t gg = min(g, a.n_groups - 1);
        {
            // one register, three group-wide words: lane 0 = the attribute kernel's pair count, lane 1 + s = the group's FIRST offset of lazy length
            // variable s (lane 0's start: every other lane's start is its neighbour's end)
            const uint32_t *src = a.ghdr + gg;
#pragma unroll
            for (uint32_t sl = 0; sl < 2; sl++) {
                if (sl >= a.n_lazy_var) break;
                const uint32_t vi = a.lazy_var[sl];
                if (vi != 5u && lane == 1u + sl) src = (vi < 5u ? a.off[vi] : a.hoff[vi - 7u]) + gg * 64u;
            }
            in.n_pairs = *src;
        }
        in.pair0 = a.gpairs[(size_t)gg * a.pair_stride + lane];
        in.res0 = (a.res_words && valid) ? a.res_match[i] : 0u;
        in.lraw[0] = in.lraw[1] = 0u;
        const uint32_t ii = valid ? i : 0u;
#pragma unroll
        for (uint32_t sl = 0; sl < 2; sl++) {
            if (sl >= a.n_lazy_var || (dbg_skip & 2048u)) break;  // (wave-uniform)
            const uint32_t vi = a.lazy_var[sl];
            if (vi == 5u) {
                in.lraw[sl] = a.port[ii];
            } else {
                const uint32_t *o = vi < 5u ? a.off[vi] : a.hoff[vi - 7u];
                in.lraw[sl] = o[ii + 1];
            }
        }
    };
    const uint32_t g_stride = gridDim.x * n_waves;
    Inputs cur;
    Bits b_nxt;
    {
        Bits b_cur;
        request_bits(blockIdx.x * n_waves + wave, b_cur);
        request_inputs(blockIdx.x * n_waves + wave, b_cur, cur);
        request_bits(blockIdx.x * n_waves + wave + g_stride, b_nxt);
    }

    for (uint32_t g = blockIdx.x * n_waves + wave; g < a.n_groups; g += g_stride) {
        const uint32_t i = g * 64 + lane;
        const bool valid = i < a.n;
        const unsigned long long valid_mask = __ballot(valid);
        Inputs nxt;
        request_inputs(g + g_stride, b_nxt, nxt);
        request_bits(g + 2 * g_stride, b_nxt);

        // 1. the rule bitmap starts from the rules that need no positive column (a term made of negations only)
        for (uint32_t k = lane; k < rulew; k += 64) rulebm[k] = k < 64 ? h_always : a.always_rules[k];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

        const uint32_t flags = cur.flags;
        const uint4 *pairs = a.gpairs + (size_t)g * a.pair_stride;
        const uint32_t n_pairs = (uint32_t)__builtin_amdgcn_readlane((int)cur.n_pairs, 0);
        const unsigned long long verified_mask = __ballot(valid && (flags & PWAF_FLAG_CAPTCHA_VERIFIED));

        uint32_t n_entries = 1;  // (entry 0 = TRUE)
        // a column's rules: the rule bitmap gets the trigger list of every appended column
        auto triggers = [&](const uint32_t c) {
            if (dbg_skip & 8u) return;
            const uint32_t kb = LT ? (uint32_t)l_trig_off[c] : a.trig_off[c], ke = LT ? (uint32_t)l_trig_off[c + 1] : a.trig_off[c + 1];
            for (uint32_t k = kb; k < ke; k++) {
                const uint32_t r = LT ? (uint32_t)l_trig_rules[k] : (uint32_t)a.trig_rules[k];
                atomicOr(&rulebm[r >> 5], 1u << (r & 31));
            }
        };
        // `cnt` entries, lane k < cnt holding entry n_entries + k (distinct columns, none of them appended before)
        if (true_triggers && lane == 0) triggers(0);  // (entry 0 = TRUE is never appended: a match-all rule is filed under column 0)
        auto append_batch = [&](const uint32_t c, const uint32_t lo, const uint32_t hi, const uint32_t cnt) {
            if (lane < cnt) {
                const uint32_t e = n_entries + lane;
                const unsigned long long m = ((unsigned long long)hi << 32) | lo;
                if (e < e_cap) {
                    slot[c] = (uint8_t)(e + 1u);
                    vals[e] = m;
                    ecol[e] = (uint16_t)c;
                } else {
                    slot[c] = 255;
                    atomicExch(spill + c, m);  // (a read-modify-write, like everything that touches a spilled word: performed at L2 in order)
                }
                triggers(c);
            }
            n_entries += cnt;
        };
        // the batch registers: the attribute kernel's first pairs are entries as they come (lane k = pair k); the scans' entries are gathered
        // behind them one (wave-uniform) column at a time — one batch, one append, in the common case
        const uint32_t n_first = (dbg_skip & 2u) ? 0u : min(n_pairs, 64u);
        uint32_t b_col = cur.pair0.x, b_lo = cur.pair0.z, b_hi = cur.pair0.w, bn = n_first;
        if (bn == 64) {
            append_batch(b_col, b_lo, b_hi, 64);
            bn = 0;
        }
        auto flush = [&]() {
            if (bn == 0) return;
            append_batch(b_col, b_lo, b_hi, bn);
            bn = 0;
        };
        auto append = [&](const uint32_t c, const unsigned long long m) {
            park96(b_col, b_lo, b_hi, c, m, bn);
            if (++bn == 64) flush();
        };
        // one wave-uniform column that MAY have an entry already (passes with overflow chains): through slot[]
        auto merge_or_append = [&](const uint32_t c, const unsigned long long m) {
            const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)slot[c]);
            if (s == 0) {
                const uint32_t e = n_entries++;
                if (lane == 0) {
                    if (e < e_cap) {
                        slot[c] = (uint8_t)(e + 1u);
                        vals[e] = m;
                        ecol[e] = (uint16_t)c;
                    } else {
                        slot[c] = 255;
                        atomicExch(spill + c, m);
                    }
                    triggers(c);
                }
            } else if (lane == 0) {
                if (s < 255u) vals[s - 1u] |= m;
                else atomicOr(spill + c, m);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        };
        // 2. scan results: per pass one entry per DISTINCT atom its records name (lanes naming the same atom are one ballot)
        auto mark_hits = [&](const uint32_t rv, const uint32_t base) {
            if (__ballot(rv != 0) == 0) return;
            const bool chained = (rv & REC_OVERFLOW) != 0;
            const bool any_chain = __ballot(chained) != 0;
            if (any_chain) {
                flush();
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
            const uint32_t x0 = chained ? 0u : rv & 0x7FFFu, x1 = chained ? 0u : (rv >> 15) & 0x7FFFu;
            unsigned long long t0 = __ballot(x0 != 0), t1 = __ballot(x1 != 0);
            while ((t0 | t1) != 0) {
                uint32_t xa;
                if (t0 != 0) xa = (uint32_t)__builtin_amdgcn_readlane((int)x0, __builtin_ctzll(t0));
                else xa = (uint32_t)__builtin_amdgcn_readlane((int)x1, __builtin_ctzll(t1));
                const unsigned long long s0 = __ballot(x0 == xa), s1 = __ballot(x1 == xa);
                t0 &= ~s0;
                t1 &= ~s1;
                if (any_chain) merge_or_append(base + xa - 1u, s0 | s1);
                else append(base + xa - 1u, s0 | s1);
            }
            if (any_chain) {
                // the chains, all lanes advancing together: per step the distinct atoms of the lanes that still have one
                uint32_t k = chained ? rv & ~REC_OVERFLOW : kNone;
                while (__ballot(k != kNone) != 0) {
                    uint32_t x = 0;
                    if (k != kNone) {
                        const PoolEntry pe = a.pool[k];
                        x = pe.atom + 1u;
                        k = pe.next;
                    }
                    unsigned long long todo = __ballot(x != 0);
                    while (todo != 0) {
                        const uint32_t xa = (uint32_t)__builtin_amdgcn_readlane((int)x, __builtin_ctzll(todo));
                        const unsigned long long same = __ballot(x == xa);
                        todo &= ~same;
                        merge_or_append(base + xa - 1u, same);
                    }
                }
            }
        };
        if (!(dbg_skip & 1u)) {
#pragma unroll
            for (int q = 0; q < kPre; q++) {
                if (cur.base[q] == kNone) break;
                mark_hits(cur.rv[q], cur.base[q]);
            }
#pragma unroll
            for (int r = 0; r < kBitRegs; r++) {
                unsigned long long m = cur.rest[r];
                while (m) {
                    const int l = __builtin_ctzll(m);
                    m &= m - 1;
                    const uint32_t ps = (uint32_t)r * 64 + (uint32_t)l;
                    const unsigned long long word = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(cur.bits.w[r] >> 32), l) << 32) |
                                                    (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cur.bits.w[r], l);
                    const uint32_t base = (uint32_t)__builtin_amdgcn_readlane((int)my_base[r], l);
                    mark_hits((valid && ((word >> lane) & 1ull)) ? a.rec[(size_t)ps * a.n + i] : 0u, base);
                }
            }
        }
        // 2b. the specialized residual program's result words: one entry per rule that matched anybody in the group
        for (uint32_t w = 0; w < a.res_words; w++) {
            const uint32_t mw = w == 0 ? cur.res0 : (valid ? a.res_match[(size_t)w * a.n + i] : 0u);
            if (__ballot(mw != 0u) == 0ull) continue;
            for (uint32_t any = wave_or(mw); any; any &= any - 1u) {
                const uint32_t k = (uint32_t)__builtin_ctz(any);
                append(a.res_base + 32u * w + k, __ballot(((mw >> k) & 1u) != 0u));
            }
        }
        flush();
        // 3. the attribute kernel's pairs beyond the first 64 (rare)
        if (!(dbg_skip & 2u)) {
            for (uint32_t p0 = 64; p0 < n_pairs; p0 += 64) {
                const uint32_t cnt = min(64u, n_pairs - p0);
                uint4 pr = make_uint4(0u, 0u, 0u, 0u);
                if (lane < cnt) pr = pairs[p0 + lane];
                append_batch(pr.x, pr.z, pr.w, cnt);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // a column's word: two dependent LDS reads, no branch (entry 0 = TRUE stands in for a clean column's index) — unless the group
        // appended more entries than LDS holds (wave-uniform, rare): then a spilled word comes from L2, where the ORs were performed
        const bool spilled = n_entries > e_cap;
        auto col_word = [&](const uint32_t c) -> unsigned long long {
            const uint32_t s = slot[c];
            if (!spilled) {
                const unsigned long long v = vals[s ? s - 1u : 0u];
                return s ? v : 0ull;
            }
            if (s == 0) return 0ull;
            return s < 255u ? vals[s - 1u] : __hip_atomic_load(spill + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        };

        // 4. ordered compaction of the rule bitmap into the candidate list (ascending rule index = evaluation order)
        uint32_t n_cand = 0;
        for (uint32_t wb = 0; wb < rulew && !(dbg_skip & 16u); wb += 64) {
            const uint32_t word = wb + lane < rulew ? rulebm[wb + lane] : 0u;
            const uint32_t pc = (uint32_t)__builtin_popcount(word), incl = wave_scan_add(pc);
            uint32_t pos = n_cand + incl - pc, wrd = word;
            while (wrd) {
                cand[pos++] = (uint16_t)((wb + lane) * 32 + (uint32_t)__builtin_ctz(wrd));
                wrd &= wrd - 1;
            }
            n_cand += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

        // 5. evaluate candidates: one lane per rule, 64 requests per ALU op; first match wins (see verdict_kernel)
        unsigned long long pending = valid_mask;
        uint32_t n_exact = 0;
        bool undecided = valid;
        uint32_t my_action = PWAF_ACTION_ALLOW, my_rule = PWAF_RULE_NONE;
        unsigned long long gated = 0;  // (HITS) requests answered by a gate pseudo rule: known after the first chunk
        unsigned long long rpending = ROUTES ? valid_mask : 0ull;  // (ROUTES) requests whose route is not known yet
        uint32_t my_route = PWAF_ROUTE_NONE;
        for (uint32_t base = 0; base < n_cand && (HITS || pending != 0 || (ROUTES && rpending != 0)) && !(dbg_skip & 32u); base += 64) {
            unsigned long long fire = 0, eff_mask = 0;
            unsigned long long match = 0;  // (HITS) the rule's match word whatever its actions
            uint32_t lit_off = 0, lit_cnt = 0;
            bool lazy_seen = false;
            bool is_route = false;
            if (base + lane < n_cand) {
                const uint32_t my_cand = cand[base + lane];
                if (ROUTES) is_route = my_cand >= a.route_base;
                uint32_t eff_u, eff_v;
                if (LT) {
                    const uint2 hdr = l_rules[my_cand];
                    lit_off = hdr.x;
                    lit_cnt = hdr.y & 0xFFFFu;
                    eff_u = (hdr.y >> 16) & 0xFFu;
                    eff_v = hdr.y >> 24;
                } else {
                    const DevRule dr = a.rules[my_cand];
                    lit_off = dr.lit_off;
                    lit_cnt = dr.lit_cnt;
                    eff_u = dr.eff_unverified;
                    eff_v = dr.eff_verified;
                }
                unsigned long long acc_or = 0, acc_and = ~0ull;
                for (uint32_t k = lit_off; k < lit_off + lit_cnt; k += 4) {
                    uint32_t lit[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) lit[q] = k + q < lit_off + lit_cnt ? (LT ? l_lits[k + q] : a.lits[k + q]) : 0u;
                    unsigned long long cw[4];
#pragma unroll
                    // (a LAZY literal's low bits are its constant, operator and slot, not a column — up to 0x7FFFF: it must not index slot[]
                    // or the spill array; its word is not used below)
                    for (int q = 0; q < 4; q++) cw[q] = (lit[q] & LIT_LAZY) ? 0ull : col_word(lit[q] & LIT_ATOM_MASK);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        // a LAZY comparison atom reads as TRUE here, negated or not: what comes out is a superset of the rule's matches
                        const unsigned long long t = (lit[q] & LIT_NEG) ? ~cw[q] : cw[q];
                        acc_and &= (lit[q] & LIT_LAZY) ? ~0ull : t;
                        lazy_seen = lazy_seen || (lit[q] & LIT_LAZY) != 0u;
                        if (lit[q] & LIT_TERM_END) {
                            acc_or |= acc_and;
                            acc_and = ~0ull;
                        }
                    }
                }
                eff_mask = (eff_u ? ~verified_mask : 0ull) | (eff_v ? verified_mask : 0ull);
                // (ROUTES: a route's lane keeps its match word in `fire` — its own eff_mask is 0 — through the exact evaluation below)
                if (ROUTES && is_route) eff_mask = valid_mask;
                fire = acc_or & eff_mask;
                if (HITS) match = acc_or & valid_mask;
            }
            // Rules with lazy comparison atoms whose OTHER literals hold for somebody (rare): the rule again, exactly, one request per lane —
            // an eager literal's bit from its column word, a lazy one from the request's own value (fetched with the group's inputs)
            // (HITS: also for a rule whose match word is non-zero while no action of its takes effect for those requests)
            if (dbg_skip & 512u) n_exact += (uint32_t)__builtin_popcountll(__ballot(lazy_seen && (HITS ? match : fire) != 0));
            for (unsigned long long need = (dbg_skip & 1024u) ? 0ull : __ballot(lazy_seen && (HITS ? match : fire) != 0); need != 0; need &= need - 1) {
                const int j = __builtin_ctzll(need);
                const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)lit_off, j), cn = (uint32_t)__builtin_amdgcn_readlane((int)lit_cnt, j);
                const unsigned long long em = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(eff_mask >> 32), j) << 32) |
                                              (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)eff_mask, j);
                bool r_or = false, r_and = true;
                for (uint32_t k = lo; k < lo + cn; k++) {
                    const uint32_t lit = (uint32_t)__builtin_amdgcn_readfirstlane((int)(LT ? l_lits[k] : a.lits[k]));
                    bool bit;
                    if (lit & LIT_LAZY) {
                        const uint32_t cc = lit & 0xFFFFu, sl = (lit >> 17) & 1u;
                        const uint32_t raw = sl ? cur.lraw[1] : cur.lraw[0];  // (no dynamic index: the inputs stay in registers)
                        uint32_t v = raw;
                        if (a.lazy_var[sl] != 5u) {  // length = end - the neighbour's end (lane 0: the group's first offset)
                            const uint32_t st0 = sl ? (uint32_t)__builtin_amdgcn_readlane((int)cur.n_pairs, 2) : (uint32_t)__builtin_amdgcn_readlane((int)cur.n_pairs, 1);
                            v = raw - (uint32_t)__builtin_amdgcn_update_dpp((int)st0, (int)raw, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
                        }
                        bit = (lit & 0x10000u) ? v <= cc : v == cc;
                        if (lit & 0x40000u) bit = !bit;  // (the atom's polarity on the device: engine.cpp, POLARITY)
                    } else {
                        bit = ((col_word(lit & LIT_ATOM_MASK) >> lane) & 1ull) != 0ull;
                    }
                    if (lit & LIT_NEG) bit = !bit;
                    r_and = r_and && bit;
                    if (lit & LIT_TERM_END) {
                        r_or = r_or || r_and;
                        r_and = true;
                    }
                }
                const unsigned long long exact_all = __ballot(r_or && valid);
                if (HITS) {  // the match word is the exact result WITHOUT the action mask (fire follows from it below)
                    uint32_t m_lo = (uint32_t)match, m_hi = (uint32_t)(match >> 32);
                    park64(m_lo, m_hi, exact_all, (uint32_t)j);
                    match = ((unsigned long long)m_hi << 32) | m_lo;
                } else {
                    uint32_t f_lo = (uint32_t)fire, f_hi = (uint32_t)(fire >> 32);
                    park64(f_lo, f_hi, exact_all & em, (uint32_t)j);
                    fire = ((unsigned long long)f_hi << 32) | f_lo;
                }
            }
            // (HITS: one word less to keep through the loop above; the same value on every valid request, and `pending` holds no other)
            if (HITS) fire = match & eff_mask;
            unsigned long long firing = __ballot(fire != 0);
            unsigned long long rfiring = 0;
            if (ROUTES) {  // the route lanes' words are picked apart from the rules': they decide no verdict
                const unsigned long long rlanes = __ballot(is_route);
                rfiring = firing & rlanes;
                firing &= ~rlanes;
            }
            uint32_t first = kNone;
            while (firing != 0 && pending != 0) {
                const int j = __builtin_ctzll(firing);
                firing &= firing - 1;
                const unsigned long long fj = (((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(fire >> 32), j) << 32) |
                                               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)fire, j)) & pending;
                if (fj & mybit) first = (uint32_t)j;
                pending &= ~fj;
            }
            if (undecided && first != kNone) {
                undecided = false;
                const uint32_t jc = cand[base + first];
                uint32_t eff_u, eff_v;
                if (LT) {
                    const uint32_t y = l_rules[jc].y;
                    eff_u = (y >> 16) & 0xFFu;
                    eff_v = y >> 24;
                    const uint32_t pi = l_pub[jc];
                    my_rule = pi >= 0xFFF0u ? 0xFFFF0000u | pi : pi;
                } else {
                    const DevRule dr = a.rules[jc];
                    eff_u = dr.eff_unverified;
                    eff_v = dr.eff_verified;
                    my_rule = dr.public_idx;
                }
                my_action = (verified_mask & mybit) ? eff_v : eff_u;
            }
            if (ROUTES) {
                // the second ordered pick: the first route lane whose word holds the request (a request leaves rpending once)
                uint32_t rfirst = kNone;
                while (rfiring != 0 && rpending != 0) {
                    const int j = __builtin_ctzll(rfiring);
                    rfiring &= rfiring - 1;
                    const unsigned long long rj = (((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(fire >> 32), j) << 32) |
                                                   (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)fire, j)) & rpending;
                    if (rj & mybit) rfirst = (uint32_t)j;
                    rpending &= ~rj;
                }
                if (rfirst != kNone) {
                    const uint32_t jc = cand[base + rfirst];
                    my_route = LT ? (uint32_t)l_pub[jc] : a.rules[jc].public_idx;
                }
            }
            if (HITS) {
                if (base == 0) gated = __ballot(valid && !undecided && my_rule >= 0xFFFFFFF0u);
                // (a gate pseudo rule's own word is a subset of `gated`: nothing of it is left, so every non-zero word is a caller rule's)
                const unsigned long long word = match & ~gated;
                unsigned long long has = __ballot(word != 0);
                if (has != 0) {
                    uint32_t pub = 0;  // the caller's index of this lane's rule (< 65520: engine.cpp)
                    if (word != 0) {
                        const uint32_t c = cand[base + lane];
                        pub = LT ? (uint32_t)l_pub[c] : a.rules[c].public_idx;
                        if (a.rule_hits != nullptr) atomicAdd(&a.rule_hits[pub], (unsigned long long)__builtin_popcountll(word));
                    }
                    if (a.n_hits != nullptr) {
                        if (q_n + (uint32_t)__builtin_popcountll(has) > 64u) q_flush();
                        if (q_n == 0) {
                            q_g0 = g;
                            q_k = 0;
                        }
                        for (; has != 0; has &= has - 1) {  // one entry per lane with a word, into lane q_n of the queue registers
                            const int j = __builtin_ctzll(has);
                            const unsigned long long wj = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(word >> 32), j) << 32) |
                                                          (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)word, j);
                            park96(q_rk, q_lo, q_hi, (uint32_t)__builtin_amdgcn_readlane((int)pub, j) | (q_k << 16), wj, q_n);
                            q_n++;
                        }
                    }
                }
            }
        }
        if (dbg_skip & 512u) my_rule = n_exact;  // profiling aid: rules evaluated exactly for their lazy comparison atoms
        if (dbg_skip & 64u) my_rule = n_cand | (n_entries << 16);  // profiling aid: candidates and entries of the group instead of the deciding rule

        // 6. outputs
        if (valid) {
            uint2 v;
            v.x = my_action;
            v.y = my_rule;
            *reinterpret_cast<uint2 *>(&a.out[i]) = v;
            if (ROUTES) a.route[i] = my_route;  // (one coalesced 4-byte store per lane; PWAF_ROUTE_NONE where no route matched)
        }
        const unsigned long long m_block = __ballot(valid && my_action == PWAF_ACTION_BLOCK);
        const unsigned long long m_captcha = __ballot(valid && my_action == PWAF_ACTION_CAPTCHA);
        const unsigned long long m_bypass = __ballot(valid && my_action == PWAF_ACTION_BYPASS);
        cnt_block += (unsigned)__builtin_popcountll(m_block);
        cnt_captcha += (unsigned)__builtin_popcountll(m_captcha);
        cnt_bypass += (unsigned)__builtin_popcountll(m_bypass);
        cnt_allow += (unsigned)__builtin_popcountll(valid_mask & ~(m_block | m_captcha | m_bypass));
        if (a.match_idx != nullptr) {
            const unsigned long long hit = m_block | m_captcha | m_bypass;
            if (hit) {
                uint32_t basei = 0;
                if (lane == 0) basei = atomicAdd(a.n_matches, (uint32_t)__builtin_popcountll(hit));
                basei = __builtin_amdgcn_readfirstlane(basei);
                if (hit & mybit) a.match_idx[basei + (uint32_t)__builtin_popcountll(hit & lt_mask)] = i;
            }
        }
        // 7. the group cleans up after itself: the slot bytes of its entries (all of slot[] when entries went beyond e_cap: their columns
        //    are not listed)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (n_entries <= e_cap) {
            for (uint32_t e = 1u + lane; e < n_entries; e += 64) slot[ecol[e]] = 0;
        } else {
            for (uint32_t k = lane; k < slot_words; k += 64) reinterpret_cast<uint32_t *>(slot)[k] = 0u;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (lane == 0) slot[0] = 1;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (HITS && q_n != 0 && ++q_k == 0x10000u) q_flush();  // (an entry's group index relative to the queue's first has 16 bits)
        cur = nxt;
    }
    if (HITS && a.n_hits != nullptr) q_flush();
    __syncthreads();
    unsigned long long *tally = reinterpret_cast<unsigned long long *>(lds);
    if (lane == 0) {
        tally[wave * 4 + PWAF_ACTION_ALLOW] = cnt_allow;
        tally[wave * 4 + PWAF_ACTION_BLOCK] = cnt_block;
        tally[wave * 4 + PWAF_ACTION_CAPTCHA] = cnt_captcha;
        tally[wave * 4 + PWAF_ACTION_BYPASS] = cnt_bypass;
    }
    __syncthreads();
    if (a.counts != nullptr && tid < 4) {
        unsigned long long sum = 0;
        for (uint32_t wv = 0; wv < n_waves; wv++) sum += tally[wv * 4 + tid];
        if (sum) atomicAdd(&a.counts[tid], sum);
    }
}

// Every instantiation, named once: launch_verdict picks from these tables, configure_verdict_kernels walks them.
// verdict_kernel [SP][LT][BR == 1], verdict2_kernel [plain / HITS / ROUTES][LT][BR == 1].
static constexpr int kBRmax = (kMaxPasses + 1 + 63) / 64;
static const void *const kVerdictFns[2][2][2] = {
    {{reinterpret_cast<const void *>(verdict_kernel<false, kBRmax, false>), reinterpret_cast<const void *>(verdict_kernel<false, 1, false>)},
     {reinterpret_cast<const void *>(verdict_kernel<true, kBRmax, false>), reinterpret_cast<const void *>(verdict_kernel<true, 1, false>)}},
    {{reinterpret_cast<const void *>(verdict_kernel<false, kBRmax, true>), reinterpret_cast<const void *>(verdict_kernel<false, 1, true>)},
     {reinterpret_cast<const void *>(verdict_kernel<true, kBRmax, true>), reinterpret_cast<const void *>(verdict_kernel<true, 1, true>)}}};
static const void *const kVerdict2Fns[3][2][2] = {
    {{reinterpret_cast<const void *>(verdict2_kernel<false, kBRmax, false, false>), reinterpret_cast<const void *>(verdict2_kernel<false, 1, false, false>)},
     {reinterpret_cast<const void *>(verdict2_kernel<true, kBRmax, false, false>), reinterpret_cast<const void *>(verdict2_kernel<true, 1, false, false>)}},
    {{reinterpret_cast<const void *>(verdict2_kernel<false, kBRmax, true, false>), reinterpret_cast<const void *>(verdict2_kernel<false, 1, true, false>)},
     {reinterpret_cast<const void *>(verdict2_kernel<true, kBRmax, true, false>), reinterpret_cast<const void *>(verdict2_kernel<true, 1, true, false>)}},
    {{reinterpret_cast<const void *>(verdict2_kernel<false, kBRmax, false, true>), reinterpret_cast<const void *>(verdict2_kernel<false, 1, false, true>)},
     {reinterpret_cast<const void *>(verdict2_kernel<true, kBRmax, false, true>), reinterpret_cast<const void *>(verdict2_kernel<true, 1, false, true>)}}};

// (the workgroup shape of the verdict kernels — verdict_shape, verdict_blocks_sp, kLdsPerGroup: verdictplan.h)
int launch_verdict(const VerdictArgs &a, void *stream) {
    VerdictShape sh = verdict_shape(a.n_cols, a.n_rules, a.n_trig, a.n_lits, a.force_global_tables != 0, (int)a.sparse_mode, a.n_passes);
    if (!verdict_launchable(sh, a.n_cols)) return (int)hipErrorInvalidValue;  // (engine_create refuses such programs)
    if (sh.sparse == 1 && (a.v_cap != sh.v_cap || (sh.v_cap < a.n_cols && a.spill == nullptr))) return (int)hipErrorInvalidValue;
    if (sh.sparse == 2 && (a.v_cap != sh.v_cap || a.spill == nullptr)) return (int)hipErrorInvalidValue;
#ifdef PWAF_PROFILING
    static const uint32_t cap_waves = getenv("PWAF_VERDICT_WAVES") ? (uint32_t)atoi(getenv("PWAF_VERDICT_WAVES")) : 0u;  // timing experiment: fewer waves per CU (same results)
    if (cap_waves && cap_waves < sh.waves) sh.waves = cap_waves;
#endif
    int variant = verdict_variant(a.n_passes);
#ifdef PWAF_PROFILING
    static const int forced_variant = getenv("PWAF_VERDICT_VARIANT") ? atoi(getenv("PWAF_VERDICT_VARIANT")) : -1;  // a MORE general variant may be forced (same results)
    if (forced_variant >= 0 && forced_variant < variant) variant = forced_variant;
#endif
    // the rule-hit variants only when a hit output was asked for (PWAF_OPT_RULE_HITS engines; the entry-list kernel only: engine_create)
    const bool want_hits = a.n_hits != nullptr || a.rule_hits != nullptr;
    if (want_hits && (sh.sparse != 2 || (a.hits == nullptr && a.n_hits != nullptr && a.hits_cap != 0))) return (int)hipErrorInvalidValue;
    // the route variants only when a route output was asked for (engines created with routes; the entry-list kernel only; one report per call)
    const bool want_routes = a.route != nullptr;
    if (want_routes && (sh.sparse != 2 || want_hits || a.route_base > a.n_rules)) return (int)hipErrorInvalidValue;
    const void *fn = sh.sparse == 2 ? kVerdict2Fns[want_routes ? 2 : want_hits ? 1 : 0][sh.lds_tables ? 1 : 0][variant] : kVerdictFns[sh.sparse ? 1 : 0][sh.lds_tables ? 1 : 0][variant];
    uint32_t blocks = (a.n_groups + sh.waves - 1) / sh.waves;
#ifdef PWAF_PROFILING
    static const uint32_t forced_cap = getenv("PWAF_VERDICT_BLOCKS") ? (uint32_t)atoi(getenv("PWAF_VERDICT_BLOCKS")) : 0u;
#else
    const uint32_t forced_cap = 0;
#endif
    // with LDS tables a workgroup fills a CU: one persistent workgroup per CU (measured: 0.331 ms vs 0.346 at 4 per CU — every
    // workgroup stages 25 KiB of tables and clears its column files once); small workgroups: a few rounds per CU
    const uint32_t cap = (forced_cap && !sh.sparse) ? forced_cap : sh.sparse ? verdict_blocks_sp(sh, a.attr_blocks) : sh.lds_tables ? std::max(1u, a.attr_blocks) : 2048u;
    if (blocks > cap) blocks = cap;
    if (blocks == 0) return 0;
    void *args[] = {const_cast<VerdictArgs *>(&a)};
    hipError_t e = hipLaunchKernel(fn, dim3(blocks), dim3(sh.waves * 64), args, sh.lds_bytes, (hipStream_t)stream);
    return (int)(e != hipSuccess ? e : hipGetLastError());
}

int configure_verdict_kernels() {
    auto raise = [](const void *const *fns, size_t count) {
        for (size_t k = 0; k < count; k++) {
            hipError_t e = hipFuncSetAttribute(fns[k], hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerGroup);
            if (e != hipSuccess) return (int)e;
        }
        return 0;
    };
    if (int e = raise(&kVerdictFns[0][0][0], sizeof(kVerdictFns) / sizeof(void *))) return e;
    return raise(&kVerdict2Fns[0][0][0], sizeof(kVerdict2Fns) / sizeof(void *));
}

}  // namespace pwaf
