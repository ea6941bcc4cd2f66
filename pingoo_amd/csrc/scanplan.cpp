// scanplan.cpp — see scanplan.h: the scan tables, the pass roles and the host half of tuning, planned without a device.
#include "scanplan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "lscan_split.h"

namespace pwaf {

int fail(int code, const std::string &msg);  // program_api.cpp: records pwaf_last_error()

std::vector<uint8_t> class_image(const DfaGroup &g, const std::vector<uint32_t> *cpos, uint32_t &ill_class) {
    std::vector<uint8_t> img(kUmapAt, 0);
    for (int b = 0; b < 256; b++) img[(size_t)b] = (uint8_t)(cpos ? (*cpos)[g.classmap[b]] : g.classmap[b]);
    ill_class = 0;
    if (g.umap.on()) {
        ScalarMap m = g.umap;
        if (cpos) {
            for (auto &c : m.stage2) c = (uint8_t)(*cpos)[c];
            m.ill_class = (uint8_t)(*cpos)[m.ill_class];
        }
        ill_class = m.ill_class;
        const std::vector<uint8_t> u = scalar_map_image(m);
        img.insert(img.end(), u.begin(), u.end());
    }
    return img;
}

// Builds the device form of one DFA group: see the cell encoding in kernels.h. `visits` (optional, one count per state) is a
// traffic profile from pwaf_engine_tune: the LDS-resident ("hot") rows are then the most visited states instead of the
// shallowest ones. The result of a scan never depends on which rows are hot.
int build_device_group(const DfaGroup &g, uint32_t lds_hot_budget, ScanImage &d, const std::vector<uint64_t> *visits, const std::vector<uint64_t> *class_freq) {
    const uint32_t C = g.n_classes, stride = C + 3, stride2 = stride * 2;
    // Class numbering = cell position inside a row. An LDS lookup conflicts when two lanes hit different dwords of one bank
    // (32 banks x 4 B = 128 B: DESIGN.md §6); lanes that sit in the SAME row — the usual case, most walks hover around the
    // start state — conflict exactly when their classes are a multiple of 64 cells apart. With more than 64 classes some
    // positions have no alias inside the row: given a traffic profile, the most frequent classes get those.
    std::vector<uint32_t> cpos(C);
    for (uint32_t c = 0; c < C; c++) cpos[c] = c;
    if (class_freq && class_freq->size() >= C && C > 64) {
        std::vector<uint32_t> by_freq(C), slots;
        for (uint32_t c = 0; c < C; c++) by_freq[c] = c;
        std::stable_sort(by_freq.begin(), by_freq.end(), [&](uint32_t x, uint32_t y) { return (*class_freq)[x] > (*class_freq)[y]; });
        // positions ordered by how many positions of the row share their bank (p mod 64): alone first, then pairs, then triples
        for (uint32_t share = 1; share <= 5; share++)
            for (uint32_t p = 0; p < C; p++) {
                const uint32_t r = p % 64, n_share = (C - 1 - r) / 64 + 1;
                if (n_share == share) slots.push_back(p);
            }
        for (uint32_t k = 0; k < C; k++) cpos[by_freq[k]] = slots[k];
    }
    if (g.n_states > kMaxDfaStates) return fail(PWAF_E_UNSUPPORTED, "DFA has more than 32767 states");
    std::vector<uint32_t> &list_off = d.list_off;
    std::vector<uint16_t> &list = d.list;
    list_off.assign(1, 0);
    list.clear();
    auto add_list = [&](const std::vector<uint16_t> &src, uint32_t b, uint32_t e) -> uint32_t {
        list.insert(list.end(), src.begin() + b, src.begin() + e);
        list_off.push_back((uint32_t)list.size());
        return (uint32_t)list_off.size() - 1;  // 1 + id
    };
    std::vector<uint32_t> emit_id(g.n_states, 0);
    for (uint32_t s = 0; s < g.n_states; s++)
        if (g.emit_off[s + 1] > g.emit_off[s]) emit_id[s] = add_list(g.emit_list, g.emit_off[s], g.emit_off[s + 1]);
    // what entering the start state emits is recorded when a request starts (start_emit); re-entering it adds nothing
    const uint32_t start_emit = emit_id[0];
    emit_id[0] = 0;

    // Row order: the start state, then by visit count (profile) or BFS depth (the DFA builder's state order).
    std::vector<uint32_t> order(g.n_states);
    for (uint32_t s = 0; s < g.n_states; s++) order[s] = s;
    if (visits && visits->size() == g.n_states)
        std::stable_sort(order.begin() + 1, order.end(), [&](uint32_t x, uint32_t y) { return (*visits)[x] > (*visits)[y]; });

    // Cell value space (uint16): [0, emit_base) plain hot rows, [emit_base, (n_hot+1)*stride) hot rows that emit + the sentinel
    // row, the rest indexes `special` (one entry per cold state). Shrink the hot set until everything fits.
    const uint32_t budget = std::min<uint32_t>(lds_hot_budget, 131070u);
    uint32_t n_hot = budget > 2 * stride2 ? (budget - stride2) / stride2 : 1;
    n_hot = std::max(1u, std::min(n_hot, g.n_states));
    for (;;) {
        const uint64_t need = (uint64_t)(n_hot + 1) * stride + (g.n_states - n_hot);
        if (need <= 65535) break;
        // (defensive: never taken. With n_hot == 1 the need is 2 * stride + n_states - 1 <= 2 * 259 + 32766 = 33284: at most 256 classes
        // (a class is a uint8_t of classmap) and at most kMaxDfaStates states (refused above))
        if (n_hot == 1) return fail(PWAF_E_UNSUPPORTED, "DFA too large for the 16-bit cell space");
        const uint32_t over = (uint32_t)(need - 65535);
        n_hot = std::max(1u, n_hot - std::max(1u, over / (stride - 1) + 1));  // an evicted row frees `stride` cells and adds one special
    }
    // hot rows: plain ones first, then the emitting ones (one compare against emit_base finds both "emits" and "special")
    std::stable_partition(order.begin() + 1, order.begin() + n_hot, [&](uint32_t s) { return emit_id[s] == 0; });
    uint32_t n_plain = n_hot;
    for (uint32_t q = 0; q < n_hot; q++)
        if (emit_id[order[q]]) { n_plain = q; break; }
    std::vector<uint32_t> pos(g.n_states);
    for (uint32_t q = 0; q < g.n_states; q++) pos[order[q]] = q;
    const uint32_t emit_base = n_plain * stride, special_base = (n_hot + 1) * stride;
    std::vector<SpecialCell> &special = d.special;
    special.clear();
    for (uint32_t q = n_hot; q < g.n_states; q++) special.push_back({q * stride2, emit_id[order[q]]});
    auto cell_of = [&](uint32_t t) -> uint16_t { return pos[t] < n_hot ? (uint16_t)(pos[t] * stride) : (uint16_t)(special_base + (pos[t] - n_hot)); };

    std::vector<uint16_t> &tab = d.tab;
    tab.assign((size_t)g.n_states * stride, 0);
    for (uint32_t q = 0; q < g.n_states; q++) {
        const uint32_t s = order[q];
        uint16_t *row = &tab[(size_t)q * stride];
        for (uint32_t c = 0; c < C; c++) row[cpos[c]] = cell_of(g.trans[(size_t)s * C + c]);
        row[C] = q < n_hot ? (uint16_t)(q * stride) : (uint16_t)0xFFFF;  // STAY
        if (g.end_off[s + 1] > g.end_off[s]) {
            // END cell: like the EMIT cell — 0x8000 | atom for a single match (whole-string equality, the usual case: no list
            // walk, no memory access when a request finishes), else 1 + list id
            if (g.end_off[s + 1] - g.end_off[s] == 1 && g.end_list[g.end_off[s]] < 0x8000u) {
                row[C + 1] = (uint16_t)(0x8000u | g.end_list[g.end_off[s]]);
            } else {
                const uint32_t id1 = add_list(g.end_list, g.end_off[s], g.end_off[s + 1]);
                if (id1 >= 0x8000u) return fail(PWAF_E_UNSUPPORTED, "too many match lists in one DFA group");
                row[C + 1] = (uint16_t)id1;
            }
        }
        if (emit_id[s]) {
            // EMIT cell of a hot row: 0x8000 | atom for a single match, else 1 + list id
            const uint32_t b = list_off[emit_id[s] - 1], en = list_off[emit_id[s]];
            if (en - b == 1 && list[b] < 0x8000u) row[C + 2] = (uint16_t)(0x8000u | list[b]);
            else if (emit_id[s] < 0x8000u) row[C + 2] = (uint16_t)emit_id[s];
            else return fail(PWAF_E_UNSUPPORTED, "too many match lists in one DFA group");
        }
    }
    if (special.empty()) special.push_back({0, 0});
    d.n_states = g.n_states;
    d.stride = stride;
    d.n_classes = C;
    d.n_hot = n_hot;
    d.start_emit = start_emit;
    d.emit_base = emit_base;
    d.special_base = special_base;
    d.atom_base = g.atom_base;
    d.n_local = g.n_local;
    d.field = g.field;
    d.classmap = class_image(g, &cpos, d.ill_class);
    d.scalar_mode = g.umap.on();
    return PWAF_OK;
}

// The flat form of a group for lscan_kernel. States are renumbered — start state first, then by visits of the tuning sample
// (discovery order without one) — so that the rows lscan_kernel stages in LDS are the ones its walks spend their steps in.
void build_flat_group(const DfaGroup &g, uint32_t lds_bytes, FlatImage &d, const std::vector<uint64_t> *visits) {
    const uint32_t S = g.n_states, C = g.n_classes;
    d.n_states = S;
    d.n_classes = C;
    std::vector<uint32_t> order(S), pos(S);
    for (uint32_t s = 0; s < S; s++) order[s] = s;
    if (visits && visits->size() == S) std::stable_sort(order.begin() + 1, order.end(), [&](uint32_t x, uint32_t y) { return (*visits)[x] > (*visits)[y]; });
    // DELTA rows. A row that is not LDS-resident costs an L2 round trip per step, and with 64 walks in lockstep some lane is in
    // such a row in nearly every group of steps once a twentieth of the steps are (hostile traffic: near misses of the rule
    // literals, deep in the patterns' prefix chains). But such states are the cheap kind: a state deep inside one literal differs
    // from a shallow state — the one its failure transitions lead back to — in one or two cells. A state within TWO cells of one
    // of the hottest rows is therefore kept in LDS as an 8-byte record (base row, two exception cells) instead of a row of 100-150
    // bytes: measured on the 1k-rule set, all of the hostile stream's steps outside the resident rows are in such states. The rows /
    // records split maximises the sample visits covered (no sample: the states covered).
    const uint32_t row_bytes = 2u * (C + 3u), budget = lds_bytes;
    const uint32_t cap_rows = std::min<uint32_t>(S, (budget - 48u) / row_bytes);
    d.n_full = cap_rows;
    d.n_delta = 0;
    std::vector<uint64_t> &delta_rec = d.delta;
    delta_rec.clear();
    if (S > cap_rows && cap_rows >= 8 && C <= 255) {
        const uint32_t B = std::min<uint32_t>(cap_rows, 512u);  // candidate base rows: the hottest ones
        struct Near { uint16_t base; uint8_t n, c[2]; };
        std::vector<Near> near(S, Near{0, 255, {0, 0}});
        for (uint32_t q = B; q < S; q++) {
            const uint32_t s = order[q];
            const uint16_t *rs = &g.trans[(size_t)s * C];
            for (uint32_t b = 0; b < B && near[s].n != 0; b++) {
                const uint16_t *rb = &g.trans[(size_t)order[b] * C];
                uint32_t nd = 0;
                uint8_t cc[2] = {0, 0};
                for (uint32_t c = 0; c < C && nd <= 2; c++)
                    if (rs[c] != rb[c]) { if (nd < 2) cc[nd] = (uint8_t)c; nd++; }
                if (nd <= 2 && nd < near[s].n) near[s] = Near{(uint16_t)b, (uint8_t)nd, {cc[0], cc[1]}};
            }
        }
        auto weight = [&](uint32_t s) { return (visits && visits->size() == S ? (double)(*visits)[s] : 0.0) + 1e-3; };
        double best_score = -1;
        uint32_t best_n = cap_rows;
        for (uint32_t n = cap_rows;; n = n >= B + 16 ? n - 16 : B) {
            const uint64_t space = (uint64_t)budget - (uint64_t)n * row_bytes;
            uint64_t room = space > 48 ? (space - 48) / 8 : 0;
            double score = 0;
            for (uint32_t q = 0; q < n; q++) score += weight(order[q]);
            for (uint32_t q = n; q < S && room; q++)
                if (near[order[q]].n <= 2) { score += weight(order[q]); room--; }
            if (score > best_score) { best_score = score; best_n = n; }
            if (n == B) break;
        }
        // rows [0, n_full), then the records (in visit order, as many as fit), then everything else
        std::vector<uint32_t> full(order.begin(), order.begin() + best_n), recs, rest;
        uint64_t room = (uint64_t)budget - (uint64_t)best_n * row_bytes > 48 ? ((uint64_t)budget - (uint64_t)best_n * row_bytes - 48) / 8 : 0;
        for (uint32_t q = best_n; q < S; q++) {
            if (near[order[q]].n <= 2 && room) { recs.push_back(order[q]); room--; }
            else rest.push_back(order[q]);
        }
        d.n_full = best_n;
        d.n_delta = (uint32_t)recs.size();
        order = full;
        order.insert(order.end(), recs.begin(), recs.end());
        order.insert(order.end(), rest.begin(), rest.end());
        for (uint32_t q = 0; q < S; q++) pos[order[q]] = q;
        // (a class that STAYS — a continuation byte of scalar mode — enters nothing: its cell, the state itself, carries no emit flag)
        auto cell_of = [&](uint32_t t, uint32_t c) { return (uint16_t)(pos[t] | ((g.emit_off[(size_t)t + 1] != g.emit_off[t] && !(c < g.class_stays.size() && g.class_stays[c])) ? 0x8000u : 0u)); };
        for (uint32_t s : recs) {
            const Near &nr = near[s];
            const uint16_t *rs = &g.trans[(size_t)s * C];
            const uint8_t c1 = nr.n >= 1 ? nr.c[0] : 0, c2 = nr.n >= 2 ? nr.c[1] : c1;
            // (no exception: both slots repeat the base row's own cell of class 0)
            const uint16_t t1 = cell_of(rs[c1], c1), t2 = cell_of(rs[c2], c2);
            delta_rec.push_back((uint64_t)nr.base | ((uint64_t)c1 << 16) | ((uint64_t)c2 << 24) | ((uint64_t)t1 << 32) | ((uint64_t)t2 << 48));
        }
    }
    for (uint32_t q = 0; q < S; q++) pos[order[q]] = q;
    // row = C transition cells (next state | 0x8000 when entering it emits) + one EMIT cell: what entering THIS state emits —
    // 0 = nothing, 0x8000 | local atom = exactly one atom (the common case: settled in registers by the kernel), else 1 + the state's
    // index into emit_off (a list). The cell rides with the row into LDS: round 2 called the out-of-line list walk (three dependent
    // global loads, ~2 us for the whole wave) for every match of every lane — benign candidates are mostly true hits, so a wave of
    // 64 candidates stalled on the order of a hundred times per walk.
    // ... one STAY cell (= the state itself, unflagged): what a lane past its field's end "reads", so that no step is conditional,
    // and one END cell (1 = the field ending in this state emits): a finished walk learns it from the row instead of two global loads.
    const uint32_t stride = C + 3;
    std::vector<uint16_t> &flat = d.flat, &emit_list = d.emit_list, &end_list = d.end_list;
    std::vector<uint32_t> &emit_off = d.emit_off, &end_off = d.end_off;
    flat.assign((size_t)S * stride, 0);
    emit_off.assign(1, 0);
    end_off.assign(1, 0);
    emit_list.clear();
    end_list.clear();
    for (uint32_t q = 0; q < S; q++) {
        const uint32_t s = order[q];
        for (uint32_t c = 0; c < C; c++) {
            const uint32_t t = g.trans[(size_t)s * C + c];
            const bool stays = c < g.class_stays.size() && g.class_stays[c];  // (a continuation byte of scalar mode: the state itself, entering nothing)
            flat[(size_t)q * stride + c] = (uint16_t)(pos[t] | ((g.emit_off[(size_t)t + 1] != g.emit_off[t] && !stays) ? 0x8000u : 0u));
        }
        const uint32_t ne = g.emit_off[(size_t)s + 1] - g.emit_off[s];
        flat[(size_t)q * stride + C] = ne == 0 ? (uint16_t)0 : (ne == 1 && g.emit_list[g.emit_off[s]] < 0x7FFFu) ? (uint16_t)(0x8000u | g.emit_list[g.emit_off[s]]) : (uint16_t)1;
        flat[(size_t)q * stride + C + 1] = (uint16_t)q;
        flat[(size_t)q * stride + C + 2] = g.end_off[(size_t)s + 1] != g.end_off[s] ? (uint16_t)1 : (uint16_t)0;  // the END cell: the field ending in this state emits (a list)
        emit_list.insert(emit_list.end(), g.emit_list.begin() + g.emit_off[s], g.emit_list.begin() + g.emit_off[(size_t)s + 1]);
        emit_off.push_back((uint32_t)emit_list.size());
        end_list.insert(end_list.end(), g.end_list.begin() + g.end_off[s], g.end_list.begin() + g.end_off[(size_t)s + 1]);
        end_off.push_back((uint32_t)end_list.size());
    }
    d.classmap = class_image(g, nullptr, d.ill_class);
    d.scalar_mode = g.umap.on();
    if (delta_rec.empty()) delta_rec.push_back(0);
}

// (scanplan.h) Called at creation and again when pwaf_engine_tune has rebuilt the filters from a traffic sample.
void plan_passes(const Program &P, const std::vector<GroupFilter> &filters, const std::vector<double> &mean_len, bool residual_specialized, bool skip_identity,
                 PassPlan &e) {
    const size_t n_groups = P.groups.size();
    e = PassPlan();
    e.roles.assign(n_groups, PassRole());
    e.owns_factors.assign(n_groups, 0);
    std::vector<uint32_t> &colmask = e.colmask;
    colmask.assign(P.n_cols, 0);
    // list slots: gated gap passes own slots [0, kGapLists) — their index is also their bit in the factor masks — and every
    // filtered pass one slot after those
    for (size_t k = 0; k < n_groups; k++) {
        PassRole &d = e.roles[k];
        const bool gap = !P.groups[k].filter_cols.empty();
        if (gap) {
            if (e.n_gap >= kGapLists) continue;  // (beyond 32 gap passes the rest simply walk every request)
            d.gate = (int)e.n_gap;
            for (uint32_t c : P.groups[k].filter_cols) colmask[c] |= 1u << e.n_gap;
            e.n_gap++;
        } else if (filters[k].enabled) {
            d.gate = (int)(kGapLists + e.n_filtered);
            d.filtered = true;
            e.n_filtered++;
            // the confirm tier built with this filter (program.h: ConfirmTable)
            const ConfirmTable &ct = filters[k].confirm;
            d.confirm = ct.enabled;
            d.confirm_walk = d.confirm && ct.has_walk;
        }
    }
    e.n_gated = e.n_gap || e.n_filtered ? kGapLists + e.n_filtered : 0;
    for (size_t k = 0; k < n_groups; k++)
        for (uint32_t c = P.groups[k].atom_base; c < P.groups[k].atom_base + P.groups[k].n_local; c++)
            if (colmask[c]) e.owns_factors[k] = 1;
    for (size_t k = 0; k < n_groups; k++) {
        PassRole &d = e.roles[k];
        if (d.gate >= 0 && !d.filtered) {
            d.visit_slot = d.gate;  // (a gap pass's visited bitmap is indexed by its list slot: enqueueing sets the bit)
            e.n_visit = std::max(e.n_visit, (uint32_t)d.gate + 1u);
        }
        // a plain pass over a field of a few bytes: the streaming DFA kernel's per-request machinery costs more than the walk itself
        const double ml = P.groups[k].field < mean_len.size() ? mean_len[P.groups[k].field] : 0.0;
        if (d.gate < 0 && (P.groups[k].field == PWAF_FIELD_METHOD ? (ml == 0 || ml < 12) : (ml > 0 && ml < 12))) d.identity = true;
    }
    // A pass whose atoms are all anchored literals of <= 8 bytes (`method == "POST"`: the only thing rules ask of the method) is not
    // walked at all: the attribute kernel compares the field's first 8 bytes (one field per engine: the first pass that qualifies).
    for (size_t k = 0; k < n_groups; k++) {
        PassRole &d = e.roles[k];
        const DfaGroup &g = P.groups[k];
        if (d.gate >= 0 || e.owns_factors[k] || g.field >= PWAF_N_FIELDS || e.short_field >= 0 || (P.flags & PWAF_OPT_NO_PREFILTER)) continue;
        std::vector<ShortAtom> mine;
        for (uint32_t l = 0; l < g.atoms.size(); l++) {
            const Atom &at = P.atoms[g.atoms[l]];
            std::string lit;
            bool exact = false;
            if (!at.pattern || !short_literal_atom(*at.pattern, lit, exact)) { mine.clear(); break; }
            uint8_t b[8] = {0};
            memcpy(b, lit.data(), lit.size());
            ShortAtom x{};
            x.col = g.atom_base + l;
            x.len_exact = (uint32_t)lit.size() | (exact ? 0x100u : 0u);
            memcpy(&x.lit_lo, b, 4);
            memcpy(&x.lit_hi, b + 4, 4);
            mine.push_back(x);
        }
        if (mine.empty()) continue;
        d.short_lit = true;
        d.identity = false;
        e.short_field = (int)g.field;
        e.short_atoms = mine;
    }
    e.n_short = (uint32_t)e.short_atoms.size();
    // gap passes whose factors all live in ONE filtered pass walk that pass's candidate list (no atomics, no list of their own)
    for (size_t k = 0; k < n_groups; k++) {
        PassRole &d = e.roles[k];
        if (d.gate < 0 || d.filtered) continue;
        int owner = -1;
        bool single = true;
        for (uint32_t c : P.groups[k].filter_cols) {
            int o = -1;
            for (size_t q = 0; q < n_groups; q++)
                if (c >= P.groups[q].atom_base && c < P.groups[q].atom_base + P.groups[q].n_local) o = (int)q;
            if (o < 0 || (owner >= 0 && o != owner)) single = false;
            owner = o;
        }
        // (an owner with a confirm tier shares its WALK list — a literal hit that calls for a sharing gap pass sends the request through the
        // walk — unless it never walks: then it enqueues)
        if (!single || owner < 0 || !e.roles[owner].filtered || (e.roles[owner].confirm && !e.roles[owner].confirm_walk)) continue;
        d.share_owner = owner;
        e.roles[owner].shared_bits |= 1u << d.gate;
        if (e.roles[owner].need_slot < 0) e.roles[owner].need_slot = (int)e.n_need++;
    }
    // the list-scan launches of every batch (lscan_split.h): per phase, consecutive calls of at most 256 descriptors each
    for (int phase = 0; phase < 2; phase++) {
        std::vector<uint32_t> per_pass(n_groups, 0);
        for (size_t k = 0; k < n_groups; k++) {
            const PassRole &d = e.roles[k];
            const lsplit::PassKind pk{d.identity && !skip_identity, d.gate >= 0, d.filtered, d.confirm, d.confirm_walk, !(P.flags & PWAF_OPT_NO_DENSE_SWITCH)};
            per_pass[k] = lsplit::descriptors(pk, phase);
        }
        e.lscan_launches[phase] = lsplit::split(per_pass.data(), per_pass.size());
    }
    // the verdict kernel's pass table: first column + where the pass's visited bitmap lives
    std::vector<PassInfo> &pt = e.pass_table;
    pt.assign(n_groups + 2, PassInfo{0u, 0u});
    pt[n_groups] = PassInfo{P.fcmp_base, 0u};  // the pseudo pass of the field-against-field atoms (dense records)
    // ... and the one of the residual rules (right after it, or in its place when there are no such atoms)
    // (dense records from the interpreter kernel; none when the specialized program runs: the verdict kernel reads its result words)
    pt[n_groups + (P.fcmp.empty() ? 0u : 1u)] = PassInfo{P.residual_base, residual_specialized ? (3u << 24) : 0u};
    uint32_t fi = 0;
    for (size_t k = 0; k < n_groups; k++) {
        const PassRole &d = e.roles[k];
        pt[k].base = P.groups[k].atom_base;
        if (d.short_lit) {
            pt[k].kind_slot = 3u << 24;  // no records at all
        } else if (d.filtered) {
            // (a pass with heads writes records outside its candidate list too: its records are zeroed and read densely)
            if (filters[k].heads.empty()) pt[k].kind_slot = (1u << 24) | fi;
            fi++;
        } else if (d.visit_slot >= 0) {
            pt[k].kind_slot = (2u << 24) | (uint32_t)d.visit_slot;
        }
    }
}

int tune_host(const Program &P, const pwaf_batch *sample, TuneOut &T) {
    const uint32_t n_fields = PWAF_N_FIELDS + (uint32_t)P.header_names.size();
    const uint32_t n = (uint32_t)std::min<uint64_t>(sample->n, 65536);
    // string column of a field id in the sample (header columns the sample does not carry are left untuned)
    auto sample_col = [&](uint32_t f) -> const pwaf_strcol * {
        if (f < PWAF_N_FIELDS) return &sample->field[f];
        const uint32_t k = f - PWAF_N_FIELDS;
        return (sample->headers && k < sample->n_headers && sample->headers[k].data && sample->headers[k].offsets) ? &sample->headers[k] : nullptr;
    };
    // host walk of every pass over the sample: how often each DFA state is the current state, and for how many requests each
    // pattern holds (patterns that hold for most traffic must not sit behind the bigram prefilter)
    std::vector<std::vector<uint64_t>> &visits = T.visits, &class_freq = T.class_freq;
    std::vector<std::vector<uint64_t>> atom_hits(P.groups.size());
    visits.assign(P.groups.size(), {});
    T.rvisits.assign(P.groups.size(), {});
    class_freq.assign(P.groups.size(), {});
    if (T.filters.size() != P.groups.size()) return fail(PWAF_E_INVALID_ARG, "tune: filters must be pre-filled with the filters in use");
    T.mean_len.assign(n_fields, 0.0);
    T.chunks.assign(P.groups.size(), 0u);  // 0 = the sample does not carry the pass's column: keep
    for (size_t k = 0; k < P.groups.size(); k++) {
        const DfaGroup &g = P.groups[k];
        std::vector<uint64_t> &v = visits[k];
        v.assign(g.n_states, 0);
        std::vector<uint64_t> &cf = class_freq[k];
        cf.assign(256, 0);
        std::vector<uint64_t> &ah = atom_hits[k];
        ah.assign(g.n_local, 0);
        std::vector<uint32_t> stamp(g.n_local, 0);
        const pwaf_strcol *sc = sample_col(g.field);
        if (!sc) continue;
        const uint8_t *data = sc->data;
        const uint32_t *off = sc->offsets;
        for (uint32_t i = 0; i < n; i++) {
            if (off[i + 1] < off[i]) return fail(PWAF_E_BATCH, "sample offsets are not monotonic");
            auto note = [&](const std::vector<uint32_t> &o, const std::vector<uint16_t> &l, uint32_t st) {
                for (uint32_t q = o[st]; q < o[st + 1]; q++)
                    if (stamp[l[q]] != i + 1) { stamp[l[q]] = i + 1; ah[l[q]]++; }
            };
            uint32_t s = 0;
            note(g.emit_off, g.emit_list, s);
            for (uint32_t p = off[i]; p < off[i + 1]; p++) {
                const uint32_t cl = dfa_class_at(g, data + off[i], p - off[i], off[i + 1] - off[i]);  // (scalar mode: the scalar's class at a lead byte)
                cf[cl]++;
                s = g.trans[(size_t)s * g.n_classes + cl];
                v[s]++;
                if (g.emit_off[s + 1] != g.emit_off[s]) note(g.emit_off, g.emit_list, s);
            }
            note(g.end_off, g.end_list, s);
        }
    }
    // bigram prefilters rebuilt for this traffic: window choice and bucketing use the sample's bigram distribution, heads are the
    // anchored literals the sample actually satisfies; a filter that would flag more than 40 % of the sample is dropped (the pass
    // then walks every request, as without a filter)
    if (!(P.flags & PWAF_OPT_NO_PREFILTER)) {
        std::vector<std::vector<double>> pair_prob(n_fields);
        std::vector<double> &mean_len = T.mean_len;
        for (uint32_t f = 0; f < n_fields; f++) {
            const pwaf_strcol *c = sample_col(f);
            pair_prob[f].assign(65536, 0.0);
            if (!c) continue;
            std::vector<uint64_t> cnt(65536, 0);
            uint64_t tot = 0;
            const uint8_t *data = c->data;
            const uint32_t *off = c->offsets;
            for (uint32_t i = 0; i < n; i++)
                for (uint32_t p = off[i]; p + 1 < off[i + 1]; p++) { cnt[filter_fold(data[p]) | (filter_fold(data[p + 1]) << 8)]++; tot++; }
            if (tot)
                for (uint32_t b = 0; b < 65536; b++) pair_prob[f][b] = (double)cnt[b] / (double)tot;
            mean_len[f] = (double)(off[n] - off[0]) / (double)n;
        }
        // (the device samples the bigrams of a stride-2 pass at the even bytes of the ARENA: a field's phase is its offset's parity)
        auto flagged = [&](const GroupFilter &f, const pwaf_strcol *sc, uint32_t i) {
            const uint32_t *off = sc->offsets;
            return filter_candidate_arena(f, sc->data, off[i], off[i + 1], off[n]);  // (the sample's arena carries no slack)
        };
        auto sample_rate = [&](const GroupFilter &f, const pwaf_strcol *sc) {
            uint64_t c = 0;
            for (uint32_t i = 0; i < n; i++) c += flagged(f, sc, i) ? 1u : 0u;
            return (double)c / (double)n;
        };
        // Stride 2 halves the table lookups per byte: a stride-1 pass is bound by them (LDS), a stride-2 pass by HBM. A pass takes it
        // when its factors stay selective with two to four sampled bigrams per alignment: at most two points more of the sample
        // flagged than at stride 1 (a candidate costs about ten times a filtered byte), never above 25 %. Every pass decides for
        // itself: both strides run in ONE launch with their workgroups interleaved (filter.hip: filter_kernel).
        // PWAF_OPT_FILTER_STRIDE2 takes it wherever it can be built.
        std::vector<GroupFilter> alt(P.groups.size());
        for (size_t k = 0; k < P.groups.size(); k++) {
            const DfaGroup &g = P.groups[k];
            FilterHints h;
            h.pair_prob = pair_prob[g.field].data();
            h.atom_hits = &atom_hits[k];
            h.n_requests = n;
            h.mean_len = mean_len[g.field];
            GroupFilter &gf = T.filters[k];
            const pwaf_strcol *sc = sample_col(g.field);
            if (!sc) continue;  // (a pass on a column the sample does not carry keeps the filter it has)
            build_group_filter(P.atoms, g, &h, gf, 1);
            if (!gf.enabled) continue;
            gf.est_candidate_rate = sample_rate(gf, sc);
            GroupFilter &g2 = alt[k];
            build_group_filter(P.atoms, g, &h, g2, 2);
            const bool forced = (P.flags & PWAF_OPT_FILTER_STRIDE2) != 0;
#ifdef PWAF_PROFILING
            static const long s2_mask = getenv("PWAF_STRIDE2_FIELDS") ? strtol(getenv("PWAF_STRIDE2_FIELDS"), nullptr, 0) : -1;  // timing experiments: fields that may take stride 2
            const bool s2_allowed = ((s2_mask >> g.field) & 1) != 0;
#else
            const bool s2_allowed = true;
#endif
            // The pass takes stride 2 when that flags at most two points more of the sample than stride 1 (never above 25 %).
            if (g2.enabled) {
                g2.est_candidate_rate = sample_rate(g2, sc);
                g2.enabled = forced ? g2.est_candidate_rate <= 0.4 : (g2.est_candidate_rate <= gf.est_candidate_rate + 0.02 && g2.est_candidate_rate <= 0.25);
            }
            const double plain_rate = g2.est_candidate_rate;
            const bool plain_ok = g2.enabled;
            // The same pass with EXTENDED windows (filter.cpp, Model::best_window: a window with fewer than four sampled bigrams reaches
            // one bigram beyond its factor on either side, and short windows get buckets of their own). What surrounds a factor in
            // THIS traffic decides whether that pays, so it is measured: a pass that takes stride 2 anyway takes whichever form flags
            // less of the sample; a pass that qualifies ONLY with extended windows (the URL pass of the 1k-rule set: "../" made 34 % of
            // the sample a candidate at stride 2, 2.8 % extended, 1.75 % at stride 1) takes stride 2 only when that costs next to no
            // candidates — measured on MI355X: with the other three arenas at stride 2 the launch is bound by HBM either
            // way (0.607 ms all stride 2, 0.599 ms mixed), while the extra candidates cost the confirm tier 0.09 ms on benign traffic and
            // 2.2 ms on the hostile stream (near misses survive half the bigrams far more often).
            {
                GroupFilter g2x;
                build_group_filter(P.atoms, g, &h, g2x, 2, true);
                if (g2x.enabled) {
                    g2x.est_candidate_rate = sample_rate(g2x, sc);
                    const bool take = forced ? (g2x.est_candidate_rate <= 0.4 && (!plain_ok || g2x.est_candidate_rate < plain_rate))
                                      : plain_ok ? g2x.est_candidate_rate < plain_rate
                                                 : (g2x.est_candidate_rate <= gf.est_candidate_rate * 1.2 + 0.001 && g2x.est_candidate_rate <= 0.25);
#ifdef PWAF_PROFILING
                    if (getenv("PWAF_TUNE_DEBUG")) fprintf(stderr, "[tune] pass %zu field %d: stride 1 flags %.4f of the sample, stride 2 %.4f (%s), with extended windows %.4f (%s)\n", k, g.field, gf.est_candidate_rate, plain_rate, plain_ok ? "ok" : "no", g2x.est_candidate_rate, take ? "taken" : "not taken");
#endif
                    if (take) g2 = std::move(g2x);
                }
            }
            if (!s2_allowed) g2.enabled = false;
#ifdef PWAF_PROFILING
            if (getenv("PWAF_TUNE_DEBUG")) fprintf(stderr, "[tune] pass %zu field %d: stride 1 flags %.4f of the sample (%zu heads), stride 2 %s %.4f, mean field length %.1f%s%s\n", k, g.field, gf.est_candidate_rate, gf.heads.size(), g2.enabled ? "taken:" : "not taken:", g2.est_candidate_rate, mean_len[g.field], g2.note.empty() ? "" : " — ", g2.note.c_str());
#endif
        }
        for (size_t k = 0; k < P.groups.size(); k++) {
            const DfaGroup &g = P.groups[k];
            GroupFilter &gf = T.filters[k];
            const pwaf_strcol *sc = sample_col(g.field);
            if (!sc || !gf.enabled) continue;
            if (alt[k].enabled) gf = alt[k];
            const uint8_t *data = sc->data;
            const uint32_t *off = sc->offsets;
            if (gf.est_candidate_rate > 0.4) {
                gf.enabled = false;
                gf.heads.clear();
                gf.note = "the filter flags more than 40 % of the sample";
                continue;
            }
            // The DFA of a filtered pass only ever walks the filter's candidates, whose states (deep inside pattern prefixes) are
            // not the ones average traffic visits: its LDS-resident rows are chosen from the candidates' walks alone — with a confirm
            // tier, from the walks of the candidates in which a regex factor was CONFIRMED, through the DFA they take (the R tier).
            std::vector<uint64_t> &v = visits[k];
            std::fill(v.begin(), v.end(), 0);
            std::vector<uint64_t> &rv = T.rvisits[k];
            if (g.rtier) rv.assign(g.rtier->n_states, 0);
            std::vector<uint8_t> padded;  // (confirm.h reads a few bytes past a factor: the caller's host arena carries no slack)
            if (gf.confirm.enabled) {
                padded.assign(data, data + off[n]);
                padded.resize(padded.size() + 2 * PWAF_ARENA_PAD, 0);
            }
            std::vector<uint16_t> lits;
            for (uint32_t i = 0; i < n; i++) {
                bool walk;
                if (gf.confirm.enabled) {
                    lits.clear();
                    walk = confirm_field_host(gf, padded.data(), off[i], off[i + 1], lits);
                } else {
                    walk = flagged(gf, sc, i);
                }
                if (!walk) continue;
                uint32_t st = 0;
                for (uint32_t p = off[i]; p < off[i + 1]; p++) {
                    st = g.trans[(size_t)st * g.n_classes + dfa_class_at(g, data + off[i], p - off[i], off[i + 1] - off[i])];
                    v[st]++;
                }
                if (g.rtier) {
                    const DfaGroup &r = *g.rtier;
                    uint32_t rs = 0;
                    for (uint32_t p = off[i]; p < off[i + 1]; p++) {
                        rs = r.trans[(size_t)rs * r.n_classes + dfa_class_at(r, data + off[i], p - off[i], off[i + 1] - off[i])];
                        rv[rs]++;
                    }
                }
            }
        }
    }
    for (size_t k = 0; k < P.groups.size(); k++) {
        const pwaf_strcol *sc = sample_col(P.groups[k].field);
        if (!sc) continue;
        const uint32_t *off = sc->offsets;
        const uint64_t total = (uint64_t)(off[n] - off[0]);
        const uint32_t t4 = 80u, t2 = 48u;  // mean field length from which a lane takes 4 / 2 chunks per iteration (measured)
        T.chunks[k] = total >= (uint64_t)t4 * n ? 4u : total >= (uint64_t)t2 * n ? 2u : 1u;
    }
    return PWAF_OK;
}

// ---- the list scan's launches (scanplan.h) ----
uint32_t list_hot_bytes(const ListShape &shape) { return shape.hot_bytes; }

// LDS budget of the list scan: 160 KiB per CU shared by wg_per_cu workgroups. Default 3 x (48 KiB, 512 threads) = 24 waves per CU;
// PWAF_LIST_SHAPE (profiling builds) tries the others.
ListShape list_shape(uint32_t variant) {
    switch (variant) {
        case 1: return ListShape{512, 72u * 1024u, 2};     // 16 waves per CU, 1.5x the rows
        case 2: return ListShape{1024, 144u * 1024u, 1};   // 16 waves per CU, 3x the rows
        case 3: return ListShape{512, 32u * 1024u, 4};     // 32 waves per CU
        default: return ListShape{kListThreads, kListHotBytes, 3};
    }
}

bool flat_wide(const DfaGroup &g, const GroupFilter &in_use) { return in_use.enabled && g.filter_cols.empty(); }
uint32_t flat_lds_bytes(bool wide) { return list_hot_bytes(list_shape(wide ? 2u : 0u)); }

void build_flat_images(const DfaGroup &g, const GroupFilter &in_use, const uint32_t lds[2], const TuneOut *T, size_t k, FlatImage &full, FlatImage &rtier) {
    build_flat_group(g, lds[flat_wide(g, in_use) ? 1 : 0], full, T ? &T->visits[k] : nullptr);
    rtier = FlatImage();
    if (g.rtier) build_flat_group(*g.rtier, lds[1], rtier, T && !T->rvisits[k].empty() ? &T->rvisits[k] : nullptr);
}

void pick_list_shapes(const std::vector<PassRole> &roles, long forced, ListShape out[2]) {
    uint32_t variant[2] = {2, 0};  // long candidate lists: 1024 threads over 144 KiB of hot rows (measured: benign 0.169 -> 0.143 ms, adversarial 4.43 -> 3.87 ms); short gap lists: 3 x 48 KiB
    // With a confirm tier on every filtered pass the phase-0 lists are short walk lists: the small workgroup shape (512 threads,
    // 48 KiB) starts on whatever wave slots the attribute kernels leave free — the 1024-thread / 144 KiB shape had to wait for a whole
    // free CU (measured: 0.04 ms alone, 0.17 ms beside the side stream).
    bool any_filtered = false, all_confirm = true;
    for (const PassRole &d : roles) {
        any_filtered = any_filtered || d.filtered;
        all_confirm = all_confirm && (!d.filtered || d.confirm);
    }
    if (any_filtered && all_confirm) variant[0] = 0;
    if (forced >= 0) {  // PWAF_LIST_SHAPE, timing experiments (same results): phase 0 | phase 1 << 4
        variant[0] = (uint32_t)forced & 15u;
        variant[1] = (uint32_t)forced >> 4;
    }
    for (int phase = 0; phase < 2; phase++) out[phase] = list_shape(variant[phase]);
}

ListResident list_resident(const FlatShape &F, const ListShape &shape) {
    // rows [0, n_full) and the delta records behind them, when this launch's LDS share holds the layout the tables were built for
    const uint32_t row_bytes = 2u * (F.n_classes + 3u), hb = list_hot_bytes(shape);
    if (F.n_delta && (uint64_t)F.n_full * row_bytes + 48u + 8ull * F.n_delta <= hb) return ListResident{F.n_full, F.n_delta};
    // (states are in visit order: the first rows are the hot ones; 48 bytes stay free for the sentinel cell and lscan_async's dummy record)
    return ListResident{std::min<uint32_t>(F.n_delta ? F.n_full : F.n_states, (hb - 48u) / row_bytes), 0u};
}

// list-driven DFA passes: first those behind a prefilter (they may feed the gap passes' lists), then the gap passes
void plan_list_scans(const std::vector<PassRole> &roles, const std::vector<FlatShape> &full, const std::vector<FlatShape> &rtier, bool dense_switch, bool skip_identity,
                     long forced_shape, ListPlan &out) {
    pick_list_shapes(roles, forced_shape, out.shapes);
    const auto has_dense = [&](size_t k) { return dense_switch && roles[k].filtered && roles[k].confirm; };  // (the pass's FilterArgs carry a dense flag)
    for (int phase = 0; phase < 2; phase++) {
        out.descs[phase].clear();
        for (size_t k = 0; k < roles.size(); k++) {
            const PassRole &d = roles[k];
            if (d.identity ? phase != 0 : (d.gate < 0 || d.filtered != (phase == 0))) continue;
            const bool dense = phase == 0 && d.confirm && has_dense(k);
            const bool owner_dense = d.share_owner >= 0 && has_dense((size_t)d.share_owner);
            ListDesc a;
            a.phase = (uint32_t)phase;
            a.pass = (uint32_t)k;
            a.behind_filter = d.filtered;
            if (d.share_owner >= 0) {
                a.share_owner = d.share_owner;
                a.need_bit = (uint32_t)d.gate;
            }
            if (dense) {
                // the pass's dense alternative: EVERY request through the full table (the whole-pass walk of PWAF_OPT_NO_CONFIRM, over the
                // identity list), records and valid bits written for all; gets work only when the device set the pass's flag
                ListDesc x = a;
                const ListResident r = list_resident(full[k], out.shapes[phase]);
                x.n_hot = r.n_hot;
                x.n_delta = r.n_delta;
                x.dense_mode = 1;
                out.descs[phase].push_back(x);
            }
            if (d.confirm && !d.confirm_walk) continue;  // every atom of the pass is a literal the confirm tier decided: nothing to walk
            if (skip_identity && d.identity) continue;
            a.rtier = d.confirm && rtier[k].n_states != 0;  // (a confirmed candidate walks the DFA of the pass's non-literal atoms)
            a.merge_rec = d.confirm;  // the R-tier walk of a pass with a confirm tier: its list is confirm_kernel's walk list, the walk starts from the record it merged
            const ListResident r = list_resident(a.rtier ? rtier[k] : full[k], out.shapes[phase]);
            a.n_hot = r.n_hot;
            a.n_delta = r.n_delta;
            a.dense_mode = dense ? 2u : owner_dense ? 3u : 0u;  // 2: idle when the pass is walked whole; 3: a gap pass riding the owner's list through need masks
            out.descs[phase].push_back(a);
        }
    }
}

void plan_program_scans(const Program &P, const TuneOut *T, const std::vector<double> &mean_len, ProgramScans &out) {
    const size_t n = P.groups.size();
    out = ProgramScans();
    out.full.resize(n);
    out.rtier.resize(n);
    const uint32_t lds[2] = {flat_lds_bytes(false), flat_lds_bytes(true)};
    std::vector<GroupFilter> filters;
    std::vector<FlatShape> fs, rs;
    for (size_t k = 0; k < n; k++) {
        filters.push_back(T ? T->filters[k] : P.groups[k].filter);
        build_flat_images(P.groups[k], filters[k], lds, T, k, out.full[k], out.rtier[k]);
        out.full_lds.push_back(lds[flat_wide(P.groups[k], filters[k]) ? 1 : 0]);
        out.rtier_lds.push_back(lds[1]);
        fs.push_back(out.full[k]);
        rs.push_back(out.rtier[k]);
    }
    plan_passes(P, filters, mean_len, false, false, out.passes);
    plan_list_scans(out.passes.roles, fs, rs, !(P.flags & PWAF_OPT_NO_DENSE_SWITCH), false, -1, out.lists);
}

}  // namespace pwaf
