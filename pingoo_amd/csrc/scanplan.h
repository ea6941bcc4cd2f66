// scanplan.h — what the scan kernels READ, decided on the host alone: the streaming table and the list-scan table of every DFA group,
// the role of every pass (gap pass or filtered pass, list slots, sharing owners, identity and short-literal passes) and the host half
// of tuning on a traffic sample (scanplan.cpp). engine.cpp uploads the results. No HIP in here and no environment reads (but the
// PWAF_PROFILING timing switches of tune_host): everything runs, and is tested, without a device (tests/scanplan_host.cpp,
// tests/test_scanplan_cpu.py).
#pragma once
#include <cstdint>
#include <vector>

#include "program.h"

namespace pwaf {

// ---- the streaming table of one DFA group (scan_kernel; kernels.h: the cell encoding) ----
struct ScanShape {  // what the engine keeps beside the uploaded vectors
    uint32_t n_states = 0, stride = 0, n_classes = 0, n_hot = 0, start_emit = 0, emit_base = 0, special_base = 0, atom_base = 0, n_local = 0;
    bool scalar_mode = false;  // the table reads scalar values (dfa.cpp): the class image holds the scalar map behind the byte map
    uint32_t ill_class = 0;
    uint8_t field = 0;
};
struct ScanImage : ScanShape {
    std::vector<uint16_t> tab;          // n_states rows of stride cells, in row order (upload pads it by 16 bytes)
    std::vector<uint8_t> classmap;      // class image (class_image below), classes numbered by their cell position
    std::vector<SpecialCell> special;   // one per cold row (one {0, 0} when there is none)
    std::vector<uint32_t> list_off;     // emit lists first (in state order), then the END lists of more than one atom
    std::vector<uint16_t> list;
};
// `visits` (optional, one count per state) is a traffic profile from tune_host: the LDS-resident ("hot") rows are then the most visited
// states instead of the shallowest ones; `class_freq` (optional) gives the most frequent classes the cell positions without a bank alias.
// The result of a scan never depends on either. PWAF_OK, or PWAF_E_UNSUPPORTED with the reason in pwaf::fail.
int build_device_group(const DfaGroup &g, uint32_t lds_hot_budget, ScanImage &out, const std::vector<uint64_t> *visits = nullptr,
                       const std::vector<uint64_t> *class_freq = nullptr);

// ---- the flat table of one DFA group for list-driven walks (lscan_kernel) ----
struct FlatShape {
    uint32_t n_states = 0, n_classes = 0;  // (n_states == 0: not built)
    bool scalar_mode = false;
    uint32_t ill_class = 0;
    uint32_t n_full = 0, n_delta = 0;  // LDS layout of the list scan: rows [0, n_full), then n_delta 8-byte delta records (states n_full ..)
};
struct FlatImage : FlatShape {
    std::vector<uint16_t> flat;     // next state | 0x8000 when entering it emits; per row an EMIT, a STAY and an END cell behind the classes
    std::vector<uint64_t> delta;    // base row | class 1 << 16 | class 2 << 24 | cell 1 << 32 | cell 2 << 48 (one 0 when there is none)
    std::vector<uint8_t> classmap;  // class image, classes as the DFA numbers them
    std::vector<uint32_t> emit_off, end_off;  // lists indexed by (renumbered) state
    std::vector<uint16_t> emit_list, end_list;
};
// lds_bytes: what the list scan's workgroup shape leaves for hot rows (list_hot_bytes below)
void build_flat_group(const DfaGroup &g, uint32_t lds_bytes, FlatImage &out, const std::vector<uint64_t> *visits = nullptr);

// A table's class lookups on the device: the 256-byte class map of the BYTES, 16 bytes of padding, then — scalar mode — the image of the
// scalar-value map (csrc/utf8.h; classes renumbered like the byte map when the table permutes its columns).
static constexpr size_t kUmapAt = 272;
std::vector<uint8_t> class_image(const DfaGroup &g, const std::vector<uint32_t> *cpos, uint32_t &ill_class);

// ---- the role of every pass ----
struct PassRole {
    int gate = -1;  // >= 0: list-driven pass (behind a bigram prefilter, or gated by prefilter factors): index of its request list
    bool filtered = false;  // the list comes from filter_kernel + compact_kernel
    bool confirm = false;      // the pass's candidates go through confirm_kernel
    bool confirm_walk = false; // ... and those with a confirmed regex factor through the DFA (the R tier if built, else the full one)
    int share_owner = -1;   // a gap pass whose factors all belong to this filtered pass: it walks the owner's list (no list of its own)
    uint32_t shared_bits = 0;  // owner: list bits of the gap passes sharing its list
    int need_slot = -1;     // owner: which need-mask array
    int visit_slot = -1;    // a gap pass: which visited bitmap (its records are valid only where it walked)
    bool identity = false;  // a plain pass over a SHORT field (`method`): walked by the list-scan kernel with the identity list
    bool short_lit = false;  // every atom is an anchored literal of <= 8 bytes: evaluated by the attribute kernel, the pass is never walked
};
struct PassShape {  // what the per-batch code reads of a pass plan besides the roles and the uploaded tables
    uint32_t n_gap = 0;       // gated gap passes (list slots [0, kGapLists), one factor-mask bit each)
    uint32_t n_filtered = 0;  // passes behind a bigram prefilter (one list slot each after the gap passes')
    uint32_t n_gated = 0;     // list slots in use
    uint32_t n_need = 0;      // sharing owners (need-mask arrays per batch)
    uint32_t n_visit = 0;     // gap passes (visited bitmaps per batch)
    std::vector<uint8_t> owns_factors;  // per pass: some of its atoms are prefilter factors of gap passes
    uint32_t n_short = 0;  // short-literal atoms (ShortAtom) of the one field handled that way
    int short_field = -1;
    std::vector<uint32_t> lscan_launches[2];  // per list-scan phase: the descriptors of each launch_scan_gated call (lscan_split.h)
};
struct PassPlan : PassShape {
    std::vector<PassRole> roles;          // per pass
    std::vector<uint32_t> colmask;        // per column: the gap passes (bit = list slot) it is a prefilter factor of
    std::vector<ShortAtom> short_atoms;   // n_short of them
    std::vector<PassInfo> pass_table;     // per pass, then the pseudo passes of the field-against-field atoms and of the residual rules
};
// Decides which passes are list-driven: a pass behind a bigram prefilter walks the filter's candidate list, a gated gap pass the list
// fed by its prefilter factors (owned by earlier passes). filters: the prefilter in use of every pass (the program's, or tune_host's);
// mean_len: per field, from the tuning sample (0 = unknown); residual_specialized: the residual rules run as the specialized program (their
// pseudo pass has no records); skip_identity: timing experiment, the identity passes take no list-scan descriptor.
void plan_passes(const Program &P, const std::vector<GroupFilter> &filters, const std::vector<double> &mean_len, bool residual_specialized, bool skip_identity,
                 PassPlan &out);

// ---- tuning ----
struct TuneOut {
    std::vector<std::vector<uint64_t>> visits, class_freq;
    std::vector<std::vector<uint64_t>> rvisits;  // per pass with an R tier: state visits of the sample's CONFIRMED candidates in that DFA
    std::vector<GroupFilter> filters;  // per pass
    std::vector<double> mean_len;      // per field (0 = the sample does not carry it)
    std::vector<uint32_t> chunks;      // per pass: 16-byte chunks per scan_kernel iteration
};
// The host half of tuning (no device involved): walks every pass over the sample and rebuilds the bigram prefilters for this traffic.
// Shared by pwaf_engine_tune (which then rebuilds the device tables) and pwaf_program_tune (host-only: the tuned filters replace the
// program's, so that the table dump shows them — CPU tests interpret tuned tables without a GPU). T.filters comes pre-filled with the
// filters in use.
int tune_host(const Program &P, const pwaf_batch *sample, TuneOut &T);

// ---- the list scan's launches: what every descriptor of a batch walks, and with what resident in LDS ----
// Workgroup shape of the list scan (lscan_kernel): threads per workgroup, LDS bytes of hot rows per workgroup, workgroups per CU.
static constexpr uint32_t kListThreads = 512;
static constexpr uint32_t kListHotBytes = 48 * 1024;  // 3 workgroups (24 waves) per CU
struct ListShape {
    uint32_t threads, hot_bytes, wg_per_cu;
};
ListShape list_shape(uint32_t variant);  // 0 = default
// LDS bytes for hot rows in a launch of this shape
uint32_t list_hot_bytes(const ListShape &shape);
// The LDS budget a pass's flat tables are BUILT for: the wide shape's for the full table of a pass behind a bigram prefilter (in_use: the
// prefilter in use — the program's, or tune_host's) and for every R tier, the default shape's for the rest.
bool flat_wide(const DfaGroup &g, const GroupFilter &in_use);
uint32_t flat_lds_bytes(bool wide);
// Both flat tables of pass k: of its every atom (full) and — a pass with an R tier — of its non-literal atoms (rtier; n_states 0 when
// there is none). lds: the budgets {narrow, wide}; T: the profile of a tuning sample (null: none).
void build_flat_images(const DfaGroup &g, const GroupFilter &in_use, const uint32_t lds[2], const TuneOut *T, size_t k, FlatImage &full, FlatImage &rtier);
// The shape each phase LAUNCHES with: long candidate lists take 1024 threads over 144 KiB of hot rows, the gap passes' short lists
// 3 x 48 KiB; with a confirm tier on every filtered pass the phase-0 lists are short walk lists and take the small shape too.
// forced >= 0: phase 0 | phase 1 << 4 (timing experiments).
void pick_list_shapes(const std::vector<PassRole> &roles, long forced, ListShape out[2]);
// What a descriptor stages of a table in a launch of `shape`: rows [0, n_hot) and n_delta delta records behind them when the launch's
// LDS share holds the layout the table was built for; else no records and as many of the first rows as fit.
struct ListResident {
    uint32_t n_hot, n_delta;
};
ListResident list_resident(const FlatShape &F, const ListShape &shape);
// One list-scan descriptor of a batch (kernels.h: ListScanArgs, minus the batch's pointers)
struct ListDesc {
    uint32_t phase = 0, pass = 0;
    bool rtier = false;  // walks the pass's R-tier table (else the full one)
    uint32_t n_hot = 0, n_delta = 0;
    bool behind_filter = false, merge_rec = false;
    uint32_t dense_mode = 0;
    int share_owner = -1;  // a gap pass riding this pass's list through need masks (bit need_bit)
    uint32_t need_bit = 0;
};
struct ListPlan {
    ListShape shapes[2];
    std::vector<ListDesc> descs[2];  // per phase, in launch order: first the passes behind a prefilter (and the identity passes), then the gap passes
};
// full / rtier: the shapes of every pass's flat tables; dense_switch: the flag-density switch is on (a pass with a confirm tier also
// gets its dense alternative). The counts per pass are lsplit::descriptors' (PassShape::lscan_launches cuts them into launches).
void plan_list_scans(const std::vector<PassRole> &roles, const std::vector<FlatShape> &full, const std::vector<FlatShape> &rtier, bool dense_switch, bool skip_identity,
                     long forced_shape, ListPlan &out);

// All of the above for a whole program, as an engine created from it (and tuned on T's sample, when given) decides it: no device.
struct ProgramScans {
    std::vector<FlatImage> full, rtier;
    std::vector<uint32_t> full_lds, rtier_lds;  // the budgets the tables were built for
    PassPlan passes;
    ListPlan lists;
};
void plan_program_scans(const Program &P, const TuneOut *T, const std::vector<double> &mean_len, ProgramScans &out);

}  // namespace pwaf
