// Host planner of the ADMM launch sequence (admm_plan.hip): the workspace carve, the GEMM
// tile lists, the thin units and teams, the search units and the device tables of one
// prepare / run call. Host code only; api.hip snapshots the switches, plans, uploads and
// launches.
// The run's form is decided here too: search_form (exhaustive / per-level / merged stage 1
// and its host tables, shared with the standalone quantizer) and schedule_run (which
// launches a run call makes, as a RunSchedule that admmq_admm_run_ex only follows). Both are
// pure functions of their arguments: tests/test_plan_digest.py pins the plan and
// tests/test_run_schedule.py the schedule (admmq_debug_admm_run_schedule against
// tests/golden/run_schedules.json), without a device.
#pragma once
#include <vector>

#include "../../include/admmq.h"
#include "admmq_internal.h"

namespace admmq {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int rup(int v, int a) { return (v + a - 1) / a * a; }

// Carves the workspace in a fixed order so that size and run agree exactly.
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base(static_cast<char*>(b)) {}
  template <class T>
  T* take(size_t n) {
    off = align_up(off, 256);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
};

// Per-slot quantizer search state of one job.
void carve_view(Carver& cv, MseView& v, int nslot, int ncand);

// The process switches the plan depends on (api.hip snapshots them once per entry-point
// call from the atomics the admmq_debug_set_* functions write). With the problems' shapes,
// num_attempts, the solve mode and the CU count they fix the plan: plan_admm reads no
// other state (its tile memo aside).
struct PlanSwitches {
  int ksplit = 1;         // K-split of the fp32 64 x 64 tiles by the factor's shape: 1 on, 0 never
  int ksplit_form = 1;    // execution form of the pieces: 1 parallel where CUs idle, 0 serial, 2 parallel
  int ksplit_bal = 1;     // parallel pieces for CU balance in launches that fill the chip
  int ksplit_cost = 1;    // ... price of a parallel piece in K-steps
  int f32_kernel = 0;     // fp32 solve kernel: 0 k_gemm, 1 k_gemm_f32p, 2 k_gemm_f32t
  int f32_rule = 1;       // tile rows of kernels 1 / 2 (f32_tile_rows)
  int gemm_stage = 3;     // staging form of the fp32 64 x 64 tiles (2: four resident workgroups per CU)
  int gemm_ks = 1;        // fp32 64 x 64 tiles with 4 (1) or 8 (2) waves
  long long wide_min_tiles = kWideMinTiles;   // 64x64 tiles of a launch from which I > 64 factors go wide
  int even_units = 1;     // big-job stage-1 units sized to fill the resident round evenly
  int fin_nv3 = 1;        // three float4 groups per search thread where that keeps the finalize fused
  int thin_loop = 1;      // persistent thin loop: 2 = 64-column workgroups wherever allowed
  int hist_reps = 0;      // forced stage-1 units per block of the non-fused search (0: planned)
  int launch_head = kLaunchHeadDefault;   // kHead* bits (admmq_internal.h): bit 0 fills the tiles' stop-test pointers
};

// CUs of the chip the device-independent choices are made for (the MI355X's 256): whatever
// moves a factor's bits, the tile memo or the 64 x 64 launch order is planned for this count
// on every device. Choices that may follow the device take plan_admm's `ncu` instead.
constexpr int kPlanChipCUs = 256;

// Where a problem's solve runs (fixed per problem in describe_problems)
enum ProbClass {
  kProbThin,     // I <= kThinRows: the VALU solve of thin_loop.hip
  kProbRows32,   // 17..32 rows: 32 x 64 tiles
  kProbWide,     // kWideRows x 128 tiles (pl.wide, I > 64, no K-split)
  kProbBig       // 64 x 64 tiles (or the f32p / f32t tile rows)
};

struct AdmmPlan {
  std::vector<ProbDesc> desc;
  std::vector<ProbClass> cls;      // per problem
  std::vector<int> order;          // the problems, longest K (ld) first
  std::vector<GemmTile> tiles;
  std::vector<Chunk> sse_chunks, fin_chunks, hist_chunks;
  std::vector<Chunk> hist_multi;   // the same units, several per block (launches without the fused finalize)
  Chunk* d_hist_multi = nullptr;
  int nhm_big = 0;                 // hist_multi blocks of the big jobs (listed first)
  ProbDesc* d_desc = nullptr;
  GemmTile* d_tiles = nullptr;
  Chunk* d_sse = nullptr;
  Chunk* d_fin = nullptr;
  Chunk* d_hist = nullptr;
  bool split = false;            // per-iteration solve on the split fp16 planes (kSolveSplit)
  std::vector<ThinLoopUnit> thin;   // solve workgroups (32 columns each) of the thin (I <= kThinRows) factors
  ThinLoopUnit* d_thin = nullptr;
  int thin_nr = 0, thin_maxld = 0;
  unsigned short* d_rank0 = nullptr;    // merged stage-1 order (kMaxMerged), then the cell index (kCells + 2)
  unsigned short* d_groups = nullptr;   // merged stage-1 tie groups (3 kMaxMerged)
  size_t bytes = 0;
  int maxIp = 0, maxld = 0, maxldm = 0, maxnbk = 0, maxI = 0, maxR = 0;
  int ntiles_wide = 0, ntiles_big = 0, ntiles_small = 0;   // 256x128, 64x64, 32x64 tiles (in that order)
  // persistent fp32 solve (k_gemm_f32p): tiles in list order, workgroup b's list [off[b], off[b+1])
  bool f32p = false;
  bool f32t = false;   // one tile per workgroup, tile rows per problem (k_gemm_f32t)
  std::vector<int> list_off;
  int* d_list_off = nullptr;
  int nslots = 0;
  int ntiles_f32t = 0;
  bool wide = false;                                       // I > 64 factors take 256x128 tiles (k_gemm<8, 1, 3, *, 2>)
  int fin_groups = 1;             // float4 groups per thread of the finalize units
  int hist_nv = 1;
  std::vector<int> small;         // jobs with I <= kThinRows (one-block fused search + finalize)
  int* d_small = nullptr;
  int nfin_big = 0, nhist_big = 0;   // finalize / stage-1 units of the other jobs (listed first)
  bool rows_aligned = true;          // every big job's stage-1 units are whole rows (fused finalize possible)
  unsigned long long* d_ready = nullptr;   // [nprob][2] fused-finalize ready words (zeroed per run)
  unsigned* d_kctr = nullptr;        // K-split arrival counters (zeroed per run)
  size_t nkctr = 0;
  bool ksplit_par = false;           // this launch runs the K-split pieces in parallel (else serially)
  int small_groups = 0;              // float4 groups per thread of the fused kernel (0: too large)
  // persistent thin-factor loop (k_thin_loop, one team of workgroups per problem): possible
  // when every problem is thin, ld <= 1152 and the workgroups fit the CUs (64-column
  // workgroups for some ld <= 512 problems where 32-column ones would not)
  std::vector<ThinLoopUnit> tl_units;
  ThinLoopUnit* d_tl_units = nullptr;
  ThinSync* d_tl_sync = nullptr;
  bool tl_ok = false;
};

// Plans one call against the workspace `ws` (null: sizing only) for a device of `ncu` CUs.
// ADMMQ_OK or an argument error (text recorded).
int plan_admm(const admmq_problem* probs, int nprob, int ncand, void* ws, const PlanSwitches& sw, int solve_mode,
              int ncu, AdmmPlan& pl);

// Fingerprint of a plan's carve (FNV-1a over the byte count, the shapes and the offsets of
// each problem's buffers from the workspace base): equal iff prepare and run lay it out alike
unsigned long long plan_fingerprint(const AdmmPlan& pl, const void* ws);

// Diagnostics (admmq_debug_admm_plan_digest): FNV-1a digests of a plan carved against
// `ws`, one per section, so that a mismatch between two planners says where the plans differ.
void plan_digest(const AdmmPlan& pl, const void* ws, uint64_t out[8]);

// The form of the MSE candidate search for (num_attempts, bits), shared by the ADMM run and
// the standalone quantizer: exhaustive (every candidate's canonical SSE) or two-stage, and
// for the two-stage search the merged-threshold stage 1 with its host tables (rank0 / groups
// as merged_tables writes them, uploaded only when `merged`) or the per-level stage 1.
struct SearchForm {
  bool exhaustive = false;
  bool merged = false;
  std::vector<unsigned short> rank0, groups;
  int ngroups = 0;
};
// merged is false unless qscheme == kMse; force_exhaustive: the process switch
// (admmq_set_exhaustive_search) or a caller that wants every candidate's SSE.
SearchForm search_form(int ncand, int bits, int qscheme, bool force_exhaustive, bool legacy_stage1);

// The process switches a run reads beyond the plan's (api.hip snapshots them once per
// entry-point call; after the snapshot the call reads no atomics).
struct RunSwitches {
  bool exhaustive = false;       // admmq_set_exhaustive_search
  bool legacy_stage1 = false;    // per-level stage 1 instead of merged thresholds
  int thin_loop = 1;             // persistent thin loop: 0 off (the plan's PlanSwitches::thin_loop)
  int fin_cap_override = 0;      // resident-block budget of the fused finalize (0: the device's)
  unsigned fin_wait_polls = kFinWaitPollsDefault;   // polls of the fused paths' bounded waits
};

// The launches of one admmq_admm_run_ex call: what is zeroed before the loop, whether the
// persistent thin loop is tried, and the launches of each of the `iters` iterations in
// stream order (GEMM group, thin solve, search, small jobs, finalize). Host-only and pure:
// tests/test_run_schedule.py pins it through admmq_debug_admm_run_schedule.
enum SearchKind {
  kSearchNone,       // not kMse, or no stage-1 unit outside the small-job kernel
  kSearchHist3,      // merged stage 1, selection and stage 2 in k_mse_hist3
  kSearchHist3Fin,   // ... with the big jobs' finalize fused (one whole-row unit per resident block)
  kSearchHist,       // per-level stage 1 (k_mse_hist)
  kSearchAll         // exhaustive: k_mse_select_all + k_mse_sse
};
struct RunSchedule {
  int iters = 0;                 // per-iteration rounds: max_iter - 1
  bool try_thin_loop = false;    // upload the teams, zero their sync words, try k_thin_loop for all rounds
  bool zero_kctr = false;        // K-split arrival counters
  bool zero_ready = false;       // fused-finalize ready words
  bool gemm = false;             // the GEMM launch group runs ...
  bool gemm_diag = false;        // ... with a diagnostic fp32 kernel (f32p / f32t) in it: event packets
  bool thin_solve = false;
  SearchKind search = kSearchNone;
  bool search_multi = false;     // hist3 reads d_hist_multi (several units per block), else d_hist
  int nh = 0;                    // blocks of the hist3 launch, units of the per-level one
  bool fuse_small = false;       // the small jobs' search and finalize in k_mse_small_admm
  int nf = 0;                    // units of the separate finalize launch (0: none)
  bool fin_wanted = false;       // the fused finalize is possible but for the device's capacity
};
// Whether schedule_run will read `fin_capacity` (hist3_fin_capacity's answer for the device):
// the caller makes that runtime query only then.
bool fin_capacity_wanted(const AdmmPlan& pl, const SearchForm& sf, int qscheme, int ncand, bool fused_allowed);
// fused_allowed: the call may take the paths that report a broken residency assumption
// through info (the fused finalize, the thin loop).
RunSchedule schedule_run(const AdmmPlan& pl, const SearchForm& sf, const RunSwitches& sw, int qscheme, int bits,
                         int ncand, int max_iter, bool fused_allowed, int fin_capacity);

// Pieces per 64 x 64 tile of an (I, R) factor, and how many of a launch's split tiles run
// their pieces in parallel (diagnostic entry points use both)
int ksplit_pieces(int I, int R);
long long ksplit_balance(const std::vector<long long>& whole, std::vector<std::pair<int, int>> cand, int ncu,
                         int slots, int cost);
// Resident 64 x 64 fp32 solve workgroups per CU (the LPT's slots): 3 for the default 3-deep
// staging ring (48 KB of LDS), 4 for the 2-deep ring (k_gemm_f32b<2>, 32 KB, 4 waves per SIMD)
inline int f32_slots(int gemm_stage) { return gemm_stage == 2 ? 4 : 3; }

}  // namespace admmq
