// C-ABI of libadmmq: workspace planning and stream-ordered launch sequences.
// See include/admmq.h for the contract and the reference interfaces replaced.
// What is left here: the error text, the pinned upload pool, the profiling marks, the process
// switches with their setters and per-call snapshots (plan_switches, run_switches), the
// workspace records, the standalone quantizer's plan and launches (QPlan, run_quant) and the
// entry points, which validate, plan, upload and launch. What a call carves, which form its
// search takes and which launches a run makes are decided in admm_plan.hip (plan_admm,
// search_form, schedule_run): admmq_admm_run_ex only follows the schedule.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "../../include/admmq.h"
#include "admmq_internal.h"
#include "admm_plan.h"

namespace admmq {

static thread_local std::string g_err;

static int fail(int code, const char* msg) {
  g_err = msg;
  return code;
}
int set_error(int code, const char* msg) { return fail(code, msg); }

static int check_hip(const char* where) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    g_err = std::string(where) + ": " + hipGetErrorString(e);
    return ADMMQ_ERR_HIP;
  }
  return ADMMQ_OK;
}

// Host -> device uploads of the plans (descriptors, tile and unit lists) through pinned
// staging chunks, so that hipMemcpyAsync is truly asynchronous: a pageable source makes
// the copy wait for the stream, which put every call's host planning on the GPU's
// critical path (the host could not run ahead of the device by one mode call). A chunk
// is reused once the event recorded after its copy has completed; one pool per device -
// the device the STREAM belongs to (the event must be on it), not the caller's current
// one. The pool is capped by bytes (kPinMaxBytes per device): when every chunk that could
// hold the plan is still in flight and the cap is reached, the plan goes up by a plain
// pageable hipMemcpyAsync instead (HIP stages a pageable source before it returns, so the
// host buffer may be reused at once; that copy may wait for the stream - the only case in
// which an entry point can block, include/admmq.h), never by waiting on a chunk's event.
struct PinnedChunk { char* p; size_t cap; hipEvent_t ev; bool used; };
static std::mutex g_pin_mu;
static std::vector<PinnedChunk> g_pin[64];
static size_t g_pin_bytes[64];
static constexpr size_t kPinMaxBytes = size_t(64) << 20;
int upload_async(void* dst, const void* src, size_t n, hipStream_t s) {
  if (n == 0) return ADMMQ_OK;
  int dev = -1;
  if (hipStreamGetDevice(s, &dev) != hipSuccess) {
    (void)hipGetLastError();
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  }
  if (dev < 0 || dev >= 64) dev = 0;
  std::lock_guard<std::mutex> g(g_pin_mu);
  std::vector<PinnedChunk>& pool = g_pin[dev];
  PinnedChunk* c = nullptr;
  for (PinnedChunk& k : pool)
    if (k.cap >= n && (!k.used || hipEventQuery(k.ev) == hipSuccess)) { c = &k; break; }
  size_t cap = 4096;
  while (cap < n) cap *= 2;
  if (!c && g_pin_bytes[dev] + cap > kPinMaxBytes) {   // pool full and busy: pageable copy
    const hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
      g_err = std::string("upload (pageable): ") + hipGetErrorString(e);
      return ADMMQ_ERR_HIP;
    }
    return ADMMQ_OK;
  }
  if (!c) {
    PinnedChunk k;
    k.cap = cap;
    k.used = false;
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (cur != dev) (void)hipSetDevice(dev);   // the event (and the chunk's mapping) on the stream's device
    const hipError_t ea = hipHostMalloc(reinterpret_cast<void**>(&k.p), k.cap, hipHostMallocDefault);
    const hipError_t ee = ea == hipSuccess ? hipEventCreateWithFlags(&k.ev, hipEventDisableTiming) : ea;
    if (cur != dev && cur >= 0) (void)hipSetDevice(cur);
    if (ea != hipSuccess) {
      (void)hipGetLastError();
      g_err = "upload: pinned staging allocation failed";
      return ADMMQ_ERR_HIP;
    }
    if (ee != hipSuccess) {
      (void)hipHostFree(k.p);
      g_err = "upload: event creation failed";
      return ADMMQ_ERR_HIP;
    }
    pool.push_back(k);
    g_pin_bytes[dev] += k.cap;
    c = &pool.back();
  }
  std::memcpy(c->p, src, n);
  hipError_t e = hipMemcpyAsync(dst, c->p, n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipEventRecord(c->ev, s);
  c->used = true;
  if (e != hipSuccess) {
    g_err = std::string("upload: ") + hipGetErrorString(e);
    return ADMMQ_ERR_HIP;
  }
  return ADMMQ_OK;
}
static int h2d(void* dst, const void* src, size_t n, hipStream_t s) { return upload_async(dst, src, n, s); }

// Optional per-launch HIP-event timing (bench.py measures the dominant kernel live on
// the stream it runs on). Events are created in admmq_profile_begin, never in a launch path.
struct Prof {
  bool on = false;
  std::vector<hipEvent_t> ev;
  std::vector<int> cls;
  size_t next = 0;
  int every = 1;        // time one ADMM iteration in `every` (events add inter-kernel gaps)
  bool sampled = true;  // the current iteration is timed
};
static Prof g_prof;
// Process-wide switches (atomics: set from any thread, read by the launch sequences).
// exhaustive: evaluate all candidates (reference-style) instead of the two-stage search;
// legacy stage 1: the per-level stage-1 form instead of merged thresholds (same integers);
// solve mode: the process default (kSolveF32: the reference's fp32 arithmetic; kSolveSplit
// opt-in) of the plain entry points, read once at prepare and recorded per workspace.
static std::atomic<bool> g_exhaustive{false};
static std::atomic<bool> g_legacy_stage1{false};
static std::atomic<int> g_solve_mode{kSolveF32};
// fused finalize (k_mse_hist3<.., true>) where the residency check allows it; 0: the
// separate k_finalize_admm launch (A/B and cross-check, same integers)
static std::atomic<bool> g_fused_finalize{true};
// stage-1 units per block of the non-fused search launch (0: sized by the planner)
static std::atomic<int> g_hist_reps{0};
// polls of the fused finalize's bounded wait for its job's selection (diagnostics can
// shrink it to force the timeout path)
static std::atomic<unsigned> g_fin_wait_polls{kFinWaitPollsDefault};
// diagnostics: a smaller resident-block budget for the fused finalize (0: the device's),
// to exercise its several-units-per-block form on small batches
static std::atomic<int> g_fin_cap_override{0};
static std::atomic<int> g_fin_nv3{1};   // diagnostics: 0 = never three float4 groups per search thread
// persistent loop of the thin factors (k_thin_loop) for calls whose problems are all
// thin: 1 on, 0 off (the per-iteration launches: A/B and cross-check), 2 on with 64-column
// workgroups wherever allowed (exercises that form on batches that fit without it)
static std::atomic<int> g_thin_loop{1};

// fp32 solve kernel: 0 = k_gemm (64 x 64 tiles), 1 = persistent tile lists (k_gemm_f32p,
// slower: DESIGN §7), 2 = one tile per workgroup with per-problem tile rows (k_gemm_f32t);
// and the tile-row rule of kernels 1 / 2 (admm_plan.hip f32_tile_rows)
static std::atomic<int> g_f32_kernel{0};
static std::atomic<int> g_f32_rule{1};
static std::atomic<int> g_even_units{1};   // big-job stage-1 units sized to fill the resident round evenly
// K-split of the fp32 64 x 64 solve tiles (admm_plan.hip ksplit_pieces): 1 = by the factor's
// shape, 0 = never (A/B)
static std::atomic<int> g_ksplit{1};
// 64x64 tiles of a launch from which its I > 64 factors without a K-split take the 256x128
// tiles (default kWideMinTiles; diagnostics: admmq_debug_set_wide_min_tiles; same bits)
static std::atomic<long long> g_wide_min_tiles{kWideMinTiles};
// execution form of the pieces (same bits either way): 1 = parallel only where the 64 x 64
// launch's whole tiles leave CUs idle, else serial (default); 0 = always serial; 2 = always parallel
static std::atomic<int> g_ksplit_par{1};
// Balance (admm_plan.hip ksplit_balance): on / off, and the price of a parallel piece in K-steps
static std::atomic<int> g_ksplit_bal{1};
static std::atomic<int> g_ksplit_cost{1};
// Launch-head forms (admmq_internal.h kHead* bits; same bits either way)
static std::atomic<int> g_launch_head{kLaunchHeadDefault};

// The planner's inputs among the switches, read once per entry-point call
static PlanSwitches plan_switches() {
  PlanSwitches sw;
  sw.ksplit = g_ksplit.load();
  sw.ksplit_form = g_ksplit_par.load();
  sw.ksplit_bal = g_ksplit_bal.load();
  sw.ksplit_cost = g_ksplit_cost.load();
  sw.f32_kernel = g_f32_kernel.load();
  sw.f32_rule = g_f32_rule.load();
  sw.gemm_stage = g_gemm_f32_stage;
  sw.gemm_ks = g_gemm_ks_f32;
  sw.wide_min_tiles = g_wide_min_tiles.load();
  sw.even_units = g_even_units.load();
  sw.fin_nv3 = g_fin_nv3.load();
  sw.thin_loop = g_thin_loop.load();
  sw.hist_reps = g_hist_reps.load();
  sw.launch_head = g_launch_head.load();
  return sw;
}
// The run's inputs among the switches, read once per entry-point call. thin_loop: the
// value the call's plan was made with (one view of the switch for the plan and the run;
// the standalone quantizer does not read it).
static RunSwitches run_switches(int thin_loop = 1) {
  RunSwitches sw;
  sw.exhaustive = g_exhaustive.load();
  sw.legacy_stage1 = g_legacy_stage1.load();
  sw.thin_loop = thin_loop;
  sw.fin_cap_override = g_fin_cap_override.load();
  sw.fin_wait_polls = g_fin_wait_polls.load();
  return sw;
}

// CUs of the current device (looked up once per device)
static int device_cus() {
  constexpr int kMaxDev = 64;
  static std::once_flag once[kMaxDev];
  static int cus[kMaxDev];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return 256;
  std::call_once(once[dev], [dev]() {
    int n = 0;
    cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
  });
  return cus[dev];
}

// What each prepare recorded for its workspace: the solve mode (the run must use the operand
// planes its prepare wrote) and a fingerprint of the carve - the problem shapes, the byte
// count and every process switch that moves buffers (tile rows, stage-1 unit sizing,
// K-split) - so a run whose plan would carve the workspace differently is refused instead of
// reading another layout. Keyed by address: a workspace freed and reallocated at the same
// address for the same problems still needs its own prepare (include/admmq.h).
struct WsRecord { int mode; unsigned long long fp; };
static std::mutex g_ws_mu;
static std::unordered_map<const void*, WsRecord> g_ws_rec;
static void record_ws(const void* ws, int mode, unsigned long long fp) {
  std::lock_guard<std::mutex> g(g_ws_mu);
  g_ws_rec[ws] = {mode, fp};
}
static bool recorded_ws(const void* ws, WsRecord& out) {
  std::lock_guard<std::mutex> g(g_ws_mu);
  auto it = g_ws_rec.find(ws);
  if (it == g_ws_rec.end()) return false;
  out = it->second;
  return true;
}
static int recorded_ws_mode(const void* ws) {
  WsRecord r;
  return recorded_ws(ws, r) ? r.mode : -1;
}

static inline void prof_mark(hipStream_t s) {
  if (!g_prof.on || !g_prof.sampled || g_prof.next >= g_prof.ev.size()) return;
  (void)hipEventRecord(g_prof.ev[g_prof.next++], s);
}
static inline void prof_class(int c) {
  if (g_prof.on && g_prof.sampled && g_prof.next < g_prof.ev.size()) g_prof.cls.push_back(c);
}
// The event pair of one sampled launch of class c, for a launcher that has its dispatches
// record them (hipExtLaunchKernelGGL: start of the kernel, end of the kernel), so the
// measured time is the kernel's own, as rocprofv3 reports it, without the dispatch gap an
// event packet between two kernels opens. Null events when not sampled.
static inline void prof_pair(int c, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (!g_prof.on || !g_prof.sampled || g_prof.next + 2 > g_prof.ev.size()) return;
  g_prof.cls.push_back(c);
  *e0 = g_prof.ev[g_prof.next++];
  *e1 = g_prof.ev[g_prof.next++];
}

static int upload_admm(const AdmmPlan& pl, hipStream_t s) {
  int rc;
  if ((rc = h2d(pl.d_desc, pl.desc.data(), pl.desc.size() * sizeof(ProbDesc), s))) return rc;
  if ((rc = h2d(pl.d_tiles, pl.tiles.data(), pl.tiles.size() * sizeof(GemmTile), s))) return rc;
  if (!pl.list_off.empty() && (rc = h2d(pl.d_list_off, pl.list_off.data(), pl.list_off.size() * sizeof(int), s)))
    return rc;
  if ((rc = h2d(pl.d_sse, pl.sse_chunks.data(), pl.sse_chunks.size() * sizeof(Chunk), s))) return rc;
  if ((rc = h2d(pl.d_fin, pl.fin_chunks.data(), pl.fin_chunks.size() * sizeof(Chunk), s))) return rc;
  if ((rc = h2d(pl.d_hist, pl.hist_chunks.data(), pl.hist_chunks.size() * sizeof(Chunk), s))) return rc;
  if ((rc = h2d(pl.d_hist_multi, pl.hist_multi.data(), pl.hist_multi.size() * sizeof(Chunk), s))) return rc;
  if (!pl.thin.empty() && (rc = h2d(pl.d_thin, pl.thin.data(), pl.thin.size() * sizeof(ThinLoopUnit), s))) return rc;
  if (!pl.small.empty() && (rc = h2d(pl.d_small, pl.small.data(), pl.small.size() * sizeof(int), s))) return rc;
  return check_hip("upload");
}

// The merged stage-1 tables of a search form (nothing unless merged; groups only when there are any)
static int upload_search_tables(const SearchForm& sf, unsigned short* d_rank0, unsigned short* d_groups, hipStream_t s) {
  int rc;
  if (!sf.merged) return ADMMQ_OK;
  if ((rc = h2d(d_rank0, sf.rank0.data(), sf.rank0.size() * 2, s))) return rc;
  if (!sf.groups.empty() && (rc = h2d(d_groups, sf.groups.data(), sf.groups.size() * 2, s))) return rc;
  return ADMMQ_OK;
}

__global__ void k_export_info(const ProbDesc* __restrict__ d, int n, int32_t* info) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    info[4 * i + 0] = d[i].flags[1];
    info[4 * i + 1] = d[i].flags[0];
    info[4 * i + 2] = d[i].flags[2];
    info[4 * i + 3] = d[i].flags[3];   // internal fault (fused-finalize wait timed out)
  }
}

// ---------------------------------------------------------------------------
// Standalone quantization
struct QPlan {
  std::vector<QJob> jobs;
  std::vector<Chunk> pack_chunks, stat_chunks, sse_chunks, hist_chunks;
  QJob* d_jobs = nullptr;
  Chunk* d_pack = nullptr;
  Chunk* d_stat = nullptr;
  Chunk* d_sse = nullptr;
  Chunk* d_hist = nullptr;
  unsigned short* d_rank0 = nullptr;    // merged stage-1 order (kMaxMerged), then the cell index (kCells + 2)
  unsigned short* d_groups = nullptr;   // merged stage-1 tie groups (3 kMaxMerged)
  size_t bytes = 0;
};

static int plan_quant(const admmq_qtensor* t, int n, int ncand, void* ws, QPlan& pl) {
  if (n <= 0 || !t) return fail(ADMMQ_ERR_ARG, "no tensors");
  if (ncand < 1) return fail(ADMMQ_ERR_ARG, "num_attempts must be >= 1");
  Carver cv(ws);
  pl.jobs.resize(n);
  for (int i = 0; i < n; ++i) {
    QJob& j = pl.jobs[i];
    std::memset(&j, 0, sizeof(j));
    if (t[i].rows <= 0 || t[i].cols <= 0) return fail(ADMMQ_ERR_ARG, "empty tensor");
    j.src = t[i].x; j.dst = t[i].y;
    j.rows = (int)t[i].rows; j.cols = (int)t[i].cols;
    j.ld = rup(j.cols, 4);
    if ((long long)j.rows * j.ld >= (1LL << 31)) return fail(ADMMQ_ERR_ARG, "tensor too large");
    j.nq = j.rows * (j.ld / 4);
    j.has_kw = t[i].has_minmax; j.tmin_kw = t[i].tmin; j.tmax_kw = t[i].tmax;
    j.Xp = cv.take<float>((size_t)j.rows * j.ld);   // (carved either way: the size does not depend on src)
    j.copy = !(j.cols % 4 == 0 && (reinterpret_cast<uintptr_t>(j.src) & 15) == 0);
    if (!j.copy) j.Xp = const_cast<float*>(j.src);   // read in place (only k_qpack's copy writes Xp)
    carve_view(cv, j.mv, 1, ncand);
    j.mv.X = j.Xp; j.mv.rows = j.rows; j.mv.cols = j.cols; j.mv.ld = j.ld; j.mv.qpr = j.ld / 4;
    j.mv.nq = j.nq; j.mv.nelem = j.rows * j.cols; j.mv.done = nullptr;
  }
  pl.pack_chunks.clear();
  pl.stat_chunks.clear();
  pl.sse_chunks.clear();
  pl.hist_chunks.clear();
  for (int i = 0; i < n; ++i) {
    const QJob& j = pl.jobs[i];
    const long long tot = (long long)j.rows * j.ld;
    for (long long e = 0; e < tot; e += kElemChunk) pl.pack_chunks.push_back({i, (int)e});
    pl.jobs[i].pu0 = (int)pl.stat_chunks.size();
    for (long long e = 0; e < tot; e += kPackElems) pl.stat_chunks.push_back({i, (int)e});
    pl.jobs[i].pun = (int)pl.stat_chunks.size() - pl.jobs[i].pu0;
    for (int q = 0; q < j.nq; q += kSseQuads) pl.sse_chunks.push_back({i, q});
    for (long long e = 0; e < tot; e += kHistElems) pl.hist_chunks.push_back({i, (int)e, j.mv.stat, nullptr, j.Xp, nullptr, tot});
    pl.jobs[i].mv.nhist = (int)((tot + kHistElems - 1) / kHistElems);
  }
  pl.d_jobs = cv.take<QJob>(n);
  pl.d_pack = cv.take<Chunk>(pl.pack_chunks.size());
  pl.d_stat = cv.take<Chunk>(pl.stat_chunks.size());
  for (int i = 0; i < n; ++i) pl.jobs[i].pstat = cv.take<unsigned>(3 * (size_t)pl.jobs[i].pun);
  pl.d_sse = cv.take<Chunk>(pl.sse_chunks.size());
  pl.d_hist = cv.take<Chunk>(pl.hist_chunks.size());
  pl.d_rank0 = cv.take<unsigned short>(kMaxMerged + kCells + 2);
  pl.d_groups = cv.take<unsigned short>(3 * kMaxMerged);
  pl.bytes = align_up(cv.off, 256);
  return ADMMQ_OK;
}

__global__ void k_qinit(QJob* jobs, int n, int ncand) {
  const MseView& v = jobs[blockIdx.x].mv;
  for (int c = threadIdx.x; c < ncand; c += blockDim.x) v.sse[c] = 0ull;
  for (int c = threadIdx.x; c < kHistRep * (ncand + 1); c += blockDim.x) { v.h1[c] = 0ull; v.h2[c] = 0ull; }
  if (threadIdx.x == 0) {
    v.stat[0] = 0u; v.stat[1] = 0xFFFFFFFFu; v.stat[2] = 0u; v.stat[3] = 0u;
    v.s2[0] = 0.0;
    v.ticket[0] = 0u;
  }
}

__global__ void k_copy_sse(const QJob* jobs, int ncand, unsigned long long* out) {
  for (int c = threadIdx.x; c < ncand; c += blockDim.x) out[c] = jobs[0].mv.sse[c];
}

// sw.exhaustive: evaluate every candidate's canonical SSE (debug table / forced mode)
// pack (optional): the final pass emits packed codes (k_qfinal_pack) instead of k_qfinal
struct PackOut {
  unsigned char* const* host_codes;   // n device pointers (host array)
  unsigned char** d_codes;            // their device copy (workspace)
  admmq_qmeta* meta;                  // device, n entries
};
static int run_quant(QPlan& pl, int n, int bits, int qscheme, int ncand, hipStream_t s, bool final_pass,
                     const RunSwitches& sw, const PackOut* pack = nullptr) {
  int rc;
  if (pack) {
    if ((rc = h2d(pack->d_codes, pack->host_codes, n * sizeof(unsigned char*), s))) return rc;
    if (hipMemsetAsync(pack->meta, 0, n * sizeof(admmq_qmeta), s) != hipSuccess) return check_hip("quantize_packed");
  }
  if ((rc = h2d(pl.d_jobs, pl.jobs.data(), n * sizeof(QJob), s))) return rc;
  if ((rc = h2d(pl.d_pack, pl.pack_chunks.data(), pl.pack_chunks.size() * sizeof(Chunk), s))) return rc;
  if ((rc = h2d(pl.d_stat, pl.stat_chunks.data(), pl.stat_chunks.size() * sizeof(Chunk), s))) return rc;
  if ((rc = h2d(pl.d_sse, pl.sse_chunks.data(), pl.sse_chunks.size() * sizeof(Chunk), s))) return rc;
  if ((rc = h2d(pl.d_hist, pl.hist_chunks.data(), pl.hist_chunks.size() * sizeof(Chunk), s))) return rc;
  hipLaunchKernelGGL(k_qinit, dim3(n), dim3(256), 0, s, pl.d_jobs, n, ncand);
  launch_qpack(pl.d_jobs, n, pl.d_stat, (int)pl.stat_chunks.size(), s);
  if (qscheme == kMse) {
    const SearchForm sf = search_form(ncand, bits, qscheme, sw.exhaustive, sw.legacy_stage1);
    if ((rc = upload_search_tables(sf, pl.d_rank0, pl.d_groups, s))) return rc;
    if (sf.merged) {
      if ((rc = launch_mse_hist3(nullptr, pl.d_jobs, pl.d_hist, (int)pl.hist_chunks.size(), ncand, bits, 0, pl.d_rank0,
                                 pl.d_groups, sf.ngroups, 1, false, 0, 0u, s)))
        return rc;
    } else if (!sf.exhaustive) {
      launch_mse_hist(nullptr, pl.d_jobs, pl.d_hist, (int)pl.hist_chunks.size(), ncand, bits, 0, 1, s);
    } else {   // exhaustive: every candidate's canonical SSE over all chunks
      launch_mse_select_all(nullptr, pl.d_jobs, n, ncand, 0, s);
      launch_mse_sse(nullptr, pl.d_jobs, pl.d_sse, (int)pl.sse_chunks.size(), ncand, bits, 0, s);
    }
  }
  if (final_pass && pack) {
    static_assert(kHistElems == 4 * kElemChunk, "k_qfinal_pack's unit sizes");
    if ((int)pl.hist_chunks.size() >= kPackMinUnits)   // enough 4096-element units to fill the chip
      launch_qfinal_pack(pl.d_jobs, pl.d_hist, (int)pl.hist_chunks.size(), 4, pack->d_codes, pack->meta, ncand, bits,
                         qscheme, s);
    else
      launch_qfinal_pack(pl.d_jobs, pl.d_pack, (int)pl.pack_chunks.size(), 1, pack->d_codes, pack->meta, ncand, bits,
                         qscheme, s);
  } else if (final_pass)
    launch_qfinal(pl.d_jobs, pl.d_pack, (int)pl.pack_chunks.size(), ncand, bits, qscheme, s);
  return check_hip("quantize");
}

}  // namespace admmq

using namespace admmq;

static int valid_scheme(int q) { return q >= 0 && q <= 3; }
static int valid_bits(int b) { return b >= 1 && b <= 16; }

static const int g_gemm_stage_env = [] {
  const char* e = std::getenv("ADMMQ_GEMM_F32_STAGE");
  if (e && *e >= '0' && *e <= '4' && e[1] == 0) g_gemm_f32_stage = *e - '0';
  const char* u = std::getenv("ADMMQ_EVEN_UNITS");   // diagnostics: 0 = kHistElems x nv stage-1 units
  if (u && u[0] == '0' && u[1] == 0) g_even_units = 0;
  const char* fc = std::getenv("ADMMQ_FIN_CAPACITY");   // diagnostics: admmq_debug_set_fin_capacity
  if (fc) g_fin_cap_override = std::atoi(fc);
  return 0;
}();

extern "C" {

int32_t admmq_version(void) { return 100; }

int32_t admmq_set_exhaustive_search(int32_t enable) {
  g_exhaustive = enable != 0;
  return ADMMQ_OK;
}

int32_t admmq_set_solve_mode(int32_t mode) {
  if (mode != kSolveF32 && mode != kSolveSplit) return fail(ADMMQ_ERR_ARG, "solve mode must be 0 (fp32) or 1 (split)");
  g_solve_mode = mode;
  return ADMMQ_OK;
}

int32_t admmq_get_solve_mode(void) { return g_solve_mode.load(); }

// diagnostics (not in include/admmq.h): 1 (default) = finalize fused into the search
// launch where its blocks are all resident, 0 = the separate finalize launch
// diagnostics: stage-1 units per block of the non-fused search launch (0 = planner's choice)
int32_t admmq_debug_set_search_units_per_block(int32_t reps) {
  if (reps < 0 || reps > 64) return fail(ADMMQ_ERR_ARG, "units per block out of range");
  g_hist_reps = reps;
  return ADMMQ_OK;
}

int32_t admmq_debug_set_fused_finalize(int32_t enable) {
  g_fused_finalize = enable != 0;
  return ADMMQ_OK;
}

// diagnostics (not in include/admmq.h): workspace bytes of the plan carved against a
// non-null base (no memory is touched), so a test can check that sizing (null base)
// and the real carve agree
size_t admmq_debug_admm_plan_bytes(const admmq_problem* probs, int32_t nprob, int32_t num_attempts, void* base) {
  AdmmPlan pl;
  if (plan_admm(probs, nprob, num_attempts, base, plan_switches(), g_solve_mode.load(), device_cus(), pl) != ADMMQ_OK) return 0;
  return pl.bytes;
}

// diagnostics (not in include/admmq.h): eight per-section digests of the plan that
// admmq_admm_prepare_ex would build with workspace = base (plan_digest; `base` is never
// dereferenced), so a test can pin the planner's output
int32_t admmq_debug_admm_plan_digest(const admmq_problem* probs, int32_t nprob, int32_t num_attempts,
                                     int32_t solve_mode, void* base, uint64_t out[8]) {
  if (!out || !base) return fail(ADMMQ_ERR_ARG, "plan digest: base and out must not be NULL");
  if (solve_mode != kSolveF32 && solve_mode != kSolveSplit) return fail(ADMMQ_ERR_ARG, "solve mode must be 0 (fp32) or 1 (split)");
  AdmmPlan pl;
  const int rc = plan_admm(probs, nprob, num_attempts, base, plan_switches(), solve_mode, device_cus(), pl);
  if (rc) return rc;
  plan_digest(pl, base, out);
  return ADMMQ_OK;
}

// diagnostics (not in include/admmq.h): 1 (default) = the search takes three float4 groups
// per thread where that keeps the finalize fused (planned at prepare), 0 = at most two
int32_t admmq_debug_set_fin_nv3(int32_t on) {
  if (on < 0 || on > 1) return fail(ADMMQ_ERR_ARG, "fin_nv3 must be 0 or 1");
  g_fin_nv3 = on;
  return ADMMQ_OK;
}

// diagnostics (not in include/admmq.h): resident-block budget of the fused finalize (0: the device's)
int32_t admmq_debug_set_fin_capacity(int32_t blocks) {
  if (blocks < 0) return fail(ADMMQ_ERR_ARG, "blocks must be >= 0");
  g_fin_cap_override = blocks;
  return ADMMQ_OK;
}

// diagnostics (not in include/admmq.h): the persistent thin-factor loop on / off / on with
// 64-column workgroups wherever allowed
int32_t admmq_debug_set_thin_loop(int32_t on) {
  if (on < 0 || on > 2) return fail(ADMMQ_ERR_ARG, "thin_loop: 0, 1 or 2");
  g_thin_loop = on;
  return ADMMQ_OK;
}

// diagnostics (not in include/admmq.h): polls of the fused finalize's bounded wait
// (default kFinWaitPollsDefault; a test sets 1 to force the timeout / internal-fault path)
int32_t admmq_debug_set_fin_wait_polls(uint32_t polls) {
  g_fin_wait_polls = polls ? polls : kFinWaitPollsDefault;
  return ADMMQ_OK;
}

// diagnostics (not in include/admmq.h): waves per fp32 64 x 64 solve tile: 1 = four waves of
// 32 x 32 (default), 2 = eight, each pair splitting a sub-tile's K-step (other bits)
int32_t admmq_debug_set_gemm_ks(int32_t ks) {
  if (ks != 1 && ks != 2) return fail(ADMMQ_ERR_ARG, "ks must be 1 or 2");
  g_gemm_ks_f32 = ks;
  return ADMMQ_OK;
}

// diagnostics (not in include/admmq.h): 1 (default) = the big jobs' stage-1 units sized to fill
// the resident round evenly, 0 = kHistElems x nv units
int32_t admmq_debug_set_even_units(int32_t on) {
  g_even_units = on != 0;
  return ADMMQ_OK;
}

// diagnostics (not in include/admmq.h): kernel of the fp32 64 x 64 tiles (same bits):
// 0 = k_gemm<2, 1, 3, false> (buffer loads to LDS from two descriptors chosen per piece,
// U prefetched), 1 = k_gemm_f32b (one wave-uniform descriptor per wave, U prefetched),
// 2 = k_gemm_f32b with a 2-deep ring, 3 = k_gemm_f32b without the U prefetch (the default:
// C3 mode 0 0.655 -> 0.597 us per 64x64 K-step per CU against 0), 4 = 3 with the waves'
// MFMA bursts at raised issue priority (s_setprio). ADMMQ_GEMM_F32_STAGE sets it at load time.
int32_t admmq_debug_set_gemm_stage(int32_t v) {
  if (v < 0 || v > 4) return fail(ADMMQ_ERR_ARG, "stage must be 0..4");
  g_gemm_f32_stage = v;
  return ADMMQ_OK;
}

// diagnostics (not in include/admmq.h): K-split of the fp32 64 x 64 solve tiles by the
// factor's shape (1, default) or never (0; changes the bits of the factors that split)
int32_t admmq_debug_set_ksplit(int32_t on) {
  if (on < 0 || on > 1) return fail(ADMMQ_ERR_ARG, "ksplit must be 0 or 1");
  g_ksplit = on;
  return ADMMQ_OK;
}
// diagnostics: execution form of the K-split pieces (same bits): 1 = parallel where the launch
// leaves CUs idle (default), 0 = always serial (one workgroup per tile), 2 = always parallel
int32_t admmq_debug_set_ksplit_form(int32_t form) {
  if (form < 0 || form > 2) return fail(ADMMQ_ERR_ARG, "ksplit form must be 0..2");
  g_ksplit_par = form;
  return ADMMQ_OK;
}
// diagnostics: parallel pieces for CU balance in launches that fill the chip (same bits):
// on / off, and the price of a parallel piece in K-steps
int32_t admmq_debug_set_ksplit_balance(int32_t on, int32_t cost) {
  if (on < 0 || on > 1 || cost < 0 || cost > 64) return fail(ADMMQ_ERR_ARG, "ksplit balance: on 0/1, cost 0..64");
  g_ksplit_bal = on;
  g_ksplit_cost = cost;
  return ADMMQ_OK;
}
// diagnostics: the parallel-piece count the balance picks for the 64 x 64 tiles of a batch
// of (I, R) factors (fp32 form, default switches), or -1 on bad arguments
int64_t admmq_debug_ksplit_balance_count(const int32_t* IR, int32_t nprob) {
  if (!IR || nprob <= 0) return -1;
  std::vector<long long> whole;
  std::vector<std::pair<int, int>> cand;
  for (int p = 0; p < nprob; ++p) {
    const int I = IR[2 * p], R = IR[2 * p + 1];
    if (I <= 32) continue;
    const int ld = rup(R, 32), np = ksplit_pieces(I, R);
    const long long nt = (long long)((I + 63) / 64) * ((ld + 63) / 64);
    for (long long t = 0; t < nt; ++t) {
      whole.push_back(ld / 32);
      if (np > 1) cand.push_back({ld / 32, np});
    }
  }
  return ksplit_balance(whole, cand, kPlanChipCUs, f32_slots(g_gemm_f32_stage), g_ksplit_cost.load());
}
// diagnostics: the wide-tile threshold (64x64 tiles per launch; default 4 x 768)
int32_t admmq_debug_set_wide_min_tiles(int64_t t) {
  if (t < 0) return fail(ADMMQ_ERR_ARG, "wide min tiles must be >= 0");
  g_wide_min_tiles = t;
  return ADMMQ_OK;
}
// diagnostics: keep every candidate in the selected set S (1), S plus the two candidates either
// side of the first stage-1 minimum (2: the list form, 1 < |S| <= kMaxSel) or the rigorous
// set (0, default): the multi-candidate paths run every time, with the same exact answer
int32_t admmq_debug_set_sel_widen(int32_t on) {
  if (on < 0 || on > 2) return fail(ADMMQ_ERR_ARG, "sel widen must be 0, 1 or 2");
  if (set_sel_widen_search(on) != 0 || set_sel_widen_thin(on) != 0) return check_hip("sel widen");
  return ADMMQ_OK;
}
// diagnostics: the K-split pieces the planner gives an (I, R) factor (0 on bad arguments)
int32_t admmq_debug_ksplit_pieces(int32_t I, int32_t R) {
  if (I <= 0 || R <= 0) return 0;
  return ksplit_pieces(I, R);
}

// diagnostics (not in include/admmq.h): persistent fp32 solve on/off and its tile rule
// (f32_tile_rows; changes the bits of the factors whose tile rows change between 64 and 32)
int32_t admmq_debug_set_f32_persistent(int32_t kernel, int32_t rule) {
  if (rule < 0 || rule > 3) return fail(ADMMQ_ERR_ARG, "rule must be 0..3");
  if (kernel < 0 || kernel > 2) return fail(ADMMQ_ERR_ARG, "kernel must be 0..2");
  g_f32_kernel = kernel;
  g_f32_rule = rule;
  return ADMMQ_OK;
}

// diagnostics (not in include/admmq.h): which launch heads take their first loads off the
// descriptor chain (kHead* bits, admmq_internal.h; default kLaunchHeadDefault, 0 = the
// descriptor-chain heads; same bits either way)
int32_t admmq_debug_set_launch_head(int32_t mask) {
  if (mask < 0 || (mask & ~kLaunchHeadAll)) return fail(ADMMQ_ERR_ARG, "launch head mask out of range");
  g_launch_head = mask;
  return ADMMQ_OK;
}
int32_t admmq_debug_get_launch_head_default(void) { return kLaunchHeadDefault; }

// diagnostics (not in include/admmq.h): 1 = per-level stage 1, 0 = merged thresholds
int32_t admmq_debug_set_legacy_stage1(int32_t enable) {
  g_legacy_stage1 = enable != 0;
  return ADMMQ_OK;
}

int32_t admmq_profile_begin(int32_t max_launches, int32_t sample_every) {
  if (g_prof.on) return fail(ADMMQ_ERR_ARG, "profiling already active");
  if (sample_every < 1) return fail(ADMMQ_ERR_ARG, "sample_every must be >= 1");
  g_prof.every = sample_every;
  g_prof.sampled = true;
  g_prof.ev.resize(2 * (size_t)std::max(max_launches, 1));
  for (auto& e : g_prof.ev)
    if (hipEventCreate(&e) != hipSuccess) return fail(ADMMQ_ERR_HIP, "hipEventCreate");
  g_prof.cls.clear();
  g_prof.next = 0;
  g_prof.on = true;
  return ADMMQ_OK;
}

int32_t admmq_profile_end(double* ms_per_class, int64_t* launches_per_class) {
  if (!g_prof.on) return fail(ADMMQ_ERR_ARG, "profiling not active");
  g_prof.on = false;
  g_prof.sampled = true;
  for (int c = 0; c < ADMMQ_PROF_CLASSES; ++c) { ms_per_class[c] = 0.0; launches_per_class[c] = 0; }
  const size_t pairs = std::min(g_prof.next / 2, g_prof.cls.size());
  int rc = ADMMQ_OK;
  if (pairs > 0 && hipEventSynchronize(g_prof.ev[2 * pairs - 1]) != hipSuccess) rc = fail(ADMMQ_ERR_HIP, "sync");
  for (size_t i = 0; rc == ADMMQ_OK && i < pairs; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) { rc = ADMMQ_ERR_HIP; break; }
    ms_per_class[g_prof.cls[i]] += ms;
    launches_per_class[g_prof.cls[i]] += 1;
  }
  for (auto& e : g_prof.ev) (void)hipEventDestroy(e);
  g_prof.ev.clear();
  g_prof.cls.clear();
  return rc;
}

const char* admmq_last_error(void) { return g_err.c_str(); }

static int check_opts(const admmq_admm_options* o) {
  if (!o) return fail(ADMMQ_ERR_ARG, "options must not be NULL");
  if (o->solve_mode != kSolveF32 && o->solve_mode != kSolveSplit)
    return fail(ADMMQ_ERR_ARG, "solve_mode must be ADMMQ_SOLVE_FP32 or ADMMQ_SOLVE_SPLIT");
  if (o->fused_finalize != 0 && o->fused_finalize != 1) return fail(ADMMQ_ERR_ARG, "fused_finalize must be 0 or 1");
  for (int r : o->reserved)
    if (r != 0) return fail(ADMMQ_ERR_ARG, "reserved option fields must be zero");
  return ADMMQ_OK;
}
static admmq_admm_options default_opts() {
  admmq_admm_options o;
  std::memset(&o, 0, sizeof(o));
  o.solve_mode = g_solve_mode.load();
  o.fused_finalize = g_fused_finalize.load() ? 1 : 0;
  return o;
}

int32_t admmq_admm_default_options(admmq_admm_options* out) {
  if (!out) return fail(ADMMQ_ERR_ARG, "options must not be NULL");
  *out = default_opts();
  return ADMMQ_OK;
}

size_t admmq_admm_workspace_size_ex(const admmq_problem* probs, int32_t nprob, int32_t num_attempts,
                                    const admmq_admm_options* opt) {
  if (check_opts(opt)) return 0;
  AdmmPlan pl;
  if (plan_admm(probs, nprob, num_attempts, nullptr, plan_switches(), opt->solve_mode, device_cus(), pl) != ADMMQ_OK) return 0;
  return pl.bytes;
}

size_t admmq_admm_workspace_size(const admmq_problem* probs, int32_t nprob, int32_t num_attempts) {
  const admmq_admm_options o = default_opts();
  return admmq_admm_workspace_size_ex(probs, nprob, num_attempts, &o);
}

int32_t admmq_admm_prepare_ex(const admmq_problem* probs, int32_t nprob, int32_t num_attempts,
                              const admmq_admm_options* opt, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_opts(opt);
  if (rc) return rc;
  AdmmPlan pl;
  rc = plan_admm(probs, nprob, num_attempts, workspace, plan_switches(), opt->solve_mode, device_cus(), pl);
  if (rc) return rc;
  if (!workspace || workspace_bytes < pl.bytes) return fail(ADMMQ_ERR_WORKSPACE, "workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = upload_admm(pl, s))) return rc;
  prof_class(ADMMQ_PROF_PREPARE); prof_mark(s);
  launch_rho(pl.d_desc, nprob, s);
  launch_pack(pl.d_desc, nprob, pl.maxIp, pl.maxld, s);
  launch_fill_a64(pl.d_desc, nprob, pl.maxldm, s);
  launch_spd_inverse(pl.d_desc, nprob, pl.maxnbk, s);
  if (pl.split) {   // fp16 planes of M and of the first right-hand side P
    launch_split_rows(pl.d_desc, nprob, pl.maxldm, 1, s);
    launch_split_rows(pl.d_desc, nprob, pl.maxIp, 0, s);
  }
  prof_mark(s);
  if ((rc = check_hip("admm_prepare"))) return rc;
  record_ws(workspace, opt->solve_mode, plan_fingerprint(pl, workspace));
  return ADMMQ_OK;
}

int32_t admmq_admm_prepare(const admmq_problem* probs, int32_t nprob, int32_t num_attempts, void* workspace,
                           size_t workspace_bytes, void* stream) {
  const admmq_admm_options o = default_opts();
  return admmq_admm_prepare_ex(probs, nprob, num_attempts, &o, workspace, workspace_bytes, stream);
}

// The per-call arguments the launches of an iteration share
struct RunArgs {
  int nprob, bits, qscheme, ncand;
  float eps;
  unsigned polls;
};

// One iteration's launches as the schedule lists them, one event pair per launch (classes:
// include/admmq.h, admmq_profile_end). ADMMQ_OK, or a search launcher's refusal (nothing
// more is launched).
static int run_iteration(const AdmmPlan& pl, const RunSchedule& rs, const SearchForm& sf, const RunArgs& a, int it,
                         hipStream_t s) {
  const int slot = it & 1;
  int rc;
  if (rs.gemm) {
    hipEvent_t g0 = nullptr, g1 = nullptr;
    // the diagnostic fp32 kernels: event packets
    if (rs.gemm_diag) { prof_class(ADMMQ_PROF_GEMM); prof_mark(s); } else { prof_pair(ADMMQ_PROF_GEMM, &g0, &g1); }
    if (pl.ntiles_wide + pl.ntiles_small + pl.ntiles_big > 0)
      launch_gemm(pl.d_desc, pl.d_tiles, pl.ntiles_wide, pl.ntiles_small, pl.ntiles_big, pl.split, slot, it, a.eps,
                  a.ncand, s, g0, g1, pl.ksplit_par);
    if (pl.nslots > 0)
      launch_gemm_f32p(pl.d_desc, pl.d_tiles + pl.ntiles_wide, pl.d_list_off, pl.nslots, slot, it, a.eps, a.ncand, s);
    if (pl.ntiles_f32t > 0)
      launch_gemm_f32t(pl.d_desc, pl.d_tiles + pl.ntiles_wide, pl.ntiles_f32t, slot, it, a.eps, a.ncand, s);
    if (rs.gemm_diag) prof_mark(s);
  }
  if (rs.thin_solve) {
    prof_class(ADMMQ_PROF_GEMM_THIN); prof_mark(s);
    launch_thin_solve(pl.d_desc, pl.d_thin, (int)pl.thin.size(), pl.thin_nr, pl.thin_maxld, slot, it, a.eps, a.ncand, s);
    prof_mark(s);
  }
  if (rs.search == kSearchHist3 || rs.search == kSearchHist3Fin) {
    hipEvent_t h0, h1;
    prof_pair(ADMMQ_PROF_SEARCH, &h0, &h1);
    if ((rc = launch_mse_hist3(pl.d_desc, nullptr, rs.search_multi ? pl.d_hist_multi : pl.d_hist, rs.nh, a.ncand, a.bits,
                               slot, pl.d_rank0, pl.d_groups, sf.ngroups, pl.hist_nv, rs.search == kSearchHist3Fin, it,
                               a.polls, s, h0, h1)))
      return rc;
  } else if (rs.search != kSearchNone) {
    prof_class(ADMMQ_PROF_SEARCH); prof_mark(s);
    if (rs.search == kSearchHist) {
      launch_mse_hist(pl.d_desc, nullptr, pl.d_hist, rs.nh, a.ncand, a.bits, slot, pl.hist_nv, s);
    } else {
      launch_mse_select_all(pl.d_desc, nullptr, a.nprob, a.ncand, slot, s);
      launch_mse_sse(pl.d_desc, nullptr, pl.d_sse, (int)pl.sse_chunks.size(), a.ncand, a.bits, slot, s);
    }
    prof_mark(s);
  }
  if (rs.fuse_small) {
    prof_class(ADMMQ_PROF_SMALL); prof_mark(s);
    if ((rc = launch_mse_small_admm(pl.d_desc, pl.d_small, (int)pl.small.size(), pl.small_groups, a.ncand, a.bits, slot,
                                    it, pl.d_rank0, pl.d_groups, sf.ngroups, s)))
      return rc;
    prof_mark(s);
  }
  if (rs.nf > 0) {
    prof_class(ADMMQ_PROF_FINALIZE); prof_mark(s);
    launch_finalize_admm(pl.d_desc, pl.d_fin, rs.nf, pl.fin_groups, a.ncand, a.bits, a.qscheme, slot, it, s);
    prof_mark(s);
  }
  return ADMMQ_OK;
}

int32_t admmq_admm_run_ex(const admmq_problem* probs, int32_t nprob, int32_t max_iter, float eps, int32_t bits,
                          int32_t qscheme, int32_t num_attempts, const admmq_admm_options* opt, void* workspace,
                          size_t workspace_bytes, int32_t* info, void* stream) {
  int rc = check_opts(opt);
  if (rc) return rc;
  if (!valid_scheme(qscheme)) return fail(ADMMQ_ERR_SCHEME, "unknown qscheme");
  if (!valid_bits(bits)) return fail(ADMMQ_ERR_ARG, "bits out of range");
  WsRecord wr;
  if (!recorded_ws(workspace, wr))
    return fail(ADMMQ_ERR_ARG, "admm_run: the workspace has not been prepared (admmq_admm_prepare)");
  const int rec = wr.mode;
  if (rec != opt->solve_mode) return fail(ADMMQ_ERR_ARG, "admm_run: solve_mode differs from the one its prepare used");
  const PlanSwitches psw = plan_switches();
  const RunSwitches sw = run_switches(psw.thin_loop);
  AdmmPlan pl;
  rc = plan_admm(probs, nprob, num_attempts, workspace, psw, rec, device_cus(), pl);
  if (rc) return rc;
  if (!workspace || workspace_bytes < pl.bytes) return fail(ADMMQ_ERR_WORKSPACE, "workspace too small");
  if (plan_fingerprint(pl, workspace) != wr.fp)
    return fail(ADMMQ_ERR_ARG, "admm_run: the problems or layout switches differ from the workspace's prepare");
  // which launches the call makes (admm_plan.hip): host code only, but for the resident-block
  // query of the fused finalize, made only where the schedule reads its answer
  const SearchForm sf = search_form(num_attempts, bits, qscheme, sw.exhaustive, sw.legacy_stage1);
  // the fused paths report a broken residency assumption only through info: without it
  // they never run (include/admmq.h)
  const bool fused_allowed = opt->fused_finalize != 0 && info != nullptr;
  const int fin_capacity = fin_capacity_wanted(pl, sf, qscheme, num_attempts, fused_allowed)
                               ? hist3_fin_capacity(num_attempts, bits, pl.hist_nv) : 0;
  const RunSchedule rs = schedule_run(pl, sf, sw, qscheme, bits, num_attempts, max_iter, fused_allowed, fin_capacity);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // descriptors carry this call's output pointers (H_out may differ from prepare's)
  if ((rc = upload_admm(pl, s))) return rc;
  if (rs.zero_kctr && hipMemsetAsync(pl.d_kctr, 0, pl.nkctr * sizeof(unsigned), s) != hipSuccess)
    return check_hip("K-split counter reset");
  if ((rc = upload_search_tables(sf, pl.d_rank0, pl.d_groups, s))) return rc;
  if (rs.zero_ready && hipMemsetAsync(pl.d_ready, 0, 2 * (size_t)nprob * sizeof(unsigned long long), s) != hipSuccess)
    return check_hip("ready reset");
  const RunArgs a{nprob, bits, qscheme, num_attempts, eps, sw.fin_wait_polls};
  bool loop_done = false;
  if (rs.try_thin_loop) {
    if ((rc = h2d(pl.d_tl_units, pl.tl_units.data(), pl.tl_units.size() * sizeof(ThinLoopUnit), s))) return rc;
    if (hipMemsetAsync(pl.d_tl_sync, 0, (size_t)nprob * sizeof(ThinSync), s) != hipSuccess)
      return check_hip("thin loop reset");
    g_prof.sampled = true;
    prof_class(ADMMQ_PROF_THIN_LOOP); prof_mark(s);
    loop_done = launch_thin_loop(pl.d_desc, pl.d_tl_units, (int)pl.tl_units.size(), pl.d_tl_sync, pl.thin_nr, pl.thin_maxld,
                                 rs.iters, eps, num_attempts, bits, a.polls, device_cus(), s) == 0;
    prof_mark(s);
  }
  for (int it = 0; !loop_done && it < rs.iters; ++it) {
    g_prof.sampled = it % g_prof.every == 0;
    if ((rc = run_iteration(pl, rs, sf, a, it, s))) return rc;
  }
  g_prof.sampled = true;
  if (max_iter > 1) launch_unpack(pl.d_desc, nprob, pl.maxI, pl.maxR, s);
  if (info) hipLaunchKernelGGL(k_export_info, dim3((nprob + 63) / 64), dim3(64), 0, s, pl.d_desc, nprob, info);
  return check_hip("admm_run");
}

int32_t admmq_admm_run(const admmq_problem* probs, int32_t nprob, int32_t max_iter, float eps, int32_t bits,
                       int32_t qscheme, int32_t num_attempts, void* workspace, size_t workspace_bytes,
                       int32_t* info, void* stream) {
  admmq_admm_options o = default_opts();
  const int rec = recorded_ws_mode(workspace);   // the mode this workspace was prepared with
  if (rec >= 0) o.solve_mode = rec;
  return admmq_admm_run_ex(probs, nprob, max_iter, eps, bits, qscheme, num_attempts, &o, workspace, workspace_bytes,
                           info, stream);
}

// diagnostics (not in include/admmq.h): the launch schedule admmq_admm_run_ex would follow
// for these problems under the current switches, planned against a fake workspace address
// (never dereferenced). fused_finalize: the option; has_info: whether the call passes an
// info array; fin_capacity: the resident blocks of the fused search kernel, so that the
// answer does not depend on the machine (negative: ask the current device, and only where the
// run would). out, one field of SearchForm / RunSchedule (admm_plan.h) per slot:
//   0 iters            1 try_thin_loop    2 zero_kctr     3 zero_ready
//   4 gemm (0 none, 1 the launch group, 2 with a diagnostic fp32 kernel in it)
//   5 thin_solve       6 search (SearchKind)
//   7 search list (0 d_hist, 1 d_hist_multi)              8 nh
//   9 fuse_small      10 nf              11 exhaustive   12 merged
//  13 ngroups         14 fin_wanted      15 the plan's finalize units
int32_t admmq_debug_admm_run_schedule(const admmq_problem* probs, int32_t nprob, int32_t num_attempts, int32_t bits,
                                      int32_t qscheme, int32_t max_iter, int32_t solve_mode, int32_t fused_finalize,
                                      int32_t has_info, int32_t fin_capacity, int32_t out[16]) {
  if (!out) return fail(ADMMQ_ERR_ARG, "run schedule: out must not be NULL");
  if (solve_mode != kSolveF32 && solve_mode != kSolveSplit) return fail(ADMMQ_ERR_ARG, "solve mode must be 0 (fp32) or 1 (split)");
  if (!valid_scheme(qscheme)) return fail(ADMMQ_ERR_SCHEME, "unknown qscheme");
  if (!valid_bits(bits)) return fail(ADMMQ_ERR_ARG, "bits out of range");
  const PlanSwitches psw = plan_switches();
  const RunSwitches sw = run_switches(psw.thin_loop);
  AdmmPlan pl;
  const int rc = plan_admm(probs, nprob, num_attempts, reinterpret_cast<void*>(uintptr_t(1) << 20), psw, solve_mode,
                           device_cus(), pl);
  if (rc) return rc;
  const SearchForm sf = search_form(num_attempts, bits, qscheme, sw.exhaustive, sw.legacy_stage1);
  const bool fused_allowed = fused_finalize != 0 && has_info != 0;
  if (fin_capacity < 0)
    fin_capacity = fin_capacity_wanted(pl, sf, qscheme, num_attempts, fused_allowed)
                       ? hist3_fin_capacity(num_attempts, bits, pl.hist_nv) : 0;
  const RunSchedule rs = schedule_run(pl, sf, sw, qscheme, bits, num_attempts, max_iter, fused_allowed, fin_capacity);
  const int32_t slots[16] = {rs.iters, rs.try_thin_loop, rs.zero_kctr, rs.zero_ready, rs.gemm ? (rs.gemm_diag ? 2 : 1) : 0,
                             rs.thin_solve, rs.search, rs.search_multi, rs.nh, rs.fuse_small, rs.nf, sf.exhaustive,
                             sf.merged, sf.ngroups, rs.fin_wanted, (int32_t)pl.fin_chunks.size()};
  std::copy(slots, slots + 16, out);
  return ADMMQ_OK;
}

// diagnostics (not in include/admmq.h): per-block timelines of the last launches (make TRACE=1)
int32_t admmq_debug_hist_trace(unsigned long long* host, int32_t n) { return copy_hist_trace(host, n); }
int32_t admmq_debug_gemm_trace(unsigned long long* host, int32_t n) { return copy_gemm_trace(host, n); }
int32_t admmq_debug_gemm_trace2(unsigned long long* host, int32_t n) { return copy_gemm_trace2(host, n); }
int32_t admmq_debug_gemm_trace3(unsigned long long* host, int32_t n) { return copy_gemm_trace3(host, n); }
int32_t admmq_debug_gemm_simd(unsigned* host, int32_t n) { return copy_gemm_simd(host, n); }
int32_t admmq_debug_setup_trace(unsigned long long* host, int32_t n) { return copy_setup_trace(host, n); }
int32_t admmq_debug_fin_trace(unsigned long long* host, int32_t n) { return copy_fin_trace(host, n); }
int32_t admmq_debug_hist_cu(unsigned long long* host, int32_t n) { return copy_hist_cu(host, n); }
int32_t admmq_debug_small_trace(unsigned long long* host, int32_t n) { return copy_small_trace(host, n); }
int32_t admmq_debug_thin_loop_trace(unsigned long long* host, int32_t n) { return copy_thin_loop_trace(host, n); }
int32_t admmq_debug_sel_stats(unsigned long long* host, int32_t reset) { return copy_sel_stats(host, reset); }
// diagnostics: multi-candidate selections whose stage 2 the fused search launch shared among
// the job's blocks, since the last reset (reset != 0 zeroes the counter); -1 on a HIP error
int64_t admmq_debug_shared_stage2_count(int32_t reset) { return copy_shared_stage2(reset); }
int32_t admmq_debug_check_thresholds(uint32_t seed, int32_t nsamp) { return check_thresholds(seed, nsamp); }
int32_t admmq_debug_check_cells(int32_t n, int32_t bits, uint32_t seed, int32_t nsamp, uint32_t* maxdev) {
  return check_cells(n, bits, seed, nsamp, maxdev);
}

int32_t admmq_admm_iteration_batched(const admmq_problem* probs, int32_t nprob, int32_t max_iter, float eps,
                                     int32_t bits, int32_t qscheme, int32_t num_attempts, void* workspace,
                                     size_t workspace_bytes, int32_t* info, void* stream) {
  int rc = admmq_admm_prepare(probs, nprob, num_attempts, workspace, workspace_bytes, stream);
  if (rc) return rc;
  return admmq_admm_run(probs, nprob, max_iter, eps, bits, qscheme, num_attempts, workspace, workspace_bytes, info,
                        stream);
}

// (A, C, B) around the channel dim and the broadcast output shape (outer x Lo); false:
// invalid arguments (error recorded)
static bool channel_geometry(const int64_t* shape, int32_t ndim, int32_t dim, long long& A, int& C, long long& B,
                             long long& outer, int& L, int& Lo) {
  if (!shape || ndim < 1 || ndim > 16) { fail(ADMMQ_ERR_ARG, "channel quantization needs 1 <= ndim <= 16"); return false; }
  if (dim < -ndim || dim >= ndim) { fail(ADMMQ_ERR_ARG, "dim out of range"); return false; }
  const int d = dim < 0 ? dim + ndim : dim;
  A = 1; B = 1;
  for (int k = 0; k < ndim; ++k) {
    if (shape[k] <= 0) { fail(ADMMQ_ERR_ARG, "empty tensor"); return false; }
    if (k < d) A *= shape[k];
    if (k > d) B *= shape[k];
  }
  if (shape[d] > (1 << 30) || A * B * shape[d] > (1LL << 40)) { fail(ADMMQ_ERR_ARG, "tensor too large"); return false; }
  C = (int)shape[d];
  L = (int)shape[ndim - 1];
  if (L != C && L != 1 && C != 1) {
    fail(ADMMQ_ERR_ARG, "the channel statistics do not broadcast against the last dimension");
    return false;
  }
  Lo = std::max(L, C);
  outer = A * B * C / L;
  return true;
}

size_t admmq_quantize_channel_workspace_size(const int64_t* shape, int32_t ndim, int32_t dim) {
  long long A, B, outer;
  int C, L, Lo;
  if (!channel_geometry(shape, ndim, dim, A, C, B, outer, L, Lo)) return 0;
  return align_up((size_t)3 * C * sizeof(unsigned), 256);
}

int32_t admmq_quantize_channel(const float* x, float* y, const int64_t* shape, int32_t ndim, int32_t dim, int32_t bits,
                               int32_t qscheme, void* workspace, size_t workspace_bytes, void* stream) {
  if (qscheme != ADMMQ_CHANNEL_SYMMETRIC && qscheme != ADMMQ_CHANNEL_AFFINE)
    return fail(ADMMQ_ERR_SCHEME, "qscheme must be ADMMQ_CHANNEL_SYMMETRIC or ADMMQ_CHANNEL_AFFINE");
  if (!valid_bits(bits) || bits > 31) return fail(ADMMQ_ERR_ARG, "bits out of range");
  if (!x || !y) return fail(ADMMQ_ERR_ARG, "null tensor");
  long long A, B, outer;
  int C, L, Lo;
  if (!channel_geometry(shape, ndim, dim, A, C, B, outer, L, Lo)) return ADMMQ_ERR_ARG;
  if (!workspace || workspace_bytes < (size_t)3 * C * sizeof(unsigned)) return fail(ADMMQ_ERR_WORKSPACE, "workspace too small");
  launch_channel_quant(x, y, A, C, B, outer, L, Lo, static_cast<unsigned*>(workspace), bits,
                       qscheme == ADMMQ_CHANNEL_SYMMETRIC ? kSymmetric : kAffine, static_cast<hipStream_t>(stream));
  return check_hip("quantize_channel");
}

size_t admmq_quantize_workspace_size(const admmq_qtensor* t, int32_t n, int32_t num_attempts) {
  QPlan pl;
  if (plan_quant(t, n, num_attempts, nullptr, pl) != ADMMQ_OK) return 0;
  return pl.bytes;
}

int32_t admmq_quantize_batched(const admmq_qtensor* t, int32_t n, int32_t bits, int32_t qscheme, int32_t num_attempts,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!valid_scheme(qscheme)) return fail(ADMMQ_ERR_SCHEME, "unknown qscheme");
  if (!valid_bits(bits)) return fail(ADMMQ_ERR_ARG, "bits out of range");
  QPlan pl;
  int rc = plan_quant(t, n, num_attempts, workspace, pl);
  if (rc) return rc;
  if (!workspace || workspace_bytes < pl.bytes) return fail(ADMMQ_ERR_WORKSPACE, "workspace too small");
  return run_quant(pl, n, bits, qscheme, num_attempts, static_cast<hipStream_t>(stream), true, run_switches());
}

size_t admmq_packed_bytes(int64_t numel, int32_t bits) {
  if (numel <= 0 || bits < 1 || bits > 8 || numel > (int64_t(1) << 56)) return 0;
  return (size_t)((numel * bits + 7) / 8);
}

// the quantize plan, then the device copy of the code pointers
static size_t packed_codes_offset(const QPlan& pl) { return align_up(pl.bytes, 256); }

size_t admmq_quantize_packed_workspace_size(const admmq_qtensor* t, int32_t n, int32_t num_attempts) {
  QPlan pl;
  if (plan_quant(t, n, num_attempts, nullptr, pl) != ADMMQ_OK) return 0;
  return align_up(packed_codes_offset(pl) + (size_t)n * sizeof(unsigned char*), 256);
}

int32_t admmq_quantize_packed(const admmq_qtensor* t, uint8_t* const* codes, admmq_qmeta* meta_dev, int32_t n,
                              int32_t bits, int32_t qscheme, int32_t num_attempts, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (!valid_scheme(qscheme)) return fail(ADMMQ_ERR_SCHEME, "quantize_packed: unknown qscheme (the four tensor schemes only)");
  if (bits < 1 || bits > 8) return fail(ADMMQ_ERR_ARG, "quantize_packed: bits must be 1..8");
  if (qscheme == kMinMax && bits == 1)
    return fail(ADMMQ_ERR_ARG, "quantize_packed: tensor_minmax with 1 bit has three output values; no 1-bit code");
  if (!codes || !meta_dev) return fail(ADMMQ_ERR_ARG, "quantize_packed: codes and meta must not be NULL");
  QPlan pl;
  int rc = plan_quant(t, n, num_attempts, workspace, pl);
  if (rc) return rc;
  for (int i = 0; i < n; ++i) {
    if (!t[i].x) return fail(ADMMQ_ERR_ARG, "quantize_packed: null tensor");
    if (!codes[i] || (reinterpret_cast<uintptr_t>(codes[i]) & 15) != 0)
      return fail(ADMMQ_ERR_ARG, "quantize_packed: every codes[i] must be a 16-byte aligned device pointer");
  }
  const size_t off = packed_codes_offset(pl);
  if (!workspace || workspace_bytes < align_up(off + (size_t)n * sizeof(unsigned char*), 256))
    return fail(ADMMQ_ERR_WORKSPACE, "workspace too small");
  PackOut po{codes, reinterpret_cast<unsigned char**>(static_cast<char*>(workspace) + off), meta_dev};
  return run_quant(pl, n, bits, qscheme, num_attempts, static_cast<hipStream_t>(stream), true, run_switches(), &po);
}

int32_t admmq_dequantize_packed(const uint8_t* const* codes, const admmq_qmeta* meta_dev, float* const* y,
                                const int64_t* numel, int32_t n, void* stream) {
  if (n <= 0 || !codes || !meta_dev || !y || !numel) return fail(ADMMQ_ERR_ARG, "dequantize_packed: null argument");
  for (int i = 0; i < n; ++i) {
    if (!codes[i] || !y[i]) return fail(ADMMQ_ERR_ARG, "dequantize_packed: null tensor");
    if ((reinterpret_cast<uintptr_t>(codes[i]) & 15) != 0)
      return fail(ADMMQ_ERR_ARG, "dequantize_packed: every codes[i] must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(y[i]) & 3) != 0) return fail(ADMMQ_ERR_ARG, "dequantize_packed: y[i] must be float aligned");
    if (numel[i] <= 0 || numel[i] >= (int64_t(1) << 40)) return fail(ADMMQ_ERR_ARG, "dequantize_packed: numel out of range");
  }
  for (int i0 = 0; i0 < n;) {   // up to kDqJobs tensors and 2^30 blocks per launch
    DqBatch b;
    std::memset(&b, 0, sizeof(b));
    b.meta0 = i0;
    long long nblk = 0;
    int k = 0;
    for (; k < kDqJobs && i0 + k < n; ++k) {
      const long long nb = (numel[i0 + k] + kDqBlockElems - 1) / kDqBlockElems;
      if (k > 0 && nblk + nb > (1LL << 30)) break;
      b.codes[k] = codes[i0 + k]; b.y[k] = y[i0 + k]; b.numel[k] = numel[i0 + k];
      b.blk0[k] = (int)nblk;
      nblk += nb;
    }
    b.blk0[k] = (int)nblk;
    b.njobs = k;
    launch_dequant_pack(b, (int)nblk, meta_dev, static_cast<hipStream_t>(stream));
    i0 += k;
  }
  return check_hip("dequantize_packed");
}

int32_t admmq_mse_sse_table(const float* x, int64_t rows, int64_t cols, int32_t bits, int32_t num_attempts,
                            uint64_t* sse_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!valid_bits(bits)) return fail(ADMMQ_ERR_ARG, "bits out of range");
  admmq_qtensor t;
  std::memset(&t, 0, sizeof(t));
  t.x = x; t.y = nullptr; t.rows = rows; t.cols = cols;
  QPlan pl;
  int rc = plan_quant(&t, 1, num_attempts, workspace, pl);
  if (rc) return rc;
  if (!workspace || workspace_bytes < pl.bytes) return fail(ADMMQ_ERR_WORKSPACE, "workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  RunSwitches sw = run_switches();
  sw.exhaustive = true;   // the table holds every candidate's SSE
  if ((rc = run_quant(pl, 1, bits, kMse, num_attempts, s, false, sw))) return rc;
  hipLaunchKernelGGL(k_copy_sse, dim3(1), dim3(256), 0, s, pl.d_jobs, num_attempts,
                     reinterpret_cast<unsigned long long*>(sse_out));
  return check_hip("mse_sse_table");
}

}  // extern "C"
