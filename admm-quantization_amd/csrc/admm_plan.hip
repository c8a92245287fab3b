// Host planner of the ADMM launch sequence (admm_plan.h). Host code only: no kernel, no HIP
// runtime call. plan_admm at the bottom lists the phases in the carve order.
#include "admm_plan.h"

#include <algorithm>
#include <array>
#include <cstring>
#include <map>
#include <mutex>

namespace admmq {

void carve_view(Carver& cv, MseView& v, int nslot, int ncand) {
  v.stat = cv.take<unsigned>(4 * (size_t)nslot);
  v.sse = cv.take<unsigned long long>((size_t)nslot * ncand);
  v.h1 = cv.take<unsigned long long>((size_t)nslot * kHistRep * (ncand + 1));
  v.h2 = cv.take<unsigned long long>((size_t)nslot * kHistRep * (ncand + 1));
  v.s2 = cv.take<double>((size_t)nslot);
  v.sel = cv.take<int>((size_t)nslot * (2 + kMaxSel));
  v.ticket = cv.take<unsigned>((size_t)nslot);
  v.ready = cv.take<unsigned long long>((size_t)nslot);
}

// Tile rows of the persistent fp32 solve per problem (fixed by the problem's shape, never
// by the batch, so every element's result is batch-independent): 0 = 64 x 64 tiles
// (32-row factors: 32 x 64); 1 = 128 x 64 tiles for the factors with ld >= 1024 whose I
// is a multiple of 128, 32 x 64 tiles for the others (finer filler tiles: the CU-level
// LPT of a launch then balances to ~0.99 at C3 instead of 0.89, where the 36-K-step 64 x 64
// tiles of the R = 1141 layers left gaps only coarse tiles could not fill); 2 = 64 x 64 for
// ld >= 1024, 32 x 64 for the others; 3 = 128 x 64 for ld >= 1024, 64 x 64 for the others.
static int f32_tile_rows(int rule, int I, int ld) {
  if (I <= 32) return 32;
  const bool big = ld >= 1024;
  switch (rule) {
    case 0: return 64;
    case 2: return big ? 64 : 32;
    case 3: return (big && I % 128 == 0) ? 128 : 64;
    default: return (big && I % 128 == 0) ? 128 : 32;
  }
}
static constexpr int kF32Slots = 2;   // k_gemm_f32p workgroups per CU (72 KB of LDS each)

// K-split of the fp32 64 x 64 solve tiles (gemm_kernels.hip ksplit_combine; PlanSwitches::
// ksplit: 1 = by ksplit_pieces, 0 = never (A/B)). A factor whose tiles alone leave most of
// the chip idle (a lone layer4 conv: 144 tiles of 36 K-steps on 256 CUs, the busiest shard
// of a multi-GPU run) splits every tile's K range into np pieces summed in piece order.
// Pieces per tile, a function of (I, R) ONLY (never of the batch, the device or the
// launch), so a factor's bits are the same in every batch: the np in 1..kKsplitMax with
// pieces of >= kKsplitMinSteps K-steps that minimises the factor's own launch length on
// a 256-CU chip, ceil(tiles np / 256) ceil(nk / np) K-steps plus kKsplitCost for the
// partial hand-off, ties to the smaller np. Only factors with fewer tiles than CUs split.
static constexpr int kKsplitCost = 4;   // K-steps (~2.5 us): partial stores, arrival, sc1 reads
int ksplit_pieces(int I, int R) {
  if (I <= 32) return 1;   // 32 x 64 tiles
  const int nk = rup(R, 32) / 32;
  const long long tiles = (long long)((I + 63) / 64) * ((rup(R, 32) + 63) / 64);
  // kPlanChipCUs (here and below), not the device's: np moves the factor's bits
  if (tiles >= kPlanChipCUs) return 1;
  int best = 1;
  long long best_cost = nk;
  for (int np = 2; np <= kKsplitMax; ++np) {
    const int len = (nk + np - 1) / np;
    if (len < kKsplitMinSteps) break;
    const long long cost = (tiles * np + kPlanChipCUs - 1) / kPlanChipCUs * len + kKsplitCost;
    if (cost < best_cost) { best = np; best_cost = cost; }
  }
  return best;
}

// Makespan (K-steps of the busiest CU) of an LPT placement of `costs` over ncu CUs with at
// most `slots` items each (order_tiles_for_cus' rule without its XCD tie-break); -1 when
// the items do not fit one resident round.
static long long lpt_makespan(std::vector<long long> costs, int ncu, int slots) {
  if ((long long)costs.size() > (long long)ncu * slots) return -1;
  std::sort(costs.begin(), costs.end(), std::greater<long long>());
  // min-heap of (load, cu) over the CUs with a free slot
  std::vector<std::pair<long long, int>> heap;
  std::vector<int> used(ncu, 0);
  for (int b = 0; b < ncu; ++b) heap.push_back({0, b});
  auto cmp = [](const std::pair<long long, int>& a, const std::pair<long long, int>& b) { return a > b; };
  std::make_heap(heap.begin(), heap.end(), cmp);
  long long mx = 0;
  for (long long c : costs) {
    std::pop_heap(heap.begin(), heap.end(), cmp);
    auto [ld, b] = heap.back();
    heap.pop_back();
    ld += c;
    mx = std::max(mx, ld);
    if (++used[b] < slots) {
      heap.push_back({ld, b});
      std::push_heap(heap.begin(), heap.end(), cmp);
    }
  }
  return mx;
}
// Balance (launches that fill the chip; PlanSwitches::ksplit_bal: 1 = run the pieces of the
// longest split tiles in parallel where that lowers the launch's CU-level LPT makespan
// (same bits), 0 = never; a parallel piece is priced ksplit_cost K-steps above its own).
// How many of the split tiles `cand` (longest first; (nk, np)) to run as parallel pieces so
// that the launch's LPT makespan is smallest (ties: fewer), `whole` = every tile's K-steps.
long long ksplit_balance(const std::vector<long long>& whole, std::vector<std::pair<int, int>> cand, int ncu,
                         int slots, int cost) {
  if (cand.empty() || (long long)whole.size() <= ncu) return 0;
  std::stable_sort(cand.begin(), cand.end(), [](auto& a, auto& b) { return a.first > b.first; });
  long long best_m = lpt_makespan(whole, ncu, slots);
  if (best_m < 0) return 0;
  long long best_k = 0;
  std::vector<long long> costs = whole;
  // remove one whole tile of each split candidate as it is split: keep a multiset by value
  for (long long k = 1; k <= (long long)cand.size(); ++k) {
    const int nk = cand[k - 1].first, np = cand[k - 1].second;
    auto it = std::find(costs.begin(), costs.end(), (long long)nk);
    if (it == costs.end()) break;
    costs.erase(it);
    for (int pc = 0; pc < np; ++pc) costs.push_back((pc + 1) * nk / np - pc * nk / np + cost);
    const long long m = lpt_makespan(costs, ncu, slots);
    if (m < 0) break;
    if (m < best_m) { best_m = m; best_k = k; }
  }
  return best_k;
}

static GemmTile mk_tile(int prob, int tm, int tn, int first, int nk) {
  GemmTile t;
  std::memset(&t, 0, sizeof(t));
  t.prob = prob; t.tm = tm; t.tn = tn; t.first = first; t.nk = nk; t.bm = 0;
  t.k0 = 0; t.np = 1; t.pc = 0; t.ser = 1;
  t.P = nullptr; t.M = nullptr; t.U = nullptr; t.eP = nullptr; t.eM = nullptr; t.ld = 0; t.ldm = 0;   // fill_tile_pointers
  return t;
}

// LPT placement of tiles on CUs with XCD affinity: every tile, largest `work` first, goes
// to the CU with the least work so far that still has a free slot (`slots` per CU; 0: no
// limit). Among the least-loaded CUs, prefer the XCD (CU b mod 8) that already holds tiles
// of the same column tile of M (they share its B panel through that XCD's L2), then of
// the same row panel of P (`row_by_bm`: the panel is row tm * bm, for lists whose tile rows
// differ per problem; else row tile tm). Returns each CU's tiles, largest first.
static std::vector<std::vector<GemmTile>> place_on_cus(std::vector<GemmTile> sorted, int ncu, int slots, bool row_by_bm,
                                                       long long (*work)(const GemmTile&)) {
  std::stable_sort(sorted.begin(), sorted.end(), [&](const GemmTile& a, const GemmTile& b) { return work(a) > work(b); });
  std::vector<std::vector<GemmTile>> bins(ncu);
  std::vector<long long> load(ncu, 0);
  constexpr int kXcd = 8;
  std::map<std::pair<int, int>, std::array<int, kXcd>> col_on, row_on;
  for (const GemmTile& t : sorted) {
    auto& cx = col_on[{t.prob, t.tn}];
    auto& rx = row_on[{t.prob, row_by_bm ? t.tm * t.bm : t.tm}];
    int best = -1;
    long long best_key = 0;
    for (int b = 0; b < ncu; ++b) {
      if (slots > 0 && (int)bins[b].size() >= slots) continue;
      // smaller is better: load first, then affinity (column, row)
      const long long key = load[b] * 1000000LL - cx[b % kXcd] * 1000LL - rx[b % kXcd];
      if (best < 0 || key < best_key) { best = b; best_key = key; }
    }
    bins[best].push_back(t);
    load[best] += work(t);
    cx[best % kXcd] += 1;
    rx[best % kXcd] += 1;
  }
  return bins;
}

// Persistent fp32 solve lists: every tile goes, largest MFMA work first, to the CU with the
// least work so far (ties: the CU whose XCD already holds tiles of the same M column / P row
// panel, which then come from that XCD's L2), then each CU's tiles are split over its
// kF32Slots workgroups (LPT again). Workgroup b runs on CU b mod ncu (round-robin dispatch;
// a different placement only costs speed). Fills `tiles` in list order and `off`.
static void plan_f32_lists(std::vector<GemmTile>& tiles, std::vector<int>& off, int ncu) {
  auto work = [](const GemmTile& t) { return (long long)t.bm * t.nk; };
  const std::vector<std::vector<GemmTile>> bins = place_on_cus(tiles, ncu, 0, true, work);
  const int nslots = ncu * kF32Slots;
  std::vector<std::vector<GemmTile>> lists(nslots);
  for (int c = 0; c < ncu; ++c) {
    long long sl[kF32Slots] = {};
    for (const GemmTile& t : bins[c]) {   // already largest first
      int k = 0;
      for (int j = 1; j < kF32Slots; ++j)
        if (sl[j] < sl[k]) k = j;
      lists[c + (size_t)k * ncu].push_back(t);
      sl[k] += work(t);
    }
  }
  tiles.clear();
  off.assign(nslots + 1, 0);
  for (int b = 0; b < nslots; ++b) {
    off[b] = (int)tiles.size();
    tiles.insert(tiles.end(), lists[b].begin(), lists[b].end());
  }
  off[nslots] = (int)tiles.size();
}

// CU-balanced order of the big GEMM tiles. When every tile of a launch is resident at
// once (at most `slots` workgroups per CU), workgroup b lands on CU b mod ncu (round
// robin over the XCDs, then over each XCD's CUs; tools/gemm_timeline.py checks it), so
// the tiles at positions b, b + ncu, b + 2 ncu share one CU's MFMA pipes. Longest-first
// order alone gives some CUs three long tiles and others two; instead every tile, longest
// first, goes to the CU with the fewest K-steps that still has a free slot.
// The grid is padded with empty tiles (nk = 0: the workgroup returns at once) to a whole
// number of rounds, so every CU may take up to `slots` tiles, not only the CUs whose
// positions exist in a partial last round (C3 mode 1: 645 tiles, max CU load 90 -> 84).
static void order_tiles_for_cus(std::vector<GemmTile>& tiles, int ncu, int slots) {
  const int n = (int)tiles.size();
  if (n <= ncu || n > ncu * slots) return;
  auto cost = [](const GemmTile& t) { return (long long)t.nk * ((t.bm > 0 ? t.bm : 64) / 32); };   // 32-row K-steps
  const std::vector<std::vector<GemmTile>> bins = place_on_cus(tiles, ncu, slots, false, cost);
  size_t rounds = 0;
  for (int b = 0; b < ncu; ++b) rounds = std::max(rounds, bins[b].size());
  GemmTile empty = mk_tile(0, 0, 0, 0, 0);
  tiles.assign(rounds * ncu, empty);
  for (int b = 0; b < ncu; ++b)
    for (int r = 0; r < (int)bins[b].size(); ++r) tiles[b + (size_t)r * ncu] = bins[b][r];
}

// 64 x 64 tiles of a kProbBig problem
static long long tiles64(const ProbDesc& d) { return (long long)(d.Ip / 64) * ((d.ld + 63) / 64); }

// One problem's buffers, in the order every carve of it takes them (d's shape fields set)
static void carve_problem(Carver& cv, ProbDesc& d, int ncand) {
  const size_t fe = (size_t)d.Ip * d.ld;
  d.Fp = cv.take<float>(fe); d.H = cv.take<float>(fe); d.U = cv.take<float>(fe);
  d.P = cv.take<float>(fe); d.X = cv.take<float>(fe); d.HT = cv.take<float>(fe);
  d.M = cv.take<float>((size_t)d.ldm * d.ldm);
  d.A64 = cv.take<double>((size_t)d.ldm * d.ldm);
  d.L64 = cv.take<double>((size_t)d.ldm * d.ldm);
  d.D64 = cv.take<double>((size_t)d.ldm * 32);
  if (d.split) {
    d.P2 = cv.take<_Float16>(2 * fe);
    d.eP = cv.take<int>(d.Ip);
    d.M2 = cv.take<_Float16>(2 * (size_t)d.ldm * d.ldm);
    d.eM = cv.take<int>(d.ldm);
  }
  if (d.ksplit > 1)   // the partial images of every 64 x 64 tile (the counters are carved after the problems)
    d.kpart = cv.take<float>((size_t)tiles64(d) * d.ksplit * 4096);
  d.res = cv.take<double>(2 * kResRep * 4);
  d.flags = cv.take<int>(4);
  d.rho = cv.take<float>(4);
  carve_view(cv, d.mv, 2, ncand);
  d.mv.X = d.HT; d.mv.U = d.U; d.mv.rows = d.I; d.mv.cols = d.R; d.mv.ld = d.ld; d.mv.qpr = (d.R + 3) / 4;
  d.mv.nq = d.nq; d.mv.nelem = d.I * d.R; d.mv.done = d.flags;
}

// Validation, the padding rules, the carve of each problem's buffers (and of the K-split
// counters after them) and the maxima. Fixes the launch-wide forms (split, wide, f32p,
// f32t), each problem's class and pl.order.
static int describe_problems(const admmq_problem* probs, int nprob, int ncand, const PlanSwitches& sw, int solve_mode,
                             Carver& cv, AdmmPlan& pl) {
  pl.desc.resize(nprob);
  pl.cls.resize(nprob);
  pl.thin_nr = 0;
  for (int i = 0; i < nprob; ++i)
    if (probs[i].I > 0 && probs[i].I <= kThinRows) pl.thin_nr = std::max(pl.thin_nr, probs[i].I);
  pl.split = solve_mode == kSolveSplit;
  // Wide tiles when the 64x64 tiles would take many rounds of the resident slots
  // (256 CUs x 3): then a CU's bytes per MAC matter more than the number of tiles, and
  // 256x128 tiles read 3/8 of the operand bytes per MAC (the Llama shapes of C5). The
  // element results do not depend on the tile shape (same K order per element).
  {
    long long t64 = 0;
    for (int i = 0; i < nprob; ++i)
      if (probs[i].I > 32) t64 += (long long)((probs[i].I + 63) / 64) * ((rup(std::max(probs[i].R, 1), 32) + 63) / 64);
    pl.wide = t64 >= sw.wide_min_tiles;
  }
  for (int i = 0; i < nprob; ++i)   // the split finalize needs whole rows in one unit
    if (probs[i].I > kThinRows && rup(std::max(probs[i].R, 1), 32) > 8192) pl.split = false;
  // persistent fp32 solve: every non-thin, non-wide factor in per-workgroup lists
  pl.f32p = !pl.split && sw.f32_kernel == 1;
  pl.f32t = !pl.split && sw.f32_kernel == 2;
  for (int i = 0; i < nprob; ++i) {
    const admmq_problem& a = probs[i];
    if (a.I <= 0 || a.R <= 0) return set_error(ADMMQ_ERR_ARG, "I and R must be positive");
    if ((long long)a.I * a.R > (1LL << 30)) return set_error(ADMMQ_ERR_ARG, "factor too large");
    ProbDesc& d = pl.desc[i];
    std::memset(&d, 0, sizeof(d));
    d.F_user = a.F; d.G_user = a.G; d.H0_user = a.H0; d.H_out = a.H_out; d.U_user = a.U;
    d.HT_dbg = a.HT_out; d.X_dbg = a.X_out;
    d.I = a.I; d.R = a.R;
    d.ld = rup(a.R, 32);
    const bool thin = a.I <= kThinRows;
    // K-split pieces (fp32 64 x 64 tiles only; by shape alone): such a factor never takes
    // the wide tiles, whatever its launch, so its bits stay those of its own shape
    d.ksplit = (!pl.split && sw.ksplit != 0 && sw.f32_kernel == 0 && sw.gemm_ks == 1 && !thin)
                   ? ksplit_pieces(a.I, a.R) : 1;
    const bool wide = pl.wide && a.I > 64 && d.ksplit == 1;
    pl.cls[i] = thin ? kProbThin : (a.I <= 32 ? kProbRows32 : (wide ? kProbWide : kProbBig));
    const bool f32p_prob = !pl.split && sw.f32_kernel != 0 && !wide && !thin;
    d.Ip = a.I <= 32 ? 32 : rup(a.I, wide ? kWideRows : (f32p_prob ? std::max(64, f32_tile_rows(sw.f32_rule, a.I, d.ld)) : 64));
    d.ldm = rup(a.R, 64);
    d.nbk = d.ldm / 32;
    d.nq = a.I * ((a.R + 3) / 4);
    // 32-bit element offsets inside a problem's padded buffers (admm_finalize_block)
    if ((long long)d.Ip * d.ld >= (1LL << 31)) return set_error(ADMMQ_ERR_ARG, "factor too large");
    d.split = (pl.split && !thin) ? 1 : 0;
    carve_problem(cv, d, ncand);
    pl.maxIp = std::max(pl.maxIp, d.Ip); pl.maxld = std::max(pl.maxld, d.ld);
    pl.maxldm = std::max(pl.maxldm, d.ldm); pl.maxnbk = std::max(pl.maxnbk, d.nbk);
    pl.maxI = std::max(pl.maxI, d.I); pl.maxR = std::max(pl.maxR, d.R);
  }
  // K-split arrival counters: one per split tile, contiguous (zeroed at the start of every run)
  pl.nkctr = 0;
  for (const ProbDesc& d : pl.desc)
    if (d.ksplit > 1) pl.nkctr += (size_t)tiles64(d);
  pl.d_kctr = cv.take<unsigned>(std::max<size_t>(pl.nkctr, 1));
  // GEMM tiles, longest K first (LPT over the grid)
  pl.order.resize(nprob);
  for (int i = 0; i < nprob; ++i) pl.order[i] = i;
  std::stable_sort(pl.order.begin(), pl.order.end(), [&](int a, int b) { return pl.desc[a].ld > pl.desc[b].ld; });
  return ADMMQ_OK;
}

// Wide tiles (kWideRows x 128, pl.wide, I > 64), placed by XCD: workgroup b runs on XCD
// b mod 8, in order of b within the XCD. These launches have I >> R (the Llama shapes),
// so the P row panel (kWideRows x ld) is the big operand: every row panel goes to ONE
// XCD (least K-step load first), which runs all of its column tiles back to back, so P is
// fetched once into that XCD's L2 instead of once per XCD (the column-major order kept
// a column tile of M per XCD and made all 8 XCDs fetch every P panel: 3.5x the
// algorithmic bytes at C5). Queue x fills positions x, x + 8, ...; a queue that runs
// out early takes tiles from the tail of the longest one.
static void plan_wide_tiles(AdmmPlan& pl) {
  constexpr int kXcd = 8;
  std::vector<std::vector<GemmTile>> q(kXcd);
  std::vector<long long> qload(kXcd, 0);
  for (int i : pl.order) {
    const ProbDesc& d = pl.desc[i];
    if (pl.cls[i] != kProbWide) continue;
    const int TM = d.Ip / kWideRows, TN = (d.ld + 127) / 128;
    for (int tm = 0; tm < TM; ++tm) {
      const int x = (int)(std::min_element(qload.begin(), qload.end()) - qload.begin());
      for (int tn = 0; tn < TN; ++tn) q[x].push_back(mk_tile(i, tm, tn, (tm == 0 && tn == 0) ? 1 : 0, d.ld / 32));
      qload[x] += (long long)TN * (d.ld / 32);
    }
  }
  std::vector<GemmTile>& wide = pl.tiles;
  std::vector<size_t> head(kXcd, 0);
  size_t left = 0;
  for (auto& v : q) left += v.size();
  for (size_t b = 0; left > 0; ++b, --left) {
    int x = (int)(b % kXcd);
    if (head[x] >= q[x].size()) {   // exhausted: the longest remaining queue donates its last tile
      int y = 0;
      for (int z = 1; z < kXcd; ++z)
        if (q[z].size() - head[z] > q[y].size() - head[y]) y = z;
      wide.push_back(q[y].back());
      q[y].pop_back();
      continue;
    }
    wide.push_back(q[x][head[x]++]);
  }
}

// The tiles of the diagnostic fp32 kernels (pl.f32p: k_gemm_f32p's per-workgroup lists;
// pl.f32t: one tile per workgroup), f32_tile_rows x 64 over every non-thin, non-wide
// factor; the two differ only in the placement. Sets list_off / nslots / ntiles_f32t.
static void plan_list_tiles(AdmmPlan& pl, const PlanSwitches& sw, int ncu) {
  std::vector<GemmTile> ft;
  for (int i : pl.order) {
    const ProbDesc& d = pl.desc[i];
    if (pl.cls[i] != kProbRows32 && pl.cls[i] != kProbBig) continue;
    const int bm = f32_tile_rows(sw.f32_rule, d.I, d.ld);
    const int TM = (d.I + bm - 1) / bm, TN = (d.ld + 63) / 64;
    for (int tm = 0; tm < TM; ++tm)
      for (int tn = 0; tn < TN; ++tn) {
        GemmTile t = mk_tile(i, tm, tn, (tm == 0 && tn == 0) ? 1 : 0, d.ld / 32);
        t.bm = bm;
        ft.push_back(t);
      }
  }
  if (pl.f32p && !ft.empty()) {
    // ncu: the lists are one per resident workgroup of this device (as found: list_off's
    // length also sizes d_list_off in the carve)
    plan_f32_lists(ft, pl.list_off, ncu);
    pl.nslots = ncu * kF32Slots;
  }
  if (pl.f32t) {
    order_tiles_for_cus(ft, kPlanChipCUs, 3);   // kPlanChipCUs: as found (the literal 256)
    pl.ntiles_f32t = (int)ft.size();
  }
  pl.tiles.insert(pl.tiles.end(), ft.begin(), ft.end());
}

// The fp32 64 x 64 tile list of a plan (pl.desc, pl.cls, pl.order set; not f32p / f32t):
// whole tiles in problem order (XCD-aware within each problem), K-split pieces in parallel
// or folded serially, then the CU-level LPT order. part / ctr are left for
// fill_tile_pointers. Every CU count in it is kPlanChipCUs: the list is memoised by the
// shapes and switches alone, and its order fixes which tiles take the parallel pieces.
static std::vector<GemmTile> build_big_tiles(const AdmmPlan& pl, const PlanSwitches& sw, bool& ksplit_par) {
  std::vector<int> big;
  for (int i : pl.order)
    if (pl.cls[i] == kProbBig) big.push_back(i);   // thin / 32-row / wide: elsewhere
  // The K-split pieces of a factor (fixed by its shape) run in parallel, np workgroups per
  // tile, only in a launch whose whole tiles leave CUs idle (a lone large factor, as in a
  // multi-GPU shard); otherwise one workgroup folds them serially (same bits, no hand-off).
  long long whole64 = 0;
  for (int i : big) whole64 += tiles64(pl.desc[i]);
  ksplit_par = sw.ksplit_form == 2 || (sw.ksplit_form == 1 && whole64 <= kPlanChipCUs);
  const int slots = f32_slots(sw.gemm_stage);
  // A launch that fills the chip runs the pieces serially, except the `npar` longest split
  // tiles (balance): their pieces in parallel fill the gaps a CU-level LPT of whole tiles
  // leaves (C3 mode 0: 36-K-step tiles, max CU load 90 against a mean of 80).
  long long npar = ksplit_par ? (1LL << 40) : 0;
  if (!ksplit_par && sw.ksplit_form == 1 && sw.ksplit_bal) {
    std::vector<long long> whole;   // K-steps of every 64 x 64 tile of the launch
    std::vector<std::pair<int, int>> cand;   // (nk, np) of the split tiles, longest first
    for (int i : big) {
      const ProbDesc& d = pl.desc[i];
      const long long nt = tiles64(d);
      for (long long t = 0; t < nt; ++t) whole.push_back(d.ld / 32);
      if (d.ksplit > 1)
        for (long long t = 0; t < nt; ++t) cand.push_back({d.ld / 32, d.ksplit});
    }
    npar = ksplit_balance(whole, cand, kPlanChipCUs, slots, sw.ksplit_cost);
  }
  // `first` marks tile (0,0). XCD-aware order: workgroups b and b+8 share an XCD
  // (round-robin dispatch), so the row tiles that read the same B tile (one column tile tn
  // of M) are laid out 8 apart: within each group of up to 8 column tiles, positions run
  // tm-major, tn-minor.
  std::vector<GemmTile> tiles;
  long long nsplit = 0;   // split tiles emitted so far (the first npar of them run in parallel)
  for (int i : big) {
    const ProbDesc& d = pl.desc[i];
    const int TM = d.Ip / 64, TN = (d.ld + 63) / 64;
    const int nk = d.ld / 32;
    for (int g0 = 0; g0 < TN; g0 += 8)
      for (int tm = 0; tm < TM; ++tm)
        for (int tn = g0; tn < std::min(TN, g0 + 8); ++tn) {
          const int np = (d.ksplit > 1 && nsplit++ < npar) ? d.ksplit : 1;
          for (int pc = 0; pc < np; ++pc) {   // parallel K-split pieces: [pc nk / np, (pc + 1) nk / np)
            const int k0 = pc * nk / np, k1 = (pc + 1) * nk / np;
            GemmTile t = mk_tile(i, tm, tn, (tm == 0 && tn == 0 && pc == 0) ? 1 : 0, k1 - k0);
            if (np > 1) {
              t.k0 = k0; t.np = np; t.pc = pc;   // (part / ctr: filled per call)
            } else {
              t.ser = d.ksplit;   // serial form (1: no K-split)
            }
            tiles.push_back(t);
          }
        }
  }
  // a launch of more tiles than resident slots (K-split pieces, C4) is dispatched in
  // order as slots free up: longest first (a no-op without pieces: problems are in ld order)
  if (tiles.size() > (size_t)kPlanChipCUs * 3)
    std::stable_sort(tiles.begin(), tiles.end(), [](const GemmTile& a, const GemmTile& b) { return a.nk > b.nk; });
  order_tiles_for_cus(tiles, kPlanChipCUs, slots);
  return tiles;
}

// The 64 x 64 tile list (pieces, serial folds, CU order) is a pure function of the
// problems' shapes and the switches: memoised, so repeated calls (prepare and run of one
// call, every ALS sweep) skip the LPT placement; the per-call pointers are filled after.
// Keyed by the inputs themselves, compared for equality (bounded; cleared when full).
// Appends the list to pl.tiles and sets pl.ksplit_par.
struct TileMemo { std::vector<GemmTile> tiles; bool ksplit_par; };
static std::mutex g_tile_mu;
static std::map<std::vector<int>, TileMemo> g_tile_memo;
static void plan_big_tiles(AdmmPlan& pl, const PlanSwitches& sw) {
  std::vector<int> key = {sw.ksplit_form, sw.ksplit_bal, sw.ksplit_cost, f32_slots(sw.gemm_stage)};
  key.reserve(key.size() + 6 * pl.order.size());
  for (int i : pl.order) {
    const ProbDesc& d = pl.desc[i];
    key.insert(key.end(), {i, d.I, d.Ip, d.ld, d.ksplit, pl.cls[i] == kProbWide ? 1 : 0});
  }
  std::unique_lock<std::mutex> g(g_tile_mu);
  auto it = g_tile_memo.find(key);
  if (it == g_tile_memo.end()) {
    g.unlock();   // (two threads may both build the same list: the second insert is a no-op)
    TileMemo m;
    m.tiles = build_big_tiles(pl, sw, m.ksplit_par);
    g.lock();
    if (g_tile_memo.size() >= 64) g_tile_memo.clear();
    it = g_tile_memo.emplace(std::move(key), std::move(m)).first;
  }
  pl.ksplit_par = it->second.ksplit_par;
  pl.tiles.insert(pl.tiles.end(), it->second.tiles.begin(), it->second.tiles.end());
}

// 32 x 64 tiles of the 17..32-row factors
static void plan_small_tiles(AdmmPlan& pl) {
  for (int i : pl.order) {
    const ProbDesc& d = pl.desc[i];
    if (pl.cls[i] != kProbRows32) continue;
    const int TN = (d.ld + 63) / 64;
    for (int tn = 0; tn < TN; ++tn) pl.tiles.push_back(mk_tile(i, 0, tn, tn == 0 ? 1 : 0, d.ld / 32));
  }
}

// The operands' addresses and strides of every tile (admmq_internal.h GemmTile), the stop
// test's inputs (launch-head bit 0), and this call's partial images and counters of the parallel K-split pieces
static void fill_tile_pointers(AdmmPlan& pl, const PlanSwitches& sw) {
  if (!pl.d_kctr) return;   // a size query carves from a null base: there are no addresses to fill
  std::vector<size_t> ctrbase(pl.desc.size(), 0);   // first counter of each split problem
  size_t n = 0;
  for (int i : pl.order) {
    const ProbDesc& d = pl.desc[i];
    if (pl.cls[i] != kProbBig || d.ksplit <= 1) continue;
    ctrbase[i] = n;
    n += (size_t)tiles64(d);
  }
  for (GemmTile& t : pl.tiles) {
    const ProbDesc& d = pl.desc[t.prob];
    t.U = d.U; t.ld = d.ld; t.ldm = d.ldm;
    if (sw.launch_head & kHeadGemmStop) { t.flags = d.flags; t.res = d.res; }   // else null: read through the descriptor
    if (d.split) {   // the fp16 planes keep the fp32 rows' strides (in floats)
      t.P = reinterpret_cast<const float*>(d.P2); t.M = reinterpret_cast<const float*>(d.M2);
      t.eP = d.eP; t.eM = d.eM;
    } else {
      t.P = d.P; t.M = d.M;
    }
    if (t.np > 1) {
      const int TN = (d.ld + 63) / 64;
      t.part = d.kpart + (size_t)(t.tm * TN + t.tn) * t.np * 4096;
      t.ctr = pl.d_kctr + ctrbase[t.prob] + (size_t)(t.tm * TN + t.tn);
    }
  }
}

// pl.tiles in launch order (each phase appends): the wide tiles, then the 64 x 64 tiles
// and the 32 x 64 tiles of the 17..32-row factors, or the f32p / f32t tiles of both (their
// own launches)
static void plan_gemm_tiles(AdmmPlan& pl, const PlanSwitches& sw, int ncu) {
  plan_wide_tiles(pl);
  pl.ntiles_wide = (int)pl.tiles.size();
  if (pl.f32p || pl.f32t) {
    plan_list_tiles(pl, sw, ncu);
  } else {
    plan_big_tiles(pl, sw);
    pl.ntiles_big = (int)pl.tiles.size() - pl.ntiles_wide;
    plan_small_tiles(pl);
    pl.ntiles_small = (int)pl.tiles.size() - pl.ntiles_wide - pl.ntiles_big;
  }
  fill_tile_pointers(pl, sw);
}

// thin factors: one solve workgroup per 32 columns (thin_loop.hip), longest rows first;
// the same list is the persistent loop's teams (rank = column block)
static void plan_thin_units(AdmmPlan& pl) {
  pl.thin_maxld = 0;
  for (int i : pl.order) {
    const ProbDesc& d = pl.desc[i];
    if (pl.cls[i] != kProbThin) continue;
    pl.thin_maxld = std::max(pl.thin_maxld, d.ld);
    for (int c = 0; c < d.ld; c += 32) {
      ThinLoopUnit u;
      std::memset(&u, 0, sizeof(u));
      u.job = i; u.col0 = c; u.cw = 32; u.rank = c / 32; u.nteam = d.ld / 32;
      pl.thin.push_back(u);
    }
  }
}

// Teams of the persistent thin-factor loop: 32-column workgroups, and while they would
// not all fit on the CUs at once, the shortest problems with ld <= 512 take 64-column ones
// (two k classes per thread, the same chains and sums: thin_loop.hip), whose per-iteration
// work (64 ld) stays below the largest team's (32 x 1152).
static bool plan_thin_teams(AdmmPlan& pl, const PlanSwitches& sw, int ncu) {
  pl.tl_units.clear();
  const int nprob = (int)pl.desc.size();
  if ((int)pl.small.size() != nprob || nprob == 0 || pl.thin_maxld > 1152) return false;
  std::vector<int> cw(nprob, 32);
  auto nwg = [&](int i) { const int ld = pl.desc[i].ld; return cw[i] == 64 ? ld / 64 + (ld % 64 ? 1 : 0) : ld / 32; };
  long long total = 0;
  for (int i = 0; i < nprob; ++i) total += nwg(i);
  const bool wide_all = sw.thin_loop == 2;
  while (total > ncu || wide_all) {
    int best = -1;
    for (int i = 0; i < nprob; ++i)
      if (cw[i] == 32 && pl.desc[i].ld <= 512 && pl.desc[i].ld >= 64 && (best < 0 || pl.desc[i].ld < pl.desc[best].ld))
        best = i;
    if (best < 0) {
      if (total > ncu) return false;
      break;
    }
    total -= nwg(best);
    cw[best] = 64;
    total += nwg(best);
  }
  for (const ThinLoopUnit& u0 : pl.thin) {   // the problems in the planner's order
    if (u0.col0 != 0) continue;
    const int i = u0.job, ld = pl.desc[i].ld;
    const int n = nwg(i);
    for (int c = 0, r = 0; c < ld; ++r) {
      const int w = std::min(cw[i], ld - c);
      ThinLoopUnit u;
      std::memset(&u, 0, sizeof(u));
      u.job = i; u.col0 = c; u.cw = w; u.rank = r; u.nteam = n;
      pl.tl_units.push_back(u);
      c += w;
    }
  }
  return true;
}

// Finalize units hold whole rows (the split solve needs each row's exponent in one pass):
// at most 1024 G elements, G in {1, 2, 4, 8}. Returns G.
static int fin_groups_for(const std::vector<ProbDesc>& desc, const std::vector<int>& jobs) {
  long long units4k = 0;
  int maxld = 0;
  for (int i : jobs) {
    units4k += ((long long)desc[i].I * desc[i].ld + kFinElems - 1) / kFinElems;
    maxld = std::max(maxld, desc[i].ld);
  }
  int g = units4k >= kFinMinUnits ? 4 : 1;   // small problem sets keep their parallelism
  while (g < 8 && 1024 * g < maxld) g *= 2;
  return g;
}

// Sets pl.hist_nv and returns the stage-1 unit size (elements) of the big jobs
// (`big_jobs`: every I > kThinRows problem). The resident blocks are counted on `ncu`, the
// device's CUs (as found: hist_nv is part of the carve's fingerprint, so prepare and run
// must see the same device).
static long long stage1_unit_elems(AdmmPlan& pl, const PlanSwitches& sw, int ncu, const std::vector<int>& big_jobs) {
  long long hist_units = 0;
  for (const ProbDesc& d : pl.desc) hist_units += ((long long)d.I * d.ld + kHistElems - 1) / kHistElems;
  pl.hist_nv = hist_units > kHistMaxUnits ? 2 : 1;   // one round of resident stage-1 blocks
  // Stage-1 unit size of the big jobs: kHistElems x hist_nv, or smaller when that would
  // leave the one round of resident blocks (2 per CU) partly filled: C3 mode 0 had 371
  // units of ~8 k elements, so 115 CUs ran two blocks (16 k elements) and 141 one; units
  // of about total / (2 x CUs) elements give every CU the same share (unit boundaries move
  // only the order of the fp64 residual partial sums, never an element's result)
  long long big_elems = 0;
  for (int i : big_jobs) big_elems += (long long)pl.desc[i].I * pl.desc[i].ld;
  // whole-row units of at most t elements of the big jobs
  auto big_units = [&](long long t) {
    long long units = 0;
    for (int i : big_jobs) {
      const ProbDesc& d = pl.desc[i];
      const long long st = d.ld <= t ? (t / d.ld) * d.ld : t;
      units += ((long long)d.I * d.ld + st - 1) / st;
    }
    return units;
  };
  const long long slots = 2LL * ncu;
  // three float4 groups per thread (k_mse_hist3<.., 3, ..>) when the units at two would
  // outnumber the fused search's resident blocks (2 per CU) and at three would not: the
  // finalize then stays in the search launch (C4: 5.7 M elements per mode, 722 units of
  // 8 k against 512 slots; without this, the separate k_finalize_admm launch)
  if (pl.hist_nv == 2 && sw.fin_nv3 && big_units((long long)kHistElems * 2) > slots &&
      big_units((long long)kHistElems * 3) <= slots)
    pl.hist_nv = 3;
  // (not with hist_nv = 1: a lone layer4 factor's 589 k elements in 512 one-row units
  // instead of 171 three-row ones made its search 22 -> 27 us - the flush atomics and the
  // ticket chain grow with the block count faster than the per-block phases shrink)
  long long hu_big = (long long)kHistElems * pl.hist_nv;
  if (pl.hist_nv >= 2 && sw.even_units) {
    int big_maxld = 0;
    for (int i : big_jobs) big_maxld = std::max(big_maxld, pl.desc[i].ld);
    for (long long t = std::max<long long>(big_maxld, (big_elems + slots - 1) / slots); t < hu_big; t += 256)
      if (big_units(t) <= slots) { hu_big = t; break; }
  }
  return hu_big;
}

// A finalize / stage-1 unit [start, end) of job i, with the job's inputs riding along
static Chunk search_unit(const ProbDesc& d, int i, long long start, long long end) {
  return {i, (int)start, d.mv.stat, d.flags, d.HT, d.U, end, d.H, d.Fp, d.mv.sel};
}

// The search's work units: exhaustive-SSE, finalize and stage-1 units of every job, and
// the small jobs' list.
static void plan_search_units(AdmmPlan& pl, const PlanSwitches& sw, int ncu) {
  std::vector<int> big_jobs;
  for (size_t i = 0; i < pl.desc.size(); ++i)
    if (pl.cls[i] != kProbThin) big_jobs.push_back((int)i);
  pl.fin_groups = fin_groups_for(pl.desc, big_jobs.empty() ? pl.order : big_jobs);
  const long long hu_big = stage1_unit_elems(pl, sw, ncu, big_jobs);
  // stage-1 / finalize units of the small jobs (I <= kThinRows) go last: when their
  // fused one-block path runs (k_mse_small_admm), the launches take only the others
  pl.rows_aligned = true;
  const long long fin_cap = 1024LL * pl.fin_groups;
  for (int pass = 0; pass < 2; ++pass) {
    for (int i : pl.order) {
      ProbDesc& d = pl.desc[i];
      if ((pl.cls[i] == kProbThin) != (pass == 1)) continue;
      if (pass == 1) pl.small.push_back(i);
      for (int q = 0; q < d.nq; q += kSseQuads) pl.sse_chunks.push_back({i, q});
      const long long tot = (long long)d.I * d.ld;
      // whole rows per unit (rows longer than a unit: plain chunks; never a split problem)
      const long long step = d.ld <= fin_cap ? (fin_cap / d.ld) * d.ld : fin_cap;
      d.fin_rows = d.ld <= fin_cap ? (int)(fin_cap / d.ld) : 0;
      for (long long e = 0; e < tot; e += step) pl.fin_chunks.push_back(search_unit(d, i, e, std::min(tot, e + step)));
      // stage-1 units: whole rows where a row fits (the fused finalize needs them), each
      // with the job's finalize inputs; `total` is the unit's end
      const long long hu = pass == 0 ? hu_big : (long long)kHistElems * pl.hist_nv;
      const long long hstep = d.ld <= hu ? (hu / d.ld) * d.ld : hu;
      if (pass == 0 && d.ld > hu) pl.rows_aligned = false;
      int nh = 0;
      for (long long e = 0; e < tot; e += hstep, ++nh)
        pl.hist_chunks.push_back(search_unit(d, i, e, std::min(tot, e + hstep)));
      d.mv.nhist = nh;
    }
    if (pass == 0) { pl.nfin_big = (int)pl.fin_chunks.size(); pl.nhist_big = (int)pl.hist_chunks.size(); }
  }
  long long small_max = 0;
  for (int i : pl.small) small_max = std::max(small_max, (long long)pl.desc[i].I * pl.desc[i].ld);
  pl.small_groups = small_admm_groups(small_max);
}

// Without the fused finalize (the search launch cannot hold every unit at once, e.g.
// C5: ~6800 units) every block repeats the table setup (~6 us) and the histogram flush
// for one 8192-element unit; instead a block takes `reps` consecutive units of its job,
// sized for about kHistMultiRounds rounds of resident blocks.
static void plan_hist_multi(AdmmPlan& pl, const PlanSwitches& sw) {
  const long long nu_all = (long long)pl.hist_chunks.size();
  const int reps = sw.hist_reps > 0 ? sw.hist_reps
                                    : (int)std::max(1LL, std::min<long long>(kHistMultiMaxReps,
                                                                             nu_all / (kHistMultiRounds * kHistMaxUnits)));
  for (size_t a = 0; a < pl.hist_chunks.size();) {
    size_t b = a;   // the job's units are contiguous
    while (b < pl.hist_chunks.size() && pl.hist_chunks[b].job == pl.hist_chunks[a].job) ++b;
    const int nblk = (int)((b - a + reps - 1) / reps);
    for (size_t c = a; c < b; c += reps) {
      const size_t e = std::min(b, c + reps) - 1;
      Chunk k = pl.hist_chunks[c];
      k.reps = (int)(e - c + 1);
      k.step = (int)(pl.hist_chunks[c].total - pl.hist_chunks[c].start);   // a full unit unless it is the last
      k.total = pl.hist_chunks[e].total;
      k.nblk = nblk;
      pl.hist_multi.push_back(k);
    }
    if ((int)a < pl.nhist_big) pl.nhm_big = (int)pl.hist_multi.size();
    a = b;
  }
}

// The device tables, sized by the lists planned above, and the thin-loop teams
static void carve_tables(AdmmPlan& pl, const PlanSwitches& sw, int ncu, Carver& cv) {
  const int nprob = (int)pl.desc.size();
  pl.d_ready = cv.take<unsigned long long>(2 * (size_t)nprob);
  for (int i = 0; i < nprob; ++i) pl.desc[i].mv.ready = pl.d_ready ? pl.d_ready + 2 * i : nullptr;
  pl.d_desc = cv.take<ProbDesc>(nprob);
  pl.d_tiles = cv.take<GemmTile>(pl.tiles.size());
  pl.d_list_off = cv.take<int>(pl.list_off.size() + 1);
  pl.d_sse = cv.take<Chunk>(pl.sse_chunks.size());
  pl.d_fin = cv.take<Chunk>(pl.fin_chunks.size());
  pl.d_hist = cv.take<Chunk>(pl.hist_chunks.size());
  pl.d_hist_multi = cv.take<Chunk>(pl.hist_multi.size());
  pl.d_small = cv.take<int>(std::max<size_t>(pl.small.size(), 1));
  pl.d_thin = cv.take<ThinLoopUnit>(pl.thin.size());
  if ((int)pl.small.size() == nprob) {   // sized by the problems alone (not by the device's CUs)
    pl.d_tl_sync = cv.take<ThinSync>(nprob);
    pl.d_tl_units = cv.take<ThinLoopUnit>(pl.thin.size());   // >= the loop's workgroups
    pl.tl_ok = plan_thin_teams(pl, sw, ncu);   // ncu: whether the teams fit this device at once
  }
  pl.d_rank0 = cv.take<unsigned short>(kMaxMerged + kCells + 2);
  pl.d_groups = cv.take<unsigned short>(3 * kMaxMerged);
  pl.bytes = align_up(cv.off, 256);
}

// The phases run in the carve order: the problems' buffers and the K-split counters
// (describe_problems), then the device tables (carve_tables), whose sizes come from the
// lists planned in between. That order is the contract between the size query, prepare
// and run: all three must carve the workspace alike.
int plan_admm(const admmq_problem* probs, int nprob, int ncand, void* ws, const PlanSwitches& sw, int solve_mode,
              int ncu, AdmmPlan& pl) {
  if (nprob <= 0 || !probs) return set_error(ADMMQ_ERR_ARG, "no problems");
  if (ncand < 1) return set_error(ADMMQ_ERR_ARG, "num_attempts must be >= 1");
  pl = AdmmPlan();
  Carver cv(ws);
  const int rc = describe_problems(probs, nprob, ncand, sw, solve_mode, cv, pl);
  if (rc) return rc;
  plan_gemm_tiles(pl, sw, ncu);
  plan_thin_units(pl);
  plan_search_units(pl, sw, ncu);
  plan_hist_multi(pl, sw);
  carve_tables(pl, sw, ncu, cv);
  return ADMMQ_OK;
}

unsigned long long plan_fingerprint(const AdmmPlan& pl, const void* ws) {
  unsigned long long h = 1469598103934665603ull;
  auto mix = [&](long long v) {
    for (int b = 0; b < 8; ++b) { h ^= (unsigned long long)((v >> (8 * b)) & 0xFF); h *= 1099511628211ull; }
  };
  const char* base = static_cast<const char*>(ws);
  auto off = [&](const void* p) { return p ? (long long)(static_cast<const char*>(p) - base) : -1LL; };
  mix((long long)pl.bytes);
  mix((long long)pl.desc.size());
  for (const ProbDesc& d : pl.desc) {
    mix(d.I); mix(d.R); mix(d.Ip); mix(d.ld); mix(d.ldm); mix(d.split); mix(d.ksplit);
    mix(off(d.Fp)); mix(off(d.M)); mix(off(d.P2)); mix(off(d.kpart)); mix(off(d.mv.h1)); mix(off(d.flags));
  }
  mix(off(pl.d_desc)); mix(off(pl.d_tiles)); mix(off(pl.d_kctr)); mix(off(pl.d_rank0)); mix(pl.hist_nv);
  return h;
}

// Sections: 0 byte count and scalars, 1 problem descriptors, 2 GEMM tiles, 3 list offsets,
// 4 exhaustive-SSE and finalize units, 5 stage-1 units (one and several per block),
// 6 thin units, thin-loop teams and small jobs, 7 device-table offsets. Mixed field by field
// (struct padding is undefined); every pointer into the workspace goes in as its offset
// from `ws` (-1: null), the caller's pointers are left out.
void plan_digest(const AdmmPlan& pl, const void* ws, uint64_t out[8]) {
  uint64_t h = 0;
  auto mix = [&](long long v) {
    for (int b = 0; b < 8; ++b) { h ^= (uint64_t)((v >> (8 * b)) & 0xFF); h *= 1099511628211ull; }
  };
  const char* base = static_cast<const char*>(ws);
  auto off = [&](const void* p) { mix(p ? (long long)(static_cast<const char*>(p) - base) : -1LL); };
  auto chunks = [&](const std::vector<Chunk>& v) {
    mix((long long)v.size());
    for (const Chunk& c : v) {
      mix(c.job); mix(c.start); off(c.stat); off(c.done); off(c.X); off(c.U); mix(c.total);
      off(c.H); off(c.F); off(c.sel); mix(c.reps); mix(c.step); mix(c.nblk);
    }
  };
  auto units = [&](const std::vector<ThinLoopUnit>& v) {
    mix((long long)v.size());
    for (const ThinLoopUnit& u : v) { mix(u.job); mix(u.col0); mix(u.cw); mix(u.rank); mix(u.nteam); }
  };
  constexpr uint64_t kFnv = 1469598103934665603ull;
  h = kFnv;
  mix((long long)pl.bytes);
  mix(pl.maxIp); mix(pl.maxld); mix(pl.maxldm); mix(pl.maxnbk); mix(pl.maxI); mix(pl.maxR);
  mix(pl.ntiles_wide); mix(pl.ntiles_big); mix(pl.ntiles_small); mix(pl.ntiles_f32t); mix(pl.nslots);
  mix(pl.wide); mix(pl.split); mix(pl.f32p); mix(pl.f32t); mix(pl.ksplit_par);
  mix(pl.fin_groups); mix(pl.hist_nv); mix(pl.nfin_big); mix(pl.nhist_big); mix(pl.nhm_big);
  mix(pl.rows_aligned); mix(pl.small_groups); mix(pl.thin_nr); mix(pl.thin_maxld);
  mix((long long)pl.nkctr); mix(pl.tl_ok);
  out[0] = h;
  h = kFnv;
  mix((long long)pl.desc.size());
  for (const ProbDesc& d : pl.desc) {
    off(d.Fp); off(d.H); off(d.U); off(d.P); off(d.X); off(d.HT); off(d.M);
    off(d.A64); off(d.L64); off(d.D64); off(d.P2); off(d.eP); off(d.M2); off(d.eM);
    const MseView& v = d.mv;
    off(v.X); off(v.U); mix(v.rows); mix(v.cols); mix(v.ld); mix(v.qpr); mix(v.nq); mix(v.nelem);
    off(v.stat); off(v.sse); off(v.h1); off(v.h2); off(v.s2); off(v.sel); off(v.ticket); off(v.ready);
    off(v.done); mix(v.nhist);
    off(d.res); off(d.flags); off(d.rho);
    mix(d.I); mix(d.R); mix(d.ld); mix(d.Ip); mix(d.ldm); mix(d.nbk); mix(d.nq); mix(d.split);
    mix(d.fin_rows); mix(d.ksplit); off(d.kpart); off(d.kctr);
  }
  out[1] = h;
  h = kFnv;
  mix((long long)pl.tiles.size());
  for (const GemmTile& t : pl.tiles) {
    mix(t.prob); mix(t.tm); mix(t.tn); mix(t.first); mix(t.nk); mix(t.bm);
    off(t.P); off(t.M); off(t.U); off(t.eP); off(t.eM); mix(t.ld); mix(t.ldm);
    mix(t.k0); mix(t.np); mix(t.pc); mix(t.ser); off(t.part); off(t.ctr);
  }
  out[2] = h;
  h = kFnv;
  mix((long long)pl.list_off.size());
  for (int o : pl.list_off) mix(o);
  out[3] = h;
  h = kFnv;
  chunks(pl.sse_chunks); chunks(pl.fin_chunks);
  out[4] = h;
  h = kFnv;
  chunks(pl.hist_chunks); chunks(pl.hist_multi);
  out[5] = h;
  h = kFnv;
  units(pl.thin); units(pl.tl_units);
  mix((long long)pl.small.size());
  for (int j : pl.small) mix(j);
  out[6] = h;
  h = kFnv;
  off(pl.d_desc); off(pl.d_tiles); off(pl.d_list_off); off(pl.d_sse); off(pl.d_fin); off(pl.d_hist);
  off(pl.d_hist_multi); off(pl.d_small); off(pl.d_thin); off(pl.d_tl_units); off(pl.d_tl_sync);
  off(pl.d_ready); off(pl.d_kctr); off(pl.d_rank0); off(pl.d_groups);
  out[7] = h;
}

// ---------------------------------------------------------------------------
// The search form and the run's launch schedule

// The two-stage search needs the per-block threshold table in LDS; otherwise exhaustive.
static bool two_stage_ok(int ncand, int bits) {
  return ncand <= kMaxStage1 && bits <= kMaxStage1Bits && hist_lds_bytes(ncand, bits) <= 64 * 1024;
}

// Exact merged order of the level thresholds for (n, qmax) (k_mse_hist3): thr[k][c] is
// within a few ulps of (2k-1) ((n-1) + 5c) times a constant, so the integer keys give
// the order; rank0[e] for e = (k-1) n + c, and the groups of equal keys as
// {first rank, size, element indices...} padded to 6 entries. false: a tie group larger
// than 4 (the per-level stage 1 is used instead).
// rank0 is returned padded to kMaxMerged entries and followed by the coarse cell index
// lower bound lo[g], g = 0..kCells (see h3_setup): the number of thresholds whose cell
// (floor of threshold * kCells / largest threshold) is below g for EVERY mx. A
// threshold's cell is floor(z (1 + d)) with z = kCells key / key_max and |d| a few ulps
// (the float thresholds and the cell scale each within ~10 ulps of the key proportion),
// so counting the keys with z (1 + 1e-4) < g can only undercount.
static bool merged_tables(int n, int qmax, std::vector<unsigned short>& rank0, std::vector<unsigned short>& groups) {
  const int M = qmax * n;
  std::vector<std::pair<long long, int>> key(M);
  for (int k = 1; k <= qmax; ++k)
    for (int c = 0; c < n; ++c) key[(k - 1) * n + c] = {(long long)(2 * k - 1) * ((n - 1) + 5LL * c), (k - 1) * n + c};
  std::sort(key.begin(), key.end());
  rank0.assign(kMaxMerged + kCells + 2, 0);
  groups.clear();
  for (int r = 0; r < M;) {
    int r1 = r + 1;
    while (r1 < M && key[r1].first == key[r].first) ++r1;
    for (int j = r; j < r1; ++j) rank0[key[j].second] = (unsigned short)j;
    if (r1 - r > 1) {
      if (r1 - r > 4) return false;
      unsigned short g[6] = {(unsigned short)r, (unsigned short)(r1 - r), 0, 0, 0, 0};
      for (int j = r; j < r1; ++j) g[2 + j - r] = (unsigned short)key[j].second;
      groups.insert(groups.end(), g, g + 6);
    }
    r = r1;
  }
  const double kmax = (double)key[M - 1].first;
  int cnt = 0;
  for (int g = 0; g <= kCells; ++g) {
    while (cnt < M && (double)kCells * (double)key[cnt].first / kmax * (1.0 + 1e-4) < (double)g) ++cnt;
    rank0[kMaxMerged + g] = (unsigned short)cnt;
  }
  return true;
}

SearchForm search_form(int ncand, int bits, int qscheme, bool force_exhaustive, bool legacy_stage1) {
  SearchForm sf;
  sf.exhaustive = force_exhaustive || !two_stage_ok(ncand, bits);
  sf.merged = !sf.exhaustive && merged_ok(ncand, bits) && !legacy_stage1 && qscheme == kMse &&
              merged_tables(ncand, 1 << (bits - 1), sf.rank0, sf.groups);
  if (!sf.merged) { sf.rank0.clear(); sf.groups.clear(); }   // (a refused tie group leaves them half written)
  sf.ngroups = (int)sf.groups.size() / 6;
  return sf;
}

// the small jobs' search and finalize in one block each (k_mse_small_admm)
static bool small_jobs_fused(const AdmmPlan& pl, const SearchForm& sf, int qscheme, int ncand) {
  return qscheme == kMse && !sf.exhaustive && sf.merged && !pl.small.empty() && pl.small_groups > 0 && ncand <= 1024;
}
// stage-1 units of the big jobs: the blocks of a search launch with the finalize fused
static int fin_blocks(const AdmmPlan& pl, bool fuse_small) {
  return fuse_small ? pl.nhist_big : (int)pl.hist_chunks.size();
}

bool fin_capacity_wanted(const AdmmPlan& pl, const SearchForm& sf, int qscheme, int ncand, bool fused_allowed) {
  return fused_allowed && qscheme == kMse && !sf.exhaustive && sf.merged && pl.rows_aligned &&
         fin_blocks(pl, small_jobs_fused(pl, sf, qscheme, ncand)) > 0;
}

RunSchedule schedule_run(const AdmmPlan& pl, const SearchForm& sf, const RunSwitches& sw, int qscheme, int bits,
                         int ncand, int max_iter, bool fused_allowed, int fin_capacity) {
  RunSchedule rs;
  rs.iters = std::max(max_iter - 1, 0);
  rs.zero_kctr = pl.nkctr > 0;
  rs.fuse_small = small_jobs_fused(pl, sf, qscheme, ncand);
  // the big jobs' finalize inside the search launch when all its blocks fit at once
  // (with a margin of one resident block per CU: see hist3_fin_capacity): one whole-row
  // unit per block, all blocks resident; a launch with more units than that takes the
  // separate finalize launch (round 3 measured blocks taking several units each with the
  // finalize fused: no faster at C4, 324 vs 318 ms per sweep, and that path held the fused
  // kernel at 40 spilled VGPRs)
  rs.fin_wanted = fin_capacity_wanted(pl, sf, qscheme, ncand, fused_allowed);
  const int fin_cap = !rs.fin_wanted ? 0 : (sw.fin_cap_override > 0 ? std::min(sw.fin_cap_override, fin_capacity) : fin_capacity);
  const int nfin_blocks = fin_blocks(pl, rs.fuse_small);
  const bool fuse_fin = rs.fin_wanted && fin_cap > 0 && nfin_blocks <= fin_cap;
  rs.zero_ready = fuse_fin;
  // every problem thin: all iterations in one persistent launch (k_thin_loop) when the
  // fused paths are allowed (the op's fault retry turns them off) and it fits the device
  rs.try_thin_loop = pl.tl_ok && sw.thin_loop != 0 && fused_allowed && qscheme == kMse && !sf.exhaustive &&
                     max_iter > 1 && ncand >= 2 && ncand <= kTLMaxCand && bits >= 2 && bits <= 5;
  rs.gemm = pl.ntiles_wide + pl.ntiles_small + pl.ntiles_big + pl.nslots + pl.ntiles_f32t > 0;
  rs.gemm_diag = pl.nslots + pl.ntiles_f32t > 0;
  rs.thin_solve = !pl.thin.empty();
  if (qscheme == kMse) {
    if (sf.exhaustive) {
      rs.search = kSearchAll;
    } else if (!sf.merged) {
      rs.search = kSearchHist;
      rs.nh = (int)pl.hist_chunks.size();
    } else {
      // two-stage: stage 1, the selection and (when |S| > 1) stage 2 all in the hist launch;
      // fused finalize: one whole-row unit per block; otherwise possibly several units per block
      rs.nh = fuse_fin ? nfin_blocks : (rs.fuse_small ? pl.nhm_big : (int)pl.hist_multi.size());
      if (rs.nh > 0) {
        rs.search = fuse_fin ? kSearchHist3Fin : kSearchHist3;
        rs.search_multi = !fuse_fin;
      }
    }
  }
  // fused: every job's finalize ran in the search launch (big jobs) or the small-job kernel
  rs.nf = fuse_fin ? 0 : (rs.fuse_small ? pl.nfin_big : (int)pl.fin_chunks.size());
  return rs;
}
}  // namespace admmq
