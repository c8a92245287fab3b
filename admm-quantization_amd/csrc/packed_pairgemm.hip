// Fused 2-way packed layer (include/admmq.h "Fused packed pair"): a back-to-back
// GEMM from two packed code streams, Y = D2 q_mid(D1 X) (+ bias), then the output quantizer.
// D1 [R, K] and D2 [M, R] are the table de-quantizations of two packed tensors (D1 optionally
// the transpose of a [K, R] tensor), each with a meta record of its own (any bits 1..8, any of
// the four tensor schemes, independently). The rank-R tensor t = D1 X between the two products
// lives in LDS only: it is never stored to memory, and the layer is one launch with no workspace.
//
// Work split. The batch and the positions form one column axis c in [0, C), C = nb N, as in
// k_packed_gemm. A workgroup (256 threads, 4 waves) owns one tile of NT (64 or 32) columns and
// one contiguous range of 64-row M tiles (blockIdx.y of `ms` splits; every split recomputes
// phase 1 for its columns - the planner only splits onto CUs that would otherwise idle).
//
//   Phase 1: t [Rp, NT] = D1 X over all of K in increasing 32-steps (Rp = R rounded up to 32).
//     A step's D1 block (Rp x 32, decoded from runs of 8 stream-consecutive codes cut out of
//     three dwords, along k for trans1 = 0 and along r for 1) and X block (32 x NT) are staged
//     k-major in a two-buffer LDS ring; the next step's global loads are issued before the
//     current step's MFMAs and stored behind them. A wave owns one 32-column block and every
//     (4 / (NT / 32))-th 32-row block of t: at most 4 accumulators of v_mfma_f32_32x32x2_f32,
//     64 VGPRs, at R = 256 and NT = 64. One chain per output over increasing k: no K split.
//   Park: the mid quantizer (fixed_quant, real rows only) is applied in registers and the tile
//     is written to LDS r-major, P[r][c] - the k-major B operand image of phase 2.
//   Phase 2: per M tile, Y [64, NT] = D2 t over R in increasing 32-steps: the D2 block
//     (64 x 32) is decoded into the ring (which reuses phase 1's staging), the B operand is
//     read from the parked tile; then bias, the output quantizer and the store. x_layout 1
//     swaps the MFMA operands so that the lanes of the result run along m, Y's contiguous axis.
//     With NT = 32 only two waves hold a 32 x 32 block of a 64-row tile; the other two decode.
//
// LDS (dynamic, floats): Rp (NT + 1) parked + max(2 * 32 (Rp + 1) + 2 * 32 (NT + 1), 2 * 32 * 65)
// staging: 148992 bytes at R = 256, NT = 64, so one workgroup per CU there.
//
// Every output's chain is a function of its own column of X and its own row of D2: zero padding
// (rows past R, k past K, columns past C) enters as exact +0 products. The bits therefore do not
// depend on N, NT, ms or the batch index. They are not those of two admmq_packed_gemm calls,
// whose first stage may cut K into pieces.
#include <algorithm>

#include "../../include/admmq.h"
#include "packed_tile.h"

namespace admmq {

constexpr int kPpBK = 32;                 // the K step of phase 1 and the R step of phase 2
constexpr int kPpRMax = 256;              // R at most (RANK_MAX of the Python layer)
constexpr int kPpCUs = 256;               // workgroups the M split fills up to (one per CU)
constexpr int kPpHalfFill = 128;          // 64-column tiles below which the 32-column tile is taken
constexpr int kPpLD2 = kPackedBM + 1;     // row stride of phase 2's D2 image
constexpr int64_t kPpKMax = int64_t(1) << 24;

typedef float pp_f32x16 __attribute__((ext_vector_type(16)));

struct PpWeight {
  const unsigned char* codes;
  long long nbytes;
  int bits, scheme, zp;
  float scale, mn, rng;
};

struct PpArgs {
  PpWeight w1, w2;
  const float* x;
  const float* bias;
  float* y;
  long long C;
  int M, K, N, R, Rp;
  int mt;             // M tiles per split
  int mq_on, oq_on;
  ActQ mq, oq;
};

// The three dwords from dword bit0 >> 5 on: they hold a run of 8 codes (<= 64 bits) that starts
// at stream bit bit0. Nothing past the stream's last byte is read; any = false reads nothing.
__device__ __forceinline__ void pp_load_run(const PpWeight& w, long long bit0, bool any, unsigned* cw) {
  cw[0] = 0u; cw[1] = 0u; cw[2] = 0u;
  if (!any) return;
  const long long wq = bit0 >> 5;
  if (4 * wq + 12 <= w.nbytes) {
    const gcu32* q = (const gcu32*)(w.codes + 4 * wq);
    cw[0] = q[0]; cw[1] = q[1]; cw[2] = q[2];
  } else {
    cw[0] = code_dword(w.codes, wq, w.nbytes);
    cw[1] = code_dword(w.codes, wq + 1, w.nbytes);
    cw[2] = code_dword(w.codes, wq + 2, w.nbytes);
  }
}

// The run's 8 de-quantized codes; code j lies at bit wsh + j bits of (cw2 : cw1 : cw0). Codes
// from nv on are exactly 0 (past the row, K, R or the matrix).
__device__ __forceinline__ void pp_decode_run(const PpWeight& w, const unsigned* cw, int wsh, int nv, float* d) {
  const unsigned mask = (1u << w.bits) - 1u;
  unsigned u[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int p = wsh + j * w.bits;   // <= 31 + 56
    const int idx = p >> 5;
    const unsigned lo = idx == 0 ? cw[0] : (idx == 1 ? cw[1] : cw[2]);
    const unsigned hi = idx == 0 ? cw[1] : (idx == 1 ? cw[2] : 0u);
    u[j] = (unsigned)(((((unsigned long long)hi) << 32) | lo) >> (p & 31)) & mask;
  }
  if (w.scheme == kMinMax) {   // (one uniform branch per run, not one per code)
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = dequant_code(u[j], kMinMax, w.bits, w.scale, w.zp, w.mn, w.rng);
  } else {                     // mse-minmax / symmetric: the affine form with zero_point 0
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = dequant_code(u[j], kAffine, w.bits, w.scale, w.zp, w.mn, w.rng);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) d[j] = j < nv ? d[j] : 0.f;
}

template <int NT, bool TRANS, bool XL>
__global__ __launch_bounds__(256) void k_packed_pairgemm(const PpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float pp_lds[];
  constexpr int CB = NT / 32;        // 32-column blocks of the tile
  constexpr int WR = 4 / CB;         // waves along the rows of t
  constexpr int NQ = 8 / WR;         // 32-row blocks of t per wave at most
  constexpr int NJ = NT / 8;         // X elements per thread and step
  constexpr int LDX = NT + 1, LDP = NT + 1;
  constexpr int XKS = 256 / NT;      // layout 0: the k stride of a thread's X elements
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave % CB, wr = wave / CB, i = lane & 31, h = lane >> 5;
  const int M = a.M, K = a.K, N = a.N, R = a.R, Rp = a.Rp;
  const long long C = a.C;
  const long long c0 = (long long)blockIdx.x * NT;
  const int LDW = Rp + 1;
  float* const sP = pp_lds;                    // [Rp][LDP] the parked tile
  float* const sS = pp_lds + Rp * LDP;         // staging: phase 1 W [2][32][LDW] + X [2][32][LDX]; phase 2 D2 [2][32][kPpLD2]
  float* const sW = sS;
  float* const sX = sS + 2 * kPpBK * LDW;

  // ---- phase 1: t = D1 X ---------------------------------------------------------------------
  // W: runs id = tid + 256 j < 4 Rp of a step's Rp x 32 block. trans1 = 0: row id >> 2, k offset
  // 8 (id & 3); trans1 = 1: k offset id / (Rp / 8), rows 8 (id % (Rp / 8)) on.
  const int nruns = 4 * Rp;
  int wrow[4], wk[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int id = tid + 256 * j;
    if (TRANS) {
      const int octs = Rp >> 3;
      wk[j] = id / octs;
      wrow[j] = 8 * (id - wk[j] * octs);
    } else {
      wrow[j] = id >> 2;
      wk[j] = 8 * (id & 3);
    }
  }
  // X: NJ elements of the step's 32 x NT block; layout 0: one column, k = xk + XKS j;
  // layout 1: one k, columns xc + 8 j. Columns past C read a clamped (valid) address and are zeroed.
  const int xc = XL ? (tid >> 5) : (tid % NT);
  const int xk = XL ? (tid & 31) : (tid / NT);
  long long xo[NJ];
  unsigned xok = 0u;
  const float* __restrict__ xp;
  if (XL) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const long long c = c0 + xc + 8 * j;
      if (c < C) xok |= 1u << j;
      xo[j] = min(c, C - 1) * K;
    }
    xp = a.x + xk;
  } else {
    const long long c = min(c0 + xc, C - 1);
    if (c0 + xc < C) xok = (1u << NJ) - 1u;
    const long long b = c / N;
#pragma unroll
    for (int j = 0; j < NJ; ++j) xo[j] = (long long)(XKS * j) * N;
    xp = a.x + (b * K * N + (c - b * N)) + (long long)xk * N;
  }
  const long long xstep = XL ? kPpBK : (long long)kPpBK * N;

  unsigned cw[4][3];
  int wsh[4], nv[4];
  float rx[NJ];
  auto load1 = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      nv[j] = 0;
      wsh[j] = 0;
      long long bit0 = 0;
      if (tid + 256 * j < nruns) {
        const int k = k0 + wk[j];
        if (TRANS) nv[j] = k < K ? min(8, R - wrow[j]) : 0;
        else nv[j] = wrow[j] < R ? min(8, K - k) : 0;
        bit0 = (TRANS ? (long long)k * R + wrow[j] : (long long)wrow[j] * K + k) * a.w1.bits;
        wsh[j] = (int)(bit0 & 31);
      }
      pp_load_run(a.w1, bit0, nv[j] > 0, cw[j]);
    }
    const gcf32* xg = (const gcf32*)xp;
    const bool full = k0 + kPpBK <= K;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const bool ok = ((xok >> j) & 1u) != 0u;
      if (full) {   // no k test: the load is taken whatever the column mask says (a valid address)
        const float v = xg[xo[j]];
        rx[j] = ok ? v : 0.f;
      } else {
        const int k = XL ? k0 + xk : k0 + xk + XKS * j;
        rx[j] = (ok && k < K) ? xg[xo[j]] : 0.f;
      }
    }
    xp += xstep;
  };
  auto store1 = [&](int buf) __attribute__((always_inline)) {
    float* const w = sW + buf * kPpBK * LDW;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (tid + 256 * j < nruns) {
        float d[8];
        pp_decode_run(a.w1, cw[j], wsh[j], nv[j], d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (TRANS) w[wk[j] * LDW + wrow[j] + e] = d[e];
          else w[(wk[j] + e) * LDW + wrow[j]] = d[e];
        }
      }
    }
    float* const x = sX + buf * kPpBK * LDX;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (XL) x[xk * LDX + xc + 8 * j] = rx[j];
      else x[(xk + XKS * j) * LDX + xc] = rx[j];
    }
  };

  pp_f32x16 acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
  load1(0);
  store1(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < K; k0 += kPpBK) {
    const bool more = k0 + kPpBK < K;
    if (more) load1(k0 + kPpBK);
    const float* w = sW + buf * kPpBK * LDW + i;
    const float* x = sX + buf * kPpBK * LDX + 32 * wn + i;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int rb = wr + WR * q;
      if (32 * rb < Rp) {   // (uniform over the wave)
#pragma unroll
        for (int s = 0; s < kPpBK / 2; ++s)
          acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[(2 * s + h) * LDW + 32 * rb], x[(2 * s + h) * LDX], acc[q], 0, 0, 0);
      }
    }
    if (more) store1(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // ---- park: q_mid(t) into LDS, r-major. Only real rows are quantized: q(0) is not 0 unless 0
  // lies on the grid, and the rows past R must stay exactly 0.
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int rb = wr + WR * q;
    if (32 * rb < Rp) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * rb + PACKED_ROW(r);
        float v = acc[q][r];
        if (a.mq_on) {
          const float vq = fixed_quant(v, a.mq);
          v = row < R ? vq : 0.f;
        }
        sP[row * LDP + 32 * wn + i] = v;
      }
    }
  }
  // (phase 1's last step ended with a barrier: its staging is free; the parked tile is read
  // after phase 2's first barrier)

  // ---- phase 2: Y = D2 t per M tile ------------------------------------------------------------
  float* const sD = sS;   // [2][32][kPpLD2], k (= r) major
  const int wm = wave / CB;
  const bool active = wm < kPackedBM / 32;
  const int drow = tid >> 2, dk = 8 * (tid & 3);
  const int tm = (M + kPackedBM - 1) / kPackedBM;
  const int t0 = (int)blockIdx.y * a.mt, t1 = min(tm, t0 + a.mt);
  const float* __restrict__ bias = a.bias;
  for (int t = t0; t < t1; ++t) {
    const int m0 = t * kPackedBM;
    unsigned dw[3];
    int dsh = 0, dnv = 0;
    auto load2 = [&](int r0) __attribute__((always_inline)) {
      const int m = m0 + drow, r = r0 + dk;
      dnv = m < M ? min(8, R - r) : 0;
      const long long bit0 = dnv > 0 ? ((long long)m * R + r) * a.w2.bits : 0;
      dsh = (int)(bit0 & 31);
      pp_load_run(a.w2, bit0, dnv > 0, dw);
    };
    auto store2 = [&](int b) __attribute__((always_inline)) {
      float d[8];
      pp_decode_run(a.w2, dw, dsh, dnv, d);
#pragma unroll
      for (int e = 0; e < 8; ++e) sD[b * kPpBK * kPpLD2 + (dk + e) * kPpLD2 + drow] = d[e];
    };
    pp_f32x16 y;
#pragma unroll
    for (int r = 0; r < 16; ++r) y[r] = 0.f;
    load2(0);
    store2(0);
    __syncthreads();
    buf = 0;
    for (int r0 = 0; r0 < Rp; r0 += kPpBK) {
      const bool more = r0 + kPpBK < Rp;
      if (more) load2(r0 + kPpBK);
      if (active) {
        const float* w = sD + buf * kPpBK * kPpLD2 + 32 * wm + i;
        const float* p = sP + r0 * LDP + 32 * wn + i;
#pragma unroll
        for (int s = 0; s < kPpBK / 2; ++s) {
          if (XL) y = __builtin_amdgcn_mfma_f32_32x32x2f32(p[(2 * s + h) * LDP], w[(2 * s + h) * kPpLD2], y, 0, 0, 0);
          else y = __builtin_amdgcn_mfma_f32_32x32x2f32(w[(2 * s + h) * kPpLD2], p[(2 * s + h) * LDP], y, 0, 0, 0);
        }
      }
      if (more) store2(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
    if (!active) continue;
    if (XL) {   // lanes along m, rows along the columns: Y[c M + m]
      const int m = m0 + 32 * wm + i;
      if (m < M) {
        const float bv = bias ? bias[m] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const long long c = c0 + 32 * wn + PACKED_ROW(r);
          float v = bias ? y[r] + bv : y[r];
          if (a.oq_on) v = fixed_quant(v, a.oq);
          if (c < C) a.y[c * M + m] = v;
        }
      }
    } else {    // lanes along the columns: Y[(b M + m) N + n]
      const long long c = c0 + 32 * wn + i;
      if (c < C) {
        const long long b = c / N;
        const long long ybase = b * M * N + (c - b * N);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + 32 * wm + PACKED_ROW(r);
          if (m < M) {
            float v = bias ? y[r] + bias[m] : y[r];
            if (a.oq_on) v = fixed_quant(v, a.oq);
            a.y[ybase + (long long)m * N] = v;
          }
        }
      }
    }
  }
}

// --- host -------------------------------------------------------------------------------------------

// The plan of one call (include/admmq.h states the rule): a function of the sizes alone.
struct PairPlan {
  int ntile, ms, mt, Rp;
  long long tn, tm, C;
  size_t lds;
};

static const char* const kPpRankText =
    "R must be 1..256 (the rank-R tile is held in LDS; a larger rank keeps the two-stage route)";

// ADMMQ_OK, or the code of the refusal with *what set to its text
static int plan_pair(int64_t M, int64_t K, int64_t N, int64_t nb, int64_t R, PairPlan& pl, const char** what) {
  if (R < 1 || R > kPpRMax) { *what = kPpRankText; return ADMMQ_ERR_ARG; }
  if (M <= 0 || K <= 0 || N <= 0 || nb <= 0) { *what = "M, K, N and nb must be positive"; return ADMMQ_ERR_ARG; }
  if (M > (int64_t(1) << 22) || K > kPpKMax || N > (int64_t(1) << 30) || nb > (int64_t(1) << 30) ||
      nb * N > (int64_t(1) << 30)) {
    *what = "sizes out of range";
    return ADMMQ_ERR_ARG;
  }
  pl.C = nb * N;
  pl.tm = (M + kPackedBM - 1) / kPackedBM;
  pl.ntile = (pl.C + 63) / 64 < kPpHalfFill ? 32 : 64;
  pl.tn = (pl.C + pl.ntile - 1) / pl.ntile;
  const long long want = std::max<long long>(1, std::min<long long>(pl.tm, kPpCUs / pl.tn));
  pl.mt = (int)((pl.tm + want - 1) / want);
  pl.ms = (int)((pl.tm + pl.mt - 1) / pl.mt);
  pl.Rp = (int)((R + 31) / 32 * 32);
  const size_t stage1 = (size_t)2 * kPpBK * (pl.Rp + 1) + (size_t)2 * kPpBK * (pl.ntile + 1);
  const size_t stage2 = (size_t)2 * kPpBK * kPpLD2;
  pl.lds = sizeof(float) * ((size_t)pl.Rp * (pl.ntile + 1) + std::max(stage1, stage2));
  return ADMMQ_OK;
}

static bool pp_actq_on(const admmq_actq* q) { return q && q->on != 0; }

static PpWeight pp_weight(const uint8_t* codes, const admmq_qmeta* meta, int64_t numel) {
  PpWeight w;
  w.codes = codes;
  w.nbytes = (long long)admmq_packed_bytes(numel, meta->bits);
  w.bits = meta->bits;
  w.scheme = meta->scheme;
  w.zp = meta->scheme == kAffine ? meta->zero_point : 0;   // (the other schemes' table has none)
  w.scale = meta->scale; w.mn = meta->mn; w.rng = meta->rng;
  return w;
}

template <int NT, bool TRANS, bool XL>
static hipError_t pp_launch(const PpArgs& a, const PairPlan& pl, hipStream_t s) {
  const void* kern = reinterpret_cast<const void*>(k_packed_pairgemm<NT, TRANS, XL>);
  if (pl.lds > 64 * 1024) {   // past the static limit: raise the kernel's dynamic LDS bound
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_packed_pairgemm<NT, TRANS, XL>), dim3((unsigned)pl.tn, (unsigned)pl.ms), dim3(256), pl.lds, s, a);
  return hipGetLastError();
}

}  // namespace admmq

using namespace admmq;

extern "C" {

int32_t admmq_packed_pairgemm_plan(int64_t M, int64_t K, int64_t N, int64_t nb, int64_t R, int32_t* out) {
  const char* const who = "packed_pairgemm_plan";
  if (!out) return packed_fail(who, ADMMQ_ERR_ARG, "out must not be NULL");
  PairPlan pl;
  const char* what = "";
  const int rc = plan_pair(M, K, N, nb, R, pl, &what);
  if (rc != ADMMQ_OK) return packed_fail(who, rc, what);
  out[0] = pl.ntile;
  out[1] = pl.ms;
  out[2] = (int32_t)pl.lds;
  out[3] = (int32_t)(pl.tn * pl.ms);
  return ADMMQ_OK;
}

int32_t admmq_packed_pairgemm(const uint8_t* codes1, const admmq_qmeta* meta1, int32_t trans1, const uint8_t* codes2,
                              const admmq_qmeta* meta2, int64_t M, int64_t K, int64_t R, const float* x, int32_t x_layout,
                              int64_t N, int32_t nb, const float* bias, float* y, const admmq_actq* mid_q,
                              const admmq_actq* out_q, void* stream) {
  const char* const who = "packed_pairgemm";
  if (!codes1 || !meta1 || !codes2 || !meta2 || !x || !y)
    return packed_fail(who, ADMMQ_ERR_ARG, "codes1, meta1, codes2, meta2, x and y must not be NULL");
  PairPlan pl;
  const char* what = "";
  int32_t rc = plan_pair(M, K, N, nb, R, pl, &what);
  if (rc != ADMMQ_OK) return packed_fail(who, rc, what);
  rc = packed_meta_check(meta1, who, false, nullptr);
  if (rc != ADMMQ_OK) return rc;
  rc = packed_meta_check(meta2, who, false, nullptr);
  if (rc != ADMMQ_OK) return rc;
  if (trans1 != 0 && trans1 != 1) return packed_fail(who, ADMMQ_ERR_ARG, "trans1 must be 0 or 1");
  if (x_layout != 0 && x_layout != 1) return packed_fail(who, ADMMQ_ERR_ARG, "x_layout must be 0 or 1");
  if (x_layout == 1 && nb != 1) return packed_fail(who, ADMMQ_ERR_ARG, "x_layout 1 (linear) needs nb = 1");
  if (((reinterpret_cast<uintptr_t>(codes1) | reinterpret_cast<uintptr_t>(codes2)) & 15) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "codes1 and codes2 must be 16-byte aligned");
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(bias)) & 3) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "x, y and bias must be float aligned");
  if (pp_actq_on(mid_q) && (mid_q->bits < 1 || mid_q->bits > 24))
    return packed_fail(who, ADMMQ_ERR_ARG, "mid_q bits must be 1..24");
  if (pp_actq_on(out_q) && (out_q->bits < 1 || out_q->bits > 24))
    return packed_fail(who, ADMMQ_ERR_ARG, "out_q bits must be 1..24");
  PpArgs a;
  a.w1 = pp_weight(codes1, meta1, R * K);
  a.w2 = pp_weight(codes2, meta2, M * R);
  a.x = x; a.bias = bias; a.y = y;
  a.C = pl.C;
  a.M = (int)M; a.K = (int)K; a.N = (int)N; a.R = (int)R; a.Rp = pl.Rp;
  a.mt = pl.mt;
  a.mq_on = pp_actq_on(mid_q) ? 1 : 0;
  a.oq_on = pp_actq_on(out_q) ? 1 : 0;
  a.mq = a.mq_on ? actq_make(mid_q) : ActQ{0.f, 0.f, 0.f, 0};
  a.oq = a.oq_on ? actq_make(out_q) : ActQ{0.f, 0.f, 0.f, 0};
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t err;
#define ADMMQ_PP_FORM(NT)                                                    \
  (trans1 ? (x_layout ? pp_launch<NT, true, true>(a, pl, s) : pp_launch<NT, true, false>(a, pl, s)) \
          : (x_layout ? pp_launch<NT, false, true>(a, pl, s) : pp_launch<NT, false, false>(a, pl, s)))
  if (pl.ntile == 32) err = ADMMQ_PP_FORM(32);
  else err = ADMMQ_PP_FORM(64);
#undef ADMMQ_PP_FORM
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

}  // extern "C"
