// The Krylov block step between the panel products (admmq.lowrank.KrylovProjector, fused
// route): one Cholesky-QR pass and one re-orthogonalisation pass, each in
// one launch, so that a block runs on this library's kernels only.
//
//   admmq_cholqr64        Q = Z L^-T,  L L^T = G + shift_scale tr(G) I   (Z, Q: m x k, k <= 64)
//   admmq_panel_reorth64  Zout = Z - K C                                 (K: m x p, C: p x k)
//
// k_cholqr64. One wave per workgroup, lane = row, 64 rows of Z per workgroup. There is no
// hand-off: every wave factors G itself. Lane r holds row r of G (then of its Schur
// complements) in registers; step j takes the pivot from lane j (v_readlane), divides
// column j, publishes it as L's column j in LDS (lane-contiguous, so conflict-free) and
// every lane subtracts l[r][j] l[c][j] from its row, reading l[c][j] at compile-time LDS
// addresses (a broadcast). The triangular solve is the same recurrence on a row of Z:
// q_j = z_j / L[j][j], then z_c -= q_j L[c][j] for c > j, which adds the terms of
// q_c = (z_c - sum_{i<c} q_i L[c][i]) / L[c][c] in the order i = 0, 1, ... All of it is
// fp64 on the VALU with correctly rounded sqrt and division (no reciprocals: the pass is
// compared element by element with a LAPACK factorisation). The matrix instructions do not
// fit: k^3 / 3 + m k^2 flops (36 MFLOP at 4096 x 64) behind a serial chain of k pivots.
// The only barriers are wave-local (a workgroup is one wave). KB (k rounded up to 16) is a
// template parameter: every register index is a constant, nothing goes to scratch; rows
// and columns past k are those of the identity. A pivot that is not > 0 (NaN included)
// changes no control flow: the steps run on, Q is filled with NaN and *info set.
//
// k_panel_reorth64. A workgroup owns 64 rows, wave w the 16-row strip w. The accumulators
// (NT = ceil(k / 16) tiles of v_mfma_f64_16x16x4_f64) start as the Z tile; C is negated as
// it is staged, so D = Z + K (-C) with exact negations. K's 64 x 32 slab and C's 32 x k
// chunk of a p-chunk go through LDS, double-buffered (the next chunk's global loads are
// issued before this chunk's MFMAs, stored after them: one barrier per chunk); both are
// loaded row-contiguous, 16 bytes per lane where the strides and pointers allow. The LDS
// row strides (34 and 80 doubles) keep the A reads (lane -> row) and the B reads (lane ->
// column, 4 rows) of each half-wave on distinct banks. The p-sum runs in index order per
// output, fixed by the shapes. Tails in m, p and k are staged as zeros.
#include <cstdint>

#include "../../include/admmq.h"
#include "admmq_internal.h"

namespace admmq {

typedef double f64x4o __attribute__((ext_vector_type(4)));
typedef double f64x2o __attribute__((ext_vector_type(2)));

static_assert(ADMMQ_CHOLQR_K_MAX == 64, "k_cholqr64: one lane per row of G");

__device__ __forceinline__ double lane_bcast(double x, int l) {
  const long long v = __double_as_longlong(x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// grid ceil(m / 64), 64 threads. Q may be Z: a lane reads its whole row before it writes it.
template <int KB>
__global__ __launch_bounds__(64) void k_cholqr64(const double* Z, int ldz, int m, int k, const double* __restrict__ G,
                                                 double shift_scale, double* Q, int ldq, int* info) {
  __shared__ double Lc[KB * KB];   // L by columns: Lc[j * KB + r] = L[r][j], r >= j
  const int lane = threadIdx.x;
  const int row = blockIdx.x * 64 + lane;
  const bool live = row < m;
  // row `lane` of G; past k the identity
  double g[KB];
  {
    const bool gl = lane < k;
    const double* gr = G + (size_t)(gl ? lane : 0) * k;
    const bool v2 = (k & 1) == 0 && (reinterpret_cast<uintptr_t>(G) & 15) == 0;
#pragma unroll
    for (int c = 0; c < KB; c += 2) {
      g[c] = lane == c ? 1.0 : 0.0; g[c + 1] = lane == c + 1 ? 1.0 : 0.0;
      if (gl && v2 && c + 1 < k) {
        const f64x2o t = *reinterpret_cast<const f64x2o*>(gr + c);
        g[c] = t[0]; g[c + 1] = t[1];
      } else if (gl) {
        if (c < k) g[c] = gr[c];
        if (c + 1 < k) g[c + 1] = gr[c + 1];
      }
    }
  }
  // trace in index order (the same bits in every workgroup), then the shifted diagonal
  double diag = 0.0;
#pragma unroll
  for (int c = 0; c < KB; ++c) diag = lane == c ? g[c] : diag;
  if (lane < KB) Lc[lane] = lane < k ? diag : 0.0;
  __syncthreads();
  double tr = 0.0;
#pragma unroll
  for (int c = 0; c < KB; ++c) tr += Lc[c];
  __syncthreads();
  const double shift = shift_scale * tr;
#pragma unroll
  for (int c = 0; c < KB; ++c) g[c] = (lane == c && lane < k) ? g[c] + shift : g[c];
  // right-looking Cholesky, one column per step
  bool bad = false;
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    const double d = lane_bcast(g[j], j);
    bad = bad || !(d > 0.0);
    const double ljj = sqrt(d);
    const double l = lane == j ? ljj : g[j] / ljj;
    if (lane < KB) Lc[j * KB + lane] = l;
    __syncthreads();
#pragma unroll
    for (int c = j + 1; c < KB; ++c) g[c] = fma(-l, Lc[j * KB + c], g[c]);
  }
  // this lane's row of Z (loaded only now: with g[] live as well, KB = 64 would spill), then the
  // forward substitution (Lc is complete: the last step's barrier)
  double z[KB];
  {
    const double* zr = Z + (size_t)(live ? row : 0) * ldz;
    const bool v2 = (ldz & 1) == 0 && (reinterpret_cast<uintptr_t>(Z) & 15) == 0;
#pragma unroll
    for (int c = 0; c < KB; c += 2) {
      z[c] = 0.0; z[c + 1] = 0.0;
      if (live && v2 && c + 1 < k) {
        const f64x2o t = *reinterpret_cast<const f64x2o*>(zr + c);
        z[c] = t[0]; z[c + 1] = t[1];
      } else if (live) {
        if (c < k) z[c] = zr[c];
        if (c + 1 < k) z[c + 1] = zr[c + 1];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    const double q = z[j] / Lc[j * KB + j];
    z[j] = q;
#pragma unroll
    for (int c = j + 1; c < KB; ++c) z[c] = fma(-q, Lc[j * KB + c], z[c]);
  }
  if (bad) {
    if (info && blockIdx.x == 0 && lane == 0) *info = 1;
#pragma unroll
    for (int c = 0; c < KB; ++c) z[c] = __builtin_nan("");
  }
  if (!live) return;
  double* qr = Q + (size_t)row * ldq;
  const bool w2 = (ldq & 1) == 0 && (reinterpret_cast<uintptr_t>(Q) & 15) == 0;
#pragma unroll
  for (int c = 0; c < KB; c += 2) {
    if (w2 && c + 1 < k) {
      *reinterpret_cast<f64x2o*>(qr + c) = f64x2o{z[c], z[c + 1]};
    } else {
      if (c < k) qr[c] = z[c];
      if (c + 1 < k) qr[c + 1] = z[c + 1];
    }
  }
}

constexpr int kReRows = 64;    // rows of a workgroup (16 per wave)
constexpr int kReChunk = 32;   // p-values per LDS stage
constexpr int kReLdK = 34;     // LDS row stride of the K slab (doubles)
constexpr int kReLdC = 80;     // LDS row stride of the C chunk (doubles)

// grid ceil(m / 64), 256 threads. Zout may be Z: a lane reads and writes the same elements.
template <int NT>
__global__ __launch_bounds__(256) void k_panel_reorth64(const double* __restrict__ K, int ldk, int m, int p,
                                                        const double* __restrict__ C, int ldc, const double* Z, int ldz,
                                                        int k, double* Zout, int ldo) {
  __shared__ __attribute__((aligned(16))) double Ks[2][kReRows * kReLdK];
  __shared__ __attribute__((aligned(16))) double Cs[2][kReChunk * kReLdC];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int i0 = blockIdx.x * kReRows;
  const bool kv2 = (ldk & 1) == 0 && (reinterpret_cast<uintptr_t>(K) & 15) == 0;
  const bool cv2 = (ldc & 1) == 0 && (reinterpret_cast<uintptr_t>(C) & 15) == 0;
  // a thread's share of a stage: 4 pairs of the K slab (64 x 16 pairs), 4 pairs of the C chunk
  // (32 rows x 32 pairs, the columns past 16 NT skipped)
  f64x2o kreg[4], creg[4];
  auto fetch = [&](int p0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int u = tid + 256 * e;
      {
        const int r = i0 + (u >> 4), c = p0 + 2 * (u & 15);
        f64x2o t = {0.0, 0.0};
        if (r < m) {
          const double* src = K + (size_t)r * ldk + c;
          if (kv2 && c + 1 < p) {
            t = *reinterpret_cast<const f64x2o*>(src);
          } else {
            if (c < p) t[0] = src[0];
            if (c + 1 < p) t[1] = src[1];
          }
        }
        kreg[e] = t;
      }
      {
        const int r = p0 + (u >> 5), c = 2 * (u & 31);
        f64x2o t = {0.0, 0.0};
        if (r < p && c < 16 * NT) {
          const double* src = C + (size_t)r * ldc + c;
          if (cv2 && c + 1 < k) {
            t = *reinterpret_cast<const f64x2o*>(src);
          } else {
            if (c < k) t[0] = src[0];
            if (c + 1 < k) t[1] = src[1];
          }
        }
        creg[e] = -t;
      }
    }
  };
  auto stage = [&](int b) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int u = tid + 256 * e;
      *reinterpret_cast<f64x2o*>(&Ks[b][(u >> 4) * kReLdK + 2 * (u & 15)]) = kreg[e];
      if (2 * (u & 31) < 16 * NT) *reinterpret_cast<f64x2o*>(&Cs[b][(u >> 5) * kReLdC + 2 * (u & 31)]) = creg[e];
    }
  };
  fetch(0);
  // D map: column 16 t + (lane & 15), row 16 w + (lane >> 4) + 4 v
  f64x4o acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = 16 * t + fr;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = i0 + 16 * w + fk + 4 * v;
      acc[t][v] = (r < m && c < k) ? Z[(size_t)r * ldz + c] : 0.0;
    }
  }
  stage(0);
  __syncthreads();
  const int nch = (p + kReChunk - 1) / kReChunk;
  for (int ch = 0; ch < nch; ++ch) {
    const int b = ch & 1;
    if (ch + 1 < nch) fetch((ch + 1) * kReChunk);
    const double* ks = &Ks[b][(16 * w + fr) * kReLdK + fk];
    const double* cs = &Cs[b][fk * kReLdC + fr];
#pragma unroll
    for (int s = 0; s < kReChunk / 4; ++s) {
      const double a = ks[4 * s];
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, cs[4 * s * kReLdC + 16 * t], acc[t], 0, 0, 0);
    }
    if (ch + 1 < nch) stage(b ^ 1);   // (its last readers passed the barrier that ended chunk ch - 1)
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = 16 * t + fr;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = i0 + 16 * w + fk + 4 * v;
      if (r < m && c < k) Zout[(size_t)r * ldo + c] = acc[t][v];
    }
  }
}

}  // namespace admmq

using namespace admmq;

extern "C" {

int32_t admmq_cholqr64(const double* Z, int64_t ldz, int64_t m, int64_t k, const double* G, double shift_scale, double* Q,
                       int64_t ldq, int32_t* info, void* stream) {
  if (!Z || !G || !Q) return set_error(ADMMQ_ERR_ARG, "cholqr64: null Z, G or Q");
  if (m <= 0 || k <= 0) return set_error(ADMMQ_ERR_ARG, "cholqr64: m and k must be positive");
  if (k > ADMMQ_CHOLQR_K_MAX) return set_error(ADMMQ_ERR_ARG, "cholqr64: k above ADMMQ_CHOLQR_K_MAX");
  if (ldz < k) return set_error(ADMMQ_ERR_ARG, "cholqr64: ldz < k");
  if (ldq < k) return set_error(ADMMQ_ERR_ARG, "cholqr64: ldq < k");
  if (m >= (1LL << 31) || ldz >= (1LL << 31) || ldq >= (1LL << 31))
    return set_error(ADMMQ_ERR_ARG, "cholqr64: sizes out of range");
  if (!(shift_scale >= 0.0)) return set_error(ADMMQ_ERR_ARG, "cholqr64: negative shift_scale");
  const dim3 grid((unsigned)((m + 63) / 64));
  hipStream_t s = static_cast<hipStream_t>(stream);
#define ADMMQ_CHOLQR(KB) \
  hipLaunchKernelGGL(k_cholqr64<KB>, grid, dim3(64), 0, s, Z, (int)ldz, (int)m, (int)k, G, shift_scale, Q, (int)ldq, info)
  if (k <= 16) ADMMQ_CHOLQR(16);
  else if (k <= 32) ADMMQ_CHOLQR(32);
  else if (k <= 48) ADMMQ_CHOLQR(48);
  else ADMMQ_CHOLQR(64);
#undef ADMMQ_CHOLQR
  return hipGetLastError() == hipSuccess ? ADMMQ_OK : set_error(ADMMQ_ERR_HIP, "cholqr64: launch failed");
}

int32_t admmq_panel_reorth64(const double* K, int64_t ldk, int64_t m, int64_t p, const double* C, int64_t ldc,
                             const double* Z, int64_t ldz, int64_t k, double* Zout, int64_t ldo, void* stream) {
  if (!K || !C || !Z || !Zout) return set_error(ADMMQ_ERR_ARG, "panel_reorth64: null K, C, Z or Zout");
  if (m <= 0 || p <= 0 || k <= 0) return set_error(ADMMQ_ERR_ARG, "panel_reorth64: m, p and k must be positive");
  if (k > ADMMQ_CHOLQR_K_MAX) return set_error(ADMMQ_ERR_ARG, "panel_reorth64: k above ADMMQ_CHOLQR_K_MAX");
  if (ldk < p) return set_error(ADMMQ_ERR_ARG, "panel_reorth64: ldk < p");
  if (ldc < k) return set_error(ADMMQ_ERR_ARG, "panel_reorth64: ldc < k");
  if (ldz < k) return set_error(ADMMQ_ERR_ARG, "panel_reorth64: ldz < k");
  if (ldo < k) return set_error(ADMMQ_ERR_ARG, "panel_reorth64: ldo < k");
  if (m >= (1LL << 31) || p > 8192 || ldk >= (1LL << 31) || ldc >= (1LL << 31) || ldz >= (1LL << 31) || ldo >= (1LL << 31))
    return set_error(ADMMQ_ERR_ARG, "panel_reorth64: sizes out of range");
  const dim3 grid((unsigned)((m + kReRows - 1) / kReRows));
  hipStream_t s = static_cast<hipStream_t>(stream);
#define ADMMQ_REORTH(NT)                                                                                              \
  hipLaunchKernelGGL(k_panel_reorth64<NT>, grid, dim3(256), 0, s, K, (int)ldk, (int)m, (int)p, C, (int)ldc, Z, (int)ldz, \
                     (int)k, Zout, (int)ldo)
  if (k <= 16) ADMMQ_REORTH(1);
  else if (k <= 32) ADMMQ_REORTH(2);
  else if (k <= 48) ADMMQ_REORTH(3);
  else ADMMQ_REORTH(4);
#undef ADMMQ_REORTH
  return hipGetLastError() == hipSuccess ? ADMMQ_OK : set_error(ADMMQ_ERR_HIP, "panel_reorth64: launch failed");
}

}  // extern "C"
