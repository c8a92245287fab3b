// Packed quant + low-rank linear layer (include/admmq.h "Packed quant + low-rank GEMM",
// DESIGN.md 2.28): y = W_q x + L (Rt x) (+ bias) with W_q the table de-quantization of packed
// codes [M, K], L [M, r] and Rt [r, K] float32, linear layout (x [C tokens, K], y [C, M]).
// Neither W_q nor L Rt exists in memory.
//
// Two kernels on k_packed_gemm's tile (256 threads, 4 waves of 32 x 32, a 64 x 64 tile, K steps
// of 32 on v_mfma_f32_32x32x2_f32, K pieces of kp = max(64, 32 ceil(K / 1024))):
//   k_lr_down            t[c, j] = sum_k Rt[j, k] x[c, k]: the float GEMM of the tile with M := r.
//                        Stored token-major ([C, r]: the layout of an x with K := r), serial
//                        form: t itself; parallel form: one image per piece.
//   k_packed_lrgemm<B>   k_packed_gemm<B, false, true> plus a tail piece: after the K pieces the
//                        W tile is staged from L and the X tile from t, in 32-wide steps over j
//                        (zero padded), summed from zero and folded last. Where k_lr_down ran in
//                        its parallel form the tail adds t's images in piece order as it stages
//                        them (there is no reduce launch for t).
// An output is ((((p0 + p1) + ...) + p_{np-1}) + q) + bias with p_i the pieces of k_packed_gemm
// and q the tail. Serial form: one workgroup runs the pieces and the tail of its tile. Parallel
// form: one workgroup per piece and one more for the tail, each writes its image to the
// workspace, k_lr_reduce adds the np + 1 images in order. Each kernel takes its regime from the
// planner on its own tile count (k_lr_down: ceil(r / 64) x ceil(C / 64) tiles). No workgroup
// waits for another, nothing is combined with atomics.
#include <algorithm>
#include <type_traits>

#include "../../include/admmq.h"
#include "packed_tile.h"

namespace admmq {

// k_packed_gemm's K step, LDS row stride and K limit (packed_gemm.hip keeps its own copies)
constexpr int kLrBK = 32;
constexpr int kLrLD = 65;
constexpr int64_t kLrKMax = int64_t(1) << 24;
constexpr int kLrRankMax = 256;

typedef float lr_f32x16 __attribute__((ext_vector_type(16)));

struct LrArgs {
  const unsigned char* codes;   // k_packed_lrgemm: the packed W_q [M, K]
  const float* wf;              // k_lr_down: the float W [M, K] (Rt, M = r)
  const float* x;               // [C, K]
  const float* bias;
  float* y;                     // serial form: [C, M]
  float* part;                  // parallel form: [np (+ 1 for the tail)][total] images in y's layout
  const float* L;               // [M, r]
  const float* t;               // [tnp][C r]: t (tnp = 1) or its images by piece (tnp = np)
  long long nbytes;             // bytes of the code stream
  long long total;              // C * M
  long long C;
  int M, K, r, tnp;
  int kp, np, parallel;
  int scheme, zp;
  float scale, mn, rng;
};

// BITS > 0: W is decoded from the code stream and the tail runs; BITS == 0: W is the float
// matrix wf, no tail (k_lr_down). The K loop is k_packed_gemm's with trans_w = 0, x_layout = 1:
// a thread takes 8 k-consecutive elements of a W row and 8 columns of one k of X; full steps
// load without k tests, columns past C read a clamped address and are zeroed by a select.
template <int BITS>
__device__ __forceinline__ void lr_tile(const LrArgs& a, float (&sW)[2][kLrBK * kLrLD], float (&sX)[2][kLrBK * kLrLD]) {
  constexpr bool CODES = BITS > 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, i = lane & 31, h = lane >> 5;
  const int M = a.M, K = a.K;
  const long long C = a.C;
  const int m0 = (int)blockIdx.y * kPackedBM;
  const long long c0 = (long long)blockIdx.x * kPackedBN;
  const int piece = (int)blockIdx.z;
  const bool tail_only = CODES && a.parallel && piece == a.np;   // the parallel form's extra workgroup
  const bool tail = CODES && (!a.parallel || piece == a.np);
  const int kb = a.parallel && !tail_only ? piece * a.kp : 0;
  const int ke = a.parallel ? (tail_only ? 0 : min(K, kb + a.kp)) : K;
  const unsigned char* __restrict__ codes = a.codes;
  const long long nbytes = a.nbytes;

  const int wrow = tid >> 2;         // m - m0 of the thread's W run
  const int wk = 8 * (tid & 3);      // k - k0 of its first element
  const bool wok = m0 + wrow < M;
  const int nvm = wok ? 8 : 0;
  const long long wrow_c = min(m0 + wrow, M - 1);   // (a row past M is never loaded: the clamp keeps the pointer inside)
  const long long bit0 = ((long long)(m0 + wrow) * K + (kb + wk)) * (CODES ? BITS : 1);
  const int wsh = (int)(bit0 & 31);
  long long wq = bit0 >> 5;
  const float* __restrict__ wp = CODES ? nullptr : a.wf + wrow_c * K + (kb + wk);
  const int xc = tid >> 5;
  const int xk = tid & 31;
  long long cc[8];      // the 8 columns, clamped
  long long xo[8];      // their element offsets in x
  unsigned xok = 0u;    // bit j: column j is inside C
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long long c = c0 + xc + 8 * j;
    if (c < C) xok |= 1u << j;
    cc[j] = min(c, C - 1);
    xo[j] = cc[j] * K;
  }
  const float* __restrict__ xp = a.x + (kb + xk);

  unsigned cw[3] = {0u, 0u, 0u};
  float rw[8];
  int nv = 0;
  float rx[8];
  auto load = [&](int k0, auto full) {
    constexpr bool FULL = decltype(full)::value;
    if (FULL) nv = nvm;
    else nv = nvm > 0 ? min(8, ke - (k0 + wk)) : 0;
    if constexpr (CODES) {
      cw[0] = 0u; cw[1] = 0u; cw[2] = 0u;
      if (nv > 0) {
        if (4 * wq + 12 <= nbytes) {   // all three inside the stream
          const gcu32* q = (const gcu32*)(codes + 4 * wq);
          cw[0] = q[0]; cw[1] = q[1]; cw[2] = q[2];
        } else {                       // the stream's end: nothing past its last byte is read
          cw[0] = code_dword(codes, wq, nbytes);
          cw[1] = code_dword(codes, wq + 1, nbytes);
          cw[2] = code_dword(codes, wq + 2, nbytes);
        }
      }
      wq += BITS;
    } else {
      const gcf32* wg = (const gcf32*)wp;
#pragma unroll
      for (int j = 0; j < 8; ++j) rw[j] = j < nv ? wg[j] : 0.f;
      wp += kLrBK;
    }
    const gcf32* xg = (const gcf32*)xp;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (FULL) {
        const float v = xg[xo[j]];
        rx[j] = ((xok >> j) & 1u) ? v : 0.f;
      } else {
        rx[j] = (((xok >> j) & 1u) && k0 + xk < ke) ? xg[xo[j]] : 0.f;
      }
    }
    xp += kLrBK;
  };
  auto store = [&](int buf) {
    float d[8];
    if constexpr (CODES) {
      constexpr unsigned mask = (1u << (CODES ? BITS : 1)) - 1u;
      const int p2 = wsh + 4 * BITS;
      const bool up = p2 >= 32;
      unsigned long long win[2];
      win[0] = (((unsigned long long)cw[1] << 32) | cw[0]) >> wsh;
      win[1] = (((unsigned long long)(up ? cw[2] : cw[1]) << 32) | (up ? cw[1] : cw[0])) >> (p2 & 31);
      if (a.scheme == kMinMax) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          d[j] = dequant_code((unsigned)(win[j >> 2] >> ((j & 3) * BITS)) & mask, kMinMax, BITS, a.scale, a.zp, a.mn, a.rng);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          d[j] = dequant_code((unsigned)(win[j >> 2] >> ((j & 3) * BITS)) & mask, kAffine, BITS, a.scale, a.zp, a.mn, a.rng);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = rw[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) sW[buf][(wk + j) * kLrLD + wrow] = j < nv ? d[j] : 0.f;   // past the piece / the matrix: exactly 0
#pragma unroll
    for (int j = 0; j < 8; ++j) sX[buf][xk * kLrLD + xc + 8 * j] = rx[j];
  };
  auto load_step = [&](int k0) {
    if (k0 + kLrBK <= ke) load(k0, std::true_type{});
    else load(k0, std::false_type{});
  };

  lr_f32x16 acc, tot;
#pragma unroll
  for (int q = 0; q < 16; ++q) { acc[q] = 0.f; tot[q] = 0.f; }
  bool first = true;
  auto fold = [&]() {   // a piece ends: tot = ((p0 + p1) + ...) + acc
    if (first) {
      tot = acc;
      first = false;
    } else {
#pragma unroll
      for (int q = 0; q < 16; ++q) tot[q] = tot[q] + acc[q];
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  };
  auto mfma_step = [&](int buf) {
    const float* w = sW[buf] + 32 * wm + i;
    const float* x = sX[buf] + 32 * wn + i;
#pragma unroll
    for (int q = 0; q < kLrBK / 2; ++q)   // operands swapped: the result's lanes run along m, y's contiguous axis
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[(2 * q + h) * kLrLD], w[(2 * q + h) * kLrLD], acc, 0, 0, 0);
  };

  if (!tail_only) {   // (uniform over the workgroup, as every branch around a barrier here)
    int pend = kb + a.kp;
    load_step(kb);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int k0 = kb; k0 < ke; k0 += kLrBK) {
      const bool more = k0 + kLrBK < ke;
      if (more) load_step(k0 + kLrBK);
      mfma_step(buf);
      if (!more || k0 + kLrBK == pend) {
        pend += a.kp;
        fold();
      }
      if (more) store(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }

  if constexpr (CODES) {
    if (tail) {
      // The tail piece q[m, c] = sum_j L[m, j] t[c, j]: W from L (a thread's 8 j of one row), X
      // from t (one j, 8 columns), t's images added in piece order. Rows past M, j past r and
      // columns past C are exact zeros. Single buffered: at most 8 steps.
      const int r = a.r;
      const long long timg = C * r;
      const float* __restrict__ lp = a.L + wrow_c * r + wk;
      for (int j0 = 0; j0 < r; j0 += kLrBK) {
        const gcf32* lg = (const gcf32*)(lp + j0);
        const int nl = wok ? min(8, r - (j0 + wk)) : 0;
        float lv[8], s[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) lv[j] = j < nl ? lg[j] : 0.f;
        const bool jok = j0 + xk < r;
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = 0.f;
        if (jok) {
          // one image at a time: issuing several images' loads together costs the kernel its occupancy
          // (four at a time: 222 VGPRs against 112), and the K loop above lives on it
          const gcf32* tg = (const gcf32*)(a.t + (j0 + xk));
          for (int p = 0; p < a.tnp; ++p) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = tg[cc[j] * r];
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = p == 0 ? v[j] : s[j] + v[j];
            tg += timg;
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) sW[0][(wk + j) * kLrLD + wrow] = lv[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) sX[0][xk * kLrLD + xc + 8 * j] = ((xok >> j) & 1u) ? s[j] : 0.f;
        __syncthreads();
        mfma_step(0);
        __syncthreads();
      }
      fold();
    }
  }

  float* const dst = a.parallel ? a.part + (long long)piece * a.total : a.y;
  const float* __restrict__ bias = a.parallel ? nullptr : a.bias;
  const int m = m0 + 32 * wm + i;
  if (m >= M) return;
  const float bv = bias ? bias[m] : 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const long long c = c0 + 32 * wn + PACKED_ROW(q);
    if (c < C) dst[c * M + m] = bias ? tot[q] + bv : tot[q];
  }
}

__global__ __launch_bounds__(256) void k_lr_down(const LrArgs a) {
  __shared__ float sW[2][kLrBK * kLrLD];
  __shared__ float sX[2][kLrBK * kLrLD];
  lr_tile<0>(a, sW, sX);
}

template <int BITS>
__global__ __launch_bounds__(256) void k_packed_lrgemm(const LrArgs a) {
  __shared__ float sW[2][kLrBK * kLrLD];
  __shared__ float sX[2][kLrBK * kLrLD];
  lr_tile<BITS>(a, sW, sX);
}

// y[e] = (((part_0[e] + part_1[e]) + ...) + part_{nimg-1}[e]) + bias[e % M]: the serial form's order
__global__ __launch_bounds__(256) void k_lr_reduce(const float* __restrict__ part, int nimg, long long total,
                                                   const float* __restrict__ bias, float* __restrict__ y, int M) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  float s = part[e];
  for (int p = 1; p < nimg; ++p) s = s + part[(long long)p * total + e];
  if (bias) s = s + bias[e % M];
  y[e] = s;
}

// The two plans of a call (functions of the sizes alone) and the workspace's layout:
// [np + 1 images of y, parallel form only][t: one image, or np where k_lr_down runs in parallel]
struct LrPlan {
  PackedPlan g, d;     // the GEMM on (M, K, N), the down-projection on (r, K, N)
  size_t part_bytes;   // the y images
  size_t ws;           // in all
};

static bool plan_lr(int64_t M, int64_t K, int64_t N, int64_t r, LrPlan& pl) {
  if (r < 1 || r > kLrRankMax) return false;
  if (!plan_packed(M, K, N, 1, kLrBK, kLrKMax, sizeof(float), pl.g) || M * K >= (int64_t(1) << 40)) return false;
  if (!plan_packed(r, K, N, 1, kLrBK, kLrKMax, sizeof(float), pl.d)) return false;
  pl.part_bytes = pl.g.parallel ? (size_t)(pl.g.np + 1) * (size_t)pl.g.total * sizeof(float) : 0;
  pl.ws = pl.part_bytes + (size_t)(pl.d.parallel ? pl.d.np : 1) * (size_t)pl.d.total * sizeof(float);
  return true;
}

}  // namespace admmq

using namespace admmq;

extern "C" {

size_t admmq_packed_lrgemm_workspace_size(int64_t M, int64_t K, int64_t N, int32_t r) {
  LrPlan pl;
  return plan_lr(M, K, N, r, pl) ? pl.ws : 0;
}

int32_t admmq_packed_lrgemm(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const float* L,
                            const float* Rt, int32_t r, const float* x, int64_t N, const float* bias, float* y,
                            void* workspace, size_t workspace_bytes, void* stream) {
  const char* const who = "packed_lrgemm";
  if (!codes || !x || !y || !meta || !L || !Rt)
    return packed_fail(who, ADMMQ_ERR_ARG, "codes, meta, L, Rt, x and y must not be NULL");
  if (M <= 0 || K <= 0 || N <= 0) return packed_fail(who, ADMMQ_ERR_ARG, "M, K and N must be positive");
  if (r < 1 || r > kLrRankMax) return packed_fail(who, ADMMQ_ERR_ARG, "rank r must be 1..256");
  int32_t rc = packed_meta_check(meta, who, false, nullptr);
  if (rc != ADMMQ_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(codes) & 15) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "codes must be 16-byte aligned");
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(bias) |
        reinterpret_cast<uintptr_t>(L) | reinterpret_cast<uintptr_t>(Rt)) & 3) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "L, Rt, x, y and bias must be float aligned");
  LrPlan pl;
  if (!plan_lr(M, K, N, r, pl)) return packed_fail(who, ADMMQ_ERR_ARG, "sizes out of range");
  PackedPlan whole = pl.g;   // (the size that packed_ws_check tests: the images and t)
  whole.ws = pl.ws;
  rc = packed_ws_check(who, whole, workspace, workspace_bytes, "float");
  if (rc != ADMMQ_OK) return rc;

  float* const part = static_cast<float*>(workspace);
  float* const t = reinterpret_cast<float*>(static_cast<char*>(workspace) + pl.part_bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);

  LrArgs d = {};   // t = Rt x: M := r
  d.wf = Rt; d.x = x; d.y = t; d.part = t;
  d.total = pl.d.total; d.C = pl.d.C;
  d.M = r; d.K = (int)K;
  d.kp = pl.d.kp; d.np = pl.d.np; d.parallel = pl.d.parallel;
  hipLaunchKernelGGL(k_lr_down, dim3((unsigned)pl.d.tiles_c, (unsigned)pl.d.tiles_m, pl.d.parallel ? (unsigned)pl.d.np : 1u),
                     dim3(256), 0, s, d);

  LrArgs a = {};
  a.codes = codes; a.x = x; a.bias = bias; a.y = y;
  a.part = pl.g.parallel ? part : nullptr;
  a.L = L; a.t = t;
  a.nbytes = (long long)admmq_packed_bytes(M * K, meta->bits);
  a.total = pl.g.total; a.C = pl.g.C;
  a.M = (int)M; a.K = (int)K; a.r = r; a.tnp = pl.d.parallel ? pl.d.np : 1;
  a.kp = pl.g.kp; a.np = pl.g.np; a.parallel = pl.g.parallel;
  a.scheme = meta->scheme;
  a.zp = meta->scheme == kAffine ? meta->zero_point : 0;
  a.scale = meta->scale; a.mn = meta->mn; a.rng = meta->rng;
  const dim3 grid((unsigned)pl.g.tiles_c, (unsigned)pl.g.tiles_m, pl.g.parallel ? (unsigned)pl.g.np + 1u : 1u);
#define ADMMQ_LR_BITS(B) hipLaunchKernelGGL((k_packed_lrgemm<B>), grid, dim3(256), 0, s, a)
  PACKED_BITS_SWITCH(meta->bits, ADMMQ_LR_BITS)
#undef ADMMQ_LR_BITS
  if (pl.g.parallel)
    hipLaunchKernelGGL(k_lr_reduce, dim3((unsigned)((pl.g.total + 255) / 256)), dim3(256), 0, s, part, pl.g.np + 1,
                       pl.g.total, bias, y, (int)M);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

}  // extern "C"
