// Skinny quant + low-rank GEMV for decode shapes (include/admmq.h "Skinny quant + low-rank GEMV",
// DESIGN.md 2.33): y[c, m] = (v[c, m] + q[c, m]) (+ bias[m]) for 1 <= N <= 8 rows of x, with v the value of
// admmq_packed_gemv on the codes (W = D, before the bias) and q = L (Rt x) the low-rank tail, L [M, r] and
// Rt [r, K] in float32 or x's 16-bit type, x in float32, bfloat16 or float16.
//
// Two kernels, and the reduce where the code sum is split over K.
//   k_lr_down_gemv   t = x Rt^T. Rt is read once, so the kernel is a stream: a workgroup of four waves owns
//     four rows j of Rt, a wave one of them, over the workgroup's K range; the range is walked in chunks of
//     1024 k whose x image (gv_stage's dense layout, zeros past the range, past K and past N) the four waves
//     share. In every step of 256 k a lane owns the four k = k0 + 256 s + 4 lane .. + 3: one 16-byte load of a
//     float32 row (8 bytes of a 16-bit row, widened in registers; element loads where Rt's rows do not sit
//     on such boundaries), one 16-byte LDS read a column, four FMAs a column in increasing k. The four
//     steps' loads are issued before the image is staged. The 64 lanes meet in the fixed tree of
//     packed_gemv.h inside each 16-lane DPP row, the four row sums as ((s0 + s1) + s2) + s3.
//     r / 4 workgroups do not fill the chip, so plan_lrgv (a function of K and r alone) cuts K into nsd
//     ranges over gridDim.z; range z writes its image tpart[z][c][j]. There is no reduce launch for t: the
//     consumer adds the images in range order while it stages them.
//   k_packed_lrgemv  k_packed_gemv<BITS, NB, true> (packed_gemv.h): k_packed_gemv's body with the tail behind the
//     code chunks. In the K-split plan of the code sum (plan_gv's, on the same M and K) the tail is one more
//     slice of gridDim.z that writes q as image ns, and k_packed_lrgemv_reduce adds the ns code images in
//     range order, runs the epilogue and adds q and then the bias.
// No atomics, no workgroup waits for another, and no sum depends on N: an output has the same bits at
// every N, column position and call.
#include "packed_gemv.h"

namespace admmq {

constexpr int kLdRows = 4;                    // rows of Rt per workgroup, one a wave
constexpr int kLdStep = 64 * 4;               // k per step: four a lane
constexpr int kLdSteps = 4;                   // steps per chunk
constexpr int kLdCh = kLdSteps * kLdStep;     // k per chunk: 1024
constexpr int kLdMinK = kLdStep;              // k per range at least, and what a range is a multiple of

struct GvDown {
  const void* Rt;     // [r, K] row-major, float32 or a 16-bit type
  float* tpart;       // [nsd][N][r]
  int r, ksd;         // the rank, k per range
  int fdt;            // ADMMQ_DT_* of Rt
  int ral;            // every row of Rt starts on a boundary of four elements and holds whole groups of four
};

typedef unsigned gv_u32x2 __attribute__((ext_vector_type(2)));

// Rt[row + k .. + 3] widened to float32; elements past K are 0 (they meet zeros of the image)
__device__ __forceinline__ void ld_row4(const GvDown& d, long long row, int k, int K, float (&v)[4]) {
  if (d.ral) {
    if (d.fdt == ADMMQ_DT_F32) {
      const gv_u32x4 q = *reinterpret_cast<const gv_u32x4*>(static_cast<const float*>(d.Rt) + row + k);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = __uint_as_float(q[i]);
    } else {
      const gv_u32x2 q = *reinterpret_cast<const gv_u32x2*>(static_cast<const unsigned short*>(d.Rt) + row + k);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        v[2 * i] = gv_half_bits(q[i] & 0xFFFFu, d.fdt);
        v[2 * i + 1] = gv_half_bits(q[i] >> 16, d.fdt);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = k + i < K ? gv_widen(d.Rt, row + k + i, d.fdt) : 0.f;
  }
}

template <int NB>
__global__ __launch_bounds__(256) void k_lr_down_gemv(const GvArgs a, const GvDown d) {
  __shared__ __attribute__((aligned(16))) float xs[NB * kLdCh];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = a.K;
  const int kb = (int)blockIdx.z * d.ksd, ke = min(K, kb + d.ksd);
  const int j = (int)blockIdx.x * kLdRows + wave;                 // the wave's row (past r: the last row, never stored)
  const long long row = (long long)min(j, d.r - 1) * K;
  float acc[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) acc[c] = 0.f;

  for (int k0 = kb; k0 < ke; k0 += kLdCh) {
    float rv[kLdSteps][4];
#pragma unroll
    for (int s = 0; s < kLdSteps; ++s) {
      const int k = k0 + kLdStep * s + 4 * lane;
      if (k < ke) ld_row4(d, row, k, K, rv[s]);   // (ke is K or a multiple of 256: a group never straddles it)
    }
    __syncthreads();   // the last chunk's image has been read
    gv_stage<NB, kLdCh, kLdCh, kLdCh>(a, xs, k0, ke);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kLdSteps; ++s) {
      const int kk = kLdStep * s + 4 * lane;
      if (k0 + kk < ke) {
#pragma unroll
        for (int c = 0; c < NB; ++c) {
          const float4 xv = *reinterpret_cast<const float4*>(xs + c * kLdCh + kk);
          acc[c] = __builtin_fmaf(rv[s][0], xv.x, acc[c]);
          acc[c] = __builtin_fmaf(rv[s][1], xv.y, acc[c]);
          acc[c] = __builtin_fmaf(rv[s][2], xv.z, acc[c]);
          acc[c] = __builtin_fmaf(rv[s][3], xv.w, acc[c]);
        }
      }
    }
  }
  // the 64 lanes: the tree inside each 16-lane DPP row, then the four row sums in lane order
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    const unsigned v = __float_as_uint(gv_row_sum(acc[c]));
    const float s = ((__uint_as_float(readlane_u32(v, 15)) + __uint_as_float(readlane_u32(v, 31))) +
                     __uint_as_float(readlane_u32(v, 47))) + __uint_as_float(readlane_u32(v, 63));
    if (lane == 0 && j < d.r && c < a.N) d.tpart[((long long)blockIdx.z * a.N + c) * d.r + j] = s;
  }
}

template <int BITS, int NB>
constexpr auto k_packed_lrgemv = k_packed_gemv<BITS, NB, true>;

// y[e] = (epilogue(((part_0[e] + part_1[e]) + ...), the sums of x alike) + part_ns[e]) + bias[m]: part_ns is q
__global__ __launch_bounds__(256) void k_packed_lrgemv_reduce(const GvArgs a) {
  const long long total = (long long)a.N * a.M;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  float s = a.part[e];
  for (int p = 1; p < a.ns; ++p) s = s + a.part[(long long)p * total + e];
  const int c = (int)(e / a.M), m = (int)(e - (long long)c * a.M);
  float sx = 0.f;
  if (a.scheme == kMinMax) {
    sx = a.xpart[c];
    for (int p = 1; p < a.ns; ++p) sx = sx + a.xpart[p * a.N + c];
  }
  float v = gv_value(s, sx, a, false, 0.f) + a.part[(long long)a.ns * total + e];
  if (a.bias) v = v + a.bias[m];
  gv_store(a.y, e, v, a.ydt);
}

// --- host side ------------------------------------------------------------------------------------

// The plan of one call: plan_gv's split of the code sum (ns ranges of ks), and the split of the
// down-projection, a function of K and r alone: ceil(r / 4) workgroups a range, enough ranges for one
// workgroup a CU, kGvSplitMax at most, each a multiple of 256 k. The workspace holds, in this order,
// tpart [nsd][N][r], and where ns > 1 part [ns + 1][N][M] (image ns: q) and, for tensor_minmax, xpart [ns][N].
struct LrgvPlan {
  GvPlan gv;
  int ksd, nsd, launches;
  size_t ws;
};

static bool plan_lrgv(const ::admmq_qmeta* meta, int64_t M, int64_t K, int64_t N, int64_t r, LrgvPlan& pl) {
  if (r < 1 || r > kGvRankMax || !plan_gv(meta, 0, M, K, N, pl.gv)) return false;
  const int64_t groups = (r + kLdRows - 1) / kLdRows;
  const int64_t want = std::min<int64_t>({(kGvOneLaunch + groups - 1) / groups, (int64_t)kGvSplitMax, (K + kLdMinK - 1) / kLdMinK});
  const int64_t ksd = kLdMinK * ((((K + want - 1) / want) + kLdMinK - 1) / kLdMinK);
  pl.ksd = (int)ksd;
  pl.nsd = (int)((K + ksd - 1) / ksd);
  pl.launches = pl.gv.ns > 1 ? 3 : 2;
  pl.ws = (size_t)pl.nsd * (size_t)N * (size_t)r * sizeof(float);
  if (pl.gv.ns > 1) pl.ws += pl.gv.ws + (size_t)N * (size_t)M * sizeof(float);
  return true;
}

static bool lrgv_dt_ok(int32_t dt) { return dt == ADMMQ_DT_F32 || dt == ADMMQ_DT_F16 || dt == ADMMQ_DT_BF16; }

static int32_t packed_lrgemv_run(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const void* L,
                                 const void* Rt, int32_t f_dtype, int32_t r, const void* x, int32_t x_dtype, int64_t N,
                                 const float* bias, void* y, int32_t y_dtype, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  const char* const who = "packed_lrgemv";
  if (!codes || !x || !y || !meta || !L || !Rt)
    return packed_fail(who, ADMMQ_ERR_ARG, "codes, meta, L, Rt, x and y must not be NULL");
  if (M <= 0 || K <= 0) return packed_fail(who, ADMMQ_ERR_ARG, "M and K must be positive");
  if (N < 1 || N > ADMMQ_GEMV_N_MAX) return packed_fail(who, ADMMQ_ERR_ARG, "N must be 1..8 (ADMMQ_GEMV_N_MAX)");
  if (r < 1 || r > kGvRankMax) return packed_fail(who, ADMMQ_ERR_ARG, "rank r must be 1..256");
  int32_t rc = packed_meta_check(meta, who, false, nullptr);
  if (rc != ADMMQ_OK) return rc;
  if (!lrgv_dt_ok(x_dtype)) return packed_fail(who, ADMMQ_ERR_ARG, "x_dtype must be ADMMQ_DT_F32, ADMMQ_DT_F16 or ADMMQ_DT_BF16");
  if (y_dtype != ADMMQ_DT_F32 && y_dtype != x_dtype)
    return packed_fail(who, ADMMQ_ERR_ARG, "y_dtype must be ADMMQ_DT_F32 or x_dtype");
  if (f_dtype != ADMMQ_DT_F32 && (f_dtype != x_dtype || !lrgv_dt_ok(f_dtype)))
    return packed_fail(who, ADMMQ_ERR_ARG, "f_dtype must be ADMMQ_DT_F32 or a 16-bit x_dtype");
  // admmq_packed_gemv's limit on a half x: the integer operand is one exact in x's type
  const int64_t q = int64_t(1) << (meta->bits - 1);
  const int64_t zp = meta->scheme == kAffine ? (int64_t)meta->zero_point : 0;
  const int64_t lim = x_dtype == ADMMQ_DT_BF16 ? 256 : 2048;
  if (x_dtype != ADMMQ_DT_F32 && meta->scheme != kMinMax && (-q - zp < -lim || q - 1 - zp > lim))
    return packed_fail(who, ADMMQ_ERR_ARG, "affine zero_point puts (u - q) - zero_point outside the integers exact in x_dtype");
  if ((reinterpret_cast<uintptr_t>(codes) & 15) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "codes must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(x) & (gv_dt_bytes(x_dtype) - 1)) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "x must be aligned to its element");
  if ((reinterpret_cast<uintptr_t>(y) & (gv_dt_bytes(y_dtype) - 1)) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "y must be aligned to its element");
  if (((reinterpret_cast<uintptr_t>(L) | reinterpret_cast<uintptr_t>(Rt)) & (gv_dt_bytes(f_dtype) - 1)) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "L and Rt must be aligned to their element");
  if ((reinterpret_cast<uintptr_t>(bias) & 3) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "bias must be float aligned");
  LrgvPlan pl;
  if (!plan_lrgv(meta, M, K, N, r, pl)) return packed_fail(who, ADMMQ_ERR_ARG, "sizes out of range");
  if (!workspace || workspace_bytes < pl.ws) return set_error(ADMMQ_ERR_WORKSPACE, "workspace too small");
  if ((reinterpret_cast<uintptr_t>(workspace) & 3) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "workspace must be float aligned");
  const int ns = pl.gv.ns;
  float* const tpart = static_cast<float*>(workspace);
  GvArgs a;
  a.codes = codes; a.x = x; a.bias = bias; a.y = y;
  a.part = ns > 1 ? tpart + (size_t)pl.nsd * (size_t)N * (size_t)r : nullptr;
  a.xpart = ns > 1 ? a.part + (size_t)(ns + 1) * (size_t)N * (size_t)M : nullptr;
  a.nbytes = (long long)admmq_packed_bytes(M * K, meta->bits);
  a.M = (int)M; a.K = (int)K; a.N = (int)N;
  a.ks = pl.gv.ks; a.ns = ns;
  a.scheme = meta->scheme;
  a.off = meta->scheme == kMinMax ? 0 : (int)(q + zp);
  a.xdt = x_dtype; a.ydt = y_dtype;
  a.xal = ((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (K * (int64_t)gv_dt_bytes(x_dtype)) % 16 == 0) ? 1 : 0;
  a.scale = meta->scale; a.mn = meta->mn; a.rng = meta->rng;
  a.nlev = (float)((1 << meta->bits) - 1);
  GvDown d;
  d.Rt = Rt; d.tpart = tpart; d.r = r; d.ksd = pl.ksd; d.fdt = f_dtype;
  d.ral = ((reinterpret_cast<uintptr_t>(Rt) & (4 * gv_dt_bytes(f_dtype) - 1)) == 0 && K % 4 == 0) ? 1 : 0;
  GvLr lr;
  lr.L = L; lr.tpart = tpart; lr.r = r; lr.rp = 32 * ((r + 31) / 32); lr.nsd = pl.nsd; lr.fdt = f_dtype;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 dgrid((unsigned)((r + kLdRows - 1) / kLdRows), 1u, (unsigned)pl.nsd);
  const dim3 grid((unsigned)pl.gv.tiles, 1u, (unsigned)(ns > 1 ? ns + 1 : 1));
#define ADMMQ_LRGV_DOWN(NB) hipLaunchKernelGGL((k_lr_down_gemv<NB>), dgrid, dim3(256), 0, s, a, d)
#define ADMMQ_LRGV_MAIN(B, NB) hipLaunchKernelGGL((k_packed_lrgemv<B, NB>), grid, dim3(256), 0, s, a, lr)
#define ADMMQ_LRGV_BITS(B)                   \
  if (N == 1) ADMMQ_LRGV_MAIN(B, 1);         \
  else if (N == 2) ADMMQ_LRGV_MAIN(B, 2);    \
  else if (N <= 4) ADMMQ_LRGV_MAIN(B, 4);    \
  else ADMMQ_LRGV_MAIN(B, 8)
  if (N == 1) ADMMQ_LRGV_DOWN(1);
  else if (N == 2) ADMMQ_LRGV_DOWN(2);
  else if (N <= 4) ADMMQ_LRGV_DOWN(4);
  else ADMMQ_LRGV_DOWN(8);
  PACKED_BITS_SWITCH(meta->bits, ADMMQ_LRGV_BITS)
#undef ADMMQ_LRGV_BITS
#undef ADMMQ_LRGV_MAIN
#undef ADMMQ_LRGV_DOWN
  if (ns > 1)
    hipLaunchKernelGGL(k_packed_lrgemv_reduce, dim3((unsigned)((N * M + 255) / 256)), dim3(256), 0, s, a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

}  // namespace admmq

using namespace admmq;

extern "C" {

size_t admmq_packed_lrgemv_workspace_size(const admmq_qmeta* meta, int64_t M, int64_t K, int64_t N, int32_t r) {
  LrgvPlan pl;
  return plan_lrgv(meta, M, K, N, r, pl) ? pl.ws : 0;
}

int32_t admmq_packed_lrgemv_plan(const admmq_qmeta* meta, int64_t M, int64_t K, int32_t r, int32_t out[3]) {
  LrgvPlan pl;
  if (!out || !plan_lrgv(meta, M, K, 1, r, pl)) return ADMMQ_ERR_ARG;
  out[0] = pl.gv.ns; out[1] = pl.nsd; out[2] = pl.launches;
  return ADMMQ_OK;
}

int32_t admmq_packed_lrgemv(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const void* L,
                            const void* Rt, int32_t f_dtype, int32_t r, const void* x, int32_t x_dtype, int64_t N,
                            const float* bias, void* y, int32_t y_dtype, void* workspace, size_t workspace_bytes,
                            void* stream) {
  return packed_lrgemv_run(codes, meta, M, K, L, Rt, f_dtype, r, x, x_dtype, N, bias, y, y_dtype, workspace,
                           workspace_bytes, stream);
}

}  // extern "C"
