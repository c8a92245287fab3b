// Skinny GEMV of a packed weight for decode shapes (include/admmq.h "Skinny packed GEMV",
// DESIGN.md 2.32): y[c, m] = sum_k W[m, k] x[c, k] (+ bias[m]) for 1 <= N <= 8 rows of x, W = D or
// D^T, D the table de-quantization of a packed tensor's codes, x in float32, bfloat16 or float16.
// No MFMA and no LDS image of the weight: every code is cut out of registers and multiplied
// into float32 accumulators with one FMA per column.
//
// The weight enters as the exact integer a = (u - q) - zp (tensor_minmax: u) converted to
// float32 and its scale is applied behind the sum, as in packed_hgemm.hip. The activations are
// widened to float32 exactly, once per workgroup and K chunk, into an LDS image that the FMAs
// read; so x's type is a run-time property of the staging and of the store, and the kernels are
// instantiated on (BITS, NB) only, NB = 1 / 2 / 4 / 8 the columns held in registers.
//
// The two orientations are two kernels.
//   k_packed_gemv   (W = D, a row's codes run along k; in packed_gemv.h, which packed_lrgemv.hip
//     shares). A workgroup of four waves owns 32 rows:
//     a wave's two halves of 32 lanes own four rows each, and a lane owns the run of 32 codes
//     k = k0 + 32 (lane & 31) .. + 31 of each of them in every chunk of 1024 k. 32 codes are
//     BITS whole dwords, so a row's runs all start at the row's bit offset in a dword: a lane
//     loads BITS + 1 dwords a row and funnel-shifts them into BITS aligned ones (v_alignbit),
//     from which every code is cut with compile-time shifts. The four rows share the lane's x
//     values. A lane adds its terms in increasing k; the 32 lanes of a row meet in a fixed tree
//     (row_shr 1, 2, 4, 8 inside each 16-lane DPP row, then the two row sums through LDS, lower
//     k first).
//   k_packed_gemv_t (W = D^T, a row of the stream runs along m). Lanes run along m, four
//     consecutive m a lane (4 BITS <= 32 bits out of two dwords, one v_alignbit), 256 m a
//     workgroup. Each of the four waves walks its quarter of every chunk of 512 k with the x
//     values broadcast from LDS, no cross-lane reduction at all, and the waves' sums meet through
//     LDS in wave order.
// Few rows of tiles do not fill the chip, so the host planner (plan_gv, a function of M, K, bits
// and trans_w - not of N, so that an output's sum order does not depend on N) may cut K into ns
// ranges over gridDim.z. The split workgroups write float32 partial sums to the workspace and
// k_packed_gemv_reduce adds them in range order and runs the epilogue. No workgroup waits for
// another and nothing is combined with atomics. Codes past a range's end, rows past M and
// columns past N meet an x image of exact zeros (fma(a, 0, s) = s) or are never stored; the
// stream's last dwords are read with code_dword, so nothing past the stream is read.
#include "packed_gemv.h"

namespace admmq {

template <int BITS, int NB>
__global__ __launch_bounds__(256) void k_packed_gemv_t(const GvArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[NB * kGtCh];   // the x image; then the waves' sums [c][256]
  __shared__ float sxr[NB];
  constexpr unsigned mask = (1u << BITS) - 1u;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.M, K = a.K;
  const int kb = (int)blockIdx.z * a.ks, ke = min(K, kb + a.ks);
  const unsigned char* __restrict__ codes = a.codes;
  const long long nbytes = a.nbytes;
  const bool mm = a.scheme == kMinMax;   // (uniform)
  const int off = a.off;
  const int ml = (int)blockIdx.x * kGtTile + kGtJ * lane;   // the lane's first m
  const bool on = ml < M;

  float acc[kGtJ][NB], sx[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    sx[c] = 0.f;
#pragma unroll
    for (int j = 0; j < kGtJ; ++j) acc[j][c] = 0.f;
  }
  for (int k0 = kb; k0 < ke; k0 += kGtCh) {
    __syncthreads();   // the last chunk's image has been read
    gv_stage<NB, kGtCh, kGtCh, kGtCh>(a, xs, k0, ke);
    __syncthreads();
    const int kw0 = k0 + wave * (kGtCh / 4), kw1 = min(ke, kw0 + kGtCh / 4);
    if (mm) {   // the sums of x over the wave's quarter, in the order of the FMAs below
      for (int k = kw0; k < kw1; k += 4)
#pragma unroll
        for (int c = 0; c < NB; ++c) {
          const float4 t = *reinterpret_cast<const float4*>(xs + c * kGtCh + (k - k0));
          sx[c] = (((sx[c] + t.x) + t.y) + t.z) + t.w;
        }
    }
    // four rows of the stream a step; a row past the range meets zeros of the image (and, past the
    // stream, code_dword's zeros)
    for (int k = kw0; k < kw1; k += 4) {
      unsigned v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long bit0 = ((long long)(k + i) * M + ml) * BITS;
        const long long q = bit0 >> 5;
        unsigned lo = 0u, hi = 0u;
        if (on) {
          if (4 * (q + 2) <= nbytes) {
            const gcu32* p = (const gcu32*)(codes + 4 * q);
            lo = p[0]; hi = p[1];
          } else {
            lo = code_dword(codes, q, nbytes);
            hi = code_dword(codes, q + 1, nbytes);
          }
        }
        v[i] = __builtin_amdgcn_alignbit(hi, lo, (unsigned)(bit0 & 31));   // 4 BITS <= 32 bits from bit 0
      }
      float xv[NB][4];
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        const float4 t = *reinterpret_cast<const float4*>(xs + c * kGtCh + (k - k0));   // (a broadcast read)
        xv[c][0] = t.x; xv[c][1] = t.y; xv[c][2] = t.z; xv[c][3] = t.w;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < kGtJ; ++j) {
          const float af = (float)((int)((v[i] >> (j * BITS)) & mask) - off);
#pragma unroll
          for (int c = 0; c < NB; ++c) acc[j][c] = __builtin_fmaf(af, xv[c][i], acc[j][c]);
        }
      }
    }
  }
  // the waves' sums meet in wave order: ((s0 + s1) + s2) + s3
  for (int w = 1; w < 4; ++w) {
    __syncthreads();   // (w = 1: every wave has left the image)
    if (wave == w) {
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        *reinterpret_cast<float4*>(xs + c * kGtTile + kGtJ * lane) = make_float4(acc[0][c], acc[1][c], acc[2][c], acc[3][c]);
        if (lane == 0) sxr[c] = sx[c];
      }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        const float4 t = *reinterpret_cast<const float4*>(xs + c * kGtTile + kGtJ * lane);
        acc[0][c] = acc[0][c] + t.x; acc[1][c] = acc[1][c] + t.y;
        acc[2][c] = acc[2][c] + t.z; acc[3][c] = acc[3][c] + t.w;
        sx[c] = sx[c] + sxr[c];
      }
    }
  }
  if (wave != 0 || !on) return;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    if (c >= a.N) break;
#pragma unroll
    for (int j = 0; j < kGtJ; ++j)
      if (ml + j < M) gv_emit(a, c, ml + j, acc[j][c], sx[c], ml + j == 0);
  }
}

// y[e] = epilogue(((part_0[e] + part_1[e]) + ...), ((xpart_0[c] + xpart_1[c]) + ...)): range order
__global__ __launch_bounds__(256) void k_packed_gemv_reduce(const GvArgs a) {
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
  gv_store(a.y, e, gv_value(s, sx, a, a.bias != nullptr, a.bias ? a.bias[m] : 0.f), a.ydt);
}

// --- host side ------------------------------------------------------------------------------------

template <int BITS, int NB>
static void gv_launch(const GvArgs& a, int32_t trans_w, dim3 grid, hipStream_t s) {
  if (trans_w) hipLaunchKernelGGL((k_packed_gemv_t<BITS, NB>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_packed_gemv<BITS, NB>), grid, dim3(256), 0, s, a, GvNoLr{});
}

static int32_t packed_gemv_run(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                               const void* x, int32_t x_dtype, int64_t N, const float* bias, void* y, int32_t y_dtype,
                               void* workspace, size_t workspace_bytes, void* stream) {
  const char* const who = "packed_gemv";
  if (!codes || !x || !y || !meta) return packed_fail(who, ADMMQ_ERR_ARG, "codes, meta, x and y must not be NULL");
  if (M <= 0 || K <= 0) return packed_fail(who, ADMMQ_ERR_ARG, "M and K must be positive");
  if (N < 1 || N > ADMMQ_GEMV_N_MAX) return packed_fail(who, ADMMQ_ERR_ARG, "N must be 1..8 (ADMMQ_GEMV_N_MAX)");
  int32_t rc = packed_meta_check(meta, who, false, nullptr);
  if (rc != ADMMQ_OK) return rc;
  if (trans_w != 0 && trans_w != 1) return packed_fail(who, ADMMQ_ERR_ARG, "trans_w must be 0 or 1");
  if (x_dtype != ADMMQ_DT_F32 && x_dtype != ADMMQ_DT_F16 && x_dtype != ADMMQ_DT_BF16)
    return packed_fail(who, ADMMQ_ERR_ARG, "x_dtype must be ADMMQ_DT_F32, ADMMQ_DT_F16 or ADMMQ_DT_BF16");
  if (y_dtype != ADMMQ_DT_F32 && y_dtype != x_dtype)
    return packed_fail(who, ADMMQ_ERR_ARG, "y_dtype must be ADMMQ_DT_F32 or x_dtype");
  // admmq_packed_hgemm's limit on a half x: the integer operand is one exact in x's type
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
  if ((reinterpret_cast<uintptr_t>(bias) & 3) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "bias must be float aligned");
  GvPlan pl;
  if (!plan_gv(meta, trans_w, M, K, N, pl)) return packed_fail(who, ADMMQ_ERR_ARG, "sizes out of range");
  if (pl.ws > 0 && (!workspace || workspace_bytes < pl.ws)) return set_error(ADMMQ_ERR_WORKSPACE, "workspace too small");
  if (pl.ws > 0 && (reinterpret_cast<uintptr_t>(workspace) & 3) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "workspace must be float aligned");
  GvArgs a;
  a.codes = codes; a.x = x; a.bias = bias; a.y = y;
  a.part = pl.ns > 1 ? static_cast<float*>(workspace) : nullptr;
  a.xpart = pl.ns > 1 ? a.part + (size_t)pl.ns * (size_t)N * (size_t)M : nullptr;
  a.nbytes = (long long)admmq_packed_bytes(M * K, meta->bits);
  a.M = (int)M; a.K = (int)K; a.N = (int)N;
  a.ks = pl.ks; a.ns = pl.ns;
  a.scheme = meta->scheme;
  a.off = meta->scheme == kMinMax ? 0 : (int)(q + zp);
  a.xdt = x_dtype; a.ydt = y_dtype;
  a.xal = ((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (K * (int64_t)gv_dt_bytes(x_dtype)) % 16 == 0) ? 1 : 0;
  a.scale = meta->scale; a.mn = meta->mn; a.rng = meta->rng;
  a.nlev = (float)((1 << meta->bits) - 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)pl.tiles, 1u, (unsigned)pl.ns);
#define ADMMQ_GV_BITS(B)                                   \
  if (N == 1) gv_launch<B, 1>(a, trans_w, grid, s);        \
  else if (N == 2) gv_launch<B, 2>(a, trans_w, grid, s);   \
  else if (N <= 4) gv_launch<B, 4>(a, trans_w, grid, s);   \
  else gv_launch<B, 8>(a, trans_w, grid, s)
  PACKED_BITS_SWITCH(meta->bits, ADMMQ_GV_BITS)
#undef ADMMQ_GV_BITS
  if (pl.ns > 1)
    hipLaunchKernelGGL(k_packed_gemv_reduce, dim3((unsigned)((N * M + 255) / 256)), dim3(256), 0, s, a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

}  // namespace admmq

using namespace admmq;

extern "C" {

size_t admmq_packed_gemv_workspace_size(const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K, int64_t N) {
  GvPlan pl;
  return plan_gv(meta, trans_w, M, K, N, pl) ? pl.ws : 0;
}

int32_t admmq_packed_gemv(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                          const void* x, int32_t x_dtype, int64_t N, const float* bias, void* y, int32_t y_dtype,
                          void* workspace, size_t workspace_bytes, void* stream) {
  return packed_gemv_run(codes, meta, trans_w, M, K, x, x_dtype, N, bias, y, y_dtype, workspace, workspace_bytes, stream);
}

}  // extern "C"
