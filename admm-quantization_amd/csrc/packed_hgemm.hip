// GEMM of a packed weight with bf16 / fp16 activations on the 16-bit MFMA (include/admmq.h
// "Half-precision packed GEMM"): Y = W X (+ bias), W = D or D^T, D the table
// de-quantization of a packed tensor's codes, X in bfloat16 or float16.
//
// The weight enters the MFMA as an exact integer and its scale moves into a float32 epilogue:
//   mse-minmax / symmetric / affine: a = (u - q) - zp (|a| <= 256: exact in bf16 and in fp16)
//     S = sum_k a x,  y32 = (S scale) + bias[m]
//   tensor_minmax: the operand is u itself (0..255)
//     Su = sum_k u x,  Sx = sum_k x,  y32 = ((Su rng) / n + mn Sx) + bias[m]   (dequant_code's order)
// Sx is a second accumulator against an operand of ones: it runs through the same pieces and the
// same instruction as Su, so its order is a function of K alone like everything else here.
// y32 is stored as float32 or rounded once (to nearest even) to X's type.
//
// The column axis, the two x layouts, the 64 (m) x 64 (c) tile of four waves, the K pieces
// (plan_packed with a K step of 32) and the two regimes are those of k_packed_gemm
// (packed_gemm.hip). A K step is 32: a thread cuts its run of 8 stream-consecutive codes out of
// three dwords as there, and writes them as half values into an LDS image [m][k] whose k index
// is contiguous; the activations go into an image [c][k], 8 consecutive k of one column a thread.
// A lane's operand of v_mfma_f32_32x32x16_{bf16,f16} is the 8 consecutive k = 16 kk + 8 h + j of
// its row, for both operands the same 8 (one 16-byte LDS read each). Rows past M, columns past C
// and k past the piece are exact zeros in the images. Every piece is summed in its own
// accumulator chain from zero and the pieces are added in piece order, in the serial form inside
// the workgroup and in the parallel form by k_packed_hreduce from float32 partial images: the
// same bits. No workgroup waits for another, and nothing is combined with atomics.
//
// X and Y need only be aligned to their element: X is read with 2-byte loads (layout 1: with
// one 16-byte load per thread and step when every row of X starts on a 16-byte boundary), Y is
// written with 2- or 4-byte stores.
#include <algorithm>
#include <type_traits>

#include "../../include/admmq.h"
#include "packed_tile.h"

namespace admmq {

constexpr int kHgBK = 32;                // the K step
constexpr int kHgLD = 40;                // LDS row stride in 16-bit elements: 16-byte aligned rows, 20 dwords apart
constexpr int64_t kHgKMax = int64_t(1) << 24;

typedef float hg_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 hg_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 hg_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned hg_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const unsigned short gcu16;
typedef __attribute__((address_space(1))) const hg_u32x4 gcu32x4;

struct HgArgs {
  const unsigned char* codes;
  const unsigned short* x;   // bf16 / fp16 bits
  const float* bias;
  void* y;
  float* part;        // parallel form: [np][total] float32 partial images in Y's layout
  float* xpart;       // parallel form, tensor_minmax: [np][C] partial column sums of x
  long long nbytes;   // bytes of the code stream
  long long total;    // C * M
  long long C;
  int M, K, N;
  int xl;
  int kp, np, parallel;
  int scheme;
  int off;            // the operand is u - off (q + zp; 0 for tensor_minmax)
  int xal;            // x_layout 1: every row of x starts on a 16-byte boundary
  int ydt;            // ADMMQ_DT_* of y
  float scale, mn, rng, nlev;   // nlev = float(2^bits - 1)
};

// The float32 result of one output: the sums' epilogue, operations rounded one by one
__device__ __forceinline__ float hg_value(float S, float Sx, const HgArgs& a, bool has_bias, float bv) {
  float v;
  if (a.scheme == kMinMax) v = (S * a.rng) / a.nlev + a.mn * Sx;
  else v = S * a.scale;
  return has_bias ? v + bv : v;
}

// y[e] = v as float32, or rounded to nearest even to bf16 / fp16
__device__ __forceinline__ void hg_store(void* y, long long e, float v, int ydt) {
  if (ydt == ADMMQ_DT_F32) static_cast<float*>(y)[e] = v;
  else if (ydt == ADMMQ_DT_BF16) static_cast<__bf16*>(y)[e] = static_cast<__bf16>(v);
  else static_cast<_Float16*>(y)[e] = static_cast<_Float16>(v);
}

// The 16 bits of the integer v (|v| <= 256 for bf16, <= 2048 for fp16: exact)
template <typename T>
__device__ __forceinline__ unsigned hg_int_bits(int v) {
  if constexpr (std::is_same_v<T, __bf16>) return __builtin_bit_cast(unsigned, (float)v) >> 16;
  else return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)(float)v);
}

template <typename T>
__device__ __forceinline__ hg_f32x16 hg_mfma(const hg_u32x4 a, const hg_u32x4 b, const hg_f32x16 c) {
  if constexpr (std::is_same_v<T, __bf16>)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(hg_bf16x8, a), __builtin_bit_cast(hg_bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(hg_f16x8, a), __builtin_bit_cast(hg_f16x8, b), c, 0, 0, 0);
}

template <int BITS, bool TRANS, bool XL, typename T>
__global__ __launch_bounds__(256) void k_packed_hgemm(const HgArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned short sW[2][kPackedBM * kHgLD];
  __shared__ __attribute__((aligned(16))) unsigned short sX[2][kPackedBN * kHgLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, i = lane & 31, h = lane >> 5;
  const int M = a.M, K = a.K, N = a.N;
  const long long C = a.C;
  const int m0 = (int)blockIdx.y * kPackedBM;
  const long long c0 = (long long)blockIdx.x * kPackedBN;
  const int piece = (int)blockIdx.z;
  const int kb = a.parallel ? piece * a.kp : 0;
  const int ke = a.parallel ? min(K, kb + a.kp) : K;
  const unsigned char* __restrict__ codes = a.codes;
  const long long nbytes = a.nbytes;
  const bool mm = a.scheme == kMinMax;   // (uniform)

  // W: this thread's run of 8 stream-consecutive codes of a step's 64 x 32 block, as k_packed_gemm
  const int wrow = TRANS ? 8 * (tid & 7) : (tid >> 2);   // m - m0 of the run's first code
  const int wk = TRANS ? (tid >> 3) : 8 * (tid & 3);     // k - k0 of the run's first code
  const int nvm = TRANS ? min(8, M - (m0 + wrow)) : (m0 + wrow < M ? 8 : 0);   // codes of a full step's run inside W (<= 0: none)
  const long long bit0 = (TRANS ? (long long)(kb + wk) * M + (m0 + wrow) : (long long)(m0 + wrow) * K + (kb + wk)) * BITS;
  const int wsh = (int)(bit0 & 31);    // the run's 8 BITS <= 64 bits start at bit wsh of dword wq: three dwords
  long long wq = bit0 >> 5;
  const long long wstep = TRANS ? (long long)M * BITS : BITS;   // dwords per K step
  // X: the 8 elements k = xk .. xk + 7 of one column of the step's block
  const int xc = XL ? (tid >> 2) : (tid & 63);
  const int xk = XL ? 8 * (tid & 3) : 8 * (tid >> 6);
  const bool cok = c0 + xc < C;
  const unsigned short* __restrict__ xp;
  long long xs;   // elements between two k of the column
  {
    const long long c = min(c0 + xc, C - 1);   // (a column past C reads a valid one and is zeroed)
    if (XL) {
      xp = a.x + c * K + (kb + xk);
      xs = 1;
    } else {
      const long long b = c / N;
      xp = a.x + (b * K + (kb + xk)) * N + (c - b * N);
      xs = N;
    }
  }
  const long long xstep = XL ? kHgBK : (long long)kHgBK * N;

  unsigned cw[3];
  int nv = 0;
  unsigned rx[4];
  // the loads of the next step (each call advances wq and xp by one step)
  auto load = [&](int k0, bool full) {
    cw[0] = 0u; cw[1] = 0u; cw[2] = 0u;
    if (full) nv = nvm;
    else if (TRANS) nv = k0 + wk < ke ? nvm : 0;
    else nv = nvm > 0 ? min(8, ke - (k0 + wk)) : 0;
    if (nv > 0) {
      if (4 * wq + 12 <= nbytes) {   // all three inside the stream: plain loads, issued together
        const gcu32* q = (const gcu32*)(codes + 4 * wq);
        cw[0] = q[0]; cw[1] = q[1]; cw[2] = q[2];
      } else {                       // the stream's end: nothing past its last byte is read
        cw[0] = code_dword(codes, wq, nbytes);
        cw[1] = code_dword(codes, wq + 1, nbytes);
        cw[2] = code_dword(codes, wq + 2, nbytes);
      }
    }
    wq += wstep;
    if (XL && full && a.xal) {   // a row of x from a 16-byte boundary: one load
      const hg_u32x4 v = *(const gcu32x4*)xp;
#pragma unroll
      for (int d = 0; d < 4; ++d) rx[d] = cok ? v[d] : 0u;
    } else if (full) {
      const gcu16* xg = (const gcu16*)xp;
      unsigned e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = xg[(long long)j * xs];
#pragma unroll
      for (int d = 0; d < 4; ++d) rx[d] = cok ? (e[2 * d] | (e[2 * d + 1] << 16)) : 0u;
    } else {
      const gcu16* xg = (const gcu16*)xp;
      const int nk = max(0, min(8, ke - (k0 + xk)));   // elements of the 8 inside the piece
      unsigned e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = j < nk ? (unsigned)xg[(long long)j * xs] : 0u;
#pragma unroll
      for (int d = 0; d < 4; ++d) rx[d] = cok ? (e[2 * d] | (e[2 * d + 1] << 16)) : 0u;
    }
    xp += xstep;
  };
  auto store = [&](int buf) {
    constexpr unsigned mask = (1u << BITS) - 1u;
    // codes 0..3 lie in bits [wsh, wsh + 4 BITS) of (cw1 : cw0); codes 4..7 from bit p2 = wsh + 4 BITS <= 63
    const int p2 = wsh + 4 * BITS;
    const bool up = p2 >= 32;
    unsigned long long win[2];
    win[0] = (((unsigned long long)cw[1] << 32) | cw[0]) >> wsh;
    win[1] = (((unsigned long long)(up ? cw[2] : cw[1]) << 32) | (up ? cw[1] : cw[0])) >> (p2 & 31);
    unsigned b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int v = (int)((unsigned)(win[j >> 2] >> ((j & 3) * BITS)) & mask) - a.off;
      b[j] = j < nv ? hg_int_bits<T>(v) : 0u;   // past the run's row / the piece / the matrix: exactly 0
    }
    if (TRANS) {
#pragma unroll
      for (int j = 0; j < 8; ++j) sW[buf][(wrow + j) * kHgLD + wk] = (unsigned short)b[j];
    } else {
      hg_u32x4 v;
#pragma unroll
      for (int d = 0; d < 4; ++d) v[d] = b[2 * d] | (b[2 * d + 1] << 16);
      *reinterpret_cast<hg_u32x4*>(&sW[buf][wrow * kHgLD + wk]) = v;
    }
    hg_u32x4 xv;
#pragma unroll
    for (int d = 0; d < 4; ++d) xv[d] = rx[d];
    *reinterpret_cast<hg_u32x4*>(&sX[buf][xc * kHgLD + xk]) = xv;
  };

  // the ones operand of the column sums (tensor_minmax): 1.0 in every element
  const unsigned one2 = hg_int_bits<T>(1) * 0x10001u;
  hg_u32x4 ones;
#pragma unroll
  for (int d = 0; d < 4; ++d) ones[d] = one2;

  hg_f32x16 acc, tot, xacc, xtot;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[r] = 0.f; tot[r] = 0.f; xacc[r] = 0.f; xtot[r] = 0.f; }
  bool first = true;
  int pend = kb + a.kp;   // the current piece's end
  load(kb, kb + kHgBK <= ke);
  store(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = kb; k0 < ke; k0 += kHgBK) {
    const bool more = k0 + kHgBK < ke;
    if (more) load(k0 + kHgBK, k0 + 2 * kHgBK <= ke);
    const unsigned short* w = sW[buf] + (32 * wm + i) * kHgLD + 8 * h;
    const unsigned short* x = sX[buf] + (32 * wn + i) * kHgLD + 8 * h;
#pragma unroll
    for (int kk = 0; kk < kHgBK / 16; ++kk) {
      const hg_u32x4 av = *reinterpret_cast<const hg_u32x4*>(w + 16 * kk);
      const hg_u32x4 bv = *reinterpret_cast<const hg_u32x4*>(x + 16 * kk);
      if (XL) acc = hg_mfma<T>(bv, av, acc);
      else acc = hg_mfma<T>(av, bv, acc);
      if (mm) {
        if (XL) xacc = hg_mfma<T>(bv, ones, xacc);
        else xacc = hg_mfma<T>(ones, bv, xacc);
      }
    }
    if (!more || k0 + kHgBK == pend) {   // a piece ends: fold it into the running sums
      pend += a.kp;
      if (first) {
        tot = acc;
        xtot = xacc;
        first = false;
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) { tot[r] = tot[r] + acc[r]; xtot[r] = xtot[r] + xacc[r]; }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[r] = 0.f; xacc[r] = 0.f; }
    }
    if (more) store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // Epilogue. XL: lanes along m, rows along the columns (Y[c M + m]); else lanes along the
  // columns (Y[(b M + m) N + n]). Parallel form: the piece's sums as they are; the column sums
  // of x (every row of xtot holds them) are written by the first row of tiles.
  if (a.parallel) {
    float* const dst = a.part + (long long)piece * a.total;
    float* const xdst = (mm && blockIdx.y == 0) ? a.xpart + (long long)piece * C : nullptr;
    if (XL) {
      const int m = m0 + 32 * wm + i;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long c = c0 + 32 * wn + PACKED_ROW(r);
        if (c < C && m < M) dst[c * M + m] = tot[r];
        if (xdst && wm == 0 && i == 0 && c < C) xdst[c] = xtot[r];
      }
    } else {
      const long long c = c0 + 32 * wn + i;
      if (c >= C) return;
      const long long b = c / N;
      const long long ybase = b * M * N + (c - b * N);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + 32 * wm + PACKED_ROW(r);
        if (m < M) dst[ybase + (long long)m * N] = tot[r];
      }
      if (xdst && wm == 0 && h == 0) xdst[c] = xtot[0];
    }
    return;
  }
  const float* __restrict__ bias = a.bias;
  if (XL) {
    const int m = m0 + 32 * wm + i;
    if (m >= M) return;
    const float bv = bias ? bias[m] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long c = c0 + 32 * wn + PACKED_ROW(r);
      if (c < C) hg_store(a.y, c * M + m, hg_value(tot[r], xtot[r], a, bias != nullptr, bv), a.ydt);
    }
  } else {
    const long long c = c0 + 32 * wn + i;
    if (c >= C) return;
    const long long b = c / N;
    const long long ybase = b * M * N + (c - b * N);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + 32 * wm + PACKED_ROW(r);
      if (m < M)
        hg_store(a.y, ybase + (long long)m * N, hg_value(tot[r], xtot[r], a, bias != nullptr, bias ? bias[m] : 0.f), a.ydt);
    }
  }
}

// Y[e] = epilogue(((part_0[e] + part_1[e]) + ...), ((xpart_0[c] + xpart_1[c]) + ...)): the piece order of the serial form
__global__ __launch_bounds__(256) void k_packed_hreduce(const HgArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  float s = a.part[e];
  for (int p = 1; p < a.np; ++p) s = s + a.part[(long long)p * a.total + e];
  const int M = a.M, N = a.N;
  int m;
  long long c;
  if (a.xl) {
    c = e / M;
    m = (int)(e - c * M);
  } else {
    const long long bm = e / N;   // b M + m
    const long long b = bm / M;
    m = (int)(bm - b * M);
    c = b * N + (e - bm * N);
  }
  float sx = 0.f;
  if (a.scheme == kMinMax) {
    sx = a.xpart[c];
    for (int p = 1; p < a.np; ++p) sx = sx + a.xpart[(long long)p * a.C + c];
  }
  hg_store(a.y, e, hg_value(s, sx, a, a.bias != nullptr, a.bias ? a.bias[m] : 0.f), a.ydt);
}

// --- host side ------------------------------------------------------------------------------------

// The float path's plan (K step 32, K <= 2^24, M K < 2^40, float32 partial images); tensor_minmax adds
// the partial column sums of x in the parallel regime: np C floats behind the images
static bool plan_hg(const ::admmq_qmeta* meta, int64_t M, int64_t K, int64_t N, int64_t nb, PackedPlan& pl) {
  if (!meta) return false;
  if (!plan_packed(M, K, N, nb, kHgBK, kHgKMax, sizeof(float), pl) || M * K >= (int64_t(1) << 40)) return false;
  if (pl.parallel && meta->scheme == kMinMax) pl.ws += (size_t)pl.np * (size_t)pl.C * sizeof(float);
  return true;
}

static size_t dt_bytes(int32_t dt) { return dt == ADMMQ_DT_F32 ? 4 : 2; }

static int32_t packed_hgemm_run(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                                const void* x, int32_t x_dtype, int32_t x_layout, int64_t N, int32_t nb,
                                const float* bias, void* y, int32_t y_dtype, void* workspace, size_t workspace_bytes,
                                void* stream) {
  const char* const who = "packed_hgemm";
  if (!codes || !x || !y || !meta) return packed_fail(who, ADMMQ_ERR_ARG, "codes, meta, x and y must not be NULL");
  if (M <= 0 || K <= 0 || N <= 0 || nb <= 0) return packed_fail(who, ADMMQ_ERR_ARG, "M, K, N and nb must be positive");
  int32_t rc = packed_meta_check(meta, who, false, nullptr);
  if (rc != ADMMQ_OK) return rc;
  if (trans_w != 0 && trans_w != 1) return packed_fail(who, ADMMQ_ERR_ARG, "trans_w must be 0 or 1");
  if (x_layout != 0 && x_layout != 1) return packed_fail(who, ADMMQ_ERR_ARG, "x_layout must be 0 or 1");
  if (x_layout == 1 && nb != 1) return packed_fail(who, ADMMQ_ERR_ARG, "x_layout 1 (linear) needs nb = 1");
  if (x_dtype != ADMMQ_DT_F16 && x_dtype != ADMMQ_DT_BF16)
    return packed_fail(who, ADMMQ_ERR_ARG, "x_dtype must be ADMMQ_DT_F16 or ADMMQ_DT_BF16");
  if (y_dtype != ADMMQ_DT_F32 && y_dtype != x_dtype)
    return packed_fail(who, ADMMQ_ERR_ARG, "y_dtype must be ADMMQ_DT_F32 or x_dtype");
  // the integer operand must be exact in x's type: 8 significant bits in bf16, 11 in fp16
  const int64_t q = int64_t(1) << (meta->bits - 1);
  const int64_t zp = meta->scheme == kAffine ? (int64_t)meta->zero_point : 0;
  const int64_t lim = x_dtype == ADMMQ_DT_BF16 ? 256 : 2048;
  if (meta->scheme != kMinMax && (-q - zp < -lim || q - 1 - zp > lim))
    return packed_fail(who, ADMMQ_ERR_ARG, "affine zero_point puts (u - q) - zero_point outside the integers exact in x_dtype");
  if ((reinterpret_cast<uintptr_t>(codes) & 15) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "codes must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(x) & 1) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "x must be aligned to its 2-byte element");
  if ((reinterpret_cast<uintptr_t>(y) & (dt_bytes(y_dtype) - 1)) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "y must be aligned to its element");
  if ((reinterpret_cast<uintptr_t>(bias) & 3) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "bias must be float aligned");
  PackedPlan pl;
  if (!plan_hg(meta, M, K, N, nb, pl)) return packed_fail(who, ADMMQ_ERR_ARG, "sizes out of range");
  rc = packed_ws_check(who, pl, workspace, workspace_bytes, "float");
  if (rc != ADMMQ_OK) return rc;
  HgArgs a;
  a.codes = codes; a.x = static_cast<const unsigned short*>(x); a.bias = bias; a.y = y;
  a.part = pl.parallel ? static_cast<float*>(workspace) : nullptr;
  a.xpart = pl.parallel ? a.part + (size_t)pl.np * (size_t)pl.total : nullptr;
  a.nbytes = (long long)admmq_packed_bytes(M * K, meta->bits);
  a.total = pl.total; a.C = pl.C;
  a.M = (int)M; a.K = (int)K; a.N = (int)N;
  a.xl = x_layout;
  a.kp = pl.kp; a.np = pl.np; a.parallel = pl.parallel;
  a.scheme = meta->scheme;
  a.off = meta->scheme == kMinMax ? 0 : (int)(q + zp);
  a.xal = (x_layout == 1 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && K % 8 == 0) ? 1 : 0;
  a.ydt = y_dtype;
  a.scale = meta->scale; a.mn = meta->mn; a.rng = meta->rng;
  a.nlev = (float)((1 << meta->bits) - 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)pl.tiles_c, (unsigned)pl.tiles_m, pl.parallel ? (unsigned)pl.np : 1u);
  const bool bf = x_dtype == ADMMQ_DT_BF16;
#define ADMMQ_HG_LAUNCH(B, T, X)                                                                   \
  do {                                                                                             \
    if (bf) hipLaunchKernelGGL((k_packed_hgemm<B, T, X, __bf16>), grid, dim3(256), 0, s, a);       \
    else hipLaunchKernelGGL((k_packed_hgemm<B, T, X, _Float16>), grid, dim3(256), 0, s, a);        \
  } while (0)
#define ADMMQ_HG_BITS(B)                                     \
  if (trans_w && x_layout) ADMMQ_HG_LAUNCH(B, true, true);   \
  else if (trans_w) ADMMQ_HG_LAUNCH(B, true, false);         \
  else if (x_layout) ADMMQ_HG_LAUNCH(B, false, true);        \
  else ADMMQ_HG_LAUNCH(B, false, false)
  PACKED_BITS_SWITCH(meta->bits, ADMMQ_HG_BITS)
#undef ADMMQ_HG_BITS
#undef ADMMQ_HG_LAUNCH
  if (pl.parallel)
    hipLaunchKernelGGL(k_packed_hreduce, dim3((unsigned)((pl.total + 255) / 256)), dim3(256), 0, s, a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

}  // namespace admmq

using namespace admmq;

extern "C" {

size_t admmq_packed_hgemm_workspace_size(const admmq_qmeta* meta, int64_t M, int64_t K, int64_t N, int32_t nb) {
  PackedPlan pl;
  return plan_hg(meta, M, K, N, nb, pl) ? pl.ws : 0;
}

int32_t admmq_packed_hgemm(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                           const void* x, int32_t x_dtype, int32_t x_layout, int64_t N, int32_t nb, const float* bias,
                           void* y, int32_t y_dtype, void* workspace, size_t workspace_bytes, void* stream) {
  return packed_hgemm_run(codes, meta, trans_w, M, K, x, x_dtype, x_layout, N, nb, bias, y, y_dtype, workspace,
                          workspace_bytes, stream);
}

}  // extern "C"
