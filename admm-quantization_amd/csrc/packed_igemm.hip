// Integer-arithmetic packed layers (include/admmq.h "Integer packed GEMM"):
// activation codes as a tensor of their own (k_act_encode / k_act_decode), the integer row
// sums of a packed weight (k_packed_rowsum) and the GEMM of a packed weight with activation
// codes on v_mfma_i32_32x32x32_i8 (k_packed_igemm, k_packed_ireduce).
//
//   W = s a,  a[m,k] = (uw - q) - zp  (an int8)      x = g ux + mn_x,  g = rng_x / n_x
//   S[m,c] = sum_k a[m,k] ux[k,c]     A[m] = sum_k a[m,k]              (exact integers)
//   y[m,c] = float(double(s) (g double(S) + double(mn_x) double(A[m])) + double(bias[m]))
//
// The column axis, the two x layouts, the 64 (m) x 64 (c) tile of four waves and the two
// regimes are those of k_packed_gemm (packed_gemm.hip). A K step is 64: the step's weight
// codes are cut out of the bit stream in runs of 8 (three dwords a run, two runs a thread)
// and written as int8 a into an LDS image [m][k] whose k index is contiguous; the activation
// bytes are written as ux - 128 (one xor: an int8) into an image [c][k]. A lane's MFMA
// operand is 16 consecutive k of its row, for both operands the same 16 (k = 32 kk + 16 h + j
// for element j of lane half h): the product sums over k, so the only property of the
// instruction's operand map that the result depends on is that element j of lane half h means
// the same k in A as in B. The accumulator holds sum_k a (ux - 128); the epilogue adds
// 128 A[m] back. Rows past M, columns past C and k past K are the int8 value 0 in the images.
// The sum is an integer, so every order gives the same bits: the serial regime keeps one
// accumulator over all of K, the parallel one (few tiles) writes one int32 partial image per
// K piece and k_packed_ireduce adds them and runs the epilogue.
#include <algorithm>

#include "../../include/admmq.h"
#include "packed_tile.h"

namespace admmq {

constexpr int kIgBK = 64;                // the K step (kPackedPieceMin is a multiple of it)
constexpr int kIgLD = 80;                // LDS row stride in bytes: 16-byte aligned rows, 20 dwords apart
constexpr int64_t kIgKMax = 65536;       // 128 255 K < 2^31

typedef int ig_i32x16 __attribute__((ext_vector_type(16)));
typedef int ig_i32x4 __attribute__((ext_vector_type(4)));

// --- activation codes ---------------------------------------------------------------------------
// fixed_quant's r and qi; the code is qi clamped to [0, n] (a NaN: 0). cnt counts the clamped ones.
__device__ __forceinline__ unsigned act_code(float x, const ActQ& q, int& cnt) {
  const float r = (x - q.mn) / q.rng;
  const float qi = __builtin_floorf(r * q.n + 0.5f);
  const bool in = qi >= 0.f && qi <= q.n;   // false for a NaN
  cnt += in ? 0 : 1;
  const float c = qi >= 0.f ? (qi <= q.n ? qi : q.n) : 0.f;
  return (unsigned)(int)c;
}
__device__ __forceinline__ float act_value(unsigned u, const ActQ& q) { return ((float)u * q.rng) / q.n + q.mn; }

// The block's count into *counter by one atomic (none for a zero count). All 256 threads call.
__device__ __forceinline__ void block_count_add(int cnt, int* counter) {
  __shared__ int sc[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = sc[0] + sc[1] + sc[2] + sc[3];
    if (t > 0) atomicAdd(counter, t);
  }
}

// codes[i] = act_code(x[i]), grid-stride. Elements [head, head + 16 nvec) go as four 16-byte loads
// and one 16-byte store (the host sets head so that both pointers are 16-byte aligned there;
// nvec = 0 when they cannot be), the rest one by one, as k_fixed_quant.
__global__ __launch_bounds__(256) void k_act_encode(const float* __restrict__ x, unsigned char* __restrict__ y,
                                                    long long numel, long long head, long long nvec, const ActQ q,
                                                    int* __restrict__ clamped) {
  const long long step = (long long)blockDim.x * gridDim.x;
  const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const float4* xv = reinterpret_cast<const float4*>(x + head);
  uint4* yv = reinterpret_cast<uint4*>(y + head);
  int cnt = 0;
  for (long long i = t0; i < nvec; i += step) {
    unsigned w[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const float4 v = xv[4 * i + d];
      w[d] = act_code(v.x, q, cnt) | (act_code(v.y, q, cnt) << 8) | (act_code(v.z, q, cnt) << 16) |
             (act_code(v.w, q, cnt) << 24);
    }
    yv[i] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  const long long vend = head + 16 * nvec;
  const long long ns = head + (numel - vend);   // scalar elements: [0, head) and [vend, numel)
  for (long long s = t0; s < ns; s += step) {
    const long long e = s < head ? s : vend + (s - head);
    y[e] = (unsigned char)act_code(x[e], q, cnt);
  }
  if (clamped) block_count_add(cnt, clamped);   // (uniform: a kernel argument)
}

__global__ __launch_bounds__(256) void k_act_decode(const unsigned char* __restrict__ x, float* __restrict__ y,
                                                    long long numel, long long head, long long nvec, const ActQ q) {
  const long long step = (long long)blockDim.x * gridDim.x;
  const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const uint4* xv = reinterpret_cast<const uint4*>(x + head);
  float4* yv = reinterpret_cast<float4*>(y + head);
  for (long long i = t0; i < nvec; i += step) {
    const uint4 v = xv[i];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int d = 0; d < 4; ++d)
      yv[4 * i + d] = make_float4(act_value(w[d] & 255u, q), act_value((w[d] >> 8) & 255u, q),
                                  act_value((w[d] >> 16) & 255u, q), act_value(w[d] >> 24, q));
  }
  const long long vend = head + 16 * nvec;
  const long long ns = head + (numel - vend);
  for (long long s = t0; s < ns; s += step) {
    const long long e = s < head ? s : vend + (s - head);
    y[e] = act_value(x[e], q);
  }
}

// --- row sums -----------------------------------------------------------------------------------
// Code i of a stream (any bit offset: two dwords at most for bits <= 8)
__device__ __forceinline__ unsigned code_at(const unsigned char* __restrict__ c, long long i, int bits, long long nbytes) {
  const long long bit = i * bits;
  const long long w = bit >> 5;
  const int sh = (int)(bit & 31);
  unsigned long long win = code_dword(c, w, nbytes);
  if (sh + bits > 32) win |= (unsigned long long)code_dword(c, w + 1, nbytes) << 32;
  return (unsigned)(win >> sh) & ((1u << bits) - 1u);
}

// A[m] = sum_k a[m,k] = (sum_k uw) - K off, off = q + zp. trans 0 (the stream is [M][K]): one wave
// per row, the lanes stride over k. trans 1 (the stream is [K][M]): a wave takes 64 neighbouring m
// (its lanes read neighbouring codes) and a quarter of the k, and the block's four waves are
// added through LDS. Runs once per weight.
__global__ __launch_bounds__(256) void k_packed_rowsum(const unsigned char* __restrict__ codes, long long nbytes, int bits,
                                                       int trans, int M, int K, int off, int* __restrict__ A) {
  if (trans) {
    __shared__ int part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long m = (long long)blockIdx.x * 64 + lane;
    int s = 0;
    if (m < M)
      for (int k = wave; k < K; k += 4) s += (int)code_at(codes, (long long)k * M + m, bits, nbytes);
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && m < M) A[m] = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane] - K * off;
  } else {
    const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;   // (a whole wave; no barrier on this path)
    int s = 0;
    for (int k = threadIdx.x & 63; k < K; k += 64) s += (int)code_at(codes, m * K + k, bits, nbytes);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) A[m] = s - K * off;
  }
}

// --- the GEMM -----------------------------------------------------------------------------------
struct IgArgs {
  const unsigned char* codes;
  const unsigned char* x;
  const float* bias;
  const int* rowsum;
  float* y;
  unsigned char* yc;
  int* part;          // parallel form: [np][total] int32 partial images in Y's layout
  int* clamped;       // codes output: the clamp counter, or NULL
  long long nbytes;   // bytes of the code stream
  long long total;    // C * M
  long long C;
  int M, K, N;
  int xl;
  int kp, np, parallel;
  int off;            // q + zp: a = uw - off
  int xal;            // x_layout 1: every row of x starts on a dword, so full steps load dwords
  int out;            // (k_packed_ireduce) 0 float, 1 float + quantizer, 2 codes
  double s, g, mnx;   // the weight's scale, rng_x / n_x, mn_x
  ActQ oq;
};

// The output formula: double operations rounded one by one (-ffp-contract=off), one rounding to float32.
// acc = sum_k a (ux - 128); S = acc + 128 A is exact in int64 and in double.
__device__ __forceinline__ float ig_value(int acc, int A, const IgArgs& a, bool has_bias, float bv) {
  const double S = (double)((long long)acc + 128ll * (long long)A);
  double v = a.s * (a.g * S + a.mnx * (double)A);
  if (has_bias) v = v + (double)bv;
  return (float)v;
}

constexpr int kIgFloat = 0, kIgQuant = 1, kIgCodes = 2;

template <int BITS, bool TRANS, bool XL, int OUT>
__global__ __launch_bounds__(256) void k_packed_igemm(const IgArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char sW[2][kPackedBM * kIgLD];
  __shared__ __attribute__((aligned(16))) unsigned char sX[2][kPackedBN * kIgLD];
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

  // W: two runs of 8 stream-consecutive codes of a step's 64 x 64 block (run id = tid + 256 u;
  // 8 runs to a row of the stream: along k for TRANS = 0, along m for 1). A step advances the
  // stream by 64 (x M) BITS bits, whole dwords, so a run's bit offset in its first dword is fixed.
  int wrow[2], wk[2], nvm[2], wsh[2];
  long long wq[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int id = tid + 256 * u;
    wrow[u] = TRANS ? 8 * (id & 7) : (id >> 3);   // m - m0 of the run's first code
    wk[u] = TRANS ? (id >> 3) : 8 * (id & 7);     // k - k0 of the run's first code
    nvm[u] = TRANS ? min(8, M - (m0 + wrow[u])) : (m0 + wrow[u] < M ? 8 : 0);
    const long long bit0 =
        (TRANS ? (long long)(kb + wk[u]) * M + (m0 + wrow[u]) : (long long)(m0 + wrow[u]) * K + (kb + wk[u])) * BITS;
    wsh[u] = (int)(bit0 & 31);
    wq[u] = bit0 >> 5;
  }
  const long long wstep = TRANS ? (long long)2 * M * BITS : 2 * BITS;   // dwords per K step
  // X: the 16 bytes k = xk .. xk + 15 of one column of the step's block
  const int xc = XL ? (tid >> 2) : (tid & 63);
  const int xk = XL ? 16 * (tid & 3) : 16 * (tid >> 6);
  const bool cok = c0 + xc < C;
  const unsigned char* __restrict__ xp;
  long long xs;   // bytes between two k of the column
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
  const long long xstep = XL ? kIgBK : (long long)kIgBK * N;

  unsigned cw[2][3];
  int nv[2] = {0, 0};
  unsigned rx[4];
  // the loads of the next step (each call advances wq and xp by one step)
  auto load = [&](int k0, bool full) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      cw[u][0] = 0u; cw[u][1] = 0u; cw[u][2] = 0u;
      if (full) nv[u] = nvm[u];
      else if (TRANS) nv[u] = k0 + wk[u] < ke ? nvm[u] : 0;
      else nv[u] = nvm[u] > 0 ? min(8, ke - (k0 + wk[u])) : 0;
      if (nv[u] > 0) {
        if (4 * wq[u] + 12 <= nbytes) {   // all three inside the stream
          const unsigned* q = reinterpret_cast<const unsigned*>(codes + 4 * wq[u]);
          cw[u][0] = q[0]; cw[u][1] = q[1]; cw[u][2] = q[2];
        } else {                          // the stream's end: nothing past its last byte is read
          cw[u][0] = code_dword(codes, wq[u], nbytes);
          cw[u][1] = code_dword(codes, wq[u] + 1, nbytes);
          cw[u][2] = code_dword(codes, wq[u] + 2, nbytes);
        }
      }
      wq[u] += wstep;
    }
    if (XL && full && a.xal) {   // a row of x from a dword boundary: four dwords
      const unsigned* q = reinterpret_cast<const unsigned*>(xp);
#pragma unroll
      for (int d = 0; d < 4; ++d) rx[d] = cok ? (q[d] ^ 0x80808080u) : 0u;
    } else {
      const int nk = full ? 16 : max(0, min(16, ke - (k0 + xk)));   // bytes of the 16 inside the piece
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        unsigned v = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * d + j < nk) v |= ((unsigned)xp[(long long)(4 * d + j) * xs] ^ 0x80u) << (8 * j);
        rx[d] = cok ? v : 0u;
      }
    }
    xp += xstep;
  };
  auto store = [&](int buf) {
    constexpr unsigned mask = (1u << BITS) - 1u;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      // codes 0..3 lie in bits [wsh, wsh + 4 BITS) of (cw1 : cw0); codes 4..7 from bit p2 = wsh + 4 BITS <= 63
      const int p2 = wsh[u] + 4 * BITS;
      const bool up = p2 >= 32;
      unsigned long long win[2];
      win[0] = (((unsigned long long)cw[u][1] << 32) | cw[u][0]) >> wsh[u];
      win[1] = (((unsigned long long)(up ? cw[u][2] : cw[u][1]) << 32) | (up ? cw[u][1] : cw[u][0])) >> (p2 & 31);
      unsigned b[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = (int)((unsigned)(win[j >> 2] >> ((j & 3) * BITS)) & mask) - a.off;
        b[j] = j < nv[u] ? ((unsigned)v & 255u) : 0u;   // past the run's row / the piece / the matrix: 0
      }
      if (TRANS) {
#pragma unroll
        for (int j = 0; j < 8; ++j) sW[buf][(wrow[u] + j) * kIgLD + wk[u]] = (unsigned char)b[j];
      } else {
        const unsigned lo = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        const unsigned hi = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        *reinterpret_cast<uint2*>(&sW[buf][wrow[u] * kIgLD + wk[u]]) = make_uint2(lo, hi);
      }
    }
    *reinterpret_cast<uint4*>(&sX[buf][xc * kIgLD + xk]) = make_uint4(rx[0], rx[1], rx[2], rx[3]);
  };

  ig_i32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0;
  load(kb, kb + kIgBK <= ke);
  store(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = kb; k0 < ke; k0 += kIgBK) {
    const bool more = k0 + kIgBK < ke;
    if (more) load(k0 + kIgBK, k0 + 2 * kIgBK <= ke);
    const unsigned char* w = sW[buf] + (32 * wm + i) * kIgLD + 16 * h;
    const unsigned char* x = sX[buf] + (32 * wn + i) * kIgLD + 16 * h;
#pragma unroll
    for (int kk = 0; kk < kIgBK / 32; ++kk) {
      const ig_i32x4 av = *reinterpret_cast<const ig_i32x4*>(w + 32 * kk);
      const ig_i32x4 bv = *reinterpret_cast<const ig_i32x4*>(x + 32 * kk);
      if (XL) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(bv, av, acc, 0, 0, 0);
      else acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc, 0, 0, 0);
    }
    if (more) store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // Epilogue. XL: lanes along m, rows along the columns (Y[c M + m]); else lanes along the
  // columns (Y[(b M + m) N + n]). An output element belongs to one lane and one register.
  int cnt = 0;
  if (XL) {
    const int m = m0 + 32 * wm + i;
    const bool mok = m < M;
    const int A = (mok && !a.parallel) ? a.rowsum[m] : 0;
    const bool hb = a.bias != nullptr;
    const float bv = (mok && hb && !a.parallel) ? a.bias[m] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long c = c0 + 32 * wn + PACKED_ROW(r);
      if (!mok || c >= C) continue;
      const long long e = c * M + m;
      if (a.parallel) {
        a.part[(long long)piece * a.total + e] = acc[r];
      } else {
        const float v = ig_value(acc[r], A, a, hb, bv);
        if constexpr (OUT == kIgCodes) a.yc[e] = (unsigned char)act_code(v, a.oq, cnt);
        else if constexpr (OUT == kIgQuant) a.y[e] = fixed_quant(v, a.oq);
        else a.y[e] = v;
      }
    }
  } else {
    const long long c = c0 + 32 * wn + i;
    const bool ok = c < C;
    const long long cc = ok ? c : 0;
    const long long b = cc / N;
    const long long ybase = b * M * N + (cc - b * N);
    const bool hb = a.bias != nullptr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + 32 * wm + PACKED_ROW(r);
      if (!ok || m >= M) continue;
      const long long e = ybase + (long long)m * N;
      if (a.parallel) {
        a.part[(long long)piece * a.total + e] = acc[r];
      } else {
        const float v = ig_value(acc[r], a.rowsum[m], a, hb, hb ? a.bias[m] : 0.f);
        if constexpr (OUT == kIgCodes) a.yc[e] = (unsigned char)act_code(v, a.oq, cnt);
        else if constexpr (OUT == kIgQuant) a.y[e] = fixed_quant(v, a.oq);
        else a.y[e] = v;
      }
    }
  }
  if constexpr (OUT == kIgCodes) {
    if (a.clamped) block_count_add(cnt, a.clamped);   // (uniform; every thread arrives: no return above)
  }
}

// The parallel regime's second kernel: S = sum of the piece images (any order: integers), then the epilogue.
__global__ __launch_bounds__(256) void k_packed_ireduce(const IgArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  int cnt = 0;
  if (e < a.total) {
    int s = a.part[e];
    for (int p = 1; p < a.np; ++p) s += a.part[(long long)p * a.total + e];
    const int m = (int)(a.xl ? e % a.M : (e / a.N) % a.M);
    const bool hb = a.bias != nullptr;
    const float v = ig_value(s, a.rowsum[m], a, hb, hb ? a.bias[m] : 0.f);
    if (a.out == kIgCodes) a.yc[e] = (unsigned char)act_code(v, a.oq, cnt);
    else if (a.out == kIgQuant) a.y[e] = fixed_quant(v, a.oq);
    else a.y[e] = v;
  }
  if (a.out == kIgCodes && a.clamped) block_count_add(cnt, a.clamped);
}

// The integer path's plan (plan_packed, packed_gemm.hip): K <= 65536, pieces that are multiples of
// the 64-wide K step, int32 partial images
static bool plan_ig(int64_t M, int64_t K, int64_t N, int64_t nb, PackedPlan& pl) {
  return plan_packed(M, K, N, nb, kIgBK, kIgKMax, sizeof(int32_t), pl);
}
static bool plan_ig_dw(int64_t M, int64_t K, int64_t Ho, int64_t Wo, int64_t nb, PackedPlan& pl) {
  return plan_packed_dw(M, K, Ho, Wo, nb, kIgBK, kIgKMax, sizeof(int32_t), pl);
}

static bool act_bits_ok(const admmq_actq* q) { return q && q->on != 0 && q->bits >= 2 && q->bits <= 8; }

// head / nvec of the element-wise kernels: 16 elements a vector, both pointers 16-byte aligned at head
static void vec_split(uintptr_t bytes_ptr, uintptr_t float_ptr, long long numel, long long& head, long long& nvec) {
  head = (long long)((16 - (bytes_ptr & 15)) & 15);
  nvec = 0;
  if (head > numel) head = numel;
  if (((float_ptr + 4 * (uintptr_t)head) & 15) == 0) nvec = (numel - head) / 16;
  else head = numel;
}

// The GEMM's arguments common to admmq_packed_igemm and admmq_packed_idwgemm. x_q: the quantizer
// of the GEMM's activation operand (x, or the mid quantizer of the fused stage).
static void ig_fill(IgArgs& a, const uint8_t* codes, const admmq_qmeta* meta, int off, const uint8_t* x,
                    const admmq_actq* x_q, const int32_t* rowsums, const float* bias, float* y, uint8_t* y_codes,
                    const admmq_actq* out_q, int32_t* clamped, void* workspace, const PackedPlan& pl, int64_t M, int64_t K,
                    int64_t N, int32_t x_layout) {
  const bool oq = out_q && out_q->on != 0;
  a.codes = codes; a.x = x; a.bias = bias; a.rowsum = rowsums; a.y = y; a.yc = y_codes;
  a.part = pl.parallel ? static_cast<int*>(workspace) : nullptr;
  a.clamped = y_codes ? clamped : nullptr;
  a.nbytes = (long long)admmq_packed_bytes(M * K, meta->bits);
  a.total = pl.total; a.C = pl.C;
  a.M = (int)M; a.K = (int)K; a.N = (int)N;
  a.xl = x_layout;
  a.kp = pl.kp; a.np = pl.np; a.parallel = pl.parallel;
  a.off = off;
  a.xal = (x_layout == 1 && (reinterpret_cast<uintptr_t>(x) & 3) == 0 && (K & 3) == 0) ? 1 : 0;
  a.out = y_codes ? kIgCodes : (oq ? kIgQuant : kIgFloat);
  a.s = (double)meta->scale;
  a.g = (double)x_q->rng / (double)((1 << x_q->bits) - 1);
  a.mnx = (double)x_q->mn;
  a.oq = oq ? actq_make(out_q) : ActQ{0.f, 0.f, 0.f, 0};
}

// Zeroes a clamp counter on the stream (none: nothing)
static int32_t counter_reset(int32_t* counter, hipStream_t s) {
  if (!counter) return ADMMQ_OK;
  const hipError_t e = hipMemsetAsync(counter, 0, sizeof(int32_t), s);
  return e == hipSuccess ? ADMMQ_OK : set_error(ADMMQ_ERR_HIP, hipGetErrorString(e));
}

// The parallel form's second kernel, then the launches' status
static int32_t ig_finish(const IgArgs& a, const PackedPlan& pl, hipStream_t s) {
  if (pl.parallel)
    hipLaunchKernelGGL(k_packed_ireduce, dim3((unsigned)((pl.total + 255) / 256)), dim3(256), 0, s, a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

}  // namespace admmq

using namespace admmq;

extern "C" {

int32_t admmq_act_encode(const float* x, uint8_t* codes, int64_t numel, const admmq_actq* q, int32_t* clamped,
                         void* stream) {
  if (!x || !codes) return set_error(ADMMQ_ERR_ARG, "act_encode: x and codes must not be NULL");
  if (!q || q->on == 0) return set_error(ADMMQ_ERR_ARG, "act_encode: q must not be NULL or off (on == 0)");
  if (q->bits < 2 || q->bits > 8) return set_error(ADMMQ_ERR_ARG, "act_encode: bits must be 2..8 (1 bit has no code form)");
  if (numel <= 0) return set_error(ADMMQ_ERR_ARG, "act_encode: numel must be positive");
  const uintptr_t xa = reinterpret_cast<uintptr_t>(x), ya = reinterpret_cast<uintptr_t>(codes);
  if ((xa & 3) != 0) return set_error(ADMMQ_ERR_ARG, "act_encode: x must be float aligned");
  if ((reinterpret_cast<uintptr_t>(clamped) & 3) != 0) return set_error(ADMMQ_ERR_ARG, "act_encode: clamped must be int32 aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (clamped) {
    const hipError_t e = hipMemsetAsync(clamped, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(e));
  }
  long long head, nvec;
  vec_split(ya, xa, numel, head, nvec);
  const long long ns = head + (numel - (head + 16 * nvec));
  long long nblk = (std::max(nvec, ns) + 255) / 256;
  nblk = std::min<long long>(std::max<long long>(nblk, 1), 8192);
  hipLaunchKernelGGL(k_act_encode, dim3((unsigned)nblk), dim3(256), 0, s, x, codes, (long long)numel, head, nvec,
                     actq_make(q), clamped);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

int32_t admmq_act_decode(const uint8_t* codes, float* y, int64_t numel, const admmq_actq* q, void* stream) {
  if (!codes || !y) return set_error(ADMMQ_ERR_ARG, "act_decode: codes and y must not be NULL");
  if (!q || q->on == 0) return set_error(ADMMQ_ERR_ARG, "act_decode: q must not be NULL or off (on == 0)");
  if (q->bits < 2 || q->bits > 8) return set_error(ADMMQ_ERR_ARG, "act_decode: bits must be 2..8 (1 bit has no code form)");
  if (numel <= 0) return set_error(ADMMQ_ERR_ARG, "act_decode: numel must be positive");
  const uintptr_t xa = reinterpret_cast<uintptr_t>(codes), ya = reinterpret_cast<uintptr_t>(y);
  if ((ya & 3) != 0) return set_error(ADMMQ_ERR_ARG, "act_decode: y must be float aligned");
  long long head, nvec;
  vec_split(xa, ya, numel, head, nvec);
  const long long ns = head + (numel - (head + 16 * nvec));
  long long nblk = (std::max(nvec, ns) + 255) / 256;
  nblk = std::min<long long>(std::max<long long>(nblk, 1), 8192);
  hipLaunchKernelGGL(k_act_decode, dim3((unsigned)nblk), dim3(256), 0, static_cast<hipStream_t>(stream), codes, y,
                     (long long)numel, head, nvec, actq_make(q));
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

int32_t admmq_packed_rowsums(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                             int32_t* rowsums, void* stream) {
  if (!codes || !meta || !rowsums) return set_error(ADMMQ_ERR_ARG, "packed_rowsums: codes, meta and rowsums must not be NULL");
  if (M <= 0 || K <= 0) return set_error(ADMMQ_ERR_ARG, "packed_rowsums: M and K must be positive");
  int off = 0;
  const int32_t rc = packed_meta_check(meta, "packed_rowsums", true, &off);
  if (rc != ADMMQ_OK) return rc;
  if (trans_w != 0 && trans_w != 1) return set_error(ADMMQ_ERR_ARG, "packed_rowsums: trans_w must be 0 or 1");
  if (K > kIgKMax) return set_error(ADMMQ_ERR_ARG, "packed_rowsums: K must be at most 65536");
  if (M > (int64_t(1) << 22)) return set_error(ADMMQ_ERR_ARG, "packed_rowsums: sizes out of range");
  if ((reinterpret_cast<uintptr_t>(codes) & 15) != 0) return set_error(ADMMQ_ERR_ARG, "packed_rowsums: codes must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(rowsums) & 3) != 0) return set_error(ADMMQ_ERR_ARG, "packed_rowsums: rowsums must be int32 aligned");
  const long long nbytes = (long long)admmq_packed_bytes(M * K, meta->bits);
  const unsigned nblk = (unsigned)(trans_w ? (M + 63) / 64 : (M + 3) / 4);
  hipLaunchKernelGGL(k_packed_rowsum, dim3(nblk), dim3(256), 0, static_cast<hipStream_t>(stream), codes, nbytes,
                     (int)meta->bits, (int)trans_w, (int)M, (int)K, off, rowsums);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

size_t admmq_packed_igemm_workspace_size(int64_t M, int64_t K, int64_t N, int32_t nb) {
  PackedPlan pl;
  return plan_ig(M, K, N, nb, pl) ? pl.ws : 0;
}

int32_t admmq_packed_igemm(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                           const uint8_t* x, const admmq_actq* x_q, const int32_t* rowsums, int32_t x_layout, int64_t N,
                           int32_t nb, const float* bias, float* y, uint8_t* y_codes, const admmq_actq* out_q,
                           int32_t* clamped, void* workspace, size_t workspace_bytes, void* stream) {
  if (!codes || !x || !meta || !rowsums || !x_q)
    return set_error(ADMMQ_ERR_ARG, "packed_igemm: codes, meta, x, x_q and rowsums must not be NULL");
  if ((y == nullptr) == (y_codes == nullptr))
    return set_error(ADMMQ_ERR_ARG, "packed_igemm: exactly one of y and y_codes must be given");
  if (M <= 0 || K <= 0 || N <= 0 || nb <= 0) return set_error(ADMMQ_ERR_ARG, "packed_igemm: M, K, N and nb must be positive");
  int off = 0;
  int32_t rc = packed_meta_check(meta, "packed_igemm", true, &off);
  if (rc != ADMMQ_OK) return rc;
  if (K > kIgKMax) return set_error(ADMMQ_ERR_ARG, "packed_igemm: K must be at most 65536 (the int32 sum 128 * 255 * K)");
  if (!act_bits_ok(x_q)) return set_error(ADMMQ_ERR_ARG, "packed_igemm: x_q must be on with bits 2..8");
  const bool oq = out_q && out_q->on != 0;
  if (y_codes && !act_bits_ok(out_q))
    return set_error(ADMMQ_ERR_ARG, "packed_igemm: a codes output needs out_q on with bits 2..8");
  if (y && oq && (out_q->bits < 1 || out_q->bits > 24)) return set_error(ADMMQ_ERR_ARG, "packed_igemm: out_q bits must be 1..24");
  if (trans_w != 0 && trans_w != 1) return set_error(ADMMQ_ERR_ARG, "packed_igemm: trans_w must be 0 or 1");
  if (x_layout != 0 && x_layout != 1) return set_error(ADMMQ_ERR_ARG, "packed_igemm: x_layout must be 0 or 1");
  if (x_layout == 1 && nb != 1) return set_error(ADMMQ_ERR_ARG, "packed_igemm: x_layout 1 (linear) needs nb = 1");
  if ((reinterpret_cast<uintptr_t>(codes) & 15) != 0) return set_error(ADMMQ_ERR_ARG, "packed_igemm: codes must be 16-byte aligned");
  if (((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(rowsums) |
        reinterpret_cast<uintptr_t>(clamped)) & 3) != 0)
    return set_error(ADMMQ_ERR_ARG, "packed_igemm: y, bias, rowsums and clamped must be 4-byte aligned");
  PackedPlan pl;
  if (!plan_ig(M, K, N, nb, pl)) return set_error(ADMMQ_ERR_ARG, "packed_igemm: sizes out of range");
  rc = packed_ws_check("packed_igemm", pl, workspace, workspace_bytes, "int32");
  if (rc != ADMMQ_OK) return rc;
  IgArgs a;
  ig_fill(a, codes, meta, off, x, x_q, rowsums, bias, y, y_codes, out_q, clamped, workspace, pl, M, K, N, x_layout);
  hipStream_t s = static_cast<hipStream_t>(stream);
  rc = counter_reset(a.clamped, s);
  if (rc != ADMMQ_OK) return rc;
  const dim3 grid((unsigned)pl.tiles_c, (unsigned)pl.tiles_m, pl.parallel ? (unsigned)pl.np : 1u);
  const int kout = pl.parallel ? kIgFloat : a.out;   // the parallel form's epilogue runs in k_packed_ireduce
#define ADMMQ_IG_LAUNCH(B, T, X)                                                                                  \
  do {                                                                                                            \
    if (kout == kIgCodes) hipLaunchKernelGGL((k_packed_igemm<B, T, X, kIgCodes>), grid, dim3(256), 0, s, a);      \
    else if (kout == kIgQuant) hipLaunchKernelGGL((k_packed_igemm<B, T, X, kIgQuant>), grid, dim3(256), 0, s, a); \
    else hipLaunchKernelGGL((k_packed_igemm<B, T, X, kIgFloat>), grid, dim3(256), 0, s, a);                       \
  } while (0)
#define ADMMQ_IG_BITS(B)                                   \
  if (trans_w && x_layout) ADMMQ_IG_LAUNCH(B, true, true); \
  else if (trans_w) ADMMQ_IG_LAUNCH(B, true, false);       \
  else if (x_layout) ADMMQ_IG_LAUNCH(B, false, true);      \
  else ADMMQ_IG_LAUNCH(B, false, false)
  PACKED_BITS_SWITCH(meta->bits, ADMMQ_IG_BITS)
#undef ADMMQ_IG_BITS
#undef ADMMQ_IG_LAUNCH
  return ig_finish(a, pl, s);
}

}  // extern "C"

// --- integer fused depthwise + 1x1 stage (include/admmq.h "Integer fused depthwise + 1x1") ---
// k_packed_igemm<BITS, false, false, OUT> with the X loader replaced by an integer stencil over
// the codes of t: for an element (k, column) of the step's block
//   D  = sum_V c[tap,k] ut[b,k,ih,iw]      Cv = sum_V c[tap,k]      (V: the taps inside the image)
//   z  = float(double(s_c) (g_t double(D) + double(mn_t) double(Cv)))     uz = act_code(z; mid_q)
// and uz - 128 is the byte of the [c][k] image. A thread owns one column and the 16 k of its
// wave (xk = 16 wave), as the layout-0 loader of k_packed_igemm: the tap weights of a step are
// one aligned 16-byte uniform load a tap from the int8 image [tap][Kp] (k_packed_taps_i8). The
// column's window position, its validity masks and its plane pointer are derived once, as in
// k_packed_dwgemm; a tap outside the image reads the plane's first byte and enters with the
// weight 0 (a select, no branch around the load); a tap's 16 byte loads are issued together,
// ahead of the selects (the empty asm). Elements that are not real (a column past C, a k past
// the piece or K) are the int8 value 0 and are neither encoded nor counted. z, its code and the
// bias by 128 are formed in the load phase: four packed dwords are all that lives across the
// step's two MFMAs. Workgroups with blockIdx.y == 0 count the clamped codes of Z: the column
// tiles and the K pieces partition Z, the row tiles repeat it.
namespace admmq {

struct IgDwArgs {
  IgArgs g;                  // x = t's codes [nb, K, H, W]; N = Ho Wo; C = nb N; g, mnx: the mid quantizer's
  const signed char* taps;   // [kh kw][Kp] int8
  int* midc;                 // clamp counter of Z, or NULL
  long long H, W, HW, Kp;
  int Wo;
  int kh, kw, sh, sw, ph, pw;
  double sc, gt, mnt;        // s_c, rng_t / n_t, mn_t
  ActQ mq;
};

__global__ __launch_bounds__(256) void k_packed_taps_i8(const unsigned char* __restrict__ codes, long long nbytes, int bits,
                                                        int ntaps, int K, int Kp, int off, signed char* __restrict__ image) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;   // ntaps Kp <= 49 * 65536
  if (e >= ntaps * Kp) return;
  const int tap = e / Kp, k = e - tap * Kp;
  image[e] = k < K ? (signed char)((int)code_at(codes, (long long)tap * K + k, bits, nbytes) - off) : (signed char)0;
}

template <int BITS, int OUT>
__global__ __launch_bounds__(256) void k_packed_idwgemm(const IgDwArgs d) {
  __shared__ __attribute__((aligned(16))) unsigned char sW[2][kPackedBM * kIgLD];
  __shared__ __attribute__((aligned(16))) unsigned char sX[2][kPackedBN * kIgLD];
  const IgArgs& a = d.g;
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

  // W: as k_packed_igemm with TRANS = 0
  int wrow[2], wk[2], nvm[2], wsh[2];
  long long wq[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int id = tid + 256 * u;
    wrow[u] = id >> 3;
    wk[u] = 8 * (id & 7);
    nvm[u] = m0 + wrow[u] < M ? 8 : 0;
    const long long bit0 = ((long long)(m0 + wrow[u]) * K + (kb + wk[u])) * BITS;
    wsh[u] = (int)(bit0 & 31);
    wq[u] = bit0 >> 5;
  }
  const long long wstep = 2 * BITS;
  // Z: one column, k = xk .. xk + 15 (uniform over the wave)
  const int xc = tid & 63;
  const int xk = __builtin_amdgcn_readfirstlane(16 * (tid >> 6));
  const bool cok = c0 + xc < C;
  const int kh = d.kh, kw = d.kw;
  const long long W = d.W, HW = d.HW;
  long long tbase;                   // byte offset of the window's first position in a channel plane (may be negative)
  unsigned rmask = 0u, cmask = 0u;   // bit a / b: window row a / column b lies inside the image
  const unsigned char* __restrict__ tp;
  {
    const long long c = min(c0 + xc, C - 1);   // (a column past C reads a valid one and is zeroed)
    const long long b = c / N;
    const int n = (int)(c - b * N);
    const int oh = n / d.Wo, ow = n - oh * d.Wo;
    const long long ih0 = (long long)oh * d.sh - d.ph, iw0 = (long long)ow * d.sw - d.pw;
    for (int ta = 0; ta < kh; ++ta)
      if (ih0 + ta >= 0 && ih0 + ta < d.H) rmask |= 1u << ta;
    for (int tb = 0; tb < kw; ++tb)
      if (iw0 + tb >= 0 && iw0 + tb < W) cmask |= 1u << tb;
    tbase = ih0 * W + iw0;
    tp = a.x + (b * K + (kb + xk)) * HW;
  }
  const signed char* __restrict__ wp = d.taps + (kb + xk);
  const long long tstep = (long long)kIgBK * HW;
  const bool counting = d.midc != nullptr && blockIdx.y == 0;   // (uniform)

  unsigned cw[2][3];
  int nv[2] = {0, 0};
  unsigned rx[4];
  int mcnt = 0;
  auto load = [&](int k0, auto full) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full)::value;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      cw[u][0] = 0u; cw[u][1] = 0u; cw[u][2] = 0u;
      if (FULL) nv[u] = nvm[u];
      else nv[u] = nvm[u] > 0 ? min(8, ke - (k0 + wk[u])) : 0;
      if (nv[u] > 0) {
        if (4 * wq[u] + 12 <= nbytes) {
          const unsigned* q = reinterpret_cast<const unsigned*>(codes + 4 * wq[u]);
          cw[u][0] = q[0]; cw[u][1] = q[1]; cw[u][2] = q[2];
        } else {
          cw[u][0] = code_dword(codes, wq[u], nbytes);
          cw[u][1] = code_dword(codes, wq[u] + 1, nbytes);
          cw[u][2] = code_dword(codes, wq[u] + 2, nbytes);
        }
      }
      wq[u] += wstep;
    }
    const int nk = FULL ? 16 : max(0, min(16, ke - (k0 + xk)));   // the thread's real k of this step (uniform)
    rx[0] = 0u; rx[1] = 0u; rx[2] = 0u; rx[3] = 0u;
    if (nk > 0) {
      long long jo[16];   // plane offsets of the 16 k; a k past the end reads the last real one and is dropped
#pragma unroll
      for (int j = 0; j < 16; ++j) jo[j] = (long long)(FULL ? j : min(j, nk - 1)) * HW;
      int D[16], Cv[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) { D[j] = 0; Cv[j] = 0; }
      const int ntap = kh * kw;
      int ta = 0, tb = 0;
      for (int tap = 0; tap < ntap; ++tap) {
        const bool ok = ((rmask >> ta) & (cmask >> tb) & 1u) != 0u;
        const unsigned char* __restrict__ p = tp + (ok ? tbase + ta * W + tb : 0);   // outside: the plane's first byte, not used
        const ig_i32x4 wv = *reinterpret_cast<const ig_i32x4*>(wp + (long long)tap * d.Kp);   // 16 int8 weights, uniform
        unsigned v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = p[jo[j]];
        // one statement over all 16: the loads are issued together and ahead of the selects (with
        // one statement an element the prologue's copy of this loop waited for every load by itself)
        asm("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]),
                 "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15]));
        const int okm = ok ? -1 : 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int c = (wv[j >> 2] << (24 - 8 * (j & 3))) >> 24;   // (uniform: scalar)
          const int cm = c & okm;
          D[j] += __mul24(cm, (int)v[j]);   // 8-bit operands: the full-rate 24-bit multiply-add
          Cv[j] += cm;
        }
        if (++tb == kw) { tb = 0; ++ta; }
      }
#pragma unroll
      for (int dd = 0; dd < 4; ++dd) {
        unsigned w = 0u;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int j = 4 * dd + jj;
          const double zd = d.sc * (d.gt * (double)D[j] + d.mnt * (double)Cv[j]);
          int cl = 0;
          const unsigned u = act_code((float)zd, d.mq, cl);
          const bool real = cok && j < nk;
          mcnt += real ? cl : 0;
          w |= (real ? (u ^ 0x80u) : 0u) << (8 * jj);
        }
        rx[dd] = w;
      }
    }
    tp += tstep;
    wp += kIgBK;
  };
  auto store = [&](int buf) __attribute__((always_inline)) {
    constexpr unsigned mask = (1u << BITS) - 1u;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p2 = wsh[u] + 4 * BITS;
      const bool up = p2 >= 32;
      unsigned long long win[2];
      win[0] = (((unsigned long long)cw[u][1] << 32) | cw[u][0]) >> wsh[u];
      win[1] = (((unsigned long long)(up ? cw[u][2] : cw[u][1]) << 32) | (up ? cw[u][1] : cw[u][0])) >> (p2 & 31);
      unsigned b[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = (int)((unsigned)(win[j >> 2] >> ((j & 3) * BITS)) & mask) - a.off;
        b[j] = j < nv[u] ? ((unsigned)v & 255u) : 0u;
      }
      const unsigned lo = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
      const unsigned hi = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
      *reinterpret_cast<uint2*>(&sW[buf][wrow[u] * kIgLD + wk[u]]) = make_uint2(lo, hi);
    }
    *reinterpret_cast<uint4*>(&sX[buf][xc * kIgLD + xk]) = make_uint4(rx[0], rx[1], rx[2], rx[3]);
  };
  auto load_step = [&](int k0) __attribute__((always_inline)) {
    if (k0 + kIgBK <= ke) load(k0, std::true_type{});
    else load(k0, std::false_type{});
  };

  ig_i32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0;
  load_step(kb);
  store(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = kb; k0 < ke; k0 += kIgBK) {
    const bool more = k0 + kIgBK < ke;
    if (more) load_step(k0 + kIgBK);
    const unsigned char* w = sW[buf] + (32 * wm + i) * kIgLD + 16 * h;
    const unsigned char* x = sX[buf] + (32 * wn + i) * kIgLD + 16 * h;
#pragma unroll
    for (int kk = 0; kk < kIgBK / 32; ++kk) {
      const ig_i32x4 av = *reinterpret_cast<const ig_i32x4*>(w + 32 * kk);
      const ig_i32x4 bv = *reinterpret_cast<const ig_i32x4*>(x + 32 * kk);
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc, 0, 0, 0);
    }
    if (more) store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // Epilogue: k_packed_igemm's for x_layout 0
  int cnt = 0;
  {
    const long long c = c0 + 32 * wn + i;
    const bool ok = c < C;
    const long long cc = ok ? c : 0;
    const long long b = cc / N;
    const long long ybase = b * M * N + (cc - b * N);
    const bool hb = a.bias != nullptr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + 32 * wm + PACKED_ROW(r);
      if (!ok || m >= M) continue;
      const long long e = ybase + (long long)m * N;
      if (a.parallel) {
        a.part[(long long)piece * a.total + e] = acc[r];
      } else {
        const float v = ig_value(acc[r], a.rowsum[m], a, hb, hb ? a.bias[m] : 0.f);
        if constexpr (OUT == kIgCodes) a.yc[e] = (unsigned char)act_code(v, a.oq, cnt);
        else if constexpr (OUT == kIgQuant) a.y[e] = fixed_quant(v, a.oq);
        else a.y[e] = v;
      }
    }
  }
  if (counting) block_count_add(mcnt, d.midc);   // (uniform; every thread arrives: no return above)
  if constexpr (OUT == kIgCodes) {
    if (a.clamped) {
      __syncthreads();   // block_count_add's LDS words are those of the call above
      block_count_add(cnt, a.clamped);
    }
  }
}

static int64_t taps_kp(int64_t K) { return kIgBK * ((K + kIgBK - 1) / kIgBK); }

}  // namespace admmq

extern "C" {

size_t admmq_packed_taps_i8_bytes(int32_t ntaps, int64_t K) {
  if (ntaps <= 0 || ntaps > 49 || K <= 0 || K > kIgKMax) return 0;
  return (size_t)ntaps * (size_t)taps_kp(K);
}

int32_t admmq_packed_taps_i8(const uint8_t* codes, const admmq_qmeta* meta, int32_t ntaps, int64_t K, int8_t* image,
                             void* stream) {
  if (!codes || !meta || !image) return set_error(ADMMQ_ERR_ARG, "packed_taps_i8: codes, meta and image must not be NULL");
  if (ntaps <= 0 || K <= 0) return set_error(ADMMQ_ERR_ARG, "packed_taps_i8: ntaps and K must be positive");
  if (ntaps > 49) return set_error(ADMMQ_ERR_ARG, "packed_taps_i8: ntaps must be at most 49 (a 7 x 7 window)");
  int off = 0;
  const int32_t rc = packed_meta_check(meta, "packed_taps_i8", true, &off);
  if (rc != ADMMQ_OK) return rc;
  if (K > kIgKMax) return set_error(ADMMQ_ERR_ARG, "packed_taps_i8: K must be at most 65536");
  if ((reinterpret_cast<uintptr_t>(codes) & 15) != 0) return set_error(ADMMQ_ERR_ARG, "packed_taps_i8: codes must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(image) & 15) != 0) return set_error(ADMMQ_ERR_ARG, "packed_taps_i8: image must be 16-byte aligned");
  const int Kp = (int)taps_kp(K);
  const long long nbytes = (long long)admmq_packed_bytes((int64_t)ntaps * K, meta->bits);
  const unsigned nblk = (unsigned)(((long long)ntaps * Kp + 255) / 256);
  hipLaunchKernelGGL(k_packed_taps_i8, dim3(nblk), dim3(256), 0, static_cast<hipStream_t>(stream), codes, nbytes,
                     (int)meta->bits, (int)ntaps, (int)K, Kp, off, reinterpret_cast<signed char*>(image));
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

size_t admmq_packed_idwgemm_workspace_size(int64_t M, int64_t K, int64_t Ho, int64_t Wo, int32_t nb) {
  PackedPlan pl;
  return plan_ig_dw(M, K, Ho, Wo, nb, pl) ? pl.ws : 0;
}

int32_t admmq_packed_idwgemm(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const uint8_t* t_codes,
                             const admmq_actq* t_q, int32_t nb, int64_t H, int64_t W, const int8_t* taps_i8, float s_c,
                             int32_t kh, int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw,
                             const int32_t* rowsums, const float* bias, float* y, uint8_t* y_codes,
                             const admmq_actq* mid_q, const admmq_actq* out_q, int32_t* mid_clamped, int32_t* clamped,
                             void* workspace, size_t workspace_bytes, void* stream) {
  const char* const who = "packed_idwgemm";
  if (!codes || !meta || !t_codes || !t_q || !taps_i8 || !rowsums)
    return set_error(ADMMQ_ERR_ARG, "packed_idwgemm: codes, meta, t_codes, t_q, taps_i8 and rowsums must not be NULL");
  if ((y == nullptr) == (y_codes == nullptr))
    return set_error(ADMMQ_ERR_ARG, "packed_idwgemm: exactly one of y and y_codes must be given");
  if (M <= 0 || K <= 0 || H <= 0 || W <= 0 || nb <= 0)
    return set_error(ADMMQ_ERR_ARG, "packed_idwgemm: M, K, H, W and nb must be positive");
  int off = 0;
  int32_t rc = packed_meta_check(meta, who, true, &off);
  if (rc != ADMMQ_OK) return rc;
  if (K > kIgKMax) return set_error(ADMMQ_ERR_ARG, "packed_idwgemm: K must be at most 65536 (the int32 sum 128 * 255 * K)");
  if (!act_bits_ok(t_q)) return set_error(ADMMQ_ERR_ARG, "packed_idwgemm: t_q must be on with bits 2..8");
  if (!act_bits_ok(mid_q))
    return set_error(ADMMQ_ERR_ARG, "packed_idwgemm: mid_q must be given and on with bits 2..8 (the GEMM operand is codes)");
  const bool oq = out_q && out_q->on != 0;
  if (y_codes && !act_bits_ok(out_q))
    return set_error(ADMMQ_ERR_ARG, "packed_idwgemm: a codes output needs out_q on with bits 2..8");
  if (y && oq && (out_q->bits < 1 || out_q->bits > 24)) return set_error(ADMMQ_ERR_ARG, "packed_idwgemm: out_q bits must be 1..24");
  int64_t Ho = 0, Wo = 0;
  rc = packed_dw_geometry_check(who, H, W, kh, kw, sh, sw, ph, pw, &Ho, &Wo);
  if (rc != ADMMQ_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(codes) & 15) != 0) return set_error(ADMMQ_ERR_ARG, "packed_idwgemm: codes must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(taps_i8) & 15) != 0)
    return set_error(ADMMQ_ERR_ARG, "packed_idwgemm: taps_i8 must be 16-byte aligned");
  if (((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(rowsums) |
        reinterpret_cast<uintptr_t>(clamped) | reinterpret_cast<uintptr_t>(mid_clamped)) & 3) != 0)
    return set_error(ADMMQ_ERR_ARG, "packed_idwgemm: y, bias, rowsums, mid_clamped and clamped must be 4-byte aligned");
  PackedPlan pl;
  if (!plan_ig_dw(M, K, Ho, Wo, nb, pl)) return set_error(ADMMQ_ERR_ARG, "packed_idwgemm: sizes out of range");
  rc = packed_dw_extent_check(who, nb, K, H, W);
  if (rc != ADMMQ_OK) return rc;
  rc = packed_ws_check(who, pl, workspace, workspace_bytes, "int32");
  if (rc != ADMMQ_OK) return rc;
  IgDwArgs d;
  IgArgs& a = d.g;   // (the GEMM's activation operand is Z: the mid quantizer's codes)
  ig_fill(a, codes, meta, off, t_codes, mid_q, rowsums, bias, y, y_codes, out_q, clamped, workspace, pl, M, K, Ho * Wo, 0);
  d.taps = reinterpret_cast<const signed char*>(taps_i8);
  d.midc = mid_clamped;
  d.H = H; d.W = W; d.HW = H * W; d.Kp = taps_kp(K);
  d.Wo = (int)Wo;
  d.kh = kh; d.kw = kw; d.sh = sh; d.sw = sw; d.ph = ph; d.pw = pw;
  d.sc = (double)s_c;
  d.gt = (double)t_q->rng / (double)((1 << t_q->bits) - 1);
  d.mnt = (double)t_q->mn;
  d.mq = actq_make(mid_q);
  hipStream_t s = static_cast<hipStream_t>(stream);
  rc = counter_reset(mid_clamped, s);
  if (rc != ADMMQ_OK) return rc;
  rc = counter_reset(a.clamped, s);
  if (rc != ADMMQ_OK) return rc;
  const dim3 grid((unsigned)pl.tiles_c, (unsigned)pl.tiles_m, pl.parallel ? (unsigned)pl.np : 1u);
  const int kout = pl.parallel ? kIgFloat : a.out;   // the parallel form's epilogue runs in k_packed_ireduce
#define ADMMQ_IDW_BITS(B)                                                                                   \
  if (kout == kIgCodes) hipLaunchKernelGGL((k_packed_idwgemm<B, kIgCodes>), grid, dim3(256), 0, s, d);      \
  else if (kout == kIgQuant) hipLaunchKernelGGL((k_packed_idwgemm<B, kIgQuant>), grid, dim3(256), 0, s, d); \
  else hipLaunchKernelGGL((k_packed_idwgemm<B, kIgFloat>), grid, dim3(256), 0, s, d)
  PACKED_BITS_SWITCH(meta->bits, ADMMQ_IDW_BITS)
#undef ADMMQ_IDW_BITS
  return ig_finish(a, pl, s);
}

}  // extern "C"
