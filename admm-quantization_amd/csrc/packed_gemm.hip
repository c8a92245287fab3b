// GEMM on a weight kept as packed integer codes (include/admmq.h "Packed-weight GEMM",
// DESIGN.md 2.22): Y = W X (+ bias) with W = D or D^T, D the table de-quantization of a
// packed tensor's codes (dequant_code, quant_device.h), decoded tile by tile into LDS and
// multiplied on the fp32 MFMA - the float32 weight never exists in memory.
//
// The batch and the positions form one column axis c in [0, C), C = nb N:
//   x_layout 0 (NCHW 1x1 conv): c = b N + n, X[(b K + k) N + n], Y[(b M + m) N + n]
//   x_layout 1 (linear, nb = 1): c = token,  X[c K + k],         Y[c M + m]
// A workgroup (256 threads, 4 waves of 32 x 32) owns a 64 (m) x 64 (c) tile and steps
// through K in 32s: the W block of a step is decoded from the bit stream (a thread takes a
// run of 8 consecutive codes of the stream: along k for trans_w = 0, along m for 1; a run
// starts at any bit, so it is cut out of three dwords) into a k-major LDS image, the X
// block is copied beside it, and each wave issues 16 v_mfma_f32_32x32x2_f32. x_layout 1
// swaps the MFMA operands so that the lanes of the result run along m, Y's contiguous axis.
//
// K is cut into pieces of kp = max(64, 32 ceil(K / 1024)) (a function of K alone; at most
// 32 pieces). Every piece is summed in its own accumulator chain from zero, and an output is
// ((p0 + p1) + p2) + ... (+ bias) in piece order. Two forms give those same bits: serial (one
// workgroup runs all pieces of its tile and folds the accumulator at each piece end) and
// parallel (one workgroup per piece writes its partial image to the workspace, and
// k_packed_reduce adds the images in piece order). The planner takes the parallel form when
// the serial one would start fewer than kPackedParallelBelow workgroups (the weight-streaming
// regime: few columns, the work is reading the code stream). No workgroup waits for
// another, and nothing is combined with atomics.
//
// The host pieces that the integer path (packed_igemm.hip) uses too - the planner and the
// argument checks - are defined here and declared in admmq_internal.h.
#include <algorithm>
#include <type_traits>

#include "../../include/admmq.h"
#include "packed_tile.h"

namespace admmq {

constexpr int kPgBK = 32;               // the K step
constexpr int kPgLD = 65;               // LDS row stride: the k-major fragment reads and both store patterns spread over the banks
constexpr int64_t kPgKMax = int64_t(1) << 24;

typedef float pg_f32x16 __attribute__((ext_vector_type(16)));

struct PgArgs {
  const unsigned char* codes;
  const float* x;
  const float* bias;
  float* y;
  float* part;        // parallel form: [np][total] partial images in Y's layout
  long long nbytes;   // bytes of the code stream
  long long total;    // C * M
  long long C;
  int M, K, N;
  int xl;
  int kp, np, parallel;
  int scheme, zp;
  float scale, mn, rng;
};

// Output quantizer: the quantized instantiations take the same record with the
// quantizer behind it, so the plain ones keep their arguments and their code.
struct PgArgsQ : PgArgs {
  ActQ oq;
};

// The per-step addresses are hoisted: a run's bit offset in its first dword is the same in
// every step (a step advances the stream by 32 (x M) BITS bits: whole dwords), so the thread
// keeps one dword index and adds a constant; X is read through one pointer plus 8 fixed
// offsets. FULL steps (all 32 k inside the piece) load without k tests; columns past C read
// a clamped (valid) address and are zeroed by a select, not a branch.
// OQ: the serial form's epilogue stores fixed_quant(tot (+ bias)) (the parallel form quantizes
// in k_packed_reduce<true> and runs the plain kernel).
template <int BITS, bool TRANS, bool XL, bool OQ = false>
__global__ __launch_bounds__(256) void k_packed_gemm(const std::conditional_t<OQ, PgArgsQ, PgArgs> a) {
  __shared__ float sW[2][kPgBK * kPgLD];
  __shared__ float sX[2][kPgBK * kPgLD];
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

  // W: this thread's run of 8 stream-consecutive codes of a step's 64 x 32 block
  // (neighbouring lanes take neighbouring runs of the stream: 8 runs of a k row, 4 runs of an m row)
  const int wrow = TRANS ? 8 * (tid & 7) : (tid >> 2);   // m - m0 of the run's first code
  const int wk = TRANS ? (tid >> 3) : 8 * (tid & 3);     // k - k0 of the run's first code
  const int nvm = TRANS ? min(8, M - (m0 + wrow)) : (m0 + wrow < M ? 8 : 0);   // codes of a full step's run inside W (<= 0: none)
  const long long bit0 = (TRANS ? (long long)(kb + wk) * M + (m0 + wrow) : (long long)(m0 + wrow) * K + (kb + wk)) * BITS;
  const int wsh = (int)(bit0 & 31);    // the run's 8 BITS <= 64 bits start at bit wsh of dword wq: three dwords
  long long wq = bit0 >> 5;
  const long long wstep = TRANS ? (long long)M * BITS : BITS;   // dwords per K-step
  // X: 8 elements of the step's 32 x 64 block; layout 0: one column, k = xk + 4 j;
  // layout 1: one k, columns xc + 8 j
  const int xc = XL ? (tid >> 5) : (tid & 63);
  const int xk = XL ? (tid & 31) : (tid >> 6);
  long long xo[8];      // element offsets of the 8 loads from xp
  unsigned xok = 0u;    // bit j: load j's column is inside C
  const float* __restrict__ xp;
  if (XL) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long c = c0 + xc + 8 * j;
      if (c < C) xok |= 1u << j;
      xo[j] = min(c, C - 1) * K;
    }
    xp = a.x + (kb + xk);
  } else {
    const long long c = min(c0 + xc, C - 1);
    if (c0 + xc < C) xok = 0xFFu;
    const long long b = c / N;
#pragma unroll
    for (int j = 0; j < 8; ++j) xo[j] = (long long)(4 * j) * N;
    xp = a.x + (b * K * N + (c - b * N)) + (long long)(kb + xk) * N;
  }
  const long long xstep = XL ? kPgBK : (long long)kPgBK * N;

  unsigned cw[3];
  int nv = 0;
  float rx[8];
  // the loads of the next step in stream order (each call advances wq and xp by one step)
  auto load = [&](int k0, auto full) {
    constexpr bool FULL = decltype(full)::value;
    cw[0] = 0u; cw[1] = 0u; cw[2] = 0u;
    if (FULL) nv = nvm;
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
    const gcf32* xg = (const gcf32*)xp;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (FULL) {
        const float v = xg[xo[j]];
        rx[j] = ((xok >> j) & 1u) ? v : 0.f;
      } else {
        const int k = XL ? k0 + xk : k0 + xk + 4 * j;
        rx[j] = (((xok >> j) & 1u) && k < ke) ? xg[xo[j]] : 0.f;
      }
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
    float d[8];
    if (a.scheme == kMinMax) {   // (one uniform branch per step, not one per code)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        d[j] = dequant_code((unsigned)(win[j >> 2] >> ((j & 3) * BITS)) & mask, kMinMax, BITS, a.scale, a.zp, a.mn, a.rng);
    } else {                     // mse-minmax / symmetric: the affine form with zero_point 0 (an exact integer)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        d[j] = dequant_code((unsigned)(win[j >> 2] >> ((j & 3) * BITS)) & mask, kAffine, BITS, a.scale, a.zp, a.mn, a.rng);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = j < nv ? d[j] : 0.f;   // past the run's row / the piece / the matrix: exactly 0
      if (TRANS) sW[buf][wk * kPgLD + wrow + j] = v;
      else sW[buf][(wk + j) * kPgLD + wrow] = v;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (XL) sX[buf][xk * kPgLD + xc + 8 * j] = rx[j];
      else sX[buf][(xk + 4 * j) * kPgLD + xc] = rx[j];
    }
  };
  auto load_step = [&](int k0) {
    if (k0 + kPgBK <= ke) load(k0, std::true_type{});
    else load(k0, std::false_type{});
  };

  pg_f32x16 acc, tot;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[r] = 0.f; tot[r] = 0.f; }
  bool first = true;
  int pend = kb + a.kp;   // the current piece's end
  load_step(kb);
  store(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = kb; k0 < ke; k0 += kPgBK) {
    const bool more = k0 + kPgBK < ke;
    if (more) load_step(k0 + kPgBK);
    const float* w = sW[buf] + 32 * wm + i;
    const float* x = sX[buf] + 32 * wn + i;
#pragma unroll
    for (int q = 0; q < kPgBK / 2; ++q) {
      if (XL) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[(2 * q + h) * kPgLD], w[(2 * q + h) * kPgLD], acc, 0, 0, 0);
      else acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[(2 * q + h) * kPgLD], x[(2 * q + h) * kPgLD], acc, 0, 0, 0);
    }
    if (!more || k0 + kPgBK == pend) {   // a piece ends: fold it into the running sum
      pend += a.kp;
      if (first) {
        tot = acc;
        first = false;
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[r] = tot[r] + acc[r];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
    if (more) store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  float* const dst = a.parallel ? a.part + (long long)piece * a.total : a.y;
  const float* __restrict__ bias = a.parallel ? nullptr : a.bias;
  if (XL) {   // lanes along m, rows along the columns: Y[c M + m]
    const int m = m0 + 32 * wm + i;
    if (m >= M) return;
    const float bv = bias ? bias[m] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long c = c0 + 32 * wn + PACKED_ROW(r);
      if constexpr (OQ) {
        if (c < C) dst[c * M + m] = fixed_quant(bias ? tot[r] + bv : tot[r], a.oq);
      } else {
        if (c < C) dst[c * M + m] = bias ? tot[r] + bv : tot[r];
      }
    }
  } else {    // lanes along the columns: Y[(b M + m) N + n]
    const long long c = c0 + 32 * wn + i;
    if (c >= C) return;
    const long long b = c / N;
    const long long ybase = b * M * N + (c - b * N);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + 32 * wm + PACKED_ROW(r);
      if constexpr (OQ) {
        if (m < M) dst[ybase + (long long)m * N] = fixed_quant(bias ? tot[r] + bias[m] : tot[r], a.oq);
      } else {
        if (m < M) dst[ybase + (long long)m * N] = bias ? tot[r] + bias[m] : tot[r];
      }
    }
  }
}

// Y[e] = ((part_0[e] + part_1[e]) + ...) + bias[m(e)]: the piece order of the serial form
// OQ: the output quantizer behind the bias (the plain form does not read oq)
template <bool OQ>
__global__ __launch_bounds__(256) void k_packed_reduce(const float* __restrict__ part, int np, long long total,
                                                       const float* __restrict__ bias, float* __restrict__ y, int M,
                                                       int N, int xl, const ActQ oq) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  float s = part[e];
  for (int p = 1; p < np; ++p) s = s + part[(long long)p * total + e];
  if (bias) s = s + bias[xl ? e % M : (e / N) % M];
  y[e] = OQ ? fixed_quant(s, oq) : s;
}

// Fused depthwise kh x kw + 1x1 stage of a packed CP layer (include/admmq.h "Fused depthwise
// + 1x1"): k_packed_gemm<BITS, false, false> with the X loader replaced by a
// stencil. The activation operand Z[k, (b, oh, ow)] = sum_tap taps[tap][k] t[b, k, ih, iw] is
// formed while the X tile is staged and never exists in memory; the W decode, the K pieces,
// the fold, the two regimes and the epilogue are those of k_packed_gemm (a kernel of its own,
// so that the existing instantiations' code does not change).
struct PgDwArgs {
  PgArgs g;            // x = t [nb, K, H, W]; N = Ho Wo; C = nb N
  const float* taps;   // [kh kw][K]
  long long H, W, HW;
  int Wo;
  int kh, kw, sh, sw, ph, pw;
};

// Quantized forms, as PgArgsQ: the plain record first, the quantizers behind it
struct PgDwArgsQ : PgDwArgs {
  ActQ mq, oq;
};

// A thread's column (b, oh, ow) is fixed over the K steps: its first input position, the
// rows / columns of the window that lie inside the image (two bit masks) and the channel
// plane it starts in are derived once; a step then advances one pointer by 32 H W. A thread's
// k within a step is xk + 4 j with xk uniform over the wave, so the tap weights are uniform
// reads. The tap sum of an element is z = z + w v in tap order from +0.0, product and sum
// rounded separately; a tap outside the image is skipped (a select), a k past the piece's or
// K's end reads nothing and yields exactly 0, a column past C reads the clamped column and is
// zeroed. The sums are formed in the load phase, two taps (16 loads) at a time (kh kw 8 raw
// values do not fit the register file for the larger windows): the next step's stencil is
// issued and summed before the current step's 16 MFMAs, the decode and the LDS stores come
// after them.
// QM bit 0: the mid quantizer - an element of Z becomes fixed_quant(z) as it is staged. Only
// real elements: a column past C, a k past the piece's or K's end (and with it the zero fill of
// a partial step) stay exactly 0 - q(0) is not 0 unless 0 lies on the grid, and a quantized
// padding element would enter every output of the tile. QM bit 1: the output quantizer in the
// serial form's epilogue, as k_packed_gemm's OQ.
// PG_DW_CALL: the quantized forms' larger load / store bodies would otherwise stay calls with
// their captures in scratch; the plain form's calls are written as they were.
#define PG_DW_CALL(call)             \
  do {                               \
    if constexpr (QM != 0) {         \
      [[clang::always_inline]] call; \
    } else {                         \
      call;                          \
    }                                \
  } while (0)
template <int BITS, int QM = 0>
__global__ __launch_bounds__(256) void k_packed_dwgemm(const std::conditional_t<QM != 0, PgDwArgsQ, PgDwArgs> d) {
  __shared__ float sW[2][kPgBK * kPgLD];
  __shared__ float sX[2][kPgBK * kPgLD];
  const PgArgs& a = d.g;
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

  // W: as k_packed_gemm with trans_w = 0
  const int wrow = tid >> 2;
  const int wk = 8 * (tid & 3);
  const int nvm = m0 + wrow < M ? 8 : 0;
  const long long bit0 = ((long long)(m0 + wrow) * K + (kb + wk)) * BITS;
  const int wsh = (int)(bit0 & 31);
  long long wq = bit0 >> 5;
  // Z: one column, k = xk + 4 j
  const int xc = tid & 63;
  const int xk = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool cok = c0 + xc < C;
  const int kh = d.kh, kw = d.kw;
  const long long W = d.W, HW = d.HW;
  long long tbase;            // element offset of the window's first position in a channel plane (may be negative)
  unsigned rmask = 0u, cmask = 0u;   // bit a / b: window row a / column b lies inside the image
  const float* __restrict__ tp;
  {
    const long long c = min(c0 + xc, C - 1);
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
  const float* __restrict__ wp = d.taps + (kb + xk);
  const long long tstep = (long long)kPgBK * HW;

  unsigned cw[3];
  int nv = 0;
  float rx[8];
  [[maybe_unused]] unsigned zreal = 0u;   // (mid quantizer) bit j: rx[j] is an element of Z, not padding
  auto load = [&](int k0, auto full) {
    constexpr bool FULL = decltype(full)::value;
    cw[0] = 0u; cw[1] = 0u; cw[2] = 0u;
    if (FULL) nv = nvm;
    else nv = nvm > 0 ? min(8, ke - (k0 + wk)) : 0;
    if (nv > 0) {
      if (4 * wq + 12 <= nbytes) {
        const gcu32* q = (const gcu32*)(codes + 4 * wq);
        cw[0] = q[0]; cw[1] = q[1]; cw[2] = q[2];
      } else {
        cw[0] = code_dword(codes, wq, nbytes);
        cw[1] = code_dword(codes, wq + 1, nbytes);
        cw[2] = code_dword(codes, wq + 2, nbytes);
      }
    }
    wq += BITS;
    const gcf32* tg = (const gcf32*)tp;
    const gcf32* wg = (const gcf32*)wp;
    float z[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = 0.f;
    // two taps at a time: their 16 loads are issued together, then taken whatever the masks
    // say (the empty asm: the loads stay together and ahead of the selects, instead of one load
    // and one wait inside a branch per element), then summed in tap order; an odd count's last
    // pair repeats the last tap with its second half switched off
    const int ntap = kh * kw;
    int ta = 0, tb = 0;
    for (int tap = 0; tap < ntap; tap += 2) {
      const bool two = tap + 1 < ntap;
      int ta1 = ta, tb1 = tb;
      if (two && ++tb1 == kw) { tb1 = 0; ++ta1; }
      const bool ok0 = ((rmask >> ta) & (cmask >> tb) & 1u) != 0u;
      const bool ok1 = two && ((rmask >> ta1) & (cmask >> tb1) & 1u) != 0u;
      const long long off0 = ok0 ? tbase + ta * W + tb : 0;   // outside: the plane's first element, not used
      const long long off1 = ok1 ? tbase + ta1 * W + tb1 : 0;
      const gcf32* wt0 = wg + (long long)tap * K;
      const gcf32* wt1 = wg + (long long)(two ? tap + 1 : tap) * K;
      float w0[8], w1[8], v0[8], v1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (FULL) {
          w0[j] = wt0[4 * j];
          w1[j] = wt1[4 * j];
          v0[j] = tg[off0 + (long long)(4 * j) * HW];
          v1[j] = tg[off1 + (long long)(4 * j) * HW];
        } else {
          const bool in = k0 + xk + 4 * j < ke;   // (uniform over the wave)
          w0[j] = in ? wt0[4 * j] : 0.f;
          w1[j] = in ? wt1[4 * j] : 0.f;
          v0[j] = in ? tg[off0 + (long long)(4 * j) * HW] : 0.f;
          v1[j] = in ? tg[off1 + (long long)(4 * j) * HW] : 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) asm("" : "+v"(v0[j]), "+v"(v1[j]));
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float s = z[j] + w0[j] * v0[j];
        z[j] = ok0 ? s : z[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float s = z[j] + w1[j] * v1[j];
        z[j] = ok1 ? s : z[j];
      }
      ta = ta1; tb = tb1;
      if (++tb == kw) { tb = 0; ++ta; }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) rx[j] = cok ? z[j] : 0.f;
    if constexpr ((QM & 1) != 0) {   // the step's real elements, for store()
      const int nk = FULL ? 8 : (ke - (k0 + xk) + 3) >> 2;   // js with k0 + xk + 4 j < ke
      zreal = cok ? (nk >= 8 ? 0xFFu : (nk > 0 ? (1u << nk) - 1u : 0u)) : 0u;
    }
    tp += tstep;
    wp += kPgBK;
  };
  auto store = [&](int buf) {
    constexpr unsigned mask = (1u << BITS) - 1u;
    const int p2 = wsh + 4 * BITS;
    const bool up = p2 >= 32;
    unsigned long long win[2];
    win[0] = (((unsigned long long)cw[1] << 32) | cw[0]) >> wsh;
    win[1] = (((unsigned long long)(up ? cw[2] : cw[1]) << 32) | (up ? cw[1] : cw[0])) >> (p2 & 31);
    float dq[8];
    if (a.scheme == kMinMax) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        dq[j] = dequant_code((unsigned)(win[j >> 2] >> ((j & 3) * BITS)) & mask, kMinMax, BITS, a.scale, a.zp, a.mn, a.rng);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        dq[j] = dequant_code((unsigned)(win[j >> 2] >> ((j & 3) * BITS)) & mask, kAffine, BITS, a.scale, a.zp, a.mn, a.rng);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) sW[buf][(wk + j) * kPgLD + wrow] = j < nv ? dq[j] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if constexpr ((QM & 1) != 0) {   // quantized here, after the step's MFMAs: the load phase keeps its registers
        const float zq = fixed_quant(rx[j], d.mq);
        sX[buf][(xk + 4 * j) * kPgLD + xc] = ((zreal >> j) & 1u) ? zq : 0.f;
      } else {
        sX[buf][(xk + 4 * j) * kPgLD + xc] = rx[j];
      }
    }
  };
  auto load_step = [&](int k0) {
    if (k0 + kPgBK <= ke) PG_DW_CALL(load(k0, std::true_type{}));
    else PG_DW_CALL(load(k0, std::false_type{}));
  };

  pg_f32x16 acc, tot;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[r] = 0.f; tot[r] = 0.f; }
  bool first = true;
  int pend = kb + a.kp;
  PG_DW_CALL(load_step(kb));
  PG_DW_CALL(store(0));
  __syncthreads();
  int buf = 0;
  for (int k0 = kb; k0 < ke; k0 += kPgBK) {
    const bool more = k0 + kPgBK < ke;
    if (more) PG_DW_CALL(load_step(k0 + kPgBK));
    const float* w = sW[buf] + 32 * wm + i;
    const float* x = sX[buf] + 32 * wn + i;
#pragma unroll
    for (int q = 0; q < kPgBK / 2; ++q)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[(2 * q + h) * kPgLD], x[(2 * q + h) * kPgLD], acc, 0, 0, 0);
    if (!more || k0 + kPgBK == pend) {
      pend += a.kp;
      if (first) {
        tot = acc;
        first = false;
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[r] = tot[r] + acc[r];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
    if (more) PG_DW_CALL(store(buf ^ 1));
    __syncthreads();
    buf ^= 1;
  }

  float* const dst = a.parallel ? a.part + (long long)piece * a.total : a.y;
  const float* __restrict__ bias = a.parallel ? nullptr : a.bias;
  const long long c = c0 + 32 * wn + i;
  if (c >= C) return;
  const long long b = c / N;
  const long long ybase = b * M * N + (c - b * N);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + 32 * wm + PACKED_ROW(r);
    if constexpr ((QM & 2) != 0) {
      if (m < M) dst[ybase + (long long)m * N] = fixed_quant(bias ? tot[r] + bias[m] : tot[r], d.oq);
    } else {
      if (m < M) dst[ybase + (long long)m * N] = bias ? tot[r] + bias[m] : tot[r];
    }
  }
}

#undef PG_DW_CALL

// --- host pieces shared with packed_igemm.hip (declared in admmq_internal.h) -----------------------

int packed_fail(const char* who, int code, const char* what) {
  static thread_local char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return set_error(code, msg);
}

// A function of the sizes alone; false when they are out of range. A K step of BK, K <= Kmax,
// partial images of elem_bytes an element.
bool plan_packed(int64_t M, int64_t K, int64_t N, int64_t nb, int BK, int64_t Kmax, size_t elem_bytes, PackedPlan& pl) {
  if (M <= 0 || K <= 0 || N <= 0 || nb <= 0) return false;
  if (M > (int64_t(1) << 22) || K > Kmax || N > (int64_t(1) << 30) || nb > (int64_t(1) << 30)) return false;
  const int64_t C = nb * N;
  if (C > (int64_t(1) << 30)) return false;
  pl.C = C;
  pl.total = C * M;   // < 2^52
  const int64_t span = (int64_t)BK * kPackedPiecesMax;
  pl.kp = (int)std::max<int64_t>(kPackedPieceMin, BK * ((K + span - 1) / span));
  pl.np = (int)((K + pl.kp - 1) / pl.kp);
  pl.tiles_m = (M + kPackedBM - 1) / kPackedBM;
  pl.tiles_c = (C + kPackedBN - 1) / kPackedBN;
  pl.parallel = (pl.np > 1 && pl.tiles_m * pl.tiles_c < kPackedParallelBelow) ? 1 : 0;
  pl.ws = pl.parallel ? (size_t)pl.np * (size_t)pl.total * elem_bytes : 0;
  return true;
}

// plan_packed for a depthwise stage's Ho x Wo output positions
bool plan_packed_dw(int64_t M, int64_t K, int64_t Ho, int64_t Wo, int64_t nb, int BK, int64_t Kmax, size_t elem_bytes,
                    PackedPlan& pl) {
  if (Ho <= 0 || Wo <= 0 || Ho > (int64_t(1) << 30) || Wo > (int64_t(1) << 30)) return false;
  return plan_packed(M, K, Ho * Wo, nb, BK, Kmax, elem_bytes, pl);
}

// The weight record's checks. The float form takes every tensor scheme (tensor_minmax from 2
// bits); the integer form needs W = scale * int8: no tensor_minmax, and (u - q) - zero_point
// inside int8 - then *off = q + zero_point.
int packed_meta_check(const ::admmq_qmeta* meta, const char* who, bool integer_form, int* off) {
  if (meta->bits < 1 || meta->bits > 8) return packed_fail(who, ADMMQ_ERR_ARG, "meta bits must be 1..8");
  if (meta->scheme < kMse || meta->scheme > kAffine)
    return packed_fail(who, ADMMQ_ERR_ARG, "unknown meta scheme (the four tensor schemes only)");
  if (integer_form && meta->scheme == kMinMax)
    return packed_fail(who, ADMMQ_ERR_SCHEME,
                       "tensor_minmax weights have no integer form (their de-quantization is not scale * integer)");
  if (!integer_form && meta->scheme == kMinMax && meta->bits == 1)
    return packed_fail(who, ADMMQ_ERR_ARG, "tensor_minmax has no 1 bit code");
  if (meta->bad != 0) return packed_fail(who, ADMMQ_ERR_ARG, "meta bad != 0: not a valid packed tensor");
  if (integer_form) {
    const int64_t q = int64_t(1) << (meta->bits - 1);
    const int64_t zp = meta->scheme == kAffine ? (int64_t)meta->zero_point : 0;
    if (-q - zp < -128 || q - 1 - zp > 127)
      return packed_fail(who, ADMMQ_ERR_ARG, "affine zero_point puts (u - q) - zero_point outside int8");
    *off = (int)(q + zp);
  }
  return ADMMQ_OK;
}

// The depthwise window's checks; the output's Ho x Wo on success
int packed_dw_geometry_check(const char* who, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw,
                             int64_t* Ho, int64_t* Wo) {
  if (kh < 1 || kh > 7 || kw < 1 || kw > 7) return packed_fail(who, ADMMQ_ERR_ARG, "kernel size must be 1..7 x 1..7");
  if (sh < 1 || sw < 1) return packed_fail(who, ADMMQ_ERR_ARG, "stride must be at least 1");
  if (ph < 0 || ph >= kh || pw < 0 || pw >= kw) return packed_fail(who, ADMMQ_ERR_ARG, "padding must be in [0, kernel size)");
  if (H > (int64_t(1) << 40) || W > (int64_t(1) << 40) || H > (int64_t(1) << 40) / W)
    return packed_fail(who, ADMMQ_ERR_ARG, "sizes out of range");
  if (H + 2 * ph < kh || W + 2 * pw < kw)
    return packed_fail(who, ADMMQ_ERR_ARG, "the window does not fit the padded image (Ho, Wo >= 1)");
  *Ho = (H + 2 * ph - kh) / sh + 1;
  *Wo = (W + 2 * pw - kw) / sw + 1;
  return ADMMQ_OK;
}

// The depthwise input's extent: nb K H W <= 2^40 - 1, tested without overflow
int packed_dw_extent_check(const char* who, int64_t nb, int64_t K, int64_t H, int64_t W) {
  const int64_t tmax = (int64_t(1) << 40) - 1;
  if (K > tmax / (H * W) || nb > tmax / (H * W * K))
    return packed_fail(who, ADMMQ_ERR_ARG, "sizes out of range (nb K H W must be below 2^40)");
  return ADMMQ_OK;
}

// The parallel form's workspace: present, large enough, aligned for its elements (elem: their name in the message)
int packed_ws_check(const char* who, const PackedPlan& pl, const void* workspace, size_t workspace_bytes, const char* elem) {
  if (pl.ws > 0 && (!workspace || workspace_bytes < pl.ws)) return set_error(ADMMQ_ERR_WORKSPACE, "workspace too small");
  if (pl.ws > 0 && (reinterpret_cast<uintptr_t>(workspace) & 3) != 0) {
    char what[64];
    snprintf(what, sizeof what, "workspace must be %s aligned", elem);
    return packed_fail(who, ADMMQ_ERR_ARG, what);
  }
  return ADMMQ_OK;
}

// --- the float entry points -------------------------------------------------------------------------

// The float path's plan: K up to 2^24, and the code stream's M K below 2^40
static bool plan_pg(int64_t M, int64_t K, int64_t N, int64_t nb, PackedPlan& pl) {
  return plan_packed(M, K, N, nb, kPgBK, kPgKMax, sizeof(float), pl) && M * K < (int64_t(1) << 40);
}
static bool plan_pg_dw(int64_t M, int64_t K, int64_t Ho, int64_t Wo, int64_t nb, PackedPlan& pl) {
  return plan_packed_dw(M, K, Ho, Wo, nb, kPgBK, kPgKMax, sizeof(float), pl) && M * K < (int64_t(1) << 40);
}

// The kernels' form of a caller's quantizer; false for none (NULL or on == 0). bits checked by the caller.
static bool actq_on(const admmq_actq* q) { return q && q->on != 0; }
static bool actq_bits_ok(const admmq_actq* q) { return !actq_on(q) || (q->bits >= 1 && q->bits <= 24); }
static ActQ actq_or_none(const admmq_actq* q) { return actq_on(q) ? actq_make(q) : ActQ{0.f, 0.f, 0.f, 0}; }

static void pg_fill(PgArgs& a, const uint8_t* codes, const admmq_qmeta* meta, const float* x, const float* bias, float* y,
                    void* workspace, const PackedPlan& pl, int64_t M, int64_t K, int64_t N, int32_t x_layout) {
  a.codes = codes; a.x = x; a.bias = bias; a.y = y;
  a.part = pl.parallel ? static_cast<float*>(workspace) : nullptr;
  a.nbytes = (long long)admmq_packed_bytes(M * K, meta->bits);
  a.total = pl.total; a.C = pl.C;
  a.M = (int)M; a.K = (int)K; a.N = (int)N;
  a.xl = x_layout;
  a.kp = pl.kp; a.np = pl.np; a.parallel = pl.parallel;
  a.scheme = meta->scheme;
  a.zp = meta->scheme == kAffine ? meta->zero_point : 0;   // (the other schemes' table has none)
  a.scale = meta->scale; a.mn = meta->mn; a.rng = meta->rng;
}

static dim3 packed_grid(const PackedPlan& pl) {
  return dim3((unsigned)pl.tiles_c, (unsigned)pl.tiles_m, pl.parallel ? (unsigned)pl.np : 1u);
}

// The parallel form's second kernel (the output quantizer runs here, behind the bias), then the launches' status
static int32_t pg_finish(const PgArgs& a, const PackedPlan& pl, bool oq, const ActQ& q, hipStream_t s) {
  const dim3 grid((unsigned)((pl.total + 255) / 256));
  if (pl.parallel && oq)
    hipLaunchKernelGGL(k_packed_reduce<true>, grid, dim3(256), 0, s, a.part, pl.np, pl.total, a.bias, a.y, a.M, a.N, a.xl, q);
  else if (pl.parallel)
    hipLaunchKernelGGL(k_packed_reduce<false>, grid, dim3(256), 0, s, a.part, pl.np, pl.total, a.bias, a.y, a.M, a.N, a.xl, q);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

static int32_t packed_gemm_run(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                               const float* x, int32_t x_layout, int64_t N, int32_t nb, const float* bias, float* y,
                               const admmq_actq* out_q, void* workspace, size_t workspace_bytes, void* stream) {
  const char* const who = "packed_gemm";
  if (!codes || !x || !y || !meta) return set_error(ADMMQ_ERR_ARG, "packed_gemm: codes, meta, x and y must not be NULL");
  if (M <= 0 || K <= 0 || N <= 0 || nb <= 0) return set_error(ADMMQ_ERR_ARG, "packed_gemm: M, K, N and nb must be positive");
  int32_t rc = packed_meta_check(meta, who, false, nullptr);
  if (rc != ADMMQ_OK) return rc;
  if (trans_w != 0 && trans_w != 1) return set_error(ADMMQ_ERR_ARG, "packed_gemm: trans_w must be 0 or 1");
  if (x_layout != 0 && x_layout != 1) return set_error(ADMMQ_ERR_ARG, "packed_gemm: x_layout must be 0 or 1");
  if (x_layout == 1 && nb != 1) return set_error(ADMMQ_ERR_ARG, "packed_gemm: x_layout 1 (linear) needs nb = 1");
  if ((reinterpret_cast<uintptr_t>(codes) & 15) != 0)
    return set_error(ADMMQ_ERR_ARG, "packed_gemm: codes must be 16-byte aligned");
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(bias)) & 3) != 0)
    return set_error(ADMMQ_ERR_ARG, "packed_gemm: x, y and bias must be float aligned");
  PackedPlan pl;
  if (!plan_pg(M, K, N, nb, pl)) return set_error(ADMMQ_ERR_ARG, "packed_gemm: sizes out of range");
  rc = packed_ws_check(who, pl, workspace, workspace_bytes, "float");
  if (rc != ADMMQ_OK) return rc;
  PgArgsQ aq;   // the plain record, the output quantizer behind it
  PgArgs& a = aq;
  pg_fill(a, codes, meta, x, bias, y, workspace, pl, M, K, N, x_layout);
  // the output quantizer: in the serial form's epilogue (the OQ kernels), in the parallel form's reduction
  const bool oq = actq_on(out_q);
  aq.oq = actq_or_none(out_q);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid = packed_grid(pl);
#define ADMMQ_PG_LAUNCH(B, T, X)                                                                           \
  do {                                                                                                     \
    if (oq && !pl.parallel) hipLaunchKernelGGL((k_packed_gemm<B, T, X, true>), grid, dim3(256), 0, s, aq); \
    else hipLaunchKernelGGL((k_packed_gemm<B, T, X>), grid, dim3(256), 0, s, a);                           \
  } while (0)
#define ADMMQ_PG_BITS(B)                                     \
  if (trans_w && x_layout) ADMMQ_PG_LAUNCH(B, true, true);   \
  else if (trans_w) ADMMQ_PG_LAUNCH(B, true, false);         \
  else if (x_layout) ADMMQ_PG_LAUNCH(B, false, true);        \
  else ADMMQ_PG_LAUNCH(B, false, false)
  PACKED_BITS_SWITCH(meta->bits, ADMMQ_PG_BITS)
#undef ADMMQ_PG_BITS
#undef ADMMQ_PG_LAUNCH
  return pg_finish(a, pl, oq, aq.oq, s);
}

static int32_t packed_dwgemm_run(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const float* t,
                                 int32_t nb, int64_t H, int64_t W, const float* taps, int32_t kh, int32_t kw, int32_t sh,
                                 int32_t sw, int32_t ph, int32_t pw, const float* bias, float* y,
                                 const admmq_actq* mid_q, const admmq_actq* out_q, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  const char* const who = "packed_dwgemm";
  if (!codes || !t || !taps || !y || !meta)
    return set_error(ADMMQ_ERR_ARG, "packed_dwgemm: codes, meta, t, taps and y must not be NULL");
  if (M <= 0 || K <= 0 || H <= 0 || W <= 0 || nb <= 0)
    return set_error(ADMMQ_ERR_ARG, "packed_dwgemm: M, K, H, W and nb must be positive");
  int32_t rc = packed_meta_check(meta, who, false, nullptr);
  if (rc != ADMMQ_OK) return rc;
  int64_t Ho = 0, Wo = 0;
  rc = packed_dw_geometry_check(who, H, W, kh, kw, sh, sw, ph, pw, &Ho, &Wo);
  if (rc != ADMMQ_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(codes) & 15) != 0)
    return set_error(ADMMQ_ERR_ARG, "packed_dwgemm: codes must be 16-byte aligned");
  if (((reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(taps) | reinterpret_cast<uintptr_t>(y) |
        reinterpret_cast<uintptr_t>(bias)) & 3) != 0)
    return set_error(ADMMQ_ERR_ARG, "packed_dwgemm: t, taps, y and bias must be float aligned");
  PackedPlan pl;
  if (!plan_pg_dw(M, K, Ho, Wo, nb, pl)) return set_error(ADMMQ_ERR_ARG, "packed_dwgemm: sizes out of range");
  rc = packed_dw_extent_check(who, nb, K, H, W);
  if (rc != ADMMQ_OK) return rc;
  rc = packed_ws_check(who, pl, workspace, workspace_bytes, "float");
  if (rc != ADMMQ_OK) return rc;
  PgDwArgsQ dq;   // the plain record, the quantizers behind it
  PgDwArgs& d = dq;
  PgArgs& a = d.g;
  pg_fill(a, codes, meta, t, bias, y, workspace, pl, M, K, Ho * Wo, 0);
  d.taps = taps;
  d.H = H; d.W = W; d.HW = H * W;
  d.Wo = (int)Wo;
  d.kh = kh; d.kw = kw; d.sh = sh; d.sw = sw; d.ph = ph; d.pw = pw;
  // the mid quantizer runs in the kernel in both forms; the output quantizer in the serial
  // form's epilogue or in the parallel form's reduction
  const bool mq = actq_on(mid_q), oq = actq_on(out_q);
  const int qm = (mq ? 1 : 0) | (oq && !pl.parallel ? 2 : 0);
  dq.mq = actq_or_none(mid_q);
  dq.oq = actq_or_none(out_q);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid = packed_grid(pl);
#define ADMMQ_PG_BITS(B)                                                                        \
  if (qm == 0) hipLaunchKernelGGL((k_packed_dwgemm<B>), grid, dim3(256), 0, s, d);              \
  else if (qm == 1) hipLaunchKernelGGL((k_packed_dwgemm<B, 1>), grid, dim3(256), 0, s, dq);     \
  else if (qm == 2) hipLaunchKernelGGL((k_packed_dwgemm<B, 2>), grid, dim3(256), 0, s, dq);     \
  else hipLaunchKernelGGL((k_packed_dwgemm<B, 3>), grid, dim3(256), 0, s, dq)
  PACKED_BITS_SWITCH(meta->bits, ADMMQ_PG_BITS)
#undef ADMMQ_PG_BITS
  return pg_finish(a, pl, oq, dq.oq, s);
}

}  // namespace admmq

using namespace admmq;

extern "C" {

size_t admmq_packed_gemm_workspace_size(int64_t M, int64_t K, int64_t N, int32_t nb) {
  PackedPlan pl;
  return plan_pg(M, K, N, nb, pl) ? pl.ws : 0;
}

int32_t admmq_packed_gemm(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                          const float* x, int32_t x_layout, int64_t N, int32_t nb, const float* bias, float* y,
                          void* workspace, size_t workspace_bytes, void* stream) {
  return packed_gemm_run(codes, meta, trans_w, M, K, x, x_layout, N, nb, bias, y, nullptr, workspace, workspace_bytes,
                         stream);
}

int32_t admmq_packed_gemm_act(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                              const float* x, int32_t x_layout, int64_t N, int32_t nb, const float* bias, float* y,
                              const admmq_actq* out_q, void* workspace, size_t workspace_bytes, void* stream) {
  if (!actq_bits_ok(out_q)) return set_error(ADMMQ_ERR_ARG, "packed_gemm_act: out_q bits must be 1..24");
  return packed_gemm_run(codes, meta, trans_w, M, K, x, x_layout, N, nb, bias, y, out_q, workspace, workspace_bytes,
                         stream);
}

size_t admmq_packed_dwgemm_workspace_size(int64_t M, int64_t K, int64_t Ho, int64_t Wo, int32_t nb) {
  PackedPlan pl;
  return plan_pg_dw(M, K, Ho, Wo, nb, pl) ? pl.ws : 0;
}

int32_t admmq_packed_dwgemm(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const float* t,
                            int32_t nb, int64_t H, int64_t W, const float* taps, int32_t kh, int32_t kw, int32_t sh,
                            int32_t sw, int32_t ph, int32_t pw, const float* bias, float* y, void* workspace,
                            size_t workspace_bytes, void* stream) {
  return packed_dwgemm_run(codes, meta, M, K, t, nb, H, W, taps, kh, kw, sh, sw, ph, pw, bias, y, nullptr, nullptr,
                           workspace, workspace_bytes, stream);
}

int32_t admmq_packed_dwgemm_act(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const float* t,
                                int32_t nb, int64_t H, int64_t W, const float* taps, int32_t kh, int32_t kw,
                                int32_t sh, int32_t sw, int32_t ph, int32_t pw, const float* bias, float* y,
                                const admmq_actq* mid_q, const admmq_actq* out_q, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (!actq_bits_ok(mid_q)) return set_error(ADMMQ_ERR_ARG, "packed_dwgemm_act: mid_q bits must be 1..24");
  if (!actq_bits_ok(out_q)) return set_error(ADMMQ_ERR_ARG, "packed_dwgemm_act: out_q bits must be 1..24");
  return packed_dwgemm_run(codes, meta, M, K, t, nb, H, W, taps, kh, kw, sh, sw, ph, pw, bias, y, mid_q, out_q,
                           workspace, workspace_bytes, stream);
}

}  // extern "C"
