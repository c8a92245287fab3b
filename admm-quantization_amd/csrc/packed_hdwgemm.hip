// Fused depthwise kh x kw + 1x1 stage of a packed CP layer on bf16 / fp16 activations
// (include/admmq.h "Half-precision fused depthwise + 1x1"):
//   z32[k, (b, oh, ow)] = sum_tap taps[tap][k] float(t[b, k, ih, iw])   k_packed_dwgemm's step 1 in float32
//   zh = z32 rounded once, to nearest even, to t's type
//   Y  = admmq_packed_hgemm's arithmetic on zh (trans_w 0, x_layout 0)
// zh is formed while the activation tile is staged and never exists in memory. The W decode, the
// LDS images, the K pieces, the fold, the ones operand of tensor_minmax, the two regimes,
// k_packed_hreduce and the float32 epilogue are k_packed_hgemm's (packed_half.h), so the result
// has the bits of admmq_packed_hgemm on a Z formed by the first two lines.
//
// Staging. A thread owns one column c = tid & 63 of the tile and the 8 consecutive channels
// k = k0 + 8 (tid >> 6) + j of a step: the k group is uniform over a wave, so the 8 tap weights of
// a tap are scalar loads, and the 8 sums leave as one 16-byte LDS store into the [c][k] image. The
// column's (b, oh, ow), its first input position, the rows / columns of the window inside the
// image (two bit masks) and its channel plane are derived once; a K step advances one pointer by
// 32 H W elements. The 2-byte loads of t are issued two taps (16 loads) at a time and taken
// whatever the masks say (the empty asm keeps them together and ahead of the selects); a tap
// outside the image reads its plane's first element and is dropped by a select; a k past the
// piece's or K's end reads nothing and yields exactly 0; a column past C reads the clamped column
// and is zeroed.
//
// Work split. On the 16-bit MFMA a step's matrix work is a quarter of the fp32 kernel's while the
// stencil costs the same, and every row tile of a column tile forms the same stencil again. RT = 2
// (the serial regime with M > 64) gives a workgroup a 128 x 64 tile: the staged z block is
// multiplied against two 64-row weight blocks (two sW images, two accumulator sets a wave, one
// shared S_x accumulator), so the stencil is formed ceil(M / 128) times a column tile. The K pieces
// and the fold order are the 64 x 64 plan's: an output's accumulator chain is the same instruction
// sequence in either form, its bits do not depend on RT. RT = 1 is k_packed_hgemm's tile, used in
// the parallel-pieces regime, where the workgroup count matters.
#include <algorithm>
#include <cstdlib>

#include "packed_half.h"

namespace admmq {

struct HdwArgs {
  HgArgs g;            // x = t [nb, K, H, W]; N = Ho Wo; C = nb N; xl = 0
  const float* taps;   // [kh kw][K]
  long long H, W, HW;
  int Wo;
  int kh, kw, sh, sw, ph, pw;
};

// float32 of the 16 bits v (exact)
template <typename T>
__device__ __forceinline__ float hdw_widen(unsigned v) {
  if constexpr (std::is_same_v<T, __bf16>) return __builtin_bit_cast(float, v << 16);
  else return (float)__builtin_bit_cast(_Float16, (unsigned short)v);
}

// (lo, hi) rounded to nearest even to T, as one dword
template <typename T>
__device__ __forceinline__ unsigned hdw_pack(float lo, float hi) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef T tx2 __attribute__((ext_vector_type(2)));
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, tx2));
}

template <int BITS, typename T, int RT>
__global__ __launch_bounds__(256) void k_packed_hdwgemm(const HdwArgs d) {
  __shared__ __attribute__((aligned(16))) unsigned short sW[2][RT * kPackedBM * kHgLD];
  __shared__ __attribute__((aligned(16))) unsigned short sX[2][kPackedBN * kHgLD];
  const HgArgs& a = d.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, i = lane & 31, h = lane >> 5;
  const int M = a.M, K = a.K, N = a.N;
  const long long C = a.C;
  const int m0 = (int)blockIdx.y * (RT * kPackedBM);
  const long long c0 = (long long)blockIdx.x * kPackedBN;
  const int piece = (int)blockIdx.z;
  const int kb = a.parallel ? piece * a.kp : 0;
  const int ke = a.parallel ? min(K, kb + a.kp) : K;
  const unsigned char* __restrict__ codes = a.codes;
  const long long nbytes = a.nbytes;
  const bool mm = a.scheme == kMinMax;   // (uniform)

  // W: as k_packed_hgemm with trans_w = 0, one run of 8 codes per 64-row block. Block rt's run
  // starts 64 K BITS bits (whole dwords) behind block 0's: the same shift, another dword index.
  const int wrow = tid >> 2;
  const int wk = 8 * (tid & 3);
  const long long bit0 = ((long long)(m0 + wrow) * K + (kb + wk)) * BITS;
  const int wsh = (int)(bit0 & 31);
  long long wq = bit0 >> 5;
  const long long wblock = 2ll * K * BITS;   // dwords between the blocks' runs
  int nvm[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) nvm[rt] = m0 + kPackedBM * rt + wrow < M ? 8 : 0;
  // Z: one column, k = xk + j
  const int xc = tid & 63;
  const int xk = __builtin_amdgcn_readfirstlane(8 * (tid >> 6));
  const bool cok = c0 + xc < C;
  const int kh = d.kh, kw = d.kw;
  const long long W = d.W, HW = d.HW;
  long long tbase;                   // element offset of the window's first position in a channel plane (may be negative)
  unsigned rmask = 0u, cmask = 0u;   // bit a / b: window row a / column b lies inside the image
  const unsigned short* __restrict__ tp;
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
  const long long tstep = (long long)kHgBK * HW;

  unsigned cw[RT][3];
  int nv[RT];
  unsigned rx[4];
  // the loads of the next step and its tap sums (each call advances wq, tp and wp by one step)
  auto load = [&](int k0, auto full) {
    constexpr bool FULL = decltype(full)::value;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      cw[rt][0] = 0u; cw[rt][1] = 0u; cw[rt][2] = 0u;
      if (FULL) nv[rt] = nvm[rt];
      else nv[rt] = nvm[rt] > 0 ? min(8, ke - (k0 + wk)) : 0;
      if (nv[rt] > 0) {
        const long long q0 = wq + rt * wblock;
        if (4 * q0 + 12 <= nbytes) {   // all three inside the stream: plain loads, issued together
          const gcu32* q = (const gcu32*)(codes + 4 * q0);
          cw[rt][0] = q[0]; cw[rt][1] = q[1]; cw[rt][2] = q[2];
        } else {                       // the stream's end: nothing past its last byte is read
          cw[rt][0] = code_dword(codes, q0, nbytes);
          cw[rt][1] = code_dword(codes, q0 + 1, nbytes);
          cw[rt][2] = code_dword(codes, q0 + 2, nbytes);
        }
      }
    }
    wq += BITS;
    const gcu16* tg = (const gcu16*)tp;
    const gcf32* wg = (const gcf32*)wp;
    float z[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = 0.f;
    // two taps at a time, summed in tap order; an odd count's last pair repeats the last tap with
    // its second half switched off
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
      float w0[8], w1[8];
      unsigned v0[8], v1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (FULL) {
          w0[j] = wt0[j];
          w1[j] = wt1[j];
          v0[j] = tg[off0 + (long long)j * HW];
          v1[j] = tg[off1 + (long long)j * HW];
        } else {
          const bool in = k0 + xk + j < ke;   // (uniform over the wave)
          w0[j] = in ? wt0[j] : 0.f;
          w1[j] = in ? wt1[j] : 0.f;
          v0[j] = in ? (unsigned)tg[off0 + (long long)j * HW] : 0u;
          v1[j] = in ? (unsigned)tg[off1 + (long long)j * HW] : 0u;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) asm("" : "+v"(v0[j]), "+v"(v1[j]));
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float s = z[j] + w0[j] * hdw_widen<T>(v0[j]);
        z[j] = ok0 ? s : z[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float s = z[j] + w1[j] * hdw_widen<T>(v1[j]);
        z[j] = ok1 ? s : z[j];
      }
      ta = ta1; tb = tb1;
      if (++tb == kw) { tb = 0; ++ta; }
    }
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) rx[dd] = cok ? hdw_pack<T>(z[2 * dd], z[2 * dd + 1]) : 0u;
    tp += tstep;
    wp += kHgBK;
  };
  auto store = [&](int buf) {
    constexpr unsigned mask = (1u << BITS) - 1u;
    const int p2 = wsh + 4 * BITS;
    const bool up = p2 >= 32;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      unsigned long long win[2];
      win[0] = (((unsigned long long)cw[rt][1] << 32) | cw[rt][0]) >> wsh;
      win[1] = (((unsigned long long)(up ? cw[rt][2] : cw[rt][1]) << 32) | (up ? cw[rt][1] : cw[rt][0])) >> (p2 & 31);
      unsigned b[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = (int)((unsigned)(win[j >> 2] >> ((j & 3) * BITS)) & mask) - a.off;
        b[j] = j < nv[rt] ? hg_int_bits<T>(v) : 0u;   // past the run's row / the piece / the matrix: exactly 0
      }
      hg_u32x4 v;
#pragma unroll
      for (int dd = 0; dd < 4; ++dd) v[dd] = b[2 * dd] | (b[2 * dd + 1] << 16);
      *reinterpret_cast<hg_u32x4*>(&sW[buf][(kPackedBM * rt + wrow) * kHgLD + wk]) = v;
    }
    hg_u32x4 xv;
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) xv[dd] = rx[dd];
    *reinterpret_cast<hg_u32x4*>(&sX[buf][xc * kHgLD + xk]) = xv;
  };
  // (every call inlined: a lambda that stays a call keeps its captures in scratch)
  auto load_step = [&](int k0) {
    if (k0 + kHgBK <= ke) [[clang::always_inline]] load(k0, std::true_type{});
    else [[clang::always_inline]] load(k0, std::false_type{});
  };

  const unsigned one2 = hg_int_bits<T>(1) * 0x10001u;
  hg_u32x4 ones;
#pragma unroll
  for (int dd = 0; dd < 4; ++dd) ones[dd] = one2;

  hg_f32x16 acc[RT], tot[RT], xacc, xtot;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) { acc[rt][r] = 0.f; tot[rt][r] = 0.f; }
    xacc[r] = 0.f; xtot[r] = 0.f;
  }
  bool first = true;
  int pend = kb + a.kp;   // the current piece's end
  [[clang::always_inline]] load_step(kb);
  [[clang::always_inline]] store(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = kb; k0 < ke; k0 += kHgBK) {
    const bool more = k0 + kHgBK < ke;
    if (more) [[clang::always_inline]] load_step(k0 + kHgBK);
    const unsigned short* w = sW[buf] + (32 * wm + i) * kHgLD + 8 * h;
    const unsigned short* x = sX[buf] + (32 * wn + i) * kHgLD + 8 * h;
#pragma unroll
    for (int kk = 0; kk < kHgBK / 16; ++kk) {
      const hg_u32x4 bv = *reinterpret_cast<const hg_u32x4*>(x + 16 * kk);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const hg_u32x4 av = *reinterpret_cast<const hg_u32x4*>(w + kPackedBM * kHgLD * rt + 16 * kk);
        acc[rt] = hg_mfma<T>(av, bv, acc[rt]);
      }
      if (mm) xacc = hg_mfma<T>(ones, bv, xacc);
    }
    if (!more || k0 + kHgBK == pend) {   // a piece ends: fold it into the running sums
      pend += a.kp;
      if (first) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) tot[rt] = acc[rt];
        xtot = xacc;
        first = false;
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) tot[rt][r] = tot[rt][r] + acc[rt][r];
          xtot[r] = xtot[r] + xacc[r];
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][r] = 0.f;
        xacc[r] = 0.f;
      }
    }
    if (more) [[clang::always_inline]] store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // Epilogue, as k_packed_hgemm's layout 0: lanes along the columns (Y[(b M + m) N + n])
  const long long c = c0 + 32 * wn + i;
  if (c >= C) return;
  const long long b = c / N;
  const long long ybase = b * M * N + (c - b * N);
  if (a.parallel) {
    float* const dst = a.part + (long long)piece * a.total;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + kPackedBM * rt + 32 * wm + PACKED_ROW(r);
        if (m < M) dst[ybase + (long long)m * N] = tot[rt][r];
      }
    }
    if (mm && blockIdx.y == 0 && wm == 0 && h == 0) a.xpart[(long long)piece * C + c] = xtot[0];
    return;
  }
  const float* __restrict__ bias = a.bias;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + kPackedBM * rt + 32 * wm + PACKED_ROW(r);
      if (m < M)
        hg_store(a.y, ybase + (long long)m * N, hg_value(tot[rt][r], xtot[r], a, bias != nullptr, bias ? bias[m] : 0.f), a.ydt);
    }
  }
}

// --- host side ------------------------------------------------------------------------------------

// plan_hg for a depthwise stage's Ho x Wo output positions (plan_packed_dw's test of them)
static bool plan_hdw(const ::admmq_qmeta* meta, int64_t M, int64_t K, int64_t Ho, int64_t Wo, int64_t nb, PackedPlan& pl) {
  if (Ho <= 0 || Wo <= 0 || Ho > (int64_t(1) << 30) || Wo > (int64_t(1) << 30)) return false;
  return plan_hg(meta, M, K, Ho * Wo, nb, pl);
}

// Diagnostics: ADMMQ_HDW_RT=1 keeps the 64-row tile in the serial regime too (the same bits; DESIGN.md 2.34's timing)
static bool hdw_wide_rows() {
  const char* e = std::getenv("ADMMQ_HDW_RT");
  return !(e && e[0] == '1' && e[1] == '\0');
}

static int32_t packed_hdwgemm_run(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const void* t,
                                  int32_t t_dtype, int32_t nb, int64_t H, int64_t W, const float* taps, int32_t kh,
                                  int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw, const float* bias, void* y,
                                  int32_t y_dtype, void* workspace, size_t workspace_bytes, void* stream) {
  const char* const who = "packed_hdwgemm";
  if (!codes || !t || !taps || !y || !meta)
    return packed_fail(who, ADMMQ_ERR_ARG, "codes, meta, t, taps and y must not be NULL");
  if (M <= 0 || K <= 0 || H <= 0 || W <= 0 || nb <= 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "M, K, H, W and nb must be positive");
  int32_t rc = packed_meta_check(meta, who, false, nullptr);
  if (rc != ADMMQ_OK) return rc;
  int64_t Ho = 0, Wo = 0;
  rc = packed_dw_geometry_check(who, H, W, kh, kw, sh, sw, ph, pw, &Ho, &Wo);
  if (rc != ADMMQ_OK) return rc;
  rc = hg_dtype_check(who, "t", meta, t_dtype, y_dtype);
  if (rc != ADMMQ_OK) return rc;
  rc = hg_align_check(who, "t", codes, t, y, y_dtype, bias);
  if (rc != ADMMQ_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(taps) & 3) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "taps must be float aligned");
  PackedPlan pl;
  if (!plan_hdw(meta, M, K, Ho, Wo, nb, pl)) return packed_fail(who, ADMMQ_ERR_ARG, "sizes out of range");
  rc = packed_dw_extent_check(who, nb, K, H, W);
  if (rc != ADMMQ_OK) return rc;
  rc = packed_ws_check(who, pl, workspace, workspace_bytes, "float");
  if (rc != ADMMQ_OK) return rc;
  HdwArgs d;
  hg_fill(d.g, codes, meta, t, bias, y, y_dtype, workspace, pl, M, K, Ho * Wo, 0);
  d.taps = taps;
  d.H = H; d.W = W; d.HW = H * W;
  d.Wo = (int)Wo;
  d.kh = kh; d.kw = kw; d.sh = sh; d.sw = sw; d.ph = ph; d.pw = pw;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the 128-row tile in the serial regime: half the row tiles, the plan's pieces as they are
  const bool wide = !pl.parallel && M > kPackedBM && hdw_wide_rows();
  const dim3 grid((unsigned)pl.tiles_c, (unsigned)(wide ? (pl.tiles_m + 1) / 2 : pl.tiles_m), pl.parallel ? (unsigned)pl.np : 1u);
  const bool bf = t_dtype == ADMMQ_DT_BF16;
#define ADMMQ_HDW_LAUNCH(B, R)                                                                 \
  do {                                                                                         \
    if (bf) hipLaunchKernelGGL((k_packed_hdwgemm<B, __bf16, R>), grid, dim3(256), 0, s, d);    \
    else hipLaunchKernelGGL((k_packed_hdwgemm<B, _Float16, R>), grid, dim3(256), 0, s, d);     \
  } while (0)
#define ADMMQ_HDW_BITS(B)                \
  if (wide) ADMMQ_HDW_LAUNCH(B, 2);      \
  else ADMMQ_HDW_LAUNCH(B, 1)
  PACKED_BITS_SWITCH(meta->bits, ADMMQ_HDW_BITS)
#undef ADMMQ_HDW_BITS
#undef ADMMQ_HDW_LAUNCH
  return hg_finish(d.g, pl, stream);
}

}  // namespace admmq

using namespace admmq;

extern "C" {

size_t admmq_packed_hdwgemm_workspace_size(const admmq_qmeta* meta, int64_t M, int64_t K, int64_t Ho, int64_t Wo, int32_t nb) {
  PackedPlan pl;
  return plan_hdw(meta, M, K, Ho, Wo, nb, pl) ? pl.ws : 0;
}

int32_t admmq_packed_hdwgemm(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const void* t,
                             int32_t t_dtype, int32_t nb, int64_t H, int64_t W, const float* taps, int32_t kh, int32_t kw,
                             int32_t sh, int32_t sw, int32_t ph, int32_t pw, const float* bias, void* y, int32_t y_dtype,
                             void* workspace, size_t workspace_bytes, void* stream) {
  return packed_hdwgemm_run(codes, meta, M, K, t, t_dtype, nb, H, W, taps, kh, kw, sh, sw, ph, pw, bias, y, y_dtype,
                            workspace, workspace_bytes, stream);
}

}  // extern "C"
