// Half-precision quant + low-rank GEMM (include/admmq.h "Half-precision quant + low-rank GEMM",
// DESIGN.md 2.35): y = x (D + L Rt)^T (+ bias) for x [N, K] in bfloat16 / float16 at any row
// count, D the table de-quantization of packed codes [M, K], L [M, r], Rt [r, K] in float32 or
// in x's type T. Everything runs on v_mfma_f32_32x32x16_{bf16,f16}; neither D, L Rt nor a
// float32 copy of x exists in memory.
//
//   k_hlr_down<T>             t32 = Rt_T x: the 64 x 64 tile of k_packed_hgemm with the W image
//                             staged from Rt (a float32 factor rounded once to T on the way).
//                             grid.z = nsd ranges of K, each one accumulator chain from zero that
//                             writes its own float32 image tpart[z][c][rp] (rp = 32 ceil(r / 32),
//                             the padding exact zeros). No reduce launch: the consumer adds them.
//   k_packed_hlrgemm<BITS, T> k_packed_hgemm<BITS, false, true, T>'s K loop (the same pieces,
//                             folds and integer operand: the same sums), then the tail in the
//                             same two LDS images: tot becomes v in place, acc is reused for
//                             q = L_T t_T. A tail step stages 8 j of a row of L and, for a
//                             column's 8 j, the sum of t's images in range order rounded once
//                             to T. Serial regime: y = (v + q) + bias. Parallel regime: one more
//                             workgroup a tile (blockIdx.z = np) runs the tail alone, image np.
//   k_packed_hlrreduce        parallel regime: the piece images in piece order, the epilogue,
//                             + q, + bias.
// No workgroup waits for another, nothing is combined with atomics, nothing is read past the
// code stream's last byte.
#include <algorithm>

#include "packed_half.h"

namespace admmq {

constexpr int kHlrRankMax = 256;
constexpr int kHlrSplitMax = 8;      // images of t at most
constexpr int kHlrRangeMin = 64;     // k per range of the down-projection at least
constexpr int kHlrOneLaunch = 256;   // workgroups the down-projection aims at (one a CU)
constexpr int kHlrBatch = 4;         // images of t whose loads a tail step issues together

typedef __attribute__((address_space(1))) const float hlr_gcf32;
typedef float hlr_f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const hlr_f32x4 hlr_gcf32x4;

struct HlrArgs {
  const void* L;      // [M, r] in fdt
  const void* Rt;     // [r, K] in fdt
  float* tpart;       // [nsd][N][rp] float32 images of t
  int r, rp;          // rp = 32 ceil(r / 32)
  int ksd, nsd;       // the down-projection's K ranges
  int fdt;            // ADMMQ_DT_F32, or x's type
  int lal;            // 8 j of a row of L are one (T) or two (float32) aligned 16-byte loads, all inside r or all outside
  int ral;            // the same for 8 k of a row of Rt
};

// The 16 bits of f rounded to nearest even to T (fp16 subnormals kept)
template <typename T>
__device__ __forceinline__ unsigned hlr_round_bits(float f) {
  return (unsigned)__builtin_bit_cast(unsigned short, static_cast<T>(f));
}

// A thread's 8 consecutive elements p[0..7] of a factor's row as four dwords of T: those at
// index >= nin are exact zeros and are not read. al: the 8 are 16-byte aligned and nin is 0 or 8.
template <typename T>
__device__ __forceinline__ void hlr_factor8(const void* base, long long off, int fdt, bool al, int nin, unsigned (&w)[4]) {
  if (fdt == ADMMQ_DT_F32) {
    const float* p = static_cast<const float*>(base) + off;
    float f[8];
    if (al) {
      hlr_f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
      if (nin > 0) {
        v0 = *(const hlr_gcf32x4*)p;
        v1 = *(const hlr_gcf32x4*)(p + 4);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) { f[j] = v0[j]; f[4 + j] = v1[j]; }
    } else {
      const hlr_gcf32* g = (const hlr_gcf32*)p;
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = j < nin ? g[j] : 0.f;
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) w[d] = hlr_round_bits<T>(f[2 * d]) | (hlr_round_bits<T>(f[2 * d + 1]) << 16);
  } else {
    const unsigned short* p = static_cast<const unsigned short*>(base) + off;
    if (al) {
      hg_u32x4 v = {0u, 0u, 0u, 0u};
      if (nin > 0) v = *(const gcu32x4*)p;
#pragma unroll
      for (int d = 0; d < 4; ++d) w[d] = v[d];
    } else {
      const gcu16* g = (const gcu16*)p;
      unsigned e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = j < nin ? (unsigned)g[j] : 0u;
#pragma unroll
      for (int d = 0; d < 4; ++d) w[d] = e[2 * d] | (e[2 * d + 1] << 16);
    }
  }
}

// A thread's 8 consecutive k of one row of x as k_packed_hgemm<.., XL = true> stages them: one
// 16-byte load where the rows sit on 16-byte boundaries and the 8 are inside, else 2-byte loads
// of the nk inside; a column past N (cok false) is zeroed by a select.
__device__ __forceinline__ void hlr_x8(const unsigned short* xp, bool al, bool cok, int nk, unsigned (&rx)[4]) {
  if (al && nk == 8) {
    const hg_u32x4 v = *(const gcu32x4*)xp;
#pragma unroll
    for (int d = 0; d < 4; ++d) rx[d] = cok ? v[d] : 0u;
  } else {
    const gcu16* xg = (const gcu16*)xp;
    unsigned e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = j < nk ? (unsigned)xg[j] : 0u;
#pragma unroll
    for (int d = 0; d < 4; ++d) rx[d] = cok ? (e[2 * d] | (e[2 * d + 1] << 16)) : 0u;
  }
}

// One K step of 32 of a wave's 32 x 32 block from the two images; lanes run along the W rows
template <typename T>
__device__ __forceinline__ hg_f32x16 hlr_step(const unsigned short* w, const unsigned short* x, hg_f32x16 acc) {
#pragma unroll
  for (int kk = 0; kk < kHgBK / 16; ++kk) {
    const hg_u32x4 av = *reinterpret_cast<const hg_u32x4*>(w + 16 * kk);
    const hg_u32x4 bv = *reinterpret_cast<const hg_u32x4*>(x + 16 * kk);
    acc = hg_mfma<T>(bv, av, acc);
  }
  return acc;
}

// t = Rt_T x, one K range a workgroup: grid (tiles of N, tiles of r, nsd)
template <typename T>
__global__ __launch_bounds__(256) void k_hlr_down(const HgArgs a, const HlrArgs lr) {
  __shared__ __attribute__((aligned(16))) unsigned short sW[2][kPackedBM * kHgLD];
  __shared__ __attribute__((aligned(16))) unsigned short sX[2][kPackedBN * kHgLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, i = lane & 31, h = lane >> 5;
  const int K = a.K, r = lr.r, rp = lr.rp;
  const long long C = a.C;
  const int j0 = (int)blockIdx.y * kPackedBM;
  const long long c0 = (long long)blockIdx.x * kPackedBN;
  const int z = (int)blockIdx.z;
  const int kb = z * lr.ksd, ke = min(K, kb + lr.ksd);

  const int row = tid >> 2, k8 = 8 * (tid & 3);   // both images: row of the tile, first k of the step's 8
  const bool jok = j0 + row < r;
  const long long wrow = (long long)min(j0 + row, r - 1) * K;   // (a row past r is never loaded)
  const bool cok = c0 + row < C;
  const unsigned short* __restrict__ xp = a.x + min(c0 + row, C - 1) * K + (kb + k8);

  unsigned rw[4], rx[4];
  auto load = [&](int k0) {
    const int nk = max(0, min(8, ke - (k0 + k8)));   // k of the 8 inside the range
    hlr_factor8<T>(lr.Rt, wrow + (k0 + k8), lr.fdt, lr.ral != 0, jok ? nk : 0, rw);
    hlr_x8(xp, a.xal != 0, cok, nk, rx);
    xp += kHgBK;
  };
  auto store = [&](int buf) {
    hg_u32x4 wv, xv;
#pragma unroll
    for (int d = 0; d < 4; ++d) { wv[d] = rw[d]; xv[d] = rx[d]; }
    *reinterpret_cast<hg_u32x4*>(&sW[buf][row * kHgLD + k8]) = wv;
    *reinterpret_cast<hg_u32x4*>(&sX[buf][row * kHgLD + k8]) = xv;
  };

  const bool live = j0 + 32 * wm < rp;   // (wave uniform) rows of t this wave writes
  hg_f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  load(kb);
  store(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = kb; k0 < ke; k0 += kHgBK) {
    const bool more = k0 + kHgBK < ke;
    if (more) load(k0 + kHgBK);
    if (live) acc = hlr_step<T>(sW[buf] + (32 * wm + i) * kHgLD + 8 * h, sX[buf] + (32 * wn + i) * kHgLD + 8 * h, acc);
    if (more) store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  // rows r .. rp - 1 of the image come from zero rows of the W image: exact zeros
  const int j = j0 + 32 * wm + i;
  if (j >= rp) return;
  float* const dst = lr.tpart + (long long)z * C * rp + j;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const long long c = c0 + 32 * wn + PACKED_ROW(q);
    if (c < C) dst[c * rp] = acc[q];
  }
}

template <int BITS, typename T>
__global__ __launch_bounds__(256) void k_packed_hlrgemm(const HgArgs a, const HlrArgs lr) {
  __shared__ __attribute__((aligned(16))) unsigned short sW[2][kPackedBM * kHgLD];
  __shared__ __attribute__((aligned(16))) unsigned short sX[2][kPackedBN * kHgLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, i = lane & 31, h = lane >> 5;
  const int M = a.M, K = a.K;
  const long long C = a.C;
  const int m0 = (int)blockIdx.y * kPackedBM;
  const long long c0 = (long long)blockIdx.x * kPackedBN;
  const int piece = (int)blockIdx.z;
  const bool tail_only = a.parallel && piece == a.np;   // the parallel regime's extra workgroup (uniform)
  const int kb = a.parallel ? piece * a.kp : 0;
  const int ke = a.parallel ? min(K, kb + a.kp) : K;
  const unsigned char* __restrict__ codes = a.codes;
  const long long nbytes = a.nbytes;
  const bool mm = a.scheme == kMinMax;   // (uniform)

  // W: the thread's run of 8 stream-consecutive codes; X: the 8 elements k = wk .. wk + 7 of
  // one column - both images take row tid >> 2 and k 8 (tid & 3), as k_packed_hgemm<.., false, true>
  const int wrow = tid >> 2;
  const int wk = 8 * (tid & 3);
  const int nvm = m0 + wrow < M ? 8 : 0;
  const bool cok = c0 + wrow < C;
  const long long ccl = min(c0 + wrow, C - 1);   // (a column past C reads a valid one and is zeroed)
  const int mcl = min(m0 + wrow, M - 1);         // (the tail: a row past M reads a valid one and is never stored)

  hg_f32x16 acc, tot, xacc, xtot;
#pragma unroll
  for (int q = 0; q < 16; ++q) { acc[q] = 0.f; tot[q] = 0.f; xacc[q] = 0.f; xtot[q] = 0.f; }

  if (!tail_only) {
    const long long bit0 = ((long long)(m0 + wrow) * K + (kb + wk)) * BITS;
    const int wsh = (int)(bit0 & 31);
    long long wq = bit0 >> 5;
    const unsigned short* __restrict__ xp = a.x + ccl * K + (kb + wk);
    unsigned cw[3];
    int nv = 0;
    unsigned rx[4];
    auto load = [&](int k0, bool full) {
      cw[0] = 0u; cw[1] = 0u; cw[2] = 0u;
      nv = full ? nvm : (nvm > 0 ? min(8, ke - (k0 + wk)) : 0);
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
      hlr_x8(xp, a.xal != 0, cok, full ? 8 : max(0, min(8, ke - (k0 + wk))), rx);
      xp += kHgBK;
    };
    auto store = [&](int buf) {
      constexpr unsigned mask = (1u << BITS) - 1u;
      const int p2 = wsh + 4 * BITS;
      const bool up = p2 >= 32;
      unsigned long long win[2];
      win[0] = (((unsigned long long)cw[1] << 32) | cw[0]) >> wsh;
      win[1] = (((unsigned long long)(up ? cw[2] : cw[1]) << 32) | (up ? cw[1] : cw[0])) >> (p2 & 31);
      unsigned b[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = (int)((unsigned)(win[j >> 2] >> ((j & 3) * BITS)) & mask) - a.off;
        b[j] = j < nv ? hg_int_bits<T>(v) : 0u;   // past the piece / the matrix: exactly 0
      }
      hg_u32x4 wv, xv;
#pragma unroll
      for (int d = 0; d < 4; ++d) { wv[d] = b[2 * d] | (b[2 * d + 1] << 16); xv[d] = rx[d]; }
      *reinterpret_cast<hg_u32x4*>(&sW[buf][wrow * kHgLD + wk]) = wv;
      *reinterpret_cast<hg_u32x4*>(&sX[buf][wrow * kHgLD + wk]) = xv;
    };

    const unsigned one2 = hg_int_bits<T>(1) * 0x10001u;   // the ones operand of the column sums (tensor_minmax)
    hg_u32x4 ones;
#pragma unroll
    for (int d = 0; d < 4; ++d) ones[d] = one2;

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
        acc = hg_mfma<T>(bv, av, acc);
        if (mm) xacc = hg_mfma<T>(bv, ones, xacc);
      }
      if (!more || k0 + kHgBK == pend) {   // a piece ends: fold it into the running sums
        pend += a.kp;
        if (first) {
          tot = acc;
          xtot = xacc;
          first = false;
        } else {
#pragma unroll
          for (int q = 0; q < 16; ++q) { tot[q] = tot[q] + acc[q]; xtot[q] = xtot[q] + xacc[q]; }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) { acc[q] = 0.f; xacc[q] = 0.f; }
      }
      if (more) store(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }

  const int m = m0 + 32 * wm + i;
  if (a.parallel && !tail_only) {   // the piece's sums as they are; the column sums by the first row of tiles
    float* const dst = a.part + (long long)piece * a.total;
    float* const xdst = (mm && blockIdx.y == 0) ? a.xpart + (long long)piece * C : nullptr;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const long long c = c0 + 32 * wn + PACKED_ROW(q);
      if (c < C && m < M) dst[c * M + m] = tot[q];
      if (xdst && wm == 0 && i == 0 && c < C) xdst[c] = xtot[q];
    }
    return;
  }

  // tot becomes v in place (the epilogue without the bias); acc, zero here, takes q
  if (!tail_only) {
#pragma unroll
    for (int q = 0; q < 16; ++q) tot[q] = hg_value(tot[q], xtot[q], a, false, 0.f);
  }

  // The tail q[c, m] = sum_j L_T[m, j] t_T[c, j] in steps of 32 j. Every barrier of the K loop is
  // behind us, so both images are free: step s stages into image s & 1 and one barrier a step is
  // enough (image s & 1 was last read in step s - 2, before step s - 1's barrier).
  {
    const int r = lr.r, rp = lr.rp, nsd = lr.nsd;
    const long long timg = C * rp;
    const long long lrow = (long long)mcl * r;
    const float* __restrict__ tp = lr.tpart + ccl * rp + wk;
    unsigned lw[4], tx[4];
    auto tload = [&](int j0) {
      hlr_factor8<T>(lr.L, lrow + (j0 + wk), lr.fdt, lr.lal != 0, nvm > 0 ? max(0, min(8, r - (j0 + wk))) : 0, lw);
      // the 8 j of this column in every image: two 16-byte loads each (the padded row keeps them
      // aligned and inside), kHlrBatch images in flight, added in range order
      const float* tg = tp + j0;
      float s[8];
      for (int z0 = 0; z0 < nsd; z0 += kHlrBatch) {
        hlr_f32x4 v[kHlrBatch][2];
#pragma unroll
        for (int b = 0; b < kHlrBatch; ++b) {
          if (z0 + b < nsd) {
            v[b][0] = *(const hlr_gcf32x4*)(tg + (long long)(z0 + b) * timg);
            v[b][1] = *(const hlr_gcf32x4*)(tg + (long long)(z0 + b) * timg + 4);
          }
        }
#pragma unroll
        for (int b = 0; b < kHlrBatch; ++b) {
          if (z0 + b < nsd) {
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = (z0 + b == 0) ? v[b][j >> 2][j & 3] : s[j] + v[b][j >> 2][j & 3];
          }
        }
      }
#pragma unroll
      for (int d = 0; d < 4; ++d)
        tx[d] = cok ? (hlr_round_bits<T>(s[2 * d]) | (hlr_round_bits<T>(s[2 * d + 1]) << 16)) : 0u;
    };
    tload(0);
    int buf = 0;
    for (int j0 = 0; j0 < r; j0 += kHgBK) {
      hg_u32x4 wv, xv;
#pragma unroll
      for (int d = 0; d < 4; ++d) { wv[d] = lw[d]; xv[d] = tx[d]; }
      *reinterpret_cast<hg_u32x4*>(&sW[buf][wrow * kHgLD + wk]) = wv;
      *reinterpret_cast<hg_u32x4*>(&sX[buf][wrow * kHgLD + wk]) = xv;
      __syncthreads();
      if (j0 + kHgBK < r) tload(j0 + kHgBK);
      acc = hlr_step<T>(sW[buf] + (32 * wm + i) * kHgLD + 8 * h, sX[buf] + (32 * wn + i) * kHgLD + 8 * h, acc);
      buf ^= 1;
    }
  }

  if (m >= M) return;
  if (tail_only) {
    float* const dst = a.part + (long long)a.np * a.total;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const long long c = c0 + 32 * wn + PACKED_ROW(q);
      if (c < C) dst[c * M + m] = acc[q];
    }
    return;
  }
  const float* __restrict__ bias = a.bias;
  const float bv = bias ? bias[m] : 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const long long c = c0 + 32 * wn + PACKED_ROW(q);
    const float vq = tot[q] + acc[q];
    if (c < C) hg_store(a.y, c * M + m, bias ? vq + bv : vq, a.ydt);
  }
}

// y[e] = (epilogue(((part_0[e] + part_1[e]) + ...), ((xpart_0[c] + ...))) + part_np[e]) + bias[m]: the serial regime's order
__global__ __launch_bounds__(256) void k_packed_hlrreduce(const HgArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  float s = a.part[e];
  for (int p = 1; p < a.np; ++p) s = s + a.part[(long long)p * a.total + e];
  const long long c = e / a.M;
  const int m = (int)(e - c * a.M);
  float sx = 0.f;
  if (a.scheme == kMinMax) {
    sx = a.xpart[c];
    for (int p = 1; p < a.np; ++p) sx = sx + a.xpart[(long long)p * a.C + c];
  }
  float v = hg_value(s, sx, a, false, 0.f) + a.part[(long long)a.np * a.total + e];
  if (a.bias) v = v + a.bias[m];
  hg_store(a.y, e, v, a.ydt);
}

// --- host side ------------------------------------------------------------------------------------

// The down-projection's split, a function of (K, r, N) alone: enough ranges for one workgroup a
// CU over its ceil(r / 64) ceil(N / 64) tiles, kHlrSplitMax at most, each a multiple of the K
// step and kHlrRangeMin k at least
static void plan_hlr_down(int64_t K, int64_t r, int64_t N, int& ksd, int& nsd) {
  const int64_t tiles = ((r + kPackedBM - 1) / kPackedBM) * ((N + kPackedBN - 1) / kPackedBN);
  const int64_t want = std::min<int64_t>({(kHlrOneLaunch + tiles - 1) / tiles, (int64_t)kHlrSplitMax,
                                          (K + kHlrRangeMin - 1) / kHlrRangeMin});
  const int64_t ks = kHgBK * ((((K + want - 1) / want) + kHgBK - 1) / kHgBK);
  ksd = (int)ks;
  nsd = (int)((K + ks - 1) / ks);
}

// The plan of one call and the workspace's layout:
// [np + 1 float32 images of y, parallel only][np N column sums, parallel + tensor_minmax only][pad to 16 bytes][nsd N rp floats of t]
struct HlrPlan {
  PackedPlan g;   // admmq_packed_hgemm's plan of (M, K, N, nb = 1)
  int ksd, nsd, rp, launches;
  size_t xoff, toff, ws;   // bytes to the column sums and to t; in all
};

static bool plan_hlr(const ::admmq_qmeta* meta, int64_t M, int64_t K, int64_t N, int64_t r, HlrPlan& pl) {
  if (r < 1 || r > kHlrRankMax || !plan_hg(meta, M, K, N, 1, pl.g)) return false;
  plan_hlr_down(K, r, N, pl.ksd, pl.nsd);
  pl.rp = (int)(32 * ((r + 31) / 32));
  pl.launches = pl.g.parallel ? 3 : 2;
  pl.xoff = pl.g.parallel ? (size_t)(pl.g.np + 1) * (size_t)pl.g.total * sizeof(float) : 0;
  const size_t xs = pl.g.parallel && meta->scheme == kMinMax ? (size_t)pl.g.np * (size_t)N * sizeof(float) : 0;
  pl.toff = (pl.xoff + xs + 15) & ~(size_t)15;
  pl.ws = pl.toff + (size_t)pl.nsd * (size_t)N * (size_t)pl.rp * sizeof(float);
  return true;
}

// 8 consecutive elements of a row of a [rows, n] factor from a multiple of 8: aligned 16-byte loads that never straddle the row's end
static int hlr_rows_aligned(const void* p, int64_t n) {
  return ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && n % 8 == 0) ? 1 : 0;
}

static int32_t packed_hlrgemm_run(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const void* L,
                                  const void* Rt, int32_t f_dtype, int32_t r, const void* x, int32_t x_dtype, int64_t N,
                                  const float* bias, void* y, int32_t y_dtype, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  const char* const who = "packed_hlrgemm";
  if (!codes || !x || !y || !meta || !L || !Rt)
    return packed_fail(who, ADMMQ_ERR_ARG, "codes, meta, L, Rt, x and y must not be NULL");
  if (M <= 0 || K <= 0 || N <= 0) return packed_fail(who, ADMMQ_ERR_ARG, "M, K and N must be positive");
  if (r < 1 || r > kHlrRankMax) return packed_fail(who, ADMMQ_ERR_ARG, "rank r must be 1..256");
  int32_t rc = packed_meta_check(meta, who, false, nullptr);
  if (rc != ADMMQ_OK) return rc;
  rc = hg_dtype_check(who, "x", meta, x_dtype, y_dtype);
  if (rc != ADMMQ_OK) return rc;
  if (f_dtype != ADMMQ_DT_F32 && f_dtype != x_dtype) return packed_fail(who, ADMMQ_ERR_ARG, "f_dtype must be ADMMQ_DT_F32 or x_dtype");
  rc = hg_align_check(who, "x", codes, x, y, y_dtype, bias);
  if (rc != ADMMQ_OK) return rc;
  if (((reinterpret_cast<uintptr_t>(L) | reinterpret_cast<uintptr_t>(Rt)) & (f_dtype == ADMMQ_DT_F32 ? 3 : 1)) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "L and Rt must be aligned to their element");
  HlrPlan pl;
  if (!plan_hlr(meta, M, K, N, r, pl)) return packed_fail(who, ADMMQ_ERR_ARG, "sizes out of range");
  PackedPlan whole = pl.g;   // (the size that packed_ws_check tests: the images, the column sums and t)
  whole.ws = pl.ws;
  rc = packed_ws_check(who, whole, workspace, workspace_bytes, "float");
  if (rc != ADMMQ_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "workspace must be 16-byte aligned");

  HgArgs a;
  hg_fill(a, codes, meta, x, bias, y, y_dtype, workspace, pl.g, M, K, N, 1);
  a.xpart = pl.g.parallel ? reinterpret_cast<float*>(static_cast<char*>(workspace) + pl.xoff) : nullptr;   // (behind np + 1 images here)
  HlrArgs lr;
  lr.L = L; lr.Rt = Rt;
  lr.tpart = reinterpret_cast<float*>(static_cast<char*>(workspace) + pl.toff);
  lr.r = r; lr.rp = pl.rp; lr.ksd = pl.ksd; lr.nsd = pl.nsd; lr.fdt = f_dtype;
  lr.lal = hlr_rows_aligned(L, r);
  lr.ral = hlr_rows_aligned(Rt, K);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool bf = x_dtype == ADMMQ_DT_BF16;
  const dim3 dgrid((unsigned)pl.g.tiles_c, (unsigned)((r + kPackedBM - 1) / kPackedBM), (unsigned)pl.nsd);
  if (bf) hipLaunchKernelGGL((k_hlr_down<__bf16>), dgrid, dim3(256), 0, s, a, lr);
  else hipLaunchKernelGGL((k_hlr_down<_Float16>), dgrid, dim3(256), 0, s, a, lr);
  const dim3 grid((unsigned)pl.g.tiles_c, (unsigned)pl.g.tiles_m, pl.g.parallel ? (unsigned)pl.g.np + 1u : 1u);
#define ADMMQ_HLR_BITS(B)                                                                    \
  if (bf) hipLaunchKernelGGL((k_packed_hlrgemm<B, __bf16>), grid, dim3(256), 0, s, a, lr);   \
  else hipLaunchKernelGGL((k_packed_hlrgemm<B, _Float16>), grid, dim3(256), 0, s, a, lr)
  PACKED_BITS_SWITCH(meta->bits, ADMMQ_HLR_BITS)
#undef ADMMQ_HLR_BITS
  if (pl.g.parallel)
    hipLaunchKernelGGL(k_packed_hlrreduce, dim3((unsigned)((pl.g.total + 255) / 256)), dim3(256), 0, s, a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

}  // namespace admmq

using namespace admmq;

extern "C" {

size_t admmq_packed_hlrgemm_workspace_size(const admmq_qmeta* meta, int64_t M, int64_t K, int64_t N, int32_t r) {
  HlrPlan pl;
  return plan_hlr(meta, M, K, N, r, pl) ? pl.ws : 0;
}

int32_t admmq_packed_hlrgemm_plan(const admmq_qmeta* meta, int64_t M, int64_t K, int64_t N, int32_t r, int32_t out[4]) {
  HlrPlan pl;
  if (!out || !plan_hlr(meta, M, K, N, r, pl)) return ADMMQ_ERR_ARG;
  out[0] = pl.g.np; out[1] = pl.g.parallel; out[2] = pl.nsd; out[3] = pl.launches;
  return ADMMQ_OK;
}

int32_t admmq_packed_hlrgemm(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const void* L,
                             const void* Rt, int32_t f_dtype, int32_t r, const void* x, int32_t x_dtype, int64_t N,
                             const float* bias, void* y, int32_t y_dtype, void* workspace, size_t workspace_bytes,
                             void* stream) {
  return packed_hlrgemm_run(codes, meta, M, K, L, Rt, f_dtype, r, x, x_dtype, N, bias, y, y_dtype, workspace,
                            workspace_bytes, stream);
}

}  // extern "C"
