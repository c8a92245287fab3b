// Integer quant + low-rank GEMM (include/admmq.h "Integer quant + low-rank GEMM"):
//   y[N, M] = x^ (D + L Rt)^T (+ bias),  x^ = g ux + mn_x,  g = rng_x / n_x
// for uint8 activation codes ux [N, K] at any row count, D = scale a the integer form of packed
// codes [M, K] (admmq_packed_igemm's), L [M, r] and Rt [r, K] in float32 or in the tail type T
// (bfloat16 / float16). The big product runs on v_mfma_i32_32x32x32_i8, the rank-r branch on
// v_mfma_f32_32x32x16_{bf16,f16}; no decoded copy of the codes exists in memory.
//
//   k_ilr_factorsums<T>        rho[j] = float(sum_k double(Rt_T[j, k])), once per weight: one wave a row,
//                              lane l adds k = l, l + 64, ... in increasing k, lane 0 adds the 64
//                              partials in increasing l.
//   k_ilr_down<T>              U32 = Rt_T ux: a 64 (j) x 64 (c) tile of four waves, K step 32. A thread
//                              turns 8 code bytes of a column into 8 exact T integers and 8 elements of
//                              a row of Rt into T (a float32 factor rounded once) for the [c][k] and
//                              [j][k] LDS images. grid.z = nsd ranges of K, each one accumulator chain
//                              from zero with its own float32 image upart[z][c][rp] (rp = 32 ceil(r / 32),
//                              the padding exact zeros). No reduce launch: the consumer adds them.
//   k_packed_ilrgemm<BITS, T, OUT>   k_packed_igemm<BITS, false, true>'s int8 K loop (64 x 64 tile, K step
//                              64, two LDS buffers of [64][80] bytes an operand), then the tail in the
//                              same LDS: a buffer holds [64][40] 16-bit elements, one 32-wide j step. Tail
//                              step s stages, into buffer s & 1, 8 j of a row of L_T and 8 j of a column's
//                              t_T = T(float(gd double(sum_z U32_z) + double(mn_x) double(rho))), then one
//                              16-bit MFMA pair into a float32 accumulator q beside the int32 one. The
//                              epilogue is double: scale (gd S + mn_x A) + q + bias, one rounding.
//                              Parallel regime (few tiles): grid.z = np + 1; piece z < np writes its
//                              int32 image, workgroup z = np runs the tail alone and writes the float32
//                              image of q.
//   k_packed_ilrreduce         parallel regime: the int32 images' sum, + q, the same epilogue.
// No workgroup waits for another, no output is combined with atomics (the clamp counter is one
// atomic a workgroup, zeroed by a one-thread kernel), nothing past the code stream's last byte
// or past the last row of ux is read.
#include <algorithm>
#include <type_traits>

#include "../../include/admmq.h"
#include "packed_half.h"

namespace admmq {

constexpr int kIlrBK = 64;             // the int8 K step (k_packed_igemm's)
constexpr int kIlrLD = 80;             // LDS row stride in bytes of both forms: 64 int8 + pad = 32 T + pad (kHgLD elements)
constexpr int64_t kIlrKMax = 65536;    // 128 255 K < 2^31
constexpr int kIlrRankMax = 256;
constexpr int kIlrSplitMax = 8;        // images of U at most
constexpr int kIlrRangeMin = 64;       // k per range of the down-projection at least
constexpr int kIlrOneLaunch = 256;     // workgroups the down-projection aims at (one a CU)
constexpr int kIlrBatch = 4;           // images of U whose loads a tail step issues together
constexpr int kIlrFloat = 0, kIlrQuant = 1, kIlrCodes = 2;
static_assert(kIlrLD == 2 * kHgLD, "the tail's 16-bit image is the int8 image's buffer");

typedef int ilr_i32x16 __attribute__((ext_vector_type(16)));
typedef int ilr_i32x4 __attribute__((ext_vector_type(4)));
typedef float ilr_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned ilr_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) const float ilr_gcf32;
typedef __attribute__((address_space(1))) const ilr_f32x4 ilr_gcf32x4;
typedef __attribute__((address_space(1))) const unsigned char ilr_gcu8;
typedef __attribute__((address_space(1))) const ilr_u32x2 ilr_gcu32x2;

struct IlrArgs {
  const unsigned char* codes;
  const unsigned char* x;   // ux [N, K]
  const float* bias;
  const int* rowsum;
  float* y;
  unsigned char* yc;
  int* part;          // parallel regime: [np][total] int32 images of the pieces
  float* qpart;       // parallel regime: [total] float32 image of q
  int* clamped;       // codes output: the clamp counter, or NULL
  const void* L;      // [M, r] in fdt
  const void* Rt;     // [r, K] in fdt
  const float* rho;   // [r]
  float* upart;       // [nsd][N][rp] float32 images of U
  long long nbytes;   // bytes of the code stream
  long long total;    // N * M
  long long C;        // N
  int M, K;
  int kp, np, parallel;
  int off;            // q + zp: a = uw - off
  int xal4, xal8;     // every row of ux starts on a 4 / 8 byte boundary and K is a multiple of it
  int out;            // kIlrFloat, kIlrQuant, kIlrCodes
  int r, rp;          // rp = 32 ceil(r / 32)
  int ksd, nsd;       // the down-projection's K ranges
  int fdt;            // ADMMQ_DT_F32 or the tail type
  int lal, ral;       // 8 elements of a row of L / Rt from a multiple of 8: aligned 16-byte loads inside the row
  double s, g, mnx;   // the weight's scale, rng_x / n_x, mn_x
  ActQ oq;
};

// The 16 bits of f rounded to nearest even to T (fp16 subnormals kept)
template <typename T>
__device__ __forceinline__ unsigned ilr_round_bits(float f) {
  return (unsigned)__builtin_bit_cast(unsigned short, static_cast<T>(f));
}
template <typename T>
__device__ __forceinline__ float ilr_from_bits(unsigned b) {
  return (float)__builtin_bit_cast(T, (unsigned short)b);
}

// A thread's 8 consecutive elements p[0..7] of a factor's row as four dwords of T: those at index
// >= nin are exact zeros and are not read. al: the 8 are 16-byte aligned and nin is 0 or 8.
template <typename T>
__device__ __forceinline__ void ilr_factor8(const void* base, long long off, int fdt, bool al, int nin, unsigned (&w)[4]) {
  if (fdt == ADMMQ_DT_F32) {
    const float* p = static_cast<const float*>(base) + off;
    float f[8];
    if (al) {
      ilr_f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
      if (nin > 0) {
        v0 = *(const ilr_gcf32x4*)p;
        v1 = *(const ilr_gcf32x4*)(p + 4);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) { f[j] = v0[j]; f[4 + j] = v1[j]; }
    } else {
      const ilr_gcf32* g = (const ilr_gcf32*)p;
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = j < nin ? g[j] : 0.f;
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) w[d] = ilr_round_bits<T>(f[2 * d]) | (ilr_round_bits<T>(f[2 * d + 1]) << 16);
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

// act_code of packed_igemm.hip: fixed_quant's level clamped to [0, n] (a NaN: 0); cnt counts the clamped ones
__device__ __forceinline__ unsigned ilr_act_code(float x, const ActQ& q, int& cnt) {
  const float r = (x - q.mn) / q.rng;
  const float qi = __builtin_floorf(r * q.n + 0.5f);
  const bool in = qi >= 0.f && qi <= q.n;
  cnt += in ? 0 : 1;
  const float c = qi >= 0.f ? (qi <= q.n ? qi : q.n) : 0.f;
  return (unsigned)(int)c;
}

// The block's count into *counter by one atomic (none for a zero count). All 256 threads call.
__device__ __forceinline__ void ilr_count(int cnt, int* counter) {
  __shared__ int sc[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = sc[0] + sc[1] + sc[2] + sc[3];
    if (t > 0) atomicAdd(counter, t);
  }
}

// t32 = float(gd double(U32) + double(mn_x) double(rho)): double operations rounded one by one
__device__ __forceinline__ float ilr_t32(float U, float rho, double g, double mnx) {
#pragma clang fp contract(off)
  const double a = g * (double)U;
  const double b = mnx * (double)rho;
  return (float)(a + b);
}

// The output formula: double operations rounded one by one, one rounding to float32.
// acc = sum_k a (ux - 128); S = acc + 128 A is exact in int64 and in double.
__device__ __forceinline__ float ilr_value(int acc, int A, float q, const IlrArgs& a, bool has_bias, float bv) {
#pragma clang fp contract(off)
  const double S = (double)((long long)acc + 128ll * (long long)A);
  const double gs = a.g * S;
  const double ma = a.mnx * (double)A;
  double v = a.s * (gs + ma);
  v = v + (double)q;
  if (has_bias) v = v + (double)bv;
  return (float)v;
}

// One output element in the call's output form (one thread an element)
template <int OUT>
__device__ __forceinline__ void ilr_out(const IlrArgs& a, long long e, float v, int& cnt) {
  if constexpr (OUT == kIlrCodes) a.yc[e] = (unsigned char)ilr_act_code(v, a.oq, cnt);
  else if constexpr (OUT == kIlrQuant) a.y[e] = fixed_quant(v, a.oq);
  else a.y[e] = v;
}

// rho[j] = float(sum_k double(Rt_T[j, k])): one wave a row, the order of the header
template <typename T>
__global__ __launch_bounds__(256) void k_ilr_factorsums(const void* Rt, int fdt, int r, int K, float* __restrict__ rho) {
  __shared__ double sp[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = (int)blockIdx.x * 4 + wave;
  double s = 0.0;
  if (j < r) {
    const long long row = (long long)j * K;
    for (int k = lane; k < K; k += 64) {
      float f;
      if (fdt == ADMMQ_DT_F32) f = ilr_from_bits<T>(ilr_round_bits<T>(static_cast<const float*>(Rt)[row + k]));
      else f = ilr_from_bits<T>(static_cast<const unsigned short*>(Rt)[row + k]);
      s = s + (double)f;
    }
  }
  sp[wave][lane] = s;
  __syncthreads();
  if (lane == 0 && j < r) {
    double t = sp[wave][0];
    for (int l = 1; l < 64; ++l) t = t + sp[wave][l];
    rho[j] = (float)t;
  }
}

// U32 = Rt_T ux, one K range a workgroup: grid (tiles of N, tiles of r, nsd)
template <typename T>
__global__ __launch_bounds__(256) void k_ilr_down(const IlrArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned short sW[2][kPackedBM * kHgLD];
  __shared__ __attribute__((aligned(16))) unsigned short sX[2][kPackedBN * kHgLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, i = lane & 31, h = lane >> 5;
  const int K = a.K, r = a.r, rp = a.rp;
  const long long C = a.C;
  const int j0 = (int)blockIdx.y * kPackedBM;
  const long long c0 = (long long)blockIdx.x * kPackedBN;
  const int z = (int)blockIdx.z;
  const int kb = z * a.ksd, ke = min(K, kb + a.ksd);

  const int row = tid >> 2, k8 = 8 * (tid & 3);   // both images: row of the tile, first k of the step's 8
  const bool jok = j0 + row < r;
  const long long wrow = (long long)min(j0 + row, r - 1) * K;   // (a row past r is never loaded)
  const bool cok = c0 + row < C;
  const unsigned char* __restrict__ xp = a.x + min(c0 + row, C - 1) * K + (kb + k8);   // (a column past N reads a valid one and is zeroed)

  unsigned rw[4], rx[2];
  auto load = [&](int k0) {
    const int nk = max(0, min(8, ke - (k0 + k8)));   // k of the 8 inside the range
    ilr_factor8<T>(a.Rt, wrow + (k0 + k8), a.fdt, a.ral != 0, jok ? nk : 0, rw);
    if (a.xal8 && nk == 8) {
      const ilr_u32x2 v = *(const ilr_gcu32x2*)xp;
      rx[0] = v[0]; rx[1] = v[1];
    } else {
      const ilr_gcu8* xg = (const ilr_gcu8*)xp;
      rx[0] = 0u; rx[1] = 0u;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < nk) rx[j >> 2] |= (unsigned)xg[j] << (8 * (j & 3));
    }
    xp += kHgBK;
  };
  auto store = [&](int buf) {
    hg_u32x4 wv, xv;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      wv[d] = rw[d];
      const unsigned b0 = (rx[d >> 1] >> (16 * (d & 1))) & 255u, b1 = (rx[d >> 1] >> (16 * (d & 1) + 8)) & 255u;
      xv[d] = cok ? (hg_int_bits<T>((int)b0) | (hg_int_bits<T>((int)b1) << 16)) : 0u;   // a code is an exact T integer
    }
    *reinterpret_cast<hg_u32x4*>(&sW[buf][row * kHgLD + k8]) = wv;
    *reinterpret_cast<hg_u32x4*>(&sX[buf][row * kHgLD + k8]) = xv;
  };

  const bool live = j0 + 32 * wm < rp;   // (wave uniform) rows of U this wave writes
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
    if (live) {
      const unsigned short* w = sW[buf] + (32 * wm + i) * kHgLD + 8 * h;
      const unsigned short* x = sX[buf] + (32 * wn + i) * kHgLD + 8 * h;
#pragma unroll
      for (int kk = 0; kk < kHgBK / 16; ++kk) {
        const hg_u32x4 av = *reinterpret_cast<const hg_u32x4*>(w + 16 * kk);
        const hg_u32x4 bv = *reinterpret_cast<const hg_u32x4*>(x + 16 * kk);
        acc = hg_mfma<T>(bv, av, acc);
      }
    }
    if (more) store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  // rows r .. rp - 1 of the image come from zero rows of the W image: exact zeros
  const int j = j0 + 32 * wm + i;
  if (j >= rp) return;
  float* const dst = a.upart + (long long)z * C * rp + j;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const long long c = c0 + 32 * wn + PACKED_ROW(q);
    if (c < C) dst[c * rp] = acc[q];
  }
}

template <int BITS, typename T, int OUT>
__global__ __launch_bounds__(256) void k_packed_ilrgemm(const IlrArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char sW[2][kPackedBM * kIlrLD];
  __shared__ __attribute__((aligned(16))) unsigned char sX[2][kPackedBN * kIlrLD];
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

  ilr_i32x16 acc;
  hg_f32x16 qacc;
#pragma unroll
  for (int q = 0; q < 16; ++q) { acc[q] = 0; qacc[q] = 0.f; }

  if (!tail_only) {
    // W: two runs of 8 stream-consecutive codes of a step's 64 x 64 block (run id = tid + 256 u, 8 runs
    // to a row); X: the 16 bytes k = xk .. xk + 15 of one column - k_packed_igemm<BITS, false, true>'s
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
    const int xc = tid >> 2, xk = 16 * (tid & 3);
    const bool cok = c0 + xc < C;
    const unsigned char* __restrict__ xp = a.x + min(c0 + xc, C - 1) * K + (kb + xk);   // (a column past N reads a valid one and is zeroed)

    unsigned cw[2][3];
    int nv[2] = {0, 0};
    unsigned rx[4];
    auto load = [&](int k0, bool full) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        cw[u][0] = 0u; cw[u][1] = 0u; cw[u][2] = 0u;
        nv[u] = full ? nvm[u] : (nvm[u] > 0 ? min(8, ke - (k0 + wk[u])) : 0);
        if (nv[u] > 0) {
          if (4 * wq[u] + 12 <= nbytes) {   // all three inside the stream
            const gcu32* q = (const gcu32*)(codes + 4 * wq[u]);
            cw[u][0] = q[0]; cw[u][1] = q[1]; cw[u][2] = q[2];
          } else {                          // the stream's end: nothing past its last byte is read
            cw[u][0] = code_dword(codes, wq[u], nbytes);
            cw[u][1] = code_dword(codes, wq[u] + 1, nbytes);
            cw[u][2] = code_dword(codes, wq[u] + 2, nbytes);
          }
        }
        wq[u] += 2 * BITS;
      }
      if (full && a.xal4) {   // a row of ux from a dword boundary: four dwords
        const gcu32* q = (const gcu32*)xp;
#pragma unroll
        for (int d = 0; d < 4; ++d) rx[d] = cok ? (q[d] ^ 0x80808080u) : 0u;
      } else {
        const ilr_gcu8* xg = (const ilr_gcu8*)xp;
        const int nk = full ? 16 : max(0, min(16, ke - (k0 + xk)));   // bytes of the 16 inside the piece
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          unsigned v = 0u;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (4 * d + j < nk) v |= ((unsigned)xg[4 * d + j] ^ 0x80u) << (8 * j);
          rx[d] = cok ? v : 0u;
        }
      }
      xp += kIlrBK;
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
          b[j] = j < nv[u] ? ((unsigned)v & 255u) : 0u;   // past the piece / the matrix: 0
        }
        const unsigned lo = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        const unsigned hi = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        *reinterpret_cast<uint2*>(&sW[buf][wrow[u] * kIlrLD + wk[u]]) = make_uint2(lo, hi);
      }
      *reinterpret_cast<uint4*>(&sX[buf][xc * kIlrLD + xk]) = make_uint4(rx[0], rx[1], rx[2], rx[3]);
    };

    load(kb, kb + kIlrBK <= ke);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int k0 = kb; k0 < ke; k0 += kIlrBK) {
      const bool more = k0 + kIlrBK < ke;
      if (more) load(k0 + kIlrBK, k0 + 2 * kIlrBK <= ke);
      const unsigned char* w = sW[buf] + (32 * wm + i) * kIlrLD + 16 * h;
      const unsigned char* x = sX[buf] + (32 * wn + i) * kIlrLD + 16 * h;
#pragma unroll
      for (int kk = 0; kk < kIlrBK / 32; ++kk) {
        const ilr_i32x4 av = *reinterpret_cast<const ilr_i32x4*>(w + 32 * kk);
        const ilr_i32x4 bv = *reinterpret_cast<const ilr_i32x4*>(x + 32 * kk);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(bv, av, acc, 0, 0, 0);
      }
      if (more) store(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }

  // lanes along m, registers along the columns: element (c, m) belongs to one lane and one register
  const int m = m0 + 32 * wm + i;
  const bool mok = m < M;
  if (a.parallel && !tail_only) {   // the piece's integer sums as they are
    int* const dst = a.part + (long long)piece * a.total;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const long long c = c0 + 32 * wn + PACKED_ROW(q);
      if (mok && c < C) dst[c * M + m] = acc[q];
    }
    return;
  }

  // The tail q[c, m] = sum_j L_T[m, j] t_T[c, j] in steps of 32 j. Every barrier of the K loop is behind
  // us, so both buffers are free: step s stages into buffer s & 1 and one barrier a step is enough
  // (buffer s & 1 was last read in step s - 2, before step s - 1's barrier).
  {
    const int r = a.r, rp = a.rp, nsd = a.nsd;
    const int trow = tid >> 2, tk = 8 * (tid & 3);   // both images: row of the tile, first j of the step's 8
    const bool lok = m0 + trow < M;
    const bool cok = c0 + trow < C;
    const long long uimg = C * rp;
    const long long lrow = (long long)min(m0 + trow, M - 1) * r;   // (a row past M is never loaded)
    const float* __restrict__ up = a.upart + min(c0 + trow, C - 1) * rp + tk;
    const double g = a.g, mnx = a.mnx;
    unsigned lw[4], tx[4];
    auto tload = [&](int j0) {
      const int nj = max(0, min(8, r - (j0 + tk)));   // j of the 8 inside r
      ilr_factor8<T>(a.L, lrow + (j0 + tk), a.fdt, a.lal != 0, lok ? nj : 0, lw);
      // the 8 j of this column in every image: two 16-byte loads each (the padded row keeps them
      // aligned and inside), kIlrBatch images in flight, added in range order
      const float* ug = up + j0;
      float s[8];
      for (int z0 = 0; z0 < nsd; z0 += kIlrBatch) {
        ilr_f32x4 v[kIlrBatch][2];
#pragma unroll
        for (int b = 0; b < kIlrBatch; ++b) {
          if (z0 + b < nsd) {
            v[b][0] = *(const ilr_gcf32x4*)(ug + (long long)(z0 + b) * uimg);
            v[b][1] = *(const ilr_gcf32x4*)(ug + (long long)(z0 + b) * uimg + 4);
          }
        }
#pragma unroll
        for (int b = 0; b < kIlrBatch; ++b) {
          if (z0 + b < nsd) {
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = (z0 + b == 0) ? v[b][j >> 2][j & 3] : s[j] + v[b][j >> 2][j & 3];
          }
        }
      }
      const ilr_gcf32* rg = (const ilr_gcf32*)(a.rho + (j0 + tk));
      unsigned e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float rj = j < nj ? rg[j] : 0.f;   // (a j past r: U is an exact zero and so is t)
        e[j] = ilr_round_bits<T>(ilr_t32(s[j], rj, g, mnx));
      }
#pragma unroll
      for (int d = 0; d < 4; ++d) tx[d] = cok ? (e[2 * d] | (e[2 * d + 1] << 16)) : 0u;
    };
    unsigned short* const tW0 = reinterpret_cast<unsigned short*>(sW[0]);
    unsigned short* const tW1 = reinterpret_cast<unsigned short*>(sW[1]);
    unsigned short* const tX0 = reinterpret_cast<unsigned short*>(sX[0]);
    unsigned short* const tX1 = reinterpret_cast<unsigned short*>(sX[1]);
    tload(0);
    int buf = 0;
    for (int j0 = 0; j0 < r; j0 += kHgBK) {
      unsigned short* const tw = buf ? tW1 : tW0;
      unsigned short* const txi = buf ? tX1 : tX0;
      hg_u32x4 wv, xv;
#pragma unroll
      for (int d = 0; d < 4; ++d) { wv[d] = lw[d]; xv[d] = tx[d]; }
      *reinterpret_cast<hg_u32x4*>(tw + trow * kHgLD + tk) = wv;
      *reinterpret_cast<hg_u32x4*>(txi + trow * kHgLD + tk) = xv;
      __syncthreads();
      if (j0 + kHgBK < r) tload(j0 + kHgBK);
      const unsigned short* w = tw + (32 * wm + i) * kHgLD + 8 * h;
      const unsigned short* x = txi + (32 * wn + i) * kHgLD + 8 * h;
#pragma unroll
      for (int kk = 0; kk < kHgBK / 16; ++kk) {
        const hg_u32x4 av = *reinterpret_cast<const hg_u32x4*>(w + 16 * kk);
        const hg_u32x4 bv = *reinterpret_cast<const hg_u32x4*>(x + 16 * kk);
        qacc = hg_mfma<T>(bv, av, qacc);
      }
      buf ^= 1;
    }
  }

  if (tail_only) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const long long c = c0 + 32 * wn + PACKED_ROW(q);
      if (mok && c < C) a.qpart[c * M + m] = qacc[q];
    }
    return;
  }
  int cnt = 0;
  {
    const int A = mok ? a.rowsum[m] : 0;
    const bool hb = a.bias != nullptr;
    const float bv = (mok && hb) ? a.bias[m] : 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const long long c = c0 + 32 * wn + PACKED_ROW(q);
      if (!mok || c >= C) continue;
      ilr_out<OUT>(a, c * M + m, ilr_value(acc[q], A, qacc[q], a, hb, bv), cnt);
    }
  }
  if constexpr (OUT == kIlrCodes) {
    if (a.clamped) ilr_count(cnt, a.clamped);   // (uniform; every thread arrives: no return above in the serial regime)
  }
}

// The parallel regime's last kernel: S = sum of the piece images (integers: any order), q's image, the epilogue
__global__ __launch_bounds__(256) void k_packed_ilrreduce(const IlrArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  int cnt = 0;
  if (e < a.total) {
    int s = a.part[e];
    for (int p = 1; p < a.np; ++p) s += a.part[(long long)p * a.total + e];
    const int m = (int)(e % a.M);
    const bool hb = a.bias != nullptr;
    const float v = ilr_value(s, a.rowsum[m], a.qpart[e], a, hb, hb ? a.bias[m] : 0.f);
    if (a.out == kIlrCodes) ilr_out<kIlrCodes>(a, e, v, cnt);
    else if (a.out == kIlrQuant) ilr_out<kIlrQuant>(a, e, v, cnt);
    else ilr_out<kIlrFloat>(a, e, v, cnt);
  }
  if (a.out == kIlrCodes && a.clamped) ilr_count(cnt, a.clamped);
}

// The clamp counter's reset on the stream: a kernel, so that a captured graph holds no memset node
__global__ void k_ilr_zero(int* counter) {
  if (threadIdx.x == 0) *counter = 0;
}

// --- host side ------------------------------------------------------------------------------------

// The plan of one call, a function of (M, K, N, r) alone, and the workspace's layout:
// [np int32 images of S][one float32 image of q] (parallel regime only) [pad to 16 bytes][nsd N rp floats of U].
// g is admmq_packed_igemm's plan of (M, K, N, nb = 1). The down-projection's split: enough ranges for
// one workgroup a CU over its ceil(r / 64) ceil(N / 64) tiles, kIlrSplitMax at most, each a multiple
// of its K step and kIlrRangeMin k at least (admmq_packed_hlrgemm's rule).
struct IlrPlan {
  PackedPlan g;
  int ksd, nsd, rp, launches;
  size_t qoff, uoff, ws;   // bytes to q's image and to U; in all
};

static bool plan_ilr(int64_t M, int64_t K, int64_t N, int64_t r, IlrPlan& pl) {
  if (r < 1 || r > kIlrRankMax) return false;
  if (!plan_packed(M, K, N, 1, kIlrBK, kIlrKMax, sizeof(int32_t), pl.g)) return false;
  const int64_t tiles = ((r + kPackedBM - 1) / kPackedBM) * ((N + kPackedBN - 1) / kPackedBN);
  const int64_t want = std::min<int64_t>({(kIlrOneLaunch + tiles - 1) / tiles, (int64_t)kIlrSplitMax,
                                          (K + kIlrRangeMin - 1) / kIlrRangeMin});
  const int64_t ks = kHgBK * ((((K + want - 1) / want) + kHgBK - 1) / kHgBK);
  pl.ksd = (int)ks;
  pl.nsd = (int)((K + ks - 1) / ks);
  pl.rp = (int)(32 * ((r + 31) / 32));
  pl.launches = pl.g.parallel ? 3 : 2;
  pl.qoff = pl.g.parallel ? (size_t)pl.g.np * (size_t)pl.g.total * sizeof(int32_t) : 0;
  pl.uoff = ((pl.g.parallel ? pl.qoff + (size_t)pl.g.total * sizeof(float) : 0) + 15) & ~(size_t)15;
  pl.ws = pl.uoff + (size_t)pl.nsd * (size_t)N * (size_t)pl.rp * sizeof(float);
  return true;
}

static bool ilr_act_bits_ok(const admmq_actq* q) { return q && q->on != 0 && q->bits >= 2 && q->bits <= 8; }
static bool ilr_half(int32_t dt) { return dt == ADMMQ_DT_BF16 || dt == ADMMQ_DT_F16; }

// 8 consecutive elements of a row of a [rows, n] factor from a multiple of 8: aligned 16-byte loads that never straddle the row's end
static int ilr_rows_aligned(const void* p, int64_t n) {
  return ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && n % 8 == 0) ? 1 : 0;
}

// The checks that the factor sums and the GEMM share
static int32_t ilr_factor_check(const char* who, int32_t f_dtype, int32_t t_dtype, int64_t r) {
  if (!ilr_half(t_dtype)) return packed_fail(who, ADMMQ_ERR_ARG, "t_dtype must be ADMMQ_DT_BF16 or ADMMQ_DT_F16");
  if (f_dtype != ADMMQ_DT_F32 && f_dtype != t_dtype) return packed_fail(who, ADMMQ_ERR_ARG, "f_dtype must be ADMMQ_DT_F32 or t_dtype");
  if (r < 1 || r > kIlrRankMax) return packed_fail(who, ADMMQ_ERR_ARG, "rank r must be 1..256");
  return ADMMQ_OK;
}

template <typename T, int OUT>
static void ilr_launch(const IlrArgs& a, int bits, dim3 grid, hipStream_t s) {
#define ADMMQ_ILR_BITS(B) hipLaunchKernelGGL((k_packed_ilrgemm<B, T, OUT>), grid, dim3(256), 0, s, a)
  PACKED_BITS_SWITCH(bits, ADMMQ_ILR_BITS)
#undef ADMMQ_ILR_BITS
}

template <typename T>
static void ilr_launch_out(const IlrArgs& a, int bits, int kout, dim3 grid, hipStream_t s) {
  if (kout == kIlrCodes) ilr_launch<T, kIlrCodes>(a, bits, grid, s);
  else if (kout == kIlrQuant) ilr_launch<T, kIlrQuant>(a, bits, grid, s);
  else ilr_launch<T, kIlrFloat>(a, bits, grid, s);
}

}  // namespace admmq

using namespace admmq;

extern "C" {

int32_t admmq_packed_lowrank_factorsums(const void* Rt, int32_t f_dtype, int32_t t_dtype, int32_t r, int64_t K, float* rho,
                                        void* stream) {
  const char* const who = "packed_lowrank_factorsums";
  if (!Rt || !rho) return packed_fail(who, ADMMQ_ERR_ARG, "Rt and rho must not be NULL");
  const int32_t rc = ilr_factor_check(who, f_dtype, t_dtype, r);
  if (rc != ADMMQ_OK) return rc;
  if (K <= 0 || K > kIlrKMax) return packed_fail(who, ADMMQ_ERR_ARG, "K must be 1..65536");
  if ((reinterpret_cast<uintptr_t>(Rt) & (f_dtype == ADMMQ_DT_F32 ? 3 : 1)) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "Rt must be aligned to its element");
  if ((reinterpret_cast<uintptr_t>(rho) & 3) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "rho must be float aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((r + 3) / 4));
  if (t_dtype == ADMMQ_DT_BF16) hipLaunchKernelGGL((k_ilr_factorsums<__bf16>), grid, dim3(256), 0, s, Rt, (int)f_dtype, (int)r, (int)K, rho);
  else hipLaunchKernelGGL((k_ilr_factorsums<_Float16>), grid, dim3(256), 0, s, Rt, (int)f_dtype, (int)r, (int)K, rho);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

size_t admmq_packed_ilrgemm_workspace_size(int64_t M, int64_t K, int64_t N, int32_t r) {
  IlrPlan pl;
  return plan_ilr(M, K, N, r, pl) ? pl.ws : 0;
}

int32_t admmq_packed_ilrgemm_plan(int64_t M, int64_t K, int64_t N, int32_t r, int32_t out[4]) {
  IlrPlan pl;
  if (!out || !plan_ilr(M, K, N, r, pl))
    return packed_fail("packed_ilrgemm_plan", ADMMQ_ERR_ARG, "NULL out or arguments out of range");
  out[0] = pl.g.np; out[1] = pl.g.parallel; out[2] = pl.nsd; out[3] = pl.launches;
  return ADMMQ_OK;
}

int32_t admmq_packed_ilrgemm(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const void* L,
                             const void* Rt, int32_t f_dtype, int32_t t_dtype, int32_t r, const float* rho,
                             const uint8_t* x, const admmq_actq* x_q, const int32_t* rowsums, int64_t N, const float* bias,
                             float* y, uint8_t* y_codes, const admmq_actq* out_q, int32_t* clamped, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const char* const who = "packed_ilrgemm";
  if (!codes || !x || !meta || !rowsums || !x_q)
    return packed_fail(who, ADMMQ_ERR_ARG, "codes, meta, x, x_q and rowsums must not be NULL");
  if (!L || !Rt) return packed_fail(who, ADMMQ_ERR_ARG, "L and Rt must not be NULL");
  if (!rho) return packed_fail(who, ADMMQ_ERR_ARG, "rho must not be NULL (admmq_packed_lowrank_factorsums writes it)");
  if ((y == nullptr) == (y_codes == nullptr)) return packed_fail(who, ADMMQ_ERR_ARG, "exactly one of y and y_codes must be given");
  if (M <= 0 || K <= 0 || N <= 0) return packed_fail(who, ADMMQ_ERR_ARG, "M, K and N must be positive");
  int32_t rc = ilr_factor_check(who, f_dtype, t_dtype, r);
  if (rc != ADMMQ_OK) return rc;
  int off = 0;
  rc = packed_meta_check(meta, who, true, &off);
  if (rc != ADMMQ_OK) return rc;
  if (K > kIlrKMax) return packed_fail(who, ADMMQ_ERR_ARG, "K must be at most 65536 (the int32 sum 128 * 255 * K)");
  if (!ilr_act_bits_ok(x_q)) return packed_fail(who, ADMMQ_ERR_ARG, "x_q must be on with bits 2..8");
  const bool oq = out_q && out_q->on != 0;
  if (y_codes && !ilr_act_bits_ok(out_q)) return packed_fail(who, ADMMQ_ERR_ARG, "a codes output needs out_q on with bits 2..8");
  if (y && oq && (out_q->bits < 1 || out_q->bits > 24)) return packed_fail(who, ADMMQ_ERR_ARG, "out_q bits must be 1..24");
  if ((reinterpret_cast<uintptr_t>(codes) & 15) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "codes must be 16-byte aligned");
  if (((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(rowsums) |
        reinterpret_cast<uintptr_t>(clamped) | reinterpret_cast<uintptr_t>(rho)) & 3) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "y, bias, rowsums, rho and clamped must be 4-byte aligned");
  if (((reinterpret_cast<uintptr_t>(L) | reinterpret_cast<uintptr_t>(Rt)) & (f_dtype == ADMMQ_DT_F32 ? 3 : 1)) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "L and Rt must be aligned to their element");
  IlrPlan pl;
  if (!plan_ilr(M, K, N, r, pl)) return packed_fail(who, ADMMQ_ERR_ARG, "sizes out of range");
  if (!workspace || workspace_bytes < pl.ws) return set_error(ADMMQ_ERR_WORKSPACE, "packed_ilrgemm: workspace too small");
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "workspace must be 16-byte aligned");

  IlrArgs a;
  char* const wsb = static_cast<char*>(workspace);
  a.codes = codes; a.x = x; a.bias = bias; a.rowsum = rowsums; a.y = y; a.yc = y_codes;
  a.part = pl.g.parallel ? reinterpret_cast<int*>(wsb) : nullptr;
  a.qpart = pl.g.parallel ? reinterpret_cast<float*>(wsb + pl.qoff) : nullptr;
  a.clamped = y_codes ? clamped : nullptr;
  a.L = L; a.Rt = Rt; a.rho = rho;
  a.upart = reinterpret_cast<float*>(wsb + pl.uoff);
  a.nbytes = (long long)admmq_packed_bytes(M * K, meta->bits);
  a.total = pl.g.total; a.C = pl.g.C;
  a.M = (int)M; a.K = (int)K;
  a.kp = pl.g.kp; a.np = pl.g.np; a.parallel = pl.g.parallel;
  a.off = off;
  a.xal4 = ((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (K & 3) == 0) ? 1 : 0;
  a.xal8 = ((reinterpret_cast<uintptr_t>(x) & 7) == 0 && (K & 7) == 0) ? 1 : 0;
  a.out = y_codes ? kIlrCodes : (oq ? kIlrQuant : kIlrFloat);
  a.r = r; a.rp = pl.rp; a.ksd = pl.ksd; a.nsd = pl.nsd; a.fdt = f_dtype;
  a.lal = ilr_rows_aligned(L, r);
  a.ral = ilr_rows_aligned(Rt, K);
  a.s = (double)meta->scale;
  a.g = (double)x_q->rng / (double)((1 << x_q->bits) - 1);
  a.mnx = (double)x_q->mn;
  a.oq = oq ? actq_make(out_q) : ActQ{0.f, 0.f, 0.f, 0};

  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool bf = t_dtype == ADMMQ_DT_BF16;
  if (a.clamped) hipLaunchKernelGGL(k_ilr_zero, dim3(1), dim3(64), 0, s, a.clamped);
  const dim3 dgrid((unsigned)pl.g.tiles_c, (unsigned)((r + kPackedBM - 1) / kPackedBM), (unsigned)pl.nsd);
  if (bf) hipLaunchKernelGGL((k_ilr_down<__bf16>), dgrid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_ilr_down<_Float16>), dgrid, dim3(256), 0, s, a);
  const dim3 grid((unsigned)pl.g.tiles_c, (unsigned)pl.g.tiles_m, pl.g.parallel ? (unsigned)pl.g.np + 1u : 1u);
  const int kout = pl.g.parallel ? kIlrFloat : a.out;   // the parallel regime's epilogue runs in k_packed_ilrreduce
  if (bf) ilr_launch_out<__bf16>(a, meta->bits, kout, grid, s);
  else ilr_launch_out<_Float16>(a, meta->bits, kout, grid, s);
  if (pl.g.parallel)
    hipLaunchKernelGGL(k_packed_ilrreduce, dim3((unsigned)((pl.g.total + 255) / 256)), dim3(256), 0, s, a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

}  // extern "C"
