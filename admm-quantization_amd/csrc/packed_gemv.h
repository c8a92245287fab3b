// What the skinny kernels of packed_gemv.hip and packed_lrgemv.hip share: the
// launch record, the x image, the code cut, the fixed lane tree, the W = D kernel k_packed_gemv - with the
// low-rank tail as a compile-time flag - and the planner of the K split.
#pragma once
#include <algorithm>
#include <type_traits>

#include "../../include/admmq.h"
#include "packed_tile.h"

namespace admmq {

constexpr int kGvR = 4;                      // rows of a lane
constexpr int kGvLK = 32;                    // lanes along k
constexpr int kGvRun = 32;                   // codes of a lane's run
constexpr int kGvCh = kGvLK * kGvRun;        // k per chunk: 1024
constexpr int kGvPad = kGvRun + 4;           // LDS floats per run: 36 dwords apart, 16-byte reads without bank conflicts
constexpr int kGvRows = 4 * 2 * kGvR;        // rows per workgroup: 32
constexpr int kGtJ = 4;                      // m of a lane (trans_w = 1)
constexpr int kGtTile = 64 * kGtJ;           // m per workgroup: 256
constexpr int kGtCh = 512;                   // k per chunk, a quarter a wave
constexpr int kGtMinK = 128;                 // k per range at least (trans_w = 1)
constexpr int kGvSplitMax = 16;              // ranges at most
constexpr int kGvFill = 512;                 // workgroups the planner aims at
constexpr int kGvOneLaunch = 256;            // tiles from which one launch fills the chip (one per CU)
constexpr int64_t kGvKMax = int64_t(1) << 24;
constexpr int kGvRankMax = 256;              // rank of the low-rank tail at most

typedef unsigned gv_u32x4 __attribute__((ext_vector_type(4)));

struct GvArgs {
  const unsigned char* codes;
  const void* x;
  const float* bias;
  void* y;
  float* part;        // split form: [ns][N][M] float32 partial sums
  float* xpart;       // split form, tensor_minmax: [ns][N] partial sums of x
  long long nbytes;   // bytes of the code stream
  int M, K, N;
  int ks, ns;         // k per range, ranges
  int scheme;
  int off;            // the operand is u - off (q + zp; 0 for tensor_minmax)
  int xdt, ydt;       // ADMMQ_DT_*
  int xal;            // every row of x starts on a 16-byte boundary and holds whole 16-byte groups
  float scale, mn, rng, nlev;   // nlev = float(2^bits - 1)
};

// The low-rank tail q[c, m] = sum_j L[m, j] t[c, j] of k_packed_gemv<BITS, NB, true> (k_packed_lrgemv). In its split
// form the tail is slice ns of gridDim.z and q is image ns of GvArgs::part.
struct GvLr {
  const void* L;        // [M, r] row-major, float32 or a 16-bit type
  const float* tpart;   // [nsd][N][r] float32: the ranges' images of t = x Rt^T, added in range order
  int r, rp;            // the rank, and r rounded up to a multiple of 32
  int nsd;              // images of t
  int fdt;              // ADMMQ_DT_* of L
};
struct GvNoLr {};       // what k_packed_gemv takes in GvLr's place without the tail

// The float32 result of one output: the sums' epilogue, operations rounded one by one
__device__ __forceinline__ float gv_value(float S, float Sx, const GvArgs& a, bool has_bias, float bv) {
  float v;
  if (a.scheme == kMinMax) v = (S * a.rng) / a.nlev + a.mn * Sx;
  else v = S * a.scale;
  return has_bias ? v + bv : v;
}

__device__ __forceinline__ void gv_store(void* y, long long e, float v, int ydt) {
  if (ydt == ADMMQ_DT_F32) static_cast<float*>(y)[e] = v;
  else if (ydt == ADMMQ_DT_BF16) static_cast<__bf16*>(y)[e] = static_cast<__bf16>(v);
  else static_cast<_Float16*>(y)[e] = static_cast<_Float16>(v);
}

// Element e of x widened to float32 (exact)
__device__ __forceinline__ float gv_widen(const void* x, long long e, int xdt) {
  if (xdt == ADMMQ_DT_F32) return static_cast<const float*>(x)[e];
  const unsigned h = static_cast<const unsigned short*>(x)[e];
  if (xdt == ADMMQ_DT_BF16) return __uint_as_float(h << 16);
  return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
}
__device__ __forceinline__ float gv_half_bits(unsigned h, int xdt) {
  if (xdt == ADMMQ_DT_BF16) return __uint_as_float(h << 16);
  return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
}

// The workgroup's x image of one chunk: xs[c * CS + pos(kk)] = x[c, k0 + kk] as float32 for kk < CH,
// exactly 0 for k >= ke and for c >= N. RUN consecutive k lie PAD floats apart (RUN = PAD: dense).
// Rows of x on 16-byte boundaries are read 16 bytes a thread, else element by element.
template <int NB, int CH, int RUN, int PAD>
__device__ __forceinline__ void gv_stage(const GvArgs& a, float* xs, int k0, int ke) {
  constexpr int CS = CH / RUN * PAD;
  const int K = a.K, N = a.N, xdt = a.xdt;
  auto pos = [](int kk) { return (kk / RUN) * PAD + (kk % RUN); };
  if (a.xal) {
    const int epv = xdt == ADMMQ_DT_F32 ? 4 : 8;   // elements of 16 bytes (K, k0, ke - or K at the end - are multiples)
    const int gpc = CH / epv;
#pragma unroll 2
    for (int g = threadIdx.x; g < NB * gpc; g += 256) {
      const int c = g / gpc, kk = (g - c * gpc) * epv;
      const int k = k0 + kk;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (c < N && k < ke) {
        const gv_u32x4 q = *reinterpret_cast<const gv_u32x4*>(static_cast<const unsigned char*>(a.x) +
                                                              ((long long)c * K + k) * (xdt == ADMMQ_DT_F32 ? 4 : 2));
        if (xdt == ADMMQ_DT_F32) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(q[j]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[2 * j] = gv_half_bits(q[j] & 0xFFFFu, xdt);
            v[2 * j + 1] = gv_half_bits(q[j] >> 16, xdt);
          }
        }
      }
      float* d = xs + c * CS + pos(kk);   // (epv divides RUN: the group stays inside one run)
      *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
      if (epv == 8) *reinterpret_cast<float4*>(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
  } else {
#pragma unroll 4
    for (int e = threadIdx.x; e < NB * CH; e += 256) {
      const int c = e / CH, kk = e - c * CH;
      const int k = k0 + kk;
      xs[c * CS + pos(kk)] = (c < N && k < ke) ? gv_widen(a.x, (long long)c * K + k, xdt) : 0.f;
    }
  }
}

// Code j of a run of aligned dwords d (compile-time j)
template <int BITS, int ND>
__device__ __forceinline__ unsigned gv_code(const unsigned (&d)[ND], int j) {
  constexpr unsigned mask = (1u << BITS) - 1u;
  const int bit = j * BITS, w = bit >> 5, o = bit & 31;
  if (o + BITS <= 32) return (d[w] >> o) & mask;
  return __builtin_amdgcn_alignbit(d[w + 1 < ND ? w + 1 : w], d[w], o) & mask;
}

template <int CTRL>
__device__ __forceinline__ float gv_dpp(float v) {
  return __uint_as_float(dpp_zero<CTRL>(__float_as_uint(v)));
}
// the sum of each 16-lane DPP row in its lane 15, a fixed tree
__device__ __forceinline__ float gv_row_sum(float v) {
  v = v + gv_dpp<0x111>(v);
  v = v + gv_dpp<0x112>(v);
  v = v + gv_dpp<0x114>(v);
  v = v + gv_dpp<0x118>(v);
  return v;
}

// One output of a workgroup: the range's partial sum (split form) or the epilogue's value
__device__ __forceinline__ void gv_emit(const GvArgs& a, int c, int m, float S, float Sx, bool first_tile_row) {
  if (a.ns > 1) {
    const long long z = blockIdx.z;
    a.part[(z * a.N + c) * a.M + m] = S;
    if (a.scheme == kMinMax && first_tile_row) a.xpart[z * a.N + c] = Sx;
  } else {
    gv_store(a.y, (long long)c * a.M + m, gv_value(S, Sx, a, a.bias != nullptr, a.bias ? a.bias[m] : 0.f), a.ydt);
  }
}

// ... with the tail: y = (v + q) + bias in one launch; in the split form slice ns of gridDim.z writes q as
// image ns and the other slices their partial sums
__device__ __forceinline__ void gv_emit_lr(const GvArgs& a, int c, int m, float S, float Sx, float Q, bool first_tile_row) {
  if (a.ns > 1) {
    if ((int)blockIdx.z == a.ns) a.part[((long long)a.ns * a.N + c) * a.M + m] = Q;
    else gv_emit(a, c, m, S, Sx, first_tile_row);
  } else {
    float v = gv_value(S, Sx, a, false, 0.f) + Q;
    if (a.bias) v = v + a.bias[m];
    gv_store(a.y, (long long)c * a.M + m, v, a.ydt);
  }
}

// k_packed_gemv (LR false: lr is empty) and k_packed_lrgemv (LR true): W = D, a row's codes run
// along k. A workgroup of four waves owns 32 rows, a wave's two halves of 32 lanes four rows each (see
// packed_gemv.hip). The tail runs behind the code chunks in the same lanes: t is staged over the x image as
// [NB][rp] (the nsd images added in range order, zeros past r and past N), the 32 lanes of a row take
// j = l, l + 32, ... of L[m, :] in increasing j from zero, and q meets in the tree of the code sum.
template <int BITS, int NB, bool LR = false>
__global__ __launch_bounds__(256) void k_packed_gemv(const GvArgs a, const std::conditional_t<LR, GvLr, GvNoLr> lr) {
  constexpr int CS = kGvLK * kGvPad;        // floats of a column's image
  constexpr int QO = kGvR * NB + NB;        // where a 16-lane row's sums of q start
  constexpr int RS = QO + (LR ? kGvR * NB : 0);   // floats of a 16-lane row's sums: [r][c], the sums of x, q [r][c]
  __shared__ __attribute__((aligned(16))) float xs[NB * CS];
  __shared__ float red[16 * RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = lane >> 5, kl = lane & 31;
  const int M = a.M, K = a.K;
  const int kb = (int)blockIdx.z * a.ks, ke = min(K, kb + a.ks);   // (the tail's slice: kb >= K, no chunk)
  const unsigned char* __restrict__ codes = a.codes;
  const long long nbytes = a.nbytes;
  const bool mm = a.scheme == kMinMax;   // (uniform)
  const int off = a.off;

  // the lane's rows (past M: the last row, computed and never stored) and their runs' place in the stream
  const int mrow = (int)blockIdx.x * kGvRows + (2 * wave + grp) * kGvR;
  long long wq[kGvR];
  int sh[kGvR];
#pragma unroll
  for (int r = 0; r < kGvR; ++r) {
    const long long bit0 = ((long long)min(mrow + r, M - 1) * K + (kb + kGvRun * kl)) * BITS;
    wq[r] = bit0 >> 5;
    sh[r] = (int)(bit0 & 31);   // the same at every chunk: a chunk is 32 BITS whole dwords further
  }
  float acc[kGvR][NB], sx[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    sx[c] = 0.f;
#pragma unroll
    for (int r = 0; r < kGvR; ++r) acc[r][c] = 0.f;
  }

  for (int k0 = kb; k0 < ke; k0 += kGvCh) {
    const bool on = k0 + kGvRun * kl < ke;   // the run holds a k of the range
    unsigned w[kGvR][BITS + 1];
    if (on) {
#pragma unroll
      for (int r = 0; r < kGvR; ++r) {
        if (4 * (wq[r] + BITS + 1) <= nbytes) {   // all inside the stream: plain loads, issued together
          const gcu32* q = (const gcu32*)(codes + 4 * wq[r]);
#pragma unroll
          for (int i = 0; i <= BITS; ++i) w[r][i] = q[i];
        } else {                                  // the stream's end: nothing past its last byte is read
#pragma unroll
          for (int i = 0; i <= BITS; ++i) w[r][i] = code_dword(codes, wq[r] + i, nbytes);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kGvR; ++r) wq[r] += (long long)kGvLK * BITS;
    __syncthreads();   // the last chunk's image has been read
    gv_stage<NB, kGvCh, kGvRun, kGvPad>(a, xs, k0, ke);
    __syncthreads();
    if (on) {
      unsigned d[kGvR][BITS];
#pragma unroll
      for (int r = 0; r < kGvR; ++r)
#pragma unroll
        for (int i = 0; i < BITS; ++i) d[r][i] = __builtin_amdgcn_alignbit(w[r][i + 1], w[r][i], sh[r]);
      const float* xl = xs + kl * kGvPad;
      if (mm) {   // the sums of x, in the order of the FMAs below (a pass of its own: no branch among those)
#pragma unroll
        for (int j4 = 0; j4 < kGvRun / 4; ++j4)
#pragma unroll
          for (int c = 0; c < NB; ++c) {
            const float4 v = *reinterpret_cast<const float4*>(xl + c * CS + 4 * j4);
            sx[c] = (((sx[c] + v.x) + v.y) + v.z) + v.w;
          }
      }
#pragma unroll
      for (int j4 = 0; j4 < kGvRun / 4; ++j4) {
        float xv[NB][4];
#pragma unroll
        for (int c = 0; c < NB; ++c) {
          const float4 v = *reinterpret_cast<const float4*>(xl + c * CS + 4 * j4);
          xv[c][0] = v.x; xv[c][1] = v.y; xv[c][2] = v.z; xv[c][3] = v.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int r = 0; r < kGvR; ++r) {
            const float af = (float)((int)gv_code<BITS, BITS>(d[r], 4 * j4 + j) - off);
#pragma unroll
            for (int c = 0; c < NB; ++c) acc[r][c] = __builtin_fmaf(af, xv[c][j], acc[r][c]);
          }
        }
        // keep the next groups' LDS reads behind this group's FMAs: hoisted, the eight groups' x
        // values of NB = 8 cost 256 registers
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  float q[LR ? kGvR : 1][LR ? NB : 1];
  if constexpr (LR) {
#pragma unroll
    for (int c = 0; c < NB; ++c)
#pragma unroll
      for (int r = 0; r < kGvR; ++r) q[r][c] = 0.f;
    if (a.ns == 1 || (int)blockIdx.z == a.ns) {   // (uniform)
      const int rk = lr.r, rp = lr.rp, N = a.N;
      __syncthreads();   // the last chunk's image has been read
      for (int e = tid; e < NB * rp; e += 256) {
        const int c = e / rp, j = e - c * rp;
        float v = 0.f;
        if (c < N && j < rk) {
          v = lr.tpart[c * rk + j];
          for (int z = 1; z < lr.nsd; ++z) v = v + lr.tpart[((long long)z * N + c) * rk + j];
        }
        xs[e] = v;
      }
      __syncthreads();
      long long lrow[kGvR];
#pragma unroll
      for (int r = 0; r < kGvR; ++r) lrow[r] = (long long)min(mrow + r, M - 1) * rk;
      for (int j = kl; j < rp; j += 32) {
        float lv[kGvR];
#pragma unroll
        for (int r = 0; r < kGvR; ++r) lv[r] = j < rk ? gv_widen(lr.L, lrow[r] + j, lr.fdt) : 0.f;   // (t is 0 there)
#pragma unroll
        for (int c = 0; c < NB; ++c) {
          const float tv = xs[c * rp + j];
#pragma unroll
          for (int r = 0; r < kGvR; ++r) q[r][c] = __builtin_fmaf(lv[r], tv, q[r][c]);
        }
      }
    }
  }

  // the 32 lanes of a row: a tree inside each 16-lane DPP row, then the two row sums, lower k first
  const int row16 = 4 * wave + (lane >> 4);
#pragma unroll
  for (int c = 0; c < NB; ++c) {
#pragma unroll
    for (int r = 0; r < kGvR; ++r) {
      const float v = gv_row_sum(acc[r][c]);
      if ((lane & 15) == 15) red[row16 * RS + r * NB + c] = v;
      if constexpr (LR) {
        const float u = gv_row_sum(q[r][c]);
        if ((lane & 15) == 15) red[row16 * RS + QO + r * NB + c] = u;
      }
    }
    if (mm) {
      const float v = gv_row_sum(sx[c]);
      if ((lane & 15) == 15) red[row16 * RS + kGvR * NB + c] = v;
    }
  }
  __syncthreads();
  if (tid < kGvRows * NB) {
    const int c = tid / kGvRows, rr = tid - c * kGvRows;   // consecutive threads: consecutive m
    const int lg = rr / kGvR, r = rr - lg * kGvR;          // the lane group 2 wave + grp and its row
    const int m = (int)blockIdx.x * kGvRows + rr;
    if (m < M && c < a.N) {
      const float* p0 = red + (2 * lg) * RS;
      const float* p1 = p0 + RS;
      const float S = p0[r * NB + c] + p1[r * NB + c];
      const float Sx = mm ? p0[kGvR * NB + c] + p1[kGvR * NB + c] : 0.f;
      if constexpr (LR) gv_emit_lr(a, c, m, S, Sx, p0[QO + r * NB + c] + p1[QO + r * NB + c], blockIdx.x == 0 && rr == 0);
      else gv_emit(a, c, m, S, Sx, blockIdx.x == 0 && rr == 0);
    }
  }
}

// --- host side ------------------------------------------------------------------------------------

// The plan of one call. The ranges are a function of M, K and trans_w alone (N only sizes the
// workspace): one launch where the tiles fill the chip or K is one range's minimum, else
// enough ranges for kGvFill workgroups, kGvSplitMax at most, each a multiple of the minimum.
struct GvPlan {
  int ks, ns;
  long long tiles;
  size_t ws;
};

inline bool plan_gv(const ::admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K, int64_t N, GvPlan& pl) {
  if (!meta || (trans_w != 0 && trans_w != 1) || M <= 0 || K <= 0 || N < 1 || N > ADMMQ_GEMV_N_MAX) return false;
  if (M > (int64_t(1) << 22) || K > kGvKMax || M * K >= (int64_t(1) << 40)) return false;   // admmq_packed_gemm's limits
  const int64_t tile = trans_w ? kGtTile : kGvRows, kmin = trans_w ? kGtMinK : kGvCh;
  pl.tiles = (M + tile - 1) / tile;
  int64_t want = 1;
  if (pl.tiles < kGvOneLaunch)
    want = std::min<int64_t>({(kGvFill + pl.tiles - 1) / pl.tiles, (int64_t)kGvSplitMax, (K + kmin - 1) / kmin});
  const int64_t ks = kmin * ((((K + want - 1) / want) + kmin - 1) / kmin);
  pl.ks = (int)ks;
  pl.ns = (int)((K + ks - 1) / ks);
  pl.ws = 0;
  if (pl.ns > 1)
    pl.ws = (size_t)pl.ns * (size_t)N * ((size_t)M + (meta->scheme == kMinMax ? 1 : 0)) * sizeof(float);
  return true;
}

inline size_t gv_dt_bytes(int32_t dt) { return dt == ADMMQ_DT_F32 ? 4 : 2; }

}  // namespace admmq
