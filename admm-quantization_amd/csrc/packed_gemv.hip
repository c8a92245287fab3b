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
//   k_packed_gemv   (W = D, a row's codes run along k). A workgroup of four waves owns 32 rows:
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

template <int BITS, int NB>
__global__ __launch_bounds__(256) void k_packed_gemv(const GvArgs a) {
  constexpr int CS = kGvLK * kGvPad;        // floats of a column's image
  constexpr int RS = kGvR * NB + NB;        // floats of a 16-lane row's sums: [r][c] and the sums of x
  __shared__ __attribute__((aligned(16))) float xs[NB * CS];
  __shared__ float red[16 * RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = lane >> 5, kl = lane & 31;
  const int M = a.M, K = a.K;
  const int kb = (int)blockIdx.z * a.ks, ke = min(K, kb + a.ks);
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

  // the 32 lanes of a row: a tree inside each 16-lane DPP row, then the two row sums, lower k first
  const int row16 = 4 * wave + (lane >> 4);
#pragma unroll
  for (int c = 0; c < NB; ++c) {
#pragma unroll
    for (int r = 0; r < kGvR; ++r) {
      const float v = gv_row_sum(acc[r][c]);
      if ((lane & 15) == 15) red[row16 * RS + r * NB + c] = v;
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
      gv_emit(a, c, m, S, Sx, blockIdx.x == 0 && rr == 0);
    }
  }
}

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

// The plan of one call. The ranges are a function of M, K and trans_w alone (N only sizes the
// workspace): one launch where the tiles fill the chip or K is one range's minimum, else
// enough ranges for kGvFill workgroups, kGvSplitMax at most, each a multiple of the minimum.
struct GvPlan {
  int ks, ns;
  long long tiles;
  size_t ws;
};

static bool plan_gv(const ::admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K, int64_t N, GvPlan& pl) {
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

static size_t gv_dt_bytes(int32_t dt) { return dt == ADMMQ_DT_F32 ? 4 : 2; }

template <int BITS, int NB>
static void gv_launch(const GvArgs& a, int32_t trans_w, dim3 grid, hipStream_t s) {
  if (trans_w) hipLaunchKernelGGL((k_packed_gemv_t<BITS, NB>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_packed_gemv<BITS, NB>), grid, dim3(256), 0, s, a);
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
