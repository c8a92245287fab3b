// What the skinny integer kernels of packed_igemv.hip and packed_ilrgemv.hip share (DESIGN.md 2.36,
// 2.38): the launch record, the staged ux image, the weight's byte lanes, the
// contract's value and output forms, the clamp count and the planner of the K split.
#pragma once
#include <algorithm>

#include "../../include/admmq.h"
#include "packed_tile.h"

namespace admmq {

constexpr int kIvR = 4;                      // rows of a lane (W = D)
constexpr int kIvLK = 32;                    // lanes along k
constexpr int kIvRun = 32;                   // codes of a lane's run
constexpr int kIvCh = kIvLK * kIvRun;        // k per chunk: 1024
constexpr int kIvPad = 48;                   // LDS bytes per run: 3 slots of 16 bytes apart
constexpr int kIvRows = 4 * 2 * kIvR;        // rows per workgroup: 32
constexpr int kItJ = 4;                      // m of a lane (W = D^T)
constexpr int kItTile = 64 * kItJ;           // m per workgroup: 256
constexpr int kItCh = 256;                   // k per chunk, a quarter a wave
constexpr int kIvSplitMax = 64;              // ranges at most
constexpr int kIvFill = 512;                 // workgroups the planner aims at (two per CU)
constexpr int kIvOneLaunch = 256;            // tiles from which one launch fills the chip
constexpr int kIvRangeBytes = 16384;         // code bytes of a full tile's range at least
constexpr int kIvOneLaunchK = 4 * kIvCh;     // W = D: K up to which one workgroup walks all of K (four chunks)
constexpr int64_t kIvKMax = 65536;           // 255 * 255 * K < 2^32

constexpr int kIvFloat = 0, kIvQuant = 1, kIvCodes = 2;

typedef unsigned iv_u32x4 __attribute__((ext_vector_type(4)));

struct IvArgs {
  const unsigned char* codes;
  const unsigned char* x;
  const float* bias;
  const int* rowsum;
  float* y;
  unsigned char* yc;
  unsigned* part;     // split form: [ns][N][M] uint32 partial sums U
  unsigned* xpart;    // split form: [ns][N] partial sums Sx
  int* clamped;       // codes output: the clamp counter, or NULL
  long long nbytes;   // bytes of the code stream
  int M, K, N;
  int ks, ns;         // k per range, ranges
  int off;            // q + zp: a = u - off
  int xal;            // every row of x starts on a 16-byte boundary and holds whole 16-byte groups
  int out;            // kIvFloat, kIvQuant, kIvCodes
  double s, g, mnx;   // the weight's scale, rng_x / n_x, mn_x
  ActQ oq;
};

// The contract's value (ig_value's sequence, packed_igemm.hip): S is exact in int64 and in double; the
// double operations are rounded one by one (-ffp-contract=off, and the pragma for a build without it).
__device__ __forceinline__ float iv_value(unsigned U, unsigned Sx, int A, const IvArgs& a, bool has_bias, float bv) {
#pragma clang fp contract(off)
  const double S = (double)((long long)U - (long long)a.off * (long long)Sx);
  double v = a.s * (a.g * S + a.mnx * (double)A);
  if (has_bias) v = v + (double)bv;
  return (float)v;
}

// act_code of packed_igemm.hip: fixed_quant's level clamped to [0, n] (a NaN: 0); cnt counts the clamped ones
__device__ __forceinline__ unsigned iv_act_code(float x, const ActQ& q, int& cnt) {
  const float r = (x - q.mn) / q.rng;
  const float qi = __builtin_floorf(r * q.n + 0.5f);
  const bool in = qi >= 0.f && qi <= q.n;
  cnt += in ? 0 : 1;
  const float c = qi >= 0.f ? (qi <= q.n ? qi : q.n) : 0.f;
  return (unsigned)(int)c;
}

// One output element in the call's output form; one thread per element
__device__ __forceinline__ void iv_out(const IvArgs& a, long long e, float v, int& cnt) {
  if (a.out == kIvCodes) a.yc[e] = (unsigned char)iv_act_code(v, a.oq, cnt);
  else if (a.out == kIvQuant) a.y[e] = fixed_quant(v, a.oq);
  else a.y[e] = v;
}

// One output of a workgroup: the range's partial sums (split form) or the epilogue's value.
// first: the one thread of the range that owns Sx[c].
__device__ __forceinline__ void iv_emit(const IvArgs& a, int c, int m, unsigned U, unsigned Sx, bool first, int& cnt) {
  if (a.ns > 1) {
    const long long z = blockIdx.z;
    a.part[(z * a.N + c) * a.M + m] = U;
    if (first) a.xpart[z * a.N + c] = Sx;
  } else {
    const bool hb = a.bias != nullptr;
    iv_out(a, (long long)c * a.M + m, iv_value(U, Sx, a.rowsum[m], a, hb, hb ? a.bias[m] : 0.f), cnt);
  }
}

// The block's count into *counter by one atomic (none for a zero count). All 256 threads call.
__device__ __forceinline__ void iv_count(int cnt, int* counter) {
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

// the sum of each 16-lane DPP row in its lane 15 (all lanes of the wave call)
__device__ __forceinline__ unsigned iv_row_sum(unsigned v) {
  v += dpp_zero<0x111>(v);
  v += dpp_zero<0x112>(v);
  v += dpp_zero<0x114>(v);
  v += dpp_zero<0x118>(v);
  return v;
}

__device__ __forceinline__ unsigned iv_dot4(unsigned w, unsigned x, unsigned acc) {
  return __builtin_amdgcn_udot4(w, x, acc, false);
}

// Where code i of a group of 16 lies among the group's 16 staged bytes. Plane widths (4 and 2 bits):
// plane j of a weight dword, (d >> BITS j) & mask, holds in byte b the dword's code j + (8 / BITS) b,
// so staged dword (dword, plane), byte b is that code's ux. Other widths: natural order.
template <int BITS>
__host__ __device__ constexpr int iv_pos(int i) {
  if (BITS != 2 && BITS != 4) return i;
  const int per = 8 / BITS, cpd = 32 / BITS;
  const int w = i / cpd, r = i % cpd;
  return (w * per + r % per) * 4 + r / per;
}

// Stages per thread: groups of 16 k over NB columns of a CH chunk
template <int NB, int CH>
constexpr int iv_ni() { return (NB * (CH / 16) + 255) / 256; }

// The workgroup's ux image of one chunk: column c's byte for k0 + kk at xs[c CS + (kk / RUN) PAD + pos], 0 for
// k >= ke and c >= N; PERM: the 16 bytes of a group in iv_pos order. A thread moves groups g = tid + 256 i
// (16 k of column g / (CH / 16)) and adds their bytes to sx[i].
template <int BITS, bool PERM, int NB, int CH, int RUN, int PAD>
__device__ __forceinline__ void iv_stage(const IvArgs& a, unsigned char* xs, int k0, int ke, unsigned (&sx)[iv_ni<NB, CH>()]) {
  constexpr int CS = CH / RUN * PAD, gpc = CH / 16;
  const int K = a.K, N = a.N;
#pragma unroll
  for (int i = 0; i < iv_ni<NB, CH>(); ++i) {
    const int g = (int)threadIdx.x + 256 * i;
    if (g >= NB * gpc) break;
    const int c = g / gpc, kk = (g - c * gpc) * 16;
    const int k = k0 + kk;
    unsigned v[4] = {0u, 0u, 0u, 0u};
    if (c < N && k < ke) {
      const unsigned char* __restrict__ p = a.x + (long long)c * K + k;
      if (a.xal && k + 16 <= ke) {
        const iv_u32x4 q = *reinterpret_cast<const iv_u32x4*>(p);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
      } else {
        const int nk = min(16, ke - k);
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (j < nk) v[j >> 2] |= (unsigned)p[j] << (8 * (j & 3));
      }
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) sx[i] = iv_dot4(v[d], 0x01010101u, sx[i]);
    unsigned o[4] = {v[0], v[1], v[2], v[3]};
    if constexpr (PERM) {
      o[0] = 0u; o[1] = 0u; o[2] = 0u; o[3] = 0u;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int p = iv_pos<BITS>(j);
        o[p >> 2] |= ((v[j >> 2] >> (8 * (j & 3))) & 255u) << (8 * (p & 3));
      }
    }
    *reinterpret_cast<iv_u32x4*>(xs + c * CS + (kk / RUN) * PAD + (kk % RUN)) = iv_u32x4{o[0], o[1], o[2], o[3]};
  }
}

// The threads' sums of ux into sxr[g / 16] (a column's groups are CH / 16 / 16 neighbouring entries).
// Every lane calls; the caller's barrier stands between this and iv_sx.
template <int NB, int CH>
__device__ __forceinline__ void iv_sx_put(const unsigned (&sx)[iv_ni<NB, CH>()], unsigned* sxr) {
#pragma unroll
  for (int i = 0; i < iv_ni<NB, CH>(); ++i) {
    const int g = (int)threadIdx.x + 256 * i;
    const unsigned v = iv_row_sum(sx[i]);
    if ((threadIdx.x & 15) == 15 && g < NB * (CH / 16)) sxr[g >> 4] = v;
  }
}
template <int CH>
__device__ __forceinline__ unsigned iv_sx(const unsigned* sxr, int c) {
  unsigned s = 0u;
#pragma unroll
  for (int r = 0; r < CH / 256; ++r) s += sxr[c * (CH / 256) + r];
  return s;
}

// Code j of a run of aligned dwords d (compile-time j): gv_code of packed_gemv.h
template <int BITS>
__device__ __forceinline__ unsigned iv_code(const unsigned (&d)[BITS], int j) {
  constexpr unsigned mask = (1u << BITS) - 1u;
  const int bit = j * BITS, w = bit >> 5, o = bit & 31;
  if (o + BITS <= 32) return (d[w] >> o) & mask;
  return __builtin_amdgcn_alignbit(d[w + 1 < BITS ? w + 1 : w], d[w], o) & mask;
}

// Byte-lane dword q (0..3) of the run's half h (16 codes), in the staged order of iv_pos
template <int BITS>
__device__ __forceinline__ unsigned iv_lanes(const unsigned (&d)[BITS], int h, int q) {
  if constexpr (BITS == 8) {
    return d[4 * h + q];
  } else if constexpr (BITS == 4) {
    return (d[2 * h + (q >> 1)] >> (4 * (q & 1))) & 0x0F0F0F0Fu;
  } else if constexpr (BITS == 2) {
    return (d[h] >> (2 * q)) & 0x03030303u;
  } else {
    const int j = 16 * h + 4 * q;
    return iv_code<BITS>(d, j) | (iv_code<BITS>(d, j + 1) << 8) | (iv_code<BITS>(d, j + 2) << 16) |
           (iv_code<BITS>(d, j + 3) << 24);
  }
}

// --- host side ------------------------------------------------------------------------------------

// The plan of one call, a function of (trans_w, M, K, bits) alone. One launch where the row tiles
// fill the chip (kIvOneLaunch of them), for W = D where K is at most kIvOneLaunchK (a workgroup walks
// four chunks in less than the reduce launch costs, measured at every N: DESIGN.md 2.36; the D^T
// kernel's workgroup is slower along k and keeps its split) or K is within one range's minimum kmin; else enough ranges
// for kIvFill workgroups, kIvSplitMax at most, each a multiple of kmin. kmin is the kernel's
// granule of k (a chunk of 1024 for W = D: every lane has a run; a chunk of 256 for D^T: every
// wave has its quarter) times the smallest power of two at which a full tile's range holds
// kIvRangeBytes of codes: 1024 x {4, 2, 2, 1, ...} for bits 1, 2, 3, 4.. (32 rows), 256 x {2, 1, ...}
// for bits 1, 2.. (256 m).
struct IvPlan {
  int ks, ns;
  long long tiles;
  size_t ws;
};

inline bool plan_iv(const ::admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K, int64_t N, IvPlan& pl) {
  if (!meta || (trans_w != 0 && trans_w != 1) || M <= 0 || K <= 0 || N < 1 || N > ADMMQ_GEMV_N_MAX) return false;
  if (meta->bits < 1 || meta->bits > 8) return false;
  if (M > (int64_t(1) << 22) || K > kIvKMax || M * K >= (int64_t(1) << 40)) return false;   // admmq_packed_igemm's limits
  const int64_t tile = trans_w ? kItTile : kIvRows, gran = trans_w ? kItCh : kIvCh;
  int64_t kmin = gran;
  while (tile * kmin * meta->bits / 8 < kIvRangeBytes) kmin *= 2;
  pl.tiles = (M + tile - 1) / tile;
  int64_t want = 1;
  if (pl.tiles < kIvOneLaunch && (trans_w || K > kIvOneLaunchK))
    want = std::min<int64_t>({(kIvFill + pl.tiles - 1) / pl.tiles, (int64_t)kIvSplitMax, (K + kmin - 1) / kmin});
  const int64_t ks = kmin * ((((K + want - 1) / want) + kmin - 1) / kmin);
  pl.ks = (int)ks;
  pl.ns = (int)((K + ks - 1) / ks);
  pl.ws = pl.ns > 1 ? (size_t)pl.ns * (size_t)N * ((size_t)M + 1) * sizeof(uint32_t) : 0;
  return true;
}

inline bool iv_act_bits_ok(const admmq_actq* q) { return q && q->on != 0 && q->bits >= 2 && q->bits <= 8; }

}  // namespace admmq
