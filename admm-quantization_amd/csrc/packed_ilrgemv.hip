// Skinny integer quant + low-rank GEMV for decode shapes (include/admmq.h "Skinny integer quant + low-rank
// GEMV"):
//   y[c, m] = x^ (D + L Rt)^T (+ bias),  x^ = g ux + mn_x,  g = rng_x / n_x
// for 1 <= N <= 8 rows of activation codes ux [N, K], D = scale a the integer form of packed codes [M, K]
// (admmq_packed_igemv's, W = D), L [M, r] and Rt [r, K] in float32 or in the tail type T (bfloat16 /
// float16). The code sum is k_packed_igemv's exact integer on the dot4 unit; the rank-r branch is float32
// fmaf chains on the factors as rounded to T. No MFMA, no decoded copy of ux or of the codes in memory.
//
//   k_ilr_down_gemv<NB>   U32 = Rt_T ux. Rt is read once, so the kernel is a stream: a workgroup of four waves
//     owns four rows j of Rt, a wave one of them, over the workgroup's K range in chunks of 1024 k whose ux
//     image the four waves share. The image stays bytes (NB x 1024 bytes a chunk, iv_stage's: 16-byte loads
//     where the rows of ux allow it, byte loads otherwise, zeros past the range, K and N). In every step of
//     256 k a lane owns the four k = k0 + 256 s + 4 lane .. + 3: one 16-byte load of a float32 row of Rt
//     (8 bytes of a T row; element loads where Rt's rows do not sit on such boundaries), rounded to T / widened
//     in registers, one ds_read_b32 a column widened by v_cvt_f32_ubyte0..3, four fmaf a column in increasing
//     k. The four steps' loads are issued before the staging barrier. The 64 lanes meet in the DPP row
//     tree, the four row sums by v_readlane as ((s15 + s31) + s47) + s63. plan_ilv (plan_lrgv's rule on K
//     and r) cuts K into nsd ranges over gridDim.z; range z writes its image tpart[z][c][j]. No reduce launch:
//     the consumer adds the images in range order.
//   k_packed_ilrgemv<BITS, NB>   iv_chunks (k_packed_igemv's chunk loop, restated here), the integer sums
//     reduced into LDS first, then the tail in the same lanes: t32 = float(gd double(sum_z U32_z) +
//     double(mn_x) double(rho)) is written over the dead ux image as [NB][rp] floats (rp = 32 ceil(r / 32),
//     zeros past r and N; t is not rounded to T), the 32 lanes of a row take j = l, l + 32, ... of L_T[m, :]
//     in increasing j from zero, and q meets in the float DPP row tree and the cross-half LDS step, lower
//     lanes first. The epilogue is double: scale (gd S + mn_x A) + q + bias, one rounding. Split plan
//     (plan_iv's ns > 1): the tail is slice ns of gridDim.z, runs no code chunk and writes the float32 image
//     of q; k_packed_ilrgemv_reduce adds the ns uint32 images and Sx and runs the epilogue with q.
// No workgroup waits for another, no output is combined with atomics (the clamp counter is one atomic a
// workgroup, zeroed by a one-thread kernel), no sum depends on N, and nothing past the code stream's last
// byte, past Rt, L or the last row of ux is read.
#include "packed_igemv.h"

namespace admmq {

constexpr int kIlvRows = 4;                    // rows of Rt per workgroup, one a wave
constexpr int kIlvStep = 64 * 4;               // k per step: four a lane
constexpr int kIlvSteps = 4;                   // steps per chunk
constexpr int kIlvCh = kIlvSteps * kIlvStep;   // k per chunk: 1024
constexpr int kIlvMinK = kIlvStep;             // k per range at least, and what a range is a multiple of
constexpr int kIlvSplitMax = 16;               // ranges of the down-projection at most (plan_lrgv's)
constexpr int kIlvOneLaunch = 256;             // workgroups the down-projection aims at (one a CU)
constexpr int kIlvRankMax = 256;

typedef unsigned ilv_u32x2 __attribute__((ext_vector_type(2)));
typedef float ilv_f32x4 __attribute__((ext_vector_type(4)));

struct IlvDown {
  const void* Rt;     // [r, K] row-major in fdt
  float* tpart;       // [nsd][N][r] float32 images of U32
  int r, ksd;         // the rank, k per range
  int fdt, tdt;       // ADMMQ_DT_F32 or the tail type; the tail type
  int ral;            // every row of Rt starts on a boundary of four elements and holds whole groups of four
};

struct IlvTail {
  const void* L;        // [M, r] row-major in fdt
  const float* tpart;   // [nsd][N][r]
  const float* rho;     // [r]
  float* qpart;         // split form: [N][M] float32 image of q
  int r, rp;            // the rank, and r rounded up to a multiple of 32
  int nsd;              // images of U32
  int fdt, tdt;
};

// f rounded to nearest even to T and widened again (the bits of tensor.to(T)); a stored T widened exactly
__device__ __forceinline__ float ilv_round(float f, int tdt) {
  return tdt == ADMMQ_DT_BF16 ? (float)static_cast<__bf16>(f) : (float)static_cast<_Float16>(f);
}
__device__ __forceinline__ float ilv_widen(unsigned h, int tdt) {
  if (tdt == ADMMQ_DT_BF16) return __uint_as_float(h << 16);
  return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
}
// element e of a factor as its T value in float32
__device__ __forceinline__ float ilv_factor(const void* p, long long e, int fdt, int tdt) {
  if (fdt == ADMMQ_DT_F32) return ilv_round(static_cast<const float*>(p)[e], tdt);
  return ilv_widen(static_cast<const unsigned short*>(p)[e], tdt);
}

// The raw bits of Rt[row + k .. + 3] (float32: four dwords; T: two), zeros past K; ilv_row4 makes T values of them.
// Two functions, so that a chunk's loads stay in flight across the staging barrier.
__device__ __forceinline__ iv_u32x4 ilv_load4(const IlvDown& d, long long row, int k, int K) {
  iv_u32x4 w = {0u, 0u, 0u, 0u};
  if (d.fdt == ADMMQ_DT_F32) {
    const unsigned* p = static_cast<const unsigned*>(d.Rt) + row + k;
    if (d.ral) {
      w = *reinterpret_cast<const iv_u32x4*>(p);
    } else {
      if (k < K) w[0] = p[0];
      if (k + 1 < K) w[1] = p[1];
      if (k + 2 < K) w[2] = p[2];
      if (k + 3 < K) w[3] = p[3];
    }
  } else {
    const unsigned short* p = static_cast<const unsigned short*>(d.Rt) + row + k;
    if (d.ral) {
      const ilv_u32x2 q = *reinterpret_cast<const ilv_u32x2*>(p);
      w[0] = q[0]; w[1] = q[1];
    } else {
      if (k < K) w[0] = (unsigned)p[0];
      if (k + 1 < K) w[0] |= (unsigned)p[1] << 16;
      if (k + 2 < K) w[1] = (unsigned)p[2];
      if (k + 3 < K) w[1] |= (unsigned)p[3] << 16;
    }
  }
  return w;
}
__device__ __forceinline__ ilv_f32x4 ilv_row4(const IlvDown& d, iv_u32x4 w) {
  if (d.fdt == ADMMQ_DT_F32)
    return ilv_f32x4{ilv_round(__uint_as_float(w[0]), d.tdt), ilv_round(__uint_as_float(w[1]), d.tdt),
                     ilv_round(__uint_as_float(w[2]), d.tdt), ilv_round(__uint_as_float(w[3]), d.tdt)};
  return ilv_f32x4{ilv_widen(w[0] & 0xFFFFu, d.tdt), ilv_widen(w[0] >> 16, d.tdt), ilv_widen(w[1] & 0xFFFFu, d.tdt),
                   ilv_widen(w[1] >> 16, d.tdt)};
}

// byte I of x as float32: the compiler's v_cvt_f32_ubyteI (no shift, no mask)
template <int I>
__device__ __forceinline__ float ilv_ubyte(unsigned x) {
  return (float)((x >> (8 * I)) & 255u);
}

// the sum of each 16-lane DPP row in its lane 15, a fixed tree (all lanes of the wave call)
template <int CTRL>
__device__ __forceinline__ float ilv_dpp(float v) {
  return __uint_as_float(dpp_zero<CTRL>(__float_as_uint(v)));
}
__device__ __forceinline__ float ilv_row_sum(float v) {
  v = v + ilv_dpp<0x111>(v);
  v = v + ilv_dpp<0x112>(v);
  v = v + ilv_dpp<0x114>(v);
  v = v + ilv_dpp<0x118>(v);
  return v;
}

// t32 = float(gd double(U32) + double(mn_x) double(rho)): double operations rounded one by one
__device__ __forceinline__ float ilv_t32(float U, float rho, double g, double mnx) {
#pragma clang fp contract(off)
  const double a = g * (double)U;
  const double b = mnx * (double)rho;
  return (float)(a + b);
}

// iv_value with q between the scaled sum and the bias
__device__ __forceinline__ float ilv_value(unsigned U, unsigned Sx, int A, float q, const IvArgs& a, bool has_bias, float bv) {
#pragma clang fp contract(off)
  const double S = (double)((long long)U - (long long)a.off * (long long)Sx);
  double v = a.s * (a.g * S + a.mnx * (double)A);
  v = v + (double)q;
  if (has_bias) v = v + (double)bv;
  return (float)v;
}

// k_packed_igemv's chunk loop (packed_igemv.hip), statement for statement: the sums U of the lane's kIvR rows from mrow (past M:
// the last row, computed and never stored) over the range [kb, ke) into acc, the staged bytes' sums into sx.
// xs: the workgroup's NB kIvLK kIvPad bytes. Every thread of the workgroup calls (barriers inside).
template <int BITS, int NB>
__device__ __forceinline__ void iv_chunks(const IvArgs& a, unsigned char* xs, int kb, int ke, int mrow, unsigned (&acc)[kIvR][NB],
                                          unsigned (&sx)[iv_ni<NB, kIvCh>()]) {
  constexpr int CS = kIvLK * kIvPad;        // bytes of a column's image
  constexpr bool PERM = BITS == 2 || BITS == 4;
  const int kl = threadIdx.x & 31;
  const int M = a.M, K = a.K;
  const unsigned char* __restrict__ codes = a.codes;
  const long long nbytes = a.nbytes;
  long long wq[kIvR];
  int sh[kIvR];
#pragma unroll
  for (int r = 0; r < kIvR; ++r) {
    const long long bit0 = ((long long)min(mrow + r, M - 1) * K + (kb + kIvRun * kl)) * BITS;
    wq[r] = bit0 >> 5;
    sh[r] = (int)(bit0 & 31);   // the same at every chunk: a chunk is 32 BITS whole dwords further
  }
#pragma unroll
  for (int i = 0; i < iv_ni<NB, kIvCh>(); ++i) sx[i] = 0u;
#pragma unroll
  for (int c = 0; c < NB; ++c)
#pragma unroll
    for (int r = 0; r < kIvR; ++r) acc[r][c] = 0u;

  for (int k0 = kb; k0 < ke; k0 += kIvCh) {
    const bool on = k0 + kIvRun * kl < ke;   // the run holds a k of the range
    unsigned w[kIvR][BITS + 1];
    if (on) {
#pragma unroll
      for (int r = 0; r < kIvR; ++r) {
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
    for (int r = 0; r < kIvR; ++r) wq[r] += (long long)kIvLK * BITS;
    __syncthreads();   // the last chunk's image has been read
    iv_stage<BITS, PERM, NB, kIvCh, kIvRun, kIvPad>(a, xs, k0, ke, sx);
    __syncthreads();
    if (on) {
      unsigned d[kIvR][BITS];
#pragma unroll
      for (int r = 0; r < kIvR; ++r)
#pragma unroll
        for (int i = 0; i < BITS; ++i) d[r][i] = __builtin_amdgcn_alignbit(w[r][i + 1], w[r][i], sh[r]);
      const unsigned char* xl = xs + kl * kIvPad;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        iv_u32x4 xv[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) xv[c] = *reinterpret_cast<const iv_u32x4*>(xl + c * CS + 16 * h);
#pragma unroll
        for (int r = 0; r < kIvR; ++r) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const unsigned wb = iv_lanes<BITS>(d[r], h, q);
#pragma unroll
            for (int c = 0; c < NB; ++c) acc[r][c] = iv_dot4(wb, xv[c][q], acc[r][c]);
          }
        }
      }
    }
  }
}

template <int NB>
__global__ __launch_bounds__(256) void k_ilr_down_gemv(const IvArgs a, const IlvDown d) {
  __shared__ __attribute__((aligned(16))) unsigned char xs[NB * kIlvCh];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = a.K;
  const int kb = (int)blockIdx.z * d.ksd, ke = min(K, kb + d.ksd);
  const int j = (int)blockIdx.x * kIlvRows + wave;                // the wave's row (past r: the last row, never stored)
  const long long row = (long long)min(j, d.r - 1) * K;
  float acc[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) acc[c] = 0.f;
  unsigned sx[iv_ni<NB, kIlvCh>()];   // iv_stage's sums of ux: not used here
#pragma unroll
  for (int i = 0; i < iv_ni<NB, kIlvCh>(); ++i) sx[i] = 0u;

  for (int k0 = kb; k0 < ke; k0 += kIlvCh) {
    iv_u32x4 rw[kIlvSteps];
#pragma unroll
    for (int s = 0; s < kIlvSteps; ++s) {
      const int k = k0 + kIlvStep * s + 4 * lane;
      rw[s] = iv_u32x4{0u, 0u, 0u, 0u};
      if (k < ke) rw[s] = ilv_load4(d, row, k, K);   // (ke is K or a multiple of 256: an aligned group never straddles it)
    }
    __syncthreads();   // the last chunk's image has been read
    iv_stage<8, false, NB, kIlvCh, kIlvCh, kIlvCh>(a, xs, k0, ke, sx);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kIlvSteps; ++s) {
      const int kk = kIlvStep * s + 4 * lane;
      if (k0 + kk < ke) {
        const ilv_f32x4 rv = ilv_row4(d, rw[s]);
#pragma unroll
        for (int c = 0; c < NB; ++c) {
          const unsigned xv = *reinterpret_cast<const unsigned*>(xs + c * kIlvCh + kk);
          acc[c] = __builtin_fmaf(rv[0], ilv_ubyte<0>(xv), acc[c]);
          acc[c] = __builtin_fmaf(rv[1], ilv_ubyte<1>(xv), acc[c]);
          acc[c] = __builtin_fmaf(rv[2], ilv_ubyte<2>(xv), acc[c]);
          acc[c] = __builtin_fmaf(rv[3], ilv_ubyte<3>(xv), acc[c]);
        }
      }
    }
  }
  // the 64 lanes: the tree inside each 16-lane DPP row, then the four row sums in lane order
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    const unsigned v = __float_as_uint(ilv_row_sum(acc[c]));
    const float s = ((__uint_as_float(readlane_u32(v, 15)) + __uint_as_float(readlane_u32(v, 31))) +
                     __uint_as_float(readlane_u32(v, 47))) + __uint_as_float(readlane_u32(v, 63));
    if (lane == 0 && j < d.r && c < a.N) d.tpart[((long long)blockIdx.z * a.N + c) * d.r + j] = s;
  }
}

template <int BITS, int NB>
__global__ __launch_bounds__(256) void k_packed_ilrgemv(const IvArgs a, const IlvTail lr) {
  constexpr int CS = kIvLK * kIvPad;        // bytes of a column's image
  constexpr int RS = kIvR * NB;             // sums of a 16-lane row: [r][c]
  static_assert(NB * CS >= NB * kIlvRankMax * (int)sizeof(float), "the t image fits the ux image");
  __shared__ __attribute__((aligned(16))) unsigned char xs[NB * CS];
  __shared__ unsigned red[16 * RS];
  __shared__ float qred[16 * RS];
  __shared__ unsigned sxr[NB * (kIvCh / 256)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kl = lane & 31;
  const int M = a.M;
  const bool tail_only = a.ns > 1 && (int)blockIdx.z == a.ns;      // the split plan's extra slice (uniform)
  const int kb = (int)blockIdx.z * a.ks, ke = min(a.K, kb + a.ks);   // (the tail's slice: kb >= K, no chunk)
  const int mrow = (int)blockIdx.x * kIvRows + (2 * wave + (lane >> 5)) * kIvR;
  const int row16 = 4 * wave + (lane >> 4);

  {
    // the integer sums go to LDS before the tail starts, so that q's registers reuse theirs
    unsigned acc[kIvR][NB], sx[iv_ni<NB, kIvCh>()];
    iv_chunks<BITS, NB>(a, xs, kb, ke, mrow, acc, sx);
#pragma unroll
    for (int c = 0; c < NB; ++c)
#pragma unroll
      for (int r = 0; r < kIvR; ++r) {
        const unsigned v = iv_row_sum(acc[r][c]);
        if ((lane & 15) == 15) red[row16 * RS + r * NB + c] = v;
      }
    iv_sx_put<NB, kIvCh>(sx, sxr);
  }

  float q[kIvR][NB];
#pragma unroll
  for (int c = 0; c < NB; ++c)
#pragma unroll
    for (int r = 0; r < kIvR; ++r) q[r][c] = 0.f;
  if (a.ns == 1 || tail_only) {   // (uniform)
    const int rk = lr.r, rp = lr.rp, N = a.N;
    float* const ts = reinterpret_cast<float*>(xs);
    __syncthreads();   // the last chunk's image has been read
    for (int e = tid; e < NB * rp; e += 256) {
      const int c = e / rp, j = e - c * rp;
      float v = 0.f;
      if (c < N && j < rk) {
        float u = lr.tpart[c * rk + j];
        for (int z = 1; z < lr.nsd; ++z) u = u + lr.tpart[((long long)z * N + c) * rk + j];
        v = ilv_t32(u, lr.rho[j], a.g, a.mnx);
      }
      ts[e] = v;
    }
    __syncthreads();
    long long lrow[kIvR];
#pragma unroll
    for (int r = 0; r < kIvR; ++r) lrow[r] = (long long)min(mrow + r, M - 1) * rk;   // (past M: the last row, never stored)
    for (int j = kl; j < rp; j += 32) {
      float lv[kIvR];
#pragma unroll
      for (int r = 0; r < kIvR; ++r) lv[r] = j < rk ? ilv_factor(lr.L, lrow[r] + j, lr.fdt, lr.tdt) : 0.f;   // (t is 0 there)
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        const float tv = ts[c * rp + j];   // 32 consecutive floats a half wave, both halves the same: no bank conflict
#pragma unroll
        for (int r = 0; r < kIvR; ++r) q[r][c] = __builtin_fmaf(lv[r], tv, q[r][c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NB; ++c)
#pragma unroll
    for (int r = 0; r < kIvR; ++r) {
      const float v = ilv_row_sum(q[r][c]);
      if ((lane & 15) == 15) qred[row16 * RS + r * NB + c] = v;
    }
  __syncthreads();
  int cnt = 0;
  if (tid < kIvRows * NB) {
    const int c = tid / kIvRows, rr = tid - c * kIvRows;   // consecutive threads: consecutive m
    const int lg = rr / kIvR, r = rr - lg * kIvR;          // the lane group 2 wave + grp and its row
    const int m = (int)blockIdx.x * kIvRows + rr;
    if (m < M && c < a.N) {
      const int o = (2 * lg) * RS + r * NB + c;
      const unsigned U = red[o] + red[o + RS], Sx = iv_sx<kIvCh>(sxr, c);
      const float Q = qred[o] + qred[o + RS];
      if (tail_only) {
        lr.qpart[(long long)c * M + m] = Q;
      } else if (a.ns > 1) {
        iv_emit(a, c, m, U, Sx, m == 0, cnt);
      } else {
        const bool hb = a.bias != nullptr;
        iv_out(a, (long long)c * M + m, ilv_value(U, Sx, a.rowsum[m], Q, a, hb, hb ? a.bias[m] : 0.f), cnt);
      }
    }
  }
  if (a.out == kIvCodes && a.clamped && a.ns == 1) iv_count(cnt, a.clamped);   // (uniform; no return above)
}

// S = sum of the ranges' images (any order: integers), q's image, then the epilogue
__global__ __launch_bounds__(256) void k_packed_ilrgemv_reduce(const IvArgs a, const float* __restrict__ qpart) {
  const long long total = (long long)a.N * a.M;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  int cnt = 0;
  if (e < total) {
    const int c = (int)(e / a.M), m = (int)(e - (long long)c * a.M);
    unsigned U = a.part[e], Sx = a.xpart[c];
    for (int p = 1; p < a.ns; ++p) {
      U += a.part[(long long)p * total + e];
      Sx += a.xpart[p * a.N + c];
    }
    const bool hb = a.bias != nullptr;
    iv_out(a, e, ilv_value(U, Sx, a.rowsum[m], qpart[e], a, hb, hb ? a.bias[m] : 0.f), cnt);
  }
  if (a.out == kIvCodes && a.clamped) iv_count(cnt, a.clamped);
}

// The clamp counter's reset on the stream: a kernel, so that a captured graph holds no memset node
__global__ void k_packed_ilrgemv_zero(int* counter) {
  if (threadIdx.x == 0) *counter = 0;
}

// --- host side ------------------------------------------------------------------------------------

// The plan of one call: plan_iv's split of the code sum on (M, K, bits) (ns ranges of ks), and the split of
// the down-projection, plan_lrgv's rule on K and r alone: ceil(r / 4) workgroups a range, enough ranges for
// one workgroup a CU, kIlvSplitMax at most, each a multiple of 256 k. The workspace holds, in this order,
// tpart [nsd][N][r] and, where ns > 1, part [ns][N][M], xpart [ns][N] and qpart [N][M].
struct IlvPlan {
  IvPlan iv;
  int ksd, nsd, launches;
  size_t ws;
};

static bool plan_ilv(const ::admmq_qmeta* meta, int64_t M, int64_t K, int64_t N, int64_t r, IlvPlan& pl) {
  if (r < 1 || r > kIlvRankMax || !plan_iv(meta, 0, M, K, N, pl.iv)) return false;
  const int64_t groups = (r + kIlvRows - 1) / kIlvRows;
  const int64_t want = std::min<int64_t>({(kIlvOneLaunch + groups - 1) / groups, (int64_t)kIlvSplitMax, (K + kIlvMinK - 1) / kIlvMinK});
  const int64_t ksd = kIlvMinK * ((((K + want - 1) / want) + kIlvMinK - 1) / kIlvMinK);
  pl.ksd = (int)ksd;
  pl.nsd = (int)((K + ksd - 1) / ksd);
  pl.launches = pl.iv.ns > 1 ? 3 : 2;
  pl.ws = (size_t)pl.nsd * (size_t)N * (size_t)r * sizeof(float);
  if (pl.iv.ns > 1) pl.ws += pl.iv.ws + (size_t)N * (size_t)M * sizeof(float);
  return true;
}

static bool ilv_half(int32_t dt) { return dt == ADMMQ_DT_BF16 || dt == ADMMQ_DT_F16; }

}  // namespace admmq

using namespace admmq;

extern "C" {

size_t admmq_packed_ilrgemv_workspace_size(const admmq_qmeta* meta, int64_t M, int64_t K, int64_t N, int32_t r) {
  IlvPlan pl;
  return plan_ilv(meta, M, K, N, r, pl) ? pl.ws : 0;
}

int32_t admmq_packed_ilrgemv_plan(const admmq_qmeta* meta, int64_t M, int64_t K, int32_t r, int32_t out[4]) {
  IlvPlan pl;
  if (!out || !plan_ilv(meta, M, K, 1, r, pl))
    return packed_fail("packed_ilrgemv_plan", ADMMQ_ERR_ARG, "NULL meta / out or arguments out of range");
  out[0] = pl.iv.ks; out[1] = pl.iv.ns; out[2] = pl.nsd; out[3] = pl.launches;
  return ADMMQ_OK;
}

int32_t admmq_packed_ilrgemv(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const void* L,
                             const void* Rt, int32_t f_dtype, int32_t t_dtype, int32_t r, const float* rho,
                             const uint8_t* x, const admmq_actq* x_q, const int32_t* rowsums, int64_t N, const float* bias,
                             float* y, uint8_t* y_codes, const admmq_actq* out_q, int32_t* clamped, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const char* const who = "packed_ilrgemv";
  if (!codes || !x || !meta || !rowsums || !x_q)
    return packed_fail(who, ADMMQ_ERR_ARG, "codes, meta, x, x_q and rowsums must not be NULL");
  if (!L || !Rt) return packed_fail(who, ADMMQ_ERR_ARG, "L and Rt must not be NULL");
  if (!rho) return packed_fail(who, ADMMQ_ERR_ARG, "rho must not be NULL (admmq_packed_lowrank_factorsums writes it)");
  if ((y == nullptr) == (y_codes == nullptr)) return packed_fail(who, ADMMQ_ERR_ARG, "exactly one of y and y_codes must be given");
  if (M <= 0 || K <= 0) return packed_fail(who, ADMMQ_ERR_ARG, "M and K must be positive");
  if (N < 1 || N > ADMMQ_GEMV_N_MAX) return packed_fail(who, ADMMQ_ERR_ARG, "N must be 1..8 (ADMMQ_GEMV_N_MAX)");
  if (!ilv_half(t_dtype)) return packed_fail(who, ADMMQ_ERR_ARG, "t_dtype must be ADMMQ_DT_BF16 or ADMMQ_DT_F16");
  if (f_dtype != ADMMQ_DT_F32 && f_dtype != t_dtype) return packed_fail(who, ADMMQ_ERR_ARG, "f_dtype must be ADMMQ_DT_F32 or t_dtype");
  if (r < 1 || r > kIlvRankMax) return packed_fail(who, ADMMQ_ERR_ARG, "rank r must be 1..256");
  int off = 0;
  const int32_t rc = packed_meta_check(meta, who, true, &off);
  if (rc != ADMMQ_OK) return rc;
  if (K > kIvKMax) return packed_fail(who, ADMMQ_ERR_ARG, "K must be at most 65536 (the uint32 sum 255 * 255 * K)");
  if (!iv_act_bits_ok(x_q)) return packed_fail(who, ADMMQ_ERR_ARG, "x_q must be on with bits 2..8");
  const bool oq = out_q && out_q->on != 0;
  if (y_codes && !iv_act_bits_ok(out_q)) return packed_fail(who, ADMMQ_ERR_ARG, "a codes output needs out_q on with bits 2..8");
  if (y && oq && (out_q->bits < 1 || out_q->bits > 24)) return packed_fail(who, ADMMQ_ERR_ARG, "out_q bits must be 1..24");
  if ((reinterpret_cast<uintptr_t>(codes) & 15) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "codes must be 16-byte aligned");
  if (((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(rowsums) |
        reinterpret_cast<uintptr_t>(clamped) | reinterpret_cast<uintptr_t>(rho)) & 3) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "y, bias, rowsums, rho and clamped must be 4-byte aligned");
  const int fb = f_dtype == ADMMQ_DT_F32 ? 4 : 2;   // bytes of a factor's element
  if (((reinterpret_cast<uintptr_t>(L) | reinterpret_cast<uintptr_t>(Rt)) & (fb - 1)) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "L and Rt must be aligned to their element");
  IlvPlan pl;
  if (!plan_ilv(meta, M, K, N, r, pl)) return packed_fail(who, ADMMQ_ERR_ARG, "sizes out of range");
  if (!workspace || workspace_bytes < pl.ws) return set_error(ADMMQ_ERR_WORKSPACE, "packed_ilrgemv: workspace too small");
  if ((reinterpret_cast<uintptr_t>(workspace) & 3) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "workspace must be 4-byte aligned");

  const int ns = pl.iv.ns;
  float* const tpart = static_cast<float*>(workspace);
  IvArgs a;
  a.codes = codes; a.x = x; a.bias = bias; a.rowsum = rowsums; a.y = y; a.yc = y_codes;
  a.part = ns > 1 ? reinterpret_cast<unsigned*>(tpart + (size_t)pl.nsd * (size_t)N * (size_t)r) : nullptr;
  a.xpart = ns > 1 ? a.part + (size_t)ns * (size_t)N * (size_t)M : nullptr;
  a.clamped = y_codes ? clamped : nullptr;
  a.nbytes = (long long)admmq_packed_bytes(M * K, meta->bits);
  a.M = (int)M; a.K = (int)K; a.N = (int)N;
  a.ks = pl.iv.ks; a.ns = ns;
  a.off = off;
  a.xal = ((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (K & 15) == 0) ? 1 : 0;
  a.out = y_codes ? kIvCodes : (oq ? kIvQuant : kIvFloat);
  a.s = (double)meta->scale;
  a.g = (double)x_q->rng / (double)((1 << x_q->bits) - 1);
  a.mnx = (double)x_q->mn;
  a.oq = oq ? actq_make(out_q) : ActQ{0.f, 0.f, 0.f, 0};
  IlvDown d;
  d.Rt = Rt; d.tpart = tpart; d.r = r; d.ksd = pl.ksd; d.fdt = f_dtype; d.tdt = t_dtype;
  d.ral = ((reinterpret_cast<uintptr_t>(Rt) & (4 * fb - 1)) == 0 && K % 4 == 0) ? 1 : 0;
  IlvTail lr;
  lr.L = L; lr.tpart = tpart; lr.rho = rho;
  lr.qpart = ns > 1 ? reinterpret_cast<float*>(a.xpart + (size_t)ns * (size_t)N) : nullptr;
  lr.r = r; lr.rp = 32 * ((r + 31) / 32); lr.nsd = pl.nsd; lr.fdt = f_dtype; lr.tdt = t_dtype;

  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a.clamped) hipLaunchKernelGGL(k_packed_ilrgemv_zero, dim3(1), dim3(64), 0, s, a.clamped);
  const dim3 dgrid((unsigned)((r + kIlvRows - 1) / kIlvRows), 1u, (unsigned)pl.nsd);
  const dim3 grid((unsigned)pl.iv.tiles, 1u, (unsigned)(ns > 1 ? ns + 1 : 1));
#define ADMMQ_ILV_DOWN(NB) hipLaunchKernelGGL((k_ilr_down_gemv<NB>), dgrid, dim3(256), 0, s, a, d)
#define ADMMQ_ILV_MAIN(B, NB) hipLaunchKernelGGL((k_packed_ilrgemv<B, NB>), grid, dim3(256), 0, s, a, lr)
#define ADMMQ_ILV_BITS(B)                   \
  if (N == 1) ADMMQ_ILV_MAIN(B, 1);         \
  else if (N == 2) ADMMQ_ILV_MAIN(B, 2);    \
  else if (N <= 4) ADMMQ_ILV_MAIN(B, 4);    \
  else ADMMQ_ILV_MAIN(B, 8)
  if (N == 1) ADMMQ_ILV_DOWN(1);
  else if (N == 2) ADMMQ_ILV_DOWN(2);
  else if (N <= 4) ADMMQ_ILV_DOWN(4);
  else ADMMQ_ILV_DOWN(8);
  PACKED_BITS_SWITCH(meta->bits, ADMMQ_ILV_BITS)
#undef ADMMQ_ILV_BITS
#undef ADMMQ_ILV_MAIN
#undef ADMMQ_ILV_DOWN
  if (ns > 1)
    hipLaunchKernelGGL(k_packed_ilrgemv_reduce, dim3((unsigned)((N * M + 255) / 256)), dim3(256), 0, s, a, lr.qpart);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

}  // extern "C"
