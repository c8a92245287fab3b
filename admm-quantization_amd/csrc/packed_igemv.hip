// Skinny integer GEMV of a packed weight for decode shapes (include/admmq.h "Skinny integer GEMV",
// DESIGN.md 2.36): admmq_packed_igemm's value for 1 <= N <= 8 rows of activation codes ux [N, K]
// in the linear layout, W = D or D^T, on the dot4 unit (v_dot4_u32_u8). No MFMA and no LDS image
// of the weight.
//
// The unsigned form: the instruction runs on the raw weight codes u and the raw activation codes,
//   U[c, m] = sum_k u[m, k] ux[c, k]        Sx[c] = sum_k ux[c, k]
//   S[c, m] = U - off Sx   (int64; off = q + zp, a = u - off)
// and the epilogue is the contract's double formula on S and A[m] (rowsums). U <= 255 * 255 * 65536
// = 2^32 - 33489151 fits the instruction's uint32 accumulator at the limit K = 65536, without slack
// for any pre-added term: off enters behind the sum, in int64. Every sum is an integer, so the
// kernels' split of K over lanes, waves and workgroups changes no bit.
//
// The activation codes of a K chunk are staged once per workgroup into LDS as packed bytes (a
// thread moves 16 k of one column; the same thread adds them into Sx with a dot4 against
// 0x01010101, so Sx costs nothing in the product loop). Rows past N and k past the range are 0.
//   k_packed_igemv   (W = D). A workgroup of four waves owns 32 rows, a wave's two halves of 32
//     lanes four rows each, and a lane the run of 32 codes k = k0 + 32 (lane & 31) .. + 31 of each
//     of them in every chunk of 1024 k: BITS + 1 dwords a row, funnel-shifted into BITS aligned
//     ones. The weight's byte lanes: 8 bits - the dwords as they are; 4 and 2 bits - a mask and a
//     shift per plane ((d >> BITS j) & 0x0F0F0F0F / 0x03030303), whose bytes hold every (8 / BITS)th
//     code, with the matching byte permutation applied once to the staged ux (iv_pos); the other
//     widths - a real cut, code by code (gv_code's), into natural order. A run's 32 bytes of a
//     column lie 48 bytes apart in LDS: three 16-byte slots, an odd count, so the 16-byte reads of
//     16 neighbouring lanes fall into 16 different slots. The 32 lanes of a row meet in a DPP tree
//     inside each 16-lane row and then through LDS.
//   k_packed_igemv_t (W = D^T). Lanes run along m, four consecutive m a lane, 256 m a workgroup.
//     Each wave walks its quarter (64 k) of every chunk of 256 k, 16 k a step: 16 windows of
//     4 BITS bits are loaded, transposed four at a time into byte lanes (a cut and a shift-or per
//     code) and multiplied with the ux dwords that every lane reads from the same LDS address
//     (a broadcast; natural byte order). The waves' sums meet through LDS.
// Few row tiles do not fill the chip, so the host planner (plan_iv, a function of trans_w, M, K
// and bits) cuts K into ns ranges over gridDim.z. The split workgroups write uint32 partial images
// [ns][N][M] (and [ns][N] of Sx) to the workspace and k_packed_igemv_reduce adds them and runs the
// epilogue. No workgroup waits for another, and no output is combined with atomics.
#include "packed_igemv.h"

namespace admmq {

template <int BITS, int NB>
__global__ __launch_bounds__(256) void k_packed_igemv(const IvArgs a) {
  constexpr int CS = kIvLK * kIvPad;        // bytes of a column's image
  constexpr int RS = kIvR * NB;             // sums of a 16-lane row: [r][c]
  constexpr bool PERM = BITS == 2 || BITS == 4;
  __shared__ __attribute__((aligned(16))) unsigned char xs[NB * CS];
  __shared__ unsigned red[16 * RS];
  __shared__ unsigned sxr[NB * (kIvCh / 256)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = lane >> 5, kl = lane & 31;
  const int M = a.M, K = a.K;
  const int kb = (int)blockIdx.z * a.ks, ke = min(K, kb + a.ks);
  const unsigned char* __restrict__ codes = a.codes;
  const long long nbytes = a.nbytes;

  // the lane's rows (past M: the last row, computed and never stored) and their runs' place in the stream
  const int mrow = (int)blockIdx.x * kIvRows + (2 * wave + grp) * kIvR;
  long long wq[kIvR];
  int sh[kIvR];
#pragma unroll
  for (int r = 0; r < kIvR; ++r) {
    const long long bit0 = ((long long)min(mrow + r, M - 1) * K + (kb + kIvRun * kl)) * BITS;
    wq[r] = bit0 >> 5;
    sh[r] = (int)(bit0 & 31);   // the same at every chunk: a chunk is 32 BITS whole dwords further
  }
  unsigned acc[kIvR][NB], sx[iv_ni<NB, kIvCh>()];
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

  // the 32 lanes of a row: a tree inside each 16-lane DPP row, then the two row sums through LDS
  const int row16 = 4 * wave + (lane >> 4);
#pragma unroll
  for (int c = 0; c < NB; ++c)
#pragma unroll
    for (int r = 0; r < kIvR; ++r) {
      const unsigned v = iv_row_sum(acc[r][c]);
      if ((lane & 15) == 15) red[row16 * RS + r * NB + c] = v;
    }
  iv_sx_put<NB, kIvCh>(sx, sxr);
  __syncthreads();
  int cnt = 0;
  if (tid < kIvRows * NB) {
    const int c = tid / kIvRows, rr = tid - c * kIvRows;   // consecutive threads: consecutive m
    const int lg = rr / kIvR, r = rr - lg * kIvR;          // the lane group 2 wave + grp and its row
    const int m = (int)blockIdx.x * kIvRows + rr;
    if (m < M && c < a.N) {
      const unsigned* p0 = red + (2 * lg) * RS;
      iv_emit(a, c, m, p0[r * NB + c] + p0[RS + r * NB + c], iv_sx<kIvCh>(sxr, c), m == 0, cnt);
    }
  }
  if (a.out == kIvCodes && a.clamped && a.ns == 1) iv_count(cnt, a.clamped);   // (uniform; no return above)
}

template <int BITS, int NB>
__global__ __launch_bounds__(256) void k_packed_igemv_t(const IvArgs a) {
  // the ux image [NB][256] bytes; then the waves' sums [c][256] uint32
  __shared__ __attribute__((aligned(16))) unsigned xs32[NB * kItTile];
  __shared__ unsigned sxr[NB * (kItCh / 256)];
  unsigned char* xs = reinterpret_cast<unsigned char*>(xs32);
  constexpr unsigned mask = (1u << BITS) - 1u;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.M, K = a.K;
  const int kb = (int)blockIdx.z * a.ks, ke = min(K, kb + a.ks);
  const unsigned char* __restrict__ codes = a.codes;
  const long long nbytes = a.nbytes;
  const int ml = (int)blockIdx.x * kItTile + kItJ * lane;   // the lane's first m
  const bool on = ml < M;
  const long long mstep = (long long)M * BITS;              // bits between two k of the stream

  unsigned acc[kItJ][NB], sx[iv_ni<NB, kItCh>()];
  sx[0] = 0u;
#pragma unroll
  for (int c = 0; c < NB; ++c)
#pragma unroll
    for (int j = 0; j < kItJ; ++j) acc[j][c] = 0u;

  for (int k0 = kb; k0 < ke; k0 += kItCh) {
    __syncthreads();   // the last chunk's image has been read
    iv_stage<BITS, false, NB, kItCh, kItCh, kItCh>(a, xs, k0, ke, sx);
    __syncthreads();
    const int kw0 = k0 + wave * (kItCh / 4), kw1 = min(ke, kw0 + kItCh / 4);
    // 16 rows of the stream a step; a row past the range is not read (its ux are zeros)
    for (int k = kw0; k < kw1; k += 16) {
      long long bit0 = ((long long)k * M + ml) * BITS;
      unsigned v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const long long q = bit0 >> 5;
        unsigned lo = 0u, hi = 0u;
        if (on && k + i < kw1) {
          if (4 * (q + 2) <= nbytes) {
            const gcu32* p = (const gcu32*)(codes + 4 * q);
            lo = p[0]; hi = p[1];
          } else {
            lo = code_dword(codes, q, nbytes);
            hi = code_dword(codes, q + 1, nbytes);
          }
        }
        v[i] = __builtin_amdgcn_alignbit(hi, lo, (unsigned)(bit0 & 31));   // 4 BITS <= 32 bits from bit 0
        bit0 += mstep;
      }
      iv_u32x4 xv[NB];
#pragma unroll
      for (int c = 0; c < NB; ++c) xv[c] = *reinterpret_cast<const iv_u32x4*>(xs + c * kItCh + (k - k0));   // (a broadcast read)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int j = 0; j < kItJ; ++j) {
          const unsigned wb = ((v[4 * q] >> (j * BITS)) & mask) | (((v[4 * q + 1] >> (j * BITS)) & mask) << 8) |
                              (((v[4 * q + 2] >> (j * BITS)) & mask) << 16) | (((v[4 * q + 3] >> (j * BITS)) & mask) << 24);
#pragma unroll
          for (int c = 0; c < NB; ++c) acc[j][c] = iv_dot4(wb, xv[c][q], acc[j][c]);
        }
      }
    }
  }
  iv_sx_put<NB, kItCh>(sx, sxr);
  // the waves' sums meet in wave 0
  for (int w = 1; w < 4; ++w) {
    __syncthreads();   // (w = 1: every wave has left the image)
    if (wave == w) {
#pragma unroll
      for (int c = 0; c < NB; ++c)
        *reinterpret_cast<iv_u32x4*>(xs32 + c * kItTile + kItJ * lane) = iv_u32x4{acc[0][c], acc[1][c], acc[2][c], acc[3][c]};
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        const iv_u32x4 t = *reinterpret_cast<const iv_u32x4*>(xs32 + c * kItTile + kItJ * lane);
        acc[0][c] += t[0]; acc[1][c] += t[1]; acc[2][c] += t[2]; acc[3][c] += t[3];
      }
    }
  }
  int cnt = 0;
  if (wave == 0 && on) {
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      if (c >= a.N) break;
      const unsigned Sx = iv_sx<kItCh>(sxr, c);
#pragma unroll
      for (int j = 0; j < kItJ; ++j)
        if (ml + j < M) iv_emit(a, c, ml + j, acc[j][c], Sx, ml + j == 0, cnt);
    }
  }
  if (a.out == kIvCodes && a.clamped && a.ns == 1) iv_count(cnt, a.clamped);   // (uniform; no return above)
}

// S = sum of the ranges' images (any order: integers), then the epilogue
__global__ __launch_bounds__(256) void k_packed_igemv_reduce(const IvArgs a) {
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
    iv_out(a, e, iv_value(U, Sx, a.rowsum[m], a, hb, hb ? a.bias[m] : 0.f), cnt);
  }
  if (a.out == kIvCodes && a.clamped) iv_count(cnt, a.clamped);
}

// The clamp counter's reset on the stream: a kernel, so that a captured graph holds no memset node
__global__ void k_packed_igemv_zero(int* counter) {
  if (threadIdx.x == 0) *counter = 0;
}

// --- host side (plan_iv: packed_igemv.h) ----------------------------------------------------------

template <int BITS, int NB>
static void iv_launch(const IvArgs& a, int32_t trans_w, dim3 grid, hipStream_t s) {
  if (trans_w) hipLaunchKernelGGL((k_packed_igemv_t<BITS, NB>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_packed_igemv<BITS, NB>), grid, dim3(256), 0, s, a);
}

}  // namespace admmq

using namespace admmq;

extern "C" {

size_t admmq_packed_igemv_workspace_size(const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K, int64_t N) {
  IvPlan pl;
  return plan_iv(meta, trans_w, M, K, N, pl) ? pl.ws : 0;
}

int32_t admmq_packed_igemv_plan(const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K, int32_t out[3]) {
  IvPlan pl;
  if (!out || !plan_iv(meta, trans_w, M, K, 1, pl))
    return packed_fail("packed_igemv_plan", ADMMQ_ERR_ARG, "NULL meta / out or arguments out of range");
  out[0] = pl.ks; out[1] = pl.ns; out[2] = pl.ns > 1 ? 2 : 1;
  return ADMMQ_OK;
}

int32_t admmq_packed_igemv(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                           const uint8_t* x, const admmq_actq* x_q, const int32_t* rowsums, int64_t N, const float* bias,
                           float* y, uint8_t* y_codes, const admmq_actq* out_q, int32_t* clamped, void* workspace,
                           size_t workspace_bytes, void* stream) {
  const char* const who = "packed_igemv";
  if (!codes || !x || !meta || !rowsums || !x_q)
    return packed_fail(who, ADMMQ_ERR_ARG, "codes, meta, x, x_q and rowsums must not be NULL");
  if ((y == nullptr) == (y_codes == nullptr)) return packed_fail(who, ADMMQ_ERR_ARG, "exactly one of y and y_codes must be given");
  if (M <= 0 || K <= 0) return packed_fail(who, ADMMQ_ERR_ARG, "M and K must be positive");
  if (N < 1 || N > ADMMQ_GEMV_N_MAX) return packed_fail(who, ADMMQ_ERR_ARG, "N must be 1..8 (ADMMQ_GEMV_N_MAX)");
  int off = 0;
  int32_t rc = packed_meta_check(meta, who, true, &off);
  if (rc != ADMMQ_OK) return rc;
  if (K > kIvKMax) return packed_fail(who, ADMMQ_ERR_ARG, "K must be at most 65536 (the uint32 sum 255 * 255 * K)");
  if (!iv_act_bits_ok(x_q)) return packed_fail(who, ADMMQ_ERR_ARG, "x_q must be on with bits 2..8");
  const bool oq = out_q && out_q->on != 0;
  if (y_codes && !iv_act_bits_ok(out_q)) return packed_fail(who, ADMMQ_ERR_ARG, "a codes output needs out_q on with bits 2..8");
  if (y && oq && (out_q->bits < 1 || out_q->bits > 24)) return packed_fail(who, ADMMQ_ERR_ARG, "out_q bits must be 1..24");
  if (trans_w != 0 && trans_w != 1) return packed_fail(who, ADMMQ_ERR_ARG, "trans_w must be 0 or 1");
  if ((reinterpret_cast<uintptr_t>(codes) & 15) != 0) return packed_fail(who, ADMMQ_ERR_ARG, "codes must be 16-byte aligned");
  if (((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(rowsums) |
        reinterpret_cast<uintptr_t>(clamped)) & 3) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "y, bias, rowsums and clamped must be 4-byte aligned");
  IvPlan pl;
  if (!plan_iv(meta, trans_w, M, K, N, pl)) return packed_fail(who, ADMMQ_ERR_ARG, "sizes out of range");
  if (pl.ws > 0 && (!workspace || workspace_bytes < pl.ws)) return set_error(ADMMQ_ERR_WORKSPACE, "packed_igemv: workspace too small");
  if (pl.ws > 0 && (reinterpret_cast<uintptr_t>(workspace) & 3) != 0)
    return packed_fail(who, ADMMQ_ERR_ARG, "workspace must be uint32 aligned");
  IvArgs a;
  a.codes = codes; a.x = x; a.bias = bias; a.rowsum = rowsums; a.y = y; a.yc = y_codes;
  a.part = pl.ns > 1 ? static_cast<unsigned*>(workspace) : nullptr;
  a.xpart = pl.ns > 1 ? a.part + (size_t)pl.ns * (size_t)N * (size_t)M : nullptr;
  a.clamped = y_codes ? clamped : nullptr;
  a.nbytes = (long long)admmq_packed_bytes(M * K, meta->bits);
  a.M = (int)M; a.K = (int)K; a.N = (int)N;
  a.ks = pl.ks; a.ns = pl.ns;
  a.off = off;
  a.xal = ((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (K & 15) == 0) ? 1 : 0;
  a.out = y_codes ? kIvCodes : (oq ? kIvQuant : kIvFloat);
  a.s = (double)meta->scale;
  a.g = (double)x_q->rng / (double)((1 << x_q->bits) - 1);
  a.mnx = (double)x_q->mn;
  a.oq = oq ? actq_make(out_q) : ActQ{0.f, 0.f, 0.f, 0};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a.clamped) hipLaunchKernelGGL(k_packed_igemv_zero, dim3(1), dim3(64), 0, s, a.clamped);
  const dim3 grid((unsigned)pl.tiles, 1u, (unsigned)pl.ns);
#define ADMMQ_IV_BITS(B)                                   \
  if (N == 1) iv_launch<B, 1>(a, trans_w, grid, s);        \
  else if (N == 2) iv_launch<B, 2>(a, trans_w, grid, s);   \
  else if (N <= 4) iv_launch<B, 4>(a, trans_w, grid, s);   \
  else iv_launch<B, 8>(a, trans_w, grid, s)
  PACKED_BITS_SWITCH(meta->bits, ADMMQ_IV_BITS)
#undef ADMMQ_IV_BITS
  if (pl.ns > 1)
    hipLaunchKernelGGL(k_packed_igemv_reduce, dim3((unsigned)((N * M + 255) / 256)), dim3(256), 0, s, a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(ADMMQ_ERR_HIP, hipGetErrorString(err));
  return ADMMQ_OK;
}

}  // extern "C"
