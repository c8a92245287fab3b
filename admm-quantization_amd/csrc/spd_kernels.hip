// M = (G + rho I)^-1 once per admm_iteration call (replaces torch.linalg.cholesky +
// torch.cholesky_solve of source/admm.py:54,56 by an explicit inverse so that every
// inner iteration is one GEMM). Computed in fp64 and rounded once to fp32.
//
// 32 x 32 blocked, batched over problems, fp64 VALU:
//   for s:  k_chol_step(s)    one launch per block column: the column workgroups (i, s) apply
//                             update s - 1 to A_ss (in LDS) and A_is, factor A_ss (-> D64) and
//                             form L_is = A_is L_ss^-T; the trailing workgroups (i, j), j > s,
//                             apply update s - 1, A_ij -= L_i,s-1 L_j,s-1^T
//   once:   k_diag_inv        Linv_ii = L_ii^-1
//           k_linv_cols_w     Linv_ij = -Linv_ii sum_{t=j}^{i-1} L_it Linv_tj by column slices
//                             (k_linv_row(i), one launch per block row, above 56 blocks)
//   once:   k_minv_tile       M_ij = sum_{t>=i} Linv_ti^T Linv_tj  (fp32, symmetric,
//                              zero outside R x R)
// The earlier forms stay in the build and give the same bits (admmq_debug_set_spd_form, kSpd*
// bits of admmq_internal.h): k_chol_panel(k) + k_chol_update(k) as two launches per block
// column, k_linv_cols with 128-thread groups, k_minv with a 1 x 4 strip per thread. Every
// element keeps its chain of fp64 operations in all of them: sums over block t ascending, then
// k ascending, from 0 per block product; one `dst -= acc` per update, ascending.
// A non-positive pivot sets flags[2] (the reference raises torch.linalg.LinAlgError).
#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "../../include/admmq.h"
#include "admmq_internal.h"

namespace admmq {

constexpr int NB = 32;
constexpr int LS = NB + 1;  // LDS row stride (doubles) to spread banks

__device__ __forceinline__ void load_regs(double r[4], const double* A, int ldm, int bi, int bj);
__device__ __forceinline__ void store_regs(double* dst, const double r[4]);
// blocks of 256 threads: all four loads of a thread issue before the first LDS store
__device__ __forceinline__ void load_block(double* dst, const double* A, int ldm, int bi, int bj) {
  double r[4];
  load_regs(r, A, ldm, bi, bj);
  store_regs(dst, r);
}
__device__ __forceinline__ void store_block(double* A, int ldm, int bi, int bj, const double* src) {
  for (int t = threadIdx.x; t < NB * NB; t += blockDim.x) {
    const int r = t >> 5, c = t & 31;
    A[(size_t)(bi * NB + r) * ldm + bj * NB + c] = src[r * LS + c];
  }
}

// A 32x32 block through registers (blocks of 256 threads: 4 doubles each), so the next
// block's loads can be in flight while the current one is multiplied.
__device__ __forceinline__ void load_regs(double r[4], const double* A, int ldm, int bi, int bj) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int t = threadIdx.x + 256 * q;
    r[q] = A[(size_t)(bi * NB + (t >> 5)) * ldm + bj * NB + (t & 31)];
  }
}
__device__ __forceinline__ void store_regs(double* dst, const double r[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int t = threadIdx.x + 256 * q;
    dst[(t >> 5) * LS + (t & 31)] = r[q];
  }
}

__device__ __forceinline__ double readlane_d(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ double shfl_d(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __shfl((int)b, lane, 64);
  const int hi = __shfl((int)(b >> 32), lane, 64);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// In-LDS Cholesky of a 32x32 SPD block (lower); upper part zeroed. One wave, all 64 lanes:
// lane (r, h) = r + 32 h holds row r's columns 2 j + h in registers, so each of the 32
// right-looking steps (pivot by readlane, l_r = a_rc / sqrt(pivot), a_rs -= l_r l_s with l_s
// shuffled from lane s) is about half the instructions per lane of a one-row-per-lane form
// (which also kept ~60 broadcast values in SGPRs and spilled them): 17.0 -> 10.6 us per
// block, the same operations per element (same bits; tools/probes/chol_probe.hip). No
// workgroup barrier inside.
__device__ __forceinline__ void chol32_wave(double* a, int* err) {   // wave 0 only
  {
    const int r = threadIdx.x & 31, h = threadIdx.x >> 5;
    double rw[NB / 2];
#pragma unroll
    for (int j = 0; j < NB / 2; ++j) rw[j] = a[r * LS + 2 * j + h];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      // row r's entry c lives in lane r + 32 (c & 1), slot c >> 1
      const double rc = shfl_d(rw[c >> 1], r + 32 * (c & 1));
      const double d = readlane_d(rw[c >> 1], c + 32 * (c & 1));
      if (threadIdx.x == 0 && !(d > 0.0)) *err = 1;
      const double sd = sqrt(d);
      const double l = r > c ? rc / sd : (r == c ? sd : 0.0);
      if ((c & 1) == h) rw[c >> 1] = l;
#pragma unroll
      for (int j = 0; j < NB / 2; ++j) {
        if (2 * j + 1 <= c) continue;   // (uniform: both columns of slot j at or before c)
        const int sc = 2 * j + h;       // this lane's column of slot j
        const double ls = shfl_d(l, sc);
        if (sc > c) rw[j] -= l * ls;
      }
    }
#pragma unroll
    for (int j = 0; j < NB / 2; ++j) {
      const int sc = 2 * j + h;
      a[r * LS + sc] = sc <= r ? rw[j] : 0.0;
    }
  }
}
__device__ void chol32(double* a, int* err) {
  if (threadIdx.x < 64) chol32_wave(a, err);
  __syncthreads();
}

// Inverse of a lower-triangular 32x32 block: column c by thread c, held in registers.
// Reciprocal pivots are formed first, off the chain; each row's entries of l are read into
// registers before its FMA chains (read at their use, every LDS read was waited for on
// its own: 50.6 -> 21.1 us for chol32 + trinv32 over 576 blocks, tools/spd_probe.hip, same
// bits), and each row's sum runs as two interleaved FMA chains.
// The 32 reciprocal pivots are divided once, one per thread, into x's spare column 32 (every
// thread dividing all 32 was ~1000 VALU instructions per thread; the same quotients).
__device__ __forceinline__ void trinv32_cols(const double* l, double* x) {   // threads 0..31 only
  {
    const int c = threadIdx.x;
    x[c * LS + NB] = 1.0 / l[c * LS + c];
    __builtin_amdgcn_wave_barrier();   // (one wave: its LDS writes land before its later reads)
    asm volatile("" ::: "memory");
    double rinv[NB], col[NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) rinv[r] = x[r * LS + NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) {
      double lr[NB];
#pragma unroll
      for (int t = 0; t < r; ++t) lr[t] = l[r * LS + t];
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int t = 0; t + 1 < r; t += 2) {   // col[t] = 0 for t < c
        s0 += lr[t] * col[t];
        s1 += lr[t + 1] * col[t + 1];
      }
      if (r & 1) s0 += lr[r - 1] * col[r - 1];
      col[r] = r < c ? 0.0 : (r == c ? rinv[r] : -(s0 + s1) * rinv[r]);
    }
#pragma unroll
    for (int r = 0; r < NB; ++r) x[r * LS + c] = col[r];
  }
}
__device__ __forceinline__ void trinv32(const double* l, double* x) {
  if (threadIdx.x < NB) trinv32_cols(l, x);
  __syncthreads();
}

// acc[4] += A(rows r0..) * B^T or A * B for a 32x32x32 product; thread owns 4 outputs.
// out(r, c) for r = tid>>3 (0..31), c = (tid&7)*4 + q
// (mm_nt_at: the strip at row r, columns cb .. cb + 3, for a thread that is given its strip)
__device__ __forceinline__ void mm_nt_at(const double* a, const double* b, double acc[4], int r, int cb) {
  for (int t = 0; t < NB; ++t) {
    const double av = a[r * LS + t];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] += av * b[(cb + q) * LS + t];
  }
}
__device__ __forceinline__ void mm_nt(const double* a, const double* b, double acc[4]) {  // a * b^T
  mm_nt_at(a, b, acc, threadIdx.x >> 3, (threadIdx.x & 7) * 4);
}
__device__ __forceinline__ void mm_nn(const double* a, const double* b, double acc[4]) {  // a * b
  const int r = threadIdx.x >> 3, cb = (threadIdx.x & 7) * 4;
  for (int t = 0; t < NB; ++t) {
    const double av = a[r * LS + t];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] += av * b[t * LS + cb + q];
  }
}
__device__ __forceinline__ void mm_tn(const double* a, const double* b, double acc[4]) {  // a^T * b
  const int r = threadIdx.x >> 3, cb = (threadIdx.x & 7) * 4;
  for (int t = 0; t < NB; ++t) {
    const double av = a[t * LS + r];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] += av * b[t * LS + cb + q];
  }
}

__global__ __launch_bounds__(256) void k_chol_panel(const ProbDesc* __restrict__ probs, int k) {
  const ProbDesc& p = probs[blockIdx.y];
  const int i = k + blockIdx.x;
  if (k >= p.nbk || i >= p.nbk) return;
  __shared__ double lkk[NB * LS], x[NB * LS], aik[NB * LS];
  __shared__ int err;
  if (threadIdx.x == 0) err = 0;
  double ra[4];                      // A_ik in flight while L_kk is factored and inverted
  if (i != k) load_regs(ra, p.A64, p.ldm, i, k);
  load_block(lkk, p.A64, p.ldm, k, k);
  __syncthreads();
  chol32(lkk, &err);
  if (i == k) {   // siblings still read A_kk in this launch: L_kk goes to the diagonal store
    if (err && threadIdx.x == 0) p.flags[2] = 1;
    store_block(p.D64, NB, k, 0, lkk);
    return;
  }
  trinv32(lkk, x);                   // x = L_kk^-1
  store_regs(aik, ra);
  __syncthreads();
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  mm_nt(aik, x, acc);                // L_ik = A_ik * (L_kk^-1)^T
  __syncthreads();
  const int r = threadIdx.x >> 3, cb = (threadIdx.x & 7) * 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) aik[r * LS + cb + q] = acc[q];
  __syncthreads();
  store_block(p.A64, p.ldm, i, k, aik);
}

__global__ __launch_bounds__(256) void k_chol_update(const ProbDesc* __restrict__ probs, int k) {
  const ProbDesc& p = probs[blockIdx.y];
  const int n = p.nbk - k - 1;
  if (n <= 0) return;
  const int q = blockIdx.x;
  if (q >= n * (n + 1) / 2) return;
  // q -> (ii, jj) with 0 <= jj <= ii < n, row-major lower triangle
  int ii = (int)((sqrt(8.0 * q + 1.0) - 1.0) * 0.5);
  while ((ii + 1) * (ii + 2) / 2 <= q) ++ii;
  while (ii * (ii + 1) / 2 > q) --ii;
  const int jj = q - ii * (ii + 1) / 2;
  const int i = k + 1 + ii, j = k + 1 + jj;
  __shared__ double li[NB * LS], lj[NB * LS];
  load_block(li, p.A64, p.ldm, i, k);
  load_block(lj, p.A64, p.ldm, j, k);
  __syncthreads();
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  mm_nt(li, lj, acc);
  const int r = threadIdx.x >> 3, cb = (threadIdx.x & 7) * 4;
  double* dst = p.A64 + (size_t)(i * NB + r) * p.ldm + j * NB + cb;
#pragma unroll
  for (int t = 0; t < 4; ++t) dst[t] -= acc[t];
}

// Block column s in one launch (kSpdFusedChol): the column workgroups (i, s), i >= s, first
// apply update s - 1 to what they own - A_ss (every one of them, as chol32(A_ss) is redundant)
// and A_is - and then do the panel's work; the trailing workgroups (i, j), s < j <= i, apply
// update s - 1 to the rest. Column s is touched by its column workgroups only, the trailing
// ones read column s - 1 and write columns > s, so no block is read in the launch that writes
// it and every block still takes its updates in the order 0, 1, 2, ... with the arithmetic of
// k_chol_update / k_chol_panel (same bits). The updated A_ss stays in LDS: nothing reads a
// diagonal block of A64 after its own launch (the solves refill A64 per evaluation).
//
// Workgroup id -> (problem, i, j), every problem's column workgroups first so the chain's
// blocks are dispatched ahead of the trailing ones. Host-callable for the map test.
struct CholStepWork { int prob, i, j; };   // j == s: column workgroup, j > s: trailing
__host__ __device__ inline int chol_step_cols(int s, int maxnbk) { return maxnbk - s; }
__host__ __device__ inline int chol_step_trail(int s, int maxnbk) {
  const int n = maxnbk - s - 1;
  return s > 0 ? n * (n + 1) / 2 : 0;
}
__host__ __device__ inline CholStepWork chol_step_work(int s, int maxnbk, int nprob, int id) {
  const int ncol = chol_step_cols(s, maxnbk);
  CholStepWork w;
  if (id < ncol * nprob) {
    w.prob = id / ncol;
    w.i = s + id % ncol;
    w.j = s;
    return w;
  }
  const int e = id - ncol * nprob, ntr = chol_step_trail(s, maxnbk);
  w.prob = e / ntr;
  const int q = e % ntr;   // -> (ii, jj), 0 <= jj <= ii, row-major lower triangle
  int ii = (int)((sqrt(8.0 * q + 1.0) - 1.0) * 0.5);
  while ((ii + 1) * (ii + 2) / 2 <= q) ++ii;
  while (ii * (ii + 1) / 2 > q) --ii;
  w.i = s + 1 + ii;
  w.j = s + 1 + (q - ii * (ii + 1) / 2);
  return w;
}

__global__ __launch_bounds__(256) void k_chol_step(const ProbDesc* __restrict__ probs, int s, int maxnbk, int nprob) {
  const CholStepWork w = chol_step_work(s, maxnbk, nprob, blockIdx.x);
  const ProbDesc& p = probs[w.prob];
  const int i = w.i, j = w.j, ldm = p.ldm;
  if (i >= p.nbk) return;   // (i >= j >= s: a problem with nbk <= s does nothing)
  __shared__ double b0[NB * LS], b1[NB * LS], b2[NB * LS];
  __shared__ int err;
  const int r = threadIdx.x >> 3, cb = (threadIdx.x & 7) * 4;
  if (j > s) {   // trailing: A_ij -= L_{i,s-1} L_{j,s-1}^T
    load_block(b0, p.A64, ldm, i, s - 1);
    load_block(b1, p.A64, ldm, j, s - 1);
    __syncthreads();
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    mm_nt(b0, b1, acc);
    double* dst = p.A64 + (size_t)(i * NB + r) * ldm + j * NB + cb;
#pragma unroll
    for (int t = 0; t < 4; ++t) dst[t] -= acc[t];
    return;
  }
  // column: b0 = A_ss -> L_ss -> L_is, b1 = L_{s,s-1} -> L_ss^-1, b2 = L_{i,s-1} -> A_is
  if (threadIdx.x == 0) err = 0;
  double rs[4], rp[4], rl[4];
  load_regs(rs, p.A64, ldm, s, s);
  if (s > 0) {
    load_regs(rp, p.A64, ldm, s, s - 1);
    if (i != s) load_regs(rl, p.A64, ldm, i, s - 1);
  }
  // A_is by strips of 4, held by waves 1..3 (strip st: row st >> 3, columns (st & 7) * 4 ..)
  // while wave 0 factors: threads 64..127 hold two strips
  double v[2][4];
  if (i != s && threadIdx.x >= 64) {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int st = threadIdx.x - 64 + 192 * m;
      if (st < 256) {
        const double* src = p.A64 + (size_t)(i * NB + (st >> 3)) * ldm + s * NB + (st & 7) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[m][q] = src[q];
      }
    }
  }
  store_regs(b0, rs);
  if (s > 0) {
    store_regs(b1, rp);
    if (i != s) store_regs(b2, rl);
  }
  __syncthreads();
  if (s > 0) {   // A_ss -= L_{s,s-1} L_{s,s-1}^T: the one product added in front of the chain
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    mm_nt(b1, b1, acc);
#pragma unroll
    for (int q = 0; q < 4; ++q) b0[r * LS + cb + q] -= acc[q];
    __syncthreads();
  }
  if (threadIdx.x < 64) {
    chol32_wave(b0, &err);
  } else if (i != s && s > 0) {   // A_is -= L_{i,s-1} L_{s,s-1}^T beside the factorisation
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int st = threadIdx.x - 64 + 192 * m;
      if (st < 256) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        mm_nt_at(b2, b1, acc, st >> 3, (st & 7) * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[m][q] -= acc[q];
      }
    }
  }
  __syncthreads();   // L_ss is in b0; b1 and b2 have been read
  if (i == s) {
    if (err && threadIdx.x == 0) p.flags[2] = 1;
    store_block(p.D64, NB, s, 0, b0);
    return;
  }
  if (threadIdx.x < NB) {
    trinv32_cols(b0, b1);   // b1 = L_ss^-1
  } else if (threadIdx.x >= 64) {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int st = threadIdx.x - 64 + 192 * m;
      if (st < 256) {
#pragma unroll
        for (int q = 0; q < 4; ++q) b2[(st >> 3) * LS + (st & 7) * 4 + q] = v[m][q];
      }
    }
  }
  __syncthreads();
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  mm_nt(b2, b1, acc);                // L_is = A_is * (L_ss^-1)^T
#pragma unroll
  for (int q = 0; q < 4; ++q) b0[r * LS + cb + q] = acc[q];   // (b0 = L_ss was read by wave 0 only, before the barrier)
  __syncthreads();
  store_block(p.A64, ldm, i, s, b0);
}

__global__ __launch_bounds__(256) void k_linv_row(const ProbDesc* __restrict__ probs, int i) {
  const ProbDesc& p = probs[blockIdx.y];
  const int j = blockIdx.x;
  if (i >= p.nbk || j > i) return;
  __shared__ double lii[NB * LS], xi[NB * LS], ta[NB * LS], tb[NB * LS];
  load_block(lii, p.D64, NB, i, 0);
  __syncthreads();
  trinv32(lii, xi);
  if (j == i) {
    store_block(p.L64, p.ldm, i, i, xi);
    return;
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  // the blocks of step t + 1 are loaded into registers while step t multiplies
  double ra[4], rb[4];
  if (j < i) { load_regs(ra, p.A64, p.ldm, i, j); load_regs(rb, p.L64, p.ldm, j, j); }
  for (int t = j; t < i; ++t) {
    store_regs(ta, ra);   // L_it
    store_regs(tb, rb);   // Linv_tj
    __syncthreads();
    if (t + 1 < i) { load_regs(ra, p.A64, p.ldm, i, t + 1); load_regs(rb, p.L64, p.ldm, t + 1, j); }
    mm_nn(ta, tb, acc);
    __syncthreads();
  }
  const int r = threadIdx.x >> 3, cb = (threadIdx.x & 7) * 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) ta[r * LS + cb + q] = acc[q];
  __syncthreads();
  double out[4] = {0.0, 0.0, 0.0, 0.0};
  mm_nn(xi, ta, out);                     // Linv_ii * S
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) tb[r * LS + cb + q] = -out[q];
  __syncthreads();
  store_block(p.L64, p.ldm, i, j, tb);
}

// Diagonal blocks of Linv: Linv_ii = L_ii^-1, all i of all problems in one launch.
__global__ __launch_bounds__(256) void k_diag_inv(const ProbDesc* __restrict__ probs) {
  const ProbDesc& p = probs[blockIdx.y];
  const int i = blockIdx.x;
  if (i >= p.nbk) return;
  __shared__ double lii[NB * LS], xi[NB * LS];
  load_block(lii, p.D64, NB, i, 0);
  __syncthreads();
  trinv32(lii, xi);
  store_block(p.L64, p.ldm, i, i, xi);
}

// Off-diagonal blocks of Linv by column slices: the columns of Linv are independent
// forward substitutions, so one workgroup owns a 4-column slice of block column j and
// produces its blocks i = j+1 .. nbk-1 with the finished ones kept in LDS:
//   Linv_ij = -Linv_ii S_i,   S_i = sum_{t=j}^{i-1} L_it Linv_tj
// One launch replaces the nbk dependent row launches. Right-looking: as soon as block t
// of the slice is final, every pending S_i (i > t) takes its L_it Linv_tj term. The
// 1024 threads are 8 groups of 128; group g owns the S_i with i = j+1+g (mod 8) in
// registers (thread (r, c) of a group: row r, slice column c), so per block t the
// pending products run 8 wide and the serial chain is ~1/8 of the slice's work.
// Sums run over t, then k, in order (the row-launch order).
constexpr int kLinvCols = 4;
constexpr int kLinvGroups = 8;
constexpr int kLinvMaxNbk = 56;   // LDS panel: nbk x 32 x 4 doubles (56 KB at the cap)
constexpr int kLinvPer = (kLinvMaxNbk + kLinvGroups - 1) / kLinvGroups;
__global__ __launch_bounds__(1024) void k_linv_cols(const ProbDesc* __restrict__ probs) {
  // grid ((maxnbk-1) * nsl, nprob). Measured: a j-major grid (every problem's long small-j
  // slices dispatched together) is 3x slower - the 8 slices of a block column each stream
  // the same L rows, and all of them at once thrash L2.
  const ProbDesc& p = probs[blockIdx.y];
  constexpr int nsl = NB / kLinvCols;
  const int j = blockIdx.x / nsl, c0 = (blockIdx.x % nsl) * kLinvCols;
  const int nbk = p.nbk, ldm = p.ldm;
  if (j >= nbk - 1) return;
  // dynamic LDS: panel [maxnbk][32][4] (block rows t >= j used), then sbuf [32][4]
  extern __shared__ double linv_lds[];
  double* panel = linv_lds;
  double* sbuf = linv_lds + (size_t)(gridDim.x / nsl + 1) * NB * kLinvCols;
  const int g = threadIdx.x >> 7, lt = threadIdx.x & 127;
  const int r = lt >> 2, c = lt & 3;
  const double* A64 = p.A64;
  double* L64 = p.L64;
  if (g == 0)   // block (j, j) of the slice: Linv_jj, written by k_diag_inv
    panel[(j * NB + r) * kLinvCols + c] = L64[(size_t)(j * NB + r) * ldm + j * NB + c0 + c];
  double acc[kLinvPer];
#pragma unroll
  for (int q = 0; q < kLinvPer; ++q) acc[q] = 0.0;
  __syncthreads();
  for (int t = j; t < nbk - 1; ++t) {
    const double* pt = panel + t * NB * kLinvCols + c;
    // pending S_i of this group, i = j + 1 + g + 8q > t
#pragma unroll
    for (int q = 0; q < kLinvPer; ++q) {
      const int i = j + 1 + g + kLinvGroups * q;
      if (i > t && i < nbk) {
        const double2* lp = reinterpret_cast<const double2*>(A64 + (size_t)(i * NB + r) * ldm + t * NB);
        double a = acc[q];
#pragma unroll
        for (int k = 0; k < NB; k += 2) {
          const double2 x = lp[k / 2];
          a += x.x * pt[k * kLinvCols];
          a += x.y * pt[(k + 1) * kLinvCols];
        }
        acc[q] = a;
      }
    }
    // S_{t+1} is complete: its owner group publishes it, then forms Linv_{t+1, j}
    const int i = t + 1;
    const int og = (i - j - 1) % kLinvGroups, oq = (i - j - 1) / kLinvGroups;
    if (g == og) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < kLinvPer; ++q) v = q == oq ? acc[q] : v;
      sbuf[r * kLinvCols + c] = v;
    }
    __syncthreads();
    if (g == og) {
      const double2* dp = reinterpret_cast<const double2*>(L64 + (size_t)(i * NB + r) * ldm + i * NB);
      double o = 0.0;
#pragma unroll
      for (int k = 0; k < NB; k += 2) {
        const double2 d = dp[k / 2];
        o += d.x * sbuf[k * kLinvCols + c];
        o += d.y * sbuf[(k + 1) * kLinvCols + c];
      }
      panel[(i * NB + r) * kLinvCols + c] = -o;
      L64[(size_t)(i * NB + r) * ldm + j * NB + c0 + c] = -o;
    }
    __syncthreads();   // block i of the panel is read by every group next step; sbuf is rewritten
  }
}

// The same with groups of one wave (kSpdWideLinv): 512 threads, lane (r, c) of a group owns
// row r and one half of the slice's W columns, so a row of L_it is loaded by two lanes instead
// of four and a lane runs W / 2 independent chains. k_linv_cols (124 registers x 1024 threads)
// has a CU to itself, and the batched launch is short of resident slices, not of flops: at
// W = 4 and at most 5 pending S per group (CAP = kLinvMidNbk blocks) this form fits the 128
// registers of 4 waves per SIMD, so two workgroups share a CU - the form the launcher takes
// (C3: 601 -> 442 us). W = 8 and 16 (a block column's L rows streamed by 4 or 2 workgroups
// instead of 8) need 172 / 242 registers, one workgroup per CU, and measured slower; they are
// reachable through admmq_debug_set_linv_width only. The owner group's
// Linv_ii row (its first half) is loaded before the barrier that publishes S. Every element's
// chain is the one above (t, then k, ascending from 0; same bits). The LDS panel is
// (maxnbk + 1) x 32 x W doubles: W = 16 up to kLinvMaxNbk16 blocks, W = 8 up to kLinvMaxNbk.
constexpr int kLinvMaxNbk16 = 38;   // 39 x 32 x 16 doubles = 156 KB of the CU's 160 KB
constexpr int kLinvWideThreads = 64 * kLinvGroups;
constexpr int kLinvMidNbk = 40;     // W = 4: a group has at most 5 pending S (7 up to kLinvMaxNbk: 36 B of scratch)
template <int W, int CAP>
__global__ __launch_bounds__(kLinvWideThreads, W == 4 ? 4 : 2) void k_linv_cols_w(const ProbDesc* __restrict__ probs) {
  // grid ((maxnbk-1) * nsl, nprob): long columns first, as above
  constexpr int nsl = NB / W, kCpt = W / 2, kPer = (CAP + kLinvGroups - 1) / kLinvGroups;
  const ProbDesc& p = probs[blockIdx.y];
  const int j = blockIdx.x / nsl, c0 = (blockIdx.x % nsl) * W;
  const int nbk = p.nbk, ldm = p.ldm;
  if (j >= nbk - 1) return;
  extern __shared__ double linv_lds[];
  double* panel = linv_lds;
  double* sbuf = linv_lds + (size_t)(gridDim.x / nsl + 1) * NB * W;
  const int g = threadIdx.x >> 6, lt = threadIdx.x & 63;
  const int r = lt >> 1, c = (lt & 1) * kCpt;
  const double* A64 = p.A64;
  double* L64 = p.L64;
  if (g == 0) {
#pragma unroll
    for (int m = 0; m < kCpt; ++m)
      panel[(j * NB + r) * W + c + m] = L64[(size_t)(j * NB + r) * ldm + j * NB + c0 + c + m];
  }
  double acc[kPer][kCpt];
#pragma unroll
  for (int q = 0; q < kPer; ++q)
#pragma unroll
    for (int m = 0; m < kCpt; ++m) acc[q][m] = 0.0;
  __syncthreads();
  for (int t = j; t < nbk - 1; ++t) {
    const double* pt = panel + t * NB * W + c;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int i = j + 1 + g + kLinvGroups * q;
      if (i > t && i < nbk) {
        const double2* lp = reinterpret_cast<const double2*>(A64 + (size_t)(i * NB + r) * ldm + t * NB);
#pragma unroll
        for (int h = 0; h < 2; ++h) {   // the row in two halves (registers); per element k ascending
          double2 x[NB / 4];
#pragma unroll
          for (int k = 0; k < NB / 4; ++k) x[k] = lp[h * (NB / 4) + k];
#pragma unroll
          for (int k = 0; k < NB / 2; k += 2) {
#pragma unroll
            for (int m = 0; m < kCpt; ++m) acc[q][m] += x[k / 2].x * pt[(h * (NB / 2) + k) * W + m];
#pragma unroll
            for (int m = 0; m < kCpt; ++m) acc[q][m] += x[k / 2].y * pt[(h * (NB / 2) + k + 1) * W + m];
          }
        }
      }
    }
    const int i = t + 1;
    const int og = (i - j - 1) % kLinvGroups, oq = (i - j - 1) / kLinvGroups;
    double2 d[NB / 2];
    const double2* dp = reinterpret_cast<const double2*>(L64 + (size_t)(i * NB + r) * ldm + i * NB);
    if (g == og) {
#pragma unroll
      for (int k = 0; k < NB / 4; ++k) d[k] = dp[k];   // the first half in flight across the barrier
#pragma unroll
      for (int m = 0; m < kCpt; ++m) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < kPer; ++q) v = q == oq ? acc[q][m] : v;
        sbuf[r * W + c + m] = v;
      }
    }
    __syncthreads();
    if (g == og) {
#pragma unroll
      for (int k = NB / 4; k < NB / 2; ++k) d[k] = dp[k];
      double o[kCpt];
#pragma unroll
      for (int m = 0; m < kCpt; ++m) o[m] = 0.0;
#pragma unroll
      for (int k = 0; k < NB; k += 2) {
#pragma unroll
        for (int m = 0; m < kCpt; ++m) o[m] += d[k / 2].x * sbuf[k * W + c + m];
#pragma unroll
        for (int m = 0; m < kCpt; ++m) o[m] += d[k / 2].y * sbuf[(k + 1) * W + c + m];
      }
#pragma unroll
      for (int m = 0; m < kCpt; ++m) {
        panel[(i * NB + r) * W + c + m] = -o[m];
        L64[(size_t)(i * NB + r) * ldm + j * NB + c0 + c + m] = -o[m];
      }
    }
    __syncthreads();
  }
}

// k_minv with a 2 x 4 register tile (kSpdTileMinv): threads 0..127 hold rows 2 rp, 2 rp + 1 and
// four columns, 6 LDS reads per 8 products instead of 5 per 4; all 256 threads still move the
// blocks. Each element's sum runs over t, then k, ascending from 0, as in k_minv (same bits).
__global__ __launch_bounds__(256) void k_minv_tile(const ProbDesc* __restrict__ probs) {
  const ProbDesc& p = probs[blockIdx.y];
  const int q = blockIdx.x;
  const int n = p.nbk;
  if (q >= n * (n + 1) / 2) return;
  int i = (int)((sqrt(8.0 * q + 1.0) - 1.0) * 0.5);
  while ((i + 1) * (i + 2) / 2 <= q) ++i;
  while (i * (i + 1) / 2 > q) --i;
  const int j = q - i * (i + 1) / 2;      // j <= i
  __shared__ double ta[NB * LS], tb[NB * LS];
  const int r0 = ((threadIdx.x >> 3) & 15) * 2, cb = (threadIdx.x & 7) * 4;
  double acc[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
  double ra[4], rb[4];
  load_regs(ra, p.L64, p.ldm, i, i);
  load_regs(rb, p.L64, p.ldm, i, j);
  for (int t = i; t < n; ++t) {
    store_regs(ta, ra);   // Linv_ti
    store_regs(tb, rb);   // Linv_tj
    __syncthreads();
    if (t + 1 < n) { load_regs(ra, p.L64, p.ldm, t + 1, i); load_regs(rb, p.L64, p.ldm, t + 1, j); }
    if (threadIdx.x < 128) {
      for (int k = 0; k < NB; ++k) {
        const double a0 = ta[k * LS + r0], a1 = ta[k * LS + r0 + 1];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const double bv = tb[k * LS + cb + m];
          acc[0][m] += a0 * bv;
          acc[1][m] += a1 * bv;
        }
      }
    }
    __syncthreads();
  }
  if (threadIdx.x >= 128) return;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int gr = i * NB + r0 + h;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int gc = j * NB + cb + t;
      const float v = (gr < p.R && gc < p.R) ? (float)acc[h][t] : 0.f;
      p.M[(size_t)gr * p.ldm + gc] = v;
      p.M[(size_t)gc * p.ldm + gr] = v;
    }
  }
}

__global__ __launch_bounds__(256) void k_minv(const ProbDesc* __restrict__ probs) {
  const ProbDesc& p = probs[blockIdx.y];
  const int q = blockIdx.x;
  const int n = p.nbk;
  if (q >= n * (n + 1) / 2) return;
  int i = (int)((sqrt(8.0 * q + 1.0) - 1.0) * 0.5);
  while ((i + 1) * (i + 2) / 2 <= q) ++i;
  while (i * (i + 1) / 2 > q) --i;
  const int j = q - i * (i + 1) / 2;      // j <= i
  __shared__ double ta[NB * LS], tb[NB * LS];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  double ra[4], rb[4];
  load_regs(ra, p.L64, p.ldm, i, i);
  load_regs(rb, p.L64, p.ldm, i, j);
  for (int t = i; t < n; ++t) {
    store_regs(ta, ra);   // Linv_ti
    store_regs(tb, rb);   // Linv_tj
    __syncthreads();
    if (t + 1 < n) { load_regs(ra, p.L64, p.ldm, t + 1, i); load_regs(rb, p.L64, p.ldm, t + 1, j); }
    mm_tn(ta, tb, acc);
    __syncthreads();
  }
  const int r = threadIdx.x >> 3, cb = (threadIdx.x & 7) * 4;
  const int gr = i * NB + r;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int gc = j * NB + cb + t;
    const float v = (gr < p.R && gc < p.R) ? (float)acc[t] : 0.f;
    p.M[(size_t)gr * p.ldm + gc] = v;
    p.M[(size_t)gc * p.ldm + gr] = v;
  }
}

// Which forms the launchers take (admmq_debug_set_spd_form; same bits either way) and the
// slice width k_linv_cols_w is held to (admmq_debug_set_linv_width: 8 or 16; 0 = the launcher's own form)
static std::atomic<int> g_spd_form{kSpdFormDefault};
static std::atomic<int> g_linv_width{0};

// Form of the L^-1 column kernel for a launch: 4 is k_linv_cols, 2 / 8 / 16 are k_linv_cols_w
static int linv_width(int maxnbk) {
  if (!(g_spd_form.load() & kSpdWideLinv)) return kLinvCols;
  const int w = g_linv_width.load();
  if (w == 16 && maxnbk <= kLinvMaxNbk16) return 16;
  if (w == 8 || w == 16) return 8;
  return maxnbk <= kLinvMidNbk ? 2 : kLinvCols;   // 2: 4-column slices, two columns per lane
}

template <int W, int CAP>
static void launch_linv_cols_w(const ProbDesc* d, int nprob, int maxnbk, hipStream_t s) {
  const size_t lds = (size_t)(maxnbk + 1) * NB * W * sizeof(double);
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_linv_cols_w<W, CAP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
  hipLaunchKernelGGL((k_linv_cols_w<W, CAP>), dim3((maxnbk - 1) * (NB / W), nprob), dim3(kLinvWideThreads), lds, s, d);
}

// L (lower, in A64) and Linv = L^-1 (lower blocks of L64; the upper off-diagonal blocks are
// not written) of A64 = L L^T; flags[2] on a non-positive pivot. Every launch reads the block
// count from the descriptor, so a descriptor whose nbk is 0 turns them all into no-ops (the
// blocked EPC step's rounds after its search is done, solve64.hip).
void launch_spd_linv(const ProbDesc* d, int nprob, int maxnbk, hipStream_t s) {
  if (g_spd_form.load() & kSpdFusedChol) {
    for (int k = 0; k < maxnbk; ++k) {
      const int nwg = nprob * (chol_step_cols(k, maxnbk) + chol_step_trail(k, maxnbk));
      hipLaunchKernelGGL(k_chol_step, dim3(nwg), dim3(256), 0, s, d, k, maxnbk, nprob);
    }
  } else {
    for (int k = 0; k < maxnbk; ++k) {
      hipLaunchKernelGGL(k_chol_panel, dim3(maxnbk - k, nprob), dim3(256), 0, s, d, k);
      const int n = maxnbk - k - 1;
      if (n > 0) hipLaunchKernelGGL(k_chol_update, dim3(n * (n + 1) / 2, nprob), dim3(256), 0, s, d, k);
    }
  }
  if (maxnbk <= kLinvMaxNbk) {
    hipLaunchKernelGGL(k_diag_inv, dim3(maxnbk, nprob), dim3(256), 0, s, d);
    if (maxnbk > 1) {
      const int w = linv_width(maxnbk);
      if (w == 16) launch_linv_cols_w<16, kLinvMaxNbk16>(d, nprob, maxnbk, s);
      else if (w == 8) launch_linv_cols_w<8, kLinvMaxNbk>(d, nprob, maxnbk, s);
      else if (w == 2) launch_linv_cols_w<4, kLinvMidNbk>(d, nprob, maxnbk, s);
      else
        hipLaunchKernelGGL(k_linv_cols, dim3((maxnbk - 1) * (NB / kLinvCols), nprob), dim3(1024),
                           (size_t)(maxnbk + 1) * NB * kLinvCols * sizeof(double), s, d);
    }
  } else {   // panel would not fit in LDS: one launch per block row
    for (int i = 0; i < maxnbk; ++i) hipLaunchKernelGGL(k_linv_row, dim3(i + 1, nprob), dim3(256), 0, s, d, i);
  }
}

void launch_spd_inverse(const ProbDesc* d, int nprob, int maxnbk, hipStream_t s) {
  launch_spd_linv(d, nprob, maxnbk, s);
  const dim3 grid(maxnbk * (maxnbk + 1) / 2, nprob);
  if (g_spd_form.load() & kSpdTileMinv) hipLaunchKernelGGL(k_minv_tile, grid, dim3(256), 0, s, d);
  else hipLaunchKernelGGL(k_minv, grid, dim3(256), 0, s, d);
}

// A64 = G + shift I in fp64 (G: R x R fp64), identity past R (admmq_debug_spd_inverse)
__global__ __launch_bounds__(256) void k_spd_debug_fill(const ProbDesc* __restrict__ probs, const double* const* __restrict__ G,
                                                        double shift) {
  const ProbDesc& p = probs[blockIdx.y];
  const double* g = G[blockIdx.y];
  const long long total = (long long)p.ldm * p.ldm;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int r = (int)(e / p.ldm), c = (int)(e - (long long)r * p.ldm);
    double v;
    if (r < p.R && c < p.R) v = g[(size_t)r * p.R + c] + (r == c ? shift : 0.0);
    else v = r == c ? 1.0 : 0.0;
    p.A64[e] = v;
  }
}

}  // namespace admmq

using namespace admmq;

extern "C" {

// diagnostics (not in include/admmq.h): which forms of the SPD inverse run (kSpd* bits,
// admmq_internal.h; default kSpdFormDefault, 0 = the two-launch Cholesky, the 4-column
// slices and the strip k_minv; same bits either way)
int32_t admmq_debug_set_spd_form(int32_t mask) {
  if (mask < 0 || (mask & ~kSpdFormAll)) return set_error(ADMMQ_ERR_ARG, "spd form mask out of range");
  g_spd_form = mask;
  return ADMMQ_OK;
}
int32_t admmq_debug_get_spd_form_default(void) { return kSpdFormDefault; }
// diagnostics: the slice width of the wide L^-1 column kernel, 8 or 16 (16 only where its
// panel fits), 0 = chosen from the launch's block count
int32_t admmq_debug_set_linv_width(int32_t w) {
  if (w != 0 && w != 8 && w != 16) return set_error(ADMMQ_ERR_ARG, "linv width must be 0, 8 or 16");
  g_linv_width = w;
  return ADMMQ_OK;
}
// diagnostics: the slice width launch_spd_linv takes at maxnbk under the current switches
int32_t admmq_debug_linv_width(int32_t maxnbk) { return maxnbk >= 2 && maxnbk <= kLinvMaxNbk ? linv_width(maxnbk) : 0; }

// diagnostics: workgroup `id` of k_chol_step(s) for a batch with block counts nbk[nprob]:
// out = {problem, i, j} (j == s: a column workgroup, j > s: a trailing one); returns the
// launch's workgroup count, or -1 on bad arguments; out[0] = -1 for a workgroup that returns
// at once (its problem has fewer blocks). Host code only.
int32_t admmq_debug_chol_step_work(int32_t s, int32_t nprob, const int32_t* nbk, int32_t id, int32_t* out) {
  if (!nbk || !out || nprob < 1 || s < 0) return -1;
  int maxnbk = 0;
  for (int q = 0; q < nprob; ++q) maxnbk = std::max(maxnbk, nbk[q]);
  if (s >= maxnbk) return -1;
  const int nwg = nprob * (chol_step_cols(s, maxnbk) + chol_step_trail(s, maxnbk));
  if (id < 0 || id >= nwg) return -1;
  const CholStepWork w = chol_step_work(s, maxnbk, nprob, id);
  const bool on = w.i < nbk[w.prob];
  out[0] = on ? w.prob : -1; out[1] = w.i; out[2] = w.j;
  return nwg;
}

// diagnostics: M = (G + shift I)^-1 of nprob standalone problems in one batched
// launch_spd_inverse, as the ADMM prepare runs it. Host pointers: G[q] is R[q] x R[q] fp64;
// per problem, with ldm = 32 ceil(R / 32): M (ldm x ldm fp32), A (ldm x ldm: L in the strictly
// lower blocks), Linv (ldm x ldm: the lower blocks), D (ldm x 32: the diagonal L blocks),
// flags2 (a non-positive pivot). ms: the device time of the last of `reps` inverses.
int32_t admmq_debug_spd_inverse(int32_t nprob, const int32_t* R, const double* const* G, double shift, float* const* M,
                                double* const* A, double* const* Linv, double* const* D, int32_t* flags2, int32_t reps,
                                float* ms) {
  if (nprob < 1 || nprob > 64 || !R || !G || reps < 1) return set_error(ADMMQ_ERR_ARG, "spd_inverse: bad arguments");
  std::vector<ProbDesc> desc(nprob);
  std::vector<const double*> dG(nprob);
  std::vector<void*> owned;
  auto dev = [&](size_t bytes) -> void* {
    void* q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) return nullptr;
    owned.push_back(q);
    return q;
  };
  auto done = [&](int rc, const char* msg) {
    (void)hipDeviceSynchronize();
    for (void* q : owned) (void)hipFree(q);
    return rc == ADMMQ_OK ? rc : set_error(rc, msg);
  };
  int maxnbk = 0, maxldm = 0;
  int* dflags = static_cast<int*>(dev((size_t)nprob * 4 * sizeof(int)));
  if (!dflags || hipMemset(dflags, 0, (size_t)nprob * 4 * sizeof(int)) != hipSuccess) return done(ADMMQ_ERR_HIP, "spd_inverse: alloc");
  for (int q = 0; q < nprob; ++q) {
    if (R[q] < 1 || R[q] > 8192 || !G[q]) return done(ADMMQ_ERR_ARG, "spd_inverse: bad problem");
    ProbDesc& d = desc[q];
    std::memset(&d, 0, sizeof(d));
    d.R = R[q]; d.ldm = (R[q] + NB - 1) / NB * NB; d.nbk = d.ldm / NB;
    const size_t l2 = (size_t)d.ldm * d.ldm;
    d.A64 = static_cast<double*>(dev(l2 * 8));
    d.L64 = static_cast<double*>(dev(l2 * 8));
    d.D64 = static_cast<double*>(dev((size_t)d.ldm * NB * 8));
    d.M = static_cast<float*>(dev(l2 * 4));
    double* g = static_cast<double*>(dev((size_t)R[q] * R[q] * 8));
    d.flags = dflags + 4 * q;
    if (!d.A64 || !d.L64 || !d.D64 || !d.M || !g) return done(ADMMQ_ERR_HIP, "spd_inverse: alloc");
    if (hipMemset(d.L64, 0, l2 * 8) != hipSuccess || hipMemset(d.M, 0, l2 * 4) != hipSuccess ||
        hipMemcpy(g, G[q], (size_t)R[q] * R[q] * 8, hipMemcpyHostToDevice) != hipSuccess)
      return done(ADMMQ_ERR_HIP, "spd_inverse: upload");
    dG[q] = g;
    maxnbk = std::max(maxnbk, d.nbk);
    maxldm = std::max(maxldm, d.ldm);
  }
  ProbDesc* ddesc = static_cast<ProbDesc*>(dev(nprob * sizeof(ProbDesc)));
  const double** ddG = static_cast<const double**>(dev(nprob * sizeof(double*)));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!ddesc || !ddG || hipMemcpy(ddesc, desc.data(), nprob * sizeof(ProbDesc), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(ddG, dG.data(), nprob * sizeof(double*), hipMemcpyHostToDevice) != hipSuccess ||
      hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
    return done(ADMMQ_ERR_HIP, "spd_inverse: upload");
  const int fb = (int)std::min<long long>(1024, ((long long)maxldm * maxldm + 255) / 256);
  for (int it = 0; it < reps; ++it) {
    hipLaunchKernelGGL(k_spd_debug_fill, dim3(fb, nprob), dim3(256), 0, nullptr, ddesc, ddG, shift);
    (void)hipEventRecord(e0, nullptr);
    launch_spd_inverse(ddesc, nprob, maxnbk, nullptr);
    (void)hipEventRecord(e1, nullptr);
  }
  float t = 0.f;
  bool ok = hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (ms) *ms = t;
  std::vector<int> hf((size_t)nprob * 4);
  ok = ok && hipMemcpy(hf.data(), dflags, hf.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
  for (int q = 0; ok && q < nprob; ++q) {
    const ProbDesc& d = desc[q];
    const size_t l2 = (size_t)d.ldm * d.ldm;
    if (flags2) flags2[q] = hf[4 * q + 2];
    if (M && M[q]) ok = ok && hipMemcpy(M[q], d.M, l2 * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (A && A[q]) ok = ok && hipMemcpy(A[q], d.A64, l2 * 8, hipMemcpyDeviceToHost) == hipSuccess;
    if (Linv && Linv[q]) ok = ok && hipMemcpy(Linv[q], d.L64, l2 * 8, hipMemcpyDeviceToHost) == hipSuccess;
    if (D && D[q]) ok = ok && hipMemcpy(D[q], d.D64, (size_t)d.ldm * NB * 8, hipMemcpyDeviceToHost) == hipSuccess;
  }
  return done(ok ? ADMMQ_OK : ADMMQ_ERR_HIP, "spd_inverse: run failed");
}

}  // extern "C"

