/* Host AddressSanitizer / UBSan check of libadmmq's host code (optional
 * -fsanitize=address host build). Built by `make -C admm-quantization_amd/csrc asan`
 * against build/asan/libadmmq_asan.so, whose host code is instrumented (-Xarch_host
 * -fsanitize=address,undefined; device code untouched). Runs without a GPU: it drives the
 * host-only planners (workspace-size queries: problem layout, tile lists and their CU
 * ordering, stage-1 chunking, the finalize / small-job plans; the search form and the
 * run's launch schedule through admmq_debug_admm_run_schedule) over the bench configs
 * C3 / C4 / C5 and seeded random batches, the ALS planner through admmq_debug_cp_plan over
 * random CP batches, and the argument-validation error paths. Any
 * heap / stack overflow or UB in that code aborts with a sanitizer report.
 * usage: build/asan/asan_host_check   (exit 0 = clean) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../include/admmq.h"

static uint64_t rng = 88172645463325252ull;
static int rnd(int lo, int hi) { /* xorshift64, inclusive range */
  rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
  return lo + (int)(rng % (uint64_t)(hi - lo + 1));
}

/* diagnostics entry point (csrc/api.hip, not in admmq.h): the run's launch schedule */
int32_t admmq_debug_admm_run_schedule(const admmq_problem* probs, int32_t nprob, int32_t num_attempts, int32_t bits,
                                      int32_t qscheme, int32_t max_iter, int32_t solve_mode, int32_t fused_finalize,
                                      int32_t has_info, int32_t fin_capacity, int32_t out[16]);

/* diagnostics entry point (csrc/spd_kernels.hip, not in admmq.h): workgroup `id` of the fused
 * Cholesky launch s -> {problem or -1, i, j}; returns the launch's workgroup count or -1 */
int32_t admmq_debug_chol_step_work(int32_t s, int32_t nprob, const int32_t* nbk, int32_t id, int32_t* out);

static size_t ws_of(const int (*ir)[2], int n) {
  admmq_problem* p = calloc((size_t)n, sizeof(admmq_problem));
  for (int i = 0; i < n; ++i) { p[i].I = ir[i][0]; p[i].R = ir[i][1]; }
  size_t b = admmq_admm_workspace_size(p, n, 200);
  free(p);
  return b;
}

/* the search form and the launch schedule of the batch (host code only: the capacity of
 * the fused finalize is an argument), over the bit widths and candidate counts that take
 * the merged, per-level and exhaustive forms (24 combinations; a caller with many batches
 * takes every step-th from `first`); failures counted */
static int schedules_of(const int (*ir)[2], int n, int first, int step) {
  static const int bits[4] = {1, 4, 6, 8}, ncand[3] = {1, 200, 1100}, cap[3] = {0, 16, 512};
  admmq_problem* p = calloc((size_t)n, sizeof(admmq_problem));
  for (int i = 0; i < n; ++i) { p[i].I = ir[i][0]; p[i].R = ir[i][1]; }
  int bad = 0;
  for (int k = first; k < 24; k += step) {
    int32_t out[16] = {0};
    const int mse = k < 12;
    bad += admmq_debug_admm_run_schedule(p, n, ncand[k % 3], bits[k % 4], mse ? ADMMQ_TENSOR_MSEMINMAX_SYMMETRIC
                                                                             : ADMMQ_TENSOR_MINMAX,
                                         1 + k % 4, 0, k % 5 != 0, k % 7 != 0, cap[(k / 2) % 3], out) != ADMMQ_OK;
    bad += out[0] != k % 4 || out[10] < 0 || out[10] > out[15] || (!mse && out[6] != 0);
  }
  free(p);
  return bad;
}

int main(void) {
  int fails = 0;
  /* C3: resnet18 16 3x3 convs, every mode (I_m, R) */
  static const int r18[16][3] = {{64, 64, 134}, {64, 64, 134}, {64, 64, 134}, {64, 64, 134}, {128, 64, 183},
                                 {128, 128, 278}, {128, 128, 278}, {128, 128, 278}, {256, 128, 375},
                                 {256, 256, 566}, {256, 256, 566}, {256, 256, 566}, {512, 256, 759},
                                 {512, 512, 1141}, {512, 512, 1141}, {512, 512, 1141}};
  for (int m = 0; m < 3; ++m) {
    int ir[16][2];
    for (int l = 0; l < 16; ++l) { ir[l][0] = m == 2 ? 9 : r18[l][m]; ir[l][1] = r18[l][2]; }
    size_t b = ws_of((const int(*)[2])ir, 16);
    printf("C3 mode %d: workspace %zu B\n", m, b);
    fails += b == 0;
    fails += schedules_of((const int(*)[2])ir, 16, 0, 1);
  }
  /* C5: one Llama-7B decoder layer, both modes (the wide-tile plan) */
  static const int ll[7][3] = {{4096, 4096, 1024}, {4096, 4096, 1024}, {4096, 4096, 1024}, {4096, 4096, 1024},
                               {11008, 4096, 1492}, {11008, 4096, 1492}, {4096, 11008, 1492}};
  for (int m = 0; m < 2; ++m) {
    int ir[7][2];
    for (int l = 0; l < 7; ++l) { ir[l][0] = ll[l][m]; ir[l][1] = ll[l][2]; }
    size_t b = ws_of((const int(*)[2])ir, 7);
    printf("C5 mode %d: workspace %zu B\n", m, b);
    fails += b == 0;
    fails += schedules_of((const int(*)[2])ir, 7, 0, 1);
  }
  /* seeded random batches: thin (I <= 16), 32-row, 64x64 and wide mixes, ragged R */
  size_t tot = 0;
  for (int t = 0; t < 400; ++t) {
    int n = rnd(1, 48), ir[48][2];
    for (int i = 0; i < n; ++i) {
      const int cls = rnd(0, 3);
      ir[i][0] = cls == 0 ? rnd(1, 16) : (cls == 1 ? rnd(17, 32) : (cls == 2 ? rnd(33, 700) : rnd(700, 4096)));
      ir[i][1] = rnd(1, t % 50 == 0 ? 3000 : 1200);
    }
    size_t b = ws_of((const int(*)[2])ir, n);
    fails += b == 0;
    fails += schedules_of((const int(*)[2])ir, n, t % 4, 4);
    tot += b;
  }
  printf("400 random batches: total workspace %zu B\n", tot);
  /* quantizer planner: ragged tensors */
  for (int t = 0; t < 200; ++t) {
    admmq_qtensor q[8] = {0};
    const int n = rnd(1, 8);
    for (int i = 0; i < n; ++i) { q[i].rows = rnd(1, 3000); q[i].cols = rnd(1, 3000); }
    fails += admmq_quantize_workspace_size(q, n, rnd(1, 400)) == 0;
  }
  /* argument validation: each must fail cleanly (no device call is reached) */
  admmq_problem bad = {0};
  bad.I = 0; bad.R = 5;
  fails += admmq_admm_workspace_size(&bad, 1, 200) != 0;
  bad.I = 5; bad.R = -1;
  fails += admmq_admm_workspace_size(&bad, 1, 200) != 0;
  bad.I = 1 << 16; bad.R = 1 << 15;
  fails += admmq_admm_workspace_size(&bad, 1, 200) != 0;
  fails += admmq_admm_workspace_size(NULL, 3, 200) != 0;
  bad.I = 8; bad.R = 8;
  fails += admmq_admm_workspace_size(&bad, 1, 0) != 0;
  fails += admmq_admm_prepare(&bad, 1, 200, NULL, 0, NULL) == ADMMQ_OK;
  fails += admmq_quantize_batched(NULL, 1, 4, 99, 200, NULL, 0, NULL) != ADMMQ_ERR_SCHEME;
  /* the fused Cholesky launch's workgroup map (csrc/spd_kernels.hip chol_step_work): every
   * workgroup of every launch of random mixed batches lands on a block of its problem */
  for (int t = 0; t < 60; ++t) {
    int32_t nbk[8], out[3];
    const int n = rnd(1, 8);
    int maxnbk = 0;
    for (int i = 0; i < n; ++i) { nbk[i] = rnd(1, t % 10 == 0 ? 56 : 12); if (nbk[i] > maxnbk) maxnbk = nbk[i]; }
    for (int s = 0; s < maxnbk; ++s) {
      const int nwg = admmq_debug_chol_step_work(s, n, nbk, 0, out);
      fails += nwg <= 0;
      for (int id = 0; id < nwg; ++id) {
        fails += admmq_debug_chol_step_work(s, n, nbk, id, out) != nwg;
        fails += out[0] >= n || out[2] < s || out[1] < out[2] || out[1] >= maxnbk || (out[0] >= 0 && out[1] >= nbk[out[0]]);
      }
      fails += admmq_debug_chol_step_work(s, n, nbk, nwg, out) != -1;
    }
    fails += admmq_debug_chol_step_work(maxnbk, n, nbk, 0, out) != -1;
  }
  /* packed-weight GEMM: the planner over ragged sizes (a function of its arguments), then
   * every refusal of the entry point (made-up device addresses: nothing may be launched) */
  for (int t = 0; t < 400; ++t) {
    const int64_t M = rnd(1, 6000), K = rnd(1, 6000), N = rnd(1, t % 3 ? 70 : 4000);
    const int32_t nb = rnd(1, 8);
    fails += admmq_packed_gemm_workspace_size(M, K, N, nb) != admmq_packed_gemm_workspace_size(M, K, N, nb);
  }
  fails += admmq_packed_gemm_workspace_size(512, 1141, 4, 1) == 0;
  fails += admmq_packed_gemm_workspace_size(0, 8, 8, 1) != 0;
  fails += admmq_packed_gemm_workspace_size(8, -1, 8, 1) != 0;
  fails += admmq_packed_gemm_workspace_size(8, 8, 8, 0) != 0;
  fails += admmq_packed_gemm_workspace_size((int64_t)1 << 40, 8, 8, 1) != 0;
  {
    const uint8_t* c = (const uint8_t*)0x1000;
    const float* x = (const float*)0x10000;
    float* y = (float*)0x20000;
    void* ws = (void*)0x100000;
    admmq_qmeta qm = {ADMMQ_TENSOR_MSEMINMAX_SYMMETRIC, 4, 0.125f, 0, 0.f, 0.f, -1, 0}, q2;
    fails += admmq_packed_gemm(NULL, &qm, 0, 8, 8, x, 0, 4, 1, NULL, y, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
    fails += admmq_packed_gemm(c, NULL, 0, 8, 8, x, 0, 4, 1, NULL, y, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
    fails += admmq_packed_gemm(c, &qm, 0, 8, 8, NULL, 0, 4, 1, NULL, y, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
    fails += admmq_packed_gemm(c, &qm, 0, 8, 8, x, 0, 4, 1, NULL, NULL, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
    fails += admmq_packed_gemm(c, &qm, 0, 0, 8, x, 0, 4, 1, NULL, y, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
    fails += admmq_packed_gemm(c, &qm, 0, 8, 8, x, 0, -4, 1, NULL, y, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
    fails += admmq_packed_gemm(c, &qm, 0, 8, 8, x, 1, 4, 2, NULL, y, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
    fails += admmq_packed_gemm(c + 4, &qm, 0, 8, 8, x, 0, 4, 1, NULL, y, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
    q2 = qm; q2.bits = 9;
    fails += admmq_packed_gemm(c, &q2, 0, 8, 8, x, 0, 4, 1, NULL, y, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
    q2 = qm; q2.scheme = 7;
    fails += admmq_packed_gemm(c, &q2, 0, 8, 8, x, 0, 4, 1, NULL, y, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
    q2 = qm; q2.scheme = ADMMQ_TENSOR_MINMAX; q2.bits = 1;
    fails += admmq_packed_gemm(c, &q2, 0, 8, 8, x, 0, 4, 1, NULL, y, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
    q2 = qm; q2.bad = 3;
    fails += admmq_packed_gemm(c, &q2, 0, 8, 8, x, 0, 4, 1, NULL, y, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
    fails += admmq_packed_gemm(c, &qm, 0, 512, 1141, x, 0, 4, 1, NULL, y, ws, 16, NULL) != ADMMQ_ERR_WORKSPACE;
    fails += admmq_packed_gemm(c, &qm, 0, 512, 1141, x, 0, 4, 1, NULL, y, NULL, 0, NULL) != ADMMQ_ERR_WORKSPACE;
    /* the quant + low-rank GEMM: the workspace always holds t (at least the GEMM's images and
     * 4 r N bytes), and every refusal before any launch */
    {
      const float* lf = (const float*)0x30000;
      const float* rt = (const float*)0x40000;
      for (int t = 0; t < 400; ++t) {
        const int64_t M = rnd(1, 6000), K = rnd(1, 6000), N = rnd(1, t % 3 ? 70 : 4000);
        const int32_t r = rnd(1, 256);
        const size_t w = admmq_packed_lrgemm_workspace_size(M, K, N, r);
        fails += w != admmq_packed_lrgemm_workspace_size(M, K, N, r);
        fails += w < admmq_packed_gemm_workspace_size(M, K, N, 1) + (size_t)4 * r * N;
      }
      fails += admmq_packed_lrgemm_workspace_size(0, 8, 8, 4) != 0;
      fails += admmq_packed_lrgemm_workspace_size(8, 8, -1, 4) != 0;
      fails += admmq_packed_lrgemm_workspace_size(8, 8, 8, 0) != 0;
      fails += admmq_packed_lrgemm_workspace_size(8, 8, 8, 257) != 0;
      fails += admmq_packed_lrgemm_workspace_size((int64_t)1 << 40, 8, 8, 4) != 0;
      fails += admmq_packed_lrgemm_workspace_size(8, 8, 4, 4) != 64;
#define LR(cc, mm, M, K, ll, rr, r, xx, N, yy, ws, wsb) admmq_packed_lrgemm(cc, mm, M, K, ll, rr, r, xx, N, NULL, yy, ws, wsb, NULL)
      fails += LR(NULL, &qm, 8, 8, lf, rt, 4, x, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += LR(c, NULL, 8, 8, lf, rt, 4, x, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += LR(c, &qm, 8, 8, NULL, rt, 4, x, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += LR(c, &qm, 8, 8, lf, NULL, 4, x, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += LR(c, &qm, 8, 8, lf, rt, 4, NULL, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += LR(c, &qm, 8, 8, lf, rt, 4, x, 4, NULL, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += LR(c, &qm, 0, 8, lf, rt, 4, x, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += LR(c, &qm, 8, 8, lf, rt, 4, x, -4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += LR(c, &qm, 8, 8, lf, rt, 0, x, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += LR(c, &qm, 8, 8, lf, rt, 257, x, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += LR(c + 4, &qm, 8, 8, lf, rt, 4, x, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += LR(c, &qm, 8, 8, (const float*)0x30002, rt, 4, x, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      q2 = qm; q2.bits = 9;
      fails += LR(c, &q2, 8, 8, lf, rt, 4, x, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      q2 = qm; q2.scheme = ADMMQ_TENSOR_MINMAX; q2.bits = 1;
      fails += LR(c, &q2, 8, 8, lf, rt, 4, x, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      q2 = qm; q2.bad = 3;
      fails += LR(c, &q2, 8, 8, lf, rt, 4, x, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += LR(c, &qm, (int64_t)1 << 30, 8, lf, rt, 4, x, 4, y, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += LR(c, &qm, 512, 1141, lf, rt, 8, x, 4, y, ws, 16) != ADMMQ_ERR_WORKSPACE;
      fails += LR(c, &qm, 8, 8, lf, rt, 4, x, 4, y, ws, 63) != ADMMQ_ERR_WORKSPACE;
      fails += LR(c, &qm, 1024, 134, lf, rt, 8, x, 1024, y, NULL, 0) != ADMMQ_ERR_WORKSPACE;
#undef LR
    }
    /* the half-precision GEMM: the float GEMM's workspace, plus 4 np nb N bytes for tensor_minmax where
     * that is positive, and every refusal before any launch */
    {
      admmq_qmeta qx = qm;
      qx.scheme = ADMMQ_TENSOR_MINMAX;
      for (int t = 0; t < 400; ++t) {
        const int64_t M = rnd(1, 6000), K = rnd(1, 6000), N = rnd(1, t % 3 ? 70 : 4000);
        const int32_t nb = rnd(1, 4);
        const size_t w = admmq_packed_gemm_workspace_size(M, K, N, nb);
        const int64_t kp = K > 2048 ? 32 * ((K + 1023) / 1024) : 64;
        fails += admmq_packed_hgemm_workspace_size(&qm, M, K, N, nb) != w;
        fails += admmq_packed_hgemm_workspace_size(&qx, M, K, N, nb) != (w ? w + (size_t)4 * ((K + kp - 1) / kp) * nb * N : 0);
      }
      fails += admmq_packed_hgemm_workspace_size(NULL, 8, 65, 4, 1) != 0;
      fails += admmq_packed_hgemm_workspace_size(&qm, 0, 8, 8, 1) != 0;
      fails += admmq_packed_hgemm_workspace_size(&qm, 8, 8, -1, 1) != 0;
      fails += admmq_packed_hgemm_workspace_size(&qm, (int64_t)1 << 40, 8, 8, 1) != 0;
      fails += admmq_packed_hgemm_workspace_size(&qx, 8, 65, 4, 1) != 2 * 4 * 8 * 4 + 2 * 4 * 4;
#define HG(cc, mm, tr, M, K, xx, xd, xl, N, nb, bb, yy, yd, wsp, wsb) \
  admmq_packed_hgemm(cc, mm, tr, M, K, xx, xd, xl, N, nb, bb, yy, yd, wsp, wsb, NULL)
      const void* hx = (const void*)0x10000;
      void* hy = (void*)0x20000;
      const int32_t BF = ADMMQ_DT_BF16, HF = ADMMQ_DT_F16, F32 = ADMMQ_DT_F32;
      fails += HG(NULL, &qm, 0, 8, 8, hx, BF, 0, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, NULL, 0, 8, 8, hx, BF, 0, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 8, 8, NULL, BF, 0, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 8, 8, hx, BF, 0, 4, 1, NULL, NULL, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 0, 8, hx, BF, 0, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 8, 8, hx, BF, 0, -4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 2, 8, 8, hx, BF, 0, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 8, 8, hx, BF, 2, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 8, 8, hx, BF, 1, 4, 2, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 8, 8, hx, F32, 0, 4, 1, NULL, hy, F32, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 8, 8, hx, 3, 0, 4, 1, NULL, hy, F32, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 8, 8, hx, HF, 0, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c + 4, &qm, 0, 8, 8, hx, BF, 0, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 8, 8, (const void*)0x10001, BF, 0, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 8, 8, hx, BF, 0, 4, 1, NULL, (void*)0x20001, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 8, 8, hx, BF, 0, 4, 1, NULL, (void*)0x20002, F32, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 8, 8, hx, BF, 0, 4, 1, (const float*)0x30002, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      q2 = qm; q2.bits = 9;
      fails += HG(c, &q2, 0, 8, 8, hx, BF, 0, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      q2 = qm; q2.scheme = ADMMQ_TENSOR_MINMAX; q2.bits = 1;
      fails += HG(c, &q2, 0, 8, 8, hx, BF, 0, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      q2 = qm; q2.bad = 3;
      fails += HG(c, &q2, 0, 8, 8, hx, BF, 0, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      q2 = qm; q2.scheme = ADMMQ_TENSOR_AFFINE; q2.bits = 8; q2.zero_point = 200;
      fails += HG(c, &q2, 0, 8, 8, hx, BF, 0, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      q2.zero_point = -3000;
      fails += HG(c, &q2, 0, 8, 8, hx, HF, 0, 4, 1, NULL, hy, HF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, (int64_t)1 << 30, 8, hx, BF, 0, 4, 1, NULL, hy, BF, ws, 1 << 20) != ADMMQ_ERR_ARG;
      fails += HG(c, &qm, 0, 512, 1141, hx, BF, 0, 4, 1, NULL, hy, BF, ws, 16) != ADMMQ_ERR_WORKSPACE;
      fails += HG(c, &qm, 0, 512, 1141, hx, BF, 0, 4, 1, NULL, hy, BF, NULL, 0) != ADMMQ_ERR_WORKSPACE;
      fails += HG(c, &qx, 0, 512, 1141, hx, BF, 0, 4, 1, NULL, hy, BF, ws, 18 * 512 * 4 * 4) != ADMMQ_ERR_WORKSPACE;
#undef HG
    }
    /* the fused depthwise + 1x1 stage: the same workspace as the GEMM on (M, K, Ho Wo, nb),
     * and every refusal before any launch */
    const float* tp = (const float*)0x18000;
    for (int t = 0; t < 400; ++t) {
      const int64_t M = rnd(1, 6000), K = rnd(1, 6000), Ho = rnd(1, t % 3 ? 9 : 70), Wo = rnd(1, t % 3 ? 9 : 70);
      const int32_t nb = rnd(1, 8);
      fails += admmq_packed_dwgemm_workspace_size(M, K, Ho, Wo, nb) != admmq_packed_gemm_workspace_size(M, K, Ho * Wo, nb);
    }
    fails += admmq_packed_dwgemm_workspace_size(512, 1141, 2, 2, 1) == 0;
    fails += admmq_packed_dwgemm_workspace_size(8, 8, 0, 4, 1) != 0;
    fails += admmq_packed_dwgemm_workspace_size(8, 8, 4, -4, 1) != 0;
    fails += admmq_packed_dwgemm_workspace_size(8, 8, (int64_t)1 << 62, (int64_t)1 << 62, 1) != 0;
    fails += admmq_packed_dwgemm_workspace_size(8, 8, (int64_t)1 << 20, (int64_t)1 << 20, 1) != 0;
#define DW(cc, mm, M, K, tt, nb, H, W, pp, kh, kw, sh, sw, ph, pw, yy, wsb) \
  admmq_packed_dwgemm(cc, mm, M, K, tt, nb, H, W, pp, kh, kw, sh, sw, ph, pw, NULL, yy, ws, wsb, NULL)
    fails += DW(NULL, &qm, 8, 8, x, 1, 6, 6, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, NULL, 8, 8, x, 1, 6, 6, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, NULL, 1, 6, 6, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, x, 1, 6, 6, NULL, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, x, 1, 6, 6, tp, 3, 3, 1, 1, 1, 1, NULL, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 0, 8, x, 1, 6, 6, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, x, 0, 6, 6, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, x, 1, 0, 6, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, x, 1, 6, 6, tp, 0, 3, 1, 1, 0, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, x, 1, 9, 9, tp, 3, 8, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, x, 1, 6, 6, tp, 3, 3, 0, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, x, 1, 6, 6, tp, 3, 3, 1, 1, 3, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, x, 1, 6, 6, tp, 3, 3, 1, 1, 1, -1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, x, 1, 2, 6, tp, 5, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c + 4, &qm, 8, 8, x, 1, 6, 6, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, (const float*)0x10002, 1, 6, 6, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, x, 1, (int64_t)1 << 41, 6, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, (int64_t)1 << 20, x, 1, 1024, 1024, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 1024, x, 1024, 1024, 1024, tp, 3, 3, 64, 64, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 8, 8, x, 1, INT64_MAX, INT64_MAX, tp, 3, 3, INT32_MAX, INT32_MAX, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    q2 = qm; q2.bits = 0;
    fails += DW(c, &q2, 8, 8, x, 1, 6, 6, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    q2 = qm; q2.scheme = -2;
    fails += DW(c, &q2, 8, 8, x, 1, 6, 6, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    q2 = qm; q2.scheme = ADMMQ_TENSOR_MINMAX; q2.bits = 1;
    fails += DW(c, &q2, 8, 8, x, 1, 6, 6, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    q2 = qm; q2.bad = 1;
    fails += DW(c, &q2, 8, 8, x, 1, 6, 6, tp, 3, 3, 1, 1, 1, 1, y, 1 << 20) != ADMMQ_ERR_ARG;
    fails += DW(c, &qm, 512, 1141, x, 1, 2, 2, tp, 3, 3, 1, 1, 1, 1, y, 16) != ADMMQ_ERR_WORKSPACE;
#undef DW
    /* fixed-range activation quantizers: the record's checks come before everything else, a
     * quantizer that is off is not looked at, and the workspace is the parents' */
    {
      admmq_actq on = {4, 1, 0.3f, 1.1f}, off = {99, 0, 0.f, 0.f}, wide = {25, 1, 0.f, 1.f}, zero = {0, 1, 0.f, 1.f};
      fails += sizeof(admmq_actq) != 16;
      fails += admmq_fixed_quantize(NULL, y, 8, &on, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_fixed_quantize(x, NULL, 8, &on, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_fixed_quantize(x, y, 8, NULL, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_fixed_quantize(x, y, 8, &off, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_fixed_quantize(x, y, 8, &wide, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_fixed_quantize(x, y, 8, &zero, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_fixed_quantize(x, y, 0, &on, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_fixed_quantize(x, y, -1, &on, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_fixed_quantize((const float*)0x10002, y, 8, &on, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_gemm_act(c, &qm, 0, 8, 8, x, 0, 4, 1, NULL, y, &wide, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_gemm_act(c, &qm, 0, 8, 8, x, 0, 4, 1, NULL, y, &zero, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_gemm_act(NULL, &qm, 0, 8, 8, x, 0, 4, 1, NULL, y, &off, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_gemm_act(c, &qm, 0, 8, 8, x, 1, 4, 2, NULL, y, &on, ws, 1 << 20, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_gemm_act(c, &qm, 0, 512, 1141, x, 0, 4, 1, NULL, y, &on, ws, 16, NULL) != ADMMQ_ERR_WORKSPACE;
      fails += admmq_packed_gemm_act(c, &qm, 0, 512, 1141, x, 0, 4, 1, NULL, y, NULL, NULL, 0, NULL) != ADMMQ_ERR_WORKSPACE;
#define DWA(mm, M, K, H, W, mq, oq, wsb) \
  admmq_packed_dwgemm_act(c, mm, M, K, x, 1, H, W, tp, 3, 3, 1, 1, 1, 1, NULL, y, mq, oq, ws, wsb, NULL)
      fails += DWA(&qm, 8, 8, 6, 6, &wide, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += DWA(&qm, 8, 8, 6, 6, NULL, &zero, 1 << 20) != ADMMQ_ERR_ARG;
      fails += DWA(&qm, 8, 8, 6, 6, &on, &wide, 1 << 20) != ADMMQ_ERR_ARG;
      fails += DWA(NULL, 8, 8, 6, 6, &on, &on, 1 << 20) != ADMMQ_ERR_ARG;
      fails += DWA(&qm, 8, 8, 0, 6, &off, &on, 1 << 20) != ADMMQ_ERR_ARG;
      fails += DWA(&qm, 512, 1141, 2, 2, &on, &on, 16) != ADMMQ_ERR_WORKSPACE;
      fails += DWA(&qm, 512, 1141, 2, 2, NULL, NULL, 16) != ADMMQ_ERR_WORKSPACE;
#undef DWA
    }
    /* integer packed GEMM: the planner over ragged sizes, then every refusal of
     * the code, row-sum and GEMM entry points */
    {
      const uint8_t* xc = (const uint8_t*)0x10001;
      uint8_t* yc = (uint8_t*)0x40001;
      const int32_t* rs = (const int32_t*)0x30000;
      int32_t* cl = (int32_t*)0x50000;
      admmq_actq a8 = {8, 1, -1.f, 2.f}, a1 = {1, 1, -1.f, 2.f}, a9 = {9, 1, -1.f, 2.f}, aoff = {8, 0, 0.f, 0.f},
                 wide = {25, 1, 0.f, 1.f};
      for (int t = 0; t < 400; ++t) {
        const int64_t M = rnd(1, 6000), K = rnd(1, 70000), N = rnd(1, t % 3 ? 70 : 4000);
        const int32_t nb = rnd(1, 8);
        const size_t w = admmq_packed_igemm_workspace_size(M, K, N, nb);
        fails += w != admmq_packed_igemm_workspace_size(M, K, N, nb);
        fails += K > 65536 && w != 0;
      }
      fails += admmq_packed_igemm_workspace_size(512, 1141, 4, 1) == 0;
      fails += admmq_packed_igemm_workspace_size(0, 8, 8, 1) != 0;
      fails += admmq_packed_igemm_workspace_size(8, 65537, 8, 1) != 0;
      fails += admmq_act_encode(NULL, yc, 8, &a8, cl, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_act_encode(x, NULL, 8, &a8, cl, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_act_encode(x, yc, 8, NULL, cl, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_act_encode(x, yc, 8, &aoff, cl, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_act_encode(x, yc, 8, &a1, cl, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_act_encode(x, yc, 8, &a9, NULL, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_act_encode(x, yc, 0, &a8, cl, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_act_encode((const float*)0x10002, yc, 8, &a8, cl, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_act_encode(x, yc, 8, &a8, (int32_t*)0x50002, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_act_decode(NULL, y, 8, &a8, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_act_decode(xc, NULL, 8, &a8, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_act_decode(xc, y, 8, &a1, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_act_decode(xc, y, -1, &a8, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_act_decode(xc, (float*)0x20002, 8, &a8, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_rowsums(NULL, &qm, 0, 8, 8, (int32_t*)rs, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_rowsums(c, &qm, 0, 8, 8, NULL, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_rowsums(c, &qm, 0, 8, 65537, (int32_t*)rs, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_rowsums(c, &qm, 2, 8, 8, (int32_t*)rs, NULL) != ADMMQ_ERR_ARG;
      q2 = qm; q2.scheme = ADMMQ_TENSOR_MINMAX;
      fails += admmq_packed_rowsums(c, &q2, 0, 8, 8, (int32_t*)rs, NULL) != ADMMQ_ERR_SCHEME;
#define IG(mm, M, K, xq, N, nb, xl, yy, yyc, oq, wsb) \
  admmq_packed_igemm(c, mm, 0, M, K, xc, xq, rs, xl, N, nb, NULL, yy, yyc, oq, cl, ws, wsb, NULL)
      fails += IG(&q2, 8, 8, &a8, 4, 1, 0, y, NULL, NULL, 1 << 20) != ADMMQ_ERR_SCHEME;
      q2 = qm; q2.scheme = ADMMQ_TENSOR_AFFINE; q2.bits = 8; q2.zero_point = 1;
      fails += IG(&q2, 8, 8, &a8, 4, 1, 0, y, NULL, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      q2.zero_point = -1;
      fails += IG(&q2, 8, 8, &a8, 4, 1, 0, y, NULL, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      q2.zero_point = 0;
      fails += IG(&q2, 512, 1141, &a8, 4, 1, 0, y, NULL, NULL, 16) != ADMMQ_ERR_WORKSPACE;
      q2 = qm; q2.bad = 1;
      fails += IG(&q2, 8, 8, &a8, 4, 1, 0, y, NULL, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(NULL, 8, 8, &a8, 4, 1, 0, y, NULL, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(&qm, 8, 8, NULL, 4, 1, 0, y, NULL, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(&qm, 8, 8, &a1, 4, 1, 0, y, NULL, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(&qm, 8, 8, &a9, 4, 1, 0, y, NULL, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(&qm, 8, 8, &aoff, 4, 1, 0, y, NULL, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(&qm, 8, 65537, &a8, 4, 1, 0, y, NULL, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(&qm, 8, 8, &a8, 4, 1, 0, NULL, NULL, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(&qm, 8, 8, &a8, 4, 1, 0, y, yc, &a8, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(&qm, 8, 8, &a8, 4, 1, 0, NULL, yc, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(&qm, 8, 8, &a8, 4, 1, 0, NULL, yc, &a9, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(&qm, 8, 8, &a8, 4, 1, 0, y, NULL, &wide, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(&qm, 8, 8, &a8, 4, 2, 1, y, NULL, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(&qm, 0, 8, &a8, 4, 1, 0, y, NULL, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IG(&qm, 512, 1141, &a8, 4, 1, 0, NULL, yc, &a8, 16) != ADMMQ_ERR_WORKSPACE;
      fails += IG(&qm, 512, 1141, &a8, 4, 1, 0, y, NULL, NULL, 16) != ADMMQ_ERR_WORKSPACE;
#undef IG
      /* integer fused depthwise + 1x1: the workspace identity over ragged sizes, the
       * tap image's size, then every refusal of the two entry points */
      const int8_t* ti = (const int8_t*)0x70000;
      int32_t* mc = (int32_t*)0x60000;
      admmq_actq a6 = {6, 1, -1.f, 2.f};
      for (int t = 0; t < 400; ++t) {
        const int64_t M = rnd(1, 6000), K = rnd(1, 70000), Ho = rnd(1, t % 3 ? 9 : 70), Wo = rnd(1, t % 3 ? 9 : 70);
        const int32_t nb = rnd(1, 8);
        const size_t w = admmq_packed_idwgemm_workspace_size(M, K, Ho, Wo, nb);
        fails += w != admmq_packed_igemm_workspace_size(M, K, Ho * Wo, nb);
        fails += K > 65536 && w != 0;
        const int32_t nt = rnd(1, 49);
        fails += admmq_packed_taps_i8_bytes(nt, K) != (K > 65536 ? 0 : (size_t)nt * (size_t)(64 * ((K + 63) / 64)));
      }
      fails += admmq_packed_idwgemm_workspace_size(512, 1141, 7, 7, 1) != (size_t)18 * 512 * 49 * 4;
      fails += admmq_packed_idwgemm_workspace_size(8, 8, 0, 4, 1) != 0;
      fails += admmq_packed_idwgemm_workspace_size(8, 8, 4, (int64_t)1 << 31, 1) != 0;
      fails += admmq_packed_taps_i8_bytes(0, 8) != 0;
      fails += admmq_packed_taps_i8_bytes(50, 8) != 0;
      fails += admmq_packed_taps_i8_bytes(9, 0) != 0;
      fails += admmq_packed_taps_i8(NULL, &qm, 9, 8, (int8_t*)ti, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_taps_i8(c, NULL, 9, 8, (int8_t*)ti, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_taps_i8(c, &qm, 9, 8, NULL, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_taps_i8(c, &qm, 0, 8, (int8_t*)ti, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_taps_i8(c, &qm, 50, 8, (int8_t*)ti, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_taps_i8(c, &qm, 9, 0, (int8_t*)ti, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_taps_i8(c, &qm, 9, 65537, (int8_t*)ti, NULL) != ADMMQ_ERR_ARG;
      fails += admmq_packed_taps_i8(c, &qm, 9, 8, (int8_t*)0x70004, NULL) != ADMMQ_ERR_ARG;
      q2 = qm; q2.scheme = ADMMQ_TENSOR_MINMAX;
      fails += admmq_packed_taps_i8(c, &q2, 9, 8, (int8_t*)ti, NULL) != ADMMQ_ERR_SCHEME;
      q2 = qm; q2.scheme = ADMMQ_TENSOR_AFFINE; q2.bits = 8; q2.zero_point = 1;
      fails += admmq_packed_taps_i8(c, &q2, 9, 8, (int8_t*)ti, NULL) != ADMMQ_ERR_ARG;
      q2 = qm; q2.bad = 1;
      fails += admmq_packed_taps_i8(c, &q2, 9, 8, (int8_t*)ti, NULL) != ADMMQ_ERR_ARG;
#define IDW(mm, M, K, tq, H, W, tt, kh, sh, ph, yy, yyc, mq, oq, wsb)                                                     \
  admmq_packed_idwgemm(c, mm, M, K, xc, tq, 1, H, W, tt, 0.125f, kh, 3, sh, 1, ph, 1, rs, NULL, yy, yyc, mq, oq, mc, cl, ws, \
                       wsb, NULL)
      q2 = qm; q2.scheme = ADMMQ_TENSOR_MINMAX;
      fails += IDW(&q2, 8, 8, &a8, 6, 6, ti, 3, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_SCHEME;
      q2 = qm; q2.scheme = ADMMQ_TENSOR_AFFINE; q2.bits = 8; q2.zero_point = -1;
      fails += IDW(&q2, 8, 8, &a8, 6, 6, ti, 3, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(NULL, 8, 8, &a8, 6, 6, ti, 3, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, NULL, 6, 6, ti, 3, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a1, 6, 6, ti, 3, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a9, 6, 6, ti, 3, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, NULL, 3, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, (const int8_t*)0x70008, 3, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 3, 1, 1, y, NULL, NULL, NULL, 1 << 20) != ADMMQ_ERR_ARG;   /* mid_q is mandatory */
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 3, 1, 1, y, NULL, &aoff, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 3, 1, 1, y, NULL, &a1, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 3, 1, 1, y, NULL, &a9, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 3, 1, 1, NULL, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 3, 1, 1, y, yc, &a6, &a8, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 3, 1, 1, NULL, yc, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 3, 1, 1, NULL, yc, &a6, &a9, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 3, 1, 1, y, NULL, &a6, &wide, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 8, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 0, 1, 0, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 3, 0, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 3, 1, 3, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 6, 6, ti, 3, 1, -1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 8, &a8, 1, 6, ti, 5, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;   /* 1 + 2 < 5 */
      fails += IDW(&qm, 8, 8, &a8, 0, 6, ti, 3, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 0, 8, &a8, 6, 6, ti, 3, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 65537, &a8, 6, 6, ti, 3, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 8, 65536, &a8, 1 << 12, 1 << 12, ti, 3, 1, 1, y, NULL, &a6, NULL, 1 << 20) != ADMMQ_ERR_ARG;
      fails += IDW(&qm, 512, 1141, &a8, 2, 2, ti, 3, 1, 1, y, NULL, &a6, NULL, 16) != ADMMQ_ERR_WORKSPACE;
      fails += IDW(&qm, 512, 1141, &a8, 2, 2, ti, 3, 1, 1, NULL, yc, &a6, &a8, 16) != ADMMQ_ERR_WORKSPACE;
#undef IDW
    }
  }
  /* the ALS planner (csrc/als_kernels.hip plan_als) through its host-only plan query and the
   * workspace size: random 2-way / 3-way batches (9-tap layers, aligned and not, among them), every
   * kind and mode, and the refusals (made-up addresses: nothing is read) */
  for (int t = 0; t < 300; ++t) {
    admmq_cp_layer L[12] = {{0}};
    int32_t out[12 * 6];
    const int n = rnd(1, 12), nd = t % 3 == 0 ? 2 : 3;
    for (int i = 0; i < n; ++i) {
      L[i].W = (const float*)(uintptr_t)(0x100000 + 4 * rnd(0, 3));
      L[i].ndim = nd; L[i].R = rnd(1, 300);
      for (int d = 0; d < nd; ++d) { L[i].factors[d] = (const float*)0x1000; L[i].dims[d] = rnd(1, t % 7 == 0 ? 1200 : 150); }
      if (nd == 3 && rnd(0, 1)) { L[i].dims[2] = 9; L[i].dims[1] = 4 * rnd(1, 40); L[i].dims[0] = 4 * rnd(1, 40); }
    }
    for (int mode = 0; mode < nd; ++mode) {
      fails += admmq_cp_workspace_size(L, n, mode) == 0;
      for (int kind = 0; kind < 3; ++kind) {
        fails += admmq_debug_cp_plan(L, n, mode, kind, out) != ADMMQ_OK;
        for (int i = 0; i < n; ++i) {
          const int32_t* o = out + 6 * i;
          fails += (kind ? o[0] != kind : (o[0] != 0 && o[0] != 3)) || (o[1] != 32 && o[1] != 64) || o[2] < 1 || o[3] < 1 || o[4] < 1;
        }
      }
    }
    fails += admmq_debug_cp_plan(L, n, nd, 0, out) != ADMMQ_ERR_ARG;
  }
  {
    admmq_cp_layer L = {(const float*)0x100000, {(const float*)0x1000, (const float*)0x1000, (const float*)0x1000},
                        NULL, NULL, {4096, 4096, 2}, 3, 3};
    int32_t out[6];
    fails += admmq_debug_cp_plan(&L, 1, 2, 0, out) != ADMMQ_ERR_ARG;   /* Khatri-Rao range 2^24 */
    L.dims[1] = 4095;
    fails += admmq_debug_cp_plan(&L, 1, 2, 0, out) != ADMMQ_OK;
    fails += admmq_debug_cp_plan(&L, 1, 0, 3, out) != ADMMQ_ERR_ARG;
    fails += admmq_debug_cp_plan(NULL, 1, 0, 0, out) != ADMMQ_ERR_ARG;
    fails += admmq_debug_cp_plan(&L, 1, 0, 0, NULL) != ADMMQ_ERR_ARG;
    L.ndim = 4;
    fails += admmq_debug_cp_plan(&L, 1, 0, 0, out) != ADMMQ_ERR_ARG;
    L.ndim = 3; L.R = 0;
    fails += admmq_debug_cp_plan(&L, 1, 0, 0, out) != ADMMQ_ERR_ARG;
  }
  printf("last error: %s\n", admmq_last_error());
  printf("%s (%d failures)\n", fails ? "FAIL" : "OK", fails);
  return fails ? 1 : 0;
}
