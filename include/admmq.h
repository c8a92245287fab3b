/*
 * libadmmq — MI355X-native ADMM quantized tensor-factorization hot path (C ABI).
 *
 * Every entry point is stream-ordered on the caller's HIP stream (`stream` is a
 * hipStream_t passed as void*), takes plain device pointers to row-major float32
 * buffers, uses only caller-owned workspace, and returns an int32 status
 * (ADMMQ_OK = 0). No entry point allocates device memory or synchronises with the
 * device: plans (descriptor and work-unit tables) go up with hipMemcpyAsync from a pool
 * of pinned host staging chunks (per device of the stream, at most 64 MB) the library
 * grows on first use and reuses once their copies have completed, so a call returns
 * while its launches are still queued. Only when every chunk is in flight and the pool
 * is at its cap does a plan go up from pageable memory, a copy that may wait for the
 * stream (it never waits on the device otherwise).
 *
 * Reference interfaces replaced (KamikaziZen/admm-quantization @ 2024_10_08):
 *   admmq_admm_prepare + admmq_admm_run  <- source/admm.py:51-67  admm_iteration(H,U,F,G,max_iter,eps,bits,qscheme)
 *                                           (batched over independent (layer, mode) problems)
 *   admmq_quantize_batched               <- source/quantization.py:69-115  quantize_tensor(tensor,bits,qscheme,**kw)
 *                                           incl. quantize_tensor_mse :118-144, min_max_quantize :48-66
 *   admmq_quantize_channel               <- source/quantization.py:69-106 quantize_tensor(tensor,bits,
 *                                           'channel_symmetric' | 'channel_affine', dim)
 *   admmq_mse_sse_table                  <- source/quantization.py:129-141 (the candidate search, exposed
 *                                           for parity tests: canonical fixed-point SSE per candidate)
 *   admmq_cp_gram_mttkrp                 <- scripts/factorize.py:215-237 (3-way) and :276-287 (2-way):
 *                                           G = B.T @ B * (C.T @ C), F = torch.einsum('abc,cr,br->ar', W, C, B), ...
 *   admmq_cp_rel_error                   <- scripts/factorize.py:246-253 + source/admm.py:14-15
 *                                           squared_relative_diff(W, torch.einsum('ir,jr,kr->ijk', A, B, C))
 *   admmq_lowrank_pre / _post            <- scripts/factorize_lowrank.py:85-101 admm_iteration(H,U,W,H2,proj_func,
 *                                           rho,max_iter,eps): the updates around the projection, device break test
 *   admmq_panel_xtq / _xy / _outer       <- scripts/factorize_lowrank.py:80-82 (torch.linalg.svd + the rank-r
 *                                           product): the X^T Q, X Y and U S V^T products of the device projection
 *   admmq_cp64_gram_mttkrp               <- source/parafac_epc.py:42-74 (tensorly parafac / musco cp_anc's MTTKRP and
 *                                           Gram-Hadamard products, fp64)
 *   admmq_spd_solve64(_ws)               <- source/parafac_epc.py:42 (parafac's torch.linalg.solve(G, F.T).T)
 *   admmq_epc_step64 / admmq_epc_*64     <- source/parafac_epc.py:61-74 (cp_anc's mode update: eigendecomposition
 *                                           of G and the multiplier of the error constraint)
 */
#ifndef ADMMQ_H_
#define ADMMQ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADMMQ_OK 0
#define ADMMQ_ERR_ARG (-1)
#define ADMMQ_ERR_HIP (-2)
#define ADMMQ_ERR_WORKSPACE (-3)
#define ADMMQ_ERR_SCHEME (-4)

/* qscheme codes (names as in source/quantization.py:91-115) */
#define ADMMQ_TENSOR_MSEMINMAX_SYMMETRIC 0
#define ADMMQ_TENSOR_MINMAX 1
#define ADMMQ_TENSOR_SYMMETRIC 2
#define ADMMQ_TENSOR_AFFINE 3

/* One ADMM problem: one factor update  H <- argmin ||F - H G|| s.t. H quantized.
 * F, H0, H_out, U: I x R; G: R x R (symmetric PSD). U is read and overwritten
 * (source/admm.py:60 mutates the caller's U in place); H0 is never written. */
typedef struct admmq_problem {
  const float* F;
  const float* G;
  const float* H0;
  float* H_out;
  float* U;
  float* HT_out; /* optional (NULL): last iteration's H_T  (debug / parity tests) */
  float* X_out;  /* optional (NULL): last iteration's H_T - U (the quantizer input) */
  int32_t I;
  int32_t R;
} admmq_problem;

/* Bytes of workspace for a batch (num_attempts: MSE candidates, 200 in the reference). */
size_t admmq_admm_workspace_size(const admmq_problem* probs, int32_t nprob, int32_t num_attempts);

/* Setup of source/admm.py:52-54 for every problem: rho = tr(G)/R, M = (G + rho I)^-1
 * (fp64 blocked Cholesky, rounded to fp32), padded copies of F/H0/U and the first
 * right-hand side. Must precede admmq_admm_run on the same workspace. */
int32_t admmq_admm_prepare(const admmq_problem* probs, int32_t nprob, int32_t num_attempts, void* workspace,
                           size_t workspace_bytes, void* stream);

/* The loop of source/admm.py:55-65: max_iter-1 iterations of {solve, quantize,
 * dual update, residual test} per problem, with the per-problem early exit when
 * r < eps and s < eps. Writes H_out and U. info (device int32[nprob*4], may be
 * NULL) receives {iterations run, converged, spd_error, internal fault} per problem
 * (internal fault: see admmq_admm_run_ex). "converged" is the break itself: it is 1 only
 * when a later iteration was skipped, so a problem that first meets the rule in iteration
 * max_iter - 1, the last one run, reports {max_iter - 1, 0} - nothing tests after the last
 * finalize, and H_out / U are those of the same call with eps = 0 either way.
 * With info == NULL the run never takes the
 * fused paths that can report an internal fault (as fused_finalize = 0), so a NULL-info
 * call always returns finalized results. Uses the solve mode its prepare recorded;
 * ADMMQ_ERR_ARG for a workspace no prepare has set up, or whose prepare planned other
 * problems or another buffer layout (the record is kept per workspace address: prepare
 * again after reallocating a workspace). */
int32_t admmq_admm_run(const admmq_problem* probs, int32_t nprob, int32_t max_iter, float eps, int32_t bits,
                       int32_t qscheme, int32_t num_attempts, void* workspace, size_t workspace_bytes,
                       int32_t* info, void* stream);

/* Per-call options of the ADMM entry points (the _ex forms). A prepare fixes the
 * operand form of the solve for its workspace: a run on that workspace must ask for the
 * same solve_mode (ADMMQ_ERR_ARG otherwise). The plain forms above take the process
 * defaults (admmq_set_solve_mode) at prepare; their run uses what its prepare recorded. */
#define ADMMQ_SOLVE_FP32 0  /* v_mfma_f32_32x32x2_f32: an fp32 FMA chain, the reference's arithmetic (default) */
#define ADMMQ_SOLVE_SPLIT 1 /* split fp16 planes on f16 MFMA (about 2^-21 relative per product; opt-in) */
typedef struct admmq_admm_options {
  int32_t solve_mode;     /* ADMMQ_SOLVE_FP32 or ADMMQ_SOLVE_SPLIT */
  int32_t fused_finalize; /* 1: projection + dual update inside the search launch where all its blocks are
                             resident at once; 0: always the separate finalize launch (same results) */
  int32_t reserved[6];    /* must be zero */
} admmq_admm_options;

/* Fills *out with the process defaults (admmq_set_solve_mode; fused finalize on). */
int32_t admmq_admm_default_options(admmq_admm_options* out);
size_t admmq_admm_workspace_size_ex(const admmq_problem* probs, int32_t nprob, int32_t num_attempts,
                                    const admmq_admm_options* opt);
int32_t admmq_admm_prepare_ex(const admmq_problem* probs, int32_t nprob, int32_t num_attempts,
                              const admmq_admm_options* opt, void* workspace, size_t workspace_bytes, void* stream);
/* info[4 p + 3] != 0: an internal fault of problem p (the fused finalize's bounded wait for
 * its job's selection timed out because the search launch's blocks were not all resident,
 * e.g. other work on the device). The affected elements were NOT finalized: H_out / U of
 * that call are invalid and the caller must restore U and re-run with fused_finalize = 0
 * (the PyTorch op does this itself). info == NULL: fused_finalize is treated as 0 (no
 * fused path runs, so no fault can go unreported). */
int32_t admmq_admm_run_ex(const admmq_problem* probs, int32_t nprob, int32_t max_iter, float eps, int32_t bits,
                          int32_t qscheme, int32_t num_attempts, const admmq_admm_options* opt, void* workspace,
                          size_t workspace_bytes, int32_t* info, void* stream);

/* prepare + run. */
int32_t admmq_admm_iteration_batched(const admmq_problem* probs, int32_t nprob, int32_t max_iter, float eps,
                                     int32_t bits, int32_t qscheme, int32_t num_attempts, void* workspace,
                                     size_t workspace_bytes, int32_t* info, void* stream);

/* One quantize_tensor call: x viewed as (rows, cols) with cols the last dimension. */
typedef struct admmq_qtensor {
  const float* x;
  float* y;
  int64_t rows;
  int64_t cols;
  float tmin; /* tensor_affine kwargs (source/quantization.py:98-101) when has_minmax */
  float tmax;
  int32_t has_minmax;
  int32_t reserved;
} admmq_qtensor;

size_t admmq_quantize_workspace_size(const admmq_qtensor* t, int32_t n, int32_t num_attempts);
int32_t admmq_quantize_batched(const admmq_qtensor* t, int32_t n, int32_t bits, int32_t qscheme, int32_t num_attempts,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Packed integer codes of the four tensor schemes (DESIGN.md "Packed codes"). Every element
 * gets an unsigned code u in [0, 2^bits), bits 1..8, with q = 2^(bits-1), n = 2^bits - 1:
 *   mse-minmax / symmetric  u = clamp(rint(x/scale), -q, q-1) + q       y = (float)(u - q) * scale
 *   affine                  u = clamp(rint(x/scale) + zp, -q, q-1) + q  y = (float)((u - q) - zp) * scale
 *   minmax (bits >= 2)      u = floor(((x - mn)/rng) * n + 0.5)         y = ((float)u * rng) / n + mn
 * (float32 operations in this order, no fused multiply-add). Element i of the tensor's flat
 * row-major order occupies bits [i*bits, (i+1)*bits) of a little-endian bit stream: byte
 * (i*bits) >> 3 from bit (i*bits) & 7, least significant bit first; no row padding; the
 * stream is admmq_packed_bytes(numel, bits) = ceil(numel*bits/8) bytes and the spare high
 * bits of its last byte are 0. De-quantizing the codes gives admmq_quantize_batched's output
 * (equal under IEEE comparison; an integer code has no -0). `bad` counts the elements for
 * which it does not (every NaN result among them; such a code is stored as 0): a tensor
 * whose bad > 0 has no valid packed form. */
typedef struct admmq_qmeta { /* 32 bytes, written on the device */
  int32_t scheme, bits;
  float scale;        /* mse / symmetric / affine */
  int32_t zero_point; /* affine, else 0 */
  float mn, rng;      /* minmax, else 0 */
  int32_t index;      /* mse: chosen candidate (first-index argmin), else -1 */
  int32_t bad;
} admmq_qmeta;

size_t admmq_packed_bytes(int64_t numel, int32_t bits); /* 0 on bad arguments */

/* t, codes: host arrays of n entries; codes[i] (device, 16-byte aligned, admmq_packed_bytes
 * bytes) and meta_dev (device, n entries) receive the result. t[i].y may be NULL (codes
 * only); when it is not, the same launch also writes admmq_quantize_batched's float32
 * output there. ADMMQ_ERR_ARG for bits outside 1..8 and for tensor_minmax with bits == 1
 * (its outputs take three values). The workspace is admmq_quantize_workspace_size's plus
 * the table of code pointers. */
size_t admmq_quantize_packed_workspace_size(const admmq_qtensor* t, int32_t n, int32_t num_attempts);
int32_t admmq_quantize_packed(const admmq_qtensor* t, uint8_t* const* codes, admmq_qmeta* meta_dev, int32_t n,
                              int32_t bits, int32_t qscheme, int32_t num_attempts, void* workspace,
                              size_t workspace_bytes, void* stream);
/* The inverse: y[i] (device, numel[i] floats) from codes[i] (device, 16-byte aligned,
 * admmq_packed_bytes(numel[i], meta_dev[i].bits) bytes: nothing past them is read) and
 * meta_dev[i]. codes, y and numel are host arrays. Needs no workspace: the job table travels
 * in the kernel arguments, 32 tensors per launch. */
int32_t admmq_dequantize_packed(const uint8_t* const* codes, const admmq_qmeta* meta_dev, float* const* y,
                                const int64_t* numel, int32_t n, void* stream);

/* Packed-weight GEMM: a weight kept as packed codes times float32
 * activations, decoded on the fly; the float32 weight is never written to memory.
 *   Y_b[M, N] = W[M, K] . X_b[K, N] (+ bias[M]),  b = 0 .. nb-1
 *   trans_w = 0: W = D, the packed tensor is [M, K];  trans_w = 1: W = D^T, it is [K, M]
 * with D the table de-quantization of the codes (the formulas above), in the layout
 * admmq_quantize_packed wrote: admmq_packed_bytes(M*K, meta->bits) bytes, nothing past them
 * is read. `meta` is a HOST record (its bits select the kernel); `bad` must be 0, `index` is
 * ignored.
 *   x_layout 0 (NCHW 1x1 conv): X [nb, K, N] and Y [nb, M, N] contiguous, N = H*W
 *   x_layout 1 (linear):        X [N, K] and Y [N, M] row-major, one row per token; nb = 1
 * codes: device, 16-byte aligned. x, y, bias (may be NULL): device, float (4-byte) aligned -
 * no wider alignment is needed or used. Accumulation is exact float32 FMA on the fp32 MFMA:
 * K is cut into pieces of max(64, 32 ceil(K/1024)), each summed in increasing k from zero,
 * and an output is ((p0 + p1) + p2) + ... (+ bias last): a function of the inputs and K only,
 * the same bits for every nb and on every call. Limits: M <= 2^22, K <= 2^24, nb*N <= 2^30,
 * M*K < 2^40. ADMMQ_ERR_ARG for NULL codes / meta / x / y, non-positive sizes or sizes past
 * the limits, meta->bits outside 1..8, an unknown scheme, tensor_minmax with 1 bit,
 * meta->bad != 0, x_layout 1 with nb != 1, misaligned pointers; ADMMQ_ERR_WORKSPACE for a
 * short workspace - all before any launch.
 * admmq_packed_gemm_workspace_size depends on its arguments only. It returns 0 both for
 * arguments out of range and when no workspace is needed (many output tiles: `workspace`
 * may then be NULL); a positive size (float aligned device memory) is needed when the K
 * pieces of a tile run as separate workgroups (few output tiles). */
size_t admmq_packed_gemm_workspace_size(int64_t M, int64_t K, int64_t N, int32_t nb);
int32_t admmq_packed_gemm(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                          const float* x, int32_t x_layout, int64_t N, int32_t nb, const float* bias, float* y,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Fused depthwise + 1x1 stage of a packed CP layer: the depthwise kh x kw
 * convolution (the C factor) and the 1x1 convolution by a packed weight (the A factor) in one
 * kernel; the rank-K intermediate between them is never written to memory.
 *   t     [nb, K, H, W] float32, contiguous (the first 1x1 stage's output)
 *   taps  [kh*kw, K]    float32, row-major (the de-quantized C factor as it is)
 *   codes, meta         the packed weight D [M, K] (not transposed), as for admmq_packed_gemm
 *   y     [nb, M, Ho, Wo],  Ho = (H + 2 ph - kh) / sh + 1,  Wo = (W + 2 pw - kw) / sw + 1 (floor)
 * 1. z starts at +0.0f; for tap = a*kw + b in increasing order
 *      z = z + taps[tap][k] * t[b_img, k, oh*sh - ph + a, ow*sw - pw + b]
 *    with the product and the sum rounded separately; a tap whose position lies outside the
 *    image contributes nothing (for finite inputs: zero padding).
 * 2. Y[b, m, oh, ow] = sum_k D[m, k] z[b, k, oh, ow] (+ bias[m]) with exactly
 *    admmq_packed_gemm's arithmetic and order for (M, K, N = Ho*Wo, nb), trans_w = 0,
 *    x_layout = 0: the same K pieces, fold order (bias last) and regimes. The result has the
 *    bits of admmq_packed_gemm on a Z formed by step 1, for every nb and on every call.
 * Limits: 1 <= kh, kw <= 7; sh, sw >= 1; 0 <= ph < kh, 0 <= pw < kw; Ho, Wo >= 1;
 * admmq_packed_gemm's limits on M, K, nb*Ho*Wo and M*K; nb*K*H*W < 2^40. codes: device,
 * 16-byte aligned; t, taps, y, bias (may be NULL): device, float aligned. ADMMQ_ERR_ARG for
 * NULL codes / meta / t / taps / y, non-positive sizes, a bad meta record (as for
 * admmq_packed_gemm), a kernel size, stride or padding outside the limits, a window that does
 * not fit the padded image, misaligned pointers, sizes past the limits; ADMMQ_ERR_WORKSPACE
 * for a short workspace - all before any launch, each with its own admmq_last_error text.
 * admmq_packed_dwgemm_workspace_size(M, K, Ho, Wo, nb) equals
 * admmq_packed_gemm_workspace_size(M, K, Ho*Wo, nb) (0 for arguments out of range): the
 * partial images of the parallel regime only; there is no buffer for Z. */
size_t admmq_packed_dwgemm_workspace_size(int64_t M, int64_t K, int64_t Ho, int64_t Wo, int32_t nb);
int32_t admmq_packed_dwgemm(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const float* t,
                            int32_t nb, int64_t H, int64_t W, const float* taps, int32_t kh, int32_t kw, int32_t sh,
                            int32_t sw, int32_t ph, int32_t pw, const float* bias, float* y, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Fixed-range ("fake") activation quantizer (source/quantization.py:147-161):
 *   bits == 1:  y = sign(x) - 1 with sign(x) = (0 < x) - (x < 0)   (mn, rng ignored; NaN -> -1)
 *   else:       r = (x - mn) / rng;  n = float(2^bits - 1);  qi = floor(r * n + 0.5)
 *               y = (qi * rng) / n + mn
 * every step a separately rounded float32 operation. There is no clamp: a value outside
 * [mn, mn + rng] maps to a level outside 0..n, so the result is a float tensor without a
 * packed-code form. NaN, +-inf, rng == 0 and rng < 0 follow IEEE. The caller derives (mn, rng)
 * from its (min, max): both as float32, rng = max - min rounded to float32.
 * A HOST record; on == 0 (or a NULL pointer where one is optional): no quantizer. */
typedef struct admmq_actq {
  int32_t bits; /* 1..24 when on != 0 */
  int32_t on;
  float mn;
  float rng;
} admmq_actq; /* 16 bytes */

/* y[i] = q(x[i]), i < numel: x, y device, float aligned, contiguous (y may be x). One launch,
 * also for one element. ADMMQ_ERR_ARG for NULL x / y, NULL q or q->on == 0, q->bits outside
 * 1..24, numel <= 0 - each with its own admmq_last_error text, before any launch. */
int32_t admmq_fixed_quantize(const float* x, float* y, int64_t numel, const admmq_actq* q, void* stream);

/* admmq_packed_gemm with an output quantizer: Y = q_out(W X (+ bias)), applied to each output
 * just before it is stored (in the K-piece-parallel regime: after the ordered sum and the
 * bias; the partial images stay unquantized). The result has the bits of
 * admmq_fixed_quantize on admmq_packed_gemm's output. out_q NULL or on == 0: the bits (and the
 * kernels) of admmq_packed_gemm. The workspace size is admmq_packed_gemm_workspace_size's.
 * Errors as admmq_packed_gemm, plus ADMMQ_ERR_ARG for out_q->on != 0 with bits outside 1..24. */
int32_t admmq_packed_gemm_act(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                              const float* x, int32_t x_layout, int64_t N, int32_t nb, const float* bias, float* y,
                              const admmq_actq* out_q, void* workspace, size_t workspace_bytes, void* stream);

/* admmq_packed_dwgemm with a mid quantizer (z = q_mid(z) after step 1's tap sum: the
 * reference's quantizer behind the depthwise stage; only the elements of Z are quantized,
 * the zero fill of a tile's padding stays 0) and an output quantizer (as above). The result
 * has the bits of admmq_packed_gemm_act on a Z formed by step 1 and quantized by
 * admmq_fixed_quantize. Either may be NULL or off; with both off: the bits (and the kernels)
 * of admmq_packed_dwgemm. The workspace size is admmq_packed_dwgemm_workspace_size's. Errors
 * as admmq_packed_dwgemm, plus ADMMQ_ERR_ARG for a quantizer that is on with bits outside 1..24. */
int32_t admmq_packed_dwgemm_act(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const float* t,
                                int32_t nb, int64_t H, int64_t W, const float* taps, int32_t kh, int32_t kw,
                                int32_t sh, int32_t sw, int32_t ph, int32_t pw, const float* bias, float* y,
                                const admmq_actq* mid_q, const admmq_actq* out_q, void* workspace,
                                size_t workspace_bytes, void* stream);

/* Integer packed GEMM: activation codes as a tensor of their own, and the
 * product of a packed weight with such codes in integer arithmetic (v_mfma_i32_32x32x32_i8).
 *
 * Activation codes: one uint8 per element, the float tensor's shape and order. The quantizer
 * is an admmq_actq with bits 2..8 (1 bit has three output values and no code form);
 * n = float(2^bits - 1).
 *   encode  r = (x - mn) / rng;  qi = floor(r * n + 0.5f)   (admmq_fixed_quantize's r and qi:
 *           separately rounded float32 operations, an IEEE division);  u = clamp(qi, 0, n).
 *           An element whose qi lies outside [0, n] or is NaN is clamped (a NaN encodes as 0)
 *           and adds 1 to *clamped (device int32, may be NULL; zeroed on the stream first).
 *   decode  y = ((float)u * rng) / n + mn   in float32.
 * Where nothing was clamped, decode(encode(x)) has the bits of admmq_fixed_quantize(x). The
 * clamp is the one deliberate difference from the clamp-free quantizer; the counter shows it.
 * x, y: device, float aligned; codes: device, any address. ADMMQ_ERR_ARG for NULL x / codes / y,
 * NULL q or q->on == 0, bits outside 2..8, numel <= 0, misaligned x / y / clamped - before any
 * launch, each with its own admmq_last_error text. */
int32_t admmq_act_encode(const float* x, uint8_t* codes, int64_t numel, const admmq_actq* q, int32_t* clamped,
                         void* stream);
int32_t admmq_act_decode(const uint8_t* codes, float* y, int64_t numel, const admmq_actq* q, void* stream);

/* Weights: packed codes as admmq_quantize_packed wrote them, schemes mse-minmax, symmetric and
 * affine. With q = 2^(bits-1): a[m,k] = (uw - q) - zp (zp = 0 unless affine), an integer that
 * must fit int8; W = scale * a. Activations: x = g * ux + mn_x, g = rng_x / n_x.
 *   S[m,c] = sum_k a[m,k] ux[k,c]      A[m] = sum_k a[m,k]        (exact integer sums)
 *   y[m,c] = float( double(scale) * ( (double(rng_x) / double(n_x)) * double(S)
 *                                     + double(mn_x) * double(A[m]) ) + double(bias[m]) )
 * every operation in double, rounded separately (no fused multiply-add), one rounding to
 * float32; without a bias the last term is not added. S is an integer, so the result is the
 * same bits for every nb, on every call and in both regimes: no summation order is specified.
 *
 * admmq_packed_rowsums writes A[m], m < M (device int32), for W = D (trans_w 0, the packed
 * tensor is [M, K]) or D^T (trans_w 1, it is [K, M]); it runs once per weight and the caller
 * keeps the result.
 *
 * admmq_packed_igemm follows admmq_packed_gemm_act (layouts, trans_w, N, nb, bias, regimes), with
 * x the uint8 codes of the activations (any address) and x_q their quantizer, rowsums the row
 * sums of the same weight and orientation, and the output either
 *   y        float32 (y_codes NULL); with out_q on (bits 1..24): admmq_fixed_quantize of y, or
 *   y_codes  uint8   (y NULL; out_q on, bits 2..8): encode's code of y, with the same clamped
 *            counter rule (*clamped, may be NULL, is zeroed on the stream first). Every output
 *            byte is written by exactly one thread.
 * `meta` is a HOST record. All refusals come before any launch, each with its own
 * admmq_last_error text: ADMMQ_ERR_SCHEME for tensor_minmax weights (their de-quantization is
 * not scale * a); ADMMQ_ERR_ARG for an affine record with -q - zp < -128 or q - 1 - zp > 127,
 * K > 65536 (128 * 255 * K must stay below 2^31), activation bits outside 2..8, both or neither
 * of y / y_codes, and admmq_packed_gemm's own refusals (NULL pointers, sizes, bad != 0,
 * x_layout 1 with nb != 1, misaligned codes / y / bias / rowsums / clamped / workspace);
 * ADMMQ_ERR_WORKSPACE for a short workspace.
 * admmq_packed_igemm_workspace_size depends on its arguments only: 0 for arguments out of range
 * and when none is needed; else the int32 partial images of the K-piece-parallel regime (few
 * output tiles), which k_packed_ireduce sums. No output is combined with atomics and no
 * workgroup waits for another. No entry point allocates or synchronises. */
int32_t admmq_packed_rowsums(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                             int32_t* rowsums, void* stream);
size_t admmq_packed_igemm_workspace_size(int64_t M, int64_t K, int64_t N, int32_t nb);
int32_t admmq_packed_igemm(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                           const uint8_t* x, const admmq_actq* x_q, const int32_t* rowsums, int32_t x_layout, int64_t N,
                           int32_t nb, const float* bias, float* y, uint8_t* y_codes, const admmq_actq* out_q,
                           int32_t* clamped, void* workspace, size_t workspace_bytes, void* stream);

/* Integer fused depthwise + 1x1: admmq_packed_dwgemm_act's stage on activation
 * codes, in integer arithmetic from the stencil to the GEMM (v_mfma_i32_32x32x32_i8). With it a
 * 3-way CP layer's activations are uint8 codes from its input encode to its last epilogue.
 *   t_codes [nb, K, H, W] uint8 codes of the first 1x1 stage's output, t_q their quantizer (bits
 *           2..8): t = g_t ut + mn_t, g_t = double(rng_t) / double(n_t), n_t = 2^bits - 1
 *   taps_i8 [kh*kw][Kp] int8, Kp = 64 ceil(K / 64): the depthwise factor C [kh*kw, K] as integers
 *           c[tap,k] = (uc - q_c) - zp_c (columns k >= K are 0), written once per weight by
 *           admmq_packed_taps_i8; s_c is the scale of C's host meta record (passed as the float)
 *   codes, meta, rowsums   the packed weight D [M, K] and its row sums, as for admmq_packed_igemm
 *   mid_q   the quantizer of the depthwise stage's output, MANDATORY, bits 2..8
 * 1. For the output position (b, oh, ow) and channel k let V be the taps (a, bb) whose input
 *    position (oh*sh - ph + a, ow*sw - pw + bb) lies inside the image. With the exact integers
 *      D = sum_V c[tap,k] ut[b,k,ih,iw]        Cv = sum_V c[tap,k]        (|D| <= 49 * 128 * 255)
 *      z = float( double(s_c) * ( g_t * double(D) + double(mn_t) * double(Cv) ) )
 *    every operation in double, rounded separately, one rounding to float32. This is zero padding
 *    of the de-quantized t: a position outside the image contributes the value 0, not the code 0,
 *    so Cv depends on the position at the border. uz = encode(z; mid_q), admmq_act_encode's code
 *    (r, qi, clamp, a NaN encodes as 0).
 * 2. Y = D decode(uz) (+ bias) with exactly admmq_packed_igemm's contract for (M, K, N = Ho*Wo,
 *    nb), trans_w = 0, x_layout = 0, x_q = mid_q: the same output formula, output forms (y float,
 *    y + out_q, or y_codes under out_q) and clamped rule. The result has the bits of
 *    admmq_packed_igemm on a uz formed by step 1, for every nb, on every call and in both
 *    regimes; no summation order is specified.
 * Counters (device int32, each may be NULL, each zeroed on the stream first): *mid_clamped counts
 * the elements (b, k, oh, ow) of Z whose code was clamped, each once; *clamped is the codes
 * output's counter as for admmq_packed_igemm.
 * Limits: admmq_packed_dwgemm's geometry limits (1 <= kh, kw <= 7; sh, sw >= 1; 0 <= ph < kh,
 * 0 <= pw < kw; Ho, Wo >= 1; nb*K*H*W < 2^40; no dilation, no groups) and admmq_packed_igemm's
 * (K <= 65536, an int8-fitting a, no tensor_minmax). codes and taps_i8: device, 16-byte aligned;
 * t_codes: device, any address. All refusals come before any launch, each with its own
 * admmq_last_error text: the union of admmq_packed_dwgemm's and admmq_packed_igemm's, plus
 * ADMMQ_ERR_ARG for mid_q NULL / off / bits outside 2..8 and t_q bits outside 2..8;
 * ADMMQ_ERR_WORKSPACE for a short workspace. No allocation, no synchronisation.
 * admmq_packed_idwgemm_workspace_size(M, K, Ho, Wo, nb) equals
 * admmq_packed_igemm_workspace_size(M, K, Ho*Wo, nb): there is no buffer for Z or its codes.
 *
 * admmq_packed_taps_i8 expands the packed C (codes: device, 16-byte aligned; meta: its HOST
 * record; ntaps = kh*kw <= 49) into `image` (device, 16-byte aligned,
 * admmq_packed_taps_i8_bytes(ntaps, K) = ntaps * Kp bytes; 0 for arguments out of range). It
 * refuses what admmq_packed_rowsums refuses of a record (ADMMQ_ERR_SCHEME for tensor_minmax,
 * ADMMQ_ERR_ARG for an affine record outside int8 or bad != 0), NULL pointers, non-positive
 * sizes, ntaps > 49, K > 65536 and misaligned pointers. */
size_t admmq_packed_taps_i8_bytes(int32_t ntaps, int64_t K);
int32_t admmq_packed_taps_i8(const uint8_t* codes, const admmq_qmeta* meta, int32_t ntaps, int64_t K, int8_t* image,
                             void* stream);
size_t admmq_packed_idwgemm_workspace_size(int64_t M, int64_t K, int64_t Ho, int64_t Wo, int32_t nb);
int32_t admmq_packed_idwgemm(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const uint8_t* t_codes,
                             const admmq_actq* t_q, int32_t nb, int64_t H, int64_t W, const int8_t* taps_i8, float s_c,
                             int32_t kh, int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw,
                             const int32_t* rowsums, const float* bias, float* y, uint8_t* y_codes,
                             const admmq_actq* mid_q, const admmq_actq* out_q, int32_t* mid_clamped, int32_t* clamped,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Packed quant + low-rank GEMM: the deployable form of W ~ W_q + W_r
 * (admmq.lowrank): W_q as packed codes, W_r as its thin factors, one call
 *   y[N, M] = x[N, K] . (D + L Rt)^T (+ bias[M])
 * with D [M, K] the table de-quantization of `codes` (as for admmq_packed_gemm, trans_w = 0),
 * L [M, r] and Rt [r, K] row-major float32, 1 <= r <= 256. Linear layout only: x and y
 * row-major, one row per token. Neither D nor L Rt is written to memory.
 * Arithmetic, with kp = max(64, 32 ceil(K/1024)) and np = ceil(K/kp) (admmq_packed_gemm's K
 * pieces, a function of K alone), every sum an fp32 MFMA chain in increasing index from zero:
 *   t[j, c] = ((s_0 + s_1) + ...) + s_{np-1},  s_p = sum over piece p of Rt[j, k] x[c, k]
 *   y[c, m] = ((((p_0 + p_1) + ...) + p_{np-1}) + q) + bias[m]
 * with p_i the pieces of admmq_packed_gemm on D and q = sum_j L[m, j] t[j, c] (j zero-padded
 * to a multiple of 32). An output depends on its own column of x, on K and on r only: the
 * same bits for every N and on every call; with L = 0 or Rt = 0 the values of
 * admmq_packed_gemm. Launches: k_lr_down (t), k_packed_lrgemm (the pieces and the tail), and
 * k_lr_reduce where the pieces run as separate workgroups - one more than admmq_packed_gemm.
 * codes: device, 16-byte aligned; L, Rt, x, y, bias (may be NULL): device, float aligned.
 * `meta` is a HOST record. stream: a hipStream_t. Limits: admmq_packed_gemm's on M, K, N
 * (nb = 1) and M*K. ADMMQ_ERR_ARG for NULL codes / meta / L / Rt / x / y, non-positive sizes,
 * r outside 1..256, what admmq_packed_gemm refuses of a meta record, misaligned pointers,
 * sizes past the limits; ADMMQ_ERR_WORKSPACE for a NULL or short workspace - all before any
 * launch. admmq_packed_lrgemm_workspace_size depends on its arguments only: 0 for arguments
 * out of range, else positive (t always lives there: at least
 * admmq_packed_gemm_workspace_size(M, K, N, 1) + 4 r N bytes). */
size_t admmq_packed_lrgemm_workspace_size(int64_t M, int64_t K, int64_t N, int32_t r);
int32_t admmq_packed_lrgemm(const uint8_t* codes, const admmq_qmeta* meta, int64_t M, int64_t K, const float* L,
                            const float* Rt, int32_t r, const float* x, int64_t N, const float* bias, float* y,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Half-precision packed GEMM: admmq_packed_gemm's product on bfloat16 or
 * float16 activations, on v_mfma_f32_32x32x16_{bf16,f16}. Shapes, trans_w, the two x layouts,
 * the code stream and the HOST meta record are admmq_packed_gemm's. x_dtype is ADMMQ_DT_F16 or
 * ADMMQ_DT_BF16; y_dtype is ADMMQ_DT_F32 or x_dtype; bias (may be NULL) is float32.
 * Arithmetic, with kp = max(64, 32 ceil(K/1024)) and np = ceil(K/kp) (admmq_packed_gemm's K
 * pieces): the weight enters the MFMA as an exact integer half value and its scale is applied
 * in float32 behind the sum.
 *   mse-minmax, symmetric, affine: a = (u - q) - zero_point (q = 2^(bits-1); zero_point 0
 *   unless affine)
 *     S = ((s_0 + s_1) + ...) + s_{np-1},  s_p = the MFMA accumulator chain of piece p from zero
 *     over a[m, k] x[k, c];  y32 = (S * scale) + bias[m]
 *   tensor_minmax (bits >= 2): the operand is u (0 .. 255)
 *     y32 = ((S_u * rng) / n + mn * S_x) + bias[m],  n = float(2^bits - 1)
 *     with S_x the column's sum of x formed like S_u, against an operand of ones.
 * Every operation above is a separately rounded float32 one. y is y32, or y32 rounded once to
 * nearest even to x_dtype. An output depends on its own column of x, on K and on the weight
 * only: the same bits for every N and nb and on every call; no atomics. Half subnormal inputs
 * are outside the contract.
 * codes: device, 16-byte aligned; x and y: device, aligned to their element (2 or 4 bytes) - no
 * wider alignment is needed; bias: float aligned. Limits: admmq_packed_gemm's. ADMMQ_ERR_ARG
 * for NULL codes / meta / x / y, non-positive sizes or sizes past the limits, what
 * admmq_packed_gemm refuses of a meta record, an affine record whose -q - zero_point or
 * q - 1 - zero_point is not an integer exact in x_dtype (magnitude above 256 for bfloat16, 2048
 * for float16), x_layout 1 with nb != 1, a dtype pair other than the above, misaligned
 * pointers; ADMMQ_ERR_WORKSPACE for a short workspace - all before any launch.
 * admmq_packed_hgemm_workspace_size depends on its arguments only (of meta: the scheme): 0 for
 * a NULL meta or sizes out of range, else admmq_packed_gemm_workspace_size(M, K, N, nb), plus,
 * for tensor_minmax where that size is positive, 4 np nb N bytes (the pieces' sums of x). */
#define ADMMQ_DT_F32 0
#define ADMMQ_DT_F16 1
#define ADMMQ_DT_BF16 2
size_t admmq_packed_hgemm_workspace_size(const admmq_qmeta* meta, int64_t M, int64_t K, int64_t N, int32_t nb);
int32_t admmq_packed_hgemm(const uint8_t* codes, const admmq_qmeta* meta, int32_t trans_w, int64_t M, int64_t K,
                           const void* x, int32_t x_dtype, int32_t x_layout, int64_t N, int32_t nb,
                           const float* bias, void* y, int32_t y_dtype, void* workspace, size_t workspace_bytes,
                           void* stream);

/* Per-channel schemes with an explicit dim (source/quantization.py:29-33, 91-106):
 * max / min of every row of unfold(x, dim) (source/utils.py:60-74), then the
 * tensor_symmetric / tensor_affine arithmetic with those shape[dim] statistics broadcast
 * against x's LAST dimension as torch does: requires shape[ndim-1] == shape[dim] or one of
 * them 1 (ADMMQ_ERR_ARG otherwise); y holds shape[:-1] + (max(shape[ndim-1], shape[dim]),)
 * elements. x contiguous, ndim >= 1, dim in [-ndim, ndim). */
#define ADMMQ_CHANNEL_SYMMETRIC 4
#define ADMMQ_CHANNEL_AFFINE 5
size_t admmq_quantize_channel_workspace_size(const int64_t* shape, int32_t ndim, int32_t dim);
int32_t admmq_quantize_channel(const float* x, float* y, const int64_t* shape, int32_t ndim, int32_t dim, int32_t bits,
                               int32_t qscheme, void* workspace, size_t workspace_bytes, void* stream);

/* Canonical SSE table of the MSE-minmax search for one tensor (sse_out: device uint64[num_attempts]). */
int32_t admmq_mse_sse_table(const float* x, int64_t rows, int64_t cols, int32_t bits, int32_t num_attempts,
                            uint64_t* sse_out, void* workspace, size_t workspace_bytes, void* stream);

/* A/B switch for the MSE-minmax search: 1 = evaluate the canonical SSE of every
 * candidate (the reference's 200 full passes), 0 (default) = two-stage exact search
 * (level-breakpoint bounds, then the canonical SSE only for candidates that can still
 * be the argmin). Both return bit-identical results. */
int32_t admmq_set_exhaustive_search(int32_t enable);

/* Process default of the per-iteration solve's operand form H_T = P M (the
 * cholesky_solve of source/admm.py:56) for the plain (non-_ex) entry points:
 * ADMMQ_SOLVE_FP32 (0, default) = fp32 MFMA, the reference's fp32 arithmetic;
 * ADMMQ_SOLVE_SPLIT (1) = split fp16 planes on f16 MFMA (P and M as hi + lo fp16 with a
 * power-of-two exponent per row, 3 products, fp32 accumulation; about 2^-21 relative per
 * product). Both stay within the 1e-5 rel-Frobenius solve contract of SURVEY.md §8(c) P2.
 * Read once by admmq_admm_prepare, which records it for its workspace: a later change
 * does not affect runs on an already prepared workspace. */
int32_t admmq_set_solve_mode(int32_t mode);
int32_t admmq_get_solve_mode(void);

/* Optional HIP-event timing of every launch issued by admmq_admm_prepare/run on this
 * thread between begin and end, one event pair per launch, summed per class:
 * ADMMQ_PROF_GEMM k_gemm (solve, MFMA), ADMMQ_PROF_GEMM_THIN k_gemm_thin (solve of the
 * I <= 16 factors, VALU), ADMMQ_PROF_SEARCH the multi-block MSE candidate search
 * (k_mse_hist3 / k_mse_hist / the exhaustive sweep), ADMMQ_PROF_SMALL k_mse_small_admm
 * (search + projection + dual update of the I <= 16 factors in one block each),
 * ADMMQ_PROF_FINALIZE k_finalize_admm (projection + dual update), ADMMQ_PROF_PREPARE the
 * whole prepare phase (rho, SPD inverse, operand planes), ADMMQ_PROF_THIN_LOOP k_thin_loop
 * (every iteration of a call whose factors all have I <= 16, one persistent launch, always
 * timed). Only ADMM iterations it with
 * it % sample_every == 0 are timed (each event pair adds an inter-kernel gap, so the
 * bench samples instead of timing every launch). end() synchronises on the last event
 * and fills ADMMQ_PROF_CLASSES summed milliseconds and launch counts. */
#define ADMMQ_PROF_GEMM 0
#define ADMMQ_PROF_GEMM_THIN 1
#define ADMMQ_PROF_SEARCH 2
#define ADMMQ_PROF_SMALL 3
#define ADMMQ_PROF_FINALIZE 4
#define ADMMQ_PROF_PREPARE 5
#define ADMMQ_PROF_THIN_LOOP 6
#define ADMMQ_PROF_CLASSES 8
int32_t admmq_profile_begin(int32_t max_launches, int32_t sample_every);
int32_t admmq_profile_end(double* ms_per_class, int64_t* launches_per_class);

/* One CP layer of the ALS sweep (scripts/factorize.py:207-310): W is dims[0] x dims[1]
 * (x dims[2]) row-major (a 3x3 conv reshaped to (cout, cin, 9), or a 2-D weight);
 * factors[d] is dims[d] x R row-major. G / F are outputs of admmq_cp_gram_mttkrp. */
typedef struct admmq_cp_layer {
  const float* W;
  const float* factors[3]; /* factors[2] unused (NULL) when ndim == 2 */
  float* G;                /* R x R: Hadamard product of the Grams of the factors other than `mode` */
  float* F;                /* dims[mode] x R: MTTKRP of W with the Khatri-Rao product of the others */
  int32_t dims[3];
  int32_t ndim;            /* 2 or 3 */
  int32_t R;
} admmq_cp_layer;

/* Workspace bytes for admmq_cp_gram_mttkrp (this mode) and admmq_cp_rel_error on these layers. */
size_t admmq_cp_workspace_size(const admmq_cp_layer* layers, int32_t n, int32_t mode);

/* For every layer: G = Gram∘Gram of the factors other than `mode` and F = the mode-`mode`
 * MTTKRP (fp32 MFMA, deterministic split-K). factors[mode] is not read. */
int32_t admmq_cp_gram_mttkrp(const admmq_cp_layer* layers, int32_t n, int32_t mode, void* workspace,
                             size_t workspace_bytes, void* stream);

/* out[l] (device double[n]) = ||W - [[factors]]||_F / ||W||_F per layer, without
 * materialising the reconstruction (fp32 MFMA products, fp64 sums). */
int32_t admmq_cp_rel_error(const admmq_cp_layer* layers, int32_t n, double* out, void* workspace,
                           size_t workspace_bytes, void* stream);

/* fp64 per-mode contractions of the CP-ALS / EPC initialiser (admmq.parafac_epc): the
 * reference runs them inside tensorly `parafac` and musco `cp_anc` on the fp64 tensor
 * (source/parafac_epc.py:36-74). Same layout as admmq_cp_layer, in double. */
typedef struct admmq_cp_layer_f64 {
  const double* W;
  const double* factors[3]; /* factors[2] unused (NULL) when ndim == 2 */
  double* G;                /* R x R: Hadamard product of the Grams of the factors other than `mode` */
  double* F;                /* dims[mode] x R: MTTKRP of W with the Khatri-Rao product of the others */
  int32_t dims[3];
  int32_t ndim;             /* 2 or 3 */
  int32_t R;
} admmq_cp_layer_f64;

/* Workspace bytes for admmq_cp64_gram_mttkrp (this mode) on these layers. */
size_t admmq_cp64_workspace_size(const admmq_cp_layer_f64* layers, int32_t n, int32_t mode);

/* For every layer: G and F of `mode` in fp64 (f64 MFMA, Khatri-Rao operand formed on the
 * fly, deterministic split-K). factors[mode] is not read. */
int32_t admmq_cp64_gram_mttkrp(const admmq_cp_layer_f64* layers, int32_t n, int32_t mode, void* workspace,
                               size_t workspace_bytes, void* stream);

/* Quant + low-rank ADMM (scripts/factorize_lowrank.py:85-101), one iteration =
 *   admmq_lowrank_pre   Hbar = (rho (H + U) + W - H2) / (1 + rho),  X = Hbar - U
 *   (caller)            Hn = proj(X)   (quantizer: admmq_quantize_batched; or a rank projection)
 *   admmq_lowrank_post  U += Hn - Hbar; H = Hn; residuals r, s; sticky done when r < eps and s < eps
 * All buffers are n contiguous floats. The workspace holds {done, ticket, iterations, 0}
 * (int32) at offset 0 and the fp64 partial sums; admmq_lowrank_reset zeroes the state
 * before a call's first iteration. After `done`, pre/post do nothing. */
size_t admmq_lowrank_workspace_size(int64_t n);
int32_t admmq_lowrank_reset(void* workspace, size_t workspace_bytes, void* stream);
int32_t admmq_lowrank_pre(const float* H, const float* U, const float* W, const float* H2, float* Hbar, float* X,
                          int64_t n, float rho, void* workspace, size_t workspace_bytes, void* stream);
int32_t admmq_lowrank_post(const float* Hn, const float* Hbar, float* H, float* U, int64_t n, float eps,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Panel products of the rank projection (scripts/factorize_lowrank.py:80-82, the truncated
 * SVD of every low-rank inner step; admmq.lowrank.KrylovProjector builds it from these):
 *   admmq_panel_xtq    Y = X^T Q  (n x k, row-major, ld k)
 *   admmq_panel_xy     Z = X Y    (m x k, row-major, ld k)
 * X: m x n float32 with row stride ldx, read as float32 and widened exactly; Q / Y / Z
 * float64. v_mfma_f64_16x16x4_f64, fp64 accumulation in a fixed order (the result depends
 * on m, n, k only). The workspace (admmq_panel_workspace_size, zeroed once before its first
 * use) holds the cross-workgroup partials and, at its end, the arrival counters: calls on
 * one workspace must be stream-ordered and pass the same workspace_bytes (a larger
 * workspace for larger panels is a new, zeroed buffer).
 *   admmq_panel_outer  O = A B^T  (m x n float32, row stride ldo): A m x r, B n x r float64,
 * each output summed over r in fp64 and rounded once; r <= 32. */
size_t admmq_panel_workspace_size(int64_t m, int64_t n, int64_t k);
int32_t admmq_panel_xtq(const float* X, int64_t m, int64_t n, int64_t ldx, const double* Q, int64_t k, double* Y,
                        void* workspace, size_t workspace_bytes, void* stream);
int32_t admmq_panel_xy(const float* X, int64_t m, int64_t n, int64_t ldx, const double* Y, int64_t k, double* Z,
                       void* workspace, size_t workspace_bytes, void* stream);
int32_t admmq_panel_outer(const double* A, const double* B, int64_t m, int64_t n, int64_t r, float* O, int64_t ldo,
                          void* stream);
/* C = A^T B (p x q, row-major, ld q) for tall float64 A (m x p, row stride lda) and B (m x q,
 * row stride ldb): the panels' Gram / cross products (fixed summation order; the workspace,
 * admmq_gram64_workspace_size, needs no initialisation). */
size_t admmq_gram64_workspace_size(int64_t m, int64_t p, int64_t q);
int32_t admmq_gram64(const double* A, int64_t lda, const double* B, int64_t ldb, int64_t m, int64_t p, int64_t q,
                     double* C, void* workspace, size_t workspace_bytes, void* stream);

/* The EPC step's multiplier (cp_anc, source/parafac_epc.py:61-74): *mu (device double) = the
 * root mu >= 0 of normY2 - sum_i c_i (s_i + 2 mu) / (s_i + mu)^2 = delta2 (0 when already
 * below), by bracket doubling and bisection to fp64 resolution; c, s: n device doubles. */
int32_t admmq_epc_mu(const double* c, const double* s, int64_t n, double normY2, double delta2, double* mu,
                     void* stream);

/* The R x R solves of the CP-ALS / EPC initialiser on one workgroup (the fp64 matrix in LDS,
 * 1 <= n <= 136), replacing tensorly parafac's torch.linalg.solve and cp_anc's eigendecomposition
 * (source/parafac_epc.py:42, :61-74). Row-major device doubles; no host synchronisation.
 *   admmq_spd_solve64  X = F G^-1 (F, X: m x n; G: n x n SPD) by an unpivoted blocked Gauss-Jordan
 *                      inverse of G in LDS; *info (device int, may be NULL) = 0, or 1 when a pivot
 *                      is not positive (G not numerically positive definite: X untouched).
 *   admmq_epc_step64   X = F (G + mu I)^-1 with mu >= 0 the root of
 *                      normY2 - <F, X> - mu ||X||^2 = delta2 (= the eigen form
 *                      normY2 - sum_j |F v_j|^2 (s_j + 2 mu) / (s_j + mu)^2), 0 when the LS step's
 *                      error already reaches delta2; *mu (device double): in, a warm start (<= 0:
 *                      none), out, the root. work: m x n device doubles of scratch (F Q and the
 *                      solved rows, transposed: G = Q T Q^T is tridiagonalised once per call).
 *                      G is reduced to tridiagonal form once (Householder), every evaluation of
 *                      the error equation is then a set of tridiagonal L D L^T recurrences.
 *                      *info (may be NULL): 0, or 1 when no G + mu I on the search bracket was
 *                      positive definite (X NaN), the search's budget ran out or an internal
 *                      hand-off timed out. */
int32_t admmq_spd_solve64(const double* G, const double* F, int64_t m, int64_t n, double* X, int32_t* info,
                          void* stream);
int32_t admmq_epc_step64(const double* G, const double* F, int64_t m, int64_t n, double normY2, double delta2,
                         double* mu, double* X, double* work, int32_t* info, void* stream);

/* The same solves for any n (1 <= n <= 8192), spread over the chip (the resnet ranks 183 ... 1141 do
 * not fit one workgroup's LDS): A = G + shift I (fp64, shift = rel_shift * trace(G) / n), its
 * blocked Cholesky A = L L^T and L^-1 (the 32 x 32-blocked fp64 kernels of the ADMM prepare),
 * then X = (F L^-T) L^-1 as two fp64-MFMA GEMMs. Caller-owned workspace of
 * admmq_solve64_workspace_size(m, n) bytes (no initialisation; calls on one workspace must be
 * stream-ordered); no host synchronisation.
 *   admmq_spd_solve64_ws   X = F (G + shift I)^-1 (replaces source/parafac_epc.py:42, tensorly parafac's
 *                          torch.linalg.solve(G, F.T).T); *info (device int, may be NULL) = 0, or 1
 *                          when G + shift I is not numerically positive definite (X undefined). n <= 136
 *                          runs the one-workgroup kernel of admmq_spd_solve64 (no workspace used).
 *   admmq_epc_begin64 / admmq_epc_rounds64 / admmq_epc_end64
 *                          the EPC mode update of admmq_epc_step64 (replaces source/parafac_epc.py:61-74,
 *                          musco cp_anc's eigendecomposition) for any n: begin sets the multiplier
 *                          search up on the device (*mu: the warm start, <= 0 none); each round is one
 *                          evaluation (a Cholesky of G + mu I at the search's next mu, X = F (G + mu I)^-1,
 *                          and the Newton update of mu on the device); rounds after the search is done
 *                          return at once. *done (device int, may be NULL) = 1 once it is done: the
 *                          caller reads it when it chooses and asks for more rounds until then.
 *                          end writes *mu (device double) and *info (device int, may be NULL): 0
 *                          converged (X = F (G + mu I)^-1 at the returned mu), 1 no positive definite
 *                          G + mu I found or the evaluation budget (admmq_epc64_max_evals()) spent, 2 not
 *                          done yet.
 *                          Contract of one step: from begin to end the workspace belongs to that step. It
 *                          holds the search state, the Cholesky's descriptor, the GEMM job tables and the
 *                          A / L^-1 / product planes between the calls, so no other blocked solve or step
 *                          may use it in between, not even on the same stream (stream order does not
 *                          help: the step is not over when a call returns). rounds64 / end64 must be
 *                          given begin's m and n, and rounds64 begin's G, F and X: the job tables keep
 *                          begin's pointers and extents. Neither is checked.
 *   admmq_epc64_max_evals  the search's evaluation budget: after that many rounds *done is 1. */
size_t admmq_solve64_workspace_size(int64_t m, int64_t n);
int32_t admmq_epc64_max_evals(void);
int32_t admmq_spd_solve64_ws(const double* G, const double* F, int64_t m, int64_t n, double rel_shift, double* X,
                             int32_t* info, void* workspace, size_t workspace_bytes, void* stream);
int32_t admmq_epc_begin64(const double* G, const double* F, int64_t m, int64_t n, double normY2, double delta2,
                          const double* mu, double* X, void* workspace, size_t workspace_bytes, void* stream);
int32_t admmq_epc_rounds64(const double* G, const double* F, int64_t m, int64_t n, double* X, int32_t rounds,
                           int32_t* done, void* workspace, size_t workspace_bytes, void* stream);
int32_t admmq_epc_end64(int64_t m, int64_t n, double* mu, int32_t* info, void* workspace, size_t workspace_bytes,
                        void* stream);

/* cp_anc's normalisation of the factors other than the one being updated
 * (source/parafac_epc.py:61-74, musco cp_anc): outA = A / max(||A[:, r]||_2, 1e-300) per column r
 * (A: rowsA x R row-major device doubles), and the same for B into outB when B is not NULL;
 * one launch, no host synchronisation. */
int32_t admmq_cp_colnorm64(const double* A, int64_t rowsA, const double* B, int64_t rowsB, int64_t R, double* outA,
                           double* outB, void* stream);

/* Diagnostics: the multi-candidate MSE selections (|S| > 1) whose canonical-SSE sweep the fused
 * search + finalize launch shared among the job's workgroups, since the last reset (a host
 * read of a device counter: synchronises); reset != 0 zeroes it. -1 on a HIP error. */
int64_t admmq_debug_shared_stage2_count(int32_t reset);

/* Diagnostics: the kernel form the ALS planner gives every layer of an admmq_cp_gram_mttkrp
 * (kind 0: F, kind 1: G) or admmq_cp_rel_error (kind 2; mode ignored) call. Host only: no device
 * call, W and the factors are never read (W's address decides the 16-byte-aligned spatial form).
 * out: n x 6 int32 {job kind (0 generic MTTKRP, 1 Gram, 2 error, 3 spatial MTTKRP), tile rows BM
 * (32 / 64), row tiles, column tiles, nsplit (partial planes summed by k_als_reduce; 1: none),
 * kchunk (reduction rows per K chunk of the generic MTTKRP, else 0)}. Returns the planner's
 * refusal (ADMMQ_ERR_ARG: bad layer, mode out of range, Khatri-Rao index range >= 2^24). */
int32_t admmq_debug_cp_plan(const admmq_cp_layer* layers, int32_t n, int32_t mode, int32_t kind, int32_t* out);

/* Library version (major*10000 + minor*100 + patch) and the last error text of this thread. */
int32_t admmq_version(void);
const char* admmq_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* ADMMQ_H_ */
