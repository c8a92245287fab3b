// PyTorch custom operators (torch.ops.admmq.*) over the C-ABI of libadmmq.so.
//
// The Python drop-ins (admmq.admm / .quantization / .als) call these ops; each op
// validates its tensors, allocates the caller-owned workspace through PyTorch's
// caching allocator, and calls the same stream-ordered entry points of
// include/admmq.h on the current HIP stream. Reference interfaces mirrored:
//   admmq::admm_iteration_batched  <- source/admm.py:51-67 admm_iteration (batched over problems)
//   admmq::quantize_batched        <- source/quantization.py:69-144 quantize_tensor
//   admmq::quantize_packed / dequantize_packed: the packed integer codes of the tensor schemes
//                                     (no reference counterpart; DESIGN.md "Packed codes")
//   admmq::packed_gemm             a packed weight times float32 activations
//   admmq::packed_hgemm            a packed weight times bfloat16 / float16 activations
//   admmq::packed_lrgemm           packed codes + low-rank factors times float32 activations, one GEMM
//   admmq::packed_dwgemm           depthwise k x k + packed 1x1 stage of a CP layer, fused
//   admmq::fixed_quantize, packed_gemm_act, packed_dwgemm_act   fixed-range activation quantizers
//   admmq::act_encode, act_decode, packed_rowsums, packed_igemm   activation codes and the int8-MFMA GEMM
//   admmq::packed_taps_i8, packed_idwgemm   int8 tap image and the integer fused depthwise + 1x1 stage
//   admmq::quantize_channel        <- source/quantization.py:29-33, 91-106 (channel_* schemes with a dim)
//   admmq::cp_gram_mttkrp          <- scripts/factorize.py:215-237 / :276-287 (G, F of one mode)
//   admmq::cp_rel_error            <- scripts/factorize.py:246-253 + source/admm.py:14-15
// Registered for the CUDA dispatch key (HIP tensors on ROCm builds of PyTorch), with
// Meta kernels for shape propagation (fake tensors / torch.compile tracing). There is
// no CPU kernel: CPU tensors fail in the dispatcher.
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <ATen/core/grad_mode.h>
#include <c10/core/DeviceGuard.h>
#include <c10/util/Exception.h>

#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/admmq.h"

namespace {

void check_rc(int32_t rc, const char* what) {
  TORCH_CHECK(rc == ADMMQ_OK, "admmq: ", what, " failed (status ", rc, "): ", admmq_last_error());
}

void check_f32_device(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "admmq: ", name, " must live on a ROCm GPU (the MI355X path has no CPU implementation)");
  TORCH_CHECK(t.scalar_type() == at::kFloat, "admmq: ", name, " must be float32, got ", t.scalar_type());
}

// every tensor of a call on one device: the workspace, the stream and the launches use it
void check_same_device(const at::Tensor& t, const at::Tensor& ref, const char* name) {
  TORCH_CHECK(t.device() == ref.device(), "admmq: ", name, " is on ", t.device(), " but the call's first tensor is on ",
              ref.device());
}

void* stream_of(const at::Tensor& t) {
  return static_cast<void*>(c10::hip::getCurrentHIPStream(t.device().index()).stream());
}

at::Tensor workspace(size_t nbytes, const at::Tensor& like) {
  return at::empty({static_cast<int64_t>(std::max<size_t>(nbytes, 256))}, like.options().dtype(at::kByte));
}

// Calls whose internal fault was repaired by a re-run (check_fault), process-wide:
// admmq::fault_repairs (expected 0 on an undisturbed device)
std::atomic<int64_t> g_fault_repairs{0};
int64_t fault_repairs(bool reset) { return reset ? g_fault_repairs.exchange(0) : g_fault_repairs.load(); }

// --- admm_iteration_batched -------------------------------------------------------
// solve: -1 = the process default (admmq_set_solve_mode; fp32 unless changed), else
// ADMMQ_SOLVE_FP32 / ADMMQ_SOLVE_SPLIT for this call.
// check_fault (default): the call syncs once at its end to read the internal-fault column
// of `info`: when the fused finalize's bounded wait timed out somewhere (its launch's
// blocks were not all resident), the call restores U and re-runs with the separate
// finalize launch, so it never returns unfinalized factors (same results as an
// undisturbed run). check_fault = false: no sync; the caller must check info[:, 3]
// itself and repeat the call (with U restored) where it is nonzero. The returned info is
// [n, 5]: the C-ABI's {iterations run, converged, spd_error, internal fault} plus the
// re-runs this call made (0, or 1 after a repaired fault; also counted in fault_repairs).
std::tuple<std::vector<at::Tensor>, at::Tensor, std::vector<at::Tensor>, std::vector<at::Tensor>> admm_batched_cuda(
    at::TensorList H, at::TensorList U, at::TensorList F, at::TensorList G, int64_t max_iter, double eps,
    int64_t bits, int64_t qscheme, int64_t num_attempts, bool check_spd, bool debug, int64_t solve,
    bool check_fault) {
  const size_t n = H.size();
  TORCH_CHECK(n > 0, "admmq: admm_iteration_batched needs at least one problem");
  TORCH_CHECK(U.size() == n && F.size() == n && G.size() == n, "admmq: H, U, F, G lists differ in length");
  check_f32_device(H[0], "H");
  const c10::DeviceGuard guard(H[0].device());
  std::vector<at::Tensor> Hc, Uc, Fc, Gc, outs, hts, xs;
  std::vector<admmq_problem> probs(n);
  for (size_t i = 0; i < n; ++i) {
    check_f32_device(H[i], "H"); check_f32_device(U[i], "U"); check_f32_device(F[i], "F"); check_f32_device(G[i], "G");
    check_same_device(H[i], H[0], "H"); check_same_device(U[i], H[0], "U");
    check_same_device(F[i], H[0], "F"); check_same_device(G[i], H[0], "G");
    TORCH_CHECK(H[i].dim() == 2, "admm_iteration expects 2-D factors (I, R)");
    const int64_t I = H[i].size(0), R = H[i].size(1);
    TORCH_CHECK(F[i].sizes() == H[i].sizes() && U[i].sizes() == H[i].sizes() && G[i].dim() == 2 &&
                    G[i].size(0) == R && G[i].size(1) == R,
                "admm_iteration: shape mismatch H", H[i].sizes(), " U", U[i].sizes(), " F", F[i].sizes(), " G",
                G[i].sizes());
    Hc.push_back(H[i].contiguous()); Uc.push_back(U[i].contiguous());
    Fc.push_back(F[i].contiguous()); Gc.push_back(G[i].contiguous());
    outs.push_back(at::empty_like(Hc.back()));
    if (debug) { hts.push_back(at::empty_like(Hc.back())); xs.push_back(at::empty_like(Hc.back())); }
    admmq_problem& p = probs[i];
    p.F = Fc.back().data_ptr<float>(); p.G = Gc.back().data_ptr<float>(); p.H0 = Hc.back().data_ptr<float>();
    p.H_out = outs.back().data_ptr<float>(); p.U = Uc.back().data_ptr<float>();
    p.HT_out = debug ? hts.back().data_ptr<float>() : nullptr;
    p.X_out = debug ? xs.back().data_ptr<float>() : nullptr;
    p.I = static_cast<int32_t>(I); p.R = static_cast<int32_t>(R);
  }
  admmq_admm_options opt;
  check_rc(admmq_admm_default_options(&opt), "default_options");
  if (solve >= 0) opt.solve_mode = static_cast<int32_t>(solve);
  const at::Tensor& ref = Hc[0];
  void* stream = stream_of(ref);
  const int32_t nn = static_cast<int32_t>(n);
  const int32_t na = static_cast<int32_t>(num_attempts);
  const size_t nb = admmq_admm_workspace_size_ex(probs.data(), nn, na, &opt);
  TORCH_CHECK(nb != 0, "admmq: admm workspace planning failed: ", admmq_last_error());
  at::Tensor ws = workspace(nb, ref);
  at::Tensor info5 = at::zeros({nn, 5}, ref.options().dtype(at::kInt));
  at::Tensor info = at::zeros({nn, 4}, ref.options().dtype(at::kInt));   // the C-ABI's int32[nprob * 4]
  check_rc(admmq_admm_prepare_ex(probs.data(), nn, na, &opt, ws.data_ptr(), ws.numel(), stream), "admm_prepare");
  if (check_spd || max_iter <= 1) {
    // source/admm.py:54 raises before anything is modified: one sync per call
    check_rc(admmq_admm_run_ex(probs.data(), nn, 1, 0.f, 4, 0, na, &opt, ws.data_ptr(), ws.numel(),
                               info.data_ptr<int32_t>(), stream),
             "admm_info");
    TORCH_CHECK_LINALG(info.select(1, 2).max().item<int32_t>() == 0,
                       "linalg.cholesky: The factorization could not be completed because the input is not "
                       "positive-definite.");
  }
  auto info_out = [&](int64_t reruns) {
    info5.narrow(1, 0, 4).copy_(info);
    if (reruns) info5.select(1, 4).fill_(reruns);
    return info5;
  };
  if (max_iter <= 1) {   // the reference returns H unchanged (the Python drop-in returns the caller's object)
    std::vector<at::Tensor> same;
    for (const at::Tensor& h : H) same.push_back(h.clone());
    return {same, info_out(0), hts, xs};
  }
  std::vector<at::Tensor> ubak;   // U before the run: restored if the run must be repeated
  if (check_fault)
    for (const at::Tensor& u : Uc) ubak.push_back(u.clone());
  auto run = [&]() {
    check_rc(admmq_admm_run_ex(probs.data(), nn, static_cast<int32_t>(max_iter), static_cast<float>(eps),
                               static_cast<int32_t>(bits), static_cast<int32_t>(qscheme), na, &opt, ws.data_ptr(),
                               ws.numel(), info.data_ptr<int32_t>(), stream),
             "admm_run");
  };
  run();
  int64_t reruns = 0;
  if (check_fault && info.select(1, 3).max().item<int32_t>() != 0) {   // internal fault: repeat without the fused finalize
    for (size_t i = 0; i < n; ++i) Uc[i].copy_(ubak[i]);
    opt.fused_finalize = 0;
    check_rc(admmq_admm_prepare_ex(probs.data(), nn, na, &opt, ws.data_ptr(), ws.numel(), stream), "admm_prepare");
    run();
    TORCH_CHECK(info.select(1, 3).max().item<int32_t>() == 0, "admmq: internal fault in the separate-finalize re-run");
    reruns = 1;
    g_fault_repairs.fetch_add(1);
  }
  for (size_t i = 0; i < n; ++i)   // U is updated in place (source/admm.py:60)
    if (!U[i].is_same(Uc[i])) const_cast<at::Tensor&>(U[i]).copy_(Uc[i]);
  return {outs, info_out(reruns), hts, xs};
}

std::tuple<std::vector<at::Tensor>, at::Tensor, std::vector<at::Tensor>, std::vector<at::Tensor>> admm_batched_meta(
    at::TensorList H, at::TensorList U, at::TensorList F, at::TensorList G, int64_t max_iter, double eps,
    int64_t bits, int64_t qscheme, int64_t num_attempts, bool check_spd, bool debug, int64_t solve,
    bool check_fault) {
  std::vector<at::Tensor> outs, hts, xs;
  for (const at::Tensor& h : H) {
    outs.push_back(at::empty_like(h));
    if (debug) { hts.push_back(at::empty_like(h)); xs.push_back(at::empty_like(h)); }
  }
  const int64_t n = static_cast<int64_t>(H.size());
  return {outs, at::empty({n, 5}, H[0].options().dtype(at::kInt)), hts, xs};
}

// --- quantize_batched ----------------------------------------------------------------
std::vector<at::Tensor> quantize_batched_cuda(at::TensorList x, int64_t bits, int64_t qscheme, int64_t num_attempts,
                                              std::optional<double> tmin, std::optional<double> tmax) {
  TORCH_CHECK(!x.empty(), "admmq: quantize_batched needs at least one tensor");
  TORCH_CHECK(bits >= 1, "admmq: bits must be >= 1");
  check_f32_device(x[0], "tensor");
  const c10::DeviceGuard guard(x[0].device());
  const bool has_kw = qscheme == ADMMQ_TENSOR_AFFINE && tmin.has_value() && tmax.has_value();
  std::vector<at::Tensor> xs, ys;
  std::vector<admmq_qtensor> items(x.size());
  for (size_t i = 0; i < x.size(); ++i) {
    check_f32_device(x[i], "tensor");
    check_same_device(x[i], x[0], "tensor");
    TORCH_CHECK(x[i].numel() > 0, "min(): Expected reduction dim to be specified for input.numel() == 0.");
    xs.push_back(x[i].contiguous());
    ys.push_back(at::empty_like(xs.back()));
    const int64_t cols = xs.back().dim() == 0 ? 1 : xs.back().size(-1);
    admmq_qtensor& t = items[i];
    t.x = xs.back().data_ptr<float>(); t.y = ys.back().data_ptr<float>();
    t.rows = xs.back().numel() / cols; t.cols = cols;
    t.tmin = has_kw ? static_cast<float>(*tmin) : 0.f; t.tmax = has_kw ? static_cast<float>(*tmax) : 0.f;
    t.has_minmax = has_kw ? 1 : 0; t.reserved = 0;
  }
  const int32_t n = static_cast<int32_t>(items.size());
  const size_t nb = admmq_quantize_workspace_size(items.data(), n, static_cast<int32_t>(num_attempts));
  TORCH_CHECK(nb != 0, "admmq: quantize workspace planning failed: ", admmq_last_error());
  at::Tensor ws = workspace(nb, xs[0]);
  check_rc(admmq_quantize_batched(items.data(), n, static_cast<int32_t>(bits), static_cast<int32_t>(qscheme),
                                  static_cast<int32_t>(num_attempts), ws.data_ptr(), ws.numel(), stream_of(xs[0])),
           "quantize_batched");
  return ys;
}

std::vector<at::Tensor> quantize_batched_meta(at::TensorList x, int64_t bits, int64_t qscheme, int64_t num_attempts,
                                              std::optional<double> tmin, std::optional<double> tmax) {
  std::vector<at::Tensor> ys;
  for (const at::Tensor& t : x) ys.push_back(at::empty_like(t, t.options().memory_format(at::MemoryFormat::Contiguous)));
  return ys;
}

// --- quantize_packed / dequantize_packed ------------------------------------------------------
// codes[i]: uint8 [ceil(numel * bits / 8)]; meta: int32 [n, 8], the words of admmq_qmeta.
std::tuple<std::vector<at::Tensor>, at::Tensor> quantize_packed_cuda(at::TensorList x, int64_t bits, int64_t qscheme,
                                                                     int64_t num_attempts, std::optional<double> tmin,
                                                                     std::optional<double> tmax) {
  static_assert(sizeof(admmq_qmeta) == 32, "meta is int32 [n, 8]");
  TORCH_CHECK(!x.empty(), "admmq: quantize_packed needs at least one tensor");
  TORCH_CHECK(bits >= 1 && bits <= 8, "admmq: quantize_packed: bits must be 1..8");
  check_f32_device(x[0], "tensor");
  const c10::DeviceGuard guard(x[0].device());
  const bool has_kw = qscheme == ADMMQ_TENSOR_AFFINE && tmin.has_value() && tmax.has_value();
  std::vector<at::Tensor> xs, cs;
  std::vector<admmq_qtensor> items(x.size());
  std::vector<uint8_t*> cptr(x.size());
  for (size_t i = 0; i < x.size(); ++i) {
    check_f32_device(x[i], "tensor");
    check_same_device(x[i], x[0], "tensor");
    TORCH_CHECK(x[i].numel() > 0, "admmq: quantize_packed: empty tensor");
    xs.push_back(x[i].contiguous());
    cs.push_back(at::empty({static_cast<int64_t>(admmq_packed_bytes(xs.back().numel(), static_cast<int32_t>(bits)))},
                           xs.back().options().dtype(at::kByte)));
    cptr[i] = cs.back().data_ptr<uint8_t>();
    const int64_t cols = xs.back().dim() == 0 ? 1 : xs.back().size(-1);
    admmq_qtensor& t = items[i];
    t.x = xs.back().data_ptr<float>(); t.y = nullptr;
    t.rows = xs.back().numel() / cols; t.cols = cols;
    t.tmin = has_kw ? static_cast<float>(*tmin) : 0.f; t.tmax = has_kw ? static_cast<float>(*tmax) : 0.f;
    t.has_minmax = has_kw ? 1 : 0; t.reserved = 0;
  }
  const int32_t n = static_cast<int32_t>(items.size());
  at::Tensor meta = at::empty({n, 8}, xs[0].options().dtype(at::kInt));
  const size_t nb = admmq_quantize_packed_workspace_size(items.data(), n, static_cast<int32_t>(num_attempts));
  TORCH_CHECK(nb != 0, "admmq: quantize workspace planning failed: ", admmq_last_error());
  at::Tensor ws = workspace(nb, xs[0]);
  check_rc(admmq_quantize_packed(items.data(), cptr.data(), reinterpret_cast<admmq_qmeta*>(meta.data_ptr<int32_t>()), n,
                                 static_cast<int32_t>(bits), static_cast<int32_t>(qscheme),
                                 static_cast<int32_t>(num_attempts), ws.data_ptr(), ws.numel(), stream_of(xs[0])),
           "quantize_packed");
  return {cs, meta};
}

std::tuple<std::vector<at::Tensor>, at::Tensor> quantize_packed_meta(at::TensorList x, int64_t bits, int64_t qscheme,
                                                                     int64_t num_attempts, std::optional<double> tmin,
                                                                     std::optional<double> tmax) {
  TORCH_CHECK(bits >= 1 && bits <= 8, "admmq: quantize_packed: bits must be 1..8");
  std::vector<at::Tensor> cs;
  for (const at::Tensor& t : x) cs.push_back(at::empty({(t.numel() * bits + 7) / 8}, t.options().dtype(at::kByte)));
  return {cs, at::empty({static_cast<int64_t>(x.size()), 8}, x[0].options().dtype(at::kInt))};
}

std::vector<at::Tensor> dequantize_packed_cuda(at::TensorList codes, const at::Tensor& meta, at::IntArrayRef numel) {
  const size_t n = codes.size();
  TORCH_CHECK(n > 0, "admmq: dequantize_packed needs at least one tensor");
  TORCH_CHECK(numel.size() == n, "admmq: dequantize_packed: codes and numel differ in length");
  TORCH_CHECK(meta.is_cuda() && meta.scalar_type() == at::kInt && meta.dim() == 2 &&
                  meta.size(0) == static_cast<int64_t>(n) && meta.size(1) == 8,
              "admmq: dequantize_packed: meta must be a device int32 [n, 8] tensor");
  const c10::DeviceGuard guard(meta.device());
  const at::Tensor mc = meta.contiguous();
  std::vector<at::Tensor> cc, ys;
  std::vector<const uint8_t*> cptr(n);
  std::vector<float*> yptr(n);
  std::vector<int64_t> ne(numel.begin(), numel.end());
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(codes[i].is_cuda() && codes[i].scalar_type() == at::kByte, "admmq: codes must be uint8 tensors on the GPU");
    check_same_device(codes[i], meta, "codes");
    TORCH_CHECK(ne[i] > 0, "admmq: dequantize_packed: numel must be positive");
    // (the byte count for any bits <= 8 is at most numel; the kernel reads ceil(numel * bits / 8) <= codes.numel())
    cc.push_back(codes[i].contiguous());
    cptr[i] = cc.back().data_ptr<uint8_t>();
    ys.push_back(at::empty({ne[i]}, mc.options().dtype(at::kFloat)));
    yptr[i] = ys.back().data_ptr<float>();
  }
  check_rc(admmq_dequantize_packed(cptr.data(), reinterpret_cast<const admmq_qmeta*>(mc.data_ptr<int32_t>()),
                                   yptr.data(), ne.data(), static_cast<int32_t>(n), stream_of(mc)),
           "dequantize_packed");
  return ys;
}

std::vector<at::Tensor> dequantize_packed_meta(at::TensorList codes, const at::Tensor& meta, at::IntArrayRef numel) {
  std::vector<at::Tensor> ys;
  for (const int64_t ne : numel) ys.push_back(at::empty({ne}, meta.options().dtype(at::kFloat)));
  return ys;
}

// --- packed_gemm ----------------------------------------------------------------------------
// Y = W X (+ bias) with W the [M, K] de-quantization of `codes` (trans_w: of its transpose),
// decoded inside the kernel (admmq_packed_gemm). meta_words: the 8 int32 words of admmq_qmeta
// on the CPU (the host picks the kernel from its bits). x_layout 0: x [nb, K, *spatial] ->
// [nb, M, *spatial]; x_layout 1: x [..., K] -> [..., M]. Inference only: no autograd formula.
std::vector<int64_t> packed_gemm_shape(const at::Tensor& x, int64_t M, int64_t K, int64_t x_layout) {
  TORCH_CHECK(x_layout == 0 || x_layout == 1, "admmq: packed_gemm: x_layout must be 0 (NCHW) or 1 (linear)");
  TORCH_CHECK(M > 0 && K > 0, "admmq: packed_gemm: M and K must be positive");
  std::vector<int64_t> shape(x.sizes().begin(), x.sizes().end());
  if (x_layout == 0) {
    TORCH_CHECK(x.dim() >= 3 && x.size(1) == K, "admmq: packed_gemm: x must be [n, ", K, ", ...] (NCHW), got ", x.sizes());
    shape[1] = M;
  } else {
    TORCH_CHECK(x.dim() >= 1 && x.size(-1) == K, "admmq: packed_gemm: x must be [..., ", K, "], got ", x.sizes());
    shape.back() = M;
  }
  return shape;
}

// A quantizer as the ops carry it: bits (0: none) and the float32 range as schema floats (a double
// holds a float32 exactly). DESIGN.md 2.24.
admmq_actq actq_of(int64_t bits, double mn, double rng, const char* what) {
  TORCH_CHECK(bits >= 0 && bits <= 24, "admmq: ", what, ": activation quantizer bits must be 1..24 (0: none), got ", bits);
  admmq_actq q;
  q.bits = static_cast<int32_t>(bits);
  q.on = bits > 0 ? 1 : 0;
  q.mn = static_cast<float>(mn);
  q.rng = static_cast<float>(rng);
  return q;
}

// --- the call frame of the packed GEMM ops -------------------------------------
// The checks and the setup that the six packed GEMM ops share. Each piece raises under the name `who`
// of the op that calls it; the pieces are apart where the ops order them differently.
void check_inference_only(bool requires_grad, const char* who, const char* name) {
  TORCH_CHECK(!(requires_grad && at::GradMode::is_enabled()), "admmq: ", who,
              " is inference only (no backward through packed weights): call it under torch.no_grad() or detach ", name);
}

void check_codes(const at::Tensor& codes, const char* who) {
  TORCH_CHECK(codes.is_cuda() && codes.scalar_type() == at::kByte && codes.dim() == 1, "admmq: ", who,
              ": codes must be a 1-D uint8 tensor on the GPU");
}

void check_meta_words(const at::Tensor& meta_words, const char* who) {
  TORCH_CHECK(meta_words.device().is_cpu() && meta_words.scalar_type() == at::kInt && meta_words.numel() == 8, "admmq: ",
              who, ": meta_words must be the 8 int32 words of the meta record on the CPU");
}

// t contiguous at a 16-byte aligned address (a view into a larger buffer is cloned)
at::Tensor aligned16(const at::Tensor& t) {
  at::Tensor tc = t.contiguous();
  if ((reinterpret_cast<uintptr_t>(tc.data_ptr()) & 15) != 0) tc = tc.clone();
  return tc;
}

// the host meta record and the 16-byte aligned code stream of a checked [M, K] packed weight
at::Tensor packed_weight_of(const at::Tensor& codes, const at::Tensor& meta_words, int64_t M, int64_t K, const char* who,
                            admmq_qmeta& meta) {
  static_assert(sizeof(admmq_qmeta) == 32, "meta is int32 [8]");
  const at::Tensor mw = meta_words.contiguous();
  std::memcpy(&meta, mw.data_ptr<int32_t>(), sizeof(meta));
  TORCH_CHECK(meta.bits >= 1 && meta.bits <= 8, "admmq: ", who, ": bits must be 1..8");
  TORCH_CHECK(codes.numel() == static_cast<int64_t>(admmq_packed_bytes(M * K, meta.bits)), "admmq: ", who, ": a ", M, " x ",
              K, " weight with ", meta.bits, " bits needs ", admmq_packed_bytes(M * K, meta.bits), " code bytes, got ",
              codes.numel());
  return aligned16(codes);
}

// the contiguous float32 bias [M] on x's device, or an undefined tensor; refuse_grad: the integer
// ops' inference-only refusal, which they make on the bias
at::Tensor bias_of(const std::optional<at::Tensor>& bias, const at::Tensor& x, int64_t M, const char* who, bool refuse_grad) {
  if (!bias.has_value() || !bias->defined()) return at::Tensor();
  check_f32_device(*bias, "bias");
  check_same_device(*bias, x, "bias");
  if (refuse_grad) check_inference_only(bias->requires_grad(), who, "bias");
  TORCH_CHECK(bias->dim() == 1 && bias->size(0) == M, "admmq: ", who, ": bias must be [", M, "], got ", bias->sizes());
  return bias->contiguous();
}

const float* f32_or_null(const at::Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }

// batch entries nb (x_layout 1: one) and columns N per entry of a GEMM on the contiguous xc
std::pair<int32_t, int64_t> gemm_extent(const at::Tensor& xc, int64_t K, int64_t x_layout, const char* who) {
  const int64_t nb = x_layout == 0 ? xc.size(0) : 1;
  const int64_t N = x_layout == 0 ? xc.numel() / std::max<int64_t>(nb * K, 1) : xc.numel() / K;
  TORCH_CHECK(nb > 0 && N > 0, "admmq: ", who, ": empty x");
  return {static_cast<int32_t>(nb), N};
}

at::Tensor packed_gemm_impl(const at::Tensor& codes, const at::Tensor& meta_words, bool trans_w, int64_t M, int64_t K,
                            const at::Tensor& x, int64_t x_layout, const std::optional<at::Tensor>& bias,
                            const admmq_actq* out_q) {
  check_f32_device(x, "x");
  check_inference_only(x.requires_grad(), "packed_gemm", "x");
  check_codes(codes, "packed_gemm");
  check_same_device(codes, x, "codes");
  check_meta_words(meta_words, "packed_gemm");
  const std::vector<int64_t> oshape = packed_gemm_shape(x, M, K, x_layout);
  admmq_qmeta meta;
  const at::Tensor cc = packed_weight_of(codes, meta_words, M, K, "packed_gemm", meta);
  const c10::DeviceGuard guard(x.device());
  const at::Tensor xc = x.contiguous();
  const at::Tensor bc = bias_of(bias, x, M, "packed_gemm", false);
  const auto [nb, N] = gemm_extent(xc, K, x_layout, "packed_gemm");
  at::Tensor y = at::empty(oshape, xc.options());
  at::Tensor ws = workspace(admmq_packed_gemm_workspace_size(M, K, N, nb), xc);
  if (out_q) {
    check_rc(admmq_packed_gemm_act(cc.data_ptr<uint8_t>(), &meta, trans_w ? 1 : 0, M, K, xc.data_ptr<float>(),
                                   static_cast<int32_t>(x_layout), N, nb, f32_or_null(bc), y.data_ptr<float>(), out_q,
                                   ws.data_ptr(), ws.numel(), stream_of(xc)),
             "packed_gemm_act");
    return y;
  }
  check_rc(admmq_packed_gemm(cc.data_ptr<uint8_t>(), &meta, trans_w ? 1 : 0, M, K, xc.data_ptr<float>(),
                             static_cast<int32_t>(x_layout), N, nb, f32_or_null(bc), y.data_ptr<float>(), ws.data_ptr(),
                             ws.numel(), stream_of(xc)),
           "packed_gemm");
  return y;
}

at::Tensor packed_gemm_cuda(const at::Tensor& codes, const at::Tensor& meta_words, bool trans_w, int64_t M, int64_t K,
                            const at::Tensor& x, int64_t x_layout, const std::optional<at::Tensor>& bias) {
  return packed_gemm_impl(codes, meta_words, trans_w, M, K, x, x_layout, bias, nullptr);
}

// packed_gemm with the output quantizer in the kernel (admmq_packed_gemm_act); out_bits 0: none
at::Tensor packed_gemm_act_cuda(const at::Tensor& codes, const at::Tensor& meta_words, bool trans_w, int64_t M, int64_t K,
                                const at::Tensor& x, int64_t x_layout, const std::optional<at::Tensor>& bias,
                                int64_t out_bits, double out_mn, double out_rng) {
  const admmq_actq q = actq_of(out_bits, out_mn, out_rng, "packed_gemm_act");
  return packed_gemm_impl(codes, meta_words, trans_w, M, K, x, x_layout, bias, &q);
}

at::Tensor packed_gemm_act_meta(const at::Tensor& codes, const at::Tensor& meta_words, bool trans_w, int64_t M, int64_t K,
                                const at::Tensor& x, int64_t x_layout, const std::optional<at::Tensor>& bias,
                                int64_t out_bits, double out_mn, double out_rng) {
  (void)actq_of(out_bits, out_mn, out_rng, "packed_gemm_act");
  return at::empty(packed_gemm_shape(x, M, K, x_layout), x.options().dtype(at::kFloat));
}

// --- fixed_quantize -------------------------------------------------------------------------
// y = q(x) element by element (admmq_fixed_quantize, k_fixed_quant). Inference only.
at::Tensor fixed_quantize_cuda(const at::Tensor& x, int64_t bits, double mn, double rng) {
  check_f32_device(x, "x");
  TORCH_CHECK(!(x.requires_grad() && at::GradMode::is_enabled()),
              "admmq: fixed_quantize is inference only (no backward through the quantizer): call it under "
              "torch.no_grad() or detach x");
  TORCH_CHECK(bits >= 1, "admmq: fixed_quantize: activation quantizer bits must be 1..24, got ", bits);
  const admmq_actq q = actq_of(bits, mn, rng, "fixed_quantize");
  const c10::DeviceGuard guard(x.device());
  const at::Tensor xc = x.contiguous();
  at::Tensor y = at::empty_like(xc);
  if (xc.numel() == 0) return y;
  check_rc(admmq_fixed_quantize(xc.data_ptr<float>(), y.data_ptr<float>(), xc.numel(), &q, stream_of(xc)), "fixed_quantize");
  return y;
}

at::Tensor fixed_quantize_meta(const at::Tensor& x, int64_t bits, double mn, double rng) {
  TORCH_CHECK(bits >= 1 && bits <= 24, "admmq: fixed_quantize: activation quantizer bits must be 1..24, got ", bits);
  return at::empty(x.sizes(), x.options().dtype(at::kFloat));
}

// --- integer packed GEMM ---------------------------------------------------------
// Activation codes (uint8, the float tensor's shape), the row sums of a packed weight and the
// int8-MFMA GEMM over codes (admmq_act_encode / _decode, admmq_packed_rowsums, admmq_packed_igemm).
// `clamped` is an int32 [1] tensor on the device: the ops make no host read. Inference only.
admmq_actq codeq_of(int64_t bits, double mn, double rng, const char* what) {
  TORCH_CHECK(bits >= 2 && bits <= 8, "admmq: ", what, ": activation code bits must be 2..8, got ", bits);
  return actq_of(bits, mn, rng, what);
}

std::tuple<at::Tensor, at::Tensor> act_encode_cuda(const at::Tensor& x, int64_t bits, double mn, double rng) {
  check_f32_device(x, "x");
  TORCH_CHECK(!(x.requires_grad() && at::GradMode::is_enabled()),
              "admmq: act_encode is inference only (no backward through the quantizer): call it under "
              "torch.no_grad() or detach x");
  const admmq_actq q = codeq_of(bits, mn, rng, "act_encode");
  const c10::DeviceGuard guard(x.device());
  const at::Tensor xc = x.contiguous();
  at::Tensor codes = at::empty(xc.sizes(), xc.options().dtype(at::kByte));
  at::Tensor clamped = at::empty({1}, xc.options().dtype(at::kInt));
  if (xc.numel() == 0) return {codes, clamped.zero_()};
  check_rc(admmq_act_encode(xc.data_ptr<float>(), codes.data_ptr<uint8_t>(), xc.numel(), &q, clamped.data_ptr<int32_t>(),
                            stream_of(xc)),
           "act_encode");
  return {codes, clamped};
}

std::tuple<at::Tensor, at::Tensor> act_encode_meta(const at::Tensor& x, int64_t bits, double mn, double rng) {
  (void)codeq_of(bits, mn, rng, "act_encode");
  return {at::empty(x.sizes(), x.options().dtype(at::kByte)), at::empty({1}, x.options().dtype(at::kInt))};
}

at::Tensor act_decode_cuda(const at::Tensor& codes, int64_t bits, double mn, double rng) {
  TORCH_CHECK(codes.is_cuda() && codes.scalar_type() == at::kByte, "admmq: act_decode: codes must be a uint8 tensor on the GPU");
  const admmq_actq q = codeq_of(bits, mn, rng, "act_decode");
  const c10::DeviceGuard guard(codes.device());
  const at::Tensor cc = codes.contiguous();
  at::Tensor y = at::empty(cc.sizes(), cc.options().dtype(at::kFloat));
  if (cc.numel() == 0) return y;
  check_rc(admmq_act_decode(cc.data_ptr<uint8_t>(), y.data_ptr<float>(), cc.numel(), &q, stream_of(cc)), "act_decode");
  return y;
}

at::Tensor act_decode_meta(const at::Tensor& codes, int64_t bits, double mn, double rng) {
  (void)codeq_of(bits, mn, rng, "act_decode");
  return at::empty(codes.sizes(), codes.options().dtype(at::kFloat));
}

// packed_weight_of behind the integer ops' checks of its arguments (the float ops make theirs around
// their device and shape checks)
at::Tensor int_weight_of(const at::Tensor& codes, const at::Tensor& meta_words, int64_t M, int64_t K, const char* who,
                         admmq_qmeta& meta) {
  check_codes(codes, who);
  check_meta_words(meta_words, who);
  TORCH_CHECK(M > 0 && K > 0, "admmq: ", who, ": M and K must be positive");
  return packed_weight_of(codes, meta_words, M, K, who, meta);
}

// the output quantizer of an integer op: a code quantizer when the output is codes
admmq_actq outq_of(bool out_codes, int64_t bits, double mn, double rng, const char* who) {
  return out_codes ? codeq_of(bits, mn, rng, who) : actq_of(bits, mn, rng, who);
}

void check_rowsums(const at::Tensor& rowsums, const at::Tensor& x, int64_t M, const char* who) {
  TORCH_CHECK(rowsums.is_cuda() && rowsums.scalar_type() == at::kInt && rowsums.dim() == 1 && rowsums.size(0) == M,
              "admmq: ", who, ": rowsums must be an int32 [", M, "] tensor on the GPU");
  check_same_device(rowsums, x, "rowsums");
}

at::Tensor packed_rowsums_cuda(const at::Tensor& codes, const at::Tensor& meta_words, bool trans_w, int64_t M, int64_t K) {
  admmq_qmeta meta;
  const at::Tensor cc = int_weight_of(codes, meta_words, M, K, "packed_rowsums", meta);
  const c10::DeviceGuard guard(cc.device());
  at::Tensor A = at::empty({M}, cc.options().dtype(at::kInt));
  check_rc(admmq_packed_rowsums(cc.data_ptr<uint8_t>(), &meta, trans_w ? 1 : 0, M, K, A.data_ptr<int32_t>(), stream_of(cc)),
           "packed_rowsums");
  return A;
}

at::Tensor packed_rowsums_meta(const at::Tensor& codes, const at::Tensor& meta_words, bool trans_w, int64_t M, int64_t K) {
  TORCH_CHECK(M > 0 && K > 0, "admmq: packed_rowsums: M and K must be positive");
  return at::empty({M}, codes.options().dtype(at::kInt));
}

std::tuple<at::Tensor, at::Tensor> packed_igemm_cuda(const at::Tensor& codes, const at::Tensor& meta_words, bool trans_w,
                                                     int64_t M, int64_t K, const at::Tensor& x, int64_t x_bits, double x_mn,
                                                     double x_rng, const at::Tensor& rowsums, int64_t x_layout,
                                                     const std::optional<at::Tensor>& bias, int64_t out_bits, double out_mn,
                                                     double out_rng, bool out_codes) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kByte, "admmq: packed_igemm: x must be a uint8 code tensor on the GPU");
  const admmq_actq xq = codeq_of(x_bits, x_mn, x_rng, "packed_igemm");
  const admmq_actq oq = outq_of(out_codes, out_bits, out_mn, out_rng, "packed_igemm");
  admmq_qmeta meta;
  const at::Tensor cc = int_weight_of(codes, meta_words, M, K, "packed_igemm", meta);
  check_same_device(codes, x, "codes");
  check_rowsums(rowsums, x, M, "packed_igemm");
  const std::vector<int64_t> oshape = packed_gemm_shape(x, M, K, x_layout);
  const c10::DeviceGuard guard(x.device());
  const at::Tensor xc = x.contiguous();
  const at::Tensor rc = rowsums.contiguous();
  const at::Tensor bc = bias_of(bias, x, M, "packed_igemm", true);
  const auto [nb, N] = gemm_extent(xc, K, x_layout, "packed_igemm");
  at::Tensor y = at::empty(oshape, xc.options().dtype(out_codes ? at::kByte : at::kFloat));
  at::Tensor clamped = at::empty({out_codes ? 1 : 0}, xc.options().dtype(at::kInt));
  const size_t nbytes = admmq_packed_igemm_workspace_size(M, K, N, nb);
  at::Tensor ws;   // (the serial regime needs none: no allocation)
  if (nbytes > 0) ws = workspace(nbytes, xc);
  check_rc(admmq_packed_igemm(cc.data_ptr<uint8_t>(), &meta, trans_w ? 1 : 0, M, K, xc.data_ptr<uint8_t>(), &xq,
                              rc.data_ptr<int32_t>(), static_cast<int32_t>(x_layout), N, nb, f32_or_null(bc),
                              out_codes ? nullptr : y.data_ptr<float>(), out_codes ? y.data_ptr<uint8_t>() : nullptr, &oq,
                              out_codes ? clamped.data_ptr<int32_t>() : nullptr, nbytes > 0 ? ws.data_ptr() : nullptr,
                              nbytes > 0 ? static_cast<size_t>(ws.numel()) : 0, stream_of(xc)),
           "packed_igemm");
  return {y, clamped};
}

std::tuple<at::Tensor, at::Tensor> packed_igemm_meta(const at::Tensor& codes, const at::Tensor& meta_words, bool trans_w,
                                                     int64_t M, int64_t K, const at::Tensor& x, int64_t x_bits, double x_mn,
                                                     double x_rng, const at::Tensor& rowsums, int64_t x_layout,
                                                     const std::optional<at::Tensor>& bias, int64_t out_bits, double out_mn,
                                                     double out_rng, bool out_codes) {
  (void)codeq_of(x_bits, x_mn, x_rng, "packed_igemm");
  (void)outq_of(out_codes, out_bits, out_mn, out_rng, "packed_igemm");
  return {at::empty(packed_gemm_shape(x, M, K, x_layout), x.options().dtype(out_codes ? at::kByte : at::kFloat)),
          at::empty({out_codes ? 1 : 0}, x.options().dtype(at::kInt))};
}

// --- integer fused depthwise + 1x1 -------------------------------------------------
// packed_taps_i8: the int8 image [ntaps, Kp] of a packed depthwise factor (once per weight);
// packed_idwgemm: admmq_packed_idwgemm on the codes x [nb, K, H, W] -> [nb, M, Ho, Wo] (float or
// codes). Both counters are int32 [1] device tensors (clamped is empty without a codes output,
// mid_clamped without count_mid: a counter that is not asked for costs no memset).
// Kp of the image [ntaps, Kp]: K rounded up to the integer GEMM's K step, which is the library's
// image size for one tap and K = 1 (so an out-of-range K still gets its rounded-up figure in a message)
int64_t taps_kp(int64_t K) {
  const int64_t step = static_cast<int64_t>(admmq_packed_taps_i8_bytes(1, 1));
  return step * ((K + step - 1) / step);
}

// The output shape [n, M, Ho, Wo] of a fused depthwise + 1x1 op `who` on x [n, K, H, W]; its
// depthwise factor `taps_name` must be [kh kw, taps_cols].
std::vector<int64_t> packed_dw_shape(const char* who, const char* taps_name, int64_t taps_cols, const at::Tensor& x,
                                     const at::Tensor& taps, int64_t M, int64_t K, int64_t kh, int64_t kw, int64_t sh,
                                     int64_t sw, int64_t ph, int64_t pw) {
  TORCH_CHECK(M > 0 && K > 0, "admmq: ", who, ": M and K must be positive");
  TORCH_CHECK(x.dim() == 4 && x.size(1) == K, "admmq: ", who, ": x must be [n, ", K, ", H, W], got ", x.sizes());
  TORCH_CHECK(kh >= 1 && kh <= 7 && kw >= 1 && kw <= 7, "admmq: ", who, ": kernel size must be 1..7 x 1..7");
  TORCH_CHECK(sh >= 1 && sw >= 1, "admmq: ", who, ": stride must be at least 1");
  TORCH_CHECK(ph >= 0 && ph < kh && pw >= 0 && pw < kw, "admmq: ", who, ": padding must be in [0, kernel size)");
  TORCH_CHECK(taps.dim() == 2 && taps.size(0) == kh * kw && taps.size(1) == taps_cols, "admmq: ", who, ": ", taps_name,
              " must be [", kh * kw, ", ", taps_cols, "], got ", taps.sizes());
  const int64_t H = x.size(2), W = x.size(3);
  TORCH_CHECK(H + 2 * ph >= kh && W + 2 * pw >= kw, "admmq: ", who, ": the ", kh, " x ", kw,
              " window does not fit the padded image of x ", x.sizes());
  return {x.size(0), M, (H + 2 * ph - kh) / sh + 1, (W + 2 * pw - kw) / sw + 1};
}

at::Tensor packed_taps_i8_cuda(const at::Tensor& codes, const at::Tensor& meta_words, int64_t ntaps, int64_t K) {
  TORCH_CHECK(ntaps >= 1 && ntaps <= 49, "admmq: packed_taps_i8: ntaps must be 1..49, got ", ntaps);
  admmq_qmeta meta;
  const at::Tensor cc = int_weight_of(codes, meta_words, ntaps, K, "packed_taps_i8", meta);
  const c10::DeviceGuard guard(cc.device());
  at::Tensor image = at::empty({ntaps, taps_kp(K)}, cc.options().dtype(at::kChar));
  check_rc(admmq_packed_taps_i8(cc.data_ptr<uint8_t>(), &meta, static_cast<int32_t>(ntaps), K, image.data_ptr<int8_t>(),
                                stream_of(cc)),
           "packed_taps_i8");
  return image;
}

at::Tensor packed_taps_i8_meta(const at::Tensor& codes, const at::Tensor& meta_words, int64_t ntaps, int64_t K) {
  TORCH_CHECK(ntaps >= 1 && ntaps <= 49, "admmq: packed_taps_i8: ntaps must be 1..49, got ", ntaps);
  TORCH_CHECK(K > 0, "admmq: packed_taps_i8: K must be positive");
  return at::empty({ntaps, taps_kp(K)}, codes.options().dtype(at::kChar));
}

std::vector<int64_t> packed_idwgemm_shape(const at::Tensor& x, const at::Tensor& taps, int64_t M, int64_t K, int64_t kh,
                                          int64_t kw, int64_t sh, int64_t sw, int64_t ph, int64_t pw) {
  return packed_dw_shape("packed_idwgemm", "taps_i8", taps_kp(K), x, taps, M, K, kh, kw, sh, sw, ph, pw);
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> packed_idwgemm_cuda(
    const at::Tensor& codes, const at::Tensor& meta_words, int64_t M, int64_t K, const at::Tensor& x, int64_t x_bits,
    double x_mn, double x_rng, const at::Tensor& taps_i8, double s_c, int64_t kh, int64_t kw, int64_t sh, int64_t sw,
    int64_t ph, int64_t pw, const at::Tensor& rowsums, const std::optional<at::Tensor>& bias, int64_t mid_bits,
    double mid_mn, double mid_rng, int64_t out_bits, double out_mn, double out_rng, bool out_codes, bool count_mid) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kByte, "admmq: packed_idwgemm: x must be a uint8 code tensor on the GPU");
  TORCH_CHECK(taps_i8.is_cuda() && taps_i8.scalar_type() == at::kChar,
              "admmq: packed_idwgemm: taps_i8 must be an int8 tensor on the GPU (packed_taps_i8 makes it)");
  const admmq_actq xq = codeq_of(x_bits, x_mn, x_rng, "packed_idwgemm");
  const admmq_actq mq = codeq_of(mid_bits, mid_mn, mid_rng, "packed_idwgemm");
  const admmq_actq oq = outq_of(out_codes, out_bits, out_mn, out_rng, "packed_idwgemm");
  admmq_qmeta meta;
  const at::Tensor cc = int_weight_of(codes, meta_words, M, K, "packed_idwgemm", meta);
  check_same_device(codes, x, "codes");
  check_same_device(taps_i8, x, "taps_i8");
  check_rowsums(rowsums, x, M, "packed_idwgemm");
  const std::vector<int64_t> oshape = packed_idwgemm_shape(x, taps_i8, M, K, kh, kw, sh, sw, ph, pw);
  TORCH_CHECK(std::max(sh, sw) <= INT32_MAX && x.size(0) <= INT32_MAX, "admmq: packed_idwgemm: sizes out of range");
  TORCH_CHECK(x.numel() > 0, "admmq: packed_idwgemm: empty x");
  const c10::DeviceGuard guard(x.device());
  const at::Tensor xc = x.contiguous();
  const at::Tensor rc = rowsums.contiguous();
  const at::Tensor tc = aligned16(taps_i8);
  const at::Tensor bc = bias_of(bias, x, M, "packed_idwgemm", true);
  const int32_t nb = static_cast<int32_t>(xc.size(0));
  at::Tensor y = at::empty(oshape, xc.options().dtype(out_codes ? at::kByte : at::kFloat));
  at::Tensor mid_clamped = at::empty({count_mid ? 1 : 0}, xc.options().dtype(at::kInt));   // (not counted: no memset)
  at::Tensor clamped = at::empty({out_codes ? 1 : 0}, xc.options().dtype(at::kInt));
  const size_t nbytes = admmq_packed_idwgemm_workspace_size(M, K, oshape[2], oshape[3], nb);
  at::Tensor ws;   // (the serial regime needs none: no allocation)
  if (nbytes > 0) ws = workspace(nbytes, xc);
  check_rc(admmq_packed_idwgemm(cc.data_ptr<uint8_t>(), &meta, M, K, xc.data_ptr<uint8_t>(), &xq, nb, xc.size(2), xc.size(3),
                                tc.data_ptr<int8_t>(), static_cast<float>(s_c), static_cast<int32_t>(kh),
                                static_cast<int32_t>(kw), static_cast<int32_t>(sh), static_cast<int32_t>(sw),
                                static_cast<int32_t>(ph), static_cast<int32_t>(pw), rc.data_ptr<int32_t>(),
                                f32_or_null(bc), out_codes ? nullptr : y.data_ptr<float>(),
                                out_codes ? y.data_ptr<uint8_t>() : nullptr, &mq, &oq, count_mid ? mid_clamped.data_ptr<int32_t>() : nullptr,
                                out_codes ? clamped.data_ptr<int32_t>() : nullptr, nbytes > 0 ? ws.data_ptr() : nullptr,
                                nbytes > 0 ? static_cast<size_t>(ws.numel()) : 0, stream_of(xc)),
           "packed_idwgemm");
  return {y, mid_clamped, clamped};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> packed_idwgemm_meta(
    const at::Tensor& codes, const at::Tensor& meta_words, int64_t M, int64_t K, const at::Tensor& x, int64_t x_bits,
    double x_mn, double x_rng, const at::Tensor& taps_i8, double s_c, int64_t kh, int64_t kw, int64_t sh, int64_t sw,
    int64_t ph, int64_t pw, const at::Tensor& rowsums, const std::optional<at::Tensor>& bias, int64_t mid_bits,
    double mid_mn, double mid_rng, int64_t out_bits, double out_mn, double out_rng, bool out_codes, bool count_mid) {
  (void)codeq_of(x_bits, x_mn, x_rng, "packed_idwgemm");
  (void)codeq_of(mid_bits, mid_mn, mid_rng, "packed_idwgemm");
  (void)outq_of(out_codes, out_bits, out_mn, out_rng, "packed_idwgemm");
  return {at::empty(packed_idwgemm_shape(x, taps_i8, M, K, kh, kw, sh, sw, ph, pw),
                    x.options().dtype(out_codes ? at::kByte : at::kFloat)),
          at::empty({count_mid ? 1 : 0}, x.options().dtype(at::kInt)),
          at::empty({out_codes ? 1 : 0}, x.options().dtype(at::kInt))};
}

at::Tensor packed_gemm_meta(const at::Tensor& codes, const at::Tensor& meta_words, bool trans_w, int64_t M, int64_t K,
                            const at::Tensor& x, int64_t x_layout, const std::optional<at::Tensor>& bias) {
  return at::empty(packed_gemm_shape(x, M, K, x_layout), x.options().dtype(at::kFloat));
}

// --- packed_hgemm ---------------------------------------------------------------------------
// packed_gemm on bfloat16 / float16 activations (admmq_packed_hgemm): the result
// has x's dtype, or float32 with out_f32. bias: float32. Inference only.
at::Tensor packed_hgemm_cuda(const at::Tensor& codes, const at::Tensor& meta_words, bool trans_w, int64_t M, int64_t K,
                             const at::Tensor& x, int64_t x_layout, const std::optional<at::Tensor>& bias, bool out_f32) {
  TORCH_CHECK(x.is_cuda(), "admmq: x must live on a ROCm GPU (the MI355X path has no CPU implementation)");
  TORCH_CHECK(x.scalar_type() == at::kHalf || x.scalar_type() == at::kBFloat16,
              "admmq: packed_hgemm: x must be float16 or bfloat16, got ", x.scalar_type());
  check_inference_only(x.requires_grad(), "packed_gemm", "x");
  check_codes(codes, "packed_hgemm");
  check_same_device(codes, x, "codes");
  check_meta_words(meta_words, "packed_hgemm");
  const std::vector<int64_t> oshape = packed_gemm_shape(x, M, K, x_layout);
  admmq_qmeta meta;
  const at::Tensor cc = packed_weight_of(codes, meta_words, M, K, "packed_hgemm", meta);
  const c10::DeviceGuard guard(x.device());
  const at::Tensor xc = x.contiguous();
  const at::Tensor bc = bias_of(bias, x, M, "packed_hgemm", false);
  const auto [nb, N] = gemm_extent(xc, K, x_layout, "packed_hgemm");
  const int32_t xdt = x.scalar_type() == at::kHalf ? ADMMQ_DT_F16 : ADMMQ_DT_BF16;
  at::Tensor y = at::empty(oshape, out_f32 ? xc.options().dtype(at::kFloat) : xc.options());
  at::Tensor ws = workspace(admmq_packed_hgemm_workspace_size(&meta, M, K, N, nb), xc);
  check_rc(admmq_packed_hgemm(cc.data_ptr<uint8_t>(), &meta, trans_w ? 1 : 0, M, K, xc.data_ptr(), xdt,
                              static_cast<int32_t>(x_layout), N, nb, f32_or_null(bc), y.data_ptr(),
                              out_f32 ? ADMMQ_DT_F32 : xdt, ws.data_ptr(), ws.numel(), stream_of(xc)),
           "packed_hgemm");
  return y;
}

at::Tensor packed_hgemm_meta(const at::Tensor& codes, const at::Tensor& meta_words, bool trans_w, int64_t M, int64_t K,
                             const at::Tensor& x, int64_t x_layout, const std::optional<at::Tensor>& bias, bool out_f32) {
  TORCH_CHECK(x.scalar_type() == at::kHalf || x.scalar_type() == at::kBFloat16,
              "admmq: packed_hgemm: x must be float16 or bfloat16, got ", x.scalar_type());
  return at::empty(packed_gemm_shape(x, M, K, x_layout), out_f32 ? x.options().dtype(at::kFloat) : x.options());
}

// --- packed_lrgemm --------------------------------------------------------------------------
// y = x (D + L Rt)^T (+ bias): D the [M, K] de-quantization of `codes`, L [M, r], Rt [r, K]
// (admmq_packed_lrgemm). x [..., K] -> [..., M]. Inference only.
std::vector<int64_t> packed_lrgemm_shape(const at::Tensor& x, const at::Tensor& L, const at::Tensor& Rt, int64_t M, int64_t K) {
  TORCH_CHECK(M > 0 && K > 0, "admmq: packed_lrgemm: M and K must be positive");
  TORCH_CHECK(L.dim() == 2 && Rt.dim() == 2 && L.size(0) == M && Rt.size(1) == K && L.size(1) == Rt.size(0),
              "admmq: packed_lrgemm: L must be [", M, ", r] and Rt [r, ", K, "], got ", L.sizes(), " and ", Rt.sizes());
  TORCH_CHECK(L.size(1) >= 1 && L.size(1) <= 256, "admmq: packed_lrgemm: rank r must be 1..256, got ", L.size(1));
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) == K, "admmq: packed_lrgemm: x must be [..., ", K, "], got ", x.sizes());
  std::vector<int64_t> shape(x.sizes().begin(), x.sizes().end());
  shape.back() = M;
  return shape;
}

at::Tensor packed_lrgemm_cuda(const at::Tensor& codes, const at::Tensor& meta_words, int64_t M, int64_t K,
                              const at::Tensor& L, const at::Tensor& Rt, const at::Tensor& x,
                              const std::optional<at::Tensor>& bias) {
  check_f32_device(x, "x");
  check_f32_device(L, "L");
  check_f32_device(Rt, "Rt");
  check_inference_only(x.requires_grad() || L.requires_grad() || Rt.requires_grad(), "packed_lrgemm", "x");
  check_codes(codes, "packed_lrgemm");
  check_same_device(codes, x, "codes");
  check_same_device(L, x, "L");
  check_same_device(Rt, x, "Rt");
  check_meta_words(meta_words, "packed_lrgemm");
  const std::vector<int64_t> oshape = packed_lrgemm_shape(x, L, Rt, M, K);
  admmq_qmeta meta;
  const at::Tensor cc = packed_weight_of(codes, meta_words, M, K, "packed_lrgemm", meta);
  const c10::DeviceGuard guard(x.device());
  const at::Tensor xc = x.contiguous(), Lc = L.contiguous(), Rc = Rt.contiguous();
  const at::Tensor bc = bias_of(bias, x, M, "packed_lrgemm", false);
  const int64_t N = gemm_extent(xc, K, 1, "packed_lrgemm").second;
  const int32_t r = static_cast<int32_t>(Lc.size(1));
  at::Tensor y = at::empty(oshape, xc.options());
  at::Tensor ws = workspace(admmq_packed_lrgemm_workspace_size(M, K, N, r), xc);
  check_rc(admmq_packed_lrgemm(cc.data_ptr<uint8_t>(), &meta, M, K, Lc.data_ptr<float>(), Rc.data_ptr<float>(), r,
                               xc.data_ptr<float>(), N, f32_or_null(bc), y.data_ptr<float>(), ws.data_ptr(), ws.numel(),
                               stream_of(xc)),
           "packed_lrgemm");
  return y;
}

at::Tensor packed_lrgemm_meta(const at::Tensor& codes, const at::Tensor& meta_words, int64_t M, int64_t K,
                              const at::Tensor& L, const at::Tensor& Rt, const at::Tensor& x,
                              const std::optional<at::Tensor>& bias) {
  return at::empty(packed_lrgemm_shape(x, L, Rt, M, K), x.options().dtype(at::kFloat));
}

// --- packed_dwgemm --------------------------------------------------------------------------
// The depthwise kh x kw stage (taps [kh kw, K]) and the 1x1 stage by the packed [M, K] weight
// in one kernel (admmq_packed_dwgemm): x [nb, K, H, W] -> [nb, M, Ho, Wo]. Inference only.
std::vector<int64_t> packed_dwgemm_shape(const at::Tensor& x, const at::Tensor& taps, int64_t M, int64_t K, int64_t kh,
                                         int64_t kw, int64_t sh, int64_t sw, int64_t ph, int64_t pw) {
  return packed_dw_shape("packed_dwgemm", "taps", K, x, taps, M, K, kh, kw, sh, sw, ph, pw);
}

at::Tensor packed_dwgemm_impl(const at::Tensor& codes, const at::Tensor& meta_words, int64_t M, int64_t K,
                              const at::Tensor& x, const at::Tensor& taps, int64_t kh, int64_t kw, int64_t sh,
                              int64_t sw, int64_t ph, int64_t pw, const std::optional<at::Tensor>& bias,
                              const admmq_actq* mid_q, const admmq_actq* out_q) {
  check_f32_device(x, "x");
  check_inference_only(x.requires_grad(), "packed_dwgemm", "x");
  check_f32_device(taps, "taps");
  check_same_device(taps, x, "taps");
  check_codes(codes, "packed_dwgemm");
  check_same_device(codes, x, "codes");
  check_meta_words(meta_words, "packed_dwgemm");
  const std::vector<int64_t> oshape = packed_dwgemm_shape(x, taps, M, K, kh, kw, sh, sw, ph, pw);
  TORCH_CHECK(std::max(sh, sw) <= INT32_MAX && x.size(0) <= INT32_MAX, "admmq: packed_dwgemm: sizes out of range");
  admmq_qmeta meta;
  const at::Tensor cc = packed_weight_of(codes, meta_words, M, K, "packed_dwgemm", meta);
  TORCH_CHECK(x.numel() > 0, "admmq: packed_dwgemm: empty x");
  const c10::DeviceGuard guard(x.device());
  const at::Tensor xc = x.contiguous();
  const at::Tensor tc = taps.detach().contiguous();
  const at::Tensor bc = bias_of(bias, x, M, "packed_dwgemm", false);
  const int32_t nb = static_cast<int32_t>(xc.size(0));
  at::Tensor y = at::empty(oshape, xc.options());
  at::Tensor ws = workspace(admmq_packed_dwgemm_workspace_size(M, K, oshape[2], oshape[3], nb), xc);
  if (mid_q || out_q) {
    check_rc(admmq_packed_dwgemm_act(cc.data_ptr<uint8_t>(), &meta, M, K, xc.data_ptr<float>(), nb, xc.size(2), xc.size(3),
                                     tc.data_ptr<float>(), static_cast<int32_t>(kh), static_cast<int32_t>(kw),
                                     static_cast<int32_t>(sh), static_cast<int32_t>(sw), static_cast<int32_t>(ph),
                                     static_cast<int32_t>(pw), f32_or_null(bc), y.data_ptr<float>(), mid_q, out_q,
                                     ws.data_ptr(), ws.numel(), stream_of(xc)),
             "packed_dwgemm_act");
    return y;
  }
  check_rc(admmq_packed_dwgemm(cc.data_ptr<uint8_t>(), &meta, M, K, xc.data_ptr<float>(), nb, xc.size(2), xc.size(3),
                               tc.data_ptr<float>(), static_cast<int32_t>(kh), static_cast<int32_t>(kw),
                               static_cast<int32_t>(sh), static_cast<int32_t>(sw), static_cast<int32_t>(ph),
                               static_cast<int32_t>(pw), f32_or_null(bc), y.data_ptr<float>(), ws.data_ptr(), ws.numel(),
                               stream_of(xc)),
           "packed_dwgemm");
  return y;
}

at::Tensor packed_dwgemm_cuda(const at::Tensor& codes, const at::Tensor& meta_words, int64_t M, int64_t K,
                              const at::Tensor& x, const at::Tensor& taps, int64_t kh, int64_t kw, int64_t sh,
                              int64_t sw, int64_t ph, int64_t pw, const std::optional<at::Tensor>& bias) {
  return packed_dwgemm_impl(codes, meta_words, M, K, x, taps, kh, kw, sh, sw, ph, pw, bias, nullptr, nullptr);
}

// packed_dwgemm with the mid and the output quantizer in the kernel (admmq_packed_dwgemm_act); bits 0: none
at::Tensor packed_dwgemm_act_cuda(const at::Tensor& codes, const at::Tensor& meta_words, int64_t M, int64_t K,
                                  const at::Tensor& x, const at::Tensor& taps, int64_t kh, int64_t kw, int64_t sh,
                                  int64_t sw, int64_t ph, int64_t pw, const std::optional<at::Tensor>& bias,
                                  int64_t mid_bits, double mid_mn, double mid_rng, int64_t out_bits, double out_mn,
                                  double out_rng) {
  const admmq_actq mq = actq_of(mid_bits, mid_mn, mid_rng, "packed_dwgemm_act");
  const admmq_actq oq = actq_of(out_bits, out_mn, out_rng, "packed_dwgemm_act");
  return packed_dwgemm_impl(codes, meta_words, M, K, x, taps, kh, kw, sh, sw, ph, pw, bias, &mq, &oq);
}

at::Tensor packed_dwgemm_act_meta(const at::Tensor& codes, const at::Tensor& meta_words, int64_t M, int64_t K,
                                  const at::Tensor& x, const at::Tensor& taps, int64_t kh, int64_t kw, int64_t sh,
                                  int64_t sw, int64_t ph, int64_t pw, const std::optional<at::Tensor>& bias,
                                  int64_t mid_bits, double mid_mn, double mid_rng, int64_t out_bits, double out_mn,
                                  double out_rng) {
  (void)actq_of(mid_bits, mid_mn, mid_rng, "packed_dwgemm_act");
  (void)actq_of(out_bits, out_mn, out_rng, "packed_dwgemm_act");
  return at::empty(packed_dwgemm_shape(x, taps, M, K, kh, kw, sh, sw, ph, pw), x.options().dtype(at::kFloat));
}

at::Tensor packed_dwgemm_meta(const at::Tensor& codes, const at::Tensor& meta_words, int64_t M, int64_t K,
                              const at::Tensor& x, const at::Tensor& taps, int64_t kh, int64_t kw, int64_t sh,
                              int64_t sw, int64_t ph, int64_t pw, const std::optional<at::Tensor>& bias) {
  return at::empty(packed_dwgemm_shape(x, taps, M, K, kh, kw, sh, sw, ph, pw), x.options().dtype(at::kFloat));
}

// --- quantize_channel (channel_symmetric / channel_affine with an explicit dim) ----------------
at::Tensor quantize_channel_cuda(const at::Tensor& x, int64_t bits, int64_t qscheme, int64_t dim) {
  check_f32_device(x, "tensor");
  const c10::DeviceGuard guard(x.device());
  TORCH_CHECK(x.dim() >= 1, "admmq: quantize_channel needs a tensor with at least one dimension");
  TORCH_CHECK(x.numel() > 0, "min(): Expected reduction dim to be specified for input.numel() == 0.");
  const at::Tensor xc = x.contiguous();
  const int64_t nd = xc.dim();
  const int64_t d = dim < 0 ? dim + nd : dim;
  TORCH_CHECK_INDEX(d >= 0 && d < nd, "Dimension out of range (expected to be in range of [", -nd, ", ", nd - 1,
                    "], but got ", dim, ")");
  const int64_t C = xc.size(d), L = xc.size(nd - 1);
  TORCH_CHECK(L == C || L == 1 || C == 1, "The size of tensor a (", L, ") must match the size of tensor b (", C,
              ") at non-singleton dimension ", nd - 1);
  std::vector<int64_t> shape(xc.sizes().begin(), xc.sizes().end());
  std::vector<int64_t> oshape = shape;
  oshape[nd - 1] = std::max(L, C);
  at::Tensor y = at::empty(oshape, xc.options());
  const size_t nb = admmq_quantize_channel_workspace_size(shape.data(), static_cast<int32_t>(nd), static_cast<int32_t>(d));
  TORCH_CHECK(nb != 0, "admmq: quantize_channel planning failed: ", admmq_last_error());
  at::Tensor ws = workspace(nb, xc);
  check_rc(admmq_quantize_channel(xc.data_ptr<float>(), y.data_ptr<float>(), shape.data(), static_cast<int32_t>(nd),
                                  static_cast<int32_t>(d), static_cast<int32_t>(bits), static_cast<int32_t>(qscheme),
                                  ws.data_ptr(), ws.numel(), stream_of(xc)),
           "quantize_channel");
  return y;
}

at::Tensor quantize_channel_meta(const at::Tensor& x, int64_t bits, int64_t qscheme, int64_t dim) {
  const int64_t nd = x.dim();
  const int64_t d = dim < 0 ? dim + nd : dim;
  std::vector<int64_t> oshape(x.sizes().begin(), x.sizes().end());
  oshape[nd - 1] = std::max(x.size(nd - 1), x.size(d));
  return at::empty(oshape, x.options());
}

// --- ALS sweep contractions ---------------------------------------------------------------
// Layer l has tensor W[l] (2-D or 3-D) and factors[off_l .. off_l + W[l].dim()), off_l the
// running sum of the layers' dims.
std::vector<admmq_cp_layer> cp_layers(at::TensorList W, at::TensorList factors, std::vector<at::Tensor>& keep,
                                      std::vector<at::Tensor>* G, std::vector<at::Tensor>* F, int64_t mode) {
  std::vector<admmq_cp_layer> L(W.size());
  size_t off = 0;
  for (size_t l = 0; l < W.size(); ++l) {
    check_f32_device(W[l], "W");
    check_same_device(W[l], W[0], "W");
    const int64_t nd = W[l].dim();
    TORCH_CHECK(nd == 2 || nd == 3, "admmq: CP layer tensor must be 2-D or 3-D, got ", nd, "-D");
    TORCH_CHECK(off + nd <= factors.size(), "admmq: too few factors for the layers");
    keep.push_back(W[l].contiguous());
    admmq_cp_layer& c = L[l];
    c.W = keep.back().data_ptr<float>();
    const int64_t R = factors[off].size(1);
    for (int64_t d = 0; d < 3; ++d) {
      c.factors[d] = nullptr;
      c.dims[d] = d < nd ? static_cast<int32_t>(W[l].size(d)) : 0;
      if (d < nd) {
        const at::Tensor& f = factors[off + d];
        check_f32_device(f, "factor");
        check_same_device(f, W[0], "factor");
        TORCH_CHECK(f.dim() == 2 && f.size(0) == W[l].size(d) && f.size(1) == R, "admmq: factor ", d, " has shape ",
                    f.sizes(), ", expected (", W[l].size(d), ", ", R, ")");
        keep.push_back(f.contiguous());
        c.factors[d] = keep.back().data_ptr<float>();
      }
    }
    c.ndim = static_cast<int32_t>(nd);
    c.R = static_cast<int32_t>(R);
    c.G = nullptr; c.F = nullptr;
    if (G) {
      TORCH_CHECK(mode >= 0 && mode < nd, "admmq: mode ", mode, " out of range for a ", nd, "-way tensor");
      G->push_back(at::empty({R, R}, W[l].options()));
      F->push_back(at::empty({W[l].size(mode), R}, W[l].options()));
      c.G = G->back().data_ptr<float>();
      c.F = F->back().data_ptr<float>();
    }
    off += nd;
  }
  return L;
}

std::tuple<std::vector<at::Tensor>, std::vector<at::Tensor>> cp_gram_mttkrp_cuda(at::TensorList W,
                                                                                 at::TensorList factors, int64_t mode) {
  TORCH_CHECK(!W.empty(), "admmq: cp_gram_mttkrp needs at least one layer");
  check_f32_device(W[0], "W");
  const c10::DeviceGuard guard(W[0].device());
  std::vector<at::Tensor> keep, G, F;
  std::vector<admmq_cp_layer> L = cp_layers(W, factors, keep, &G, &F, mode);
  const int32_t n = static_cast<int32_t>(L.size());
  const size_t nb = admmq_cp_workspace_size(L.data(), n, static_cast<int32_t>(mode));
  TORCH_CHECK(nb != 0, "admmq: cp workspace planning failed: ", admmq_last_error());
  at::Tensor ws = workspace(nb, keep[0]);
  check_rc(admmq_cp_gram_mttkrp(L.data(), n, static_cast<int32_t>(mode), ws.data_ptr(), ws.numel(), stream_of(keep[0])),
           "cp_gram_mttkrp");
  return {G, F};
}

std::tuple<std::vector<at::Tensor>, std::vector<at::Tensor>> cp_gram_mttkrp_meta(at::TensorList W,
                                                                                 at::TensorList factors, int64_t mode) {
  std::vector<at::Tensor> G, F;
  size_t off = 0;
  for (const at::Tensor& w : W) {
    const int64_t R = factors[off].size(1);
    G.push_back(at::empty({R, R}, w.options()));
    F.push_back(at::empty({w.size(mode), R}, w.options()));
    off += w.dim();
  }
  return {G, F};
}

at::Tensor cp_rel_error_cuda(at::TensorList W, at::TensorList factors) {
  TORCH_CHECK(!W.empty(), "admmq: cp_rel_error needs at least one layer");
  check_f32_device(W[0], "W");
  const c10::DeviceGuard guard(W[0].device());
  std::vector<at::Tensor> keep;
  std::vector<admmq_cp_layer> L = cp_layers(W, factors, keep, nullptr, nullptr, 0);
  const int32_t n = static_cast<int32_t>(L.size());
  at::Tensor out = at::empty({n}, keep[0].options().dtype(at::kDouble));
  const size_t nb = admmq_cp_workspace_size(L.data(), n, 0);
  TORCH_CHECK(nb != 0, "admmq: cp workspace planning failed: ", admmq_last_error());
  at::Tensor ws = workspace(nb, keep[0]);
  check_rc(admmq_cp_rel_error(L.data(), n, out.data_ptr<double>(), ws.data_ptr(), ws.numel(), stream_of(keep[0])),
           "cp_rel_error");
  return out;
}

at::Tensor cp_rel_error_meta(at::TensorList W, at::TensorList factors) {
  return at::empty({static_cast<int64_t>(W.size())}, W[0].options().dtype(at::kDouble));
}

}  // namespace

TORCH_LIBRARY(admmq, m) {
  m.def("admm_iteration_batched(Tensor[] H, Tensor(a!)[] U, Tensor[] F, Tensor[] G, int max_iter, float eps, "
        "int bits, int qscheme, int num_attempts=200, bool check_spd=True, bool debug=False, int solve=-1, bool check_fault=True) "
        "-> (Tensor[] H_out, Tensor info, Tensor[] HT, Tensor[] X)");
  m.def("quantize_batched(Tensor[] x, int bits, int qscheme, int num_attempts=200, float? tmin=None, "
        "float? tmax=None) -> Tensor[]");
  m.def("quantize_packed(Tensor[] x, int bits, int qscheme, int num_attempts=200, float? tmin=None, "
        "float? tmax=None) -> (Tensor[] codes, Tensor meta)");
  m.def("dequantize_packed(Tensor[] codes, Tensor meta, int[] numel) -> Tensor[]");
  m.def("packed_gemm(Tensor codes, Tensor meta_words, bool trans_w, int M, int K, Tensor x, int x_layout, "
        "Tensor? bias=None) -> Tensor");
  m.def("packed_hgemm(Tensor codes, Tensor meta_words, bool trans_w, int M, int K, Tensor x, int x_layout, "
        "Tensor? bias=None, bool out_f32=False) -> Tensor");
  m.def("packed_lrgemm(Tensor codes, Tensor meta_words, int M, int K, Tensor L, Tensor Rt, Tensor x, Tensor? bias=None) "
        "-> Tensor");
  m.def("packed_dwgemm(Tensor codes, Tensor meta_words, int M, int K, Tensor x, Tensor taps, int kh, int kw, int sh, "
        "int sw, int ph, int pw, Tensor? bias=None) -> Tensor");
  m.def("packed_gemm_act(Tensor codes, Tensor meta_words, bool trans_w, int M, int K, Tensor x, int x_layout, "
        "Tensor? bias, int out_bits, float out_mn, float out_rng) -> Tensor");
  m.def("packed_dwgemm_act(Tensor codes, Tensor meta_words, int M, int K, Tensor x, Tensor taps, int kh, int kw, int sh, "
        "int sw, int ph, int pw, Tensor? bias, int mid_bits, float mid_mn, float mid_rng, int out_bits, float out_mn, "
        "float out_rng) -> Tensor");
  m.def("fixed_quantize(Tensor x, int bits, float mn, float rng) -> Tensor");
  m.def("act_encode(Tensor x, int bits, float mn, float rng) -> (Tensor codes, Tensor clamped)");
  m.def("act_decode(Tensor codes, int bits, float mn, float rng) -> Tensor");
  m.def("packed_rowsums(Tensor codes, Tensor meta_words, bool trans_w, int M, int K) -> Tensor");
  m.def("packed_igemm(Tensor codes, Tensor meta_words, bool trans_w, int M, int K, Tensor x, int x_bits, float x_mn, "
        "float x_rng, Tensor rowsums, int x_layout, Tensor? bias, int out_bits, float out_mn, float out_rng, "
        "bool out_codes) -> (Tensor y, Tensor clamped)");
  m.def("packed_taps_i8(Tensor codes, Tensor meta_words, int ntaps, int K) -> Tensor");
  m.def("packed_idwgemm(Tensor codes, Tensor meta_words, int M, int K, Tensor x, int x_bits, float x_mn, float x_rng, "
        "Tensor taps_i8, float s_c, int kh, int kw, int sh, int sw, int ph, int pw, Tensor rowsums, Tensor? bias, "
        "int mid_bits, float mid_mn, float mid_rng, int out_bits, float out_mn, float out_rng, bool out_codes, "
        "bool count_mid) -> (Tensor y, Tensor mid_clamped, Tensor clamped)");
  m.def("quantize_channel(Tensor x, int bits, int qscheme, int dim) -> Tensor");
  m.def("cp_gram_mttkrp(Tensor[] W, Tensor[] factors, int mode) -> (Tensor[] G, Tensor[] F)");
  m.def("cp_rel_error(Tensor[] W, Tensor[] factors) -> Tensor");
  m.def("fault_repairs(bool reset=False) -> int", &fault_repairs);
}

TORCH_LIBRARY_IMPL(admmq, CUDA, m) {
  m.impl("admm_iteration_batched", &admm_batched_cuda);
  m.impl("quantize_batched", &quantize_batched_cuda);
  m.impl("quantize_packed", &quantize_packed_cuda);
  m.impl("dequantize_packed", &dequantize_packed_cuda);
  m.impl("packed_gemm", &packed_gemm_cuda);
  m.impl("packed_hgemm", &packed_hgemm_cuda);
  m.impl("packed_lrgemm", &packed_lrgemm_cuda);
  m.impl("packed_dwgemm", &packed_dwgemm_cuda);
  m.impl("packed_gemm_act", &packed_gemm_act_cuda);
  m.impl("packed_dwgemm_act", &packed_dwgemm_act_cuda);
  m.impl("fixed_quantize", &fixed_quantize_cuda);
  m.impl("act_encode", &act_encode_cuda);
  m.impl("act_decode", &act_decode_cuda);
  m.impl("packed_rowsums", &packed_rowsums_cuda);
  m.impl("packed_igemm", &packed_igemm_cuda);
  m.impl("packed_taps_i8", &packed_taps_i8_cuda);
  m.impl("packed_idwgemm", &packed_idwgemm_cuda);
  m.impl("quantize_channel", &quantize_channel_cuda);
  m.impl("cp_gram_mttkrp", &cp_gram_mttkrp_cuda);
  m.impl("cp_rel_error", &cp_rel_error_cuda);
}

TORCH_LIBRARY_IMPL(admmq, Meta, m) {
  m.impl("admm_iteration_batched", &admm_batched_meta);
  m.impl("quantize_batched", &quantize_batched_meta);
  m.impl("quantize_packed", &quantize_packed_meta);
  m.impl("dequantize_packed", &dequantize_packed_meta);
  m.impl("packed_gemm", &packed_gemm_meta);
  m.impl("packed_hgemm", &packed_hgemm_meta);
  m.impl("packed_lrgemm", &packed_lrgemm_meta);
  m.impl("packed_dwgemm", &packed_dwgemm_meta);
  m.impl("packed_gemm_act", &packed_gemm_act_meta);
  m.impl("packed_dwgemm_act", &packed_dwgemm_act_meta);
  m.impl("fixed_quantize", &fixed_quantize_meta);
  m.impl("act_encode", &act_encode_meta);
  m.impl("act_decode", &act_decode_meta);
  m.impl("packed_rowsums", &packed_rowsums_meta);
  m.impl("packed_igemm", &packed_igemm_meta);
  m.impl("packed_taps_i8", &packed_taps_i8_meta);
  m.impl("packed_idwgemm", &packed_idwgemm_meta);
  m.impl("quantize_channel", &quantize_channel_meta);
  m.impl("cp_gram_mttkrp", &cp_gram_mttkrp_meta);
  m.impl("cp_rel_error", &cp_rel_error_meta);
}
