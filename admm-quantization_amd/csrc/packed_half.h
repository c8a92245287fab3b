// What the 16-bit MFMA packed-layer kernels share: the K step and the LDS
// row stride, the argument record, the integer operand's bits, the MFMA of either type, the
// float32 epilogue and its store. k_packed_hgemm / k_packed_hreduce are in packed_hgemm.hip,
// k_packed_hdwgemm in packed_hdwgemm.hip. The host pieces below the kernels' are defined in
// packed_hgemm.hip.
#pragma once
#include <type_traits>

#include "../../include/admmq.h"
#include "packed_tile.h"

namespace admmq {

constexpr int kHgBK = 32;                // the K step
constexpr int kHgLD = 40;                // LDS row stride in 16-bit elements: 16-byte aligned rows, 20 dwords apart
constexpr int64_t kHgKMax = int64_t(1) << 24;

typedef float hg_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 hg_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 hg_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned hg_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const unsigned short gcu16;
typedef __attribute__((address_space(1))) const hg_u32x4 gcu32x4;

struct HgArgs {
  const unsigned char* codes;
  const unsigned short* x;   // bf16 / fp16 bits
  const float* bias;
  void* y;
  float* part;        // parallel form: [np][total] float32 partial images in Y's layout
  float* xpart;       // parallel form, tensor_minmax: [np][C] partial column sums of x
  long long nbytes;   // bytes of the code stream
  long long total;    // C * M
  long long C;
  int M, K, N;
  int xl;
  int kp, np, parallel;
  int scheme;
  int off;            // the operand is u - off (q + zp; 0 for tensor_minmax)
  int xal;            // x_layout 1: every row of x starts on a 16-byte boundary
  int ydt;            // ADMMQ_DT_* of y
  float scale, mn, rng, nlev;   // nlev = float(2^bits - 1)
};

// The float32 result of one output: the sums' epilogue, operations rounded one by one
__device__ __forceinline__ float hg_value(float S, float Sx, const HgArgs& a, bool has_bias, float bv) {
  float v;
  if (a.scheme == kMinMax) v = (S * a.rng) / a.nlev + a.mn * Sx;
  else v = S * a.scale;
  return has_bias ? v + bv : v;
}

// y[e] = v as float32, or rounded to nearest even to bf16 / fp16
__device__ __forceinline__ void hg_store(void* y, long long e, float v, int ydt) {
  if (ydt == ADMMQ_DT_F32) static_cast<float*>(y)[e] = v;
  else if (ydt == ADMMQ_DT_BF16) static_cast<__bf16*>(y)[e] = static_cast<__bf16>(v);
  else static_cast<_Float16*>(y)[e] = static_cast<_Float16>(v);
}

// The 16 bits of the integer v (|v| <= 256 for bf16, <= 2048 for fp16: exact)
template <typename T>
__device__ __forceinline__ unsigned hg_int_bits(int v) {
  if constexpr (std::is_same_v<T, __bf16>) return __builtin_bit_cast(unsigned, (float)v) >> 16;
  else return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)(float)v);
}

template <typename T>
__device__ __forceinline__ hg_f32x16 hg_mfma(const hg_u32x4 a, const hg_u32x4 b, const hg_f32x16 c) {
  if constexpr (std::is_same_v<T, __bf16>)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(hg_bf16x8, a), __builtin_bit_cast(hg_bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(hg_f16x8, a), __builtin_bit_cast(hg_f16x8, b), c, 0, 0, 0);
}

// --- host pieces (packed_hgemm.hip) -----------------------------------------------------------------

// The half path's plan: plan_packed with a K step of 32 and float32 partial images; tensor_minmax adds
// the partial column sums of x in the parallel regime
bool plan_hg(const ::admmq_qmeta* meta, int64_t M, int64_t K, int64_t N, int64_t nb, PackedPlan& pl);
// The dtype pair and the record's exactness in the activations' type (xn: their argument's name in the messages)
int hg_dtype_check(const char* who, const char* xn, const ::admmq_qmeta* meta, int32_t x_dtype, int32_t y_dtype);
// The alignment of codes, the activations (xn), y and bias
int hg_align_check(const char* who, const char* xn, const void* codes, const void* x, const void* y, int32_t y_dtype,
                   const float* bias);
// The record of a checked call (x_layout 0 or 1)
void hg_fill(HgArgs& a, const uint8_t* codes, const ::admmq_qmeta* meta, const void* x, const float* bias, void* y,
             int32_t y_dtype, void* workspace, const PackedPlan& pl, int64_t M, int64_t K, int64_t N, int32_t x_layout);
// k_packed_hreduce in the parallel regime, then the launches' status
int32_t hg_finish(const HgArgs& a, const PackedPlan& pl, void* stream);

}  // namespace admmq
