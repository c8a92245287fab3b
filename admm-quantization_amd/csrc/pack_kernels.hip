// Packed integer codes of the tensor schemes (include/admmq.h, DESIGN.md "Packed codes"):
// the final pass of quantize_tensor that emits the codes as a little-endian bit stream
// (k_qfinal_pack, in place of k_qfinal), and its inverse (k_dequant_pack).
#include "../../include/admmq.h"
#include "quant_device.h"

namespace admmq {

// apply_quant's result y for x (the same quotient, rounding and clamp, operation for
// operation) together with the code of the level it chose; 0 where no code can be formed.
__device__ __forceinline__ float quant_code(float x, const QParams& p, unsigned& u, bool& formed) {
  const int q = 1 << (p.bits - 1);
  u = 0u;
  formed = false;
  if (p.scheme == kMse) {
    if (p.nan_all) return __builtin_nanf("");
    const float lv = nan_clamp(__builtin_rintf(x / p.scale), p.qlo, p.qhi);
    if (lv == lv) { u = (unsigned)((int)lv + q); formed = true; }
    return lv * p.scale;
  }
  if (p.scheme == kSymmetric) {
    const float lv = nan_clamp(__builtin_rintf(x / p.scale), p.qlo, p.qhi);
    if (lv == lv) { u = (unsigned)((int)lv + q); formed = true; }
    return (float)to_i64_x86(lv) * p.scale;
  }
  if (p.scheme == kAffine) {
    const float lv = nan_clamp(__builtin_rintf(x / p.scale) + (float)p.zp, p.qlo, p.qhi);
    if (lv == lv) { u = (unsigned)((int)lv + q); formed = true; }
    const long long li = to_i64_x86(lv);
    const long long d = (long long)((unsigned long long)li - (unsigned long long)(long long)p.zp);
    return (float)d * p.scale;
  }
  // kMinMax, bits >= 2 (the host rejects 1 bit)
  const float r = (x - p.mn) / p.rng;
  const float qi = __builtin_floorf(r * p.n + 0.5f);
  if (qi >= 0.f && qi <= p.n) { u = (unsigned)(int)qi; formed = true; }
  return (qi * p.rng) / p.n + p.mn;
}

constexpr int kPackRunStride = 9;   // LDS words per run of 32 codes (8 + 1 pad: the run reads hit distinct banks)

// Is the table's de-quantization of u IEEE-equal to y? minmax: u was formed from an
// in-range integer-valued qi, so (float)u == qi and the table's ((float)u * rng) / n + mn
// repeats y's own operations on the same values: equal unless y is NaN. (Evaluating it
// cost a third IEEE division per element: 31.1 against 27.0 us for a 4096 x 4096 tensor.)
// The other schemes evaluate the table.
__device__ __forceinline__ bool code_exact(unsigned u, bool formed, float y, const QParams& p) {
  if (!formed) return false;
  if (p.scheme == kMinMax) return y == y;
  return dequant_code(u, p.scheme, p.bits, p.scale, p.zp, p.mn, p.rng) == y;
}

// One unit = 1024 NG elements of the tensor's FLAT order (NG = 4: the stage-1 units, NG = 1:
// k_qfinal's, for launches that would otherwise leave CUs idle; either table's starts cover
// rows x ld >= rows x cols), read from the user's x - the bit stream has no row padding.
// Phase 1 (all 256 threads, coalesced): float4 group 4 (t + 256 k) of the unit -> y, its four
// codes (one byte each, one LDS word) and the bad count; with dst set, y is stored here.
// Phase 2 (threads < 32 NG): a thread owns one run of 32 consecutive elements: its 32
// code bytes -> BITS whole dwords (compile-time BITS: they stay in registers), stored as
// dwords; only the tensor's final partial run stores single bytes. Every output byte
// belongs to exactly one thread.
template <int BITS, int NG>
__global__ __launch_bounds__(256) void k_qfinal_pack(const QJob* __restrict__ jobs, const Chunk* __restrict__ chunks,
                                                     unsigned char* const* __restrict__ codes,
                                                     admmq_qmeta* __restrict__ meta, int ncand, int scheme) {
  const int job = chunks[blockIdx.x].job;
  const int start = chunks[blockIdx.x].start;
  const QJob& j = jobs[job];
  int idx = -1;
  const QParams qp = block_qparams(scheme, BITS, j.mv, 0, ncand, j.has_kw, j.tmin_kw, j.tmax_kw, &idx);
  const long long numel = (long long)j.rows * j.cols;
  if (start == 0 && threadIdx.x == 0) {   // (bad was zeroed before the launch; the blocks add to it)
    admmq_qmeta* m = meta + job;
    m->scheme = scheme; m->bits = BITS;
    m->scale = qp.scale; m->zero_point = qp.zp;
    m->mn = qp.mn; m->rng = qp.rng;
    m->index = idx;
  }
  if ((long long)start >= numel) return;   // a unit of the row pads only (block-uniform)
  constexpr int kRuns = 32 * NG;
  __shared__ unsigned lds[kRuns * kPackRunStride];
  __shared__ int red[4];
  const float* __restrict__ src = j.src;
  float* const dst = j.dst;
  const bool xvec = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  const bool yvec = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  float4 xv[NG];
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    const long long e = (long long)start + 4 * (int)threadIdx.x + 1024 * k;
    if (xvec && e + 4 <= numel) {
      xv[k] = gld4(src + e);
    } else {
      xv[k].x = e < numel ? src[e] : 0.f;
      xv[k].y = e + 1 < numel ? src[e + 1] : 0.f;
      xv[k].z = e + 2 < numel ? src[e + 2] : 0.f;
      xv[k].w = e + 3 < numel ? src[e + 3] : 0.f;
    }
  }
  int bad = 0;
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    const long long e = (long long)start + 4 * (int)threadIdx.x + 1024 * k;
    const float xs[4] = {xv[k].x, xv[k].y, xv[k].z, xv[k].w};
    float ys[4];
    unsigned word = 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      unsigned u;
      bool formed;
      ys[c] = quant_code(xs[c], qp, u, formed);
      if (e + c < numel) {
        if (code_exact(u, formed, ys[c], qp)) word |= u << (8 * c);
        else ++bad;   // (its code stays 0)
      }   // past the tensor: 0, so the spare bits of the stream's last byte are 0
    }
    const int qd = (int)threadIdx.x + 256 * k;   // quad of the unit: run qd / 8, word qd % 8
    lds[(qd >> 3) * kPackRunStride + (qd & 7)] = word;
    if (dst) {
      if (yvec && e + 4 <= numel) {
        *reinterpret_cast<float4*>(dst + e) = make_float4(ys[0], ys[1], ys[2], ys[3]);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (e + c < numel) dst[e + c] = ys[c];
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tot = (red[0] + red[1]) + (red[2] + red[3]);
    if (tot) atomicAdd(&meta[job].bad, tot);
  }
  if (threadIdx.x >= kRuns) return;
  const long long e0 = (long long)start + 32 * (int)threadIdx.x;
  const long long left = numel - e0;
  if (left <= 0) return;
  unsigned w8[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) w8[q] = lds[threadIdx.x * kPackRunStride + q];
  unsigned out[BITS];
  unsigned long long acc = 0ull;
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const unsigned u = (w8[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    const int pos = k * BITS;   // compile-time
    acc |= (unsigned long long)u << (pos & 31);
    if (((pos + BITS) >> 5) != (pos >> 5)) {
      out[pos >> 5] = (unsigned)acc;
      acc >>= 32;
    }
  }
  unsigned char* const cbase = codes[job] + (e0 >> 5) * (4 * BITS);   // dword-aligned (codes[i] is 16-byte aligned)
  if (left >= 32) {
    unsigned* const o = reinterpret_cast<unsigned*>(cbase);
    if constexpr (BITS % 4 == 0) {
#pragma unroll
      for (int w = 0; w < BITS; w += 4) *reinterpret_cast<uint4*>(o + w) = make_uint4(out[w], out[w + 1], out[w + 2], out[w + 3]);
    } else if constexpr (BITS % 2 == 0) {
#pragma unroll
      for (int w = 0; w < BITS; w += 2) *reinterpret_cast<uint2*>(o + w) = make_uint2(out[w], out[w + 1]);
    } else {
#pragma unroll
      for (int w = 0; w < BITS; ++w) o[w] = out[w];
    }
  } else {   // the tensor's final partial run: whole dwords, then single bytes
    const int nbytes = ((int)left * BITS + 7) >> 3;
#pragma unroll
    for (int w = 0; w < BITS; ++w) {
      if (4 * w + 4 <= nbytes) {
        reinterpret_cast<unsigned*>(cbase)[w] = out[w];
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (4 * w + b < nbytes) cbase[4 * w + b] = (unsigned char)(out[w] >> (8 * b));
      }
    }
  }
}

// Block = kDqBlockElems flat elements of one tensor; a thread takes the float4 groups
// 4 t + 1024 g of it (coalesced stores): the 4 bits-wide codes of a group lie in one or
// two dwords of the stream.
__global__ __launch_bounds__(256) void k_dequant_pack(const DqBatch b, const admmq_qmeta* __restrict__ meta) {
  int jb = 0;
  while (jb + 1 < b.njobs && (int)blockIdx.x >= b.blk0[jb + 1]) ++jb;
  const admmq_qmeta m = meta[b.meta0 + jb];
  if (m.bits < 1 || m.bits > 8 || m.scheme < kMse || m.scheme > kAffine) return;   // not a meta record
  const long long numel = b.numel[jb];
  const long long nbytes = (numel * m.bits + 7) >> 3;
  const unsigned char* __restrict__ c = b.codes[jb];
  float* const y = b.y[jb];
  const bool vec = (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  const unsigned mask = (1u << m.bits) - 1u;
  const long long base = (long long)((int)blockIdx.x - b.blk0[jb]) * kDqBlockElems;
#pragma unroll
  for (int g = 0; g < kDqBlockElems / 1024; ++g) {
    const long long e = base + 4LL * threadIdx.x + 1024LL * g;
    if (e >= numel) break;
    const long long bit = e * m.bits;
    const long long w = bit >> 5;
    const int sh = (int)(bit & 31);
    unsigned long long win = code_dword(c, w, nbytes);
    if (sh + 4 * m.bits > 32) win |= (unsigned long long)code_dword(c, w + 1, nbytes) << 32;
    win >>= sh;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      v[k] = dequant_code((unsigned)(win >> (k * m.bits)) & mask, m.scheme, m.bits, m.scale, m.zero_point, m.mn, m.rng);
    if (vec && e + 4 <= numel) {
      *reinterpret_cast<float4*>(y + e) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < numel) y[e + k] = v[k];
    }
  }
}

void launch_qfinal_pack(const QJob* jobs, const Chunk* chunks, int nchunks, int ng, unsigned char* const* codes,
                        admmq_qmeta* meta, int ncand, int bits, int qscheme, hipStream_t s) {
  if (nchunks <= 0) return;
#define ADMMQ_PACK_CASE(B)                                                                                        \
  case B:                                                                                                         \
    if (ng == 4)                                                                                                  \
      hipLaunchKernelGGL((k_qfinal_pack<B, 4>), dim3(nchunks), dim3(256), 0, s, jobs, chunks, codes, meta, ncand, \
                         qscheme);                                                                                \
    else                                                                                                          \
      hipLaunchKernelGGL((k_qfinal_pack<B, 1>), dim3(nchunks), dim3(256), 0, s, jobs, chunks, codes, meta, ncand, \
                         qscheme);                                                                                \
    break;
  switch (bits) {
    ADMMQ_PACK_CASE(1) ADMMQ_PACK_CASE(2) ADMMQ_PACK_CASE(3) ADMMQ_PACK_CASE(4)
    ADMMQ_PACK_CASE(5) ADMMQ_PACK_CASE(6) ADMMQ_PACK_CASE(7) ADMMQ_PACK_CASE(8)
    default: break;   // (the entry point admits 1..8 only)
  }
#undef ADMMQ_PACK_CASE
}

void launch_dequant_pack(const DqBatch& b, int nblocks, const admmq_qmeta* meta, hipStream_t s) {
  if (nblocks > 0) hipLaunchKernelGGL(k_dequant_pack, dim3(nblocks), dim3(256), 0, s, b, meta);
}

}  // namespace admmq
