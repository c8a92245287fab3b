// What the four packed-layer GEMM kernels and their host sides have in common by value
// (DESIGN.md 2.27): the 64 x 64 tile, the K-piece rule's constants, the accumulator map of the
// 32 x 32 MFMAs and the dispatch on a weight record's bits. k_packed_gemm / k_packed_dwgemm are
// in packed_gemm.hip (fp32 MFMA, K step 32), k_packed_igemm / k_packed_idwgemm in packed_igemm.hip
// (int8 MFMA, K step 64).
#pragma once
#include "quant_device.h"

namespace admmq {

constexpr int kPackedBM = 64, kPackedBN = 64;   // the tile
constexpr int kPackedPieceMin = 64;             // K per piece at least
constexpr int kPackedPiecesMax = 32;            // pieces at most
constexpr int kPackedParallelBelow = 256;       // tiles below which the pieces run in parallel (one workgroup per CU at least)

typedef __attribute__((address_space(1))) const unsigned gcu32;   // (gcf32: admmq_internal.h)

// One launch expression per bits value of a weight record (bits outside 1..8 are refused before)
#define PACKED_BITS_SWITCH(bits, LAUNCH)                                             \
  switch (bits) {                                                                    \
    case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break;    \
    case 4: LAUNCH(4); break; case 5: LAUNCH(5); break; case 6: LAUNCH(6); break;    \
    case 7: LAUNCH(7); break; case 8: LAUNCH(8); break;                              \
    default: break;                                                                  \
  }

// C/D map of the 32 x 32 MFMAs: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
// (h = lane >> 5 in the caller's scope)
#define PACKED_ROW(r) (((r) & 3) + 8 * ((r) >> 2) + 4 * h)

}  // namespace admmq
