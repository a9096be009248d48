// tiling_key.hpp -- the 32-bit sort key a table row gets in the tiling order (plan.hip:
// keys_many_kernel; the reasoning sits at spconv.hip: row_mask_kernel).
#pragma once
#include "common.hpp"

namespace msmd {

// 3x3x3: bit position of offset k in the key = its rank under (|dz|+|dy|+|dx|, |dz|, |dy|):
// the centre lowest, then the 6 face neighbours, the 12 edge ones, the 8 corners highest.
static __constant__ unsigned char kRank27[27] = {19, 15, 20, 11, 5,  12, 21, 16, 22, 7,  3,  8,  1, 0,
                                                 2,  9,  4,  10, 23, 17, 24, 13, 6,  14, 25, 18, 26};

// Significant bits of the key of a K-offset table (the radix sort's end bit).
inline int row_key_bits(int kvol) { return kvol == 27 ? 27 : (kvol <= 15 ? 2 * kvol + 1 : 32); }

// K < 16: (K - popcount) << K | mask; 27: the ranked mask; 16..31 otherwise: the mask.
__device__ __forceinline__ uint32_t row_key32(const int32_t* __restrict__ nbr, int kvol, size_t ld,
                                              int o) {
  unsigned v = 0, ranked = 0;
  for (int k = 0; k < kvol; ++k)
    if (nbr[(size_t)k * ld + o] >= 0) {
      v |= 1u << k;
      if (kvol == 27) ranked |= 1u << kRank27[k];
    }
  return kvol == 27 ? ranked : (kvol <= 15 ? ((unsigned)(kvol - __popc(v)) << kvol) | v : v);
}

}  // namespace msmd
