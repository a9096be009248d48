// fps_order.hpp -- the tie order of the reference's furthest-point-sampling block reduction
// (furthest_point_sample_cuda.cu:17-23,55-137 and :214-330), shared by the coordinate form
// (points.hip) and the distance-matrix form (pointnet.hip).
//
// The reference runs bs = opt_n_threads(n) threads (largest power of two <= n, at most 1024);
// thread t scans points k = t, t + bs, ... and keeps its FIRST maximum; the shared-memory tree
// then keeps the LOWER slot of each (t, t + s) pair, s = bs/2 .. 1, unless the upper one is
// strictly greater.  Between two thread ids the one whose lowest differing bit is 0 therefore
// wins: among equal distances the point with the smallest
//   rank(k) = (bitrev(k mod bs) << 21) | (k div bs)
// is selected (n < 2^21).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msmd {

// log2 of the reference block size for n points (n >= 1)
__device__ __forceinline__ int fps_block_shift(int n) {
  const int s = 31 - __clz(n);
  return s < 10 ? s : 10;
}
__device__ __forceinline__ uint32_t fps_tie_rank(int k, int bs_shift) {
  const uint32_t rev =
      bs_shift ? (__brev((uint32_t)(k & ((1 << bs_shift) - 1))) >> (32 - bs_shift)) : 0u;
  return (rev << 21) | (uint32_t)(k >> bs_shift);
}
// inverse of fps_tie_rank
__device__ __forceinline__ int fps_rank_index(uint32_t rank, int bs_shift) {
  const uint32_t tid_ref = bs_shift ? (__brev(rank >> 21) >> (32 - bs_shift)) : 0u;
  return (int)((rank & 0x1FFFFFu) << bs_shift) | (int)tid_ref;
}

}  // namespace msmd
