// chamfer_common.hpp -- the Chamfer criterion and torch.min's selection rule, shared by
// vote.hip (chamfer_min_*) and h3d.hip (the cue-target kernel): one definition, so a nearest
// neighbour found inside a fused kernel is the one msmd_chamfer_fwd_f32 finds, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace msmd {

enum { kL2 = 0, kL1 = 1, kSmoothL1 = 2 };

// per coordinate on d = q - r, float32, one rounding per operation
template <int MODE>
__device__ __forceinline__ float criterion(float q, float r) {
  const float d = __fsub_rn(q, r);
  if (MODE == kL2) return __fmul_rn(d, d);
  const float z = fabsf(d);
  if (MODE == kL1) return z;
  return z < 1.f ? __fmul_rn(__fmul_rn(0.5f, z), z) : __fsub_rn(z, 0.5f);
}

// (cx + cy) + cz
template <int MODE>
__device__ __forceinline__ float distance(const float* q, const float* r) {
  return __fadd_rn(__fadd_rn(criterion<MODE>(q[0], r[0]), criterion<MODE>(q[1], r[1])),
                   criterion<MODE>(q[2], r[2]));
}

// torch.min: strictly smaller replaces; the first NaN replaces anything that is not NaN
__device__ __forceinline__ void take_min(float d, int j, float& best, int& at) {
  if (d < best || (d != d && best == best)) {
    best = d;
    at = j;
  }
}

}  // namespace msmd
