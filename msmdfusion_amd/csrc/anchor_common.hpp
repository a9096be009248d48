// anchor_common.hpp -- what anchor.hip (Anchor3DHead, COVERAGE n3) and free_anchor.hip
// (FreeAnchor3DHead, n6) share: the nearest-BEV IoU as mmdet writes it, the staging of
// ground-truth boxes through LDS, the wave maximum behind the integer atomicMax, and the
// fixed-order second stage of the deterministic loss sums.  Both files must evaluate the IoU
// with the SAME function: their equality tests on IoU values rely on it.
#pragma once
#include "common.hpp"

namespace msmd {
namespace {

constexpr int kAnchorBlock = 256;        // anchors per workgroup: one lane each
constexpr int kAnchorGtChunk = 128;      // ground-truth boxes staged in LDS at a time

// mmdet bbox_overlaps(mode='iou', eps=1e-6) on (x1, y1, x2, y2), float32, as written:
// overlap / max(area1 + area2 - overlap, eps), wh = clamp(rb - lt, 0).
__device__ __forceinline__ float bev_iou(const float4 g, const float4 a) {
  const float area_g = (g.z - g.x) * (g.w - g.y);
  const float area_a = (a.z - a.x) * (a.w - a.y);
  const float w = fmaxf(fminf(g.z, a.z) - fmaxf(g.x, a.x), 0.f);
  const float h = fmaxf(fminf(g.w, a.w) - fmaxf(g.y, a.y), 0.f);
  const float overlap = w * h;
  const float uni = fmaxf(area_g + area_a - overlap, 1e-6f);
  return overlap / uni;
}

// bev_iou drops a NaN operand in fmaxf / fminf (they return the other one): a NaN box against a
// finite one gives a finite, meaningless number.  This form gives NaN when any coordinate of
// either box is NaN, as the same expression in torch does (torch.max / min / clamp propagate
// NaN), and bev_iou otherwise.
__device__ __forceinline__ bool box_has_nan(const float4 b) {
  return b.x != b.x || b.y != b.y || b.z != b.z || b.w != b.w;
}
__device__ __forceinline__ float bev_iou_nan(const float4 g, const float4 a) {
  return (box_has_nan(g) || box_has_nan(a)) ? __int_as_float(0x7fc00000) : bev_iou(g, a);
}

// The ground-truth list of segment s, clipped to the entries that exist.
__device__ __forceinline__ int gt_list(const int32_t* __restrict__ gt_offsets, int s, int entries,
                                       int& begin) {
  begin = gt_offsets[s];
  const int end = gt_offsets[s + 1];
  if (begin < 0 || begin > entries) return 0;
  const int n = min(end, entries) - begin;
  return n > 0 ? n : 0;
}

// Stage entries [c0, c0 + count) of the list into LDS; an index outside [0, num_gt) becomes a
// NaN box (what its IoU then is depends on the form: see bev_iou_nan).
__device__ __forceinline__ void stage_boxes(const float* __restrict__ gt_bev,
                                            const int32_t* __restrict__ gt_index, int num_gt,
                                            int first, int count, float4* boxes) {
  for (int j = threadIdx.x; j < count; j += kAnchorBlock) {
    const int g = gt_index ? gt_index[first + j] : first + j;
    float4 v;
    if ((unsigned)g < (unsigned)num_gt) {
      const float* p = gt_bev + (size_t)g * 4;
      v = make_float4(p[0], p[1], p[2], p[3]);
    } else {
      const float q = __int_as_float(0x7fc00000);
      v = make_float4(q, q, q, q);
    }
    boxes[j] = v;
  }
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, kWave));
  return v;
}

__device__ __forceinline__ float pow_gamma(float v, float gamma) {
  return gamma == 2.f ? v * v : powf(v, gamma);
}

// Sum of one double per lane over a workgroup of BLOCK lanes -> partial[blockIdx.x], in a
// fixed order (the first stage of a deterministic loss sum).
template <int BLOCK>
__device__ __forceinline__ void block_partial_sum(double loss, double* __restrict__ partial) {
  __shared__ double sh[BLOCK / kWave];
  for (int off = kWave / 2; off > 0; off >>= 1) loss += __shfl_down(loss, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = loss;
  __syncthreads();
  if (threadIdx.x == 0) {
    double l = 0;
    for (int k = 0; k < BLOCK / kWave; ++k) l += sh[k];
    partial[blockIdx.x] = l;
  }
}

// fixed-order sum of the block partials -> out[0]
__global__ __launch_bounds__(256) void partials_finish_kernel(
    const double* __restrict__ partial, int blocks, float* __restrict__ out) {
  __shared__ double sh[256];
  double l = 0;
  for (int b = threadIdx.x; b < blocks; b += 256) l += partial[b];
  sh[threadIdx.x] = l;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)sh[0];
}

}  // namespace
}  // namespace msmd
