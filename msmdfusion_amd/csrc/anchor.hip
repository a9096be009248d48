// anchor.hip -- target assignment and classification loss of Anchor3DHead (COVERAGE n3).
//
//   anchor_gt_max_kernel   pass one of MaxIoUAssigner.assign_wrt_overlaps (mmdet 2.x
//   anchor_assign_kernel   core/bbox/assigners/max_iou_assigner.py) over the nearest-BEV IoU of
//                          BboxOverlapsNearest3D (mmdet3d/core/bbox/iou_calculators/
//                          iou3d_calculator.py:94-150 -> mmdet bbox_overlaps): the reference
//                          builds a [num_gt, num_anchors] matrix per sample and per assigner,
//                          reduces it along both axes and walks the ground truths in a Python
//                          loop.  Here the matrix is never formed: one lane per anchor, the
//                          segment's ground-truth boxes staged through LDS in chunks.
//   anchor_targets_kernel  the rest of AnchorTrainMixin.anchor_target_single_assigner
//                          (mmdet3d/models/dense_heads/train_mixins.py:237-314):
//                          DeltaXYZWLHRBBoxCoder.encode, get_direction_target (:317-346), labels
//                          and the four weight tensors, written in the interleaved order of
//                          anchor_target_3d_single (:125-182).
//   sigmoid_focal_kernel   mmdet FocalLoss(use_sigmoid=True) as Anchor3DHead.loss_single calls it
//                          (anchor3d_head.py:217-218).
//
// A segment is one (sample, assigner group): a run of anchors and a list of ground truths.  The
// anchors' side of the segmentation is known to the host (it follows from the feature-map
// sizes) and travels by value in the kernel arguments; the ground truths' side (which depends
// on the labels under assign_per_class) stays on the device.  Nothing is read back.
//
// The per-ground-truth maximum over a segment's anchors is an integer atomicMax on the bits of
// the non-negative IoU (as pool.hip does): independent of the order of arrival, so the result
// is bitwise reproducible.  Both passes evaluate the IoU with the same function, which is what
// the equality test of rule 4 (gt_max_assign_all) relies on.
#include "anchor_common.hpp"

namespace msmd {
namespace {

constexpr int kAnchorMaxSegments = 64;   // segments per call (the table is a kernel argument)

struct AnchorSegments {
  int n;
  int offsets[kAnchorMaxSegments + 1];   // output rows of segment s: offsets[s] .. offsets[s+1]
  float pos_iou_thr[kAnchorMaxSegments];
  float neg_iou_thr[kAnchorMaxSegments];
  float min_pos_iou[kAnchorMaxSegments];
};

// Workgroup b -> (segment, first output row).  Uniform: every lane walks the same table.
__device__ __forceinline__ bool locate(const AnchorSegments& sg, int& seg, int& row0) {
  int b = blockIdx.x;
  for (int s = 0; s < sg.n; ++s) {
    const int len = sg.offsets[s + 1] - sg.offsets[s];
    const int nb = (len + kAnchorBlock - 1) / kAnchorBlock;
    if (b < nb) {
      seg = s;
      row0 = sg.offsets[s] + b * kAnchorBlock;
      return true;
    }
    b -= nb;
  }
  return false;
}

// Pass one: gt_max_bits[entry] = max over the segment's anchors of the IoU's bit pattern.
__global__ __launch_bounds__(kAnchorBlock) void anchor_gt_max_kernel(
    const AnchorSegments sg, const float* __restrict__ anchor_bev, int anchor_rows,
    const float* __restrict__ gt_bev, int num_gt, const int32_t* __restrict__ gt_index,
    const int32_t* __restrict__ gt_offsets, int entries, uint32_t* __restrict__ gt_max_bits) {
  __shared__ float4 boxes[kAnchorGtChunk];
  int seg, row0;
  if (!locate(sg, seg, row0)) return;
  int gbegin;
  const int ng = gt_list(gt_offsets, seg, entries, gbegin);
  if (ng == 0) return;
  const int row = row0 + threadIdx.x;
  const bool live = row < sg.offsets[seg + 1];
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float* p = anchor_bev + (size_t)(row % anchor_rows) * 4;
    a = make_float4(p[0], p[1], p[2], p[3]);
  }
  const int lane = threadIdx.x & (kWave - 1);
  for (int c0 = 0; c0 < ng; c0 += kAnchorGtChunk) {
    const int count = min(ng - c0, kAnchorGtChunk);
    __syncthreads();
    stage_boxes(gt_bev, gt_index, num_gt, gbegin + c0, count, boxes);
    __syncthreads();
    for (int j = 0; j < count; ++j) {
      const float iou = live ? bev_iou(boxes[j], a) : 0.f;
      // NaN and (impossible) negative values stay out of the integer order
      const uint32_t bits = iou > 0.f ? __float_as_uint(iou) : 0u;
      if (__ballot(bits != 0u) == 0ull) continue;      // uniform over the wave
      const uint32_t m = wave_max_u32(bits);
      if (lane == 0) atomicMax(&gt_max_bits[gbegin + c0 + j], m);
    }
  }
}

// Pass two: rules 1-4 per anchor, the IoU recomputed against the staged boxes.
__global__ __launch_bounds__(kAnchorBlock) void anchor_assign_kernel(
    const AnchorSegments sg, const float* __restrict__ anchor_bev, int anchor_rows,
    const float* __restrict__ gt_bev, int num_gt, const int32_t* __restrict__ gt_index,
    const int32_t* __restrict__ gt_offsets, int entries,
    const uint32_t* __restrict__ gt_max_bits, int32_t* __restrict__ assigned_gt,
    float* __restrict__ max_overlaps, int32_t* __restrict__ num_pos) {
  __shared__ float4 boxes[kAnchorGtChunk];
  __shared__ float gmax[kAnchorGtChunk];
  int seg, row0;
  if (!locate(sg, seg, row0)) return;
  int gbegin;
  const int ng = gt_list(gt_offsets, seg, entries, gbegin);
  const int row = row0 + threadIdx.x;
  const bool live = row < sg.offsets[seg + 1];
  if (ng == 0) {                      // train_mixins.py:278-284: every anchor is a negative
    if (live) {
      assigned_gt[row] = 0;
      max_overlaps[row] = 0.f;
    }
    return;
  }
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float* p = anchor_bev + (size_t)(row % anchor_rows) * 4;
    a = make_float4(p[0], p[1], p[2], p[3]);
  }
  const float pos_thr = sg.pos_iou_thr[seg], neg_thr = sg.neg_iou_thr[seg];
  const float min_pos = sg.min_pos_iou[seg];
  float best = -1.f;
  int arg = -1, low = -1;             // low: the last ground truth that claims this anchor (rule 4)
  for (int c0 = 0; c0 < ng; c0 += kAnchorGtChunk) {
    const int count = min(ng - c0, kAnchorGtChunk);
    __syncthreads();
    stage_boxes(gt_bev, gt_index, num_gt, gbegin + c0, count, boxes);
    for (int j = threadIdx.x; j < count; j += kAnchorBlock)
      gmax[j] = __uint_as_float(gt_max_bits[gbegin + c0 + j]);
    __syncthreads();
    if (!live) continue;
    for (int j = 0; j < count; ++j) {
      const float iou = bev_iou(boxes[j], a);
      if (iou > best) {               // strict: ties go to the lowest index
        best = iou;
        arg = c0 + j;
      }
      const float gm = gmax[j];
      if (gm >= min_pos && iou == gm) low = c0 + j;
    }
  }
  int result = -1;                                        // rule 1
  if (live) {
    if (best >= 0.f && best < neg_thr) result = 0;        // rule 2
    if (best >= pos_thr) result = arg + 1;                // rule 3
    if (low >= 0) result = low + 1;                       // rule 4
    assigned_gt[row] = result;
    max_overlaps[row] = best;
  }
  const int in_wave = __popcll(__ballot(live && result > 0));
  if ((threadIdx.x & (kWave - 1)) == 0 && in_wave) atomicAdd(&num_pos[seg], in_wave);
}

// One lane per anchor of a segment: everything anchor_target_single_assigner writes.
__global__ __launch_bounds__(kAnchorBlock) void anchor_targets_kernel(
    const AnchorSegments sg, const int32_t* __restrict__ assigned_gt,
    const float* __restrict__ anchors, int anchor_rows, int code,
    const float* __restrict__ gt_boxes, const int64_t* __restrict__ gt_labels, int num_gt,
    const int32_t* __restrict__ gt_index, const int32_t* __restrict__ gt_offsets, int entries,
    const int32_t* __restrict__ dest, int num_classes, float pos_weight, float dir_offset,
    int64_t* __restrict__ labels, float* __restrict__ label_weights,
    float* __restrict__ bbox_targets, float* __restrict__ bbox_weights,
    int64_t* __restrict__ dir_targets, float* __restrict__ dir_weights) {
  int seg, row0;
  if (!locate(sg, seg, row0)) return;
  const int row = row0 + threadIdx.x;
  if (row >= sg.offsets[seg + 1]) return;
  const int local = row % anchor_rows;
  int out = row;
  if (dest) {
    const int d = dest[local];
    if ((unsigned)d >= (unsigned)anchor_rows) return;
    out = row - local + d;
  }
  int gbegin;
  const int ng = gt_list(gt_offsets, seg, entries, gbegin);
  const int assigned = assigned_gt[row];
  int g = -1;
  if (assigned > 0 && assigned <= ng) {
    g = gt_index ? gt_index[gbegin + assigned - 1] : gbegin + assigned - 1;
    if ((unsigned)g >= (unsigned)num_gt) g = -1;
  }
  float* bt = bbox_targets + (size_t)out * code;
  float* bw = bbox_weights + (size_t)out * code;
  if (g < 0) {
    labels[out] = num_classes;
    label_weights[out] = assigned == 0 ? 1.f : 0.f;
    dir_targets[out] = 0;
    dir_weights[out] = 0.f;
    for (int k = 0; k < code; ++k) {
      bt[k] = 0.f;
      bw[k] = 0.f;
    }
    return;
  }
  const float* an = anchors + (size_t)local * code;
  const float* gt = gt_boxes + (size_t)g * code;
  // DeltaXYZWLHRBBoxCoder.encode (delta_xyzwhlr_bbox_coder.py:20-54), float32 as written
  const float xa = an[0], ya = an[1], wa = an[3], la = an[4], ha = an[5], ra = an[6];
  const float xg = gt[0], yg = gt[1], wg = gt[3], lg = gt[4], hg = gt[5], rg = gt[6];
  const float za = an[2] + ha / 2.f, zg = gt[2] + hg / 2.f;
  const float diagonal = sqrtf(la * la + wa * wa);
  const float rt = rg - ra;
  bt[0] = (xg - xa) / diagonal;
  bt[1] = (yg - ya) / diagonal;
  bt[2] = (zg - za) / ha;
  bt[3] = logf(wg / wa);
  bt[4] = logf(lg / la);
  bt[5] = logf(hg / ha);
  bt[6] = rt;
  for (int k = 7; k < code; ++k) bt[k] = gt[k] - an[k];
  for (int k = 0; k < code; ++k) bw[k] = 1.f;
  // get_direction_target (train_mixins.py:334-337): limit_period(rot_gt - dir_offset, 0, 2 pi),
  // two bins
  const float two_pi = 6.283185307179586f, pi = 3.141592653589793f;
  const float val = (rt + ra) - dir_offset;
  const float offset_rot = val - floorf(val / two_pi + 0.f) * two_pi;
  long bin = (long)floorf(offset_rot / pi);
  bin = bin < 0 ? 0 : (bin > 1 ? 1 : bin);
  dir_targets[out] = bin;
  dir_weights[out] = 1.f;
  labels[out] = gt_labels[g];
  label_weights[out] = pos_weight > 0.f ? pos_weight : 1.f;
}

constexpr int kSigFocalBlock = 256;
constexpr int kSigFocalPerThread = 8;

// loss_ic = BCE_with_logits(x, t) * (alpha t + (1 - alpha)(1 - t)) * pt^gamma * weight_i,
// t = [label_i == c], pt = (1 - p) t + p (1 - t), p = sigmoid(x).  Both probabilities are taken
// from their own exponential, so neither cancels at large |x|.
__global__ __launch_bounds__(kSigFocalBlock) void sigmoid_focal_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ labels,
    const float* __restrict__ weights, long n, int c, float gamma, float alpha,
    float* __restrict__ grad, double* __restrict__ partial) {
  double loss = 0;
  const long total = n * c;
  const long base = (long)blockIdx.x * kSigFocalBlock * kSigFocalPerThread;
#pragma unroll
  for (int u = 0; u < kSigFocalPerThread; ++u) {
    const long i = base + (long)u * kSigFocalBlock + threadIdx.x;
    if (i >= total) continue;
    const long r = i / c;
    const int ch = (int)(i - r * c);
    const float xi = x[i], w = weights[r];
    const bool t = labels[r] == (int64_t)ch;
    const float z = t ? xi : -xi;                 // the loss of a negative is that of -x
    const float e = expf(-fabsf(z));
    const float sp = fmaxf(-z, 0.f) + log1pf(e);  // softplus(-z) = -log sigmoid(z)
    const float p = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);   // sigmoid(z)
    const float q = z >= 0.f ? e / (1.f + e) : 1.f / (1.f + e);   // 1 - sigmoid(z)
    const float a = t ? alpha : 1.f - alpha;
    const float u_ = pow_gamma(q, gamma);
    loss += (double)(a * u_ * sp * w);
    if (grad) {
      // d/dz [q^gamma softplus(-z)] = q^gamma (-gamma p softplus(-z) - q)
      const float dz = a * u_ * (-gamma * p * sp - q) * w;
      grad[i] = t ? dz : -dz;
    }
  }
  block_partial_sum<kSigFocalBlock>(loss, partial);
}

// The host's half of the segmentation: ascending offsets from 0, at most kAnchorMaxSegments.
// -> number of workgroups, or -1.
int fill_segments(const int32_t* anchor_offsets, int num_segments, AnchorSegments& sg) {
  if (!anchor_offsets || num_segments < 1 || num_segments > kAnchorMaxSegments) return -1;
  if (anchor_offsets[0] != 0) return -1;
  long blocks = 0;
  sg.n = num_segments;
  sg.offsets[0] = 0;
  for (int s = 0; s < num_segments; ++s) {
    if (anchor_offsets[s + 1] < anchor_offsets[s]) return -1;
    sg.offsets[s + 1] = anchor_offsets[s + 1];
    blocks += ceil_div((long)anchor_offsets[s + 1] - anchor_offsets[s], kAnchorBlock);
  }
  return (int)blocks;
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_anchor_max_segments(void) { return kAnchorMaxSegments; }
MSMD_EXPORT int msmd_anchor_gt_chunk(void) { return kAnchorGtChunk; }

MSMD_EXPORT size_t msmd_anchor_assign_workspace_bytes(int gt_entries) {
  if (gt_entries < 0) return 0;
  return align_up((size_t)(gt_entries > 0 ? gt_entries : 1) * sizeof(uint32_t));
}

MSMD_EXPORT int msmd_anchor_assign_f32(const float* anchor_bev, int anchor_rows,
                                       const int32_t* anchor_offsets, int num_segments,
                                       const float* gt_bev, int num_gt, const int32_t* gt_index,
                                       const int32_t* gt_offsets, int gt_entries,
                                       const float* pos_iou_thr, const float* neg_iou_thr,
                                       const float* min_pos_iou, int32_t* assigned_gt,
                                       float* max_overlaps, int32_t* num_pos, void* workspace,
                                       size_t workspace_bytes, msmd_stream_t stream) {
  if (anchor_rows < 0 || num_segments < 0 || num_gt < 0 || gt_entries < 0)
    return MSMD_ERR_INVALID_ARG;
  if (num_segments == 0) return MSMD_OK;
  if (num_segments > kAnchorMaxSegments) return MSMD_ERR_RANGE;
  if (!pos_iou_thr || !neg_iou_thr || !min_pos_iou) return MSMD_ERR_INVALID_ARG;
  AnchorSegments sg;
  const int blocks = fill_segments(anchor_offsets, num_segments, sg);
  if (blocks < 0) return MSMD_ERR_INVALID_ARG;
  const int total = sg.offsets[num_segments];
  if (!gt_offsets || !num_pos) return MSMD_ERR_INVALID_ARG;
  if (total > 0 && (!anchor_bev || anchor_rows < 1 || !assigned_gt || !max_overlaps))
    return MSMD_ERR_INVALID_ARG;
  if (gt_entries > 0 && (!gt_bev || num_gt < 1)) return MSMD_ERR_INVALID_ARG;
  if (!gt_index && gt_entries > num_gt) return MSMD_ERR_INVALID_ARG;
  if (!workspace || ((uintptr_t)workspace & 3) ||
      workspace_bytes < msmd_anchor_assign_workspace_bytes(gt_entries))
    return MSMD_ERR_WORKSPACE;
  for (int s = 0; s < num_segments; ++s) {
    sg.pos_iou_thr[s] = pos_iou_thr[s];
    sg.neg_iou_thr[s] = neg_iou_thr[s];
    sg.min_pos_iou[s] = min_pos_iou[s];
  }
  hipStream_t st = (hipStream_t)stream;
  uint32_t* gt_max = (uint32_t*)workspace;
  if (hipMemsetAsync(num_pos, 0, sizeof(int32_t) * (size_t)num_segments, st) != hipSuccess)
    return MSMD_ERR_LAUNCH;
  if (blocks == 0) return launch_status();
  if (gt_entries > 0) {
    if (hipMemsetAsync(gt_max, 0, sizeof(uint32_t) * (size_t)gt_entries, st) != hipSuccess)
      return MSMD_ERR_LAUNCH;
    MSMD_LAUNCH(anchor_gt_max_kernel, dim3(blocks), dim3(kAnchorBlock), 0, st, sg, anchor_bev,
                anchor_rows, gt_bev, num_gt, gt_index, gt_offsets, gt_entries, gt_max);
  }
  MSMD_LAUNCH(anchor_assign_kernel, dim3(blocks), dim3(kAnchorBlock), 0, st, sg, anchor_bev,
              anchor_rows, gt_bev, num_gt, gt_index, gt_offsets, gt_entries, gt_max, assigned_gt,
              max_overlaps, num_pos);
  return launch_status();
}

MSMD_EXPORT int msmd_anchor_targets_f32(const int32_t* assigned_gt, const float* anchors,
                                        int anchor_rows, int code_size,
                                        const int32_t* anchor_offsets, int num_segments,
                                        const float* gt_boxes, const int64_t* gt_labels,
                                        int num_gt, const int32_t* gt_index,
                                        const int32_t* gt_offsets, int gt_entries,
                                        const int32_t* dest, int num_classes, float pos_weight,
                                        float dir_offset, int64_t* labels, float* label_weights,
                                        float* bbox_targets, float* bbox_weights,
                                        int64_t* dir_targets, float* dir_weights,
                                        msmd_stream_t stream) {
  if (anchor_rows < 0 || num_segments < 0 || num_gt < 0 || gt_entries < 0 || num_classes < 0)
    return MSMD_ERR_INVALID_ARG;
  if (code_size < 7 || code_size > 16) return MSMD_ERR_UNSUPPORTED;
  if (num_segments == 0) return MSMD_OK;
  if (num_segments > kAnchorMaxSegments) return MSMD_ERR_RANGE;
  AnchorSegments sg;
  const int blocks = fill_segments(anchor_offsets, num_segments, sg);
  if (blocks < 0) return MSMD_ERR_INVALID_ARG;
  const int total = sg.offsets[num_segments];
  if (blocks == 0) return MSMD_OK;
  if (!assigned_gt || !anchors || anchor_rows < 1 || !gt_offsets || !labels || !label_weights ||
      !bbox_targets || !bbox_weights || !dir_targets || !dir_weights)
    return MSMD_ERR_INVALID_ARG;
  if (gt_entries > 0 && (!gt_boxes || !gt_labels || num_gt < 1)) return MSMD_ERR_INVALID_ARG;
  if (!gt_index && gt_entries > num_gt) return MSMD_ERR_INVALID_ARG;
  // a permutation of the rows of one sample: the output is whole samples
  if (dest && total % anchor_rows != 0) return MSMD_ERR_INVALID_ARG;
  for (int s = 0; s < num_segments; ++s)
    sg.pos_iou_thr[s] = sg.neg_iou_thr[s] = sg.min_pos_iou[s] = 0.f;
  MSMD_LAUNCH(anchor_targets_kernel, dim3(blocks), dim3(kAnchorBlock), 0, (hipStream_t)stream, sg,
              assigned_gt, anchors, anchor_rows, code_size, gt_boxes, gt_labels, num_gt, gt_index,
              gt_offsets, gt_entries, dest, num_classes, pos_weight, dir_offset, labels,
              label_weights, bbox_targets, bbox_weights, dir_targets, dir_weights);
  return launch_status();
}

MSMD_EXPORT size_t msmd_sigmoid_focal_workspace_bytes(int64_t n, int num_classes) {
  if (n < 0 || num_classes < 1) return 0;
  const long per = (long)kSigFocalBlock * kSigFocalPerThread;
  const long blocks = (n * num_classes + per - 1) / per;
  return align_up((size_t)(blocks > 0 ? blocks : 1) * sizeof(double));
}

MSMD_EXPORT int msmd_sigmoid_focal_f32(const float* logits, const int64_t* labels,
                                       const float* weights, int64_t n, int num_classes,
                                       float gamma, float alpha, float* grad, float* sum,
                                       void* workspace, size_t workspace_bytes,
                                       msmd_stream_t stream) {
  if (n < 0 || num_classes < 1 || !sum || !(gamma >= 0.f)) return MSMD_ERR_INVALID_ARG;
  if (n > 0 && (!logits || !labels || !weights)) return MSMD_ERR_INVALID_ARG;
  const long per = (long)kSigFocalBlock * kSigFocalPerThread;
  const long blocks = (n * num_classes + per - 1) / per;
  if (blocks >= 2147483647L) return MSMD_ERR_RANGE;
  if (!workspace || ((uintptr_t)workspace & 7) ||
      workspace_bytes < msmd_sigmoid_focal_workspace_bytes(n, num_classes))
    return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (blocks > 0)
    MSMD_LAUNCH(sigmoid_focal_kernel, dim3((unsigned)blocks), dim3(kSigFocalBlock), 0, st, logits,
                labels, weights, (long)n, num_classes, gamma, alpha, grad, (double*)workspace);
  MSMD_LAUNCH(partials_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace,
              (int)blocks, sum);
  return launch_status();
}
