// roi_targets.hip -- Part-A2's second-stage targets (COVERAGE n10): what
// PartAggregationROIHead._assign_and_sample (models/roi_heads/part_aggregation_roi_head.py:
// 222-294) and PartA2BboxHead.get_targets (bbox_heads/parta2_bbox_head.py:356-460) compute per
// sample and per class in Python, for the whole batch in three launches with nothing read back.
//
//   roi_gt_max_kernel    pass one of MaxIoUAssigner.assign_wrt_overlaps over the 3-D IoU of
//   roi_assign_kernel    BboxOverlaps3D(coordinate='lidar'), as anchor.hip does it for the
//                        nearest-BEV IoU: one lane per proposal, the sample's ground truths
//                        staged through LDS kRoiGtChunk at a time, the per-ground-truth maximum
//                        by integer atomicMax on the bits of the non-negative IoU (independent
//                        of the order of arrival), rules 1-4 in pass two with the IoU
//                        recomputed by the same function.  The IoU matrix is never formed.
//                        Class-aware form: an IoU is only formed where the proposal's label
//                        equals the ground truth's label and lies in [0, C) -- the reference's
//                        pred_per_cls / gt_per_cls split -- and the thresholds are those of
//                        that class.  Single form: no label test, one threshold triple.
//   roi_sample_targets_kernel
//                        IoUNegPiecewiseSampler.sample (core/bbox/samplers/
//                        iou_neg_piecewise_sampler.py) and _get_target_single, one workgroup per
//                        sample, no atomics.  random_choice(gallery, n) is "the n entries with
//                        the smallest keys, ties to the lower proposal index": a lane ranks its
//                        proposal among those of its category by a walk over the keys in LDS.
//
// The pair IoU is bev::iou3d_pair, the function boxes_iou3d_kernel calls, with the ground truth
// as the first box -- the assigner's `iou_calculator(gt_bboxes, bboxes)` (the float32 polygon
// area is not symmetric in its arguments): max_overlaps equals the entries of
// msmd_boxes_iou3d_f32(gt, proposals) bit for bit.  A proposal or ground truth with a NaN
// coordinate takes part in no pair (fminf / fmaxf would drop the NaN and return a finite,
// meaningless number): its own row is "ignored", every other row is what it would be without it.
#include <math.h>

#include "box_overlap.hpp"

namespace msmd {
namespace {

constexpr int kRoiBlock = 256;           // proposals per workgroup of the assigner: one lane each
constexpr int kRoiGtChunk = 64;          // ground truths staged in LDS at a time
constexpr int kRoiMaxSamples = 64;       // samples per call (the tables are kernel arguments)
constexpr int kRoiMaxClasses = 8;
constexpr int kRoiMaxProposals = 2048;   // proposals per sample of the sampler (LDS resident)
constexpr int kRoiMaxNum = 1024;         // sampler's `num`
constexpr int kRoiMaxPieces = 8;
constexpr int kRoiCats = kRoiMaxPieces + 2;   // positive, pieces, negative outside every piece

struct RoiSegments {
  int n;
  int prop[kRoiMaxSamples + 1];          // proposals of sample s: prop[s] .. prop[s+1]
  int gt[kRoiMaxSamples + 1];            // ground truths of sample s
};

struct RoiThresholds {
  int num_classes;                       // 0: the single-assigner form
  float pos[kRoiMaxClasses], neg[kRoiMaxClasses], min_pos[kRoiMaxClasses];
};

struct RoiSampler {
  int num, expected_pos, pieces;
  double neg_pos_ub;                     // < 0: none
  double fraction[kRoiMaxPieces];
  float piece_thr[kRoiMaxPieces];
  float cls_pos_thr, cls_neg_thr;
};

__device__ __forceinline__ bool locate(const RoiSegments& sg, int& seg, int& row0) {
  int b = blockIdx.x;
  for (int s = 0; s < sg.n; ++s) {
    const int len = sg.prop[s + 1] - sg.prop[s];
    const int nb = (len + kRoiBlock - 1) / kRoiBlock;
    if (b < nb) {
      seg = s;
      row0 = sg.prop[s] + b * kRoiBlock;
      return true;
    }
    b -= nb;
  }
  return false;
}

__device__ __forceinline__ bool row_has_nan(const float* r) {
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 7; ++k) bad = bad || r[k] != r[k];
  return bad;
}

// Class of a row for the pair test, -1: outside [0, C), matches nobody.  kNanRow is set on top
// for a row with a NaN coordinate: it still counts as a ground truth of its class (the
// reference's assigner would see it) but takes part in no pair.
constexpr int kNanRow = 0x100;
__device__ __forceinline__ int pair_class(const RoiThresholds& th, int64_t label, bool nan) {
  int c = 0;
  if (th.num_classes != 0) c = (label >= 0 && label < th.num_classes) ? (int)label : -1;
  return (c >= 0 && nan) ? (c | kNanRow) : c;
}

// Stage ground truths [first, first + count) of the flat list: 7 floats and the pair class.
__device__ __forceinline__ void stage_gt(const RoiThresholds& th, const float* __restrict__ gt_boxes,
                                         const int64_t* __restrict__ gt_labels, int first,
                                         int count, float* boxes, int* cls) {
  for (int k = threadIdx.x; k < count * 7; k += kRoiBlock) boxes[k] = gt_boxes[(size_t)first * 7 + k];
  __syncthreads();
  for (int j = threadIdx.x; j < count; j += kRoiBlock)
    cls[j] = pair_class(th, gt_labels ? gt_labels[first + j] : 0, row_has_nan(boxes + j * 7));
}

__device__ __forceinline__ uint32_t wave_max_bits(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, kWave));
  return v;
}

// Pass one: gt_max_bits[g] = max over the sample's proposals of g's class of the IoU's bits.
__global__ __launch_bounds__(kRoiBlock) void roi_gt_max_kernel(
    const RoiSegments sg, const RoiThresholds th, const float* __restrict__ proposals,
    const int64_t* __restrict__ prop_labels, const float* __restrict__ gt_boxes,
    const int64_t* __restrict__ gt_labels, uint32_t* __restrict__ gt_max_bits) {
  __shared__ float boxes[kRoiGtChunk * 7];
  __shared__ int gcls[kRoiGtChunk];
  int seg, row0;
  if (!locate(sg, seg, row0)) return;
  const int gbegin = sg.gt[seg], ng = sg.gt[seg + 1] - gbegin;
  if (ng <= 0) return;
  const int row = row0 + threadIdx.x;
  const bool live = row < sg.prop[seg + 1];
  float p[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int pc = -1;
  if (live) {
#pragma unroll
    for (int k = 0; k < 7; ++k) p[k] = proposals[(size_t)row * 7 + k];
    pc = pair_class(th, prop_labels ? prop_labels[row] : 0, row_has_nan(p));
  }
  const int lane = threadIdx.x & (kWave - 1);
  for (int c0 = 0; c0 < ng; c0 += kRoiGtChunk) {
    const int count = min(ng - c0, kRoiGtChunk);
    __syncthreads();
    stage_gt(th, gt_boxes, gt_labels, gbegin + c0, count, boxes, gcls);
    __syncthreads();
    for (int j = 0; j < count; ++j) {
      const bool pair = pc >= 0 && pc < kNanRow && gcls[j] == pc;
      if (__ballot(pair) == 0ull) continue;                 // uniform over the wave
      const float iou = pair ? bev::iou3d_pair(boxes + j * 7, p, false) : 0.f;
      const uint32_t bits = iou > 0.f ? __float_as_uint(iou) : 0u;   // NaN stays out
      const uint32_t m = wave_max_bits(bits);
      if (lane == 0 && m) atomicMax(&gt_max_bits[gbegin + c0 + j], m);
    }
  }
}

// Pass two: rules 1-4 per proposal.
__global__ __launch_bounds__(kRoiBlock) void roi_assign_kernel(
    const RoiSegments sg, const RoiThresholds th, const float* __restrict__ proposals,
    const int64_t* __restrict__ prop_labels, const float* __restrict__ gt_boxes,
    const int64_t* __restrict__ gt_labels, const uint32_t* __restrict__ gt_max_bits,
    int32_t* __restrict__ gt_inds, float* __restrict__ max_overlaps,
    int64_t* __restrict__ labels) {
  __shared__ float boxes[kRoiGtChunk * 7];
  __shared__ int gcls[kRoiGtChunk];
  __shared__ float gmax[kRoiGtChunk];
  int seg, row0;
  if (!locate(sg, seg, row0)) return;
  const int gbegin = sg.gt[seg], ng = max(sg.gt[seg + 1] - gbegin, 0);
  const int row = row0 + threadIdx.x;
  const bool live = row < sg.prop[seg + 1];
  float p[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int pc = -1;
  bool nan_row = false;
  if (live) {
#pragma unroll
    for (int k = 0; k < 7; ++k) p[k] = proposals[(size_t)row * 7 + k];
    nan_row = row_has_nan(p);
    pc = pair_class(th, prop_labels ? prop_labels[row] : 0, nan_row);
  }
  float best = -1.f;
  int arg = -1, low = -1, same = 0;     // same: ground truths of this proposal's class
  for (int c0 = 0; c0 < ng; c0 += kRoiGtChunk) {
    const int count = min(ng - c0, kRoiGtChunk);
    __syncthreads();
    stage_gt(th, gt_boxes, gt_labels, gbegin + c0, count, boxes, gcls);
    for (int j = threadIdx.x; j < count; j += kRoiBlock)
      gmax[j] = __uint_as_float(gt_max_bits[gbegin + c0 + j]);
    __syncthreads();
    if (pc < 0 || nan_row) continue;
    const float min_pos = th.min_pos[pc];
    for (int j = 0; j < count; ++j) {
      if ((gcls[j] & (kNanRow - 1)) != pc || gcls[j] < 0) continue;
      ++same;
      if (gcls[j] != pc) continue;      // a NaN ground truth: counted, never matched
      const float iou = bev::iou3d_pair(boxes + j * 7, p, false);
      if (iou > best) {                 // strict: ties go to the lowest index
        best = iou;
        arg = c0 + j;
      }
      const float gm = gmax[j];
      if (gm >= min_pos && iou == gm) low = c0 + j;   // rule 4: the last claimant wins
    }
  }
  if (!live) return;
  int result;
  float overlap;
  if (nan_row) {                        // takes part in no pair: ignored
    result = -1;
    overlap = __int_as_float(0x7fc00000);
  } else if (pc < 0 || same == 0) {     // no assigner ran (:246-249), or it had no ground truth
    result = 0;
    overlap = 0.f;
  } else {
    if (best < 0.f) best = 0.f;         // every ground truth of the class is a NaN box
    result = -1;                                          // rule 1
    if (best >= 0.f && best < th.neg[pc]) result = 0;     // rule 2
    if (best >= th.pos[pc] && arg >= 0) result = arg + 1; // rule 3
    if (low >= 0) result = low + 1;                       // rule 4
    overlap = best;
  }
  gt_inds[row] = result;
  max_overlaps[row] = overlap;
  labels[row] = (result > 0 && gt_labels) ? gt_labels[gbegin + result - 1] : (int64_t)-1;
}

// torch.remainder(a, b) for b > 0 as ATen computes it: fmod, then the sign fix.
__device__ __forceinline__ float remainder_pos(float a, float b) {
  float m = fmodf(a, b);
  if (m != 0.f && m < 0.f) m = __fadd_rn(m, b);
  return m;
}

// One workgroup per sample.
__global__ __launch_bounds__(kRoiBlock) void roi_sample_targets_kernel(
    const RoiSegments sg, const RoiSampler sp, const float* __restrict__ proposals,
    const int32_t* __restrict__ gt_inds, const float* __restrict__ max_overlaps,
    const float* __restrict__ keys, const float* __restrict__ gt_boxes,
    float* __restrict__ rois /* [B,num,8] */, float* __restrict__ ious /* [B,num] */,
    float* __restrict__ label, float* __restrict__ label_weights, int64_t* __restrict__ reg_mask,
    float* __restrict__ bbox_weights, float* __restrict__ pos_gt_bboxes /* [B,num,7] */,
    float* __restrict__ bbox_targets /* [B,num,7] */, int32_t* __restrict__ sampled_inds,
    int32_t* __restrict__ counts /* [B,2] */) {
  __shared__ float key[kRoiMaxProposals];
  __shared__ signed char cat[kRoiMaxProposals];
  __shared__ int wave_counts[kRoiBlock / kWave][kRoiCats];
  __shared__ int scan_smem[kRoiBlock / kWave];
  __shared__ int s_count[kRoiCats], s_quota[kRoiCats + 2];   // + the two totals
  const int s = blockIdx.x, tid = threadIdx.x;
  const int pbegin = sg.prop[s], np = sg.prop[s + 1] - pbegin;
  const int gbegin = sg.gt[s], ng = max(sg.gt[s + 1] - gbegin, 0);
  const int pieces = sp.pieces;

  // categories: 0 positive, 1 + k negative of piece k, 1 + pieces negative outside every piece
  int mine[kRoiCats];
#pragma unroll
  for (int c = 0; c < kRoiCats; ++c) mine[c] = 0;
  for (int i = tid; i < np; i += kRoiBlock) {
    const int g = gt_inds[pbegin + i];
    const float ov = max_overlaps[pbegin + i];
    int c = -1;
    if (g > 0) {
      c = 0;
    } else if (g == 0) {
      c = 1 + pieces;
      for (int k = 0; k < pieces; ++k) {
        const float lo = k == pieces - 1 ? 0.f : sp.piece_thr[k + 1];
        if (ov >= lo && ov < sp.piece_thr[k]) {
          c = 1 + k;
          break;                        // (pieces descend: the first that holds it)
        }
      }
    }
    key[i] = keys[pbegin + i];
    cat[i] = (signed char)c;
#pragma unroll
    for (int q = 0; q < kRoiCats; ++q) mine[q] += (c == q);
  }
#pragma unroll
  for (int q = 0; q < kRoiCats; ++q) {
    const int v = wave_sum(mine[q]);
    if ((tid & (kWave - 1)) == 0) wave_counts[tid / kWave][q] = v;
  }
  __syncthreads();
  // the reference's quota arithmetic (sample :132-147, _sample_neg :56-96), by one lane
  if (tid == 0) {
    int count[kRoiCats];
    for (int q = 0; q < kRoiCats; ++q) {
      int v = 0;
      for (int w = 0; w < kRoiBlock / kWave; ++w) v += wave_counts[w][q];
      count[q] = v;
      s_count[q] = v;
      s_quota[q] = 0;
    }
    const int pos = min(count[0], max(sp.expected_pos, 0));
    s_quota[0] = pos;
    int expected_neg = sp.num - pos;
    if (sp.neg_pos_ub >= 0) {
      const int upper = (int)(sp.neg_pos_ub * (double)max(1, pos));
      if (expected_neg > upper) expected_neg = upper;
    }
    int all_neg = 0;
    for (int q = 1; q <= 1 + pieces; ++q) all_neg += count[q];
    int neg = 0;
    if (all_neg <= expected_neg) {      // :61-62: every negative, also those no piece holds
      for (int q = 1; q <= 1 + pieces; ++q) s_quota[q] = count[q];
      neg = all_neg;
    } else {
      int extend = 0;
      for (int k = 0; k < pieces; ++k) {
        const int want = k == pieces - 1 ? expected_neg - neg
                                         : (int)((double)expected_neg * sp.fraction[k]) + extend;
        int got;
        if (count[1 + k] < want) {
          got = count[1 + k];
          extend += want - got;
        } else {
          got = max(want, 0);
          extend = 0;
        }
        s_quota[1 + k] = got;
        neg += got;
      }
    }
    s_quota[kRoiCats] = pos;
    s_quota[kRoiCats + 1] = neg;
  }
  __syncthreads();
  const int n_pos = s_quota[kRoiCats], n_neg = s_quota[kRoiCats + 1];
  const int total = min(n_pos + n_neg, sp.num);      // (n_pos + n_neg <= num by construction)

  // rank within the category, select, compact: positives ascending, then negatives ascending
  int base_pos = 0, base_neg = 0;
  const size_t out0 = (size_t)s * sp.num;
  for (int i0 = 0; i0 < np; i0 += kRoiBlock) {
    const int i = i0 + tid;
    int c = -1;
    bool take = false;
    if (i < np) {
      c = cat[i];
      if (c >= 0) {
        const int q = s_quota[c];
        if (q >= s_count[c]) {
          take = q > 0;
        } else if (q > 0) {
          const float kx = key[i];
          int rank = 0;
          for (int j = 0; j < np; ++j)
            rank += (cat[j] == c) && (key[j] < kx || (key[j] == kx && j < i));
          take = rank < q;
        }
      }
    }
    const int packed = take ? (c == 0 ? 1 : 1 << 16) : 0;
    int tot;
    const int ex = block_excl_scan<kRoiBlock>(packed, scan_smem, &tot);
    if (take) {
      const int r = c == 0 ? base_pos + (ex & 0xffff) : n_pos + base_neg + (ex >> 16);
      if (r < sp.num) {
        const size_t o = out0 + r;
        const float* box = proposals + (size_t)(pbegin + i) * 7;
        float roi[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) roi[k] = box[k];
        rois[o * 8] = (float)s;
#pragma unroll
        for (int k = 0; k < 7; ++k) rois[o * 8 + 1 + k] = roi[k];
        const float ov = max_overlaps[pbegin + i];
        ious[o] = ov;
        sampled_inds[o] = i;
        // _get_target_single :413-421
        float lb = ov > sp.cls_pos_thr ? 1.f : 0.f;
        if (!(ov > sp.cls_pos_thr) && !(ov < sp.cls_neg_thr))
          lb = __fsub_rn(__fmul_rn(ov, 2.f), 0.5f);
        label[o] = lb;
        label_weights[o] = lb >= 0.f ? 1.f : 0.f;
        reg_mask[o] = c == 0 ? 1 : 0;
        bbox_weights[o] = c == 0 ? 1.f : 0.f;
        float* gt_out = pos_gt_bboxes + o * 7;
        float* bt = bbox_targets + o * 7;
        const int g = gt_inds[pbegin + i] - 1;
        if (c == 0 && g >= 0 && g < ng) {
          const float* gt = gt_boxes + (size_t)(gbegin + g) * 7;
          float ct[7];
#pragma unroll
          for (int k = 0; k < 7; ++k) {
            ct[k] = gt[k];
            gt_out[k] = gt[k];
          }
          // :428-448, float32 as written
          const float two_pi = 6.283185307179586f, pi = 3.141592653589793f;
          const float half_pi = 1.5707963267948966f, pi15 = 4.71238898038469f;
          const float roi_ry = remainder_pos(roi[6], two_pi);
          const float dx = __fsub_rn(ct[0], roi[0]), dy = __fsub_rn(ct[1], roi[1]);
          const float dz = __fsub_rn(ct[2], roi[2]);
          const float angle = -__fadd_rn(roi_ry, half_pi);
          const float sn = sinf(angle), cs = cosf(angle);
          ct[0] = __fadd_rn(__fadd_rn(__fmul_rn(dx, cs), __fmul_rn(dy, sn)), __fmul_rn(dz, 0.f));
          ct[1] = __fadd_rn(__fadd_rn(__fmul_rn(dx, -sn), __fmul_rn(dy, cs)), __fmul_rn(dz, 0.f));
          ct[2] = __fadd_rn(__fadd_rn(__fmul_rn(dx, 0.f), __fmul_rn(dy, 0.f)), dz);
          float ry = remainder_pos(__fsub_rn(ct[6], roi_ry), two_pi);
          if (ry > half_pi && ry < pi15) ry = remainder_pos(__fadd_rn(ry, pi), two_pi);
          if (ry > pi) ry = __fsub_rn(ry, two_pi);
          ry = ry < -half_pi ? -half_pi : (ry > half_pi ? half_pi : ry);     // NaN goes through
          // DeltaXYZWLHRBBoxCoder.encode against (0, 0, 0, w, l, h, 0)
          const float wa = roi[3], la = roi[4], ha = roi[5];
          const float za = __fadd_rn(0.f, ha / 2.f), zg = __fadd_rn(ct[2], ct[5] / 2.f);
          const float diagonal = sqrtf(__fadd_rn(__fmul_rn(la, la), __fmul_rn(wa, wa)));
          bt[0] = ct[0] / diagonal;
          bt[1] = ct[1] / diagonal;
          bt[2] = __fsub_rn(zg, za) / ha;
          bt[3] = logf(ct[3] / wa);
          bt[4] = logf(ct[4] / la);
          bt[5] = logf(ct[5] / ha);
          bt[6] = ry;
        } else {
#pragma unroll
          for (int k = 0; k < 7; ++k) {
            gt_out[k] = 0.f;
            bt[k] = 0.f;
          }
        }
      }
    }
    base_pos += tot & 0xffff;
    base_neg += tot >> 16;
  }

  // the padding rows of this sample: every output element is written
  for (int r = total + tid; r < sp.num; r += kRoiBlock) {
    const size_t o = out0 + r;
    for (int k = 0; k < 8; ++k) rois[o * 8 + k] = 0.f;
    ious[o] = 0.f;
    sampled_inds[o] = -1;
    label[o] = 0.f;
    label_weights[o] = 0.f;
    reg_mask[o] = 0;
    bbox_weights[o] = 0.f;
    for (int k = 0; k < 7; ++k) {
      pos_gt_bboxes[o * 7 + k] = 0.f;
      bbox_targets[o * 7 + k] = 0.f;
    }
  }
  if (tid == 0) {
    counts[s * 2] = min(n_pos, total);
    counts[s * 2 + 1] = total - min(n_pos, total);
  }
}

// The host's tables: ascending offsets from 0.  -> workgroups of the assigner, or -1.
int fill_roi_segments(const int32_t* prop_offsets, const int32_t* gt_offsets, int batch,
                      RoiSegments& sg) {
  if (!prop_offsets || !gt_offsets || batch < 1 || batch > kRoiMaxSamples) return -1;
  if (prop_offsets[0] != 0 || gt_offsets[0] != 0) return -1;
  long blocks = 0;
  sg.n = batch;
  sg.prop[0] = sg.gt[0] = 0;
  for (int s = 0; s < batch; ++s) {
    if (prop_offsets[s + 1] < prop_offsets[s] || gt_offsets[s + 1] < gt_offsets[s]) return -1;
    sg.prop[s + 1] = prop_offsets[s + 1];
    sg.gt[s + 1] = gt_offsets[s + 1];
    blocks += ceil_div((long)prop_offsets[s + 1] - prop_offsets[s], kRoiBlock);
  }
  return (int)blocks;
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_roi_assign_max_samples(void) { return kRoiMaxSamples; }
MSMD_EXPORT int msmd_roi_assign_max_classes(void) { return kRoiMaxClasses; }
MSMD_EXPORT int msmd_roi_assign_gt_chunk(void) { return kRoiGtChunk; }
MSMD_EXPORT int msmd_roi_sample_max_proposals(void) { return kRoiMaxProposals; }
MSMD_EXPORT int msmd_roi_sample_max_num(void) { return kRoiMaxNum; }
MSMD_EXPORT int msmd_roi_sample_max_pieces(void) { return kRoiMaxPieces; }

MSMD_EXPORT size_t msmd_roi_assign3d_workspace_bytes(int num_gt) {
  if (num_gt < 0) return 0;
  return align_up((size_t)(num_gt > 0 ? num_gt : 1) * sizeof(uint32_t));
}

MSMD_EXPORT int msmd_roi_assign3d_f32(const float* proposals, const int64_t* proposal_labels,
                                      const int32_t* proposal_offsets, const float* gt_boxes,
                                      const int64_t* gt_labels, const int32_t* gt_offsets,
                                      int batch, int num_classes, int single,
                                      const float* pos_iou_thr, const float* neg_iou_thr,
                                      const float* min_pos_iou, int32_t* gt_inds,
                                      float* max_overlaps, int64_t* labels, void* workspace,
                                      size_t workspace_bytes, msmd_stream_t stream) {
  if (batch < 0 || num_classes < 1 || (single != 0 && single != 1)) return MSMD_ERR_INVALID_ARG;
  if (batch == 0) return MSMD_OK;
  if (batch > kRoiMaxSamples || num_classes > kRoiMaxClasses) return MSMD_ERR_RANGE;
  if (!pos_iou_thr || !neg_iou_thr || !min_pos_iou) return MSMD_ERR_INVALID_ARG;
  RoiSegments sg;
  const int blocks = fill_roi_segments(proposal_offsets, gt_offsets, batch, sg);
  if (blocks < 0) return MSMD_ERR_INVALID_ARG;
  const int total = sg.prop[batch], num_gt = sg.gt[batch];
  if ((long)total * 7 >= 2147483647L || (long)num_gt * 7 >= 2147483647L) return MSMD_ERR_RANGE;
  if (total == 0) return MSMD_OK;
  if (!proposals || !gt_inds || !max_overlaps || !labels) return MSMD_ERR_INVALID_ARG;
  if (!single && !proposal_labels) return MSMD_ERR_INVALID_ARG;
  if (num_gt > 0 && (!gt_boxes || !gt_labels)) return MSMD_ERR_INVALID_ARG;
  if (!workspace || ((uintptr_t)workspace & 3) ||
      workspace_bytes < msmd_roi_assign3d_workspace_bytes(num_gt))
    return MSMD_ERR_WORKSPACE;
  RoiThresholds th;
  th.num_classes = single ? 0 : num_classes;
  for (int c = 0; c < kRoiMaxClasses; ++c) {
    const int k = single ? 0 : (c < num_classes ? c : 0);
    th.pos[c] = pos_iou_thr[k];
    th.neg[c] = neg_iou_thr[k];
    th.min_pos[c] = min_pos_iou[k];
  }
  hipStream_t st = (hipStream_t)stream;
  uint32_t* gt_max = (uint32_t*)workspace;
  if (num_gt > 0) {
    if (hipMemsetAsync(gt_max, 0, sizeof(uint32_t) * (size_t)num_gt, st) != hipSuccess)
      return MSMD_ERR_LAUNCH;
    MSMD_LAUNCH(roi_gt_max_kernel, dim3(blocks), dim3(kRoiBlock), 0, st, sg, th, proposals,
                single ? nullptr : proposal_labels, gt_boxes, gt_labels, gt_max);
  }
  MSMD_LAUNCH(roi_assign_kernel, dim3(blocks), dim3(kRoiBlock), 0, st, sg, th, proposals,
              single ? nullptr : proposal_labels, gt_boxes, gt_labels, gt_max, gt_inds,
              max_overlaps, labels);
  return launch_status();
}

MSMD_EXPORT int msmd_roi_sample_targets_f32(
    const float* proposals, const int32_t* proposal_offsets, const int32_t* gt_inds,
    const float* max_overlaps, const float* keys, const float* gt_boxes,
    const int32_t* gt_offsets, int batch, int num, int num_expected_pos, double neg_pos_ub,
    int num_pieces, const double* neg_piece_fractions, const float* neg_iou_piece_thrs,
    float cls_pos_thr, float cls_neg_thr, float* rois, float* ious, float* label,
    float* label_weights, int64_t* reg_mask, float* bbox_weights, float* pos_gt_bboxes,
    float* bbox_targets, int32_t* sampled_inds, int32_t* counts, msmd_stream_t stream) {
  if (batch < 0 || num < 1 || num_expected_pos < 0 || num_pieces < 1 || neg_pos_ub != neg_pos_ub)
    return MSMD_ERR_INVALID_ARG;
  if (num_expected_pos > num) return MSMD_ERR_INVALID_ARG;   // the positives fit into `num` rows
  if (batch == 0) return MSMD_OK;
  if (batch > kRoiMaxSamples || num > kRoiMaxNum || num_pieces > kRoiMaxPieces)
    return MSMD_ERR_RANGE;
  if (!neg_piece_fractions || !neg_iou_piece_thrs) return MSMD_ERR_INVALID_ARG;
  RoiSegments sg;
  if (fill_roi_segments(proposal_offsets, gt_offsets, batch, sg) < 0) return MSMD_ERR_INVALID_ARG;
  for (int s = 0; s < batch; ++s)
    if (sg.prop[s + 1] - sg.prop[s] > kRoiMaxProposals) return MSMD_ERR_RANGE;
  const int total = sg.prop[batch], num_gt = sg.gt[batch];
  if ((long)total * 7 >= 2147483647L || (long)num_gt * 7 >= 2147483647L) return MSMD_ERR_RANGE;
  // the quotas stay within `num` only for fractions in [0, 1] that sum to at most 1
  double sum = 0;
  for (int k = 0; k < num_pieces; ++k) {
    const double f = neg_piece_fractions[k];
    if (!(f >= 0.0 && f <= 1.0)) return MSMD_ERR_INVALID_ARG;
    if (k < num_pieces - 1) sum += f;
    // pieces are [thr[k+1], thr[k]): disjoint only when the bounds do not ascend
    if (k > 0 && !(neg_iou_piece_thrs[k] <= neg_iou_piece_thrs[k - 1])) return MSMD_ERR_INVALID_ARG;
  }
  if (sum > 1.0) return MSMD_ERR_INVALID_ARG;
  if (!rois || !ious || !label || !label_weights || !reg_mask || !bbox_weights ||
      !pos_gt_bboxes || !bbox_targets || !sampled_inds || !counts)
    return MSMD_ERR_INVALID_ARG;
  if (total > 0 && (!proposals || !gt_inds || !max_overlaps || !keys)) return MSMD_ERR_INVALID_ARG;
  if (num_gt > 0 && !gt_boxes) return MSMD_ERR_INVALID_ARG;
  RoiSampler sp;
  sp.num = num;
  sp.expected_pos = num_expected_pos;
  sp.pieces = num_pieces;
  sp.neg_pos_ub = neg_pos_ub;
  for (int k = 0; k < kRoiMaxPieces; ++k) {
    sp.fraction[k] = k < num_pieces ? neg_piece_fractions[k] : 0.0;
    sp.piece_thr[k] = k < num_pieces ? neg_iou_piece_thrs[k] : 0.f;
  }
  sp.cls_pos_thr = cls_pos_thr;
  sp.cls_neg_thr = cls_neg_thr;
  MSMD_LAUNCH(roi_sample_targets_kernel, dim3(batch), dim3(kRoiBlock), 0, (hipStream_t)stream, sg,
              sp, proposals, gt_inds, max_overlaps, keys, gt_boxes, rois, ious, label,
              label_weights, reg_mask, bbox_weights, pos_gt_bboxes, bbox_targets, sampled_inds,
              counts);
  return launch_status();
}
