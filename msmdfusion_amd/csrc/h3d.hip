// h3d.hip -- H3DNet's second stage (COVERAGE n8): the cue centres of a box and the fused cue
// targets of H3DBboxHead.
//
//   box_cue_centers      DepthInstance3DBoxes.get_surface_line_center
//                        (core/bbox/structures/depth_box3d.py:277-330): about thirty small
//                        torch ops there; one lane per box here, forward and backward.
//   h3d_cue_targets      H3DBboxHead.get_targets_single
//                        (models/roi_heads/bbox_heads/h3d_bbox_head.py:761-932) under multi_apply:
//                        per sample three chamfer_distance calls that expand [1, N, M, 3], two
//                        get_surface_line_center calls and about sixty small ops, seven of
//                        them masked assignments (a nonzero and a host read each).  One launch
//                        for the batch here, nothing read back.
//
// Cue geometry (cue_center, shared by both): the 6 face centres and 12 edge centres of a box in
// gravity-centre form (cx, cy, cz, sx, sy, sz, yaw).  Row r = box * 6 + f (resp. box * 12 + l)
// is the box's centre plus its half-size offset turned about z by the yaw OF BOX r % n, n the
// number of boxes of the call: the reference repeats its rotation matrices with
// rot_mat_T.repeat(6, 1, 1) against box-major offset rows, and this is reproduced.  The angle
// is -yaw (sin(-yaw), cos(-yaw)), as there.  The arithmetic is double from the float32 inputs,
// rounded to float32 once per coordinate.
//
// Cue targets: a workgroup owns 14 proposals x 18 cues = 252 of its 256 lanes, one lane per
// (proposal, cue).  Every lane finds its proposal's nearest ground-truth centre (the sample's
// centres pass through LDS 64 at a time, every lane reads the same address: a broadcast), takes
// that box's cue centre, then walks the predicted surface centres (cues 0-5) or line centres
// (cues 6-17) through LDS 256 at a time -- both sets are staged side by side, so a wavefront
// that holds both kinds of lanes costs max(Ns, Nl) steps, not Ns + Nl, and reads two LDS
// addresses per step.  Distances and the minimum are chamfer_common.hpp's, so every index is the
// one msmd_chamfer_fwd_f32 gives.  The OR over a proposal's 18 cues goes through LDS.  No
// atomics, every output element has one writer.
#include <math.h>

#include "chamfer_common.hpp"
#include "common.hpp"

namespace msmd {
namespace {

constexpr int kCues = 18;            // 6 faces, then 12 edges
constexpr int kCueFaces = 6;
constexpr int kCueProposals = 14;    // proposals per workgroup: 14 * 18 = 252 lanes of 256
constexpr int kCueGtChunk = 64;      // ground-truth centres per LDS chunk
constexpr int kCuePredChunk = 256;   // predicted centres per LDS chunk, per set
constexpr int kCueTileStride = kCuePredChunk * 3 + 3;  // words from the surface to the line tile
constexpr int kCueMaxClasses = 4096;

// depth_box3d.py:297-298 and :305-308, before the division by 2
__constant__ signed char kCueSign[kCues][3] = {
    {0, 0, 1},  {0, 0, -1}, {0, 1, 0},  {0, -1, 0},  {1, 0, 0},  {-1, 0, 0},
    {1, 0, 1},  {-1, 0, 1}, {0, 1, 1},  {0, -1, 1},  {1, 0, -1}, {-1, 0, -1},
    {0, 1, -1}, {0, -1, -1}, {1, 1, 0}, {1, -1, 0},  {-1, 1, 0}, {-1, -1, 0}};

// which box turns row (box, cue) of a call over n boxes
__device__ __forceinline__ int cue_rotator(int box, int cue, int n) {
  const bool face = cue < kCueFaces;
  const long r = face ? (long)box * kCueFaces + cue
                      : (long)box * (kCues - kCueFaces) + (cue - kCueFaces);
  return (int)(r % n);
}

// cue `cue` (0-5 faces, 6-17 edges) of box `box` among the n boxes at `boxes` ([n, 7])
__device__ __forceinline__ void cue_center(const float* __restrict__ boxes, int n, int box,
                                           int cue, float* out) {
  const float* me = boxes + (size_t)box * 7;
  const double yaw = (double)boxes[(size_t)cue_rotator(box, cue, n) * 7 + 6];
  const double s = sin(-yaw), c = cos(-yaw);
  const double vx = 0.5 * kCueSign[cue][0] * (double)me[3];
  const double vy = 0.5 * kCueSign[cue][1] * (double)me[4];
  const double vz = 0.5 * kCueSign[cue][2] * (double)me[5];
  out[0] = (float)((double)me[0] + (c * vx - s * vy));
  out[1] = (float)((double)me[1] + (s * vx + c * vy));
  out[2] = (float)((double)me[2] + vz);
}

__global__ __launch_bounds__(256) void box_cue_centers_kernel(const float* __restrict__ boxes,
                                                              int n, float* __restrict__ surface,
                                                              float* __restrict__ line) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
#pragma unroll 1
  for (int cue = 0; cue < kCues; ++cue) {
    float c[3];
    cue_center(boxes, n, b, cue, c);
    float* out = cue < kCueFaces
                     ? surface + ((size_t)b * kCueFaces + cue) * 3
                     : line + ((size_t)b * (kCues - kCueFaces) + (cue - kCueFaces)) * 3;
    out[0] = c[0], out[1] = c[1], out[2] = c[2];
  }
}

// One lane per box b.  Centre and sizes: its own 18 rows, each turned by box r % n.  Yaw: the
// 6 + 12 rows r = b (mod n), i.e. r = b + k * n, which belong to box r / 6 (resp. r / 12).
// Ascending cue / k order, double sums, rounded once.
__global__ __launch_bounds__(256) void box_cue_centers_bwd_kernel(
    const float* __restrict__ boxes, int n, const float* __restrict__ g_surface,
    const float* __restrict__ g_line, float* __restrict__ grad) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
  const float* me = boxes + (size_t)b * 7;
  double gc[3] = {0., 0., 0.}, gs[3] = {0., 0., 0.}, gyaw = 0.;
#pragma unroll 1
  for (int cue = 0; cue < kCues; ++cue) {
    const bool face = cue < kCueFaces;
    const float* g = face ? g_surface + ((size_t)b * kCueFaces + cue) * 3
                          : g_line + ((size_t)b * (kCues - kCueFaces) + (cue - kCueFaces)) * 3;
    const double yaw = (double)boxes[(size_t)cue_rotator(b, cue, n) * 7 + 6];
    const double s = sin(-yaw), c = cos(-yaw);
    const double gx = g[0], gy = g[1], gz = g[2];
    gc[0] += gx, gc[1] += gy, gc[2] += gz;
    gs[0] += 0.5 * kCueSign[cue][0] * (c * gx + s * gy);
    gs[1] += 0.5 * kCueSign[cue][1] * (c * gy - s * gx);
    gs[2] += 0.5 * kCueSign[cue][2] * gz;
  }
  const double yaw = (double)me[6];
  const double s = sin(-yaw), c = cos(-yaw);
#pragma unroll 1
  for (int part = 0; part < 2; ++part) {
    const int per = part == 0 ? kCueFaces : kCues - kCueFaces;
    const float* gbase = part == 0 ? g_surface : g_line;
    for (int k = 0; k < per; ++k) {
      const long r = (long)b + (long)k * n;
      const int box = (int)(r / per);
      const int cue = (int)(r - (long)box * per) + (part == 0 ? 0 : kCueFaces);
      const float* o = boxes + (size_t)box * 7;
      const double vx = 0.5 * kCueSign[cue][0] * (double)o[3];
      const double vy = 0.5 * kCueSign[cue][1] * (double)o[4];
      const float* g = gbase + (size_t)r * 3;
      // d/dyaw of (c vx - s vy, s vx + c vy) with s = sin(-yaw), c = cos(-yaw)
      gyaw += (double)g[0] * (s * vx + c * vy) + (double)g[1] * (s * vy - c * vx);
    }
  }
  float* out = grad + (size_t)b * 7;
  out[0] = (float)gc[0], out[1] = (float)gc[1], out[2] = (float)gc[2];
  out[3] = (float)gs[0], out[4] = (float)gs[1], out[5] = (float)gs[2];
  out[6] = (float)gyaw;
}

struct CueThresholds {
  float near_thr, far_thr, label_surface, label_line, mask_surface, mask_line;
};

// grid: B * ceil(P / 14) workgroups of 256
__global__ __launch_bounds__(256) void h3d_cue_targets_kernel(
    const float* __restrict__ aggregated, const float* __restrict__ gt_boxes,
    const int32_t* __restrict__ gt_counts, const int64_t* __restrict__ gt_labels,
    const float* __restrict__ surface_pred, const float* __restrict__ line_pred,
    const float* __restrict__ surface_sem, const float* __restrict__ line_sem,
    const float* __restrict__ surface_obj, const float* __restrict__ line_obj, int P, int G,
    int Ns, int Nl, int C, CueThresholds thr, int64_t* __restrict__ cues_objectness_label,
    int64_t* __restrict__ cues_sem_label, int64_t* __restrict__ cues_matching_label,
    float* __restrict__ cues_mask, int64_t* __restrict__ proposal_objectness_label,
    float* __restrict__ proposal_objectness_mask, float* __restrict__ cues_match_mask,
    float* __restrict__ obj_center) {
  __shared__ float gt_c[kCueGtChunk * 3];
  // one array for both tiles, the line tile 3 words past a multiple of the 32 banks: every
  // wavefront holds face and edge lanes, and the two addresses of a step never share a bank
  __shared__ float tiles[2 * kCueTileStride];
  float* tile_s = tiles;
  float* tile_l = tiles + kCueTileStride;
  __shared__ int flag[256];
  const int per_sample = (P + kCueProposals - 1) / kCueProposals;
  const int b = blockIdx.x / per_sample;
  const int t = threadIdx.x;
  const int pl = t / kCues, cue = t - pl * kCues;
  const int p = (blockIdx.x - b * per_sample) * kCueProposals + pl;
  const bool live = pl < kCueProposals && p < P;
  const bool face = cue < kCueFaces;
  // a count outside 1 .. G is clipped: rows past the count are never read
  int n = gt_counts[b];
  n = n < 1 ? 1 : (n > G ? G : n);
  const float* boxes = gt_boxes + (size_t)b * G * 7;

  // the proposal's nearest ground-truth centre (chamfer_distance, :804-809)
  float mine[3] = {0.f, 0.f, 0.f};
  if (live) {
    const float* a = aggregated + ((size_t)b * P + p) * 3;
    mine[0] = a[0], mine[1] = a[1], mine[2] = a[2];
  }
  float best = INFINITY;
  int at = 0;
  for (int base = 0; base < n; base += kCueGtChunk) {
    const int cnt = min(n - base, kCueGtChunk);
    __syncthreads();
    for (int k = t; k < cnt * 3; k += 256) {
      const int j = k / 3;
      gt_c[k] = boxes[(size_t)(base + j) * 7 + (k - j * 3)];
    }
    __syncthreads();
    if (live)
      for (int j = 0; j < cnt; ++j) take_min(distance<kL2>(mine, gt_c + j * 3), base + j, best, at);
  }

  // that box's cue centre (:823-831), then the nearest predicted primitive centre (:836-841)
  float target[3] = {0.f, 0.f, 0.f};
  if (live) cue_center(boxes, n, at, cue, target);
  const float* tile = face ? tile_s : tile_l;
  const int longest = Ns > Nl ? Ns : Nl;
  const float* sp = surface_pred + (size_t)b * Ns * 3;
  const float* lp = line_pred + (size_t)b * Nl * 3;
  float best2 = INFINITY;
  int at2 = 0;
  for (int base = 0; base < longest; base += kCuePredChunk) {
    const int cs = max(0, min(Ns - base, kCuePredChunk));
    const int cl = max(0, min(Nl - base, kCuePredChunk));
    __syncthreads();
    for (int k = t; k < cs * 3; k += 256) tile_s[k] = sp[(size_t)base * 3 + k];
    for (int k = t; k < cl * 3; k += 256) tile_l[k] = lp[(size_t)base * 3 + k];
    __syncthreads();
    const int cnt = face ? cs : cl;
    if (live)
      for (int j = 0; j < cnt; ++j)
        take_min(distance<kL2>(target, tile + j * 3), base + j, best2, at2);
  }

  int label = 0;
  if (live) {
    const int row = face ? cue * P + p : kCueFaces * P + (cue - kCueFaces) * P + p;
    const size_t out = (size_t)b * kCues * P + row;
    const float* sel = (face ? sp : lp) + (size_t)at2 * 3;
    const float* scores = face ? surface_sem + ((size_t)b * Ns + at2) * C
                               : line_sem + ((size_t)b * Nl + at2) * C;
    // torch.argmax: the lowest index among the maxima, a NaN is a maximum
    float top = scores[0];
    int sem = 0;
    for (int c = 1; c < C; ++c) {
      const float v = scores[c];
      if (v > top || (v != v && top == top)) top = v, sem = c;
    }
    const float* own = face ? surface_obj + ((size_t)b * kCueFaces * P + row) * 3
                            : line_obj + ((size_t)b * (kCues - kCueFaces) * P +
                                          (row - kCueFaces * P)) * 3;
    const float d_center = sqrtf(__fadd_rn(best, 1e-6f));
    const float d_prim = sqrtf(__fadd_rn(best2, 1e-6f));
    const float d_own = sqrtf(__fadd_rn(distance<kL2>(own, sel), 1e-6f));
    const bool is_near = d_center < thr.near_thr;
    const bool counted = is_near || d_center > thr.far_thr;
    label = d_own < (face ? thr.label_surface : thr.label_line) &&
                    d_prim < (face ? thr.mask_surface : thr.mask_line)
                ? 1 : 0;
    const int sem_label = label && (float)sem == (float)gt_labels[(size_t)b * G + at] ? 1 : 0;
    // the two torch.cat copies are taken before the in-place *= with the proposal's label
    cues_objectness_label[out] = label;
    cues_sem_label[out] = sem_label;
    cues_matching_label[out] = is_near ? label : 0;
    cues_mask[out] = counted ? 1.f : 0.f;
    obj_center[out * 3] = target[0], obj_center[out * 3 + 1] = target[1];
    obj_center[out * 3 + 2] = target[2];
    if (cue == 0) {
      proposal_objectness_label[(size_t)b * P + p] = is_near ? 1 : 0;
      proposal_objectness_mask[(size_t)b * P + p] = counted ? 1.f : 0.f;
    }
  }
  // cues_match_mask: any of the proposal's 18 unmultiplied labels (:922-924)
  __syncthreads();
  flag[t] = label;
  __syncthreads();
  if (live && cue == 0) {
    int any = 0;
#pragma unroll
    for (int k = 0; k < kCues; ++k) any |= flag[t + k];
    cues_match_mask[(size_t)b * P + p] = any ? 1.f : 0.f;
  }
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_h3d_cue_gt_chunk(void) { return kCueGtChunk; }
MSMD_EXPORT int msmd_h3d_cue_pred_chunk(void) { return kCuePredChunk; }
MSMD_EXPORT int msmd_h3d_cue_proposals(void) { return kCueProposals; }

MSMD_EXPORT int msmd_box_cue_centers_f32(const float* boxes, int n, float* surface, float* line,
                                         msmd_stream_t stream) {
  if (n < 0) return MSMD_ERR_INVALID_ARG;
  if ((long)n * (kCues - kCueFaces) * 3 >= 2147483647L) return MSMD_ERR_RANGE;
  if (n == 0) return MSMD_OK;
  if (!boxes || !surface || !line) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(box_cue_centers_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream,
              boxes, n, surface, line);
  return launch_status();
}

MSMD_EXPORT int msmd_box_cue_centers_bwd_f32(const float* boxes, int n, const float* grad_surface,
                                             const float* grad_line, float* grad_boxes,
                                             msmd_stream_t stream) {
  if (n < 0) return MSMD_ERR_INVALID_ARG;
  if ((long)n * (kCues - kCueFaces) * 3 >= 2147483647L) return MSMD_ERR_RANGE;
  if (n == 0) return MSMD_OK;
  if (!boxes || !grad_surface || !grad_line || !grad_boxes) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(box_cue_centers_bwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0,
              (hipStream_t)stream, boxes, n, grad_surface, grad_line, grad_boxes);
  return launch_status();
}

MSMD_EXPORT int msmd_h3d_cue_targets_f32(
    const float* aggregated, const float* gt_boxes, const int32_t* gt_counts,
    const int64_t* gt_labels, const float* surface_pred, const float* line_pred,
    const float* surface_sem, const float* line_sem, const float* surface_obj,
    const float* line_obj, int batch, int num_proposals, int max_gt, int num_surface,
    int num_line, int num_classes, float near_threshold, float far_threshold,
    float label_surface_threshold, float label_line_threshold, float mask_surface_threshold,
    float mask_line_threshold, int64_t* cues_objectness_label, int64_t* cues_sem_label,
    int64_t* cues_matching_label, float* cues_mask, int64_t* proposal_objectness_label,
    float* proposal_objectness_mask, float* cues_match_mask, float* obj_surface_line_center,
    msmd_stream_t stream) {
  if (batch < 0 || num_proposals < 0 || max_gt < 0 || num_surface < 0 || num_line < 0 ||
      num_classes < 0)
    return MSMD_ERR_INVALID_ARG;
  const float thr[6] = {near_threshold,       far_threshold,          label_surface_threshold,
                        label_line_threshold, mask_surface_threshold, mask_line_threshold};
  for (float v : thr)
    if (v != v) return MSMD_ERR_INVALID_ARG;
  const long limit = 2147483647L;
  if (num_classes > kCueMaxClasses) return MSMD_ERR_RANGE;
  if ((long)batch * num_proposals * kCues * 3 >= limit || (long)batch * max_gt * 7 >= limit ||
      (long)batch * num_surface * 3 >= limit || (long)batch * num_line * 3 >= limit)
    return MSMD_ERR_RANGE;
  if (batch == 0 || num_proposals == 0) return MSMD_OK;
  // every sample has at least one box (the reference pads an empty one), every cue a
  // primitive to select and that primitive a class
  if (max_gt < 1 || num_surface < 1 || num_line < 1 || num_classes < 1)
    return MSMD_ERR_INVALID_ARG;
  if (!aggregated || !gt_boxes || !gt_counts || !gt_labels || !surface_pred || !line_pred ||
      !surface_sem || !line_sem || !surface_obj || !line_obj || !cues_objectness_label ||
      !cues_sem_label || !cues_matching_label || !cues_mask || !proposal_objectness_label ||
      !proposal_objectness_mask || !cues_match_mask || !obj_surface_line_center)
    return MSMD_ERR_INVALID_ARG;
  const CueThresholds t = {thr[0], thr[1], thr[2], thr[3], thr[4], thr[5]};
  const long blocks = (long)batch * ceil_div(num_proposals, kCueProposals);
  MSMD_LAUNCH(h3d_cue_targets_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
              aggregated, gt_boxes, gt_counts, gt_labels, surface_pred, line_pred, surface_sem,
              line_sem, surface_obj, line_obj, num_proposals, max_gt, num_surface, num_line,
              num_classes, t, cues_objectness_label, cues_sem_label, cues_matching_label,
              cues_mask, proposal_objectness_label, proposal_objectness_mask, cues_match_mask,
              obj_surface_line_center);
  return launch_status();
}
