// ssd3d.hip -- 3DSSD's candidate targets (COVERAGE n5): SSD3DHead.get_targets_single and
// _assign_targets_by_points_inside (models/dense_heads/ssd_3d_head.py:307-437, 545-572) for the
// whole batch in one launch.
//
// The reference runs, per sample, a Python function of about sixty small tensor ops with two
// points_in_boxes_gpu launches, a data-dependent gt[valid] compaction and a host read
// (`if valid_gt.sum() == 0`).  Here one lane owns one (sample, candidate).  What depends on a
// box alone -- the coder's encode, the corners, sin / cos of -yaw, the enlarged table -- is
// computed once by the caller over the batch's concatenated boxes (torch, element-wise, so
// every value gathered here is the reference's bit for bit); the kernel does what depends on
// the candidate:
//
//   assignment   the first box of the sample, ascending, whose label is not -1 and that holds the
//                aggregated point (points_in_boxes_gpu's `break` over gt[valid]); when none does,
//                the sample's LAST valid box (`assignment[assignment == num_bbox] = num_bbox - 1`
//                after the compaction, so rows labelled -1 are skipped).
//   gathers      centre, half sizes, label, direction class / residual, corners of that box.
//   masks        positive = inside && |p - (centre + (0, 0, half_z))| < pos_distance_thr,
//                negative = !inside.
//   centerness   :385-414 as written, float32, one rounding per operation.  A candidate outside
//                every box still computes it against its fallback box (almost always 0); NaN
//                goes where the expressions send it (torch.clamp / min / max propagate NaN, and
//                NaN * 0 of the one-hot product is NaN in every class column).
//   vote         the same two assignment rules with the enlarged boxes on the seed point:
//                vote_mask, vote_target = gravity centre (of the original box) - seed.
//   empty scene  a sample without a valid row: zeros everywhere, negative = 1 (:340-360),
//                decided here -- every lane of the sample sees the same count.
//
// The sample's boxes pass through LDS kSsdGtChunk at a time (both 7-float rows and a validity
// flag); the per-box table is read once per candidate, at the row it was assigned.  No atomics,
// no reduction across lanes: a lane's result depends on its own inputs only.
#include <math.h>

#include "common.hpp"
#include "point_in_box.hpp"

namespace msmd {
namespace {

constexpr int kSsdGtChunk = 64;     // boxes per LDS chunk
constexpr int kSsdTable = 33;       // per-box floats, see msmd_hip.h

// torch.clamp(v, min=0) / torch.min / torch.max on tensors: NaN goes through
__device__ __forceinline__ float clamp_min0(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ float nan_min(float a, float b) {
  return (a != a || b != b) ? NAN : fminf(a, b);
}
__device__ __forceinline__ float nan_max(float a, float b) {
  return (a != a || b != b) ? NAN : fmaxf(a, b);
}
__device__ __forceinline__ float ratio(float a, float b) {
  return __fdiv_rn(nan_min(a, b), nan_max(a, b));
}

__device__ __forceinline__ int sample_boxes(const int32_t* __restrict__ offsets, int s, int total,
                                            int& begin) {
  begin = offsets[s];
  const int end = offsets[s + 1];
  if (begin < 0 || begin > total) return 0;
  const int n = min(end, total) - begin;
  return n > 0 ? n : 0;
}

// grid (ceil(n / 256), batch), 256 threads
__global__ __launch_bounds__(256) void ssd3d_targets_kernel(
    const float* __restrict__ aggregated, const float* __restrict__ seeds, long seed_stride, int n,
    const float* __restrict__ gt_boxes, const float* __restrict__ vote_boxes,
    const int64_t* __restrict__ labels, const int32_t* __restrict__ box_offsets, int total_boxes,
    const float* __restrict__ table, const int64_t* __restrict__ dir_class, int num_classes,
    float thr, float* __restrict__ vote_targets, float* __restrict__ center_targets,
    float* __restrict__ size_targets, int64_t* __restrict__ dir_class_targets,
    float* __restrict__ dir_res_targets, int64_t* __restrict__ mask_targets,
    float* __restrict__ centerness, float* __restrict__ corners, uint8_t* __restrict__ vote_mask,
    uint8_t* __restrict__ positive, uint8_t* __restrict__ negative) {
  __shared__ float gt[kSsdGtChunk * 7];
  __shared__ float vb[kSsdGtChunk * 7];
  __shared__ int valid[kSsdGtChunk];
  const int s = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  int b_begin;
  const int nb = sample_boxes(box_offsets, s, total_boxes, b_begin);
  const size_t row = (size_t)s * n + (live ? i : 0);
  float px = 0.f, py = 0.f, pz = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
  if (live) {
    const float* p = aggregated + row * 3;
    px = p[0], py = p[1], pz = p[2];
    const float* q = seeds + (size_t)s * seed_stride + (size_t)i * 3;
    qx = q[0], qy = q[1], qz = q[2];
  }
  int assigned = -1, voted = -1, last_valid = -1;     // rows within the sample
  for (int base = 0; base < nb; base += kSsdGtChunk) {
    const int cnt = min(nb - base, kSsdGtChunk);
    __syncthreads();
    for (int k = threadIdx.x; k < cnt * 7; k += 256) {
      gt[k] = gt_boxes[(size_t)(b_begin + base) * 7 + k];
      vb[k] = vote_boxes[(size_t)(b_begin + base) * 7 + k];
    }
    for (int k = threadIdx.x; k < cnt; k += 256) valid[k] = labels[b_begin + base + k] != -1;
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      if (!valid[j]) continue;
      last_valid = base + j;
      float lx, ly;
      if (assigned < 0 && pib::pt_in_box(px, py, pz, pib::load_box(gt + j * 7), lx, ly))
        assigned = base + j;
      if (voted < 0 && pib::pt_in_box(qx, qy, qz, pib::load_box(vb + j * 7), lx, ly))
        voted = base + j;
    }
  }
  if (!live) return;

  float* o_vote = vote_targets + row * 3;
  float* o_center = center_targets + row * 3;
  float* o_size = size_targets + row * 3;
  float* o_cness = centerness + row * num_classes;
  float* o_corner = corners + row * 24;
  if (last_valid < 0) {                                // the empty-scene branch
    for (int k = 0; k < 3; ++k) o_vote[k] = 0.f, o_center[k] = 0.f, o_size[k] = 0.f;
    for (int k = 0; k < num_classes; ++k) o_cness[k] = 0.f;
    for (int k = 0; k < 24; ++k) o_corner[k] = 0.f;
    dir_class_targets[row] = 0, dir_res_targets[row] = 0.f, mask_targets[row] = 0;
    vote_mask[row] = 0, positive[row] = 0, negative[row] = 1;
    return;
  }
  const bool inside = assigned >= 0;
  const int a = b_begin + (inside ? assigned : last_valid);
  const float* t = table + (size_t)a * kSsdTable;
  const float cx = t[0], cy = t[1], cz = t[2], hx = t[3], hy = t[4], hz = t[5];
  const int64_t label = labels[a];
  o_center[0] = cx, o_center[1] = cy, o_center[2] = cz;
  o_size[0] = hx, o_size[1] = hy, o_size[2] = hz;
  dir_class_targets[row] = dir_class[a];
  dir_res_targets[row] = t[6];
  mask_targets[row] = label;
  for (int k = 0; k < 24; ++k) o_corner[k] = t[9 + k];

  // :377-382
  const float dx = __fsub_rn(px, cx), dy = __fsub_rn(py, cy);
  const float tz = __fsub_rn(pz, __fadd_rn(cz, hz));
  const float dist = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)),
                                     __fmul_rn(tz, tz)));
  positive[row] = inside && dist < thr;
  negative[row] = !inside;

  // :385-414.  rotation_3d_in_axis(canonical, -yaw, 2): x' = x cos + y sin, y' = -x sin + y cos
  // with the box's stored sin / cos of -yaw
  const float sn = t[7], cs = t[8];
  const float dz = __fsub_rn(pz, cz);
  const float rx = __fadd_rn(__fmul_rn(dx, cs), __fmul_rn(dy, sn));
  const float ry = __fadd_rn(__fmul_rn(dx, -sn), __fmul_rn(dy, cs));
  const float front = clamp_min0(__fsub_rn(hx, rx)), back = clamp_min0(__fadd_rn(hx, rx));
  const float left = clamp_min0(__fsub_rn(hy, ry)), right = clamp_min0(__fadd_rn(hy, ry));
  const float top = clamp_min0(__fsub_rn(hz, dz)), bottom = clamp_min0(__fadd_rn(hz, dz));
  float c = __fmul_rn(__fmul_rn(ratio(front, back), ratio(left, right)), ratio(bottom, top));
  c = cbrtf(clamp_min0(c));
  c = c < 0.f ? 0.f : (c > 1.f ? 1.f : c);
  for (int k = 0; k < num_classes; ++k) o_cness[k] = __fmul_rn(c, k == label ? 1.f : 0.f);

  // :423-432
  const bool in_vote = voted >= 0;
  const float* g = table + (size_t)(b_begin + (in_vote ? voted : last_valid)) * kSsdTable;
  o_vote[0] = __fsub_rn(g[0], qx), o_vote[1] = __fsub_rn(g[1], qy), o_vote[2] = __fsub_rn(g[2], qz);
  vote_mask[row] = in_vote;
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_ssd3d_gt_chunk(void) { return kSsdGtChunk; }

MSMD_EXPORT int msmd_ssd3d_targets_f32(
    const float* aggregated, const float* seeds, int64_t seed_stride, const float* gt_boxes,
    const float* vote_boxes, const int64_t* labels, const int32_t* box_offsets,
    const float* box_table, int table_width, const int64_t* dir_class, int batch,
    int num_candidates, int total_boxes, int num_classes, float pos_distance_thr,
    float* vote_targets, float* center_targets, float* size_targets, int64_t* dir_class_targets,
    float* dir_res_targets, int64_t* mask_targets, float* centerness, float* corners,
    uint8_t* vote_mask, uint8_t* positive_mask, uint8_t* negative_mask, msmd_stream_t stream) {
  if (batch < 0 || num_candidates < 0 || total_boxes < 0 || num_classes < 1)
    return MSMD_ERR_INVALID_ARG;
  if (table_width != kSsdTable) return MSMD_ERR_INVALID_ARG;
  if (seed_stride < (int64_t)num_candidates * 3) return MSMD_ERR_INVALID_ARG;
  if (!(pos_distance_thr == pos_distance_thr)) return MSMD_ERR_INVALID_ARG;
  if (batch > 65535) return MSMD_ERR_RANGE;
  if ((long)batch * num_candidates * (num_classes > 24 ? num_classes : 24) >= 2147483647L)
    return MSMD_ERR_RANGE;
  if (batch == 0 || num_candidates == 0) return MSMD_OK;
  if (!aggregated || !seeds || !box_offsets || !vote_targets || !center_targets ||
      !size_targets || !dir_class_targets || !dir_res_targets || !mask_targets || !centerness ||
      !corners || !vote_mask || !positive_mask || !negative_mask)
    return MSMD_ERR_INVALID_ARG;
  if (total_boxes > 0 && (!gt_boxes || !vote_boxes || !labels || !box_table || !dir_class))
    return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(ssd3d_targets_kernel, dim3(ceil_div(num_candidates, 256), batch), dim3(256), 0,
              (hipStream_t)stream, aggregated, seeds, (long)seed_stride, num_candidates, gt_boxes,
              vote_boxes, labels, box_offsets, total_boxes, box_table, dir_class, num_classes,
              pos_distance_thr, vote_targets, center_targets, size_targets, dir_class_targets,
              dir_res_targets, mask_targets, centerness, corners, vote_mask, positive_mask,
              negative_mask);
  return launch_status();
}
