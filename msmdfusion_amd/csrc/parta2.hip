// parta2.hip -- Part-A2's semantic and part targets (COVERAGE n9): PointwiseSemanticHead.
// get_targets / get_targets_single (models/roi_heads/mask_heads/pointwise_semantic_head.py:78-157)
// for the whole batch in one launch.
//
// The reference runs, per sample, two points_in_boxes_gpu launches and then a Python loop over
// the ground-truth boxes: a boolean mask, a host read (`k_box_flag.any()`), a gather, a rotation
// through einsum and a masked write per box, and a torch.cat at the end.  Here one lane owns one
// voxel row:
//
//   box_idx      the FIRST box of the row's sample, ascending, that holds the centre
//                (pib::pt_in_box, so bit for bit msmd_points_in_boxes_f32), else -1.
//   in_enlarged  any box of the caller's enlarged table holds the centre, same predicate.
//   seg          labels[box_idx] copied verbatim (a -1 label stays -1), num_classes when no box
//                holds the centre, and -1 when (box_idx >= 0) != in_enlarged -- the reference's
//                XOR as written: nothing assumes that an enlarged box contains its original in
//                float32.
//   part         (centre - bottom_centre[k]) turned about z by -yaw[k] in the row-vector
//                convention of rotation_3d_in_axis(axis=2) (x' = x cos + y sin, y' = -x sin +
//                y cos), divided by dims[k], plus (0.5, 0.5, 0), clamped at 0 from below
//                (torch.clamp: NaN goes through); 0 outside every box.  sin / cos of -yaw are
//                taken once, for the chosen box.
//
// Rows are ragged: a workgroup's 256 rows may belong to any samples in any order.  The workgroup
// walks the samples 0 .. batch-1, skips (one barrier) those none of its rows belongs to, and
// passes the sample's two box tables through LDS kSemGtChunk boxes at a time; a lane tests only
// the chunks of its own sample.  A row whose batch id is outside [0, batch) gets seg = -1,
// part = 0.  The box count of a sample is read on the device and clipped into [0, max_gt].
// The rows and the part targets pass through LDS so that global loads and stores are
// contiguous.  No atomics, no reduction across lanes: a lane's result depends on its own row and
// its sample's boxes only, so the output is bitwise reproducible.
#include <math.h>

#include "common.hpp"
#include "point_in_box.hpp"

namespace msmd {
namespace {

constexpr int kSemGtChunk = 64;     // boxes per LDS chunk
constexpr int kSemRows = 256;       // rows per workgroup

// grid ceil(n / 256), 256 threads
template <typename LabelT>
__global__ __launch_bounds__(kSemRows) void semantic_targets_kernel(
    const float* __restrict__ centers, const int32_t* __restrict__ batch_ids, int n,
    const float* __restrict__ gt_boxes, const float* __restrict__ enlarged,
    const LabelT* __restrict__ labels, const int32_t* __restrict__ counts, int batch, int max_gt,
    int num_classes, int64_t* __restrict__ seg_targets, float* __restrict__ part_targets) {
  __shared__ float gt[kSemGtChunk * 7];
  __shared__ float en[kSemGtChunk * 7];
  __shared__ float rows[kSemRows * 3];
  const int tid = threadIdx.x;
  const size_t first = (size_t)blockIdx.x * kSemRows;
  const int here = (int)min((size_t)kSemRows, (size_t)n - first);      // rows of this workgroup
  for (int k = tid; k < here * 3; k += kSemRows) rows[k] = centers[first * 3 + k];
  const bool live = tid < here;
  const int bid = live ? batch_ids[first + tid] : -1;
  const bool known = live && bid >= 0 && bid < batch;
  __syncthreads();
  const float px = rows[tid * 3], py = rows[tid * 3 + 1], pz = rows[tid * 3 + 2];

  int box_idx = -1;
  bool in_enlarged = false;
  for (int s = 0; s < batch; ++s) {
    const bool mine = known && bid == s;
    if (!__syncthreads_or(mine)) continue;                 // uniform over the workgroup
    const int nb = min(max(counts[s], 0), max_gt);
    const size_t table = (size_t)s * max_gt * 7;
    for (int base = 0; base < nb; base += kSemGtChunk) {
      const int cnt = min(nb - base, kSemGtChunk);
      __syncthreads();
      for (int k = tid; k < cnt * 7; k += kSemRows) {
        gt[k] = gt_boxes[table + (size_t)base * 7 + k];
        en[k] = enlarged[table + (size_t)base * 7 + k];
      }
      __syncthreads();
      if (!mine) continue;
      for (int j = 0; j < cnt; ++j) {
        float lx, ly;
        if (box_idx < 0 && pib::pt_in_box(px, py, pz, pib::load_box(gt + j * 7), lx, ly))
          box_idx = base + j;
        if (!in_enlarged && pib::pt_in_box(px, py, pz, pib::load_box(en + j * 7), lx, ly))
          in_enlarged = true;
      }
    }
  }

  float ox = 0.f, oy = 0.f, oz = 0.f;
  int64_t seg = -1;
  if (known) {
    seg = num_classes;
    if (box_idx >= 0) {
      const size_t k = (size_t)bid * max_gt + box_idx;
      seg = (int64_t)labels[k];
      const float* b = gt_boxes + k * 7;
      const float dx = __fsub_rn(px, b[0]), dy = __fsub_rn(py, b[1]), dz = __fsub_rn(pz, b[2]);
      const float angle = -b[6];
      const float sn = sinf(angle), cs = cosf(angle);
      // the einsum's three products per output column, in column order
      const float rx = __fadd_rn(__fadd_rn(__fmul_rn(dx, cs), __fmul_rn(dy, sn)),
                                 __fmul_rn(dz, 0.f));
      const float ry = __fadd_rn(__fadd_rn(__fmul_rn(dx, -sn), __fmul_rn(dy, cs)),
                                 __fmul_rn(dz, 0.f));
      const float rz = __fadd_rn(__fadd_rn(__fmul_rn(dx, 0.f), __fmul_rn(dy, 0.f)), dz);
      ox = __fadd_rn(__fdiv_rn(rx, b[3]), 0.5f);
      oy = __fadd_rn(__fdiv_rn(ry, b[4]), 0.5f);
      oz = __fadd_rn(__fdiv_rn(rz, b[5]), 0.f);
      ox = ox < 0.f ? 0.f : ox, oy = oy < 0.f ? 0.f : oy, oz = oz < 0.f ? 0.f : oz;
    }
    if ((box_idx >= 0) != in_enlarged) seg = -1;           // fg_pt_flag ^ (enlarge_box_idx > -1)
  }
  __syncthreads();                                         // every lane has read its row
  rows[tid * 3] = ox, rows[tid * 3 + 1] = oy, rows[tid * 3 + 2] = oz;
  if (live) seg_targets[first + tid] = seg;
  __syncthreads();
  for (int k = tid; k < here * 3; k += kSemRows) part_targets[first * 3 + k] = rows[k];
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_semantic_gt_chunk(void) { return kSemGtChunk; }

MSMD_EXPORT int msmd_semantic_targets_f32(
    const float* voxel_centers, const int32_t* batch_ids, const float* gt_boxes,
    const float* enlarged_boxes, const void* labels, int labels_int64, const int32_t* gt_counts,
    int num_rows, int batch, int max_gt, int num_classes, int64_t* seg_targets,
    float* part_targets, msmd_stream_t stream) {
  if (num_rows < 0 || batch < 0 || max_gt < 0 || num_classes < 1) return MSMD_ERR_INVALID_ARG;
  if (labels_int64 != 0 && labels_int64 != 1) return MSMD_ERR_INVALID_ARG;
  if ((long)batch * max_gt * 7 >= 2147483647L) return MSMD_ERR_RANGE;
  if (num_rows == 0) return MSMD_OK;
  if (!voxel_centers || !batch_ids || !seg_targets || !part_targets) return MSMD_ERR_INVALID_ARG;
  if (batch > 0 && !gt_counts) return MSMD_ERR_INVALID_ARG;
  if (batch > 0 && max_gt > 0 && (!gt_boxes || !enlarged_boxes || !labels))
    return MSMD_ERR_INVALID_ARG;
  const dim3 grid(ceil_div(num_rows, kSemRows)), block(kSemRows);
  if (labels_int64)
    MSMD_LAUNCH(semantic_targets_kernel<int64_t>, grid, block, 0, (hipStream_t)stream,
                voxel_centers, batch_ids, num_rows, gt_boxes, enlarged_boxes,
                (const int64_t*)labels, gt_counts, batch, max_gt, num_classes, seg_targets,
                part_targets);
  else
    MSMD_LAUNCH(semantic_targets_kernel<int32_t>, grid, block, 0, (hipStream_t)stream,
                voxel_centers, batch_ids, num_rows, gt_boxes, enlarged_boxes,
                (const int32_t*)labels, gt_counts, batch, max_gt, num_classes, seg_targets,
                part_targets);
  return launch_status();
}
