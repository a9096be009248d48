// nms.hip -- the iou3d op family's suppression side (COVERAGE n2): rotated, axis-aligned and
// circle NMS, batched over segments, with the greedy reduction on the device; and the
// class-aware axis-aligned 3-D NMS of the VoteNet family (COVERAGE n4) and mmcv's `nms` pair
// test for 3DSSD's batched_nms (COVERAGE n5) on the same two kernels.
//
//   nms_mask_kernel    ops/iou3d/src/iou3d_kernel.cu nms_kernel / nms_normal_kernel (:283-419)
//                      and the pair test of core/post_processing/box3d_nms.py:158-181
//                      (circle_nms): one wavefront per (segment, 64x64 tile on or above the
//                      diagonal), column boxes staged in LDS, one 64-bit word per row.
//   nms_reduce_kernel  the host loop of ops/iou3d/src/iou3d.cpp:100-150 (nms_gpu) made
//                      device-side: one wavefront per segment walks the rows 64 at a time with
//                      the "removed" bitset in LDS.
//   boxes_iou_bev      iou3d_kernel.cu boxes_iou_bev_kernel (:269-281).
//   hit_aligned3d      the pair test of core/post_processing/box3d_nms.py:91-138
//                      (aligned_3d_nms, a Python while loop with one host read per kept box).
//   hit_mmcv           mmcv 1.x ops/csrc/nms_cuda_kernel.cuh devIoU with offset = 0, the pair test
//                      behind mmcv.ops.batched_nms (ssd_3d_head.py:512-515, one call per sample).
//
// A segment is one (task, sample) list of boxes, sorted by descending score by the caller and
// addressed through a CSR offsets array that stays on the device.  The host only knows an
// upper bound on a segment's length (`max_segment`, the caller's pre-NMS cut): rows past it
// are not part of the segment.  The reference launches per task and per sample, copies the
// N x N / 64 mask to the host and reduces it there; circle NMS is a numba double loop on the
// host.  Here every segment is handled by two launches and nothing is read back.
#include "box_overlap.hpp"

namespace msmd {
namespace {

using namespace bev;

constexpr int kNmsTile = 64;                 // rows / columns per tile = bits per mask word
constexpr int kNmsMaxSegment = 16384;        // removed bitset: 256 words = 2 KB of LDS
constexpr int kNmsMaxWords = kNmsMaxSegment / kNmsTile;

enum { kRotated = 0, kNormal = 1, kCircle = 2, kAligned3d = 3, kMmcv = 4 };

// iou3d_kernel.cu:244-251
__device__ __forceinline__ float iou_bev(const Box& a, const Box& b) {
  const float sa = (a.v[2] - a.v[0]) * (a.v[3] - a.v[1]);
  const float sb = (b.v[2] - b.v[0]) * (b.v[3] - b.v[1]);
  const float s = overlap_bev(a, b);
  return s / fmaxf(sa + sb - s, 1e-8f);
}

// iou3d_kernel.cu:333-343
__device__ __forceinline__ float iou_normal(const float* a, const float* b) {
  const float left = fmaxf(a[0], b[0]), right = fminf(a[2], b[2]);
  const float top = fmaxf(a[1], b[1]), bottom = fminf(a[3], b[3]);
  const float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
  const float inter = width * height;
  const float sa = (a[2] - a[0]) * (a[3] - a[1]);
  const float sb = (b[2] - b[0]) * (b[3] - b[1]);
  return inter / fmaxf(sa + sb - inter, 1e-8f);
}

// box3d_nms.py:176  dist = (x1[i] - x1[j])**2 + (y1[i] - y1[j])**2 on float32 scalars: two
// rounded squares and one rounded sum, never a fused multiply-add.
__device__ __forceinline__ bool circle_hit(const float* kept, const float* later, float thresh) {
  const float dx = __fsub_rn(kept[0], later[0]), dy = __fsub_rn(kept[1], later[1]);
  const float dist = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
  return dist <= thresh;
}

// box3d_nms.py:119-135 on rows (x1, y1, z1, x2, y2, z2, class): the kept row suppresses the later
// one unless iou * same <= thresh, as the reference's `score_sorted[iou <= thresh]` keeps it.
// A NaN IoU (0 / 0: two zero-volume boxes that do not intersect) therefore suppresses, and in
// any class, because NaN * 0 is NaN.  Every product, sum and the quotient rounded on its own.
__device__ __forceinline__ float volume3d(const float* b) {
  return __fmul_rn(__fmul_rn(__fsub_rn(b[3], b[0]), __fsub_rn(b[4], b[1])), __fsub_rn(b[5], b[2]));
}
__device__ __forceinline__ bool hit_aligned3d(const float* kept, const float* later, float thresh) {
  const float l = fmaxf(0.f, __fsub_rn(fminf(kept[3], later[3]), fmaxf(kept[0], later[0])));
  const float w = fmaxf(0.f, __fsub_rn(fminf(kept[4], later[4]), fmaxf(kept[1], later[1])));
  const float h = fmaxf(0.f, __fsub_rn(fminf(kept[5], later[5]), fmaxf(kept[2], later[2])));
  const float inter = __fmul_rn(__fmul_rn(l, w), h);
  const float iou =
      __fdiv_rn(inter, __fsub_rn(__fadd_rn(volume3d(kept), volume3d(later)), inter));
  const float same = kept[6] == later[6] ? 1.f : 0.f;
  return !(__fmul_rn(iou, same) <= thresh);
}

// mmcv devIoU, offset 0, on rows (x1, y1, x2, y2) the caller has already shifted by class: the
// multiply form `inter > thr * (area_i + area_j - inter)`.  Unlike iou_normal there is no
// division and no 1e-8 floor, so two zero-area boxes give 0 > 0: no suppression.
__device__ __forceinline__ bool hit_mmcv(const float* kept, const float* later, float thresh) {
  const float left = fmaxf(kept[0], later[0]), right = fminf(kept[2], later[2]);
  const float top = fmaxf(kept[1], later[1]), bottom = fminf(kept[3], later[3]);
  const float width = fmaxf(__fsub_rn(right, left), 0.f);
  const float height = fmaxf(__fsub_rn(bottom, top), 0.f);
  const float inter = __fmul_rn(width, height);
  const float sa = __fmul_rn(__fsub_rn(kept[2], kept[0]), __fsub_rn(kept[3], kept[1]));
  const float sb = __fmul_rn(__fsub_rn(later[2], later[0]), __fsub_rn(later[3], later[1]));
  return inter > __fmul_rn(thresh, __fsub_rn(__fadd_rn(sa, sb), inter));
}

// The length of segment s as the kernels see it: clipped to the caller's bound and to the
// rows that exist, so a bad offsets array cannot send an access out of `boxes` or `mask`.
__device__ __forceinline__ int segment_rows(const int32_t* __restrict__ offsets, int s,
                                            int total, int max_segment, int& begin) {
  begin = offsets[s];
  const int end = offsets[s + 1];
  if (begin < 0 || begin > total) return 0;
  int n = min(end, total) - begin;
  n = min(n, max_segment);
  return n > 0 ? n : 0;
}

// grid (col tile, row tile, segment), 64 threads.  mask[(begin + row) * words + col tile],
// `words` = ceil(max_segment / 64); only tiles with col tile >= row tile are written.
template <int KIND>
__global__ __launch_bounds__(kNmsTile) void nms_mask_kernel(
    const float* __restrict__ boxes, int ld, const int32_t* __restrict__ offsets, int total,
    int max_segment, const float* __restrict__ thresh, int words,
    unsigned long long* __restrict__ mask) {
  constexpr int kCols =
      KIND == kAligned3d ? 7 : (KIND == kCircle ? 2 : (KIND == kNormal || KIND == kMmcv ? 4 : 5));
  const int ct = blockIdx.x, rt = blockIdx.y, s = blockIdx.z;
  if (ct < rt) return;
  int begin;
  const int n = segment_rows(offsets, s, total, max_segment, begin);
  if (ct * kNmsTile >= n) return;
  const int col_size = min(n - ct * kNmsTile, kNmsTile);
  const int row_size = min(n - rt * kNmsTile, kNmsTile);
  const int lane = threadIdx.x;

  __shared__ float cols[kNmsTile * kCols];
  if (lane < col_size) {
    const float* src = boxes + (size_t)(begin + ct * kNmsTile + lane) * ld;
#pragma unroll
    for (int k = 0; k < kCols; ++k) cols[lane * kCols + k] = src[k];
  }
  __syncthreads();
  if (lane >= row_size) return;

  const int row = rt * kNmsTile + lane;
  const float* src = boxes + (size_t)(begin + row) * ld;
  float mine[kCols];
#pragma unroll
  for (int k = 0; k < kCols; ++k) mine[k] = src[k];
  const float th = thresh[s];
  unsigned long long bits = 0;
  for (int i = (rt == ct ? lane + 1 : 0); i < col_size; ++i) {
    bool hit;
    if (KIND == kAligned3d) {
      hit = hit_aligned3d(mine, cols + i * kCols, th);
    } else if (KIND == kMmcv) {
      hit = hit_mmcv(mine, cols + i * kCols, th);
    } else if (KIND == kCircle) {
      hit = circle_hit(mine, cols + i * kCols, th);
    } else if (KIND == kNormal) {
      hit = iou_normal(mine, cols + i * kCols) > th;
    } else {
      Box a, b;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        a.v[k] = mine[k];
        b.v[k] = cols[i * kCols + k];
      }
      hit = iou_bev(a, b) > th;
    }
    if (hit) bits |= 1ull << i;
  }
  mask[(size_t)(begin + row) * words + ct] = bits;
}

__device__ __forceinline__ unsigned long long wave_or(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, kWave);
  return v;
}

// One wavefront per segment.  Chunk c = rows [64c, 64c + 64): lane = row.  The diagonal word of
// every row resolves the chunk itself (64 uniform steps on registers); the kept rows then OR
// their words of the later column tiles into the bitset.  keep[s * keep_stride + p] = the p-th
// kept row (its position in the segment, or order[begin + position] when `order` is given),
// -1 past num_keep[s].
__global__ __launch_bounds__(kWave) void nms_reduce_kernel(
    const unsigned long long* __restrict__ mask, const int32_t* __restrict__ offsets, int total,
    int max_segment, int words, int post_max, const int64_t* __restrict__ order,
    int64_t* __restrict__ keep, int keep_stride, int32_t* __restrict__ num_keep) {
  __shared__ unsigned long long removed[kNmsMaxWords];
  const int s = blockIdx.x, lane = threadIdx.x;
  int begin;
  const int n = segment_rows(offsets, s, total, max_segment, begin);
  const int chunks = (n + kNmsTile - 1) / kNmsTile;
  for (int j = lane; j < chunks; j += kWave) removed[j] = 0;
  __syncthreads();
  const int limit = min(post_max, keep_stride);
  int64_t* out = keep + (size_t)s * keep_stride;
  int count = 0;
  for (int c = 0; c < chunks && count < limit; ++c) {
    const int row = c * kNmsTile + lane;
    const bool live = row < n;
    const unsigned long long* mine = mask + (size_t)(begin + (live ? row : 0)) * words;
    const unsigned long long diag = live ? mine[c] : 0ull;
    const int rows_here = min(n - c * kNmsTile, kNmsTile);
    unsigned long long rem = removed[c];
    if (rows_here < kNmsTile) rem |= ~0ull << rows_here;
    for (int b = 0; b < rows_here; ++b) {
      const unsigned long long d = __shfl(diag, b, kWave);
      if (!((rem >> b) & 1ull)) rem |= d;
    }
    const unsigned long long kept = ~rem;
    const bool is_kept = (kept >> lane) & 1ull;
    for (int j = c + 1; j < chunks; ++j) {
      const unsigned long long w = wave_or(is_kept ? mine[j] : 0ull);
      if (lane == 0) removed[j] |= w;
    }
    if (is_kept) {
      const int p = count + __popcll(kept & ((1ull << lane) - 1ull));
      if (p < limit) out[p] = order ? order[begin + row] : (int64_t)row;
    }
    count += __popcll(kept);
    __syncthreads();
  }
  count = min(count, limit);
  for (int p = count + lane; p < keep_stride; p += kWave) out[p] = -1;
  if (lane == 0) num_keep[s] = count;
}

__global__ __launch_bounds__(256) void boxes_iou_bev_kernel(const float* __restrict__ a, int na,
                                                            const float* __restrict__ b, int nb,
                                                            float* __restrict__ out) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)na * nb) return;
  Box ba, bb;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    ba.v[k] = a[(t / nb) * 5 + k];
    bb.v[k] = b[(t % nb) * 5 + k];
  }
  out[t] = iou_bev(ba, bb);
}

// The two launches of every NMS entry point, after its validation.
int nms_launch(int kind, const float* boxes, int ld, const int32_t* offsets, int num_segments,
               int total_boxes, int max_segment, const float* thresh, int post_max,
               const int64_t* order, int64_t* keep, int keep_stride, int32_t* num_keep,
               void* workspace, msmd_stream_t stream) {
  const int bound = max_segment < total_boxes ? max_segment : total_boxes;
  const int words = ceil_div(max_segment, kNmsTile);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* mask = (unsigned long long*)workspace;
  const int tiles = ceil_div(bound, kNmsTile);
  if (tiles > 0) {
    const dim3 grid(tiles, tiles, num_segments), block(kNmsTile);
    if (kind == kRotated)
      MSMD_LAUNCH(nms_mask_kernel<kRotated>, grid, block, 0, st, boxes, ld, offsets, total_boxes,
                  bound, thresh, words, mask);
    else if (kind == kNormal)
      MSMD_LAUNCH(nms_mask_kernel<kNormal>, grid, block, 0, st, boxes, ld, offsets, total_boxes,
                  bound, thresh, words, mask);
    else if (kind == kAligned3d)
      MSMD_LAUNCH(nms_mask_kernel<kAligned3d>, grid, block, 0, st, boxes, ld, offsets, total_boxes,
                  bound, thresh, words, mask);
    else if (kind == kMmcv)
      MSMD_LAUNCH(nms_mask_kernel<kMmcv>, grid, block, 0, st, boxes, ld, offsets, total_boxes,
                  bound, thresh, words, mask);
    else
      MSMD_LAUNCH(nms_mask_kernel<kCircle>, grid, block, 0, st, boxes, ld, offsets, total_boxes,
                  bound, thresh, words, mask);
  }
  MSMD_LAUNCH(nms_reduce_kernel, dim3(num_segments), dim3(kWave), 0, st, mask, offsets,
              total_boxes, bound, words, post_max, order, keep, keep_stride, num_keep);
  return launch_status();
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_boxes_iou_bev_f32(const float* boxes_a, int na, const float* boxes_b, int nb,
                                       float* out, msmd_stream_t stream) {
  if (na < 0 || nb < 0) return MSMD_ERR_INVALID_ARG;
  if ((long)na * nb == 0) return MSMD_OK;
  if ((long)na * nb >= 2147483647L) return MSMD_ERR_RANGE;
  if (!boxes_a || !boxes_b || !out) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(boxes_iou_bev_kernel, dim3(ceil_div((long)na * nb, 256)), dim3(256), 0,
              (hipStream_t)stream, boxes_a, na, boxes_b, nb, out);
  return launch_status();
}

MSMD_EXPORT size_t msmd_nms_workspace_bytes(int total_boxes, int max_segment) {
  if (total_boxes < 0 || max_segment < 0 || max_segment > kNmsMaxSegment) return 0;
  const size_t words = (size_t)ceil_div(max_segment, kNmsTile);
  return align_up((size_t)total_boxes * words * sizeof(unsigned long long));
}

MSMD_EXPORT int msmd_nms_batched_f32(int kind, const float* boxes, int ld, const int32_t* offsets,
                                     int num_segments, int total_boxes, int max_segment,
                                     const float* thresh, int post_max, const int64_t* order,
                                     int64_t* keep, int keep_stride, int32_t* num_keep,
                                     void* workspace, size_t workspace_bytes,
                                     msmd_stream_t stream) {
  if (kind < kRotated || kind > kCircle) return MSMD_ERR_INVALID_ARG;
  if (num_segments < 0 || total_boxes < 0 || max_segment < 0 || post_max < 0 || keep_stride < 0)
    return MSMD_ERR_INVALID_ARG;
  if (max_segment > kNmsMaxSegment) return MSMD_ERR_INVALID_ARG;
  if (ld < (kind == kCircle ? 2 : (kind == kNormal ? 4 : 5))) return MSMD_ERR_INVALID_ARG;
  if (num_segments > 65535) return MSMD_ERR_RANGE;
  if (num_segments == 0) return MSMD_OK;
  if (!offsets || !thresh || !num_keep || (keep_stride > 0 && !keep)) return MSMD_ERR_INVALID_ARG;
  if (total_boxes > 0 && !boxes) return MSMD_ERR_INVALID_ARG;
  const int bound = max_segment < total_boxes ? max_segment : total_boxes;
  if (bound > 0 && (!workspace || ((uintptr_t)workspace & 7) ||
                    workspace_bytes < msmd_nms_workspace_bytes(total_boxes, max_segment)))
    return MSMD_ERR_WORKSPACE;
  return nms_launch(kind, boxes, ld, offsets, num_segments, total_boxes, max_segment, thresh,
                    post_max, order, keep, keep_stride, num_keep, workspace, stream);
}

MSMD_EXPORT size_t msmd_nms_aligned3d_workspace_bytes(int total_boxes, int max_segment) {
  return msmd_nms_workspace_bytes(total_boxes, max_segment);
}

MSMD_EXPORT int msmd_nms_aligned3d_f32(const float* boxes, int ld, const int32_t* offsets,
                                       int num_segments, int total_boxes, int max_segment,
                                       const float* thresh, int post_max, const int64_t* order,
                                       int64_t* keep, int keep_stride, int32_t* num_keep,
                                       void* workspace, size_t workspace_bytes,
                                       msmd_stream_t stream) {
  if (num_segments < 0 || total_boxes < 0 || max_segment < 0 || post_max < 0 || keep_stride < 0)
    return MSMD_ERR_INVALID_ARG;
  if (max_segment > kNmsMaxSegment || ld < 7) return MSMD_ERR_INVALID_ARG;
  if (num_segments > 65535) return MSMD_ERR_RANGE;
  if (num_segments == 0) return MSMD_OK;
  if (!offsets || !thresh || !num_keep || (keep_stride > 0 && !keep)) return MSMD_ERR_INVALID_ARG;
  if (total_boxes > 0 && !boxes) return MSMD_ERR_INVALID_ARG;
  const int bound = max_segment < total_boxes ? max_segment : total_boxes;
  if (bound > 0 && (!workspace || ((uintptr_t)workspace & 7) ||
                    workspace_bytes < msmd_nms_workspace_bytes(total_boxes, max_segment)))
    return MSMD_ERR_WORKSPACE;
  return nms_launch(kAligned3d, boxes, ld, offsets, num_segments, total_boxes, max_segment,
                    thresh, post_max, order, keep, keep_stride, num_keep, workspace, stream);
}

MSMD_EXPORT int msmd_nms_mmcv_f32(const float* boxes, int ld, const int32_t* offsets,
                                  int num_segments, int total_boxes, int max_segment,
                                  const float* thresh, int post_max, const int64_t* order,
                                  int64_t* keep, int keep_stride, int32_t* num_keep,
                                  void* workspace, size_t workspace_bytes, msmd_stream_t stream) {
  if (num_segments < 0 || total_boxes < 0 || max_segment < 0 || post_max < 0 || keep_stride < 0)
    return MSMD_ERR_INVALID_ARG;
  if (max_segment > kNmsMaxSegment || ld < 4) return MSMD_ERR_INVALID_ARG;
  if (num_segments > 65535) return MSMD_ERR_RANGE;
  if (num_segments == 0) return MSMD_OK;
  if (!offsets || !thresh || !num_keep || (keep_stride > 0 && !keep)) return MSMD_ERR_INVALID_ARG;
  if (total_boxes > 0 && !boxes) return MSMD_ERR_INVALID_ARG;
  const int bound = max_segment < total_boxes ? max_segment : total_boxes;
  if (bound > 0 && (!workspace || ((uintptr_t)workspace & 7) ||
                    workspace_bytes < msmd_nms_workspace_bytes(total_boxes, max_segment)))
    return MSMD_ERR_WORKSPACE;
  return nms_launch(kMmcv, boxes, ld, offsets, num_segments, total_boxes, max_segment, thresh,
                    post_max, order, keep, keep_stride, num_keep, workspace, stream);
}
