// boxes.hip -- the box / heat-map arithmetic under TransFusionHead.loss.
//
//   boxes_iou3d       BaseInstance3DBoxes.overlaps (core/bbox/structures/base_box3d.py:352-438):
//                     rotated BEV overlap (ops/iou3d/src/iou3d_kernel.cu:36-264) x height
//                     overlap / volumes, for every sample of the batch in ONE launch (the
//                     reference launches per sample and per decoder layer and copies the
//                     BEV boxes twice on the way).
//   heatmap_gaussian  the per-box python loop of get_targets_single
//                     (models/dense_heads/transfusion_head.py:1186-1210 ->
//                     core/utils/gaussian.py:5-53): all boxes of all samples in one launch.
//   gaussian_focal    clip_sigmoid + GaussianFocalLoss (transfusion_head.py:1247-1249):
//                     value, gradient and the positive count in one pass over the map
//                     (the reference: ~15 elementwise launches + .item()).
// All three are tiny (20k box pairs, a few hundred bumps, 650k map cells): what counts
// is the launch count and the absent host round trips, not a roofline.
#include "box_overlap.hpp"

namespace msmd {
namespace {

using namespace bev;

// mode 0: IoU, 1: IoF (over boxes a), 2: BEV overlap area of 5-column xyxyr boxes
__global__ __launch_bounds__(256) void boxes_iou3d_kernel(
    const float* __restrict__ a, int lda, const float* __restrict__ b, int ldb,
    const int32_t* __restrict__ nb_valid, int batch, int na, int nb, int mode,
    float* __restrict__ out) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)batch * na * nb) return;
  const int j = (int)(t % nb);
  const long ij = t / nb;
  const int i = (int)(ij % na), s = (int)(ij / na);
  if (nb_valid && j >= nb_valid[s]) {
    out[t] = 0.f;
    return;
  }
  const float* ra = a + ((size_t)s * na + i) * lda;
  const float* rb = b + ((size_t)s * nb + j) * ldb;
  if (mode == 2) {
    Box ba, bb;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      ba.v[k] = ra[k];
      bb.v[k] = rb[k];
    }
    out[t] = overlap_bev(ba, bb);
    return;
  }
  out[t] = iou3d_pair(ra, rb, mode == 1);
}

// one workgroup per box: heat[plane] = max(heat[plane], bump clipped to the map)
__global__ __launch_bounds__(256) void heatmap_gaussian_kernel(
    const int32_t* __restrict__ plane, const int32_t* __restrict__ cx,
    const int32_t* __restrict__ cy, const int32_t* __restrict__ radius, int planes, int h,
    int w, float* __restrict__ heat) {
  const int g = blockIdx.x;
  const int pl = plane[g], r = radius[g];
  if (pl < 0 || pl >= planes || r < 0) return;
  const int x0 = cx[g], y0 = cy[g];
  const int d = 2 * r + 1;
  const double sigma = (double)d / 6.0;
  const double denom = 2 * sigma * sigma;
  const double tiny = 2.220446049250313e-16;     // np.finfo(float64).eps * h.max(), max = 1
  for (int e = threadIdx.x; e < d * d; e += 256) {
    const int dy = e / d - r, dx = e % d - r;
    const int x = x0 + dx, y = y0 + dy;
    if (x < 0 || x >= w || y < 0 || y >= h) continue;
    double v = exp(-(double)(dx * dx + dy * dy) / denom);
    if (v < tiny) v = 0;
    // values are >= 0: their bit patterns order like the floats
    atomicMax((int*)(heat + ((size_t)pl * h + y) * w + x), __float_as_int((float)v));
  }
}

constexpr int kFocalBlock = 256;
constexpr int kFocalPerThread = 8;

// p = clamp(sigmoid(x), clip, 1 - clip);  loss = -log(p + e) (1 - p)^2 [t == 1]
//                                               - log(1 - p + e) p^2 (1 - t)^4
__global__ __launch_bounds__(kFocalBlock) void gaussian_focal_kernel(
    const float* __restrict__ x, const float* __restrict__ target, long n, float clip,
    float* __restrict__ grad /* d loss_i / d x_i, or null */, double* __restrict__ partial
    /* [blocks][2]: loss sum, positives */) {
  const float e = 1e-12f;
  double loss = 0, pos = 0;
  const long base = (long)blockIdx.x * kFocalBlock * kFocalPerThread;
#pragma unroll
  for (int u = 0; u < kFocalPerThread; ++u) {
    const long i = base + (long)u * kFocalBlock + threadIdx.x;
    if (i >= n) continue;
    const float xi = x[i], t = target[i];
    const float sg = 1.f / (1.f + expf(-xi));
    const float p = fminf(fmaxf(sg, clip), 1.f - clip);
    const bool live = sg >= clip && sg <= 1.f - clip;          // clamp passes the gradient
    const float q = 1.f - p;
    const float nw = (1.f - t) * (1.f - t) * (1.f - t) * (1.f - t);
    const float lp = logf(p + e), lq = logf(q + e);
    const bool is_pos = t == 1.f;
    const float li = (is_pos ? -lp * q * q : 0.f) + -lq * p * p * nw;
    loss += (double)li;
    pos += is_pos ? 1.0 : 0.0;
    if (grad) {
      float dp = nw * (p * p / (q + e) - 2.f * p * lq);
      if (is_pos) dp += -(q * q) / (p + e) + 2.f * q * lp;
      grad[i] = live ? dp * sg * (1.f - sg) : 0.f;
    }
  }
  __shared__ double sh[2][kFocalBlock / kWave];
  for (int off = kWave / 2; off > 0; off >>= 1) {
    loss += __shfl_down(loss, off, kWave);
    pos += __shfl_down(pos, off, kWave);
  }
  const int wave = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) {
    sh[0][wave] = loss;
    sh[1][wave] = pos;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double l = 0, c = 0;
    for (int k = 0; k < kFocalBlock / kWave; ++k) {
      l += sh[0][k];
      c += sh[1][k];
    }
    partial[(size_t)blockIdx.x * 2] = l;
    partial[(size_t)blockIdx.x * 2 + 1] = c;
  }
}

// fixed-order sum of the block partials (deterministic) -> out[0] = loss sum, out[1] = positives
__global__ __launch_bounds__(256) void focal_finish_kernel(const double* __restrict__ partial,
                                                           int blocks, float* __restrict__ out) {
  __shared__ double sh[2][256];
  double l = 0, c = 0;
  for (int b = threadIdx.x; b < blocks; b += 256) {
    l += partial[(size_t)b * 2];
    c += partial[(size_t)b * 2 + 1];
  }
  sh[0][threadIdx.x] = l;
  sh[1][threadIdx.x] = c;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)sh[0][0];
    out[1] = (float)sh[1][0];
  }
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_boxes_overlap_bev_f32(const float* boxes_a, int na, const float* boxes_b,
                                           int nb, float* out, msmd_stream_t stream) {
  if (na < 0 || nb < 0) return MSMD_ERR_INVALID_ARG;
  if ((long)na * nb == 0) return MSMD_OK;
  if (!boxes_a || !boxes_b || !out) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(boxes_iou3d_kernel, dim3(ceil_div((long)na * nb, 256)), dim3(256), 0,
              (hipStream_t)stream, boxes_a, 5, boxes_b, 5, (const int32_t*)nullptr, 1, na, nb, 2,
              out);
  return launch_status();
}

MSMD_EXPORT int msmd_boxes_iou3d_f32(const float* boxes_a, int lda, const float* boxes_b, int ldb,
                                     const int32_t* nb_valid, int batch, int na, int nb, int mode,
                                     float* out, msmd_stream_t stream) {
  if (batch < 0 || na < 0 || nb < 0 || lda < 7 || ldb < 7 || (mode != 0 && mode != 1))
    return MSMD_ERR_INVALID_ARG;
  const long total = (long)batch * na * nb;
  if (total == 0) return MSMD_OK;
  if (total >= 2147483647L) return MSMD_ERR_RANGE;
  if (!boxes_a || !boxes_b || !out) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(boxes_iou3d_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
              boxes_a, lda, boxes_b, ldb, nb_valid, batch, na, nb, mode, out);
  return launch_status();
}

MSMD_EXPORT int msmd_heatmap_gaussian_f32(const int32_t* plane, const int32_t* center_x,
                                          const int32_t* center_y, const int32_t* radius, int n,
                                          int planes, int h, int w, float* heatmap,
                                          msmd_stream_t stream) {
  if (n < 0 || planes < 1 || h < 1 || w < 1 || !heatmap) return MSMD_ERR_INVALID_ARG;
  if (n == 0) return MSMD_OK;
  if (!plane || !center_x || !center_y || !radius) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(heatmap_gaussian_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, plane,
              center_x, center_y, radius, planes, h, w, heatmap);
  return launch_status();
}

MSMD_EXPORT size_t msmd_gaussian_focal_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  const long blocks = (n + kFocalBlock * kFocalPerThread - 1) / (kFocalBlock * kFocalPerThread);
  return align_up((size_t)(blocks > 0 ? blocks : 1) * 2 * sizeof(double));
}

MSMD_EXPORT int msmd_gaussian_focal_f32(const float* logits, const float* target, int64_t n,
                                        float clip, float* grad, float* sums, void* workspace,
                                        size_t workspace_bytes, msmd_stream_t stream) {
  if (n < 0 || !sums || !(clip >= 0.f && clip < 0.5f)) return MSMD_ERR_INVALID_ARG;
  if (n > 0 && (!logits || !target)) return MSMD_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < msmd_gaussian_focal_workspace_bytes(n))
    return MSMD_ERR_WORKSPACE;
  const int blocks = ceil_div(n, (long)kFocalBlock * kFocalPerThread);
  hipStream_t st = (hipStream_t)stream;
  if (blocks > 0)
    MSMD_LAUNCH(gaussian_focal_kernel, dim3(blocks), dim3(kFocalBlock), 0, st, logits, target,
                (long)n, clip, grad, (double*)workspace);
  MSMD_LAUNCH(focal_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, blocks,
              sums);
  return launch_status();
}
