// free_anchor.hip -- the training loss of FreeAnchor3DHead (COVERAGE n6;
// mmdet3d/models/dense_heads/free_anchor3d_head.py:72-242).
//
//   decode_nearest_bev_kernel   DeltaXYZWLHRBBoxCoder.decode (delta_xyzwhlr_bbox_coder.py:56-91)
//                               followed by LiDARInstance3DBoxes.nearest_bev (lidar_box3d.py:93-111)
//                               of every (sample, anchor): only the five decoded members the BEV
//                               box needs (free_anchor3d_head.py:112, inside :115-116).
//   box_prob_gt_max_kernel      free_anchor3d_head.py:115-161: the reference forms the [G, A] IoU
//   box_prob_kernel             matrix of ground truths x decoded predictions per sample, its row
//                               maximum, the saturated-linear map, and goes through
//                               sparse_coo_tensor / sparse.sum / nonzero to the per-(anchor,
//                               class) maximum.  Here: the two passes of anchor.hip (integer
//                               atomicMax on the IoU's bits, then one lane per anchor with the
//                               ground truths staged through LDS).
//   topk_*_kernel               free_anchor3d_head.py:167-173: a second [G, A] matrix (ground
//                               truths x anchors) and torch.topk over each row.  Here: an exact
//                               radix select on the 32 bits of the IoU, four digits of eight bits,
//                               the IoU recomputed in every pass, then an ordered compaction.
//   negative_bag_kernel         negative_bag_loss (:266-282), summed, with its gradient.
//
// No [G, A] array exists in global memory, nothing is read back, no float atomics are used
// (the integer ones are a max and counts), so every result is bitwise reproducible.
#include "anchor_common.hpp"

namespace msmd {
namespace {

// ---------------------------------------------------------------------------- decode + BEV
__global__ __launch_bounds__(kAnchorBlock) void decode_nearest_bev_kernel(
    const float* __restrict__ anchors, const float* __restrict__ deltas, long rows, int num_anchors,
    int code, float* __restrict__ pred_bev) {
  const long row = (long)blockIdx.x * kAnchorBlock + threadIdx.x;
  if (row >= rows) return;
  const float* an = anchors + (size_t)(row % num_anchors) * code;
  const float* dl = deltas + (size_t)row * code;
  const float xa = an[0], ya = an[1], wa = an[3], la = an[4], ra = an[6];
  const float diagonal = sqrtf(la * la + wa * wa);
  const float x = dl[0] * diagonal + xa;
  const float y = dl[1] * diagonal + ya;
  const float l = expf(dl[4]) * la;
  const float w = expf(dl[3]) * wa;
  const float r = dl[6] + ra;
  // nearest_bev: the footprint (x, y, w, l), its sides exchanged when the rotation, folded to
  // [-pi/2, pi/2), is further than pi/4 from the axis
  const float pi = 3.14159274101257324f;
  const float normed = fabsf(r - floorf(r / pi + 0.5f) * pi);
  const bool swap = normed > 0.785398185253143311f;
  const float dx = swap ? l : w, dy = swap ? w : l;
  float* o = pred_bev + (size_t)row * 4;
  o[0] = x - dx / 2.f;
  o[1] = y - dy / 2.f;
  o[2] = x + dx / 2.f;
  o[3] = y + dy / 2.f;
}

// ---------------------------------------------------------------------------- box probability
// Pass one: t2_bits[i] = max over the anchors of ground truth i's sample of the bits of
// IoU(gt i, prediction).  Grid (anchor blocks, samples).
__global__ __launch_bounds__(kAnchorBlock) void box_prob_gt_max_kernel(
    const float* __restrict__ pred_bev, int num_anchors, const float* __restrict__ gt_bev,
    int num_gt, const int32_t* __restrict__ gt_offsets, uint32_t* __restrict__ t2_bits) {
  __shared__ float4 boxes[kAnchorGtChunk];
  const int b = blockIdx.y;
  int gbegin;
  const int ng = gt_list(gt_offsets, b, num_gt, gbegin);
  if (ng == 0) return;
  const int a_idx = blockIdx.x * kAnchorBlock + threadIdx.x;
  const bool live = a_idx < num_anchors;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float* p = pred_bev + ((size_t)b * num_anchors + a_idx) * 4;
    a = make_float4(p[0], p[1], p[2], p[3]);
  }
  const int lane = threadIdx.x & (kWave - 1);
  for (int c0 = 0; c0 < ng; c0 += kAnchorGtChunk) {
    const int count = min(ng - c0, kAnchorGtChunk);
    __syncthreads();
    stage_boxes(gt_bev, nullptr, num_gt, gbegin + c0, count, boxes);
    __syncthreads();
    for (int j = 0; j < count; ++j) {
      const float iou = live ? bev_iou_nan(boxes[j], a) : 0.f;
      const uint32_t bits = iou > 0.f ? __float_as_uint(iou) : 0u;   // NaN stays out
      if (__ballot(bits != 0u) == 0ull) continue;                    // uniform over the wave
      const uint32_t m = wave_max_u32(bits);
      if (lane == 0) atomicMax(&t2_bits[gbegin + c0 + j], m);
    }
  }
}

// Pass two: box_prob[row, c] = max over the sample's ground truths i of class c of
//   clamp((iou_i - t1) / (max(t2_i, t1) - t1), 0, 1),
// float32 with a true division.  The lane owns its row: it clears it, then raises single
// entries.  DEFINED BEHAVIOUR: a ground truth whose best IoU t2 does not exceed t1 contributes
// nothing.  The reference (t2.clamp(min=t1 + 1e-12), which in float32 is t1 itself) computes
// (iou - t1) / 0 there: -inf -> 0 for every iou < t1, and 0 / 0 = NaN when an IoU equals t1 bit
// for bit; outside that one case the two agree.  A NaN IoU (a NaN coordinate in either box:
// bev_iou_nan) contributes nothing and stays out of t2 -- the reference's row maximum would turn
// the whole ground truth's t2 into NaN for one NaN prediction; a label outside
// [0, C) is skipped and never written.
__global__ __launch_bounds__(kAnchorBlock) void box_prob_kernel(
    const float* __restrict__ pred_bev, int num_anchors, const float* __restrict__ gt_bev,
    const int64_t* __restrict__ gt_labels, int num_gt, const int32_t* __restrict__ gt_offsets,
    const uint32_t* __restrict__ t2_bits, float t1, int num_classes,
    float* __restrict__ box_prob) {
  __shared__ float4 boxes[kAnchorGtChunk];
  __shared__ float t2s[kAnchorGtChunk];
  __shared__ int cls[kAnchorGtChunk];
  const int b = blockIdx.y;
  int gbegin;
  const int ng = gt_list(gt_offsets, b, num_gt, gbegin);
  const int a_idx = blockIdx.x * kAnchorBlock + threadIdx.x;
  const bool live = a_idx < num_anchors;
  const size_t row = (size_t)b * num_anchors + (live ? a_idx : 0);
  float* out = box_prob + row * num_classes;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    for (int c = 0; c < num_classes; ++c) out[c] = 0.f;
    const float* p = pred_bev + row * 4;
    a = make_float4(p[0], p[1], p[2], p[3]);
  }
  for (int c0 = 0; c0 < ng; c0 += kAnchorGtChunk) {
    const int count = min(ng - c0, kAnchorGtChunk);
    __syncthreads();
    stage_boxes(gt_bev, nullptr, num_gt, gbegin + c0, count, boxes);
    for (int j = threadIdx.x; j < count; j += kAnchorBlock) {
      t2s[j] = __uint_as_float(t2_bits[gbegin + c0 + j]);
      const int64_t l = gt_labels[gbegin + c0 + j];
      cls[j] = (l >= 0 && l < (int64_t)num_classes) ? (int)l : -1;
    }
    __syncthreads();
    if (!live) continue;
    for (int j = 0; j < count; ++j) {
      const float t2 = t2s[j];
      const int c = cls[j];
      if (!(t2 > t1) || c < 0) continue;                 // uniform over the workgroup
      const float iou = bev_iou_nan(boxes[j], a);
      if (!(iou > t1)) continue;
      const float v = fminf((iou - t1) / (t2 - t1), 1.f);
      if (v > out[c]) out[c] = v;
    }
  }
}

// ---------------------------------------------------------------------------- top-k
// Key of an IoU in the order of selection: unsigned, larger key first.  NaN is the largest (as
// torch.topk has it); otherwise the usual order-preserving map of the float's bits.
constexpr uint32_t kZeroKey = 0x80000000u;     // IoU == +0: most pairs; counted implicitly
__device__ __forceinline__ uint32_t iou_key(float iou) {
  if (iou != iou) return 0xffffffffu;
  const uint32_t u = __float_as_uint(iou);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

constexpr int kTopkMax = 256;          // cap on k
constexpr int kTopkItems = 8;          // anchors per lane in a histogram pass
constexpr int kTopkHistChunk = 16;     // ground truths per workgroup in a histogram pass (16 KB)
constexpr int kTopkDigits = 4;         // 4 x 8 bits

struct TopkState {                     // per ground truth, between the passes
  uint32_t prefix;                     // the digits selected so far (after pass 4: the key T)
  int rem;                             // entries still to take among keys with that prefix
  int zeros;                           // anchors whose IoU is exactly 0
};

// One digit's histogram over the keys that carry the prefix selected so far.  Grid (anchor
// blocks of kAnchorBlock * kTopkItems, ground-truth chunks).  Pairs of IoU 0 push nothing.
__global__ __launch_bounds__(kAnchorBlock) void topk_hist_kernel(
    const float* __restrict__ anchor_bev, int num_anchors, const float* __restrict__ gt_bev,
    int num_gt, int pass, const TopkState* __restrict__ state, int* __restrict__ hist) {
  __shared__ int lh[kTopkHistChunk][256];
  __shared__ float4 boxes[kTopkHistChunk];
  __shared__ uint32_t prefix[kTopkHistChunk];
  const int g0 = blockIdx.y * kTopkHistChunk;
  const int count = min(num_gt - g0, kTopkHistChunk);
  for (int i = threadIdx.x; i < kTopkHistChunk * 256; i += kAnchorBlock) (&lh[0][0])[i] = 0;
  if ((int)threadIdx.x < count) {
    const float* p = gt_bev + (size_t)(g0 + threadIdx.x) * 4;
    boxes[threadIdx.x] = make_float4(p[0], p[1], p[2], p[3]);
    prefix[threadIdx.x] = pass ? state[g0 + threadIdx.x].prefix : 0u;
  }
  float4 a[kTopkItems];
  bool live[kTopkItems];
  const long base = (long)blockIdx.x * kAnchorBlock * kTopkItems + threadIdx.x;
#pragma unroll
  for (int u = 0; u < kTopkItems; ++u) {
    const long i = base + (long)u * kAnchorBlock;
    live[u] = i < num_anchors;
    a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live[u]) {
      const float* p = anchor_bev + (size_t)i * 4;
      a[u] = make_float4(p[0], p[1], p[2], p[3]);
    }
  }
  __syncthreads();
  const int shift = 24 - 8 * pass;
  for (int j = 0; j < count; ++j) {
    const float4 g = boxes[j];
    const uint32_t pre = prefix[j];
#pragma unroll
    for (int u = 0; u < kTopkItems; ++u) {
      if (!live[u]) continue;
      const uint32_t key = iou_key(bev_iou_nan(g, a[u]));
      if (key == kZeroKey) continue;
      if (pass && (key >> (shift + 8)) != pre) continue;
      atomicAdd(&lh[j][(key >> shift) & 255u], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < count * 256; i += kAnchorBlock) {
    const int v = (&lh[0][0])[i];
    if (v) atomicAdd(&hist[((size_t)pass * num_gt + g0) * 256 + i], v);
  }
}

// One workgroup per ground truth: the digit at which the descending count reaches rem.
__global__ __launch_bounds__(256) void topk_select_kernel(const int* __restrict__ hist, int num_gt,
                                                          int num_anchors, int k, int pass,
                                                          TopkState* __restrict__ state) {
  __shared__ int smem[256 / kWave];
  const int g = blockIdx.x;
  const int bin = 255 - (int)threadIdx.x;              // lane t holds bin 255 - t: a descending scan
  int h = hist[((size_t)pass * num_gt + g) * 256 + bin];
  uint32_t prefix = 0u;
  int rem = k, zeros, total;
  if (pass == 0) {
    (void)block_excl_scan<256>(h, smem, &total);
    zeros = num_anchors - total;
  } else {
    const TopkState s = state[g];
    prefix = s.prefix;
    rem = s.rem;
    zeros = s.zeros;
  }
  const int shift = 24 - 8 * pass;
  const bool zero_in = pass == 0 || (kZeroKey >> (shift + 8)) == prefix;
  if (zero_in && bin == (int)((kZeroKey >> shift) & 255u)) h += zeros;
  const int above = block_excl_scan<256>(h, smem, &total);
  if (above < rem && rem <= above + h) {               // exactly one lane: total >= rem >= 1
    TopkState s;
    s.prefix = (prefix << 8) | (uint32_t)bin;
    s.rem = rem - above;
    s.zeros = zeros;
    state[g] = s;
  }
}

// After the four digits state[g].prefix is the k-th largest key T and state[g].rem how many of
// the keys EQUAL to T are taken: the first ones by anchor index.  Per (ground truth, anchor
// block): how many keys are above T and how many equal it.  Grid (anchor blocks, gt chunks).
__global__ __launch_bounds__(kAnchorBlock) void topk_count_kernel(
    const float* __restrict__ anchor_bev, int num_anchors, const float* __restrict__ gt_bev,
    int num_gt, const TopkState* __restrict__ state, int stride, int* __restrict__ cnt_above,
    int* __restrict__ cnt_equal) {
  __shared__ float4 boxes[kAnchorGtChunk];
  __shared__ uint32_t thr[kAnchorGtChunk];
  __shared__ int cnt[kAnchorGtChunk][2];
  const int g0 = blockIdx.y * kAnchorGtChunk;
  const int count = min(num_gt - g0, kAnchorGtChunk);
  stage_boxes(gt_bev, nullptr, num_gt, g0, count, boxes);
  for (int j = threadIdx.x; j < count; j += kAnchorBlock) {
    thr[j] = state[g0 + j].prefix;
    cnt[j][0] = cnt[j][1] = 0;
  }
  const int i = blockIdx.x * kAnchorBlock + threadIdx.x;
  const bool live = i < num_anchors;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float* p = anchor_bev + (size_t)i * 4;
    a = make_float4(p[0], p[1], p[2], p[3]);
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  for (int j = 0; j < count; ++j) {
    const uint32_t key = iou_key(bev_iou_nan(boxes[j], a));
    const int above = __popcll(__ballot(live && key > thr[j]));
    const int equal = __popcll(__ballot(live && key == thr[j]));
    if (lane == 0) {
      if (above) atomicAdd(&cnt[j][0], above);
      if (equal) atomicAdd(&cnt[j][1], equal);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < count; j += kAnchorBlock) {
    cnt_above[(size_t)(g0 + j) * stride + blockIdx.x] = cnt[j][0];
    cnt_equal[(size_t)(g0 + j) * stride + blockIdx.x] = cnt[j][1];
  }
}

// One workgroup per ground truth, over its anchor blocks in order, in place:
//   cnt_equal[blk] -> keys equal to T in the blocks before blk
//   cnt_above[blk] -> entries selected in the blocks before blk (cnt_above[blocks] = all: k)
__global__ __launch_bounds__(256) void topk_scan_kernel(const TopkState* __restrict__ state,
                                                        int blocks, int stride,
                                                        int* __restrict__ cnt_above,
                                                        int* __restrict__ cnt_equal) {
  __shared__ int smem[256 / kWave];
  const int g = blockIdx.x;
  int* ca = cnt_above + (size_t)g * stride;
  int* ce = cnt_equal + (size_t)g * stride;
  const int need = state[g].rem;
  int run_equal = 0, run_sel = 0;
  for (int t0 = 0; t0 < blocks; t0 += 256) {
    const int i = t0 + threadIdx.x;
    const int e = i < blocks ? ce[i] : 0;
    const int ab = i < blocks ? ca[i] : 0;
    int total_e, total_s;
    const int before_e = run_equal + block_excl_scan<256>(e, smem, &total_e);
    const int sel = ab + min(max(need - before_e, 0), e);
    const int before_s = run_sel + block_excl_scan<256>(sel, smem, &total_s);
    if (i < blocks) {
      ce[i] = before_e;
      ca[i] = before_s;
    }
    run_equal += total_e;
    run_sel += total_s;
  }
  if (threadIdx.x == 0) ca[blocks] = run_sel;
}

// The ordered compaction: every key above T, and the first state[g].rem keys equal to T, written
// at their rank in anchor order.  An anchor block that holds no selected entry of a ground truth
// (almost every one) skips it.  Grid (anchor blocks, gt chunks).
__global__ __launch_bounds__(kAnchorBlock) void topk_write_kernel(
    const float* __restrict__ anchor_bev, int num_anchors, const float* __restrict__ gt_bev,
    int num_gt, const TopkState* __restrict__ state, int stride,
    const int* __restrict__ sel_before, const int* __restrict__ equal_before, int k,
    int32_t* __restrict__ matched) {
  __shared__ float4 boxes[kAnchorGtChunk];
  __shared__ uint32_t thr[kAnchorGtChunk];
  __shared__ int need[kAnchorGtChunk], sel0[kAnchorGtChunk], sel1[kAnchorGtChunk],
      eq0[kAnchorGtChunk];
  __shared__ int smem[kAnchorBlock / kWave];
  const int g0 = blockIdx.y * kAnchorGtChunk;
  const int count = min(num_gt - g0, kAnchorGtChunk);
  stage_boxes(gt_bev, nullptr, num_gt, g0, count, boxes);
  for (int j = threadIdx.x; j < count; j += kAnchorBlock) {
    const TopkState s = state[g0 + j];
    thr[j] = s.prefix;
    need[j] = s.rem;
    const size_t at = (size_t)(g0 + j) * stride + blockIdx.x;
    sel0[j] = sel_before[at];
    sel1[j] = sel_before[at + 1];
    eq0[j] = equal_before[at];
  }
  const int i = blockIdx.x * kAnchorBlock + threadIdx.x;
  const bool live = i < num_anchors;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float* p = anchor_bev + (size_t)i * 4;
    a = make_float4(p[0], p[1], p[2], p[3]);
  }
  __syncthreads();
  for (int j = 0; j < count; ++j) {
    if (sel1[j] == sel0[j]) continue;                       // uniform over the workgroup
    const uint32_t key = iou_key(bev_iou_nan(boxes[j], a));
    const int equal = live && key == thr[j];
    int total;
    const int rank_e = eq0[j] + block_excl_scan<kAnchorBlock>(equal, smem, &total);
    const int sel = live && (key > thr[j] || (equal && rank_e < need[j]));
    const int pos = sel0[j] + block_excl_scan<kAnchorBlock>(sel, smem, &total);
    if (sel && pos < k) matched[(size_t)(g0 + j) * k + pos] = i;
  }
}

struct TopkWorkspace {
  int* hist;
  TopkState* state;
  int* cnt_above;
  int* cnt_equal;
  int blocks, stride;
  template <typename A>
  void carve(A& ar, int num_anchors, int num_gt) {
    const size_t g = num_gt > 0 ? num_gt : 1;
    blocks = ceil_div(num_anchors, kAnchorBlock);
    stride = blocks + 1;
    hist = ar.template take<int>(g * kTopkDigits * 256);
    state = ar.template take<TopkState>(g);
    cnt_above = ar.template take<int>(g * stride);
    cnt_equal = ar.template take<int>(g * stride);
  }
};

// ---------------------------------------------------------------------------- negative bag loss
constexpr int kNegBlock = 256;
constexpr int kNegPerThread = 8;

// loss = (1 - alpha) p^gamma BCE(p, 0), p = clamp(sigmoid(x) (1 - q), 0, 1), BCE as torch has it:
// -max(log(1 - p), -100), backward p / max((1 - p) p, 1e-12).  1 - p is taken as
// sigmoid(-x) + sigmoid(x) q, with sigmoid(-x) from its own exponential, so that it does not
// cancel at large x.  The clamp passes the gradient on [0, 1] and stops it outside.
__global__ __launch_bounds__(kNegBlock) void negative_bag_kernel(
    const float* __restrict__ x, const float* __restrict__ q, long total, float gamma, float alpha,
    float* __restrict__ grad, double* __restrict__ partial) {
  double loss = 0;
  const long base = (long)blockIdx.x * kNegBlock * kNegPerThread;
#pragma unroll
  for (int u = 0; u < kNegPerThread; ++u) {
    const long i = base + (long)u * kNegBlock + threadIdx.x;
    if (i >= total) continue;
    const float xi = x[i], qi = q[i];
    const float e = expf(-fabsf(xi));
    const float s = xi >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);     // sigmoid(x)
    const float sm = xi >= 0.f ? e / (1.f + e) : 1.f / (1.f + e);    // sigmoid(-x)
    const float raw = s * (1.f - qi);
    const bool inside = raw >= 0.f && raw <= 1.f;
    const float p = fminf(fmaxf(raw, 0.f), 1.f);
    const float omp = inside ? fminf(fmaxf(sm + s * qi, 0.f), 1.f) : 1.f - p;
    const float bce = -fmaxf(logf(omp), -100.f);
    const float pg = pow_gamma(p, gamma);
    loss += (double)((1.f - alpha) * pg * bce);
    if (grad) {
      const float pg1 = gamma == 2.f ? p : (gamma == 1.f ? 1.f : powf(p, gamma - 1.f));
      const float dbce = p / fmaxf(omp * p, 1e-12f);
      const float dp = (1.f - alpha) * (gamma * pg1 * bce + pg * dbce);
      grad[i] = inside ? dp * (s * sm * (1.f - qi)) : 0.f;
    }
  }
  block_partial_sum<kNegBlock>(loss, partial);
}

inline long negative_blocks(int64_t n, int c) {
  const long per = (long)kNegBlock * kNegPerThread;
  return ((long)n * c + per - 1) / per;
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_decode_nearest_bev_f32(const float* anchors, int num_anchors, int code_size,
                                            const float* deltas, int batch, float* pred_bev,
                                            msmd_stream_t stream) {
  if (num_anchors < 0 || batch < 0 || code_size < 7) return MSMD_ERR_INVALID_ARG;
  const long rows = (long)batch * num_anchors;
  if (rows == 0) return MSMD_OK;
  if (!anchors || !deltas || !pred_bev) return MSMD_ERR_INVALID_ARG;
  const long blocks = (rows + kAnchorBlock - 1) / kAnchorBlock;
  if (blocks >= 2147483647L) return MSMD_ERR_RANGE;
  MSMD_LAUNCH(decode_nearest_bev_kernel, dim3((unsigned)blocks), dim3(kAnchorBlock), 0,
              (hipStream_t)stream, anchors, deltas, rows, num_anchors, code_size, pred_bev);
  return launch_status();
}

MSMD_EXPORT size_t msmd_free_anchor_box_prob_workspace_bytes(int num_gt) {
  if (num_gt < 0) return 0;
  return align_up((size_t)(num_gt > 0 ? num_gt : 1) * sizeof(uint32_t));
}

MSMD_EXPORT int msmd_free_anchor_box_prob_f32(const float* pred_bev, int batch, int num_anchors,
                                              const float* gt_bev, const int64_t* gt_labels,
                                              int num_gt, const int32_t* gt_offsets,
                                              int num_classes, float bbox_thr, float* box_prob,
                                              void* workspace, size_t workspace_bytes,
                                              msmd_stream_t stream) {
  if (batch < 0 || num_anchors < 0 || num_gt < 0 || num_classes < 1) return MSMD_ERR_INVALID_ARG;
  if (batch > 65535) return MSMD_ERR_RANGE;
  if (batch == 0 || num_anchors == 0) return MSMD_OK;
  if (!pred_bev || !box_prob || !gt_offsets) return MSMD_ERR_INVALID_ARG;
  if (num_gt > 0 && (!gt_bev || !gt_labels)) return MSMD_ERR_INVALID_ARG;
  if (!workspace || ((uintptr_t)workspace & 3) ||
      workspace_bytes < msmd_free_anchor_box_prob_workspace_bytes(num_gt))
    return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  uint32_t* t2 = (uint32_t*)workspace;
  const dim3 grid(ceil_div(num_anchors, kAnchorBlock), batch);
  if (num_gt > 0) {
    if (hipMemsetAsync(t2, 0, sizeof(uint32_t) * (size_t)num_gt, st) != hipSuccess)
      return MSMD_ERR_LAUNCH;
    MSMD_LAUNCH(box_prob_gt_max_kernel, grid, dim3(kAnchorBlock), 0, st, pred_bev, num_anchors,
                gt_bev, num_gt, gt_offsets, t2);
  }
  MSMD_LAUNCH(box_prob_kernel, grid, dim3(kAnchorBlock), 0, st, pred_bev, num_anchors, gt_bev,
              gt_labels, num_gt, gt_offsets, t2, bbox_thr, num_classes, box_prob);
  return launch_status();
}

MSMD_EXPORT int msmd_free_anchor_max_topk(void) { return kTopkMax; }

MSMD_EXPORT size_t msmd_free_anchor_topk_workspace_bytes(int num_anchors, int num_gt) {
  if (num_anchors < 0 || num_gt < 0) return 0;
  ArenaSize ar;
  TopkWorkspace w;
  w.carve(ar, num_anchors, num_gt);
  return ar.off;
}

MSMD_EXPORT int msmd_free_anchor_topk(const float* anchor_bev, int num_anchors,
                                      const float* gt_bev, int num_gt, int k, int32_t* matched,
                                      void* workspace, size_t workspace_bytes,
                                      msmd_stream_t stream) {
  if (num_anchors < 0 || num_gt < 0) return MSMD_ERR_INVALID_ARG;
  // k > num_anchors: the reference's torch.topk raises there too ("selected index k out of range")
  if (k < 1 || k > kTopkMax || k > num_anchors) return MSMD_ERR_INVALID_ARG;
  if (num_gt == 0) return MSMD_OK;
  if (!anchor_bev || !gt_bev || !matched) return MSMD_ERR_INVALID_ARG;
  if (ceil_div(num_gt, kTopkHistChunk) > 65535) return MSMD_ERR_RANGE;
  Arena ar(workspace, workspace_bytes);
  TopkWorkspace w;
  w.carve(ar, num_anchors, num_gt);
  if (!workspace || !ar.ok()) return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(w.hist, 0, sizeof(int) * (size_t)num_gt * kTopkDigits * 256, st) !=
      hipSuccess)
    return MSMD_ERR_LAUNCH;
  const dim3 hist_grid(ceil_div(num_anchors, kAnchorBlock * kTopkItems),
                       ceil_div(num_gt, kTopkHistChunk));
  for (int pass = 0; pass < kTopkDigits; ++pass) {
    MSMD_LAUNCH(topk_hist_kernel, hist_grid, dim3(kAnchorBlock), 0, st, anchor_bev, num_anchors,
                gt_bev, num_gt, pass, w.state, w.hist);
    MSMD_LAUNCH(topk_select_kernel, dim3(num_gt), dim3(256), 0, st, w.hist, num_gt, num_anchors, k,
                pass, w.state);
  }
  const dim3 grid(w.blocks, ceil_div(num_gt, kAnchorGtChunk));
  MSMD_LAUNCH(topk_count_kernel, grid, dim3(kAnchorBlock), 0, st, anchor_bev, num_anchors, gt_bev,
              num_gt, w.state, w.stride, w.cnt_above, w.cnt_equal);
  MSMD_LAUNCH(topk_scan_kernel, dim3(num_gt), dim3(256), 0, st, w.state, w.blocks, w.stride,
              w.cnt_above, w.cnt_equal);
  MSMD_LAUNCH(topk_write_kernel, grid, dim3(kAnchorBlock), 0, st, anchor_bev, num_anchors, gt_bev,
              num_gt, w.state, w.stride, w.cnt_above, w.cnt_equal, k, matched);
  return launch_status();
}

MSMD_EXPORT size_t msmd_free_anchor_negative_workspace_bytes(int64_t n, int num_classes) {
  if (n < 0 || num_classes < 1) return 0;
  const long blocks = negative_blocks(n, num_classes);
  return align_up((size_t)(blocks > 0 ? blocks : 1) * sizeof(double));
}

MSMD_EXPORT int msmd_free_anchor_negative_f32(const float* logits, const float* box_prob,
                                              int64_t n, int num_classes, float gamma,
                                              float alpha, float* grad, float* sum,
                                              void* workspace, size_t workspace_bytes,
                                              msmd_stream_t stream) {
  // gamma < 1: d p^gamma / dp is unbounded at p = 0, where most entries are
  if (n < 0 || num_classes < 1 || !sum || !(gamma >= 1.f)) return MSMD_ERR_INVALID_ARG;
  if (n > 0 && (!logits || !box_prob)) return MSMD_ERR_INVALID_ARG;
  const long blocks = negative_blocks(n, num_classes);
  if (blocks >= 2147483647L) return MSMD_ERR_RANGE;
  if (!workspace || ((uintptr_t)workspace & 7) ||
      workspace_bytes < msmd_free_anchor_negative_workspace_bytes(n, num_classes))
    return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (blocks > 0)
    MSMD_LAUNCH(negative_bag_kernel, dim3((unsigned)blocks), dim3(kNegBlock), 0, st, logits,
                box_prob, (long)n * num_classes, gamma, alpha, grad, (double*)workspace);
  MSMD_LAUNCH(partials_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace,
              (int)blocks, sum);
  return launch_status();
}
