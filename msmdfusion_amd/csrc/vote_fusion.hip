// vote_fusion.hip -- ImVoteNet's VoteFusion (COVERAGE p4): the image votes of every seed of
// every sample in one launch (mmdet3d/models/fusion_layers/vote_fusion.py:40-212).
//
// The reference loops over the samples; per sample it builds [seed_num, bbox_num, 5 + classes]
// tensors (and a dozen temporaries of that shape) with about sixty launches and keeps, by a
// topk over the box axis, max_imvote_per_pixel (seed, box) pairs per seed.  Here one lane owns
// one (sample, seed):
//
//   project     cam = m_cam [x y z 1] (the reversed 3-D flow and DEPTH -> CAM with Rt, composed on
//               the host), (u, v) = (K cam).xy / (K cam).z, uv_origin = rint(u - 1), half to even.
//   select      the sample's boxes pass through LDS kVoteBoxChunk at a time, un-rescaled at
//               staging with bbox_2d_transform(ori2new=False)'s float32 operations in its order
//               (flip, minus crop, divide by scale: bit-identical edges).  in_box is the strict
//               l < u < r && t < v < b; score = float(in_box) + conf.  The lane keeps the K largest
//               (score, box) pairs in registers, descending, EQUAL SCORES TO THE LOWER BOX INDEX
//               (torch.topk leaves that order open), by an insertion that is unrolled over the
//               template's K: no runtime-indexed array, nothing in scratch.  A list shorter than
//               K is filled with score 0 pairs, as the reference appends zeros.
//   cues        for the K chosen boxes only (their rows are read again and un-rescaled by the
//               same operations): delta = (box centre - uv) * z_cam / fx lifted by m_vote (CAM ->
//               DEPTH with Rt, then the forward flow INCLUDING its translation, as the reference
//               applies the whole flow to an offset), ray = normalised seed + vote, xz; conf at
//               the class row; everything times float(in_box).  mask = floor(score) != 0, from
//               the formula: an out-of-box pair with conf == 1 is valid with zero cues.
//   texture     the image at rint(coord_2d_transform(uv_origin, ori2new=True)) / 255 (a true
//               division), the same value in all K slots.
//   empty list  zero cues, mask 1 in slot 0 and 0 elsewhere (the reference's bbox_num == 0
//               branch), decided here: every lane of the sample sees the same count.
//
// Slot k of seed s is column k * S + s, so every (channel, slot) store runs along the seed
// axis and is contiguous across the wave.  No [S, Nb] array exists, no atomics, nothing is read
// back, and a lane's result depends on its own inputs only.
//
// Deviations from the reference: a pixel outside img_shape (or outside the padded image), or
// one that is not finite, gives a zero texture cue and is not read (the reference's gather
// asserts on the device, or wraps into a neighbouring row where the flat index stays in
// range); a class outside [0, num_classes) contributes no semantic cue (the reference's scatter
// faults); the image is never written (the reference's `img_flatten /= 255.` can write through
// a view into the caller's image).
#include <math.h>

#include "common.hpp"

namespace msmd {
namespace {

constexpr int kVoteBoxChunk = 64;   // boxes per LDS chunk
constexpr int kVoteMaxK = 8;        // max_imvote_per_pixel of the fused path

struct Box2D {
  float l, t, r, b, conf;
};

// bbox_2d_transform(ori2new=False) on one row, coord_transform.py:156-170
__device__ __forceinline__ Box2D unrescale(const float* __restrict__ row,
                                           const msmd_vote_fusion_params& p) {
  float l = row[0], t = row[1], r = row[2], b = row[3];
  if (p.flip != 0.f) {
    const float nr = __fsub_rn(p.img_w, l), nl = __fsub_rn(p.img_w, r);
    l = nl, r = nr;
  }
  l = __fsub_rn(l, p.crop_x), r = __fsub_rn(r, p.crop_x);
  t = __fsub_rn(t, p.crop_y), b = __fsub_rn(b, p.crop_y);
  Box2D o;
  o.l = __fdiv_rn(l, p.scale_x), o.r = __fdiv_rn(r, p.scale_x);
  o.t = __fdiv_rn(t, p.scale_y), o.b = __fdiv_rn(b, p.scale_y);
  o.conf = row[4];
  return o;
}

__device__ __forceinline__ bool in_box(const Box2D& q, float u, float v) {
  return u > q.l && u < q.r && v > q.t && v < q.b;
}

__device__ __forceinline__ float dot4(const float* m, float x, float y, float z) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)),
                             __fmul_rn(m[2], z)), m[3]);
}
__device__ __forceinline__ float dot3(const float* m, float x, float y, float z) {
  return __fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z));
}

// grid (ceil(S / 256), batch), 256 threads
template <int KK>
__global__ __launch_bounds__(256) void vote_fusion_kernel(
    const float* __restrict__ seeds, int num_seeds, const float* __restrict__ boxes,
    const int32_t* __restrict__ box_offsets, int total_boxes, const float* __restrict__ imgs,
    int pad_h, int pad_w, const msmd_vote_fusion_params* __restrict__ params, int num_classes,
    float* __restrict__ feat, uint8_t* __restrict__ mask) {
  __shared__ float sl[kVoteBoxChunk], st[kVoteBoxChunk], sr[kVoteBoxChunk], sb[kVoteBoxChunk],
      sc[kVoteBoxChunk];
  const int s = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < num_seeds;
  const msmd_vote_fusion_params p = params[s];
  int b_begin = box_offsets[s];
  int nb = 0;
  if (b_begin >= 0 && b_begin <= total_boxes) {
    nb = min(box_offsets[s + 1], total_boxes) - b_begin;
    nb = nb > 0 ? nb : 0;
  }
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    const float* q = seeds + ((size_t)s * num_seeds + i) * 3;
    x = q[0], y = q[1], z = q[2];
  }
  // vote_fusion.py:52-64
  const float cx = dot4(p.m_cam, x, y, z), cy = dot4(p.m_cam + 4, x, y, z),
              cz = dot4(p.m_cam + 8, x, y, z);
  const float w = dot3(p.k + 6, cx, cy, cz);
  const float u = rintf(__fsub_rn(__fdiv_rn(dot3(p.k, cx, cy, cz), w), 1.f));
  const float v = rintf(__fsub_rn(__fdiv_rn(dot3(p.k + 3, cx, cy, cz), w), 1.f));

  // :174-181, the K best pairs.  -1: one of the zeros appended to a short list
  float score[KK];
  int idx[KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) score[k] = 0.f, idx[k] = -1;
  for (int base = 0; base < nb; base += kVoteBoxChunk) {
    const int cnt = min(nb - base, kVoteBoxChunk);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      const Box2D q = unrescale(boxes + (size_t)(b_begin + base + threadIdx.x) * 6, p);
      sl[threadIdx.x] = q.l, st[threadIdx.x] = q.t, sr[threadIdx.x] = q.r, sb[threadIdx.x] = q.b;
      sc[threadIdx.x] = q.conf;
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const bool inb = u > sl[j] && u < sr[j] && v > st[j] && v < sb[j];
      float cs = __fadd_rn(inb ? 1.f : 0.f, sc[j]);
      if (!(cs > score[KK - 1])) continue;
      int ci = base + j;
      bool ins = false;
#pragma unroll
      for (int k = 0; k < KK; ++k) {      // once placed, the rest moves down one slot
        ins = ins || cs > score[k];
        const float ts = score[k];
        const int ti = idx[k];
        score[k] = ins ? cs : ts, idx[k] = ins ? ci : ti;
        cs = ins ? ts : cs, ci = ins ? ti : ci;
      }
    }
  }
  if (!live) return;

  const size_t cols = (size_t)KK * num_seeds;
  float* o = feat + (size_t)s * (5 + num_classes + 3) * cols + i;
  uint8_t* om = mask + (size_t)s * cols + i;
#pragma unroll
  for (int k = 0; k < KK; ++k) {
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f, g4 = 0.f, sem = 0.f;
    int cls = -1;
    if (idx[k] >= 0) {
      const float* row = boxes + (size_t)(b_begin + idx[k]) * 6;
      const Box2D q = unrescale(row, p);
      const float inb = in_box(q, u, v) ? 1.f : 0.f;
      // :94-95, 110-120
      const float midx = __fdiv_rn(__fadd_rn(q.l, q.r), 2.f);
      const float midy = __fdiv_rn(__fadd_rn(q.t, q.b), 2.f);
      const float du = __fdiv_rn(__fmul_rn(__fsub_rn(midx, u), cz), p.fx);
      const float dv = __fdiv_rn(__fmul_rn(__fsub_rn(midy, v), cz), p.fx);
      // :127-142
      float r0 = __fadd_rn(x, dot4(p.m_vote, du, dv, 0.f));
      float r1 = __fadd_rn(y, dot4(p.m_vote + 4, du, dv, 0.f));
      float r2 = __fadd_rn(z, dot4(p.m_vote + 8, du, dv, 0.f));
      const float norm = __fsqrt_rn(__fadd_rn(
          __fadd_rn(__fadd_rn(__fmul_rn(r0, r0), __fmul_rn(r1, r1)), __fmul_rn(r2, r2)), 1e-6f));
      r0 = __fdiv_rn(r0, norm), r1 = __fdiv_rn(r1, norm), r2 = __fdiv_rn(r2, norm);
      // :145-146
      const float den = __fadd_rn(r1, 1e-6f);
      g0 = __fmul_rn(__fsub_rn(__fmul_rn(__fdiv_rn(r0, den), y), x), inb);
      g1 = __fmul_rn(__fsub_rn(__fmul_rn(__fdiv_rn(r2, den), y), z), inb);
      g2 = __fmul_rn(r0, inb), g3 = __fmul_rn(r1, inb), g4 = __fmul_rn(r2, inb);
      sem = __fmul_rn(q.conf, inb);
      const float c = truncf(row[5]);     // .long()
      if (c >= 0.f && c < (float)num_classes) cls = (int)c;
    }
    float* ok = o + (size_t)k * num_seeds;
    ok[0] = g0, ok[cols] = g1, ok[2 * cols] = g2, ok[3 * cols] = g3, ok[4 * cols] = g4;
    for (int c = 0; c < num_classes; ++c) ok[(size_t)(5 + c) * cols] = c == cls ? sem : 0.f;
    // :71-81 / :190-191
    om[(size_t)k * num_seeds] = nb == 0 ? (k == 0) : (floorf(score[k]) != 0.f);
  }

  // :193-205; coord_2d_transform(ori2new=True), coord_transform.py:193-203
  float rx = __fadd_rn(__fmul_rn(u, p.scale_x), p.crop_x);
  const float ry = rintf(__fadd_rn(__fmul_rn(v, p.scale_y), p.crop_y));
  if (p.flip != 0.f) rx = __fsub_rn(p.img_w, rx);
  rx = rintf(rx);
  const float wlim = fminf(p.img_w, (float)pad_w), hlim = fminf(p.img_h, (float)pad_h);
  float tex[3] = {0.f, 0.f, 0.f};
  if (rx >= 0.f && rx < wlim && ry >= 0.f && ry < hlim) {      // (false for NaN)
    const float* px = imgs + ((size_t)s * 3 * pad_h + (int)ry) * pad_w + (int)rx;
#pragma unroll
    for (int c = 0; c < 3; ++c) tex[c] = __fdiv_rn(px[(size_t)c * pad_h * pad_w], 255.f);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < KK; ++k)
      o[(size_t)(5 + num_classes + c) * cols + (size_t)k * num_seeds] = tex[c];
}

template <int KK>
void launch(int num_seeds, int batch, hipStream_t stream, const float* seeds, const float* boxes,
            const int32_t* box_offsets, int total_boxes, const float* imgs, int pad_h, int pad_w,
            const msmd_vote_fusion_params* params, int num_classes, float* feat, uint8_t* mask) {
  MSMD_LAUNCH(vote_fusion_kernel<KK>, dim3(ceil_div(num_seeds, 256), batch), dim3(256), 0, stream,
              seeds, num_seeds, boxes, box_offsets, total_boxes, imgs, pad_h, pad_w, params,
              num_classes, feat, mask);
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_vote_fusion_max_k(void) { return kVoteMaxK; }

MSMD_EXPORT int msmd_vote_fusion_f32(
    const float* seeds, int batch, int num_seeds, const float* boxes, int total_boxes,
    const int32_t* box_offsets, const int32_t* box_offsets_host, const float* imgs, int pad_h,
    int pad_w, const msmd_vote_fusion_params* params, int num_classes, int max_imvote,
    float* feat, uint8_t* mask, msmd_stream_t stream) {
  if (batch < 0 || num_seeds < 0 || total_boxes < 0 || pad_h < 0 || pad_w < 0)
    return MSMD_ERR_INVALID_ARG;
  if (num_classes < 1 || max_imvote < 1 || max_imvote > kVoteMaxK) return MSMD_ERR_INVALID_ARG;
  if (batch > 0) {
    if (!box_offsets_host || box_offsets_host[0] != 0 || box_offsets_host[batch] != total_boxes)
      return MSMD_ERR_INVALID_ARG;
    for (int b = 0; b < batch; ++b)
      if (box_offsets_host[b + 1] < box_offsets_host[b]) return MSMD_ERR_INVALID_ARG;
  }
  if (batch > 65535) return MSMD_ERR_RANGE;
  if ((long)batch * (5 + num_classes + 3) * max_imvote * num_seeds >= 2147483647L ||
      (long)batch * 3 * pad_h * pad_w >= 2147483647L)
    return MSMD_ERR_RANGE;
  if (batch == 0 || num_seeds == 0) return MSMD_OK;
  if (!seeds || !box_offsets || !params || !feat || !mask) return MSMD_ERR_INVALID_ARG;
  if (total_boxes > 0 && !boxes) return MSMD_ERR_INVALID_ARG;
  if (pad_h > 0 && pad_w > 0 && !imgs) return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
#define MSMD_VOTE_CASE(k)                                                                      \
  case k:                                                                                      \
    launch<k>(num_seeds, batch, st, seeds, boxes, box_offsets, total_boxes, imgs, pad_h, pad_w, \
              params, num_classes, feat, mask);                                                \
    break;
  switch (max_imvote) {
    MSMD_VOTE_CASE(1) MSMD_VOTE_CASE(2) MSMD_VOTE_CASE(3) MSMD_VOTE_CASE(4)
    MSMD_VOTE_CASE(5) MSMD_VOTE_CASE(6) MSMD_VOTE_CASE(7) MSMD_VOTE_CASE(8)
  }
#undef MSMD_VOTE_CASE
  return launch_status();
}
