// box_overlap.hpp -- rotated BEV rectangle overlap (ops/iou3d/src/iou3d_kernel.cu:36-242),
// shared by boxes.hip (the loss side: BaseInstance3DBoxes.overlaps), nms.hip (rotated NMS) and
// roi_targets.hip (Part-A2's 3-D IoU assigner, which must reproduce boxes.hip's values).
#pragma once
#include "common.hpp"

namespace msmd {
namespace bev {      // (roiaware.hip has a Box of its own)

struct Pt {
  float x, y;
};

__device__ __forceinline__ float cross3(Pt a, Pt b, Pt o) {
  return (a.x - o.x) * (b.y - o.y) - (b.x - o.x) * (a.y - o.y);
}

// crossing of segments p0-p1 and q0-q1 (strict straddle test, reference order of operands)
__device__ __forceinline__ bool edge_hit(Pt p1, Pt p0, Pt q1, Pt q0, Pt& hit) {
  if (!(fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
        fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y)))
    return false;
  const float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0);
  const float s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
  if (!(s1 * s2 > 0.f && s3 * s4 > 0.f)) return false;
  const float s5 = cross3(q1, p1, p0);
  if (fabsf(s5 - s1) > 1e-8f) {
    hit.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    hit.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
    const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
    const float d = a0 * b1 - a1 * b0;
    hit.x = (b0 * c1 - b1 * c0) / d;
    hit.y = (a1 * c0 - a0 * c1) / d;
  }
  return true;
}

struct Box {          // x1, y1, x2, y2, angle
  float v[5];
};

__device__ __forceinline__ bool inside(const Box& box, Pt p) {
  const float margin = 1e-5f;
  const float cx = (box.v[0] + box.v[2]) / 2, cy = (box.v[1] + box.v[3]) / 2;
  const float c = cosf(-box.v[4]), s = sinf(-box.v[4]);
  const float rx = (p.x - cx) * c + (p.y - cy) * s + cx;
  const float ry = -(p.x - cx) * s + (p.y - cy) * c + cy;
  return rx > box.v[0] - margin && rx < box.v[2] + margin && ry > box.v[1] - margin &&
         ry < box.v[3] + margin;
}

__device__ __forceinline__ void corners_of(const Box& box, Pt* out /* 5, closed */) {
  const float cx = (box.v[0] + box.v[2]) / 2, cy = (box.v[1] + box.v[3]) / 2;
  const float c = cosf(box.v[4]), s = sinf(box.v[4]);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float dx = ((k == 1 || k == 2) ? box.v[2] : box.v[0]) - cx;
    const float dy = (k >= 2 ? box.v[3] : box.v[1]) - cy;
    out[k].x = dx * c + dy * s + cx;
    out[k].y = -dx * s + dy * c + cy;
  }
  out[4] = out[0];
}

// Area of the intersection polygon: vertices = edge crossings, then corners of b inside
// a / corners of a inside b alternating; ordered by atan2 about their mean (a bubble sort
// in the reference: stable, so an insertion sort on the precomputed angles gives the same
// order), summed as a fan from vertex 0.
__device__ inline float overlap_bev(const Box& a, const Box& b) {
  Pt ca[5], cb[5], v[24];
  float ang[24];
  corners_of(a, ca);
  corners_of(b, cb);
  int n = 0;
  float mx = 0.f, my = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      Pt h;
      if (edge_hit(ca[i + 1], ca[i], cb[j + 1], cb[j], h)) {
        mx += h.x;
        my += h.y;
        v[n++] = h;
      }
    }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (inside(a, cb[k])) {
      mx += cb[k].x;
      my += cb[k].y;
      v[n++] = cb[k];
    }
    if (inside(b, ca[k])) {
      mx += ca[k].x;
      my += ca[k].y;
      v[n++] = ca[k];
    }
  }
  if (n < 3) return 0.f;                       // fan over < 3 vertices is empty
  mx /= n;
  my /= n;
  for (int i = 0; i < n; ++i) ang[i] = atan2f(v[i].y - my, v[i].x - mx);
  for (int i = 1; i < n; ++i) {                // stable: moves left only past strictly larger
    const Pt p = v[i];
    const float t = ang[i];
    int j = i - 1;
    while (j >= 0 && ang[j] > t) {
      v[j + 1] = v[j];
      ang[j + 1] = ang[j];
      --j;
    }
    v[j + 1] = p;
    ang[j + 1] = t;
  }
  float area = 0.f;
  for (int k = 0; k < n - 1; ++k) {
    const float ux = v[k].x - v[0].x, uy = v[k].y - v[0].y;
    const float wx = v[k + 1].x - v[0].x, wy = v[k + 1].y - v[0].y;
    area += ux * wy - uy * wx;
  }
  return (float)(fabs((double)area) / 2.0);
}

// LiDARInstance3DBoxes.bev (columns 0,1,3,4,6) -> xywhr2xyxyr
__device__ __forceinline__ Box bev_of(const float* r) {
  Box b;
  const float hw = r[3] / 2.f, hh = r[4] / 2.f;
  b.v[0] = r[0] - hw;
  b.v[1] = r[1] - hh;
  b.v[2] = r[0] + hw;
  b.v[3] = r[1] + hh;
  b.v[4] = r[6];
  return b;
}

// BaseInstance3DBoxes.overlaps of one pair of 7-column LiDAR rows (base_box3d.py:352-438): BEV
// overlap x height overlap over the union (iof: over a's volume).  The one place this is
// written: every kernel that needs the value calls this, so their results agree bit for bit.
__device__ inline float iou3d_pair(const float* ra, const float* rb, bool iof) {
  const float top = fminf(ra[2] + ra[5], rb[2] + rb[5]), bot = fmaxf(ra[2], rb[2]);
  const float oh = fmaxf(top - bot, 0.f);
  const float inter = overlap_bev(bev_of(ra), bev_of(rb)) * oh;
  const float va = ra[3] * ra[4] * ra[5], vb = rb[3] * rb[4] * rb[5];
  return iof ? inter / fmaxf(va, 1e-8f) : inter / fmaxf(va + vb - inter, 1e-8f);
}

}  // namespace bev
}  // namespace msmd
