// point_in_box.hpp -- the point-in-box predicate shared by roiaware.hip (RoI-aware pooling,
// points_in_boxes) and vote.hip (vote targets, points per box): one definition, so every
// caller agrees with msmd_points_in_boxes_f32 bit for bit.
#pragma once
#include <math.h>

#include "common.hpp"

namespace msmd {
namespace pib {

struct Box {
  float cx, cy, zb, w, l, h, rz;
};
__device__ __forceinline__ Box load_box(const float* __restrict__ b) {
  return Box{b[0], b[1], b[2], b[3], b[4], b[5], b[6]};
}

// check_pt_in_box3d + lidar_to_local_coords, the reference's float/double mix
__device__ __forceinline__ bool pt_in_box(float x, float y, float z, const Box& b, float& lx,
                                          float& ly) {
  const float cz = (float)((double)b.zb + (double)b.h / 2.0);
  if ((double)fabsf(z - cz) > (double)b.h / 2.0) return false;
  const float rot = (float)((double)b.rz + M_PI / 2);
  const float ca = cosf(rot), sa = sinf(rot);
  const float sx = x - b.cx, sy = y - b.cy;
  lx = sx * ca + sy * (-sa);
  ly = sx * sa + sy * ca;
  const double hl = (double)b.l / 2.0, hw = (double)b.w / 2.0;
  return (double)lx > -hl && (double)lx < hl && (double)ly > -hw && (double)ly < hw;
}

}  // namespace pib
}  // namespace msmd
