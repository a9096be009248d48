// primitive.hip -- H3DNet primitive targets (PrimitiveHead.get_targets_single) of a whole batch.
//
// The reference walks the instances of every sample on the host: a nonzero, a unique, six
// point-to-plane matches, up to twelve point-to-line matches and about fourteen
// `if tensor.sum() > n and tensor.var() < t` reads per instance, once per head.  Here:
//
//   msmd_primitive_index   (mode independent, shared by the three heads of a step)
//     1. label presence: one bit per (sample, instance label) of the foreground points,
//        atomicOr into a per-sample bitmap (the result does not depend on the order);
//     2. rank = popcount of the lower bits, so ranks follow ascending labels (torch.unique);
//        per (sample, rank): the point count and the lowest foreground point (atomicAdd /
//        atomicMin on integers: order independent);
//     3. one workgroup per (sample, rank) compacts the instance's points in ascending point
//        order with a block scan -- no sort is needed, the sweep is O(N) per instance and runs
//        once per step, not once per head.
//   msmd_primitive_targets_f32   (one launch per mode)
//     one workgroup per (sample, rank) makes three sweeps over that instance's list in steps
//     of kPointChunk: (1) plane minima, (2) counts, variance moments and coordinate sums,
//     (3) decisions and writes.  Each lane evaluates its own point's primitives in the
//     reference's write order, so the last writer wins without atomics or races.  Further
//     workgroups of the same launch zero the rows of background points and of instances
//     without a box.
//
// Every float32 operation of the plane equations and distances is rounded on its own (the
// library is built with -ffp-contract=off and a correctly rounded divide and sqrt).
#include "common.hpp"

namespace msmd {
namespace {

constexpr int kMaxLabels = 1024;   // label_bound limit: 32 bitmap words per sample
constexpr int kPointChunk = 256;   // list entries per sweep step (= block size)
constexpr int kBlock = 256;

enum { kModeZ = 0, kModeXY = 1, kModeLine = 2 };

__device__ __forceinline__ int seg_rows(const int32_t* __restrict__ offsets, int s, int total,
                                        int& begin) {
  begin = offsets[s];
  const int end = offsets[s + 1];
  if (begin < 0 || begin > total) { begin = 0; return 0; }
  const int n = min(end, total) - begin;
  return n > 0 ? n : 0;
}

// The index: all int32, strides fixed by (num_samples, total_points, label_bound).
struct Index {
  uint32_t* bitmap;   // [S, words]
  int32_t* count;     // [S, label_bound]   points of rank r
  int32_t* ninst;     // [S]
  int32_t* first;     // [S, label_bound]   lowest foreground point of rank r (sample relative)
  int32_t* start;     // [S, label_bound]   list start of rank r (sample relative)
  int32_t* rank;      // [total_points]     rank of the point's instance, -1: takes no part
  int32_t* order;     // [total_points]     the lists, sample s at its point offset
  size_t zero_bytes;  // bitmap .. ninst are contiguous and start at zero
};
template <typename A>
Index carve(A& a, int samples, int total_points, int label_bound) {
  Index x;
  const int words = (label_bound + 31) / 32;
  x.bitmap = a.template take<uint32_t>((size_t)samples * words);
  x.count = a.template take<int32_t>((size_t)samples * label_bound);
  x.ninst = a.template take<int32_t>(samples);
  x.zero_bytes = a.off;
  x.first = a.template take<int32_t>((size_t)samples * label_bound);
  x.start = a.template take<int32_t>((size_t)samples * label_bound);
  x.rank = a.template take<int32_t>(total_points);
  x.order = a.template take<int32_t>(total_points);
  return x;
}

__global__ __launch_bounds__(kBlock) void prim_bitmap_kernel(
    const int64_t* __restrict__ sem, const int64_t* __restrict__ inst,
    const int32_t* __restrict__ point_offsets, int total_points, int num_classes,
    int label_bound, uint32_t* __restrict__ bitmap) {
  const int s = blockIdx.y, words = (label_bound + 31) / 32;
  int begin;
  const int np = seg_rows(point_offsets, s, total_points, begin);
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < np; i += gridDim.x * kBlock) {
    const int64_t label = inst[begin + i];
    if (sem[begin + i] == num_classes || label < 0 || label >= label_bound) continue;
    atomicOr(&bitmap[(size_t)s * words + (int)(label >> 5)], 1u << (label & 31));
  }
}

__global__ __launch_bounds__(kBlock) void prim_rank_kernel(
    const int64_t* __restrict__ sem, const int64_t* __restrict__ inst,
    const int32_t* __restrict__ point_offsets, int total_points, int num_classes,
    int label_bound, const uint32_t* __restrict__ bitmap, int32_t* __restrict__ count,
    int32_t* __restrict__ first, int32_t* __restrict__ ninst, int32_t* __restrict__ rank) {
  __shared__ uint32_t bits[kMaxLabels / 32];
  __shared__ int base[kMaxLabels / 32];
  const int s = blockIdx.y, words = (label_bound + 31) / 32;
  if (threadIdx.x < words) bits[threadIdx.x] = bitmap[(size_t)s * words + threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int w = 0; w < words; ++w) base[w] = run, run += __popc(bits[w]);
    if (blockIdx.x == 0) ninst[s] = run;
  }
  __syncthreads();
  int begin;
  const int np = seg_rows(point_offsets, s, total_points, begin);
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < np; i += gridDim.x * kBlock) {
    const int64_t label = inst[begin + i];
    int r = -1;
    if (sem[begin + i] != num_classes && label >= 0 && label < label_bound) {
      const int w = (int)(label >> 5), b = (int)(label & 31);
      r = base[w] + __popc(bits[w] & ((1u << b) - 1u));
      atomicAdd(&count[(size_t)s * label_bound + r], 1);
      atomicMin(&first[(size_t)s * label_bound + r], i);
    }
    rank[begin + i] = r;
  }
}

// grid (rank slot, sample): the block's instances in ascending point order
__global__ __launch_bounds__(kBlock) void prim_list_kernel(
    const int32_t* __restrict__ point_offsets, int total_points, int label_bound,
    const int32_t* __restrict__ count, const int32_t* __restrict__ ninst,
    const int32_t* __restrict__ rank, int32_t* __restrict__ start, int32_t* __restrict__ order) {
  __shared__ int smem[kBlock / kWave];
  const int s = blockIdx.y;
  int begin;
  const int np = seg_rows(point_offsets, s, total_points, begin);
  const int n = min(ninst[s], label_bound);
  const int32_t* cnt = count + (size_t)s * label_bound;
  for (int r = blockIdx.x; r < n; r += gridDim.x) {
    int below = 0;
    for (int q = threadIdx.x; q < r; q += kBlock) below += cnt[q];
    int lo;
    block_excl_scan<kBlock>(below, smem, &lo);
    const int want = cnt[r];
    if (threadIdx.x == 0) start[(size_t)s * label_bound + r] = lo;
    int done = 0;
    for (int i0 = 0; i0 < np && done < want; i0 += kBlock) {
      const int i = i0 + threadIdx.x;
      const int hit = (i < np && rank[begin + i] == r) ? 1 : 0;
      int tot;
      const int ex = block_excl_scan<kBlock>(hit, smem, &tot);
      const int at = lo + done + ex;
      if (hit && at < np) order[begin + at] = i;
      done += tot;
    }
  }
}

// ---------------------------------------------------------------------------------------------

struct Cfg {
  float dist_thresh, var_thresh, lower_thresh, line_thresh;
  int num_point, num_point_line, with_yaw;
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return (ax * bx + ay * by) + az * bz;
}

// the four planes of a mode as (nx, ny, nz, d); false: the reference raises for this box
struct Planes {
  float p[4][4];
};
__device__ bool side_planes(const float* c, int a0, int a1, int b0, int b1, int on, const int* far,
                            float lower, float* near_p, float* far_p) {
  // normal = (c[a0] - c[a1]) x (c[b0] - c[b1]) through c[on], normalised; the far plane has
  // the same normal through the mean of four corners
  const float ux = c[a0 * 3] - c[a1 * 3], uy = c[a0 * 3 + 1] - c[a1 * 3 + 1],
              uz = c[a0 * 3 + 2] - c[a1 * 3 + 2];
  const float vx = c[b0 * 3] - c[b1 * 3], vy = c[b0 * 3 + 1] - c[b1 * 3 + 1],
              vz = c[b0 * 3 + 2] - c[b1 * 3 + 2];
  float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  float d = -dot3(nx, ny, nz, c[on * 3], c[on * 3 + 1], c[on * 3 + 2]);
  const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
  nx /= len, ny /= len, nz /= len, d /= len;
  float sum = 0.f;
  for (int k = 0; k < 4; ++k)
    sum += dot3(c[far[k] * 3], c[far[k] * 3 + 1], c[far[k] * 3 + 2], nx, ny, nz);
  near_p[0] = nx, near_p[1] = ny, near_p[2] = nz, near_p[3] = d;
  far_p[0] = nx, far_p[1] = ny, far_p[2] = nz, far_p[3] = -(sum / 4.f);
  return nz < lower;  // false for NaN
}

template <int MODE>
__device__ bool make_planes(const float* c, float lower, Planes& pl) {
  bool ok = true;
  float lo[4] = {0.f, 0.f, 1.f, -c[7 * 3 + 2]}, up[4];
  {
    const float z1 = c[1 * 3 + 2], z2 = c[2 * 3 + 2], z5 = c[5 * 3 + 2], z6 = c[6 * 3 + 2];
    ok = ok && z1 == z2 && z2 == z5 && z5 == z6 && (0.f + 0.f < lower);
    const int top[4] = {1, 2, 5, 6};
    float sum = 0.f;
    for (int k = 0; k < 4; ++k)
      sum += (c[top[k] * 3] * 0.f + c[top[k] * 3 + 1] * 0.f) + c[top[k] * 3 + 2] * 1.f;
    up[0] = 0.f, up[1] = 0.f, up[2] = 1.f, up[3] = -(sum / 4.f);
    const float off = (((z1 + up[3]) + (z2 + up[3])) + (z5 + up[3])) + (z6 + up[3]);
    ok = ok && (off / 4.0f < lower);
  }
  float le[4], ri[4], fr[4], ba[4];
  const int right[4] = {4, 5, 7, 6}, back[4] = {3, 2, 7, 6};
  ok = side_planes(c, 2, 3, 3, 0, 0, right, lower, le, ri) && ok;
  ok = side_planes(c, 0, 4, 4, 5, 5, back, lower, fr, ba) && ok;
  const float* src[4];
  if (MODE == kModeZ) src[0] = lo, src[1] = up, src[2] = lo, src[3] = up;
  else if (MODE == kModeXY) src[0] = le, src[1] = ri, src[2] = fr, src[3] = ba;
  else src[0] = lo, src[1] = up, src[2] = le, src[3] = ri;
  for (int k = 0; k < 4; ++k)
    for (int j = 0; j < 4; ++j) pl.p[k][j] = src[k][j];
  return ok;
}

__device__ __forceinline__ float plane_dist(const float* p, float x, float y, float z) {
  return fabsf(((x * p[0] + y * p[1]) + z * p[2]) + p[3]);
}

// the twelve lines of mode `line` in write order: plane slot, corner pair, and without yaw the
// coordinate test (0 xmin, 1 xmax, 2 ymin, 3 ymax) and the axis that takes the corner mean
__constant__ int8_t kLinePlane[12] = {0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3};
__constant__ int8_t kLineA[12] = {0, 4, 0, 3, 1, 5, 1, 2, 0, 3, 4, 7};
__constant__ int8_t kLineB[12] = {3, 7, 4, 7, 2, 6, 5, 6, 1, 2, 5, 6};
__constant__ int8_t kLineTest[12] = {0, 1, 2, 3, 0, 1, 2, 3, 2, 3, 2, 3};
__constant__ int8_t kLineAxis[12] = {1, 1, 0, 0, 1, 1, 0, 0, 2, 2, 2, 2};
// surface corner pairs: mode z (bottom, top), mode xy (left, right, front, back)
__constant__ int8_t kSurfA[2][4] = {{0, 1, 0, 1}, {0, 4, 0, 3}};
__constant__ int8_t kSurfB[2][4] = {{7, 6, 7, 6}, {1, 5, 1, 2}};

// PrimitiveHead.point2line_dist in its own form; NaN (negative radicand) selects nothing
__device__ __forceinline__ bool on_line_yaw(const float* c, int a, int b, float x, float y,
                                            float z, float thresh) {
  const float bx = c[b * 3] - c[a * 3], by = c[b * 3 + 1] - c[a * 3 + 1],
              bz = c[b * 3 + 2] - c[a * 3 + 2];
  const float px = x - c[a * 3], py = y - c[a * 3 + 1], pz = z - c[a * 3 + 2];
  const float length = dot3(px, py, pz, bx, by, bz) / sqrtf((bx * bx + by * by) + bz * bz);
  const float norm = sqrtf((px * px + py * py) + pz * pz);
  const float dist = sqrtf(norm * norm - length * length);
  return dist < thresh;
}

struct Extent {  // corners.min(0) / max(0) / mean(0)
  float lo[3], hi[3], mean[3];
};
__device__ Extent corner_extent(const float* c) {
  Extent e;
  for (int a = 0; a < 3; ++a) {
    float lo = c[a], hi = c[a];
    double sum = (double)c[a];  // the mean of eight float32 values, rounded once
    bool nan = c[a] != c[a];
    for (int k = 1; k < 8; ++k) {
      const float v = c[k * 3 + a];
      nan = nan || v != v;
      lo = fminf(lo, v), hi = fmaxf(hi, v), sum += (double)v;
    }
    const float q = __builtin_nanf("");
    e.lo[a] = nan ? q : lo, e.hi[a] = nan ? q : hi, e.mean[a] = (float)(sum / 8.0);
  }
  return e;
}

__device__ __forceinline__ bool on_line(const float* c, const Extent& e, int j, int with_yaw,
                                        float x, float y, float z, float thresh) {
  if (with_yaw) return on_line_yaw(c, kLineA[j], kLineB[j], x, y, z, thresh);
  const int t = kLineTest[j];
  const float ref = t == 0 ? e.lo[0] : t == 1 ? e.hi[0] : t == 2 ? e.lo[1] : e.hi[1];
  return fabsf((t < 2 ? x : y) - ref) < thresh;
}

__device__ __forceinline__ double block_sum(double v, double* sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = ((sm[0] + sm[1]) + sm[2]) + sm[3];
  __syncthreads();
  return t;
}

template <int MODE>
struct Shape {
  static constexpr int kPlanes = MODE == kModeZ ? 2 : 4;
  static constexpr int kPrims = MODE == kModeZ ? 2 : (MODE == kModeXY ? 4 : 12);
  static constexpr int kSums = MODE == kModeXY ? 4 : 3;  // z: S1 S2 z; xy: S1 S2 x y; line: x y z
  static constexpr int kWidth = MODE == kModeZ ? 6 : (MODE == kModeXY ? 5 : 4);
};

// grid (slot, sample): slots below `inst_blocks` own instances (striding), the others zero the
// rows no instance block writes
template <int MODE>
__global__ __launch_bounds__(kBlock) void prim_targets_kernel(
    const float* __restrict__ points, int ld, const int64_t* __restrict__ sem,
    const int32_t* __restrict__ point_offsets, int total_points,
    const float* __restrict__ corners, const int32_t* __restrict__ box_offsets, int total_boxes,
    int inst_blocks, Cfg cfg, int label_bound, const int32_t* __restrict__ count,
    const int32_t* __restrict__ ninst, const int32_t* __restrict__ first,
    const int32_t* __restrict__ start, const int32_t* __restrict__ rank,
    const int32_t* __restrict__ order, float* __restrict__ point_mask,
    float* __restrict__ point_offset, float* __restrict__ point_sem) {
  using S = Shape<MODE>;
  constexpr int P = S::kPlanes, J = S::kPrims, A = S::kSums, W = S::kWidth;
  __shared__ double red[kBlock / kWave];
  __shared__ float s_min[4];
  __shared__ int s_cnt[J];
  __shared__ double s_sum[J][A];
  __shared__ int s_on[J];
  __shared__ float s_row[J][W];  // centre, sizes, class
  __shared__ float s_c[24];      // the instance's box corners

  const int s = blockIdx.y;
  int p_begin, b_begin;
  const int np = seg_rows(point_offsets, s, total_points, p_begin);
  const int nb = seg_rows(box_offsets, s, total_boxes, b_begin);
  const int live = np > 0 ? min(min(ninst[s], nb), label_bound) : 0;  // instances with a box

  if ((int)blockIdx.x >= inst_blocks) {
    const int fill = gridDim.x - inst_blocks;
    for (int i = (blockIdx.x - inst_blocks) * kBlock + threadIdx.x; i < np; i += fill * kBlock) {
      const int r = rank[p_begin + i];
      if (r >= 0 && r < live) continue;
      const size_t row = (size_t)p_begin + i;
      point_mask[row] = 0.f;
      for (int k = 0; k < 3; ++k) point_offset[row * 3 + k] = 0.f;
      for (int k = 0; k < W; ++k) point_sem[row * W + k] = 0.f;
    }
    return;
  }

  for (int r = blockIdx.x; r < live; r += inst_blocks) {
    if (threadIdx.x < 24) s_c[threadIdx.x] = corners[((size_t)b_begin + r) * 24 + threadIdx.x];
    __syncthreads();
    const float* c = s_c;  // indexed by corner tables: LDS, not scratch
    Planes pl;
    const bool ok = make_planes<MODE>(c, cfg.lower_thresh, pl);
    const Extent ext = corner_extent(c);
    int lo = start[(size_t)s * label_bound + r];
    int n = count[(size_t)s * label_bound + r];
    lo = min(max(lo, 0), np);
    n = min(max(n, 0), np - lo);
    const int32_t* list = order + p_begin + lo;

    // sweep 1: the minimum distance to each plane (torch.min: a NaN distance is the minimum)
    float mn[P];
    int nan = 0;
    for (int k = 0; k < P; ++k) mn[k] = __builtin_inff();
    for (int t = threadIdx.x; t < n; t += kPointChunk) {
      const unsigned i = (unsigned)list[t];
      if (i >= (unsigned)np) continue;
      const float* q = points + ((size_t)p_begin + i) * ld;
      const float x = q[0], y = q[1], z = q[2];
      for (int k = 0; k < P; ++k) {
        const float d = plane_dist(pl.p[k], x, y, z);
        if (d != d) nan |= 1 << k;
        mn[k] = fminf(mn[k], d);
      }
    }
    for (int k = 0; k < P; ++k) {
      float v = mn[k];
      int f = (nan >> k) & 1;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        v = fminf(v, __shfl_xor(v, o, 64));
        f |= __shfl_xor(f, o, 64);
      }
      float* part = (float*)red;  // 4 minima, then 4 flags
      if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v, part[4 + (threadIdx.x >> 6)] = (float)f;
      __syncthreads();
      if (threadIdx.x == 0) {
        const float m = fminf(fminf(part[0], part[1]), fminf(part[2], part[3]));
        const bool any = (part[4] + part[5] + part[6] + part[7]) > 0.f;
        s_min[k] = any ? __builtin_nanf("") : m;
      }
      __syncthreads();
    }
    for (int k = 0; k < P; ++k) mn[k] = s_min[k];

    // sweep 2: per primitive the count, and in double the moments / coordinate sums
    int cnt[J];
    double acc[J][A];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      cnt[j] = 0;
#pragma unroll
      for (int a = 0; a < A; ++a) acc[j][a] = 0.0;
    }
    for (int t = threadIdx.x; t < n; t += kPointChunk) {
      const unsigned i = (unsigned)list[t];
      if (i >= (unsigned)np) continue;
      const float* q = points + ((size_t)p_begin + i) * ld;
      const float x = q[0], y = q[1], z = q[2];
      bool sel[P];
      float dist[P];
      for (int k = 0; k < P; ++k) {
        dist[k] = plane_dist(pl.p[k], x, y, z);
        sel[k] = fabsf(dist[k] - mn[k]) < cfg.dist_thresh;
      }
      if (MODE == kModeLine) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
          if (!sel[kLinePlane[j]] || !on_line(c, ext, j, cfg.with_yaw, x, y, z, cfg.line_thresh))
            continue;
          cnt[j] += 1;
          acc[j][0] += (double)x, acc[j][1] += (double)y, acc[j][2] += (double)z;
        }
      } else {
#pragma unroll
        for (int j = 0; j < J; ++j) {
          if (!sel[j >= P ? 0 : j]) continue;
          const double e = (double)dist[j] - (double)mn[j];
          cnt[j] += 1;
          acc[j][0] += e, acc[j][1] += e * e;
          if (MODE == kModeZ) acc[j][2] += (double)z;
          else acc[j][2] += (double)x, acc[j][A - 1] += (double)y;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const double total = block_sum((double)cnt[j], red);
      if (threadIdx.x == 0) s_cnt[j] = (int)total;
#pragma unroll
      for (int a = 0; a < A; ++a) {
        const double v = block_sum(acc[j][a], red);
        if (threadIdx.x == 0) s_sum[j][a] = v;
      }
    }
    __syncthreads();

    // one lane per primitive: the decision, the centre and the row the reference writes
    if (threadIdx.x < J) {
      const int j = threadIdx.x, m = s_cnt[j];
      const double inv = 1.0 / (double)m;
      int f0 = first[(size_t)s * label_bound + r];
      f0 = min(max(f0, 0), np - 1);
      const float cls = (float)sem[(size_t)p_begin + f0];
      bool on = ok;
      float cx, cy, cz, s0 = 0.f, s1 = 0.f;
      if (MODE == kModeLine) {
        on = on && m > cfg.num_point_line;
        const int a = kLineA[j], b = kLineB[j];
        if (cfg.with_yaw) {
          cx = (c[a * 3] + c[b * 3]) / 2.f, cy = (c[a * 3 + 1] + c[b * 3 + 1]) / 2.f;
          cz = (c[a * 3 + 2] + c[b * 3 + 2]) / 2.f;
        } else {
          cx = (float)(s_sum[j][0] * inv), cy = (float)(s_sum[j][1] * inv);
          cz = (float)(s_sum[j][2] * inv);
          const int axis = kLineAxis[j];
          if (axis == 0) cx = ext.mean[0];
          else if (axis == 1) cy = ext.mean[1];
          else cz = ext.mean[2];
        }
      } else {
        const double s1d = s_sum[j][0], s2d = s_sum[j][1];
        const double var = (s2d - s1d * s1d * inv) / (double)(m - 1);
        on = on && m > cfg.num_point && var < (double)cfg.var_thresh;
        const int a = kSurfA[MODE == kModeXY][j], b = kSurfB[MODE == kModeXY][j];
        if (MODE == kModeZ) {
          cz = (float)(s_sum[j][2] * inv);
          if (cfg.with_yaw) {
            cx = (c[a * 3] + c[b * 3]) / 2.0f, cy = (c[a * 3 + 1] + c[b * 3 + 1]) / 2.0f;
            // |c4 - c0|, |c3 - c0|: float32 differences, the norm in double rounded once
            const double ax = c[12] - c[0], ay = c[13] - c[1], az = c[14] - c[2];
            const double bx = c[9] - c[0], by = c[10] - c[1], bz = c[11] - c[2];
            s0 = (float)sqrt((ax * ax + ay * ay) + az * az);
            s1 = (float)sqrt((bx * bx + by * by) + bz * bz);
          } else {
            cx = ext.mean[0], cy = ext.mean[1];
            s0 = ext.hi[0] - ext.lo[0], s1 = ext.hi[1] - ext.lo[1];
          }
        } else {
          cx = (float)(s_sum[j][2] * inv), cy = (float)(s_sum[j][A - 1] * inv);
          if (cfg.with_yaw) {
            cz = (c[a * 3 + 2] + c[b * 3 + 2]) / 2.0f;
            s0 = c[b * 3 + 2] - c[a * 3 + 2];
          } else {
            cz = ext.mean[2];
            s0 = ext.hi[2] - ext.lo[2];
          }
        }
      }
      s_on[j] = on ? 1 : 0;
      s_row[j][0] = cx, s_row[j][1] = cy, s_row[j][2] = cz;
      if (W > 4) s_row[j][3] = s0;
      if (W > 5) s_row[j][4] = s1;
      s_row[j][W - 1] = cls;
    }
    __syncthreads();

    // sweep 3: every lane resolves its own point in the reference's write order
    for (int t = threadIdx.x; t < n; t += kPointChunk) {
      const unsigned i = (unsigned)list[t];
      if (i >= (unsigned)np) continue;
      const size_t row = (size_t)p_begin + i;
      const float* q = points + row * ld;
      const float x = q[0], y = q[1], z = q[2];
      bool sel[P];
      for (int k = 0; k < P; ++k)
        sel[k] = fabsf(plane_dist(pl.p[k], x, y, z) - mn[k]) < cfg.dist_thresh;
      int last = -1;
      for (int j = 0; j < J; ++j) {
        if (!s_on[j]) continue;
        bool hit;
        if (MODE == kModeLine)
          hit = sel[kLinePlane[j]] && on_line(c, ext, j, cfg.with_yaw, x, y, z, cfg.line_thresh);
        else
          hit = sel[j >= P ? 0 : j];
        if (hit) last = j;
      }
      point_mask[row] = last >= 0 ? 1.f : 0.f;
      float out[W];
      for (int k = 0; k < W; ++k) out[k] = last >= 0 ? s_row[last][k] : 0.f;
      point_offset[row * 3 + 0] = last >= 0 ? out[0] - x : 0.f;
      point_offset[row * 3 + 1] = last >= 0 ? out[1] - y : 0.f;
      point_offset[row * 3 + 2] = last >= 0 ? out[2] - z : 0.f;
      for (int k = 0; k < W; ++k) point_sem[row * W + k] = out[k];
    }
    __syncthreads();  // s_c / s_on / s_row are rewritten by the next instance
  }
}

bool index_shape_ok(int num_samples, int total_points, int label_bound) {
  return num_samples >= 0 && total_points >= 0 && label_bound >= 1 && label_bound <= kMaxLabels;
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_primitive_max_labels(void) { return kMaxLabels; }
MSMD_EXPORT int msmd_primitive_point_chunk(void) { return kPointChunk; }

MSMD_EXPORT size_t msmd_primitive_index_workspace_bytes(int num_samples, int total_points,
                                                        int label_bound) {
  if (!index_shape_ok(num_samples, total_points, label_bound) || num_samples > 65535) return 0;
  ArenaSize a;
  carve(a, num_samples, total_points, label_bound);
  return a.off + 256;
}

MSMD_EXPORT int msmd_primitive_index(const int64_t* sem, const int64_t* inst,
                                     const int32_t* point_offsets, int num_samples,
                                     int total_points, int max_points, int num_classes,
                                     int label_bound, int max_instances, void* index,
                                     size_t index_bytes, msmd_stream_t stream) {
  if (!index_shape_ok(num_samples, total_points, label_bound) || max_points < 0 ||
      max_instances < 0)
    return MSMD_ERR_INVALID_ARG;
  if (num_samples > 65535) return MSMD_ERR_RANGE;
  if (num_samples == 0) return MSMD_OK;
  if (!point_offsets || !index || (total_points > 0 && (!sem || !inst)))
    return MSMD_ERR_INVALID_ARG;
  if (index_bytes < msmd_primitive_index_workspace_bytes(num_samples, total_points, label_bound))
    return MSMD_ERR_INVALID_ARG;
  Arena a(index, index_bytes);
  const Index x = carve(a, num_samples, total_points, label_bound);
  if (!a.ok()) return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(x.bitmap, 0, x.zero_bytes, st) != hipSuccess ||
      hipMemsetAsync(x.first, 0x7f, (size_t)num_samples * label_bound * sizeof(int32_t), st) !=
          hipSuccess)
    return MSMD_ERR_LAUNCH;
  if (total_points == 0) return MSMD_OK;
  const int bound = max_points < total_points ? max_points : total_points;
  const int blocks = bound > 0 ? ceil_div(bound, kBlock) : 1;
  MSMD_LAUNCH(prim_bitmap_kernel, dim3(blocks, num_samples), dim3(kBlock), 0, st, sem, inst,
              point_offsets, total_points, num_classes, label_bound, x.bitmap);
  MSMD_LAUNCH(prim_rank_kernel, dim3(blocks, num_samples), dim3(kBlock), 0, st, sem, inst,
              point_offsets, total_points, num_classes, label_bound, x.bitmap, x.count, x.first,
              x.ninst, x.rank);
  int slots = max_instances < label_bound ? max_instances : label_bound;
  if (slots < 1) slots = 1;
  MSMD_LAUNCH(prim_list_kernel, dim3(slots, num_samples), dim3(kBlock), 0, st, point_offsets,
              total_points, label_bound, x.count, x.ninst, x.rank, x.start, x.order);
  return launch_status();
}

MSMD_EXPORT int msmd_primitive_targets_f32(
    const float* points, int ld, const int64_t* sem, const int32_t* point_offsets,
    const float* corners, const int32_t* box_offsets, int num_samples, int total_points,
    int total_boxes, int max_points, int max_boxes, int with_yaw, int mode, int num_dims,
    float dist_thresh, float var_thresh, float lower_thresh, int num_point, int num_point_line,
    float line_thresh, int label_bound, const void* index, size_t index_bytes, float* point_mask,
    float* point_offset, float* point_sem, msmd_stream_t stream) {
  if (!index_shape_ok(num_samples, total_points, label_bound) || total_boxes < 0 ||
      max_points < 0 || max_boxes < 0 || ld < 3)
    return MSMD_ERR_INVALID_ARG;
  if (mode < kModeZ || mode > kModeLine) return MSMD_ERR_INVALID_ARG;
  if (num_dims != (mode == kModeZ ? 2 : (mode == kModeXY ? 1 : 0))) return MSMD_ERR_INVALID_ARG;
  if (num_samples > 65535) return MSMD_ERR_RANGE;
  if (num_samples == 0 || total_points == 0) return MSMD_OK;
  if (!points || !sem || !point_offsets || !box_offsets || !index || !point_mask ||
      !point_offset || !point_sem || (total_boxes > 0 && !corners))
    return MSMD_ERR_INVALID_ARG;
  if (index_bytes < msmd_primitive_index_workspace_bytes(num_samples, total_points, label_bound))
    return MSMD_ERR_INVALID_ARG;
  Arena a(const_cast<void*>(index), index_bytes);
  const Index x = carve(a, num_samples, total_points, label_bound);
  if (!a.ok()) return MSMD_ERR_INVALID_ARG;
  const Cfg cfg = {dist_thresh, var_thresh, lower_thresh, line_thresh,
                   num_point,   num_point_line, with_yaw ? 1 : 0};
  const int bound = max_points < total_points ? max_points : total_points;
  int fill = bound > 0 ? ceil_div(bound, kBlock) : 1;
  if (fill > 1024) fill = 1024;
  int inst_blocks = max_boxes < label_bound ? max_boxes : label_bound;
  if (inst_blocks > total_boxes) inst_blocks = total_boxes;
  if (inst_blocks < 1 && total_boxes > 0) inst_blocks = 1;  // the bound only sizes the grid
  const dim3 grid(inst_blocks + fill, num_samples);
  hipStream_t st = (hipStream_t)stream;
#define MSMD_PRIM_LAUNCH(M)                                                                    \
  MSMD_LAUNCH(prim_targets_kernel<M>, grid, dim3(kBlock), 0, st, points, ld, sem, point_offsets, \
              total_points, corners, box_offsets, total_boxes, inst_blocks, cfg, label_bound,   \
              x.count, x.ninst, x.first, x.start, x.rank, x.order, point_mask, point_offset,    \
              point_sem)
  if (mode == kModeZ) MSMD_PRIM_LAUNCH(kModeZ);
  else if (mode == kModeXY) MSMD_PRIM_LAUNCH(kModeXY);
  else MSMD_PRIM_LAUNCH(kModeLine);
#undef MSMD_PRIM_LAUNCH
  return launch_status();
}
