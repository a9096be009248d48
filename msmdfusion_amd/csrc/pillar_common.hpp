// pillar_common.hpp -- what the voxel-table encoders share (pillar.hip: PillarFeatureNet,
// hard_vfe.hip: HardVFE): the decoration of a tile of raw [N, M, C] rows in LDS and the moments
// pass over the decorated rows (s = sum f, G = sum f f^T), from which the first BatchNorm's
// batch statistics follow in closed form.
#pragma once
#include <algorithm>

#include "common.hpp"

namespace msmd {
namespace {

constexpr int kRows = 256;     // decorated rows (pillar slots) a workgroup holds at a time
constexpr int kKMax = 16;      // decorated channels
constexpr int kKP = 17;        // LDS row pitch (odd: rows written by consecutive lanes)
constexpr int kUMax = 128;     // output channels
constexpr int kMMax = 64;      // slots per pillar
constexpr int kMomEntries = kKMax + kKMax * (kKMax + 1) / 2;   // s + upper triangle of G
constexpr int kMomBlocks = 1024;
constexpr int kBwdBlocks = 512;
constexpr int kBwdPitch = kKMax + 1;                           // A[u][0..16) and sg[u]

// kCenterZ: the voxel centre has a third channel, z - (coors[1] vz + z_offset) (HardVFE)
enum { kCluster = 1, kCenter = 2, kDistance = 4, kLegacy = 8, kCenterZ = 16 };

struct PillarArgs {
  const float* vox;        // [N, M, C]
  const int32_t* npts;     // [N]
  const int32_t* coors;    // [N, 4] (b, z, y, x)
  int n, m, c, k, flags;
  float vx, vy, xoff, yoff;
  float vz, zoff;          // read under kCenterZ only
};

inline int pillars_per_tile(int m) { return kRows / m; }

// Decorated rows of pillars [p0, p0 + np) -> dec[(p * M + slot) * kKP + j], j < 16 (columns
// [K, 16) zero).  raw: kRows * kKMax floats, mean: kRows * 3 floats.  Ends with a barrier.
__device__ __forceinline__ void decorate_tile(const PillarArgs& a, int p0, int np, float* raw,
                                              float* mean, float* dec) {
  const int tid = threadIdx.x, M = a.m, C = a.c;
  const int total = np * M * C;
  const float* src = a.vox + (long)p0 * M * C;
  for (int i = tid; i < total; i += 256) raw[i] = src[i];
  __syncthreads();
  if (a.flags & kCluster) {
    // the sum runs over all M slots (zero-filled past num_points), pillar_encoder.py:106-108
    for (int p = tid; p < np; p += 256) {
      float sx = 0.f, sy = 0.f, sz = 0.f;
      const float* r = raw + p * M * C;
      for (int s = 0; s < M; ++s, r += C) { sx += r[0]; sy += r[1]; sz += r[2]; }
      const float cnt = (float)a.npts[p0 + p];
      mean[p * 3 + 0] = sx / cnt;
      mean[p * 3 + 1] = sy / cnt;
      mean[p * 3 + 2] = sz / cnt;
    }
    __syncthreads();
  }
  for (int r = tid; r < np * M; r += 256) {
    const int p = r / M, s = r - p * M;
    float* d = dec + r * kKP;
    int j = 0;
    if (s < a.npts[p0 + p]) {
      const float* x = raw + r * C;
      float dx = 0.f, dy = 0.f, dz = 0.f;
      if (a.flags & kCenter) {
        dx = x[0] - ((float)a.coors[(long)(p0 + p) * 4 + 3] * a.vx + a.xoff);
        dy = x[1] - ((float)a.coors[(long)(p0 + p) * 4 + 2] * a.vy + a.yoff);
        if (a.flags & kCenterZ)
          dz = x[2] - ((float)a.coors[(long)(p0 + p) * 4 + 1] * a.vz + a.zoff);
      }
      // legacy: f_center is a view of the input, so the subtraction lands in raw channels 0, 1
      // as well -- after f_cluster was taken from the unmodified x, y (pillar_encoder.py:124-130)
      const bool moved = (a.flags & kCenter) && (a.flags & kLegacy);
      const float x0 = moved ? dx : x[0], x1 = moved ? dy : x[1];
      d[j++] = x0;
      d[j++] = x1;
      for (int q = 2; q < C; ++q) d[j++] = x[q];
      if (a.flags & kCluster) {
        d[j++] = x[0] - mean[p * 3 + 0];
        d[j++] = x[1] - mean[p * 3 + 1];
        d[j++] = x[2] - mean[p * 3 + 2];
      }
      if (a.flags & kCenter) {
        d[j++] = dx;
        d[j++] = dy;
        if (a.flags & kCenterZ) d[j++] = dz;
      }
      if (a.flags & kDistance) d[j++] = sqrtf(x0 * x0 + x1 * x1 + x[2] * x[2]);
    }
    for (; j < kKMax; ++j) d[j] = 0.f;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void pillar_moments_kernel(PillarArgs a, int ntiles,
                                                             double* __restrict__ part) {
  __shared__ float raw[kRows * kKMax];
  __shared__ float dec[kRows * kKP];
  __shared__ float mean[kRows * 3];
  const int tid = threadIdx.x;
  // entry tid: s[tid] for tid < 16, else the (i, j >= i) element of G
  int ei = tid, ej = -1;
  if (tid >= kKMax) {
    int e = tid - kKMax;
    ei = 0;
    while (e >= kKMax - ei && ei < kKMax - 1) { e -= kKMax - ei; ++ei; }
    ej = ei + e;
  }
  const bool live = tid < kMomEntries;
  const int P = kRows / a.m;
  double acc = 0.0;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int p0 = t * P, np = min(P, a.n - p0);
    decorate_tile(a, p0, np, raw, mean, dec);
    if (live) {
      const int rows = np * a.m;
      if (ej < 0) {
        for (int r = 0; r < rows; ++r) acc += (double)dec[r * kKP + ei];
      } else {
        for (int r = 0; r < rows; ++r)
          acc += (double)dec[r * kKP + ei] * (double)dec[r * kKP + ej];
      }
    }
    __syncthreads();
  }
  if (live) part[(long)blockIdx.x * kMomEntries + tid] = acc;
}

// moments[0..16) = s, moments[16 + i * 16 + j] = G[i][j]; partials added in block order
__global__ __launch_bounds__(256) void pillar_moments_combine_kernel(
    const double* __restrict__ part, int nblocks, double* __restrict__ moments) {
  const int tid = threadIdx.x;
  if (tid >= kMomEntries) return;
  double acc = 0.0;
  for (int b = 0; b < nblocks; ++b) acc += part[(long)b * kMomEntries + tid];
  if (tid < kKMax) { moments[tid] = acc; return; }
  int e = tid - kKMax, i = 0;
  while (e >= kKMax - i && i < kKMax - 1) { e -= kKMax - i; ++i; }
  const int j = i + e;
  moments[kKMax + i * kKMax + j] = acc;
  moments[kKMax + j * kKMax + i] = acc;
}

// partials of `entries` doubles per workgroup, added in block order (pillar backward:
// sums[u * 17 + k] = A[u][k] for k < 16, sg[u] at k = 16)
__global__ __launch_bounds__(256) void pillar_bwd_combine_kernel(const double* __restrict__ part,
                                                                 int nblocks, int entries,
                                                                 double* __restrict__ sums) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  double acc = 0.0;
  for (int b = 0; b < nblocks; ++b) acc += part[(long)b * entries + e];
  sums[e] = acc;
}


int decorated_channels(int c, int flags) {
  return c + ((flags & kCluster) ? 3 : 0) +
         ((flags & kCenter) ? ((flags & kCenterZ) ? 3 : 2) : 0) +
         ((flags & kDistance) ? 1 : 0);
}

int tiles_of(int n, int m) { return ceil_div(n, pillars_per_tile(m)); }

}  // namespace
}  // namespace msmd
