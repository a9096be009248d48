// pillar.hip -- the PointPillars voxel encoder (PillarFeatureNet with one PFNLayer) fused:
// point decoration, Linear (no bias), BatchNorm1d, ReLU and the max / mean over the slots of a
// pillar, without the [N, M, U] activations the reference materialises four times.
//
// reference: mmdet3d/models/voxel_encoders/pillar_encoder.py:91-150 (decoration, mask) and
//            mmdet3d/models/voxel_encoders/utils.py:191-227 (PFNLayer.forward)
//
// Three passes over the raw [N, M, C] table, each rebuilding the decorated rows in LDS:
//   moments : s[K] = sum f, G[K][K] = sum f f^T over all N*M rows (padded rows are zero rows but
//             count in n) -- BatchNorm's batch statistics of W f follow from them in closed form;
//   forward : out[n][u] = max_m | sum_m / num_points  relu(scale_u * (w_u . f) + shift_u);
//   backward: A[U][K] = sum g f, sg[U] = sum g with g the gradient reaching the BatchNorm output.
// Sums are accumulated in fp64 (products of two floats are exact there) per workgroup and the
// workgroup partials are added in block order by a second kernel: no float atomics, two runs
// give the same bits.
#include "pillar_common.hpp"

namespace msmd {
namespace {

// W[U][K], scale[U], shift[U] -> wt[k * U + u] (k < 16, zero past K), sc, sh.  No barrier.
__device__ __forceinline__ void load_affine(const float* __restrict__ w, const float* scale,
                                            const float* shift, int U, int K, float* wt, float* sc,
                                            float* sh) {
  for (int i = threadIdx.x; i < kKMax * U; i += 256) {
    const int k = i / U, u = i - k * U;
    wt[i] = k < K ? w[u * K + k] : 0.f;
  }
  for (int u = threadIdx.x; u < U; u += 256) { sc[u] = scale[u]; sh[u] = shift[u]; }
}

__device__ __forceinline__ float pfn_unit(const float* wreg, const float* f, float sc, float sh) {
  float z = 0.f;
#pragma unroll
  for (int k = 0; k < kKMax; ++k) z = fmaf(wreg[k], f[k], z);
  return z * sc + sh;        // BatchNorm folded to one scale and shift; the ReLU is the caller's
}

template <bool MAX>
__global__ __launch_bounds__(256) void pillar_pfn_fwd_kernel(
    PillarArgs a, int ntiles, const float* __restrict__ w, const float* __restrict__ scale,
    const float* __restrict__ shift, int U, float* __restrict__ out,
    uint8_t* __restrict__ argmax) {
  __shared__ float raw[kRows * kKMax];
  __shared__ float dec[kRows * kKP];
  __shared__ float mean[kRows * 3];
  __shared__ float wt[kKMax * kUMax];
  __shared__ float sc[kUMax], sh[kUMax];
  load_affine(w, scale, shift, U, a.k, wt, sc, sh);    // (decorate_tile's barriers cover it)
  const int P = kRows / a.m, M = a.m;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int p0 = t * P, np = min(P, a.n - p0);
    decorate_tile(a, p0, np, raw, mean, dec);
    for (int o = threadIdx.x; o < np * U; o += 256) {
      const int p = o / U, u = o - p * U;
      float wreg[kKMax];
#pragma unroll
      for (int k = 0; k < kKMax; ++k) wreg[k] = wt[k * U + u];
      const float s = sc[u], h = sh[u];
      const float* f = dec + p * M * kKP;
      if (MAX) {
        float best = -1.f;      // relu output is >= 0: the first slot always takes it
        int arg = 0;
        for (int m = 0; m < M; ++m, f += kKP) {
          const float y = fmaxf(pfn_unit(wreg, f, s, h), 0.f);
          if (y > best) { best = y; arg = m; }       // strict: smallest slot on ties
        }
        out[(long)(p0 + p) * U + u] = best;
        argmax[(long)(p0 + p) * U + u] = (uint8_t)arg;
      } else {
        float sum = 0.f;        // padded slots included (utils.py:218-220)
        for (int m = 0; m < M; ++m, f += kKP) sum += fmaxf(pfn_unit(wreg, f, s, h), 0.f);
        out[(long)(p0 + p) * U + u] = sum / (float)a.npts[p0 + p];
      }
    }
    __syncthreads();
  }
}

template <bool MAX>
__global__ __launch_bounds__(256) void pillar_pfn_bwd_kernel(
    PillarArgs a, int ntiles, const float* __restrict__ w, const float* __restrict__ scale,
    const float* __restrict__ shift, int U, const float* __restrict__ grad_out,
    const uint8_t* __restrict__ argmax, double* __restrict__ part) {
  // raw and dec are one buffer: after the last tile its head holds the workgroup's fp64 sums
  __shared__ __align__(16) float buf[kRows * kKMax + kRows * kKP];
  __shared__ float mean[kRows * 3];
  __shared__ float wt[kKMax * kUMax];
  __shared__ float sc[kUMax], sh[kUMax];
  float* raw = buf;
  float* dec = buf + kRows * kKMax;
  load_affine(w, scale, shift, U, a.k, wt, sc, sh);
  const int P = kRows / a.m, M = a.m;
  const int groups = 256 / U;                 // U <= 128: at least two pillars in flight
  const int tid = threadIdx.x, grp = tid / U, u = tid - grp * U;
  const bool live = grp < groups;
  double acc[kBwdPitch];
#pragma unroll
  for (int k = 0; k < kBwdPitch; ++k) acc[k] = 0.0;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int p0 = t * P, np = min(P, a.n - p0);
    decorate_tile(a, p0, np, raw, mean, dec);
    if (live) {
      float wreg[kKMax];
#pragma unroll
      for (int k = 0; k < kKMax; ++k) wreg[k] = wt[k * U + u];
      const float s = sc[u], h = sh[u];
      for (int p = grp; p < np; p += groups) {
        float go = grad_out[(long)(p0 + p) * U + u];
        int m0 = 0, m1 = M;
        if (MAX) {
          m0 = min((int)argmax[(long)(p0 + p) * U + u], M - 1);
          m1 = m0 + 1;
        } else {
          go = go / (float)a.npts[p0 + p];
        }
        for (int m = m0; m < m1; ++m) {
          const float* f = dec + (p * M + m) * kKP;
          if (pfn_unit(wreg, f, s, h) > 0.f) {
            const double g = (double)go;
#pragma unroll
            for (int k = 0; k < kKMax; ++k) acc[k] += g * (double)f[k];
            acc[kKMax] += g;
          }
        }
      }
    }
    __syncthreads();
  }
  // the groups add their sums one after the other: a fixed order
  double* red = (double*)buf;                 // U * 17 doubles <= 17 KB of the 33 KB buffer
  for (int g = 0; g < groups; ++g) {
    if (live && grp == g) {
#pragma unroll
      for (int k = 0; k < kBwdPitch; ++k) {
        if (g == 0) red[u * kBwdPitch + k] = acc[k];
        else red[u * kBwdPitch + k] += acc[k];
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < U * kBwdPitch; e += 256)
    part[(long)blockIdx.x * U * kBwdPitch + e] = red[e];
}

// 0, or the status that refuses the shape
int pillar_shape_status(int n, int m, int c, int flags, int u) {
  if (n < 0 || m < 1 || c < 3 || u < 1 || (flags & ~15)) return MSMD_ERR_INVALID_ARG;
  if (m > kMMax || u > kUMax || decorated_channels(c, flags) > kKMax) return MSMD_ERR_UNSUPPORTED;
  if ((double)n * m * c >= 9.0e18) return MSMD_ERR_RANGE;
  return MSMD_OK;
}


}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT size_t msmd_pillar_workspace_bytes(int num_pillars, int max_points,
                                               int out_channels) {
  if (num_pillars < 0 || max_points < 1 || max_points > kMMax || out_channels < 1 ||
      out_channels > kUMax)
    return 0;
  const int tiles = tiles_of(num_pillars, max_points);
  const size_t mom = (size_t)std::min(std::max(tiles, 1), kMomBlocks) * kMomEntries;
  const size_t bwd = (size_t)std::min(std::max(tiles, 1), kBwdBlocks) * out_channels * kBwdPitch;
  return align_up(std::max(mom, bwd) * sizeof(double));
}

static PillarArgs pillar_args(const float* voxels, const int32_t* num_points,
                              const int32_t* coors, int n, int m, int c, int flags, float vx,
                              float vy, float xoff, float yoff) {
  PillarArgs a;
  a.vox = voxels; a.npts = num_points; a.coors = coors;
  a.n = n; a.m = m; a.c = c; a.k = decorated_channels(c, flags); a.flags = flags;
  a.vx = vx; a.vy = vy; a.xoff = xoff; a.yoff = yoff;
  a.vz = 0.f; a.zoff = 0.f;
  return a;
}

MSMD_EXPORT int msmd_pillar_moments_f32(const float* voxels, const int32_t* num_points,
                                        const int32_t* coors, int num_pillars, int max_points,
                                        int num_features, int flags, float vx, float vy,
                                        float x_offset, float y_offset, double* moments,
                                        void* workspace, size_t workspace_bytes,
                                        msmd_stream_t stream) {
  int rc = pillar_shape_status(num_pillars, max_points, num_features, flags, 1);
  if (rc) return rc;
  if (!moments) return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (num_pillars == 0) return MSMD_OK;
  if (!voxels || !num_points || !coors) return MSMD_ERR_INVALID_ARG;
  const int tiles = tiles_of(num_pillars, max_points), blocks = std::min(tiles, kMomBlocks);
  if (!workspace || ((uintptr_t)workspace & 255) ||
      workspace_bytes < (size_t)blocks * kMomEntries * sizeof(double))
    return MSMD_ERR_WORKSPACE;
  PillarArgs a = pillar_args(voxels, num_points, coors, num_pillars, max_points, num_features,
                             flags, vx, vy, x_offset, y_offset);
  MSMD_LAUNCH(pillar_moments_kernel, dim3(blocks), dim3(256), 0, st, a, tiles,
              (double*)workspace);
  MSMD_LAUNCH(pillar_moments_combine_kernel, dim3(1), dim3(256), 0, st,
              (const double*)workspace, blocks, moments);
  return launch_status();
}

MSMD_EXPORT int msmd_pillar_pfn_fwd_f32(const float* voxels, const int32_t* num_points,
                                        const int32_t* coors, int num_pillars, int max_points,
                                        int num_features, int flags, float vx, float vy,
                                        float x_offset, float y_offset, const float* weight,
                                        const float* scale, const float* shift, int out_channels,
                                        int mode_max, float* out, uint8_t* argmax,
                                        msmd_stream_t stream) {
  int rc = pillar_shape_status(num_pillars, max_points, num_features, flags, out_channels);
  if (rc) return rc;
  if (num_pillars == 0) return MSMD_OK;
  if (!voxels || !num_points || !coors || !weight || !scale || !shift || !out ||
      (mode_max && !argmax))
    return MSMD_ERR_INVALID_ARG;
  const int tiles = tiles_of(num_pillars, max_points);
  const int blocks = std::min(tiles, 8192);
  PillarArgs a = pillar_args(voxels, num_points, coors, num_pillars, max_points, num_features,
                             flags, vx, vy, x_offset, y_offset);
  if (mode_max)
    MSMD_LAUNCH(pillar_pfn_fwd_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a,
                tiles, weight, scale, shift, out_channels, out, argmax);
  else
    MSMD_LAUNCH(pillar_pfn_fwd_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a,
                tiles, weight, scale, shift, out_channels, out, argmax);
  return launch_status();
}

MSMD_EXPORT int msmd_pillar_pfn_bwd_f32(const float* voxels, const int32_t* num_points,
                                        const int32_t* coors, int num_pillars, int max_points,
                                        int num_features, int flags, float vx, float vy,
                                        float x_offset, float y_offset, const float* weight,
                                        const float* scale, const float* shift, int out_channels,
                                        int mode_max, const float* grad_out,
                                        const uint8_t* argmax, double* sums, void* workspace,
                                        size_t workspace_bytes, msmd_stream_t stream) {
  int rc = pillar_shape_status(num_pillars, max_points, num_features, flags, out_channels);
  if (rc) return rc;
  if (!sums) return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int entries = out_channels * kBwdPitch;
  if (num_pillars == 0) return MSMD_OK;
  if (!voxels || !num_points || !coors || !weight || !scale || !shift || !grad_out ||
      (mode_max && !argmax))
    return MSMD_ERR_INVALID_ARG;
  const int tiles = tiles_of(num_pillars, max_points), blocks = std::min(tiles, kBwdBlocks);
  if (!workspace || ((uintptr_t)workspace & 255) ||
      workspace_bytes < (size_t)blocks * entries * sizeof(double))
    return MSMD_ERR_WORKSPACE;
  PillarArgs a = pillar_args(voxels, num_points, coors, num_pillars, max_points, num_features,
                             flags, vx, vy, x_offset, y_offset);
  if (mode_max)
    MSMD_LAUNCH(pillar_pfn_bwd_kernel<true>, dim3(blocks), dim3(256), 0, st, a, tiles, weight,
                scale, shift, out_channels, grad_out, argmax, (double*)workspace);
  else
    MSMD_LAUNCH(pillar_pfn_bwd_kernel<false>, dim3(blocks), dim3(256), 0, st, a, tiles, weight,
                scale, shift, out_channels, grad_out, argmax, (double*)workspace);
  MSMD_LAUNCH(pillar_bwd_combine_kernel, dim3(ceil_div(entries, 256)), dim3(256), 0, st,
              (const double*)workspace, blocks, entries, sums);
  return launch_status();
}
