// dynamic_voxel.hip -- dynamic voxelization and DynamicScatter (sum / mean / max, fwd + bwd)
// for gfx950.
//
// Replaces dynamic_voxelize_gpu (mmdet3d/ops/voxel/src/voxelization_cuda.cu:25-61, 328-371) and
// dynamic_point_to_voxel_forward_gpu / _backward_gpu (scatter_points_cuda.cu:246-383), split
// into an index half that depends on the coordinates only and a feature half that streams the
// features over the index half's segment table:
//
//   index half (msmd_scatter_index): once per coordinate set, reusable by every scatter and
//     gather on it (DynamicVFE runs 2-4 of them per forward on the same coordinates)
//     1. per-column OR of the valid rows -> bit width of every column; key = the columns
//        packed most significant first in those widths (64-bit: the reference's int32 linear
//        id overflows at 2^31 cells), invalid rows (any negative entry) -> all ones
//     2. stable radix sort of (key, point index): the keys in lexicographic row order, the
//        points of one voxel in ascending point index
//     3. one scan over the sorted keys: voxel id = rank of the key's first occurrence;
//        emits voxel_coors, point2voxel, the segment starts; the voxel count is the only
//        value the host reads
//   feature half: voxel-stationary (v, c) threads walk their segment in ascending point
//     index -- fixed summation order, no float atomics, bitwise reproducible; max keeps the
//     first (smallest) point index that attains the maximum, the index the reference's
//     atomicMin traceback picks.  Backward and the voxel -> point gather are point-stationary
//     and write every element once.
//
// Integer atomics only (column OR, the max traceback of the shim's backward); all results exact
// or in a fixed order.
#include <hipcub/hipcub.hpp>

#include "common.hpp"
#include "scan.hpp"

namespace msmd {
namespace {

constexpr uint64_t kInvalidKey = ~0ull;   // sorts after every valid key (valid keys < 2^63)
constexpr int kMaxNDim = 8;

struct DynGeom {
  float vs[3], lo[3];
  int grid[3];  // x,y,z
};

// voxelization_cuda.cu:25-61, write pattern included: x out of range writes slot 0 only, y
// slots 0-1, z all three; slots not written keep the caller's values.  Rows of `ndim` ints.
__global__ __launch_bounds__(256) void dyn_voxelize_kernel(const float* __restrict__ points, int n,
                                                           int c, DynGeom g, int ndim,
                                                           int32_t* __restrict__ coors) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* p = points + (size_t)i * c;
  int32_t* o = coors + (size_t)i * ndim;
  const int cx = (int)floorf((p[0] - g.lo[0]) / g.vs[0]);
  if (cx < 0 || cx >= g.grid[0]) {
    o[0] = -1;
    return;
  }
  const int cy = (int)floorf((p[1] - g.lo[1]) / g.vs[1]);
  if (cy < 0 || cy >= g.grid[1]) {
    o[0] = -1;
    o[1] = -1;
    return;
  }
  const int cz = (int)floorf((p[2] - g.lo[2]) / g.vs[2]);
  if (cz < 0 || cz >= g.grid[2]) {
    o[0] = -1;
    o[1] = -1;
    o[2] = -1;
  } else {
    o[0] = cz;
    o[1] = cy;
    o[2] = cx;
  }
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// step 1a: OR of every column over the valid rows (colbits zero-filled before)
__global__ __launch_bounds__(256) void dyn_col_or(const int32_t* __restrict__ coors, int n,
                                                  int ndim, uint32_t* __restrict__ colbits) {
  uint32_t acc[kMaxNDim];
#pragma unroll
  for (int d = 0; d < kMaxNDim; ++d) acc[d] = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int32_t* r = coors + (size_t)i * ndim;
    bool ok = true;
    uint32_t v[kMaxNDim];
#pragma unroll
    for (int d = 0; d < kMaxNDim; ++d) {
      v[d] = 0;
      if (d < ndim) {
        const int32_t x = r[d];
        ok = ok && x >= 0;
        v[d] = (uint32_t)x;
      }
    }
    if (ok)
#pragma unroll
      for (int d = 0; d < kMaxNDim; ++d) acc[d] |= v[d];
  }
  // wave, then block, then one atomic per column and block (same-address atomics of every
  // wave: 115 us at the stress size, measured)
  __shared__ uint32_t part[256 / 64][kMaxNDim];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 0; d < kMaxNDim; ++d) {
    const uint32_t x = wave_or(acc[d]);
    if (lane == 0) part[w][d] = x;
  }
  __syncthreads();
  if (threadIdx.x < ndim) {
    uint32_t x = 0;
    for (int i = 0; i < 256 / 64; ++i) x |= part[i][threadIdx.x];
    if (x) atomicOr(&colbits[threadIdx.x], x);
  }
}

// step 1b: packed keys + identity values for the sort; info[1] <- 1 when the widths exceed 63
__global__ __launch_bounds__(256) void dyn_keys(const int32_t* __restrict__ coors, int n, int ndim,
                                                const uint32_t* __restrict__ colbits,
                                                uint64_t* __restrict__ keys,
                                                int32_t* __restrict__ vals,
                                                int32_t* __restrict__ info) {
  int width[kMaxNDim], total = 0;
#pragma unroll
  for (int d = 0; d < kMaxNDim; ++d) {
    width[d] = 0;
    if (d < ndim) {
      const uint32_t b = colbits[d];
      width[d] = b ? 32 - __clz((int)b) : 0;
      total += width[d];
    }
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) info[1] = total > 63 ? 1 : 0;
  if (i >= n) return;
  const int32_t* r = coors + (size_t)i * ndim;
  uint64_t k = 0;
  bool ok = total <= 63;
#pragma unroll
  for (int d = 0; d < kMaxNDim; ++d) {
    if (d >= ndim) break;
    const int32_t x = r[d];
    ok = ok && x >= 0;
    k = (width[d] ? (k << width[d]) : k) | (uint64_t)(uint32_t)(x >= 0 ? x : 0);
  }
  keys[i] = ok ? k : kInvalidKey;
  vals[i] = i;
}

struct SegFirst {  // 1 when sorted element i opens a voxel
  const uint64_t* skeys;
  __device__ int operator()(int i) const {
    const uint64_t k = skeys[i];
    return k != kInvalidKey && (i == 0 || skeys[i - 1] != k);
  }
};
struct SegEmit {
  const uint64_t* skeys;
  const int32_t* perm;
  const int32_t* coors;
  int n, ndim;
  int32_t *voxel_coors, *point2voxel, *seg_start;
  __device__ void operator()(int i, int p, int v) const {
    const uint64_t k = skeys[i];
    const int pt = perm[i];
    if (k == kInvalidKey) {
      point2voxel[pt] = -1;
      return;
    }
    const int id = p + v - 1;
    point2voxel[pt] = id;
    if (v) {
      seg_start[id] = i;
      for (int d = 0; d < ndim; ++d)
        voxel_coors[(size_t)id * ndim + d] = coors[(size_t)pt * ndim + d];
    }
    if (i == n - 1 || skeys[i + 1] == kInvalidKey) seg_start[id + 1] = i + 1;
  }
};

__global__ __launch_bounds__(256) void dyn_counts(int n, const int32_t* __restrict__ info,
                                                  int32_t* __restrict__ seg_start,
                                                  int32_t* __restrict__ counts) {
  const int m = info[0];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0 && m == 0) seg_start[0] = 0;
  if (i < m) counts[i] = seg_start[i + 1] - seg_start[i];
}

struct IdxWs {
  uint64_t *keys, *skeys;
  int32_t* vals;
  uint32_t* colbits;
  int* tiles;
  void* cub;
  size_t cub_bytes;
};
template <typename A>
void carve_idx(A& a, IdxWs* w, int n) {
  const int m = n > 0 ? n : 1;
  size_t cb = 0;
  hipcub::DeviceRadixSort::SortPairs(nullptr, cb, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                     (int32_t*)nullptr, (int32_t*)nullptr, m);
  IdxWs v;
  v.keys = a.template take<uint64_t>(m);
  v.skeys = a.template take<uint64_t>(m);
  v.vals = a.template take<int32_t>(m);
  v.colbits = a.template take<uint32_t>(kMaxNDim);
  v.tiles = a.template take<int>(scan_num_tiles(m) + 1);
  v.cub_bytes = cb;
  v.cub = a.template take<char>(cb);
  if (w) *w = v;
}

// ---- feature half ----------------------------------------------------------------------
// out[v, c] over the points of segment v in ascending point index (reduce 0 sum, 1 mean,
// 2 max + argmax).
__global__ __launch_bounds__(256) void seg_reduce(const float* __restrict__ feats, int c,
                                                  const int32_t* __restrict__ seg_points,
                                                  const int32_t* __restrict__ seg_start, int m,
                                                  int reduce, float* __restrict__ out,
                                                  int32_t* __restrict__ argmax) {
  const long total = (long)m * c;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int v = (int)(t / c), ch = (int)(t - (long)v * c);
    const int b = seg_start[v], e = seg_start[v + 1];
    if (reduce == 2) {
      int arg = seg_points[b];
      float mx = feats[(size_t)arg * c + ch];
      for (int j = b + 1; j < e; ++j) {
        const int pt = seg_points[j];
        const float x = feats[(size_t)pt * c + ch];
        if (x > mx) {
          mx = x;
          arg = pt;
        }
      }
      out[t] = mx;
      if (argmax) argmax[t] = arg;
    } else {
      float s = 0.f;
      for (int j = b; j < e; ++j) s += feats[(size_t)seg_points[j] * c + ch];
      out[t] = reduce == 1 ? s / (float)(e - b) : s;
    }
  }
}

// grad_in[i, c]: sum -> g[v, c], mean -> g[v, c] / count[v], max -> g[v, c] where
// argmax[v, c] == i; 0 for every other point and for invalid points
__global__ __launch_bounds__(256) void seg_reduce_bwd(const float* __restrict__ grad_out, int n,
                                                      int c, const int32_t* __restrict__ p2v,
                                                      int m, const int32_t* __restrict__ counts,
                                                      const int32_t* __restrict__ argmax,
                                                      int reduce, float* __restrict__ grad_in) {
  const long total = (long)n * c;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int i = (int)(t / c), ch = (int)(t - (long)i * c);
    const int v = p2v[i];
    float g = 0.f;
    if (v >= 0 && v < m) {
      const size_t o = (size_t)v * c + ch;
      if (reduce == 0)
        g = grad_out[o];
      else if (reduce == 1)
        g = grad_out[o] / (float)counts[v];
      else if (argmax[o] == i)
        g = grad_out[o];
    }
    grad_in[t] = g;
  }
}

__global__ __launch_bounds__(256) void fill_i32(int32_t* __restrict__ p, long n, int32_t value) {
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long)gridDim.x * 256)
    p[t] = value;
}

// max_reduce_traceback_scatter_idx_kernel: smallest point index whose value equals the voxel's
// (integer atomicMin: the result does not depend on the order)
__global__ __launch_bounds__(256) void max_traceback(const float* __restrict__ feats, int n, int c,
                                                     const int32_t* __restrict__ p2v,
                                                     const float* __restrict__ reduced, int m,
                                                     int32_t* __restrict__ argmax) {
  const long total = (long)n * c;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int i = (int)(t / c), ch = (int)(t - (long)i * c);
    const int v = p2v[i];
    if (v < 0 || v >= m) continue;
    const size_t o = (size_t)v * c + ch;
    if (feats[t] == reduced[o]) atomicMin(&argmax[o], i);
  }
}

__global__ __launch_bounds__(256) void point_gather(const float* __restrict__ voxel_feats, int m,
                                                    int n, int c, const int32_t* __restrict__ p2v,
                                                    float* __restrict__ out) {
  const long total = (long)n * c;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int i = (int)(t / c), ch = (int)(t - (long)i * c);
    const int v = p2v[i];
    out[t] = v >= 0 && v < m ? voxel_feats[(size_t)v * c + ch] : 0.f;
  }
}

inline int stream_grid(long work) {
  long b = (work + 255) / 256;
  if (b > 8192) b = 8192;
  return (int)(b > 0 ? b : 1);
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_dynamic_voxelize(const float* points, int num_points, int num_features,
                                      const float* voxel_size, const float* coors_range, int ndim,
                                      int32_t* coors, msmd_stream_t stream) {
  if (num_points < 0 || num_features < 3 || ndim < 3 || !voxel_size || !coors_range ||
      (num_points > 0 && (!points || !coors)))
    return MSMD_ERR_INVALID_ARG;
  DynGeom g;
  for (int i = 0; i < 3; ++i) {
    g.vs[i] = voxel_size[i];
    g.lo[i] = coors_range[i];
    // voxelization_cuda.cu:350-352 -- round() of the float quotient
    g.grid[i] = (int)roundf((coors_range[3 + i] - coors_range[i]) / voxel_size[i]);
  }
  if (num_points == 0) return MSMD_OK;
  MSMD_LAUNCH(dyn_voxelize_kernel, dim3(ceil_div(num_points, 256)), dim3(256), 0,
              (hipStream_t)stream, points, num_points, num_features, g, ndim, coors);
  return launch_status();
}

MSMD_EXPORT size_t msmd_scatter_index_workspace_bytes(int num_points) {
  if (num_points < 0) return 0;
  ArenaSize a;
  carve_idx(a, (IdxWs*)nullptr, num_points);
  return a.off;
}

MSMD_EXPORT int msmd_scatter_index(const int32_t* coors, int num_points, int ndim,
                                   int32_t* voxel_coors, int32_t* point2voxel,
                                   int32_t* seg_points, int32_t* seg_start, int32_t* counts,
                                   int32_t* info, void* workspace, size_t workspace_bytes,
                                   msmd_stream_t stream) {
  if (num_points < 0 || ndim < 1 || ndim > kMaxNDim || !info || !seg_start ||
      (num_points > 0 && (!coors || !voxel_coors || !point2voxel || !seg_points || !counts)))
    return MSMD_ERR_INVALID_ARG;
  Arena a(workspace, workspace_bytes);
  IdxWs w;
  carve_idx(a, &w, num_points);
  if (!a.ok()) return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int n = num_points;
  hipMemsetAsync(info, 0, 2 * sizeof(int32_t), st);
  if (n > 0) {
    hipMemsetAsync(w.colbits, 0, kMaxNDim * sizeof(uint32_t), st);
    const int nb = ceil_div(n, 256);
    MSMD_LAUNCH(dyn_col_or, dim3(nb < 256 ? nb : 256), dim3(256), 0, st, coors, n, ndim,
                w.colbits);
    MSMD_LAUNCH(dyn_keys, dim3(nb), dim3(256), 0, st, coors, n, ndim,
                (const uint32_t*)w.colbits, w.keys, w.vals, info);
    size_t cb = w.cub_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, w.keys, w.skeys, w.vals, seg_points, n, 0,
                                           64, st) != hipSuccess)
      return MSMD_ERR_LAUNCH;
  }
  device_scan(SegFirst{w.skeys},
              SegEmit{w.skeys, seg_points, coors, n, ndim, voxel_coors, point2voxel, seg_start},
              n, w.tiles, info, -1, st);
  MSMD_LAUNCH(dyn_counts, dim3(n > 0 ? ceil_div(n, 256) : 1), dim3(256), 0, st, n,
              (const int32_t*)info, seg_start, counts);
  return launch_status();
}

MSMD_EXPORT int msmd_scatter_reduce_f32(const float* feats, int num_points, int num_channels,
                                        const int32_t* seg_points, const int32_t* seg_start,
                                        int num_voxels, int reduce, float* out, int32_t* argmax,
                                        msmd_stream_t stream) {
  if (num_points < 0 || num_channels < 1 || num_voxels < 0 || num_voxels > num_points ||
      reduce < 0 || reduce > 2)
    return MSMD_ERR_INVALID_ARG;
  if (num_voxels == 0) return MSMD_OK;
  if (!feats || !seg_points || !seg_start || !out) return MSMD_ERR_INVALID_ARG;
  const long work = (long)num_voxels * num_channels;
  MSMD_LAUNCH(seg_reduce, dim3(stream_grid(work)), dim3(256), 0, (hipStream_t)stream, feats,
              num_channels, seg_points, seg_start, num_voxels, reduce, out,
              reduce == 2 ? argmax : nullptr);
  return launch_status();
}

MSMD_EXPORT int msmd_scatter_reduce_bwd_f32(const float* grad_out, int num_voxels,
                                            int num_points, int num_channels,
                                            const int32_t* point2voxel,
                                            const int32_t* counts, const int32_t* argmax,
                                            int reduce, float* grad_in, msmd_stream_t stream) {
  if (num_points < 0 || num_channels < 1 || num_voxels < 0 || reduce < 0 || reduce > 2)
    return MSMD_ERR_INVALID_ARG;
  if (num_points == 0) return MSMD_OK;
  if ((num_voxels > 0 && !grad_out) || !point2voxel || !grad_in || (reduce == 1 && !counts) ||
      (reduce == 2 && !argmax))
    return MSMD_ERR_INVALID_ARG;
  const long work = (long)num_points * num_channels;
  MSMD_LAUNCH(seg_reduce_bwd, dim3(stream_grid(work)), dim3(256), 0, (hipStream_t)stream,
              grad_out, num_points, num_channels, point2voxel, num_voxels, counts, argmax, reduce,
              grad_in);
  return launch_status();
}

MSMD_EXPORT int msmd_scatter_max_argmax_f32(const float* feats, int num_points, int num_channels,
                                            const int32_t* point2voxel, const float* reduced,
                                            int num_voxels, int32_t* argmax,
                                            msmd_stream_t stream) {
  if (num_points < 0 || num_channels < 1 || num_voxels < 0) return MSMD_ERR_INVALID_ARG;
  if (num_voxels == 0) return MSMD_OK;
  if (!reduced || !argmax || (num_points > 0 && (!feats || !point2voxel)))
    return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long mc = (long)num_voxels * num_channels;
  MSMD_LAUNCH(fill_i32, dim3(stream_grid(mc)), dim3(256), 0, st, argmax, mc, num_points);
  if (num_points > 0) {
    const long work = (long)num_points * num_channels;
    MSMD_LAUNCH(max_traceback, dim3(stream_grid(work)), dim3(256), 0, st, feats, num_points,
                num_channels, point2voxel, reduced, num_voxels, argmax);
  }
  return launch_status();
}

MSMD_EXPORT int msmd_scatter_gather_f32(const float* voxel_feats, int num_voxels,
                                        int num_channels, const int32_t* point2voxel,
                                        int num_points, float* out, msmd_stream_t stream) {
  if (num_points < 0 || num_channels < 1 || num_voxels < 0) return MSMD_ERR_INVALID_ARG;
  if (num_points == 0) return MSMD_OK;
  if (!point2voxel || !out || (num_voxels > 0 && !voxel_feats)) return MSMD_ERR_INVALID_ARG;
  const long work = (long)num_points * num_channels;
  MSMD_LAUNCH(point_gather, dim3(stream_grid(work)), dim3(256), 0, (hipStream_t)stream,
              voxel_feats, num_voxels, num_points, num_channels, point2voxel, out);
  return launch_status();
}
