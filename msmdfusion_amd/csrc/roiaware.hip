// roiaware.hip -- RoI-aware 3-D pooling (max / avg, fwd + bwd) and points-in-boxes for gfx950.
//
// Replaces roiaware_pool3d_ext.forward / backward / points_in_boxes_gpu / points_in_boxes_batch
// (mmdet3d/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu, points_in_boxes_cuda.cu), split
// into an index half that depends on the RoIs and points only and a feature half that streams
// the features over it.  Contract, element by element:
//
//   point-in-box (check_pt_in_box3d, box = x, y, z(bottom), w, l, h, rz), float/double mix kept:
//     cz = (float)(z_bottom + h / 2.0); reject when fabsf(z - cz) > h / 2.0 (double compare);
//     rot = (float)(rz + M_PI / 2); cosf / sinf; sx = x - cx, sy = y - cy;
//     local_x = sx * cos - sy * sin, local_y = sx * sin + sy * cos (float);
//     inside when -l/2.0 < local_x < l/2.0 and -w/2.0 < local_y < w/2.0 (strict, double)
//   voxel of a point inside RoI r (float, the library builds with -ffp-contract=off and
//     correctly rounded division): ix = int((local_x + l/2) / (l/out_x)), iy likewise over
//     w / out_y, iz = int((z - z_bottom) / (h/out_z)), each clamped to [0, out-1];
//     out_x/y/z in 1..256 (the reference packs 8 bits per axis and aliases above; refused here)
//   point lists: (r, voxel) keeps its first max_pts_per_voxel - 1 points in ascending point
//     index (slot 0 of the reference table is the counter: max_pts_per_voxel = 1 keeps none)
//   max: running maximum from -inf, replaced only when strictly greater (ties -> smallest
//     point index, NaN never wins); no winner -> pooled 0, argmax -1
//   avg: float32 sum in ascending point index, then / count; empty -> 0
//   backward: grad_in[p, c] = sum over p's kept hits in ascending RoI order, float32, no float
//     atomics (bitwise reproducible); max adds grad_out[r, v, c] where argmax == p, avg adds
//     grad_out[r, v, c] * (1.f / fmaxf(count, 1)) (a product, as the reference)
//   points_in_boxes: first box k (ascending) holding the point else -1, or all 0/1 flags
//
// Index half (msmd_roiaware_count + msmd_roiaware_index), one launch set for the whole batch:
//   1. (RoI, 2048-point tile) blocks test their pairs -- batch id, BEV bounding circle, then the
//      predicate -- and count the hits; one scan gives every tile its output offset and the
//      total, the only value the host reads
//   2. the same blocks emit (key = r * V + voxel, point) in (RoI, point) order, ranked
//      item-major inside the tile (ascending point index)
//   3. stable radix sort on the key: each voxel's points stay in ascending point index;
//      vox_start[cell] = first hit of the cell (binary search), count = min(size, cap)
//   4. inverse for the backward: kept hits re-sorted by point (stable, so ascending RoI)
// No N x M mask, no padded table: the pooling and backward kernels read the compact index.
// The padded pts_idx_of_voxels layout is written only for the pybind-signature shim, which
// also rebuilds the index from a table it is handed (msmd_roiaware_table_*).
#include <hipcub/hipcub.hpp>
#include <math.h>

#include "common.hpp"
#include "point_in_box.hpp"
#include "scan.hpp"

namespace msmd {
namespace {

constexpr int kRoiMaxOut = 256;
constexpr long kRoiMaxBlocks = (1L << 24) - 1;  // blocks of one (RoI, tile) launch

using pib::Box;
using pib::load_box;
using pib::pt_in_box;

// min(max(int(q), 0), n - 1) for the finite q of a point inside; 0 for NaN
__device__ __forceinline__ int clamp_idx(float q, int n) {
  if (q >= (float)n) return n - 1;
  return q > 0.f ? (int)q : 0;
}

struct RoiGeom {
  const float* rois;
  const int32_t* roi_batch;  // NULL: all 0
  const float* pts;
  const int32_t* pts_batch;  // NULL: all 0
  int nr, np, ntp;           // RoIs, points, 2048-point tiles per RoI
  int ox, oy, oz;
};

// Flat voxel (x-major, the reference's (out_x, out_y, out_z) layout) of point i in RoI r, or
// -1.  The BEV circle cull cannot reject an inside point: |local| < half diagonal, and the
// margin covers the float rounding of the rotation.
__device__ __forceinline__ int roi_hit(const RoiGeom& g, const Box& b, int rb, float r2, int i) {
  if (g.pts_batch ? g.pts_batch[i] != rb : rb != 0) return -1;
  const float x = g.pts[(size_t)i * 3], y = g.pts[(size_t)i * 3 + 1], z = g.pts[(size_t)i * 3 + 2];
  const float dx = x - b.cx, dy = y - b.cy;
  if (dx * dx + dy * dy > r2) return -1;
  float lx, ly;
  if (!pt_in_box(x, y, z, b, lx, ly)) return -1;
  const float xres = b.l / g.ox, yres = b.w / g.oy, zres = b.h / g.oz;
  const int ix = clamp_idx((lx + b.l / 2) / xres, g.ox);
  const int iy = clamp_idx((ly + b.w / 2) / yres, g.oy);
  const int iz = clamp_idx((z - b.zb) / zres, g.oz);
  return (ix * g.oy + iy) * g.oz + iz;
}

__device__ __forceinline__ void roi_block_setup(const RoiGeom& g, int& r, int& tile, Box& b,
                                                int& rb, float& r2) {
  r = blockIdx.x / g.ntp;
  tile = blockIdx.x - r * g.ntp;
  b = load_box(g.rois + (size_t)r * 7);
  rb = g.roi_batch ? g.roi_batch[r] : 0;
  r2 = 0.25f * (b.l * b.l + b.w * b.w) * 1.001f + 1e-4f;
}

// step 1: hits of every (RoI, tile) -> tile_start[r * ntp + tile]
__global__ __launch_bounds__(kScanBlock) void roi_count_kernel(RoiGeom g,
                                                               int32_t* __restrict__ tile_start) {
  __shared__ int smem[kScanBlock / 64];
  int r, tile, rb;
  Box b;
  float r2;
  roi_block_setup(g, r, tile, b, rb, r2);
  int s = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    const int i = tile * kScanTile + j * kScanBlock + threadIdx.x;
    if (i < g.np) s += roi_hit(g, b, rb, r2, i) >= 0;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kScanBlock / 64; ++w) t += smem[w];
    tile_start[blockIdx.x] = t;
  }
}

struct ReadI32 {
  const int32_t* a;
  __device__ int operator()(int i) const { return a[i]; }
};
struct WriteI32 {
  int32_t* a;
  __device__ void operator()(int i, int p, int) const { a[i] = p; }
};

// step 2: (key, point) pairs in (RoI, ascending point) order
__global__ __launch_bounds__(kScanBlock) void roi_emit_kernel(RoiGeom g,
                                                              const int32_t* __restrict__ tile_start,
                                                              int nhits, uint64_t* __restrict__ keys,
                                                              int32_t* __restrict__ vals) {
  __shared__ int smem[kScanSmem];
  int r, tile, rb;
  Box b;
  float r2;
  roi_block_setup(g, r, tile, b, rb, r2);
  int cell[kScanItems], v[kScanItems], ex[kScanItems];
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    const int i = tile * kScanTile + j * kScanBlock + threadIdx.x;
    cell[j] = i < g.np ? roi_hit(g, b, rb, r2, i) : -1;
    v[j] = cell[j] >= 0;
  }
  tile_excl_scan(v, ex, smem);
  const int base = tile_start[blockIdx.x];
  const uint64_t vol = (uint64_t)g.ox * g.oy * g.oz;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    const int pos = base + ex[j];
    if (v[j] && pos >= 0 && pos < nhits) {
      keys[pos] = (uint64_t)r * vol + (uint64_t)cell[j];
      vals[pos] = tile * kScanTile + j * kScanBlock + threadIdx.x;
    }
  }
}

template <typename K>
__device__ __forceinline__ int lower_bound(const K* __restrict__ a, int n, K x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// step 3: vox_start[c] = first sorted hit of cell c, c in [0, ncells] (the last = nhits)
__global__ __launch_bounds__(256) void roi_vox_start(const uint64_t* __restrict__ skeys, int nhits,
                                                     long ncells, int32_t* __restrict__ vox_start) {
  for (long c = (long)blockIdx.x * 256 + threadIdx.x; c <= ncells; c += (long)gridDim.x * 256)
    vox_start[c] = lower_bound<uint64_t>(skeys, nhits, (uint64_t)c);
}

// step 4a: kept hits keyed by their point (dropped ones by num_points: they sort last)
__global__ __launch_bounds__(256) void roi_inv_keys(const uint64_t* __restrict__ skeys,
                                                    const int32_t* __restrict__ spts, int nhits,
                                                    const int32_t* __restrict__ vox_start, int cap,
                                                    int np, uint32_t* __restrict__ k2,
                                                    uint64_t* __restrict__ v2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nhits) return;
  const uint64_t c = skeys[i];
  const bool kept = i - vox_start[c] < cap;
  k2[i] = kept ? (uint32_t)spts[i] : (uint32_t)np;
  v2[i] = c;
}

// step 4b: pt_start[p] = first inverse entry of point p, p in [0, np]
__global__ __launch_bounds__(256) void roi_pt_start(const uint32_t* __restrict__ sk2, int nhits,
                                                    int np, int32_t* __restrict__ pt_start) {
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p <= np; p += (long)gridDim.x * 256)
    pt_start[p] = lower_bound<uint32_t>(sk2, nhits, (uint32_t)p);
}

inline int grid_of(long work) {
  long b = (work + 255) / 256;
  if (b > 8192) b = 8192;
  return (int)(b > 0 ? b : 1);
}

// radix-sort end bit for keys < v (at least one bit)
inline int sort_bits(long v) {
  const int b = next_pow2_bits(v);
  return b < 1 ? 1 : b;
}

// ---- feature half ----------------------------------------------------------------------
// (cell, channel) threads over the index; mode 0 max (+ argmax), 1 avg.  ref_writes: write
// only where the reference does (max: pooled where a point won, argmax always; avg: pooled
// where count > 0) -- the shim's in-place contract; otherwise every element is written.
__global__ __launch_bounds__(256) void roi_pool_kernel(const float* __restrict__ feats, int c,
                                                       const int32_t* __restrict__ hit_pts,
                                                       const int32_t* __restrict__ vox_start,
                                                       long ncells, int cap, int mode,
                                                       int ref_writes, float* __restrict__ pooled,
                                                       int32_t* __restrict__ argmax) {
  const long total = ncells * c;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const long cell = t / c;
    const int ch = (int)(t - cell * c);
    const int s = vox_start[cell];
    int n = vox_start[cell + 1] - s;
    n = n < cap ? n : cap;
    if (mode == 0) {
      float mx = -INFINITY;
      int arg = -1;
      for (int k = 0; k < n; ++k) {
        const int p = hit_pts[s + k];
        const float x = feats[(size_t)p * c + ch];
        if (x > mx) {
          mx = x;
          arg = p;
        }
      }
      if (arg >= 0 || !ref_writes) pooled[t] = arg >= 0 ? mx : 0.f;
      if (argmax) argmax[t] = arg;
    } else {
      float sum = 0.f;
      for (int k = 0; k < n; ++k) sum += feats[(size_t)hit_pts[s + k] * c + ch];
      if (n > 0 || !ref_writes) pooled[t] = n > 0 ? sum / n : 0.f;
    }
  }
}

// (point, channel) threads over the inverse index, hits in ascending RoI order
__global__ __launch_bounds__(256) void roi_pool_bwd_kernel(
    const float* __restrict__ grad_out, int c, const int32_t* __restrict__ vox_start, int cap,
    const uint64_t* __restrict__ inv_cell, const int32_t* __restrict__ pt_start, int np,
    const int32_t* __restrict__ argmax, int mode, int accumulate, float* __restrict__ grad_in) {
  const long total = (long)np * c;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int p = (int)(t / c), ch = (int)(t - (long)p * c);
    const int b = pt_start[p], e = pt_start[p + 1];
    float acc = 0.f;
    for (int j = b; j < e; ++j) {
      const uint64_t cell = inv_cell[j];
      const size_t o = (size_t)cell * c + ch;
      if (mode == 0) {
        if (argmax[o] == p) acc += grad_out[o];
      } else {
        int n = vox_start[cell + 1] - vox_start[cell];
        n = n < cap ? n : cap;
        acc += grad_out[o] * (1.f / fmaxf((float)n, 1.f));
      }
    }
    grad_in[t] = accumulate ? grad_in[t] + acc : acc;
  }
}

// the reference's pts_idx_of_voxels [cells, M]: slot 0 = count, slots 1..count = the points;
// the other slots keep the caller's values
__global__ __launch_bounds__(256) void roi_table_kernel(const int32_t* __restrict__ hit_pts,
                                                        const int32_t* __restrict__ vox_start,
                                                        long ncells, int m,
                                                        int32_t* __restrict__ table) {
  const long total = ncells * m;
  const int cap = m - 1;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const long cell = t / m;
    const int slot = (int)(t - cell * m);
    const int s = vox_start[cell];
    int n = vox_start[cell + 1] - s;
    n = n < cap ? n : cap;
    if (slot == 0)
      table[t] = n;
    else if (slot <= n)
      table[t] = hit_pts[s + slot - 1];
  }
}

// ---- index from a caller's padded table (shim backward) -------------------------------
struct TableCount {  // count of cell i, clamped to [0, m - 1]
  const int32_t* table;
  int m;
  __device__ int operator()(int i) const {
    const int n = table[(size_t)i * m];
    return n < 0 ? 0 : (n > m - 1 ? m - 1 : n);
  }
};

// entries in cell order; points outside [0, np) are left out of the inverse (key np)
__global__ __launch_bounds__(256) void table_entries(const int32_t* __restrict__ table,
                                                     long ncells, int m,
                                                     const int32_t* __restrict__ vox_start, int np,
                                                     int nentries, int32_t* __restrict__ hit_pts,
                                                     uint32_t* __restrict__ k2,
                                                     uint64_t* __restrict__ v2) {
  const long total = ncells * (m - 1);
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const long cell = t / (m - 1);
    const int k = (int)(t - cell * (m - 1));
    const int s = vox_start[cell];
    if (k >= vox_start[cell + 1] - s || s + k >= nentries) continue;
    const int p = table[cell * m + 1 + k];
    hit_pts[s + k] = p;
    k2[s + k] = p >= 0 && p < np ? (uint32_t)p : (uint32_t)np;
    v2[s + k] = (uint64_t)cell;
  }
}

// ---- points in boxes ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void pib_first_kernel(const float* __restrict__ boxes,
                                                        const float* __restrict__ pts, int nb,
                                                        int npts, int32_t* __restrict__ out) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npts) return;
  const float* p = pts + ((size_t)b * npts + i) * 3;
  const float x = p[0], y = p[1], z = p[2];
  int hit = -1;
  for (int k = 0; k < nb; ++k) {
    float lx, ly;
    if (pt_in_box(x, y, z, load_box(boxes + ((size_t)b * nb + k) * 7), lx, ly)) {
      hit = k;
      break;
    }
  }
  out[(size_t)b * npts + i] = hit;
}

// out[b, i, k], k fastest (coalesced stores)
__global__ __launch_bounds__(256) void pib_all_kernel(const float* __restrict__ boxes,
                                                      const float* __restrict__ pts, int nbatch,
                                                      int nb, int npts, int32_t* __restrict__ out) {
  const long total = (long)nbatch * npts * nb;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const long bi = t / nb;
    const int k = (int)(t - bi * nb);
    const long b = bi / npts;
    const float* p = pts + (size_t)bi * 3;
    float lx, ly;
    out[t] = pt_in_box(p[0], p[1], p[2], load_box(boxes + ((size_t)b * nb + k) * 7), lx, ly);
  }
}

struct InvWs {
  uint64_t *keys, *skeys, *v2;
  int32_t* vals;
  uint32_t *k2, *sk2;
  void* cub;
  size_t cub_bytes;
};
template <typename A>
void carve_inv(A& a, InvWs* w, int nhits) {
  const int m = nhits > 0 ? nhits : 1;
  size_t cb1 = 0, cb2 = 0;
  hipcub::DeviceRadixSort::SortPairs(nullptr, cb1, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                     (int32_t*)nullptr, (int32_t*)nullptr, m);
  hipcub::DeviceRadixSort::SortPairs(nullptr, cb2, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                     (uint64_t*)nullptr, (uint64_t*)nullptr, m);
  InvWs v;
  v.keys = a.template take<uint64_t>(m);
  v.skeys = a.template take<uint64_t>(m);
  v.v2 = a.template take<uint64_t>(m);
  v.vals = a.template take<int32_t>(m);
  v.k2 = a.template take<uint32_t>(m);
  v.sk2 = a.template take<uint32_t>(m);
  v.cub_bytes = cb1 > cb2 ? cb1 : cb2;
  v.cub = a.template take<char>(v.cub_bytes);
  if (w) *w = v;
}

// step 4 on (k2, v2): stable sort by point, then the per-point starts
int build_inverse(InvWs& w, int nhits, int np, uint64_t* inv_cell, int32_t* pt_start,
                  hipStream_t st) {
  if (nhits > 0) {
    size_t cb = w.cub_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, w.k2, w.sk2, w.v2, inv_cell, nhits, 0,
                                           sort_bits((long)np + 1), st) != hipSuccess)
      return MSMD_ERR_LAUNCH;
  }
  MSMD_LAUNCH(roi_pt_start, dim3(grid_of((long)np + 1)), dim3(256), 0, st,
              (const uint32_t*)w.sk2, nhits, np, pt_start);
  return MSMD_OK;
}

bool out_ok(int ox, int oy, int oz) {
  return ox >= 1 && ox <= kRoiMaxOut && oy >= 1 && oy <= kRoiMaxOut && oz >= 1 &&
         oz <= kRoiMaxOut;
}

int roi_tiles(int np) { return np > 0 ? ceil_div(np, kScanTile) : 0; }

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT size_t msmd_roiaware_num_tiles(int num_rois, int num_points) {
  if (num_rois < 0 || num_points < 0) return 0;
  return (size_t)num_rois * roi_tiles(num_points);
}

MSMD_EXPORT size_t msmd_roiaware_count_workspace_bytes(int num_rois, int num_points) {
  if (num_rois < 0 || num_points < 0) return 0;
  ArenaSize a;
  a.take<int>(scan_num_tiles((long)num_rois * roi_tiles(num_points)) + 1);
  return a.off;
}

MSMD_EXPORT int msmd_roiaware_count(const float* rois, const int32_t* roi_batch, int num_rois,
                                    const float* pts, const int32_t* pts_batch, int num_points,
                                    int32_t* tile_start, void* workspace, size_t workspace_bytes,
                                    msmd_stream_t stream) {
  if (num_rois < 0 || num_points < 0 || !tile_start || (num_rois > 0 && !rois) ||
      (num_points > 0 && !pts))
    return MSMD_ERR_INVALID_ARG;
  const int ntp = roi_tiles(num_points);
  const long nt = (long)num_rois * ntp;
  if (nt > kRoiMaxBlocks) return MSMD_ERR_UNSUPPORTED;
  Arena a(workspace, workspace_bytes);
  int* tiles = a.take<int>(scan_num_tiles(nt) + 1);
  if (!a.ok()) return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (nt > 0) {
    RoiGeom g{rois, roi_batch, pts, pts_batch, num_rois, num_points, ntp, 1, 1, 1};
    MSMD_LAUNCH(roi_count_kernel, dim3((int)nt), dim3(kScanBlock), 0, st, g, tile_start);
  }
  // in place: every element is read, then written, by the same thread of the apply kernel
  device_scan(ReadI32{tile_start}, WriteI32{tile_start}, (int)nt, tiles, tile_start + nt, -1, st);
  return launch_status();
}

MSMD_EXPORT size_t msmd_roiaware_index_workspace_bytes(int num_hits) {
  if (num_hits < 0) return 0;
  ArenaSize a;
  carve_inv(a, (InvWs*)nullptr, num_hits);
  return a.off;
}

MSMD_EXPORT int msmd_roiaware_index(const float* rois, const int32_t* roi_batch, int num_rois,
                                    const float* pts, const int32_t* pts_batch, int num_points,
                                    int out_x, int out_y, int out_z, int max_pts_per_voxel,
                                    const int32_t* tile_start, int num_hits, int32_t* hit_pts,
                                    int32_t* vox_start, int64_t* inv_cell, int32_t* pt_start,
                                    void* workspace, size_t workspace_bytes,
                                    msmd_stream_t stream) {
  if (!out_ok(out_x, out_y, out_z)) return MSMD_ERR_UNSUPPORTED;
  if (num_rois < 0 || num_points < 0 || num_hits < 0 || max_pts_per_voxel < 1 || !vox_start ||
      !pt_start || (num_rois > 0 && !rois) || (num_points > 0 && !pts) ||
      (num_hits > 0 && (!tile_start || !hit_pts || !inv_cell)))
    return MSMD_ERR_INVALID_ARG;
  const int ntp = roi_tiles(num_points);
  const long nt = (long)num_rois * ntp;
  if (nt > kRoiMaxBlocks) return MSMD_ERR_UNSUPPORTED;
  if (num_hits > 0 && nt == 0) return MSMD_ERR_INVALID_ARG;
  Arena a(workspace, workspace_bytes);
  InvWs w;
  carve_inv(a, &w, num_hits);
  if (!a.ok()) return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const long vol = (long)out_x * out_y * out_z;
  const long ncells = (long)num_rois * vol;
  if (num_hits > 0) {
    RoiGeom g{rois, roi_batch, pts, pts_batch, num_rois, num_points, ntp, out_x, out_y, out_z};
    MSMD_LAUNCH(roi_emit_kernel, dim3((int)nt), dim3(kScanBlock), 0, st, g, tile_start, num_hits,
                w.keys, w.vals);
    size_t cb = w.cub_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, w.keys, w.skeys, w.vals, hit_pts, num_hits,
                                           0, sort_bits(ncells), st) != hipSuccess)
      return MSMD_ERR_LAUNCH;
  }
  MSMD_LAUNCH(roi_vox_start, dim3(grid_of(ncells + 1)), dim3(256), 0, st,
              (const uint64_t*)w.skeys, num_hits, ncells, vox_start);
  if (num_hits > 0)
    MSMD_LAUNCH(roi_inv_keys, dim3(ceil_div(num_hits, 256)), dim3(256), 0, st,
                (const uint64_t*)w.skeys, (const int32_t*)hit_pts, num_hits,
                (const int32_t*)vox_start, max_pts_per_voxel - 1, num_points, w.k2, w.v2);
  const int e = build_inverse(w, num_hits, num_points, (uint64_t*)inv_cell, pt_start, st);
  if (e) return e;
  return launch_status();
}

MSMD_EXPORT int msmd_roiaware_pool_f32(const float* pts_feature, int num_points, int num_channels,
                                       const int32_t* hit_pts, const int32_t* vox_start,
                                       int64_t num_cells, int max_pts_per_voxel, int mode,
                                       int ref_writes, float* pooled, int32_t* argmax,
                                       msmd_stream_t stream) {
  if (num_points < 0 || num_channels < 1 || num_cells < 0 || max_pts_per_voxel < 1 || mode < 0 ||
      mode > 1)
    return MSMD_ERR_INVALID_ARG;
  if (num_cells == 0) return MSMD_OK;
  // hit_pts is read only through non-empty cells: an index without hits (RoIs and points that
  // never meet) has an empty list, whose pointer may be NULL
  if (!vox_start || !pooled || (mode == 0 && ref_writes && !argmax) ||
      (num_points > 0 && !pts_feature))
    return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(roi_pool_kernel, dim3(grid_of(num_cells * num_channels)), dim3(256), 0,
              (hipStream_t)stream, pts_feature, num_channels, hit_pts, vox_start, (long)num_cells,
              max_pts_per_voxel - 1, mode, ref_writes, pooled, mode == 0 ? argmax : nullptr);
  return launch_status();
}

MSMD_EXPORT int msmd_roiaware_pool_bwd_f32(const float* grad_out, int64_t num_cells,
                                           int num_channels, const int32_t* vox_start,
                                           int max_pts_per_voxel, const int64_t* inv_cell,
                                           const int32_t* pt_start, int num_points,
                                           const int32_t* argmax, int mode, int accumulate,
                                           float* grad_in, msmd_stream_t stream) {
  if (num_points < 0 || num_channels < 1 || num_cells < 0 || max_pts_per_voxel < 1 || mode < 0 ||
      mode > 1)
    return MSMD_ERR_INVALID_ARG;
  if (num_points == 0) return MSMD_OK;
  if (!grad_in || !pt_start || !vox_start || (num_cells > 0 && !grad_out) ||
      (mode == 0 && num_cells > 0 && !argmax))
    return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(roi_pool_bwd_kernel, dim3(grid_of((long)num_points * num_channels)), dim3(256), 0,
              (hipStream_t)stream, grad_out, num_channels, vox_start, max_pts_per_voxel - 1,
              (const uint64_t*)inv_cell, pt_start, num_points, argmax, mode, accumulate, grad_in);
  return launch_status();
}

MSMD_EXPORT int msmd_roiaware_write_table(const int32_t* hit_pts, const int32_t* vox_start,
                                          int64_t num_cells, int max_pts_per_voxel,
                                          int32_t* pts_idx_of_voxels, msmd_stream_t stream) {
  if (num_cells < 0 || max_pts_per_voxel < 1) return MSMD_ERR_INVALID_ARG;
  if (num_cells == 0) return MSMD_OK;
  if (!vox_start || !pts_idx_of_voxels) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(roi_table_kernel, dim3(grid_of(num_cells * max_pts_per_voxel)), dim3(256), 0,
              (hipStream_t)stream, hit_pts, vox_start, (long)num_cells, max_pts_per_voxel,
              pts_idx_of_voxels);
  return launch_status();
}

MSMD_EXPORT size_t msmd_roiaware_table_workspace_bytes(int64_t num_cells, int num_entries) {
  if (num_cells < 0 || num_entries < 0) return 0;
  ArenaSize a;
  a.take<int>(scan_num_tiles(num_cells) + 1);
  carve_inv(a, (InvWs*)nullptr, num_entries);
  return a.off;
}

MSMD_EXPORT int msmd_roiaware_table_count(const int32_t* pts_idx_of_voxels, int64_t num_cells,
                                          int max_pts_per_voxel, int32_t* vox_start,
                                          void* workspace, size_t workspace_bytes,
                                          msmd_stream_t stream) {
  if (num_cells < 0 || num_cells >= (1L << 31) - 1 || max_pts_per_voxel < 1 || !vox_start ||
      (num_cells > 0 && !pts_idx_of_voxels))
    return MSMD_ERR_INVALID_ARG;
  Arena a(workspace, workspace_bytes);
  int* tiles = a.take<int>(scan_num_tiles(num_cells) + 1);
  if (!a.ok()) return MSMD_ERR_WORKSPACE;
  device_scan(TableCount{pts_idx_of_voxels, max_pts_per_voxel}, WriteI32{vox_start},
              (int)num_cells, tiles, vox_start + num_cells, -1, (hipStream_t)stream);
  return launch_status();
}

MSMD_EXPORT int msmd_roiaware_table_index(const int32_t* pts_idx_of_voxels, int64_t num_cells,
                                          int max_pts_per_voxel, int num_points, int num_entries,
                                          const int32_t* vox_start, int32_t* hit_pts,
                                          int64_t* inv_cell, int32_t* pt_start, void* workspace,
                                          size_t workspace_bytes, msmd_stream_t stream) {
  if (num_cells < 0 || max_pts_per_voxel < 1 || num_points < 0 || num_entries < 0 ||
      !vox_start || !pt_start || (num_entries > 0 && (!pts_idx_of_voxels || !hit_pts || !inv_cell)))
    return MSMD_ERR_INVALID_ARG;
  Arena a(workspace, workspace_bytes);
  a.take<int>(scan_num_tiles(num_cells) + 1);
  InvWs w;
  carve_inv(a, &w, num_entries);
  if (!a.ok()) return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (num_entries > 0 && max_pts_per_voxel > 1)
    MSMD_LAUNCH(table_entries, dim3(grid_of(num_cells * (max_pts_per_voxel - 1))), dim3(256), 0,
                st, pts_idx_of_voxels, (long)num_cells, max_pts_per_voxel, vox_start, num_points,
                num_entries, hit_pts, w.k2, w.v2);
  const int e = build_inverse(w, num_entries, num_points, (uint64_t*)inv_cell, pt_start, st);
  if (e) return e;
  return launch_status();
}

MSMD_EXPORT int msmd_points_in_boxes_f32(const float* boxes, const float* pts, int batch_size,
                                         int num_boxes, int num_points, int all_hits,
                                         int32_t* out, msmd_stream_t stream) {
  if (batch_size < 0 || num_boxes < 0 || num_points < 0 || batch_size > 65535)
    return MSMD_ERR_INVALID_ARG;
  if (batch_size == 0 || num_points == 0 || (all_hits && num_boxes == 0)) return MSMD_OK;
  if (!pts || !out || (num_boxes > 0 && !boxes)) return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (all_hits)
    MSMD_LAUNCH(pib_all_kernel, dim3(grid_of((long)batch_size * num_points * num_boxes)),
                dim3(256), 0, st, boxes, pts, batch_size, num_boxes, num_points, out);
  else
    MSMD_LAUNCH(pib_first_kernel, dim3(ceil_div(num_points, 256), batch_size), dim3(256), 0, st,
                boxes, pts, num_boxes, num_points, out);
  return launch_status();
}
