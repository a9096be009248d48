// point_sample.hip -- PointFusion's multi-level image sampler for gfx950: every point of every
// sample projected once, four channels-last rows gathered per level, the concatenated
// [N, sum C_l] row written directly; and its deterministic, cell-stationary backward.
//
// Replaces point_sample() and PointFusion.obtain_mlvl_feats' sampling loop
// (mmdet3d/models/fusion_layers/point_fusion.py:10-95, :257-270): per (sample, level)
// apply_3d_transformation (coord_transform.py:7-90), a 4x4 matmul, clamp, two divides, the image
// augmentation, F.grid_sample on an NCHW map, squeeze().t(), one cat per sample and one per batch.
//
// Forward, per point (the library builds with -ffp-contract=off, every line is one rounding):
//   q  = M [x y z 1]          M: the sample's 3x4 matrix (reverse 3-D flow composed with lidar2img)
//   z  = max(q.z, 1e-5)
//   px = q.x / z * scale_x - crop_x;  py likewise;  flip: px = img_w - px
//   per level: gx = px / pad_w * 2 - 1, gy = py / pad_h * 2 - 1, then grid_sample's bilinear
//   unnormalisation (align_corners: (g + 1) / 2 * (size - 1); else ((g + 1) * size - 1) / 2),
//   corners nw, ne, sw, se with weights (x1 - ix)(y1 - iy), (ix - x0)(y1 - iy), (x1 - ix)(iy - y0),
//   (ix - x0)(iy - y0), accumulated in that order from 0; a corner outside the map adds nothing.
//   Bounds are tested on the floats (floor(ix) in [0, W - 1]) before any conversion to integer:
//   points behind the camera divide by 1e-5 and land at 1e8 and beyond.
// Deviation: a point whose pixel coordinate (px, py) is not finite reads zeros in every level and
// takes no part in the backward (torch's grid_sample result for a NaN coordinate depends on the
// backend's float -> int conversion).
//
// Forward kernel: a wave takes kWavePoints consecutive points (16: at N = 36 000 that is 2 250
// waves; with 64 points a wave -- 563 waves -- the same launch measured 0.41 ms instead of 0.14).
// Lane i projects point i (once per point);
// then the wave walks its points, (px, py, sample) broadcast from the owning lane, lanes running
// along the channels of the concatenated row: 16-byte loads / stores for a level whose C_l, column
// offset and row length are multiples of 4 (and 16-byte aligned bases), single floats otherwise.
//
// Backward: a contribution is (point, level, corner), id t = (p L + l) 4 + k.  The index pass
// stores cell[t] (cell_base[l] + (b H_l + y) W_l + x, or -1) and weight[t], inverts by cell with
// msmd_point_inverse_index's stable radix sort (every cell's list in ascending t), and scans the
// number of kChunk-sized pieces of the lists longer than kChunk.  The gradient pass is
// cell-stationary, one wave per list piece, lanes along channels, float32, list order:
//   1. every piece of a long list -> partial[piece] (pieces are separate waves);
//   2. every cell: a short list summed directly, a long one by adding its partials in piece order;
//      an empty list writes exact zeros.
// No float atomics; the result depends on the index alone, not on the grid or arrival order.
#include <math.h>

#include "common.hpp"
#include "scan.hpp"

namespace msmd {
namespace {

constexpr int kMaxLevels = MSMD_POINT_SAMPLE_MAX_LEVELS;
constexpr int kChunk = 64;       // contributions per list piece (= one wave's prefetch)
constexpr int kFwdBlock = 256;   // 4 waves
constexpr int kWavePoints = 16;  // points per wave of the forward (<= 64)
constexpr int kBlockPoints = kFwdBlock / 64 * kWavePoints;

struct FwdLevel {
  const float* map;
  int h, w, c, offset;
  int unit;        // floats per slot: 4 (16-byte path) or 1
  int slot_end;    // running end of this level's slots in the row
};
struct FwdTable {
  FwdLevel lv[kMaxLevels];
  int num_levels, total_slots, row;   // row = sum C_l
};
struct CellTable {
  float* grad[kMaxLevels];
  int h[kMaxLevels], w[kMaxLevels], c[kMaxLevels], offset[kMaxLevels];
  int cell_base[kMaxLevels + 1];
  int num_levels;
};

struct Pixel {
  float x, y;
  int b;        // sample, or -1: not finite / no sample
};

// sample of point p: the last b with sample_start[b] <= p (empty samples are skipped over)
__device__ __forceinline__ int sample_of(const int32_t* __restrict__ sample_start, int nb, int p) {
  int lo = 0, hi = nb;   // invariant: sample_start[lo] <= p < sample_start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (sample_start[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ Pixel project(const float* __restrict__ points, int stride,
                                         const int32_t* __restrict__ sample_start, int nb,
                                         const msmd_point_sample_params* __restrict__ params,
                                         int p) {
  Pixel r;
  const int b = sample_of(sample_start, nb, p);
  const msmd_point_sample_params& s = params[b];
  const float* pt = points + (size_t)p * stride;
  const float x = pt[0], y = pt[1], z = pt[2];
  const float qx = ((s.m[0] * x + s.m[1] * y) + s.m[2] * z) + s.m[3];
  const float qy = ((s.m[4] * x + s.m[5] * y) + s.m[6] * z) + s.m[7];
  const float qz = ((s.m[8] * x + s.m[9] * y) + s.m[10] * z) + s.m[11];
  const float zc = fmaxf(qz, 1e-5f);       // (NaN -> 1e-5, as torch.clamp does not: see below)
  float px = qx / zc * s.scale_x - s.crop_x;
  const float py = qy / zc * s.scale_y - s.crop_y;
  if (s.flip != 0.f) px = s.img_w - px;
  r.x = px;
  r.y = py;
  // qz NaN: torch.clamp keeps the NaN and both coordinates become NaN
  r.b = (isfinite(px) && isfinite(py) && qz == qz) ? b : -1;
  return r;
}

struct Corners {
  float w[4];        // nw, ne, sw, se
  int x0, y0;        // valid only where ok
  bool okx0, okx1, oky0, oky1;
};

__device__ __forceinline__ float unnormalize(float g, int size, int align_corners) {
  return align_corners ? ((g + 1.f) / 2.f) * (float)(size - 1)
                       : ((g + 1.f) * (float)size - 1.f) / 2.f;
}

__device__ __forceinline__ Corners corners_of(float px, float py, float pad_w, float pad_h, int w,
                                              int h, int align_corners) {
  Corners c;
  const float gx = px / pad_w * 2.f - 1.f, gy = py / pad_h * 2.f - 1.f;
  const float ix = unnormalize(gx, w, align_corners), iy = unnormalize(gy, h, align_corners);
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
  c.w[0] = (fx1 - ix) * (fy1 - iy);
  c.w[1] = (ix - fx0) * (fy1 - iy);
  c.w[2] = (fx1 - ix) * (iy - fy0);
  c.w[3] = (ix - fx0) * (iy - fy0);
  // float tests first: |ix| reaches 1e30 (inf too), far outside int
  const float wm = (float)(w - 1), hm = (float)(h - 1);
  c.okx0 = fx0 >= 0.f && fx0 <= wm;
  c.okx1 = fx1 >= 0.f && fx1 <= wm;
  c.oky0 = fy0 >= 0.f && fy0 <= hm;
  c.oky1 = fy1 >= 0.f && fy1 <= hm;
  // in range of at least one corner => fx0 in [-1, w - 1]: safe to convert
  c.x0 = (c.okx0 || c.okx1) ? (int)fx0 : 0;
  c.y0 = (c.oky0 || c.oky1) ? (int)fy0 : 0;
  return c;
}

template <typename V>
__device__ __forceinline__ V vzero();
template <>
__device__ __forceinline__ float vzero<float>() { return 0.f; }
template <>
__device__ __forceinline__ float4 vzero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void vfma(float& a, float v, float w) { a = a + v * w; }
__device__ __forceinline__ void vfma(float4& a, const float4& v, float w) {
  a.x = a.x + v.x * w; a.y = a.y + v.y * w; a.z = a.z + v.z * w; a.w = a.w + v.w * w;
}
__device__ __forceinline__ void vadd(float& a, float v) { a = a + v; }
__device__ __forceinline__ void vadd(float4& a, const float4& v) {
  a.x = a.x + v.x; a.y = a.y + v.y; a.z = a.z + v.z; a.w = a.w + v.w;
}

// one slot of one point's row: V = float4 or float at element `e` of level lv
template <typename V>
__device__ __forceinline__ void sample_slot(const FwdLevel& lv, const Corners& c, int b, int e,
                                            float* __restrict__ orow) {
  V acc = vzero<V>();
  const size_t plane = (size_t)b * lv.h;
  if (c.oky0) {
    const size_t r = (plane + c.y0) * lv.w;
    if (c.okx0) vfma(acc, *(const V*)(lv.map + (r + c.x0) * lv.c + e), c.w[0]);
    if (c.okx1) vfma(acc, *(const V*)(lv.map + (r + c.x0 + 1) * lv.c + e), c.w[1]);
  }
  if (c.oky1) {
    const size_t r = (plane + c.y0 + 1) * lv.w;
    if (c.okx0) vfma(acc, *(const V*)(lv.map + (r + c.x0) * lv.c + e), c.w[2]);
    if (c.okx1) vfma(acc, *(const V*)(lv.map + (r + c.x0 + 1) * lv.c + e), c.w[3]);
  }
  *(V*)(orow + lv.offset + e) = acc;
}

__global__ __launch_bounds__(kFwdBlock) void point_sample_fwd_kernel(
    const float* __restrict__ points, int stride, int n, const int32_t* __restrict__ sample_start,
    int nb, const msmd_point_sample_params* __restrict__ params, const FwdTable t,
    int align_corners, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int base = (blockIdx.x * (kFwdBlock / 64) + (threadIdx.x >> 6)) * kWavePoints;
  if (base >= n) return;
  const int cnt = min(kWavePoints, n - base);
  Pixel mine;
  mine.x = mine.y = 0.f;
  mine.b = -1;
  if (lane < cnt) mine = project(points, stride, sample_start, nb, params, base + lane);
  for (int j = 0; j < cnt; ++j) {
    const float px = __shfl(mine.x, j, 64), py = __shfl(mine.y, j, 64);
    const int b = __shfl(mine.b, j, 64);
    float* orow = out + (size_t)(base + j) * t.row;
    float pad_w = 1.f, pad_h = 1.f;
    if (b >= 0) {
      pad_w = params[b].pad_w;
      pad_h = params[b].pad_h;
    }
    for (int s = lane; s < t.total_slots; s += 64) {
      int l = 0;
      while (l < t.num_levels - 1 && s >= t.lv[l].slot_end) ++l;
      const FwdLevel& lv = t.lv[l];
      const int e = (s - (l ? t.lv[l - 1].slot_end : 0)) * lv.unit;
      if (b < 0) {
        if (lv.unit == 4) *(float4*)(orow + lv.offset + e) = vzero<float4>();
        else orow[lv.offset + e] = 0.f;
        continue;
      }
      const Corners c = corners_of(px, py, pad_w, pad_h, lv.w, lv.h, align_corners);
      if (lv.unit == 4) sample_slot<float4>(lv, c, b, e, orow);
      else sample_slot<float>(lv, c, b, e, orow);
    }
  }
}

// thread per (point, level): the four contributions' cells and weights
__global__ __launch_bounds__(256) void point_sample_cells_kernel(
    const float* __restrict__ points, int stride, int n, const int32_t* __restrict__ sample_start,
    int nb, const msmd_point_sample_params* __restrict__ params, const CellTable t,
    int align_corners, int32_t* __restrict__ cell, float* __restrict__ weight) {
  const long total = (long)n * t.num_levels;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int p = (int)(i / t.num_levels), l = (int)(i - (long)p * t.num_levels);
    const Pixel px = project(points, stride, sample_start, nb, params, p);
    int32_t ce[4] = {-1, -1, -1, -1};
    float we[4] = {0.f, 0.f, 0.f, 0.f};
    if (px.b >= 0) {
      const Corners c = corners_of(px.x, px.y, params[px.b].pad_w, params[px.b].pad_h, t.w[l],
                                   t.h[l], align_corners);
      const int rowbase = t.cell_base[l] + px.b * t.h[l] * t.w[l];
      const bool ok[4] = {c.oky0 && c.okx0, c.oky0 && c.okx1, c.oky1 && c.okx0,
                          c.oky1 && c.okx1};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (ok[k]) {
          ce[k] = rowbase + (c.y0 + (k >> 1)) * t.w[l] + c.x0 + (k & 1);
          we[k] = c.w[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      cell[i * 4 + k] = ce[k];
      weight[i * 4 + k] = we[k];
    }
  }
}

// pieces of the lists longer than kChunk (short lists need no partial)
struct PieceCount {
  const int32_t* start;
  __device__ int operator()(int i) const {
    const int len = start[i + 1] - start[i];
    return len > kChunk ? (len + kChunk - 1) / kChunk : 0;
  }
};

__device__ __forceinline__ int level_of_cell(const CellTable& t, int cell) {
  int l = 0;
  while (l < t.num_levels - 1 && cell >= t.cell_base[l + 1]) ++l;
  return l;
}

// sum of weight * grad_out over list positions [lo, hi), hi - lo <= kChunk, for the channel
// slots of this lane: lane i prefetches entry i, the walk broadcasts it.  The wave is converged.
template <typename V>
__device__ __forceinline__ void sum_piece(const int32_t* __restrict__ order,
                                          const float* __restrict__ weight,
                                          const float* __restrict__ grad_out, int row, int col0,
                                          int nslot, int per_point, int lo, int hi, int lane,
                                          V& acc) {
  constexpr int U = sizeof(V) / sizeof(float);
  int d = 0;
  float wv = 0.f;
  if (lo + lane < hi) {
    d = order[lo + lane];
    wv = weight[d];
  }
  const int cnt = hi - lo;
  for (int j = 0; j < cnt; ++j) {
    const int dj = __shfl(d, j, 64);
    const float wj = __shfl(wv, j, 64);
    const float* g = grad_out + (size_t)(dj / per_point) * row + col0;
    if (lane < nslot) vfma(acc, *(const V*)(g + lane * U), wj);
  }
}

// channel slots are walked in tiles of 64; C_l beyond one tile loops
template <typename V>
__global__ __launch_bounds__(256) void point_sample_partial_kernel(
    const int32_t* __restrict__ start, const int32_t* __restrict__ piece_start,
    const int32_t* __restrict__ order, const float* __restrict__ weight,
    const float* __restrict__ grad_out, const CellTable t, int row, int cells, int cmax,
    float* __restrict__ partial) {
  constexpr int U = sizeof(V) / sizeof(float);
  const int lane = threadIdx.x & 63;
  const int piece = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (piece >= piece_start[cells]) return;
  int lo = 0, hi = cells;   // piece_start[lo] <= piece < piece_start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (piece_start[mid] <= piece) lo = mid; else hi = mid;
  }
  // equal prefixes (cells without pieces) sit before the owner: the search lands on the last
  // cell whose prefix is <= piece, which is the owner
  const int cell = lo, l = level_of_cell(t, cell);
  const int j = piece - piece_start[cell];
  const int a = start[cell] + j * kChunk, b = min(start[cell + 1], a + kChunk);
  const int nslot = t.c[l] / U;
  float* dst = partial + (size_t)piece * cmax;
  for (int s0 = 0; s0 < nslot; s0 += 64) {
    V acc = vzero<V>();
    sum_piece<V>(order, weight, grad_out, row, t.offset[l] + s0 * U, nslot - s0,
                    t.num_levels * 4, a, b, lane, acc);
    if (s0 + lane < nslot) *(V*)(dst + (s0 + lane) * U) = acc;
  }
}

template <typename V>
__global__ __launch_bounds__(256) void point_sample_cell_kernel(
    const int32_t* __restrict__ start, const int32_t* __restrict__ piece_start,
    const int32_t* __restrict__ order, const float* __restrict__ weight,
    const float* __restrict__ grad_out, const CellTable t, int row, int cells, int cmax,
    const float* __restrict__ partial) {
  constexpr int U = sizeof(V) / sizeof(float);
  const int lane = threadIdx.x & 63;
  const int nwaves = gridDim.x * 4;
  for (int cell = blockIdx.x * 4 + (threadIdx.x >> 6); cell < cells; cell += nwaves) {
    const int l = level_of_cell(t, cell);
    const int lo = start[cell], hi = start[cell + 1];
    const int nslot = t.c[l] / U;
    float* dst = t.grad[l] + (size_t)(cell - t.cell_base[l]) * t.c[l];
    for (int s0 = 0; s0 < nslot; s0 += 64) {
      V acc = vzero<V>();
      if (hi - lo > kChunk) {
        const int p0 = piece_start[cell], p1 = piece_start[cell + 1];
        if (s0 + lane < nslot)
          for (int p = p0; p < p1; ++p)
            vadd(acc, *(const V*)(partial + (size_t)p * cmax + (s0 + lane) * U));
      } else if (hi > lo) {
        sum_piece<V>(order, weight, grad_out, row, t.offset[l] + s0 * U, nslot - s0,
                        t.num_levels * 4, lo, hi, lane, acc);
      }
      if (s0 + lane < nslot) *(V*)(dst + (s0 + lane) * U) = acc;
    }
  }
}

// ---- host side -----------------------------------------------------------------------------
struct Shape {
  long cells, contribs;
  int row, cmax;
  int cell_base[kMaxLevels + 1];
};

int check_levels(const msmd_point_sample_level* levels, int num_levels, int nb, int n,
                 bool need_map, Shape* sh) {
  if (!levels || num_levels < 1 || num_levels > kMaxLevels || nb < 1 || n < 0)
    return MSMD_ERR_INVALID_ARG;
  long cells = 0, row = 0;
  int cmax = 0;
  for (int l = 0; l < num_levels; ++l) {
    const msmd_point_sample_level& lv = levels[l];
    if (lv.c < 1 || lv.h < 1 || lv.w < 1 || (need_map && !lv.map)) return MSMD_ERR_INVALID_ARG;
    if (lv.offset != row) return MSMD_ERR_INVALID_ARG;   // levels tile the row, in order
    if (cells < (1L << 31)) sh->cell_base[l] = (int)cells;
    cells += (long)nb * lv.h * lv.w;
    if (cells >= (1L << 31)) return MSMD_ERR_UNSUPPORTED;
    row += lv.c;
    if (row >= (1L << 31)) return MSMD_ERR_UNSUPPORTED;
    cmax = lv.c > cmax ? lv.c : cmax;
  }
  sh->cell_base[num_levels] = (int)cells;
  sh->cells = cells;
  sh->row = (int)row;
  sh->cmax = cmax;
  sh->contribs = (long)n * num_levels * 4;
  if (sh->contribs >= (1L << 31)) return MSMD_ERR_UNSUPPORTED;
  return MSMD_OK;
}

int check_starts(const int32_t* sample_start_host, int nb, int n) {
  if (!sample_start_host) return MSMD_ERR_INVALID_ARG;
  if (sample_start_host[0] != 0 || sample_start_host[nb] != n) return MSMD_ERR_INVALID_ARG;
  for (int b = 0; b < nb; ++b)
    if (sample_start_host[b + 1] < sample_start_host[b]) return MSMD_ERR_INVALID_ARG;
  return MSMD_OK;
}

void fill_cells(const msmd_point_sample_level* levels, int num_levels, const Shape& sh,
                CellTable* t) {
  t->num_levels = num_levels;
  for (int l = 0; l < kMaxLevels; ++l) {
    const bool on = l < num_levels;
    t->grad[l] = on ? (float*)levels[l].map : nullptr;
    t->h[l] = on ? levels[l].h : 1;
    t->w[l] = on ? levels[l].w : 1;
    t->c[l] = on ? levels[l].c : 1;
    t->offset[l] = on ? levels[l].offset : 0;
    t->cell_base[l] = on ? sh.cell_base[l] : (int)sh.cells;
  }
  t->cell_base[kMaxLevels] = (int)sh.cells;
  t->cell_base[num_levels] = (int)sh.cells;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// an upper bound of the pieces of long lists: a list of len > kChunk has fewer than
// 2 len / kChunk pieces
inline long max_pieces(long contribs) { return 2 * contribs / kChunk + 1; }

struct IndexWs {
  int* tile_sums;
  void* inv;
  size_t inv_bytes;
};
template <typename A>
void carve_index(A& a, IndexWs* w, const Shape& sh) {
  IndexWs v;
  v.tile_sums = a.template take<int>(scan_num_tiles(sh.cells) + 1);
  v.inv_bytes = msmd_point_inverse_index_workspace_bytes(1, (int)sh.contribs);
  v.inv = a.template take<char>(v.inv_bytes);
  if (w) *w = v;
}

inline int grid_of(long work, int per_block, int cap) {
  long b = (work + per_block - 1) / per_block;
  if (b > cap) b = cap;
  return (int)(b > 0 ? b : 1);
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_point_sample_bwd_chunk(void) { return kChunk; }

MSMD_EXPORT int msmd_point_sample_fwd_f32(const float* points, int point_stride, int num_points,
                                          const int32_t* sample_start,
                                          const int32_t* sample_start_host, int batch,
                                          const msmd_point_sample_params* params,
                                          const msmd_point_sample_level* levels, int num_levels,
                                          int align_corners, float* out, msmd_stream_t stream) {
  Shape sh;
  if (int s = check_levels(levels, num_levels, batch, num_points, true, &sh)) return s;
  if (int s = check_starts(sample_start_host, batch, num_points)) return s;
  if (point_stride < 3) return MSMD_ERR_INVALID_ARG;
  if (num_points == 0) return MSMD_OK;
  if (!points || !sample_start || !params || !out) return MSMD_ERR_INVALID_ARG;
  FwdTable t{};
  t.num_levels = num_levels;
  t.row = sh.row;
  int slots = 0;
  for (int l = 0; l < num_levels; ++l) {
    FwdLevel& f = t.lv[l];
    f.map = levels[l].map;
    f.h = levels[l].h;
    f.w = levels[l].w;
    f.c = levels[l].c;
    f.offset = levels[l].offset;
    const bool vec = f.c % 4 == 0 && f.offset % 4 == 0 && sh.row % 4 == 0 && aligned16(f.map) &&
                     aligned16(out);
    f.unit = vec ? 4 : 1;
    slots += f.c / f.unit;
    f.slot_end = slots;
  }
  t.total_slots = slots;
  MSMD_LAUNCH(point_sample_fwd_kernel, dim3(ceil_div(num_points, kBlockPoints)), dim3(kFwdBlock), 0,
              (hipStream_t)stream, points, point_stride, num_points, sample_start, batch, params,
              t, align_corners ? 1 : 0, out);
  return launch_status();
}

MSMD_EXPORT size_t msmd_point_sample_index_workspace_bytes(const msmd_point_sample_level* levels,
                                                           int num_levels, int batch,
                                                           int num_points) {
  Shape sh;
  if (check_levels(levels, num_levels, batch, num_points, false, &sh)) return 0;
  ArenaSize a;
  carve_index(a, nullptr, sh);
  return a.off;
}

MSMD_EXPORT int msmd_point_sample_index(const float* points, int point_stride, int num_points,
                                        const int32_t* sample_start,
                                        const int32_t* sample_start_host, int batch,
                                        const msmd_point_sample_params* params,
                                        const msmd_point_sample_level* levels, int num_levels,
                                        int align_corners, int32_t* cell, float* weight,
                                        int32_t* start, int32_t* order, int32_t* piece_start,
                                        void* workspace, size_t workspace_bytes,
                                        msmd_stream_t stream) {
  Shape sh;
  if (int s = check_levels(levels, num_levels, batch, num_points, false, &sh)) return s;
  if (int s = check_starts(sample_start_host, batch, num_points)) return s;
  if (point_stride < 3) return MSMD_ERR_INVALID_ARG;
  if (!start || !piece_start || !workspace) return MSMD_ERR_INVALID_ARG;
  if (num_points > 0 && (!points || !sample_start || !params || !cell || !weight || !order))
    return MSMD_ERR_INVALID_ARG;
  Arena a(workspace, workspace_bytes);
  IndexWs w;
  carve_index(a, &w, sh);
  if (!a.ok()) return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  CellTable t;
  fill_cells(levels, num_levels, sh, &t);
  if (num_points > 0)
    MSMD_LAUNCH(point_sample_cells_kernel, dim3(grid_of((long)num_points * num_levels, 256, 8192)),
                dim3(256), 0, st, points, point_stride, num_points, sample_start, batch, params, t,
                align_corners ? 1 : 0, cell, weight);
  if (int e = launch_status()) return e;
  // by-cell inverse on the stable radix sort of the PointNet++ backward: cell -1 sorts behind
  // every cell and belongs to no list
  if (int s = msmd_point_inverse_index(cell, 1, (int)sh.cells, (int)sh.contribs, start, order,
                                       w.inv, w.inv_bytes, stream))
    return s;
  device_scan(PieceCount{start}, StorePrefix{piece_start}, (int)sh.cells, w.tile_sums,
              piece_start + sh.cells, -1, st);
  return launch_status();
}

MSMD_EXPORT size_t msmd_point_sample_bwd_workspace_bytes(const msmd_point_sample_level* levels,
                                                         int num_levels, int batch,
                                                         int num_points) {
  Shape sh;
  if (check_levels(levels, num_levels, batch, num_points, false, &sh)) return 0;
  return align_up((size_t)max_pieces(sh.contribs) * sh.cmax * sizeof(float));
}

MSMD_EXPORT int msmd_point_sample_bwd_f32(const float* grad_out, int num_points, int batch,
                                          const msmd_point_sample_level* grad_levels,
                                          int num_levels, const float* weight,
                                          const int32_t* start, const int32_t* order,
                                          const int32_t* piece_start, void* workspace,
                                          size_t workspace_bytes, msmd_stream_t stream) {
  Shape sh;
  if (int s = check_levels(grad_levels, num_levels, batch, num_points, true, &sh)) return s;
  if (!start || !piece_start || !workspace) return MSMD_ERR_INVALID_ARG;
  if (num_points > 0 && (!grad_out || !weight || !order)) return MSMD_ERR_INVALID_ARG;
  const size_t need = align_up((size_t)max_pieces(sh.contribs) * sh.cmax * sizeof(float));
  if (workspace_bytes < need || ((uintptr_t)workspace & 255)) return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  CellTable t;
  fill_cells(grad_levels, num_levels, sh, &t);
  float* partial = (float*)workspace;
  bool vec = sh.row % 4 == 0 && aligned16(grad_out) && sh.cmax % 4 == 0;
  for (int l = 0; l < num_levels; ++l)
    vec = vec && t.c[l] % 4 == 0 && t.offset[l] % 4 == 0 && aligned16(t.grad[l]);
  const int pieces = (int)max_pieces(sh.contribs);
  const int cells = (int)sh.cells;
  if (vec) {
    if (num_points > 0)
      MSMD_LAUNCH(point_sample_partial_kernel<float4>, dim3(ceil_div(pieces, 4)), dim3(256), 0, st,
                  start, piece_start, order, weight, grad_out, t, sh.row, cells, sh.cmax, partial);
    MSMD_LAUNCH(point_sample_cell_kernel<float4>, dim3(grid_of(cells, 4, 1 << 16)), dim3(256), 0,
                st, start, piece_start, order, weight, grad_out, t, sh.row, cells, sh.cmax,
                (const float*)partial);
  } else {
    if (num_points > 0)
      MSMD_LAUNCH(point_sample_partial_kernel<float>, dim3(ceil_div(pieces, 4)), dim3(256), 0, st,
                  start, piece_start, order, weight, grad_out, t, sh.row, cells, sh.cmax, partial);
    MSMD_LAUNCH(point_sample_cell_kernel<float>, dim3(grid_of(cells, 4, 1 << 16)), dim3(256), 0,
                st, start, piece_start, order, weight, grad_out, t, sh.row, cells, sh.cmax,
                (const float*)partial);
  }
  return launch_status();
}
