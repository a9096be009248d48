// pointnet.hip -- the PointNet++ op family for gfx950: gather_points, group_points, three_nn,
// three_interpolate, knn, furthest point sampling on a distance matrix, and one deterministic
// backward for the three differentiable ops.
//
// Replaces gather_points_ext, group_points_ext, interpolate_ext, knn_ext and
// furthest_point_sample_ext.furthest_point_sampling_with_dist_wrapper (mmdet3d/ops/
// {gather_points,group_points,interpolate,knn,furthest_point_sample}/src).  Layouts are the
// reference's: features (B, C, N) channel-major, xyz (B, N, 3), indices int32.
//
// Forward, element by element (the library builds with -ffp-contract=off):
//   gather / group   out[b, c, j] = feat[b, c, idx[b, j]], j over npoint (* nsample); a plain
//                    copy (NaN / inf pass through).  An index outside [0, N) reads as 0 (the
//                    reference reads out of bounds).
//   three_nn         d = (dx*dx + dy*dy) + dz*dz in float32; strict <, so the lowest index
//                    wins a tie; fewer than 3 known points leave index 0 and distance +inf (the
//                    reference's double 1e40 stored as float).  dist2 is the SQUARED distance.
//   three_interpolate  out[b, c, n] = (w0*f[i0] + w1*f[i1]) + w2*f[i2].
//   knn              the k nearest of N points per centre, ordered by (d2, index) ascending --
//                    what the reference's stable insertion sort leaves (knn_cuda.cu:104-166).
//                    d2 as in three_nn; the reference's chained `ssd += tmp*tmp` may be
//                    contracted by its compiler, so d2 is not claimed bit-equal to it (the
//                    ORDER is, wherever distances differ by more than that rounding).
//                    No [N x npoint] matrix: xyz tiles go through LDS, each lane owns one
//                    centre and keeps its sorted top-k as packed (d2 bits, index) words in LDS.
//                    Built for 1 <= k <= 128 (kKnnMaxK); k > N is refused.
//   fps with dist    furthest_point_sample_cuda.cu:214-330: first index 0, running minimum
//                    against row `old` of the (B, N, N) matrix, tie order of the reference's
//                    block reduction (fps_order.hpp, shared with the coordinate form).
//
// Backward of gather / group / three_interpolate is ONE operation: source point (b, n) sums
// w_j * grad_out[b, c, dest_j] over the destinations j whose index names it (w == 1 for the
// first two).  The reference scatters with float atomicAdd; here
//   1. msmd_point_inverse_index keys every destination by its source, in ascending flattened
//      destination position, and sorts the keys with a STABLE radix sort: each source's list
//      holds its destinations in ascending position, independent of any arrival order;
//      src_start[] are binary searches on the sorted keys;
//   2. msmd_point_scatter_bwd_f32 runs one thread per (b, c, n) that walks its list in order
//      and accumulates in float32 with a compensation term (Kahan: y = w * g - comp,
//      sum = acc + y, comp = (sum - acc) - y).  Ball query pads groups with the first hit, so
//      lists of hundreds to thousands of destinations are normal, and a plain running
//      float32 sum over 8192 terms measured 5x the error of torch's index_add_; the
//      compensated walk stays within an ulp or two of the float64 sum.  Lanes run along n.
// No float atomics anywhere: bitwise reproducible.  The inverse depends on the index tensor
// only; callers build it once per index tensor and reuse it for every backward.
#include <hipcub/hipcub.hpp>
#include <math.h>

#include "common.hpp"
#include "fps_order.hpp"

namespace msmd {
namespace {

constexpr int kColTile = 8;      // channels per workgroup of the gather-type kernels
constexpr int kBwdTile = 4;      // channels per thread of the backward
constexpr int kNnTile = 1024;    // known points per LDS tile of three_nn
constexpr int kKnnTile = 512;    // points per LDS tile of knn
constexpr int kKnnMaxK = 128;
constexpr int kMaxGridYZ = 65535;

// out[b, ch, j] = feat[b, ch, idx[b, j]]: lanes along j (coalesced stores), idx loaded once
// per thread and reused over kColTile channels
__global__ __launch_bounds__(256) void gather_cols_kernel(const float* __restrict__ feat,
                                                          const int32_t* __restrict__ idx, int c,
                                                          int n, int m, float* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const int b = blockIdx.z, c0 = blockIdx.y * kColTile;
  const int i = idx[(size_t)b * m + j];
  const bool ok = (unsigned)i < (unsigned)n;
#pragma unroll
  for (int t = 0; t < kColTile; ++t) {
    const int ch = c0 + t;
    if (ch >= c) break;
    const size_t plane = (size_t)b * c + ch;
    out[plane * m + j] = ok ? feat[plane * n + i] : 0.f;
  }
}

__global__ __launch_bounds__(256) void three_interpolate_kernel(
    const float* __restrict__ feat, const int32_t* __restrict__ idx,
    const float* __restrict__ weight, int c, int m, int n, float* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int b = blockIdx.z, c0 = blockIdx.y * kColTile;
  const size_t o = ((size_t)b * n + j) * 3;
  const int i0 = idx[o], i1 = idx[o + 1], i2 = idx[o + 2];
  const float w0 = weight[o], w1 = weight[o + 1], w2 = weight[o + 2];
  const bool ok0 = (unsigned)i0 < (unsigned)m, ok1 = (unsigned)i1 < (unsigned)m,
             ok2 = (unsigned)i2 < (unsigned)m;
#pragma unroll
  for (int t = 0; t < kColTile; ++t) {
    const int ch = c0 + t;
    if (ch >= c) break;
    const size_t plane = (size_t)b * c + ch;
    const float* f = feat + plane * m;
    const float f0 = ok0 ? f[i0] : 0.f, f1 = ok1 ? f[i1] : 0.f, f2 = ok2 ? f[i2] : 0.f;
    out[plane * n + j] = (w0 * f0 + w1 * f1) + w2 * f2;
  }
}

// one thread per unknown point; the known points of the batch element pass through LDS once
// per workgroup (all lanes read the same LDS word: a broadcast)
__global__ __launch_bounds__(256) void three_nn_kernel(const float* __restrict__ unknown,
                                                       const float* __restrict__ known, int n,
                                                       int m, float* __restrict__ dist2,
                                                       int32_t* __restrict__ idx) {
  __shared__ float tile[kNnTile * 3];
  const int b = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const bool ok = p < n;
  const size_t o = ((size_t)b * n + (ok ? p : 0)) * 3;
  const float ux = unknown[o], uy = unknown[o + 1], uz = unknown[o + 2];
  known += (size_t)b * m * 3;
  const float kInf = __int_as_float(0x7f800000);
  float best1 = kInf, best2 = kInf, best3 = kInf;
  int i1 = 0, i2 = 0, i3 = 0;
  for (int base = 0; base < m; base += kNnTile) {
    const int cnt = min(kNnTile, m - base);
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * 3; e += 256) tile[e] = known[(size_t)base * 3 + e];
    __syncthreads();
    for (int q = 0; q < cnt; ++q) {
      const float dx = ux - tile[q * 3], dy = uy - tile[q * 3 + 1], dz = uz - tile[q * 3 + 2];
      const float d = (dx * dx + dy * dy) + dz * dz;
      const int k = base + q;
      if (d < best1) {
        best3 = best2; i3 = i2;
        best2 = best1; i2 = i1;
        best1 = d; i1 = k;
      } else if (d < best2) {
        best3 = best2; i3 = i2;
        best2 = d; i2 = k;
      } else if (d < best3) {
        best3 = d; i3 = k;
      }
    }
  }
  if (!ok) return;
  dist2[o] = best1; dist2[o + 1] = best2; dist2[o + 2] = best3;
  idx[o] = i1; idx[o + 1] = i2; idx[o + 2] = i3;
}

// one wave per 64 centres; list[j * 64 + lane] = the lane's j-th smallest (d2 bits << 32 |
// index) so far.  d2 >= +0, so the float bits order as unsigned and the packed word orders by
// (d2, index); a NaN distance sorts behind every number.
__global__ __launch_bounds__(64) void knn_kernel(const float* __restrict__ xyz,
                                                 const float* __restrict__ centers, int n, int m,
                                                 int k, int64_t* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char knn_smem[];
  unsigned long long* list = (unsigned long long*)knn_smem;
  float* tile = (float*)(list + (size_t)k * 64);
  const int lane = threadIdx.x, b = blockIdx.y;
  const int c = blockIdx.x * 64 + lane;
  const bool ok = c < m;
  const size_t co = ((size_t)b * m + (ok ? c : 0)) * 3;
  const float cx = centers[co], cy = centers[co + 1], cz = centers[co + 2];
  xyz += (size_t)b * n * 3;
  for (int j = 0; j < k; ++j) list[j * 64 + lane] = ~0ull;
  unsigned long long worst = ~0ull;
  for (int base = 0; base < n; base += kKnnTile) {
    const int cnt = min(kKnnTile, n - base);
    __syncthreads();
    for (int e = lane; e < cnt * 3; e += 64) tile[e] = xyz[(size_t)base * 3 + e];
    __syncthreads();
    if (!ok) continue;
    for (int q = 0; q < cnt; ++q) {
      const float dx = cx - tile[q * 3], dy = cy - tile[q * 3 + 1], dz = cz - tile[q * 3 + 2];
      const float d = (dx * dx + dy * dy) + dz * dz;
      const unsigned long long key =
          ((unsigned long long)__float_as_uint(d) << 32) | (uint32_t)(base + q);
      if (key < worst) {
        int j = k - 1;
        while (j > 0) {
          const unsigned long long prev = list[(j - 1) * 64 + lane];
          if (prev <= key) break;
          list[j * 64 + lane] = prev;
          --j;
        }
        list[j * 64 + lane] = key;
        worst = list[(k - 1) * 64 + lane];
      }
    }
  }
  if (!ok) return;
  for (int j = 0; j < k; ++j)
    out[((size_t)b * k + j) * m + c] = (int64_t)(uint32_t)list[j * 64 + lane];
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
  int lo = __shfl_xor((int)(uint32_t)v, o, 64), hi = __shfl_xor((int)(v >> 32), o, 64);
  return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) {
  return a > b ? a : b;
}
// (distance, tie rank) as one word whose unsigned maximum is the reference's winner: larger
// distance first (order-preserving map of the float bits, negative values included -- a
// caller's "squared distance" a^2 + b^2 - 2ab may round below zero), then the smaller rank
__device__ __forceinline__ unsigned long long fps_pack(float d, uint32_t rank) {
  const uint32_t u = __float_as_uint(d);
  const uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)ord << 32) | (0xFFFFFFFFu - rank);
}

// One 1024-thread workgroup per batch element.  PPT > 0: the running minima live in registers
// (n <= 1024 * PPT); PPT == 0: any n, in `temp`.  Every reference thread starts from
// (best -1, index 0) and takes a point only when strictly greater: points with a running
// minimum <= -1 (or NaN) never win, and if none does the result is index 0.
template <int PPT>
__global__ __launch_bounds__(1024) void fps_dist_kernel(const float* __restrict__ dist_all, int n,
                                                        int m, float* __restrict__ temp_all,
                                                        int32_t* __restrict__ idx_all) {
  __shared__ unsigned long long red[2][16];
  constexpr int P = PPT > 0 ? PPT : 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* dist = dist_all + (size_t)blockIdx.x * n * n;
  float* temp = temp_all + (size_t)blockIdx.x * n;
  int32_t* idx = idx_all + (size_t)blockIdx.x * m;
  const int bs_shift = fps_block_shift(n);
  float pd[P];
  if (PPT > 0) {
#pragma unroll
    for (int s = 0; s < P; ++s) pd[s] = 1e10f;
  } else {
    for (int k = tid; k < n; k += 1024) temp[k] = 1e10f;   // each thread reads back its own
  }
  if (tid == 0) idx[0] = 0;
  int old = 0;
  const unsigned long long none = fps_pack(-1.f, fps_tie_rank(0, bs_shift));
  for (int j = 1; j < m; ++j) {
    const float* row = dist + (size_t)old * n;
    unsigned long long best = none;
    if (PPT > 0) {
#pragma unroll
      for (int s = 0; s < P; ++s) {
        const int k = tid + 1024 * s;
        if (k < n) {
          const float d2 = fminf(row[k], pd[s]);
          pd[s] = d2;
          if (d2 > -1.f) best = umax64(best, fps_pack(d2, fps_tie_rank(k, bs_shift)));
        }
      }
    } else {
      for (int k = tid; k < n; k += 1024) {
        const float d2 = fminf(row[k], temp[k]);
        temp[k] = d2;
        if (d2 > -1.f) best = umax64(best, fps_pack(d2, fps_tie_rank(k, bs_shift)));
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = umax64(best, shfl_xor_u64(best, o));
    const int buf = j & 1;   // double-buffered: one barrier separates write and read
    if (lane == 0) red[buf][wave] = best;
    __syncthreads();
    unsigned long long v = red[buf][lane & 15];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = umax64(v, shfl_xor_u64(v, o));
    old = fps_rank_index(0xFFFFFFFFu - (uint32_t)v, bs_shift);
    if (tid == 0) idx[j] = old;
  }
}

// ---- inverse index + backward ----------------------------------------------------------
__global__ __launch_bounds__(256) void inv_keys_kernel(const int32_t* __restrict__ idx, long total,
                                                       int n, int m, uint32_t sentinel,
                                                       uint32_t* __restrict__ keys,
                                                       int32_t* __restrict__ vals) {
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const long b = t / m;
    const int i = idx[t];
    keys[t] = (unsigned)i < (unsigned)n ? (uint32_t)(b * n + i) : sentinel;
    vals[t] = (int32_t)(t - b * m);
  }
}

__global__ __launch_bounds__(256) void inv_starts_kernel(const uint32_t* __restrict__ skeys,
                                                         int total, long nsrc,
                                                         int32_t* __restrict__ src_start) {
  for (long s = (long)blockIdx.x * 256 + threadIdx.x; s <= nsrc; s += (long)gridDim.x * 256) {
    int lo = 0, hi = total;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (skeys[mid] < (uint32_t)s) lo = mid + 1; else hi = mid;
    }
    src_start[s] = lo;
  }
}

// thread (b, channel tile, n): walks the source's destinations in ascending position.
// grad_out[b, ch, dest / div] (div = 3 for three_interpolate, whose destinations are the
// (point, slot) pairs), weight[b, dest] or 1.
__global__ __launch_bounds__(256) void point_scatter_bwd_kernel(
    const float* __restrict__ grad_out, const float* __restrict__ weight,
    const int32_t* __restrict__ src_start, const int32_t* __restrict__ dest, int c, int n, int m,
    int div, int accumulate, float* __restrict__ grad_in) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  const int b = blockIdx.z, c0 = blockIdx.y * kBwdTile;
  const int lo = src_start[(size_t)b * n + s], hi = src_start[(size_t)b * n + s + 1];
  const int mo = m / div;
  const float* g = grad_out + ((size_t)b * c + c0) * mo;
  const float* w = weight ? weight + (size_t)b * m : nullptr;
  float acc[kBwdTile], comp[kBwdTile];
#pragma unroll
  for (int t = 0; t < kBwdTile; ++t) acc[t] = comp[t] = 0.f;
  for (int j = lo; j < hi; ++j) {
    const int d = dest[j];
    const int pos = div == 1 ? d : d / div;
    const float wj = w ? w[d] : 1.f;
#pragma unroll
    for (int t = 0; t < kBwdTile; ++t)
      if (c0 + t < c) {
        const float gv = g[(size_t)t * mo + pos];
        // compensated (Kahan) step; the build has no fast-math and no contraction, so the
        // four operations stay as written
        const float y = (w ? wj * gv : gv) - comp[t];
        const float sum = acc[t] + y;
        comp[t] = (sum - acc[t]) - y;
        acc[t] = sum;
      }
  }
#pragma unroll
  for (int t = 0; t < kBwdTile; ++t)
    if (c0 + t < c) {
      float* o = grad_in + ((size_t)b * c + c0 + t) * n + s;
      *o = accumulate ? *o + acc[t] : acc[t];
    }
}

inline int grid_of(long work) {
  long b = (work + 255) / 256;
  if (b > 8192) b = 8192;
  return (int)(b > 0 ? b : 1);
}
inline int sort_bits(long v) {
  const int b = next_pow2_bits(v);
  return b < 1 ? 1 : b;
}

struct InvWs {
  uint32_t *keys, *skeys;
  int32_t* vals;
  void* cub;
  size_t cub_bytes;
};
template <typename A>
void carve_inv(A& a, InvWs* w, long total) {
  const int t = total > 0 ? (int)total : 1;
  InvWs v;
  v.cub_bytes = 0;
  hipcub::DeviceRadixSort::SortPairs(nullptr, v.cub_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                     (int32_t*)nullptr, (int32_t*)nullptr, t);
  v.keys = a.template take<uint32_t>(t);
  v.skeys = a.template take<uint32_t>(t);
  v.vals = a.template take<int32_t>(t);
  v.cub = a.template take<char>(v.cub_bytes);
  if (w) *w = v;
}

// shapes the gather-type launches can take: (b, c, src points, dst positions)
int cols_shape_status(int b, int c, int n, int m) {
  if (b < 1 || c < 1 || n < 1 || m < 0) return MSMD_ERR_INVALID_ARG;
  if (b > kMaxGridYZ || ceil_div(c, kBwdTile) > kMaxGridYZ) return MSMD_ERR_UNSUPPORTED;
  return MSMD_OK;
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_gather_points_f32(const float* features, const int32_t* idx, int b, int c,
                                       int n, int npoint, float* out, msmd_stream_t stream) {
  if (int s = cols_shape_status(b, c, n, npoint)) return s;
  if (npoint == 0) return MSMD_OK;
  if (!features || !idx || !out) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(gather_cols_kernel, dim3(ceil_div(npoint, 256), ceil_div(c, kColTile), b),
              dim3(256), 0, (hipStream_t)stream, features, idx, c, n, npoint, out);
  return launch_status();
}

MSMD_EXPORT int msmd_group_points_f32(const float* features, const int32_t* idx, int b, int c,
                                      int n, int npoint, int nsample, float* out,
                                      msmd_stream_t stream) {
  if (npoint < 0 || nsample < 0) return MSMD_ERR_INVALID_ARG;
  const long m = (long)npoint * nsample;
  if (m >= (1L << 31)) return MSMD_ERR_RANGE;
  if (int s = cols_shape_status(b, c, n, (int)m)) return s;
  if (m == 0) return MSMD_OK;
  if (!features || !idx || !out) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(gather_cols_kernel, dim3(ceil_div(m, 256), ceil_div(c, kColTile), b), dim3(256), 0,
              (hipStream_t)stream, features, idx, c, n, (int)m, out);
  return launch_status();
}

MSMD_EXPORT int msmd_three_nn_f32(const float* unknown, const float* known, int b, int n, int m,
                                  float* dist2, int32_t* idx, msmd_stream_t stream) {
  if (b < 1 || n < 0 || m < 0) return MSMD_ERR_INVALID_ARG;
  if (b > kMaxGridYZ) return MSMD_ERR_UNSUPPORTED;
  if (n == 0) return MSMD_OK;
  if (!unknown || (m > 0 && !known) || !dist2 || !idx) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(three_nn_kernel, dim3(ceil_div(n, 256), b), dim3(256), 0, (hipStream_t)stream,
              unknown, known, n, m, dist2, idx);
  return launch_status();
}

MSMD_EXPORT int msmd_three_interpolate_f32(const float* features, const int32_t* idx,
                                           const float* weight, int b, int c, int m, int n,
                                           float* out, msmd_stream_t stream) {
  if (int s = cols_shape_status(b, c, m, n)) return s;
  if (n == 0) return MSMD_OK;
  if (!features || !idx || !weight || !out) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(three_interpolate_kernel, dim3(ceil_div(n, 256), ceil_div(c, kColTile), b),
              dim3(256), 0, (hipStream_t)stream, features, idx, weight, c, m, n, out);
  return launch_status();
}

MSMD_EXPORT int msmd_knn_f32(const float* xyz, const float* center_xyz, int b, int n, int npoint,
                             int k, int64_t* idx, msmd_stream_t stream) {
  if (b < 1 || n < 1 || npoint < 0 || k < 1 || k > n) return MSMD_ERR_INVALID_ARG;
  if (k > kKnnMaxK || b > kMaxGridYZ) return MSMD_ERR_UNSUPPORTED;
  if (npoint == 0) return MSMD_OK;
  if (!xyz || !center_xyz || !idx) return MSMD_ERR_INVALID_ARG;
  const size_t lds = (size_t)k * 64 * sizeof(unsigned long long) + kKnnTile * 3 * sizeof(float);
  static LdsGrant grant;
  if (int s = optin_dynamic_lds((const void*)knn_kernel, lds, grant)) return s;
  MSMD_LAUNCH(knn_kernel, dim3(ceil_div(npoint, 64), b), dim3(64), lds, (hipStream_t)stream, xyz,
              center_xyz, n, npoint, k, idx);
  return launch_status();
}

MSMD_EXPORT int msmd_furthest_point_sample_with_dist(const float* dist, int b, int n, int m,
                                                     float* temp, int32_t* idx,
                                                     msmd_stream_t stream) {
  if (b < 1 || n < 1 || m < 0 || !dist || !idx || !temp) return MSMD_ERR_INVALID_ARG;
  if (m == 0) return MSMD_OK;
  if (n >= (1 << 21)) return MSMD_ERR_RANGE;
  hipStream_t st = (hipStream_t)stream;
  const int ppt = ceil_div(n, 1024);
#define FPSD(P) \
  MSMD_LAUNCH(fps_dist_kernel<P>, dim3(b), dim3(1024), 0, st, dist, n, m, temp, idx)
  if (ppt <= 1) FPSD(1);
  else if (ppt <= 4) FPSD(4);
  else if (ppt <= 16) FPSD(16);
  else FPSD(0);
#undef FPSD
  return launch_status();
}

MSMD_EXPORT size_t msmd_point_inverse_index_workspace_bytes(int b, int m) {
  if (b < 1 || m < 0 || (long)b * m >= (1L << 31)) return 0;
  ArenaSize a;
  carve_inv(a, nullptr, (long)b * m);
  return a.off;
}

MSMD_EXPORT int msmd_point_inverse_index(const int32_t* idx, int b, int n, int m,
                                         int32_t* src_start, int32_t* dest, void* workspace,
                                         size_t workspace_bytes, msmd_stream_t stream) {
  if (b < 1 || n < 1 || m < 0 || !src_start) return MSMD_ERR_INVALID_ARG;
  const long total = (long)b * m, nsrc = (long)b * n;
  if (total >= (1L << 31) || nsrc >= (1L << 31)) return MSMD_ERR_RANGE;
  if (total > 0 && (!idx || !dest || !workspace)) return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  InvWs w{};
  if (total > 0) {
    Arena a(workspace, workspace_bytes);
    carve_inv(a, &w, total);
    if (!a.ok()) return MSMD_ERR_WORKSPACE;
    MSMD_LAUNCH(inv_keys_kernel, dim3(grid_of(total)), dim3(256), 0, st, idx, total, n, m,
                (uint32_t)nsrc, w.keys, w.vals);
    size_t cb = w.cub_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, w.keys, w.skeys, w.vals, dest, (int)total, 0,
                                           sort_bits(nsrc + 1), st) != hipSuccess)
      return MSMD_ERR_LAUNCH;
  }
  MSMD_LAUNCH(inv_starts_kernel, dim3(grid_of(nsrc + 1)), dim3(256), 0, st,
              (const uint32_t*)w.skeys, (int)total, nsrc, src_start);
  return launch_status();
}

MSMD_EXPORT int msmd_point_scatter_bwd_f32(const float* grad_out, const float* weight,
                                           const int32_t* src_start, const int32_t* dest, int b,
                                           int c, int n, int m, int dest_per_out, int accumulate,
                                           float* grad_in, msmd_stream_t stream) {
  if (int s = cols_shape_status(b, c, n, m)) return s;
  if (dest_per_out < 1 || m % dest_per_out != 0) return MSMD_ERR_INVALID_ARG;
  if (!src_start || !grad_in || (m > 0 && (!grad_out || !dest))) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(point_scatter_bwd_kernel, dim3(ceil_div(n, 256), ceil_div(c, kBwdTile), b),
              dim3(256), 0, (hipStream_t)stream, grad_out, weight, src_start, dest, c, n, m,
              dest_per_out, accumulate, grad_in);
  return launch_status();
}
