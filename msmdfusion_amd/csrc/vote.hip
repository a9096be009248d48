// vote.hip -- the VoteNet op family (COVERAGE n4): matrix-free Chamfer distance (forward and
// backward), vote targets and points per box.
//
//   chamfer_min_*      models/losses/chamfer_distance.py:50-55: two [B, N, M, 3] expansions and a
//                      [B, N, M] matrix there, taken down by two torch.min.  Here one lane owns
//                      one query point and walks the other set; nothing of size N x M exists.
//   chamfer_grad_*     autograd through that matrix: one lane owns one output point, adds its
//                      own nearest-neighbour term and then scans the other side's index array
//                      for the points that chose it, in ascending order.  No atomics.
//   vote_targets       VoteHead.get_targets_single (models/dense_heads/vote_head.py:472-501), a
//                      Python loop over ground truths with a nonzero per box and per slot.
//   pib_count          multiclass_nms_single (vote_head.py:617-625): an [N, T] inclusion table
//                      summed over N.
//
// Chamfer, element by element (float32, no contraction): the criterion per coordinate on
// d = q - r (l2: d * d; l1: |d|; smooth_l1, beta 1: (0.5 * |d|) * |d| for |d| < 1 else
// |d| - 0.5), summed (cx + cy) + cz.  The minimum follows torch.min over a dimension: ties go
// to the lowest index, a NaN is smaller than everything and the first NaN wins.  Both
// directions run the same kernel with the roles swapped: q - r and r - q differ in sign only,
// and every criterion is even.
//
// Two shapes per direction, chosen on the host from the sizes alone:
//   tiled  one wavefront per 64 query points of one batch, the other set staged through LDS
//          256 points at a time (every lane reads the same LDS address: a broadcast)
//   flat   fewer than 64 query points per batch (the vote loss: B * num_seed batches of 1 x 3):
//          one lane per (batch, query point) across batches, the few other points read
//          directly -- a workgroup per batch would run one lane in 64
// The backward has the same two shapes and costs what the forward costs.
#include <math.h>

#include "chamfer_common.hpp"
#include "common.hpp"
#include "point_in_box.hpp"

namespace msmd {
namespace {

constexpr int kChamferTile = 256;      // other-set points per LDS tile
constexpr int kChamferFlatMax = 1024;  // flat shape: at most this many other points per batch
constexpr int kVoteGtChunk = 64;       // ground truths per LDS chunk
constexpr int kVoteSlots = 3;          // gt_per_seed of the reference loop (its clamp at 2)

// the criterion's derivative in d = q - r
template <int MODE>
__device__ __forceinline__ float slope(float d) {
  if (MODE == kL2) return __fmul_rn(2.f, d);
  const float sign = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  if (MODE == kL1) return sign;
  return fabsf(d) < 1.f ? d : sign;
}

// grid: batches * ceil(nq / 64) wavefronts
template <int MODE>
__global__ __launch_bounds__(kWave) void chamfer_min_tiled(const float* __restrict__ q, int nq,
                                                          const float* __restrict__ r, int nr,
                                                          float* __restrict__ dist,
                                                          int64_t* __restrict__ index) {
  __shared__ float tile[kChamferTile * 3];
  const int per_batch = (nq + kWave - 1) / kWave;
  const int b = blockIdx.x / per_batch;
  const int i = (blockIdx.x - b * per_batch) * kWave + threadIdx.x;
  const bool live = i < nq;
  float mine[3] = {0.f, 0.f, 0.f};
  if (live) {
    const float* p = q + ((size_t)b * nq + i) * 3;
    mine[0] = p[0], mine[1] = p[1], mine[2] = p[2];
  }
  const float* rb = r + (size_t)b * nr * 3;
  float best = INFINITY;
  int at = 0;
  for (int base = 0; base < nr; base += kChamferTile) {
    const int cnt = min(nr - base, kChamferTile);
    __syncthreads();
    for (int k = threadIdx.x; k < cnt * 3; k += kWave) tile[k] = rb[(size_t)base * 3 + k];
    __syncthreads();
    if (live)
      for (int j = 0; j < cnt; ++j) take_min(distance<MODE>(mine, tile + j * 3), base + j, best, at);
  }
  if (live) {
    dist[(size_t)b * nq + i] = best;
    index[(size_t)b * nq + i] = at;
  }
}

// one lane per (batch, query point), nq < 64
template <int MODE>
__global__ __launch_bounds__(256) void chamfer_min_flat(const float* __restrict__ q, int nq,
                                                        const float* __restrict__ r, int nr,
                                                        long total, float* __restrict__ dist,
                                                        int64_t* __restrict__ index) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long b = t / nq;
  const float mine[3] = {q[t * 3], q[t * 3 + 1], q[t * 3 + 2]};
  const float* rb = r + (size_t)b * nr * 3;
  float best = INFINITY;
  int at = 0;
  for (int j = 0; j < nr; ++j) {
    const float other[3] = {rb[j * 3], rb[j * 3 + 1], rb[j * 3 + 2]};
    take_min(distance<MODE>(mine, other), j, best, at);
  }
  dist[t] = best;
  index[t] = at;
}

// acc += g * slope(mine - other), per coordinate.  The difference is float32 (as the forward
// computed it); the product of two float32 values is exact in double, and the running sum is a
// double: a thousand points that chose one target are summed in ascending order without the
// error of a float32 left fold, and the order still fixes every bit.
template <int MODE>
__device__ __forceinline__ void add_term(float g, const float* mine, const float* other,
                                         double* acc) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
    acc[k] = __dadd_rn(acc[k],
                       __dmul_rn((double)g, (double)slope<MODE>(__fsub_rn(mine[k], other[k]))));
}

// grad of the `own` side: own[b, i] with its chosen other point i_own[b, i] and upstream
// g_own[b, i]; then every other point o (ascending) with i_oth[b, o] == i adds
// g_oth[b, o] * slope(own_i - oth_o).  An index outside its set contributes nothing.
template <int MODE>
__global__ __launch_bounds__(kWave) void chamfer_grad_tiled(
    const float* __restrict__ own, int n_own, const float* __restrict__ oth, int n_oth,
    const float* __restrict__ g_own, const int64_t* __restrict__ i_own,
    const float* __restrict__ g_oth, const int64_t* __restrict__ i_oth,
    float* __restrict__ grad) {
  __shared__ int chose[kChamferTile];
  __shared__ float weight[kChamferTile];
  const int per_batch = (n_own + kWave - 1) / kWave;
  const int b = blockIdx.x / per_batch;
  const int i = (blockIdx.x - b * per_batch) * kWave + threadIdx.x;
  const bool live = i < n_own;
  const float* ob = oth + (size_t)b * n_oth * 3;
  float mine[3] = {0.f, 0.f, 0.f};
  double acc[3] = {0., 0., 0.};
  if (live) {
    const size_t row = (size_t)b * n_own + i;
    mine[0] = own[row * 3], mine[1] = own[row * 3 + 1], mine[2] = own[row * 3 + 2];
    const int64_t at = i_own[row];
    if (at >= 0 && at < n_oth) add_term<MODE>(g_own[row], mine, ob + at * 3, acc);
  }
  for (int base = 0; base < n_oth; base += kChamferTile) {
    const int cnt = min(n_oth - base, kChamferTile);
    __syncthreads();
    for (int k = threadIdx.x; k < cnt; k += kWave) {
      const int64_t at = i_oth[(size_t)b * n_oth + base + k];
      chose[k] = at >= 0 && at < n_own ? (int)at : -1;
      weight[k] = g_oth[(size_t)b * n_oth + base + k];
    }
    __syncthreads();
    if (live)
      for (int j = 0; j < cnt; ++j)
        if (chose[j] == i) add_term<MODE>(weight[j], mine, ob + (size_t)(base + j) * 3, acc);
  }
  if (live) {
    float* out = grad + ((size_t)b * n_own + i) * 3;
    out[0] = (float)acc[0], out[1] = (float)acc[1], out[2] = (float)acc[2];
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void chamfer_grad_flat(
    const float* __restrict__ own, int n_own, const float* __restrict__ oth, int n_oth,
    long total, const float* __restrict__ g_own, const int64_t* __restrict__ i_own,
    const float* __restrict__ g_oth, const int64_t* __restrict__ i_oth,
    float* __restrict__ grad) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long b = t / n_own;
  const int i = (int)(t - b * n_own);
  const float* ob = oth + (size_t)b * n_oth * 3;
  const float mine[3] = {own[t * 3], own[t * 3 + 1], own[t * 3 + 2]};
  double acc[3] = {0., 0., 0.};
  const int64_t at = i_own[t];
  if (at >= 0 && at < n_oth) add_term<MODE>(g_own[t], mine, ob + at * 3, acc);
  for (int j = 0; j < n_oth; ++j)
    if (i_oth[(size_t)b * n_oth + j] == i)
      add_term<MODE>(g_oth[(size_t)b * n_oth + j], mine, ob + (size_t)j * 3, acc);
  grad[t * 3] = (float)acc[0], grad[t * 3 + 1] = (float)acc[1], grad[t * 3 + 2] = (float)acc[2];
}

inline bool flat_shape(int n_query, int n_other) {
  return n_query < kWave && n_other <= kChamferFlatMax;
}

template <int MODE>
void launch_min(const float* q, int nq, const float* r, int nr, int batch, float* dist,
                int64_t* index, hipStream_t st) {
  if (flat_shape(nq, nr)) {
    const long total = (long)batch * nq;
    MSMD_LAUNCH(chamfer_min_flat<MODE>, dim3(ceil_div(total, 256)), dim3(256), 0, st, q, nq, r,
                nr, total, dist, index);
  } else {
    MSMD_LAUNCH(chamfer_min_tiled<MODE>, dim3((unsigned)((long)batch * ceil_div(nq, kWave))),
                dim3(kWave), 0, st, q, nq, r, nr, dist, index);
  }
}

template <int MODE>
void launch_grad(const float* own, int n_own, const float* oth, int n_oth, int batch,
                 const float* g_own, const int64_t* i_own, const float* g_oth,
                 const int64_t* i_oth, float* grad, hipStream_t st) {
  if (flat_shape(n_own, n_oth)) {
    const long total = (long)batch * n_own;
    MSMD_LAUNCH(chamfer_grad_flat<MODE>, dim3(ceil_div(total, 256)), dim3(256), 0, st, own, n_own,
                oth, n_oth, total, g_own, i_own, g_oth, i_oth, grad);
  } else {
    MSMD_LAUNCH(chamfer_grad_tiled<MODE>, dim3((unsigned)((long)batch * ceil_div(n_own, kWave))),
                dim3(kWave), 0, st, own, n_own, oth, n_oth, g_own, i_own, g_oth, i_oth, grad);
  }
}

// rows [begin, begin + n) of sample s under CSR offsets, clipped to the rows that exist
__device__ __forceinline__ int sample_rows(const int32_t* __restrict__ offsets, int s, int total,
                                           int& begin) {
  begin = offsets[s];
  const int end = offsets[s + 1];
  if (begin < 0 || begin > total) return 0;
  const int n = min(end, total) - begin;
  return n > 0 ? n : 0;
}

// grid (blocks, sample): a block strides over its sample's points, one lane per point; the
// sample's ground truths pass through LDS 64 at a time (box + gravity centre).  k = boxes
// holding the point so far, ascending: the first fills all three slots, the second slot 1,
// every later one slot 2 -- the reference's counter clamps at 2, so its last box stays there.
__global__ __launch_bounds__(256) void vote_targets_kernel(
    const float* __restrict__ points, int ld, const int32_t* __restrict__ point_offsets,
    int total_points, const float* __restrict__ boxes, const float* __restrict__ centers,
    const int32_t* __restrict__ box_offsets, int total_boxes, float* __restrict__ targets,
    int64_t* __restrict__ mask) {
  __shared__ float gt[kVoteGtChunk * 10];
  const int s = blockIdx.y;
  int p_begin, b_begin;
  const int np = sample_rows(point_offsets, s, total_points, p_begin);
  const int nb = sample_rows(box_offsets, s, total_boxes, b_begin);
  const int rounds = (np + 255) / 256;
  for (int round = blockIdx.x; round < rounds; round += gridDim.x) {
    const int i = round * 256 + threadIdx.x;
    const bool live = i < np;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) {
      const float* p = points + (size_t)(p_begin + i) * ld;
      x = p[0], y = p[1], z = p[2];
    }
    float vote[kVoteSlots * 3];
#pragma unroll
    for (int k = 0; k < kVoteSlots * 3; ++k) vote[k] = 0.f;
    int hits = 0;
    for (int base = 0; base < nb; base += kVoteGtChunk) {
      const int cnt = min(nb - base, kVoteGtChunk);
      __syncthreads();
      for (int k = threadIdx.x; k < cnt * 10; k += 256) {
        const int j = k / 10, c = k - j * 10;
        gt[k] = c < 7 ? boxes[(size_t)(b_begin + base + j) * 7 + c]
                      : centers[(size_t)(b_begin + base + j) * 3 + (c - 7)];
      }
      __syncthreads();
      if (!live) continue;
      for (int j = 0; j < cnt; ++j) {
        const float* g = gt + j * 10;
        float lx, ly;
        if (!pib::pt_in_box(x, y, z, pib::load_box(g), lx, ly)) continue;
        const float v[3] = {g[7] - x, g[8] - y, g[9] - z};
        const int first = hits == 0 ? 0 : (hits == 1 ? 1 : 2);
        const int last = hits == 0 ? 2 : first;
        for (int slot = first; slot <= last; ++slot)
          vote[slot * 3] = v[0], vote[slot * 3 + 1] = v[1], vote[slot * 3 + 2] = v[2];
        ++hits;
      }
    }
    if (live) {
      float* out = targets + (size_t)(p_begin + i) * (kVoteSlots * 3);
#pragma unroll
      for (int k = 0; k < kVoteSlots * 3; ++k) out[k] = vote[k];
      mask[p_begin + i] = hits > 0;
    }
  }
}

// grid (box, sample): the block's lanes share one box and stride over the sample's points
__global__ __launch_bounds__(256) void pib_count_kernel(const float* __restrict__ boxes,
                                                        const float* __restrict__ pts, int ld,
                                                        int nb, int npts,
                                                        int32_t* __restrict__ count) {
  __shared__ int partial[256 / kWave];
  const int t = blockIdx.x, b = blockIdx.y;
  const pib::Box box = pib::load_box(boxes + ((size_t)b * nb + t) * 7);
  const float* pb = pts + (size_t)b * npts * ld;
  int hits = 0;
  for (int i = threadIdx.x; i < npts; i += 256) {
    const float* p = pb + (size_t)i * ld;
    float lx, ly;
    hits += pib::pt_in_box(p[0], p[1], p[2], box, lx, ly) ? 1 : 0;
  }
  hits = wave_sum(hits);
  if ((threadIdx.x & 63) == 0) partial[threadIdx.x >> 6] = hits;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < 256 / kWave; ++w) sum += partial[w];
    count[(size_t)b * nb + t] = sum;
  }
}

int chamfer_args(int batch, int n, int m, int channels, int mode) {
  if (batch < 0 || n < 0 || m < 0) return MSMD_ERR_INVALID_ARG;
  if (channels != 3 || n == 0 || m == 0) return MSMD_ERR_INVALID_ARG;
  if (mode < kL2 || mode > kSmoothL1) return MSMD_ERR_INVALID_ARG;
  const long limit = 2147483647L;
  if ((long)batch * n >= limit || (long)batch * m >= limit) return MSMD_ERR_RANGE;
  return MSMD_OK;
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_chamfer_fwd_f32(const float* src, const float* dst, int batch, int n, int m,
                                     int channels, int mode, float* d1, int64_t* i1, float* d2,
                                     int64_t* i2, msmd_stream_t stream) {
  const int e = chamfer_args(batch, n, m, channels, mode);
  if (e) return e;
  if (batch == 0) return MSMD_OK;
  if (!src || !dst || !d1 || !i1 || !d2 || !i2) return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (mode == kL2) {
    launch_min<kL2>(src, n, dst, m, batch, d1, i1, st);
    launch_min<kL2>(dst, m, src, n, batch, d2, i2, st);
  } else if (mode == kL1) {
    launch_min<kL1>(src, n, dst, m, batch, d1, i1, st);
    launch_min<kL1>(dst, m, src, n, batch, d2, i2, st);
  } else {
    launch_min<kSmoothL1>(src, n, dst, m, batch, d1, i1, st);
    launch_min<kSmoothL1>(dst, m, src, n, batch, d2, i2, st);
  }
  return launch_status();
}

MSMD_EXPORT int msmd_chamfer_bwd_f32(const float* src, const float* dst, const float* g1,
                                     const float* g2, const int64_t* i1, const int64_t* i2,
                                     int batch, int n, int m, int channels, int mode,
                                     float* grad_src, float* grad_dst, msmd_stream_t stream) {
  const int e = chamfer_args(batch, n, m, channels, mode);
  if (e) return e;
  if (batch == 0) return MSMD_OK;
  if (!src || !dst || !g1 || !g2 || !i1 || !i2 || (!grad_src && !grad_dst))
    return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (mode == kL2) {
    if (grad_src) launch_grad<kL2>(src, n, dst, m, batch, g1, i1, g2, i2, grad_src, st);
    if (grad_dst) launch_grad<kL2>(dst, m, src, n, batch, g2, i2, g1, i1, grad_dst, st);
  } else if (mode == kL1) {
    if (grad_src) launch_grad<kL1>(src, n, dst, m, batch, g1, i1, g2, i2, grad_src, st);
    if (grad_dst) launch_grad<kL1>(dst, m, src, n, batch, g2, i2, g1, i1, grad_dst, st);
  } else {
    if (grad_src) launch_grad<kSmoothL1>(src, n, dst, m, batch, g1, i1, g2, i2, grad_src, st);
    if (grad_dst) launch_grad<kSmoothL1>(dst, m, src, n, batch, g2, i2, g1, i1, grad_dst, st);
  }
  return launch_status();
}

MSMD_EXPORT int msmd_vote_targets_f32(const float* points, int ld, const int32_t* point_offsets,
                                      const float* boxes, const float* centers,
                                      const int32_t* box_offsets, int num_samples,
                                      int total_points, int total_boxes, int max_points,
                                      int gt_per_seed, float* vote_targets, int64_t* vote_mask,
                                      msmd_stream_t stream) {
  if (num_samples < 0 || total_points < 0 || total_boxes < 0 || max_points < 0)
    return MSMD_ERR_INVALID_ARG;
  if (ld < 3 || gt_per_seed != kVoteSlots) return MSMD_ERR_INVALID_ARG;
  if (num_samples > 65535) return MSMD_ERR_RANGE;
  if (num_samples == 0 || total_points == 0) return MSMD_OK;
  if (!points || !point_offsets || !box_offsets || !vote_targets || !vote_mask)
    return MSMD_ERR_INVALID_ARG;
  if (total_boxes > 0 && (!boxes || !centers)) return MSMD_ERR_INVALID_ARG;
  // max_points only sizes the grid: a longer sample is still covered, by striding
  const int bound = max_points < total_points ? max_points : total_points;
  const int blocks = bound > 0 ? ceil_div(bound, 256) : 1;
  MSMD_LAUNCH(vote_targets_kernel, dim3(blocks, num_samples), dim3(256), 0, (hipStream_t)stream,
              points, ld, point_offsets, total_points, boxes, centers, box_offsets, total_boxes,
              vote_targets, vote_mask);
  return launch_status();
}

MSMD_EXPORT int msmd_points_in_boxes_count_f32(const float* boxes, const float* pts, int ld,
                                               int batch_size, int num_boxes, int num_points,
                                               int32_t* count, msmd_stream_t stream) {
  if (batch_size < 0 || num_boxes < 0 || num_points < 0 || ld < 3) return MSMD_ERR_INVALID_ARG;
  if (batch_size > 65535) return MSMD_ERR_RANGE;
  if (batch_size == 0 || num_boxes == 0) return MSMD_OK;
  if (!boxes || !count || (num_points > 0 && !pts)) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(pib_count_kernel, dim3(num_boxes, batch_size), dim3(256), 0, (hipStream_t)stream,
              boxes, pts, ld, num_boxes, num_points, count);
  return launch_status();
}
