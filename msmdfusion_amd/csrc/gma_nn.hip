// gma_nn.hip -- the GMA-Conv neighbour search behind FPS, for all samples of a stage at
// once: nearest key (ragged over samples) -> ball query + assignment in one pass ->
// finish (batch offsets, -1 rows).  One fill and three kernels per stage; points.hip keeps
// the per-sample entries (msmd_nn_search / msmd_ball_query / msmd_nn_assign).
//
// Why the nearest key may be ordered by the INTEGER squared distance.  The per-sample
// entry orders keys by (sqrtf(d2), index).  float32 sqrt is strictly increasing on the
// integers up to 4 197 199 (the first n with sqrtf(n) == sqrtf(n + 1) is 4 197 200 > 2^22;
// tests/test_nn_integer_order_cpu.py pins it), so while the minimum d2 is at most 2^22,
// (sqrtf(d2), index) and (d2, index) have the same minimiser.  When the minimum d2 is
// above 2^22 the distance is above 2048 and the result is -1 for every dist_thresh <= 2048,
// whichever key wins.  d2 = dz^2 + dy^2 + dx^2 fits 32 unsigned bits for coordinates in
// [0, 32767] (3 * 32767^2 < 2^32), and each difference fits the 24-bit multiplier.  The
// square root is taken once per query, as sqrtf((float)d2): (float)d2 is exact below 2^24
// and monotone above, where the distance is beyond every admitted threshold anyway.
// Precondition, checked by the callers: coordinates in [0, 32767], dist_thresh <= 2048
// (and radius <= 2048: `(float)d2 < radius^2` is then the float test of the per-sample
// ball query, whose float d2 is exact below 2^24).
#include "common.hpp"

#include <math.h>

namespace msmd {
namespace {

constexpr int kChainKeys = 256;   // keys per workgroup (4 KB of LDS)
constexpr int kChainQpt = 2;      // queries per thread: one LDS read serves both
constexpr int kChainTile = 256 * kChainQpt;
constexpr int kBallUnroll = 8;    // groups of 64 points a ball-query wave loads per trip
// at 2048 representatives and 19 k keys per sample: 4 x 74 workgroups per sample, two
// to three waves per SIMD for a batch of two (one wave per SIMD leaves the LDS latency
// and the compare -> select chain exposed)

// desc: query offsets [nb+1] | key offsets [nb+1] | mode [nb] | base [nb]
struct ChainSample {
  int q0, c2, k0, nk, mode, base;
};
__device__ __forceinline__ ChainSample chain_sample(const int32_t* __restrict__ desc, int nb,
                                                    int b) {
  ChainSample s;
  s.q0 = desc[b];
  s.c2 = desc[b + 1] - s.q0;
  s.k0 = desc[nb + 1 + b];
  s.nk = desc[nb + 2 + b] - s.k0;
  s.mode = desc[2 * nb + 2 + b];
  s.base = desc[3 * nb + 2 + b];
  return s;
}
// rows of the sample that search the keys (never more than its slots)
__device__ __forceinline__ int chain_searchers(const ChainSample& s, const int32_t* fps,
                                               int fps_num, int stride) {
  int n = s.mode == MSMD_NN_CHAIN_CLUSTERED ? (fps ? fps_num : 0)
                                            : s.mode == MSMD_NN_CHAIN_DIRECT ? s.c2 : 0;
  return n < stride ? n : stride;
}
__device__ __forceinline__ int chain_row(const ChainSample& s, const int32_t* __restrict__ fps,
                                         int fps_num, int b, int i) {
  if (s.mode != MSMD_NN_CHAIN_CLUSTERED) return s.q0 + i;
  int r = fps[(size_t)b * fps_num + i];
  r = r < 0 ? 0 : (r >= s.c2 ? s.c2 - 1 : r);
  return s.q0 + r;
}
__device__ __forceinline__ uint32_t chain_d2(int4 a, int4 c) {
  const int dz = a.y - c.y, dy = a.z - c.z, dx = a.w - c.w;
  return (uint32_t)__mul24(dz, dz) + (uint32_t)__mul24(dy, dy) + (uint32_t)__mul24(dx, dx);
}
// the test of nn_final (points.hip) on a (d2 << 32 | key) slot
__device__ __forceinline__ bool chain_found(unsigned long long slot, float thresh) {
  return slot != kEmptySlot && sqrtf((float)(uint32_t)(slot >> 32)) < thresh;
}

// Nearest key: grid (query tile, key chunk, sample).  The chunk's keys are staged in LDS
// as (b,z,y,x) rows and visited in ascending index with a strict `<`, so the smallest index
// wins a tie inside the chunk; chunks combine through a packed (d2, index) 64-bit min,
// which keeps the smallest index across chunks too.
__global__ __launch_bounds__(256) void chain_nn(const int4* __restrict__ q,
                                                const int4* __restrict__ key,
                                                const int32_t* __restrict__ desc, int nb,
                                                const int32_t* __restrict__ fps, int fps_num,
                                                int stride, unsigned long long* best) {
  __shared__ int4 ks[kChainKeys];
  const int b = blockIdx.z;
  const ChainSample s = chain_sample(desc, nb, b);
  const int nq = chain_searchers(s, fps, fps_num, stride);
  const int t0 = blockIdx.x * kChainTile, kb = blockIdx.y * kChainKeys;
  if (t0 >= nq || kb >= s.nk) return;
  const int cnt = (s.nk - kb) < kChainKeys ? (s.nk - kb) : kChainKeys;
  for (int e = threadIdx.x; e < cnt; e += 256) ks[e] = key[(size_t)s.k0 + kb + e];
  int4 qv[kChainQpt];
  uint32_t bd[kChainQpt], bi[kChainQpt];
#pragma unroll
  for (int j = 0; j < kChainQpt; ++j) {
    const int i = t0 + threadIdx.x + j * 256;
    qv[j] = i < nq ? q[chain_row(s, fps, fps_num, b, i)] : make_int4(0, 0, 0, 0);
    bd[j] = 0xFFFFFFFFu;   // above every d2 (3 * 32767^2): the first key always enters
    bi[j] = 0;
  }
  __syncthreads();
#pragma unroll 4
  for (int k = 0; k < cnt; ++k) {
    const int4 kv = ks[k];
#pragma unroll
    for (int j = 0; j < kChainQpt; ++j) {
      const uint32_t d2 = chain_d2(qv[j], kv);
      if (d2 < bd[j]) {
        bd[j] = d2;
        bi[j] = k;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kChainQpt; ++j) {
    const int i = t0 + threadIdx.x + j * 256;
    if (i < nq)
      atomicMin(&best[(size_t)b * stride + i],
                ((unsigned long long)bd[j] << 32) | (uint32_t)(kb + bi[j]));
  }
}

// Ball query and assignment in one pass: one wave per representative of a CLUSTERED
// sample, the sample's queries visited in row order, 64 at a time, hits compacted with a
// ballot so that only the first `nsample` count (ball_query_cuda.cu:33-53), each of them
// taking the highest representative (the order a sequential index_put_ leaves).  A
// representative without a key within the threshold assigns nothing and leaves at once.
// A hit is d2 < r2 in integers, r2 = ceil(radius^2): the float test `d2 == 0 ||
// (float)d2 < radius^2` of the per-sample kernel for an integer d2 below 2^24 and a radius
// in (0, 2048].  The trips are serial through `cnt` and each costs an L2 round trip, which
// is what the pass is made of: kBallUnroll groups of 64 rows are loaded per trip, and the
// next trip's rows are in flight under this one's tests.  The groups are still counted in
// row order, and a group behind the nsample-th hit adds nothing (pos >= nsample).
// (Several representatives per wave, to read every row once for all of them, lost: the
// time follows the serial work of a wave, not the L2 traffic -- DESIGN.md.)
// (A representative is a row of the point set and always hits itself: the reference's "no
// hit leaves a row of zeros" case cannot arise here.)
__global__ __launch_bounds__(256) void chain_ball(const int4* __restrict__ q,
                                                  const int32_t* __restrict__ desc, int nb,
                                                  const int32_t* __restrict__ fps, int fps_num,
                                                  int stride,
                                                  const unsigned long long* __restrict__ best,
                                                  float thresh, uint32_t r2, int nsample,
                                                  int32_t* winner) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.y;
  const ChainSample s = chain_sample(desc, nb, b);
  if (s.mode != MSMD_NN_CHAIN_CLUSTERED || r >= chain_searchers(s, fps, fps_num, stride)) return;
  if (!chain_found(best[(size_t)b * stride + r], thresh)) return;
  const int4 c = q[chain_row(s, fps, fps_num, b, r)];
  const unsigned long long below = (1ull << lane) - 1ull;
  auto load = [&](int4* p, int base) {
#pragma unroll
    for (int u = 0; u < kBallUnroll; ++u) {
      const int k = base + u * 64 + lane;
      p[u] = k < s.c2 ? q[s.q0 + k] : make_int4(0, 0, 0, 0);
    }
  };
  int4 p[kBallUnroll], pn[kBallUnroll];
  load(p, 0);
  int cnt = 0;
  for (int base = 0; base < s.c2 && cnt < nsample; base += 64 * kBallUnroll) {
    load(pn, base + 64 * kBallUnroll);
#pragma unroll
    for (int u = 0; u < kBallUnroll; ++u) {
      const int k = base + u * 64 + lane;
      const unsigned long long mask = __ballot(k < s.c2 && chain_d2(p[u], c) < r2);
      if (mask == 0) continue;   // (most groups: a ball holds a few rows of thousands)
      const int pos = cnt + __popcll(mask & below);
      if (((mask >> lane) & 1) && pos < nsample) atomicMax(&winner[s.q0 + k], r);
      cnt += __popcll(mask);
    }
#pragma unroll
    for (int u = 0; u < kBallUnroll; ++u) p[u] = pn[u];
  }
}

// Finish: row i of the output takes base + its own nearest key (DIRECT) or its winning
// representative's (CLUSTERED), -1 without one; the pad rows behind the queries are -1.
__global__ __launch_bounds__(256) void chain_finish(const int32_t* __restrict__ desc, int nb,
                                                    int n_query, int n_out,
                                                    const int32_t* __restrict__ fps,
                                                    int fps_num, int stride,
                                                    const unsigned long long* __restrict__ best,
                                                    const int32_t* __restrict__ winner,
                                                    float thresh, int64_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_out) return;
  int64_t v = -1;
  if (i < n_query) {
    int b = 0;
    while (b + 1 < nb && i >= desc[b + 1]) ++b;
    const ChainSample s = chain_sample(desc, nb, b);
    int slot = -1;
    if (s.mode == MSMD_NN_CHAIN_DIRECT) slot = i - s.q0;
    else if (s.mode == MSMD_NN_CHAIN_CLUSTERED) slot = winner[i];
    if (slot >= 0 && slot < chain_searchers(s, fps, fps_num, stride)) {
      const unsigned long long w = best[(size_t)b * stride + slot];
      if (chain_found(w, thresh)) v = (int64_t)s.base + (uint32_t)w;
    }
  }
  out[i] = v;
}

// best slots [nb * stride] (64-bit) then winner slots [n_query]: one region, one fill
size_t chain_best_bytes(int nb, int nq_max) {
  return sizeof(unsigned long long) * (size_t)nb * (size_t)(nq_max > 0 ? nq_max : 0);
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT size_t msmd_gma_nn_chain_scratch_bytes(int b, int nq_max, int n_query) {
  if (b < 1 || nq_max < 0 || n_query < 0) return 0;
  return chain_best_bytes(b, nq_max) + sizeof(int32_t) * (size_t)n_query;
}

MSMD_EXPORT int msmd_gma_nn_chain(const int32_t* query_bzyx, int n_query, const int32_t* key_bzyx,
                                  int n_key, const int32_t* desc, int b, const int32_t* fps_idx,
                                  int fps_num, int nq_max, int nk_max, float dist_thresh,
                                  float radius, int max_cluster_samples, int n_pad, int64_t* out,
                                  void* scratch, size_t scratch_bytes, msmd_stream_t stream) {
  if (b < 1 || b > 65535 || n_query < 0 || n_key < 0 || n_pad < 0 || nq_max < 0 || nk_max < 0 ||
      fps_num < 1 || max_cluster_samples < 1 || !desc)
    return MSMD_ERR_INVALID_ARG;
  const long n_out = (long)n_query + n_pad;
  if (n_out == 0) return MSMD_OK;
  if (n_out >= (1L << 31) || !out) return MSMD_ERR_INVALID_ARG;
  if ((n_query > 0 && !query_bzyx) || (n_key > 0 && !key_bzyx)) return MSMD_ERR_INVALID_ARG;
  if (((uintptr_t)query_bzyx | (uintptr_t)key_bzyx) & 15) return MSMD_ERR_INVALID_ARG;
  if (nq_max > n_query || nk_max > n_key) return MSMD_ERR_INVALID_ARG;
  if (!(dist_thresh <= 2048.f) || !(radius > 0.f && radius <= 2048.f)) return MSMD_ERR_UNSUPPORTED;
  const size_t need = msmd_gma_nn_chain_scratch_bytes(b, nq_max, n_query);
  if (need > 0 && (!scratch || scratch_bytes < need || ((uintptr_t)scratch & 7)))
    return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  auto* best = (unsigned long long*)scratch;
  auto* winner = (int32_t*)((char*)scratch + chain_best_bytes(b, nq_max));
  if (need > 0) (void)hipMemsetAsync(scratch, 0xFF, need, st);
  const int4* q4 = (const int4*)query_bzyx;
  if (nq_max > 0 && nk_max > 0) {
    MSMD_LAUNCH(chain_nn, dim3(ceil_div(nq_max, kChainTile), ceil_div(nk_max, kChainKeys), b),
                dim3(256), 0, st, q4, (const int4*)key_bzyx, desc, b, fps_idx, fps_num, nq_max,
                best);
    if (fps_idx)
      MSMD_LAUNCH(chain_ball, dim3(ceil_div(nq_max < fps_num ? nq_max : fps_num, 4), b), dim3(256),
                  0, st, q4, desc, b, fps_idx, fps_num, nq_max, best, dist_thresh,
                  (uint32_t)ceilf(radius * radius), max_cluster_samples, winner);
  }
  MSMD_LAUNCH(chain_finish, dim3(ceil_div(n_out, 256)), dim3(256), 0, st, desc, b, n_query,
              (int)n_out, fps_idx, fps_num, nq_max, best, winner, dist_thresh, out);
  return launch_status();
}
