// hard_vfe.hip -- HardVFE with one or two VFELayers fused: point decoration, Linear (no bias),
// BatchNorm1d, ReLU, the max over the slots of a voxel, the concatenation [h1; max h1] and the
// second Linear + BatchNorm1d + ReLU + max, without any [N, M, U] activation in HBM.
//
// reference: mmdet3d/models/voxel_encoders/voxel_encoder.py (HardVFE.forward) and
//            mmdet3d/models/voxel_encoders/utils.py:34-106 (VFELayer.forward)
//
// Per row r = (n, slot):  y1 = W1 f, h1 = relu(s1 y1 + t1), m1[n] = max_slot h1,
//                         y2 = W2a h1 + W2b m1[n], out[n] = max_slot relu(s2 y2 + t2).
//
// One wavefront per voxel, one lane per channel (both widths <= 64), four voxels per workgroup
// step.  The rows past num_points of a voxel are zero rows: all of them are the same row, so a
// voxel's work is its num_points real rows plus ONE padded row that stands for the M -
// num_points padded slots (weighted by that count in every sum, sitting at the smallest padded
// slot for the argmax ties).  Layer 1 is cheap (K <= 16): it is run once for m1 and again per
// chunk of 8 rows, whose h1 sits in LDS while layer 2 reads it.
//
// Sums are fp64 per lane, added across the wavefronts and then across the workgroups in a
// fixed order: no float atomics, two runs give the same bits.
#include "pillar_common.hpp"

namespace msmd {
namespace {

constexpr int kVox = 4;                  // voxels per workgroup step (one wavefront each)
constexpr int kChunk = 8;                // rows of a voxel whose h1 / dy2 sit in LDS at a time
constexpr int kW = 64;                   // lanes = channels: the width limit of both layers
constexpr int kW2P = 2 * kW + 1;         // LDS pitch of a row of W2 = [W2a | W2b] (odd)
constexpr int kBlocks = 512;             // persistent workgroups (two per CU)
constexpr int kDw2Entries = kW * 2 * kW;                 // dW2 as [u2][64 h1 | 64 m1 columns]
constexpr int kBwdEntries = kDw2Entries + kW * kBwdPitch;  // ... then A1[u1][16], sg1[u1]
constexpr int kStatEntries = 2 * kW;                     // per channel: sum y2, sum (y2 - pivot)^2

enum { kStats = 0, kOut = 1, kPivot = 2 };

struct VfeArgs {
  PillarArgs p;
  const float *w1, *s1, *t1;     // [U1, K], [U1], [U1]
  const float *w2, *s2, *t2;     // [U2, 2 U1], [U2], [U2]; unused with u2 == 0 (one layer)
  int u1, u2;
};

struct VfeShared {
  union {
    float raw[kRows * kKMax];            // decorate_tile's staging, dead after it
    struct {
      float hc[kVox][kChunk][kW];        // h1 of the current chunk
      float dyc[kVox][kChunk][kW];       // backward: dy2 of the current chunk
    } c;
    double red[kW * kBwdPitch];          // the cross-wavefront sums at the end
  } b;
  float dec[kRows * kKP];
  float mean[kVox * 3 + 4];
  float w1t[kKMax * kW];                 // [k][u1]
  float w2s[kW * kW2P];                  // [u2][column], zero outside [U2, 2 U1]
  float s1[kW], t1[kW], s2[kW], t2[kW];
  float m1[kVox][kW];
  float dys[kVox][kW];                   // backward: sum over a voxel's rows of dy2
  int nrow[kVox];
};

// No barrier: the caller's follows.
__device__ __forceinline__ void load_weights(const VfeArgs& a, VfeShared& sh) {
  const int tid = threadIdx.x, K = a.p.k, U1 = a.u1, U2 = a.u2;
  for (int i = tid; i < kKMax * kW; i += 256) {
    const int k = i / kW, u = i - k * kW;
    sh.w1t[i] = (k < K && u < U1) ? a.w1[u * K + k] : 0.f;
  }
  for (int i = tid; i < kW * kW2P; i += 256) {
    const int u = i / kW2P, j = i - u * kW2P;
    sh.w2s[i] = (u < U2 && j < 2 * U1) ? a.w2[u * 2 * U1 + j] : 0.f;
  }
  if (tid < kW) {
    sh.s1[tid] = tid < U1 ? a.s1[tid] : 0.f;
    sh.t1[tid] = tid < U1 ? a.t1[tid] : 0.f;
    sh.s2[tid] = (a.s2 && tid < U2) ? a.s2[tid] : 0.f;
    sh.t2[tid] = (a.t2 && tid < U2) ? a.t2[tid] : 0.f;
  }
}

__device__ __forceinline__ float l1_act(const float* wreg, const float* f, float s, float t) {
  float z = 0.f;
#pragma unroll
  for (int k = 0; k < kKMax; ++k) z = fmaf(wreg[k], f[k], z);
  return fmaxf(z * s + t, 0.f);
}

// Decorates the voxels [p0, p0 + np) and runs layer 1 over this wavefront's voxel: its real
// row count `cnt`, its rows `nr` (cnt, + 1 for the padded row), m1 -> best (and sh.m1) and the
// smallest slot attaining it -> arg.  Ends with a barrier; returns the largest nr of the step.
__device__ __forceinline__ int step_begin(const VfeArgs& a, VfeShared& sh, int p0, int np,
                                          const float* wreg, float s1, float t1, int& cnt,
                                          int& nr, float& best, int& arg) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, M = a.p.m;
  decorate_tile(a.p, p0, np, sh.b.raw, sh.mean, sh.dec);
  cnt = 0; nr = 0; best = -1.f; arg = 0;      // relu output is >= 0: the first row takes it
  if (w < np) {
    cnt = max(0, min(a.p.npts[p0 + w], M));
    nr = cnt + (cnt < M ? 1 : 0);
    const float* f = sh.dec + w * M * kKP;
    for (int i = 0; i < nr; ++i, f += kKP) {
      const float h = l1_act(wreg, f, s1, t1);
      if (h > best) { best = h; arg = i; }     // strict: smallest slot on ties
    }
  }
  sh.m1[w][lane] = w < np ? best : 0.f;
  if (lane == 0) sh.nrow[w] = nr;
  __syncthreads();
  return max(max(sh.nrow[0], sh.nrow[1]), max(sh.nrow[2], sh.nrow[3]));
}

// h1 of the rows [c0, c0 + 8) of this wavefront's voxel -> sh.b.c.hc (zero past nr).  A barrier
// must follow.
__device__ __forceinline__ void chunk_h1(VfeShared& sh, int M, int c0, int nr, const float* wreg,
                                         float s1, float t1) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < kChunk; ++i) {
    const int r = c0 + i;
    sh.b.c.hc[w][i][lane] = r < nr ? l1_act(wreg, sh.dec + (w * M + r) * kKP, s1, t1) : 0.f;
  }
}

// y2 of the chunk's rows for channel `lane`: c2 = W2b m1 first, then the h1 columns in order
__device__ __forceinline__ void chunk_y2(const VfeShared& sh, int U1, float c2, float* acc) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < kChunk; ++i) acc[i] = c2;
  const float* wrow = sh.w2s + lane * kW2P;
  for (int j = 0; j < U1; ++j) {
    const float wv = wrow[j];
#pragma unroll
    for (int i = 0; i < kChunk; ++i) acc[i] = fmaf(wv, sh.b.c.hc[w][i][j], acc[i]);
  }
}

__device__ __forceinline__ float m1_term(const VfeShared& sh, int U1) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* wrow = sh.w2s + lane * kW2P + U1;
  float c2 = 0.f;
  for (int j = 0; j < U1; ++j) c2 = fmaf(wrow[j], sh.m1[w][j], c2);
  return c2;
}

// kStats: part[block][u2 * 2 + {0, 1}] = sum y2, sum (y2 - pivot)^2 over all N * M rows.
// kOut  : out, argmax, ymax (the pre-BatchNorm y2 at the argmax slot; one layer: not written).
// kPivot: out[u2] = y2 of (voxel 0, slot 0).  One workgroup, one step.
template <int MODE>
__global__ __launch_bounds__(256) void hard_vfe_fwd_kernel(VfeArgs a, int nsteps,
                                                           const float* __restrict__ pivot,
                                                           float* __restrict__ out,
                                                           uint8_t* __restrict__ argmax,
                                                           float* __restrict__ ymax,
                                                           double* __restrict__ part) {
  __shared__ VfeShared sh;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, M = a.p.m, U1 = a.u1, U2 = a.u2;
  load_weights(a, sh);
  __syncthreads();
  float wreg[kKMax];
#pragma unroll
  for (int k = 0; k < kKMax; ++k) wreg[k] = sh.w1t[k * kW + lane];
  const float s1 = sh.s1[lane], t1 = sh.t1[lane], s2 = sh.s2[lane], t2 = sh.t2[lane];
  const float pv = (MODE == kStats && lane < U2) ? pivot[lane] : 0.f;
  double ssum = 0.0, ssq = 0.0;
  for (int g = blockIdx.x; g < nsteps; g += gridDim.x) {
    const int p0 = g * kVox, np = min(kVox, a.p.n - p0);
    int cnt, nr, arg;
    float best;
    const int maxnr = step_begin(a, sh, p0, np, wreg, s1, t1, cnt, nr, best, arg);
    if (U2 == 0) {                                 // one layer: the output is m1
      if (MODE == kOut && w < np && lane < U1) {
        out[(long)(p0 + w) * U1 + lane] = best;
        argmax[(long)(p0 + w) * U1 + lane] = (uint8_t)arg;
      }
      continue;
    }
    const float c2 = w < np ? m1_term(sh, U1) : 0.f;
    float best2 = -1.f, ybest = 0.f;
    int arg2 = 0;
    for (int c0 = 0; c0 < maxnr; c0 += kChunk) {
      chunk_h1(sh, M, c0, nr, wreg, s1, t1);
      __syncthreads();
      if (c0 < nr) {
        float acc[kChunk];
        chunk_y2(sh, U1, c2, acc);
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
          const int r = c0 + i;
          if (r >= nr) continue;
          if (MODE == kOut) {
            const float v = fmaxf(acc[i] * s2 + t2, 0.f);
            if (v > best2) { best2 = v; arg2 = r; ybest = acc[i]; }
          } else if (MODE == kStats) {
            const double wgt = r < cnt ? 1.0 : (double)(M - cnt);
            const double d = (double)acc[i] - (double)pv;
            ssum += wgt * (double)acc[i];
            ssq += wgt * (d * d);
          } else if (r == 0 && w == 0 && lane < U2) {
            out[lane] = acc[i];
          }
        }
      }
      __syncthreads();
    }
    if (MODE == kOut && w < np && lane < U2) {
      const long o = (long)(p0 + w) * U2 + lane;
      out[o] = best2;
      argmax[o] = (uint8_t)arg2;
      ymax[o] = ybest;
    }
  }
  if (MODE == kStats) {
    __syncthreads();
    sh.b.red[(w * kW + lane) * 2 + 0] = ssum;
    sh.b.red[(w * kW + lane) * 2 + 1] = ssq;
    __syncthreads();
    if (tid < kStatEntries) {
      double acc = 0.0;
      for (int v = 0; v < kVox; ++v) acc += sh.b.red[v * kStatEntries + tid];
      part[(long)blockIdx.x * kStatEntries + tid] = acc;
    }
  }
}

// g2[N, U]: the gradient reaching the last BatchNorm's output at (n, argmax[n, u]) (grad_out
// where out > 0).  Two layers: dy2[r] = s2 g2[r] - (dp + dq y2[r]) -- dp, dq carry the batch
// statistics' terms (zero in eval mode); part[block] = dW2 [u2][64 | 64], then A1 = sum g1 f
// and sum g1 as [u1][17].  One layer: g1 = g2 at the argmax slot, only the [u1][17] block.
// Two wavefronts per SIMD (two workgroups per CU, as the LDS allows): at one, the LDS latency
// lies open and the pass takes 1.5 x as long, the few spilled registers notwithstanding.
__global__ __launch_bounds__(256, 2) void hard_vfe_bwd_kernel(VfeArgs a, int nsteps,
                                                           const float* __restrict__ g2,
                                                           const uint8_t* __restrict__ argmax,
                                                           const float* __restrict__ dp,
                                                           const float* __restrict__ dq,
                                                           double* __restrict__ part) {
  __shared__ VfeShared sh;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, M = a.p.m, U1 = a.u1, U2 = a.u2;
  load_weights(a, sh);
  __syncthreads();
  float wreg[kKMax];
#pragma unroll
  for (int k = 0; k < kKMax; ++k) wreg[k] = sh.w1t[k * kW + lane];
  const float s1 = sh.s1[lane], t1 = sh.t1[lane], s2 = sh.s2[lane];
  const float dpv = (U2 && lane < U2) ? dp[lane] : 0.f, dqv = (U2 && lane < U2) ? dq[lane] : 0.f;
  double a1[kBwdPitch];          // lane = u1: A1[u1][0..16), sg1[u1]
#pragma unroll
  for (int k = 0; k < kBwdPitch; ++k) a1[k] = 0.0;
  // dW2: thread (u2 = lane, quarter w) owns columns [16 w, 16 w + 16) of the h1 half (dw[0..16))
  // and of the m1 half (dw[16..32)) of [64 h1 | 64 m1]
  double dw[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) dw[k] = 0.0;
  for (int g = blockIdx.x; g < nsteps; g += gridDim.x) {
    const int p0 = g * kVox, np = min(kVox, a.p.n - p0);
    int cnt, nr, arg;
    float best;
    const int maxnr = step_begin(a, sh, p0, np, wreg, s1, t1, cnt, nr, best, arg);
    if (U2 == 0) {
      if (w < np && lane < U1 && best > 0.f) {
        const double gv = (double)g2[(long)(p0 + w) * U1 + lane];
        const float* f = sh.dec + (w * M + arg) * kKP;
#pragma unroll
        for (int k = 0; k < kKMax; ++k) a1[k] += gv * (double)f[k];
        a1[kKMax] += gv;
      }
      continue;
    }
    const float c2 = w < np ? m1_term(sh, U1) : 0.f;
    float gs = 0.f;              // s2 g2 of this voxel and channel, landing on row `ga`
    int ga = -1;
    if (w < np && lane < U2) {
      gs = s2 * g2[(long)(p0 + w) * U2 + lane];
      ga = (int)argmax[(long)(p0 + w) * U2 + lane];
    }
    float dysum = 0.f;
    for (int c0 = 0; c0 < maxnr; c0 += kChunk) {
      chunk_h1(sh, M, c0, nr, wreg, s1, t1);
      __syncthreads();
      {
        float acc[kChunk];
        if (c0 < nr) chunk_y2(sh, U1, c2, acc);
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
          const int r = c0 + i;
          float dy = 0.f;
          if (r < nr && lane < U2) {
            const float wgt = r < cnt ? 1.f : (float)(M - cnt);
            dy = (r == ga ? gs : 0.f) - wgt * (dpv + dqv * acc[i]);
          }
          sh.b.c.dyc[w][i][lane] = dy;
          dysum += dy;
        }
      }
      __syncthreads();
      if (c0 < nr) {             // lane = u1: dx2 = W2a^T dy2, through the ReLU of layer 1
        float dx[kChunk];
#pragma unroll
        for (int i = 0; i < kChunk; ++i) dx[i] = 0.f;
        for (int u = 0; u < U2; ++u) {
          const float wv = sh.w2s[u * kW2P + lane];
#pragma unroll
          for (int i = 0; i < kChunk; ++i) dx[i] = fmaf(wv, sh.b.c.dyc[w][i][u], dx[i]);
        }
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
          const int r = c0 + i;
          if (r < nr && lane < U1 && sh.b.c.hc[w][i][lane] > 0.f) {
            const double gv = (double)dx[i];
            const float* f = sh.dec + (w * M + r) * kKP;
#pragma unroll
            for (int k = 0; k < kKMax; ++k) a1[k] += gv * (double)f[k];
            a1[kKMax] += gv;
          }
        }
      }
      for (int v = 0; v < kVox; ++v) {       // dW2a += dy2 (x) h1 over the step's rows
        const int rows = min(kChunk, sh.nrow[v] - c0);
        for (int i = 0; i < rows; ++i) {
          const double d = (double)sh.b.c.dyc[v][i][lane];
          const float* h = &sh.b.c.hc[v][i][w * 16];
#pragma unroll
          for (int k = 0; k < 16; ++k) dw[k] += d * (double)h[k];
        }
      }
      __syncthreads();
    }
    sh.dys[w][lane] = dysum;
    __syncthreads();
    if (w < np && lane < U1 && best > 0.f) {     // dm1 = W2b^T sum dy2 lands on the argmax row of h1
      float dm = 0.f;
      for (int u = 0; u < U2; ++u) dm = fmaf(sh.w2s[u * kW2P + U1 + lane], sh.dys[w][u], dm);
      const double gv = (double)dm;
      const float* f = sh.dec + (w * M + arg) * kKP;
#pragma unroll
      for (int k = 0; k < kKMax; ++k) a1[k] += gv * (double)f[k];
      a1[kKMax] += gv;
    }
    for (int v = 0; v < np; ++v) {           // dW2b += (sum dy2) (x) m1, once per voxel
      const double d = (double)sh.dys[v][lane];
      const float* h = &sh.m1[v][w * 16];
#pragma unroll
      for (int k = 0; k < 16; ++k) dw[16 + k] += d * (double)h[k];
    }
    // (the next step's barriers stand between these reads and its writes)
  }
  double* mine = part + (long)blockIdx.x * (U2 ? kBwdEntries : kW * kBwdPitch);
  if (U2) {
#pragma unroll
    for (int k = 0; k < 32; ++k)
      mine[lane * 2 * kW + (k < 16 ? 0 : kW - 16) + w * 16 + k] = dw[k];
    mine += kDw2Entries;
  }
  __syncthreads();
  for (int v = 0; v < kVox; ++v) {             // the wavefronts add in turn: a fixed order
    if (w == v) {
#pragma unroll
      for (int k = 0; k < kBwdPitch; ++k) {
        if (v == 0) sh.b.red[lane * kBwdPitch + k] = a1[k];
        else sh.b.red[lane * kBwdPitch + k] += a1[k];
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < kW * kBwdPitch; e += 256) mine[e] = sh.b.red[e];
}

int vfe_flags(int flags) { return (flags & 1 ? kCluster : 0) | (flags & 2 ? kCenter | kCenterZ : 0); }

// 0, or the status that refuses the shape
int vfe_shape_status(int n, int m, int c, int flags, int u1, int u2) {
  if (n < 0 || m < 1 || c < 3 || u1 < 1 || u2 < 0 || (flags & ~3)) return MSMD_ERR_INVALID_ARG;
  if (m > kMMax || u1 > kW || u2 > kW || decorated_channels(c, vfe_flags(flags)) > kKMax)
    return MSMD_ERR_UNSUPPORTED;
  if ((double)n * m * c >= 9.0e18) return MSMD_ERR_RANGE;
  return MSMD_OK;
}

int steps_of(int n) { return ceil_div(n, kVox); }

VfeArgs vfe_args(const float* voxels, const int32_t* num_points, const int32_t* coors, int n,
                 int m, int c, int flags, float vx, float vy, float vz, float xoff, float yoff,
                 float zoff) {
  VfeArgs a = {};
  a.p.vox = voxels; a.p.npts = num_points; a.p.coors = coors;
  a.p.n = n; a.p.m = m; a.p.c = c; a.p.flags = vfe_flags(flags);
  a.p.k = decorated_channels(c, a.p.flags);
  a.p.vx = vx; a.p.vy = vy; a.p.vz = vz;
  a.p.xoff = xoff; a.p.yoff = yoff; a.p.zoff = zoff;
  return a;
}

bool workspace_ok(const void* ws, size_t have, size_t doubles) {
  return ws && !((uintptr_t)ws & 255) && have >= doubles * sizeof(double);
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT size_t msmd_hard_vfe_workspace_bytes(int num_voxels, int max_points) {
  if (num_voxels < 0 || max_points < 1 || max_points > kMMax) return 0;
  const size_t mom =
      (size_t)std::min(std::max(tiles_of(num_voxels, max_points), 1), kMomBlocks) * kMomEntries;
  const size_t bwd = (size_t)std::min(std::max(steps_of(num_voxels), 1), kBlocks) * kBwdEntries;
  return align_up(std::max(mom, bwd) * sizeof(double));
}

MSMD_EXPORT int msmd_hard_vfe_moments_f32(const float* voxels, const int32_t* num_points,
                                          const int32_t* coors, int num_voxels, int max_points,
                                          int num_features, int flags, float vx, float vy,
                                          float vz, float x_offset, float y_offset, float z_offset, double* moments, void* workspace,
                                          size_t workspace_bytes, msmd_stream_t stream) {
  int rc = vfe_shape_status(num_voxels, max_points, num_features, flags, 1, 0);
  if (rc) return rc;
  if (!moments) return MSMD_ERR_INVALID_ARG;
  if (num_voxels == 0) return MSMD_OK;
  if (!voxels || !num_points || !coors) return MSMD_ERR_INVALID_ARG;
  const int tiles = tiles_of(num_voxels, max_points), blocks = std::min(tiles, kMomBlocks);
  if (!workspace_ok(workspace, workspace_bytes, (size_t)blocks * kMomEntries))
    return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  VfeArgs a = vfe_args(voxels, num_points, coors, num_voxels, max_points, num_features, flags,
                       vx, vy, vz, x_offset, y_offset, z_offset);
  MSMD_LAUNCH(pillar_moments_kernel, dim3(blocks), dim3(256), 0, st, a.p, tiles,
              (double*)workspace);
  MSMD_LAUNCH(pillar_moments_combine_kernel, dim3(1), dim3(256), 0, st,
              (const double*)workspace, blocks, moments);
  return launch_status();
}

MSMD_EXPORT int msmd_hard_vfe_stats_f32(const float* voxels, const int32_t* num_points,
                                        const int32_t* coors, int num_voxels, int max_points,
                                        int num_features, int flags, float vx, float vy,
                                        float vz, float x_offset, float y_offset, float z_offset, const float* w1, const float* scale1,
                                        const float* shift1, int u1, const float* w2, int u2,
                                        float* pivot, double* sums, void* workspace,
                                        size_t workspace_bytes, msmd_stream_t stream) {
  int rc = vfe_shape_status(num_voxels, max_points, num_features, flags, u1, u2);
  if (rc) return rc;
  if (u2 < 1 || !pivot || !sums) return MSMD_ERR_INVALID_ARG;
  if (num_voxels == 0) return MSMD_OK;
  if (!voxels || !num_points || !coors || !w1 || !scale1 || !shift1 || !w2)
    return MSMD_ERR_INVALID_ARG;
  const int steps = steps_of(num_voxels), blocks = std::min(steps, kBlocks);
  if (!workspace_ok(workspace, workspace_bytes, (size_t)blocks * kStatEntries))
    return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  VfeArgs a = vfe_args(voxels, num_points, coors, num_voxels, max_points, num_features, flags,
                       vx, vy, vz, x_offset, y_offset, z_offset);
  a.w1 = w1; a.s1 = scale1; a.t1 = shift1; a.u1 = u1;
  a.w2 = w2; a.u2 = u2;               // layer 2's affine is not read here: s2, t2 stay null
  MSMD_LAUNCH(hard_vfe_fwd_kernel<kPivot>, dim3(1), dim3(256), 0, st, a, 1,
              (const float*)nullptr, pivot, (uint8_t*)nullptr, (float*)nullptr,
              (double*)nullptr);
  MSMD_LAUNCH(hard_vfe_fwd_kernel<kStats>, dim3(blocks), dim3(256), 0, st, a, steps,
              (const float*)pivot, (float*)nullptr, (uint8_t*)nullptr, (float*)nullptr,
              (double*)workspace);
  MSMD_LAUNCH(pillar_bwd_combine_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace,
              blocks, kStatEntries, sums);
  return launch_status();
}

MSMD_EXPORT int msmd_hard_vfe_fwd_f32(const float* voxels, const int32_t* num_points,
                                      const int32_t* coors, int num_voxels, int max_points,
                                      int num_features, int flags, float vx, float vy,
                                      float vz, float x_offset, float y_offset, float z_offset, const float* w1, const float* scale1,
                                      const float* shift1, int u1, const float* w2,
                                      const float* scale2, const float* shift2, int u2, float* out,
                                      uint8_t* argmax, float* ymax, msmd_stream_t stream) {
  int rc = vfe_shape_status(num_voxels, max_points, num_features, flags, u1, u2);
  if (rc) return rc;
  if (num_voxels == 0) return MSMD_OK;
  if (!voxels || !num_points || !coors || !w1 || !scale1 || !shift1 || !out || !argmax ||
      (u2 && (!w2 || !scale2 || !shift2 || !ymax)))
    return MSMD_ERR_INVALID_ARG;
  const int steps = steps_of(num_voxels), blocks = std::min(steps, kBlocks);
  VfeArgs a = vfe_args(voxels, num_points, coors, num_voxels, max_points, num_features, flags,
                       vx, vy, vz, x_offset, y_offset, z_offset);
  a.w1 = w1; a.s1 = scale1; a.t1 = shift1; a.u1 = u1;
  a.w2 = w2; a.s2 = scale2; a.t2 = shift2; a.u2 = u2;
  MSMD_LAUNCH(hard_vfe_fwd_kernel<kOut>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a,
              steps, (const float*)nullptr, out, argmax, ymax, (double*)nullptr);
  return launch_status();
}

MSMD_EXPORT int msmd_hard_vfe_bwd_f32(const float* voxels, const int32_t* num_points,
                                      const int32_t* coors, int num_voxels, int max_points,
                                      int num_features, int flags, float vx, float vy,
                                      float vz, float x_offset, float y_offset, float z_offset, const float* w1, const float* scale1,
                                      const float* shift1, int u1, const float* w2,
                                      const float* scale2, int u2, const float* g2,
                                      const uint8_t* argmax, const float* dp, const float* dq,
                                      double* sums, void* workspace, size_t workspace_bytes,
                                      msmd_stream_t stream) {
  int rc = vfe_shape_status(num_voxels, max_points, num_features, flags, u1, u2);
  if (rc) return rc;
  if (!sums) return MSMD_ERR_INVALID_ARG;
  if (num_voxels == 0) return MSMD_OK;
  if (!voxels || !num_points || !coors || !w1 || !scale1 || !shift1 || !g2 || !argmax ||
      (u2 && (!w2 || !scale2 || !dp || !dq)))
    return MSMD_ERR_INVALID_ARG;
  const int steps = steps_of(num_voxels), blocks = std::min(steps, kBlocks);
  const int entries = u2 ? kBwdEntries : kW * kBwdPitch;
  if (!workspace_ok(workspace, workspace_bytes, (size_t)blocks * entries))
    return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  VfeArgs a = vfe_args(voxels, num_points, coors, num_voxels, max_points, num_features, flags,
                       vx, vy, vz, x_offset, y_offset, z_offset);
  a.w1 = w1; a.s1 = scale1; a.t1 = shift1; a.u1 = u1;
  a.w2 = w2; a.s2 = scale2; a.u2 = u2;     // the shift is not read
  MSMD_LAUNCH(hard_vfe_bwd_kernel, dim3(blocks), dim3(256), 0, st, a, steps, g2, argmax, dp, dq,
              (double*)workspace);
  MSMD_LAUNCH(pillar_bwd_combine_kernel, dim3(ceil_div(entries, 256)), dim3(256), 0, st,
              (const double*)workspace, blocks, entries, sums);
  return launch_status();
}
