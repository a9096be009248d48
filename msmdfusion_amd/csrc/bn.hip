// bn.hip -- BatchNorm1d (+ residual) (+ ReLU) over sparse-tensor features [N,C].
//
// The reference applies nn.BatchNorm1d and nn.ReLU(inplace) to .features after
// every sparse conv (make_sparse_convmodule, mmdet3d/ops/sparse_block.py:161-190;
// SparseBasicBlock.forward :103-126: relu(bn2(conv2(.)) + identity)): three to
// five elementwise / reduction launches per conv, each a full pass over [N,C].
// Here: forward = one statistics pass + one fused normalise(+residual)(+ReLU)
// pass; backward = one reduction pass + one fused pass.  All passes stream
// 16-byte vectors, coalesced; reductions are per-block partials combined in
// fixed order in fp64 (deterministic, no float atomics).  The sums themselves are
// fp64 too, from the first add on (a float32 running sum of 128 rows is already
// several times less accurate than torch's float32 BatchNorm, which merges
// Welford pairs), and the forward statistics are sums of x - K and (x - K)^2
// about a pivot K per channel (row 0 of x; per row tile where the conv epilogue
// leaves them): sums of x and x*x lose the variance of a channel that sits many
// standard deviations from zero, and a constant channel must come out with
// variance 0 exactly.  HBM-bound:
// algorithmic bytes fwd = 4NC(2 reads + 1 write [+1 residual]), bwd = 4NC(3-4
// reads + 1-2 writes).
#include "common.hpp"

namespace msmd {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f64x4 widen(f32x4 v) { return __builtin_convertvector(v, f64x4); }
__device__ __forceinline__ f32x4 narrow(f64x4 v) { return __builtin_convertvector(v, f32x4); }
// (x - mean) * invstd [* gamma + beta] in fp64 -- ONE definition: the forward pass and the ReLU
// mask that the backward recomputes from x both go through it, so that the recomputed decision
// narrow(t) > 0 is the forward's, bit for bit
__device__ __forceinline__ f64x4 bn_xhat(f32x4 x, f32x4 mean, f32x4 invstd) {
  return (widen(x) - widen(mean)) * widen(invstd);
}
__device__ __forceinline__ f64x4 bn_affine(f32x4 x, f32x4 mean, f32x4 invstd, f32x4 gamma,
                                           f32x4 beta) {
  return bn_xhat(x, mean, invstd) * widen(gamma) + widen(beta);
}
constexpr int kBnRows = 128;  // rows per partial block (256: 351 workgroups on 256 CUs for the 90k-row layers)

// Partial sums (fp64) of F::kSums values per channel over a block of rows, where the values
// come from a per-element functor.  Threads own a fixed float4 channel group.  The block's
// slot is [c][kSums]: a channel's sums side by side, one vector load for the finalize kernel.  F::kPivot: the functor works about a per-channel pivot, pivot(g) is
// called once with the thread's channel group.
template <typename F>
__device__ __forceinline__ void block_channel_sums(F f, int n, int c, double* __restrict__ part) {
  constexpr int NV = F::kSums;
  __shared__ f64x4 sm[NV * 256];
  const int c4 = c >> 2;
  int used = (256 / c4) * c4;  // threads with a fixed channel group
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * kBnRows;
  const int r1 = (r0 + kBnRows) < n ? (r0 + kBnRows) : n;
  f64x4 acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = (f64x4){0., 0., 0., 0.};
  if (tid < used) {
    const int g = tid % c4;
    const long e0 = (long)r0 * c4, e1 = (long)r1 * c4;
    if (F::kPivot) f.pivot(g);
    for (long e = e0 + tid; e < e1; e += used) {
      f64x4 v[NV];
      f(e, g, v);
#pragma unroll
      for (int k = 0; k < NV; ++k) acc[k] += v[k];
    }
  }
  // c4 a power of two up to 32 (c = 4 .. 128: most layers): a wave's lanes with the same
  // channel group are c4 apart -- add them by shuffles first, so that the c4 threads below
  // read 4 LDS entries per sum, one per wave, instead of 256 / c4 one after the other (for 16
  // channels 64 dependent reads per sum: longer than the block's whole streaming loop)
  const bool by_wave = c4 <= 32 && (c4 & (c4 - 1)) == 0;      // (then used == 256)
  if (by_wave) {
    for (int m = c4; m < 64; m <<= 1)
#pragma unroll
      for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[k][s] += __shfl_xor(acc[k][s], m, 64);
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) sm[k * 256 + tid] = acc[k];
  __syncthreads();
  if (by_wave) {
    if (tid < c4) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        acc[k] = sm[k * 256 + tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) acc[k] += sm[k * 256 + 64 * w + tid];
        sm[k * 256 + tid] = acc[k];
      }
    }
    used = c4;                   // (same thread wrote and reads sm[k * 256 + tid])
  }
  if (tid < c4) {
    typedef double dv __attribute__((ext_vector_type(NV)));
    dv* o = (dv*)(part + ((size_t)blockIdx.x * c + 4 * tid) * NV);
    f64x4 a[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      a[k] = sm[k * 256 + tid];
      for (int t = tid + c4; t < used; t += c4) a[k] += sm[k * 256 + t];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      dv v;
#pragma unroll
      for (int k = 0; k < NV; ++k) v[k] = a[k][s];
      o[s] = v;
    }
  }
}

struct FwdStat {  // u = x - K, v = (x - K)^2 about the pivot K = row 0 of x (every block's:
  static constexpr bool kPivot = true;  // the sums are fp64 and simply add)
  static constexpr int kSums = 2;
  const f32x4* x;
  f32x4 k;
  __device__ void pivot(int g) { k = x[g]; }
  __device__ void operator()(long e, int, f64x4* o) const {
    o[0] = widen(x[e]) - widen(k);      // exact
    o[1] = o[0] * o[0];
  }
};
__global__ __launch_bounds__(256) void bn_fwd_partial(const float* __restrict__ x, int n, int c,
                                                      double* __restrict__ part) {
  block_channel_sums(FwdStat{(const f32x4*)x, (f32x4){0.f, 0.f, 0.f, 0.f}}, n, c, part);
}

// Finalize kernels run with grid = ceil(c/16), block = 256 = 16 channels x 16
// partial-lanes: lane j sums partial blocks j, j+16, ... in fp64, then the 16
// lane sums are added in lane order (fixed order -> deterministic).  Both return
// the channel this thread must finalise (lane 0 of each channel) or -1.
// combine_sums: [nblk][c][NV] fp64 slots of block_channel_sums, plainly added.
template <int NV>
__device__ __forceinline__ int combine_sums(const double* __restrict__ part, int nblk, int c,
                                            double* out) {
  typedef double dv __attribute__((ext_vector_type(NV)));
  __shared__ double sm[NV][16][17];
  const int cl = threadIdx.x & 15, lane = threadIdx.x >> 4;
  const int ch = blockIdx.x * 16 + cl;
  dv a = (dv)(0.0);
  if (ch < c) {
    // same summation order as a plain loop; 8 loads in flight per thread (the loop was one
    // L2 round trip per partial block: 10 us for 350 blocks)
    const dv* p = (const dv*)part + ch;
    int b = lane;
    for (; b + 16 * 7 < nblk; b += 16 * 8) {
      dv v[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) v[t] = p[(size_t)(b + 16 * t) * c];
#pragma unroll
      for (int t = 0; t < 8; ++t) a += v[t];
    }
    for (; b < nblk; b += 16) a += p[(size_t)b * c];
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) sm[k][cl][lane] = a[k];
  __syncthreads();
  if (lane != 0 || ch >= c) return -1;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double s = 0;
    for (int j = 0; j < 16; ++j) s += sm[k][cl][j];
    out[k] = s;
  }
  return ch;
}
// combine_tile_partials: the conv epilogue's float slots [pivot K_b][sum (x - K_b)]
// [sum (x - K_b)^2] over a row tile (`rows` rows each, the last tile the rest of n); they are
// moved to tile 0's pivot K_0 in fp64 (d = K_b - K_0: sum (x - K_0) = s_b + n_b d,
// sum (x - K_0)^2 = ss_b + 2 d s_b + n_b d^2 -- the pairwise merge of Chan et al. written about
// a common origin, so that the lanes still just add) and *k0_out = K_0.  K_0 is a sample of the
// channel: the sums stay of the order of the channel's spread, not of its offset from zero.
__device__ __forceinline__ int combine_tile_partials(const float* __restrict__ part, int nblk,
                                                     int c, int n, int rows, double* s_out,
                                                     double* ss_out, double* k0_out) {
  __shared__ double sm[2][16][17];
  const int cl = threadIdx.x & 15, lane = threadIdx.x >> 4;
  const int ch = blockIdx.x * 16 + cl;
  double s = 0, ss = 0, k0 = 0;
  if (ch < c) {
    const float* p = part + ch;
    const size_t stride = (size_t)3 * c;
    k0 = p[0];
    auto add = [&](int b, float kb, float u, float v) {
      const long left = (long)n - (long)b * rows;
      const double nb = (double)(left < rows ? left : rows), d = (double)kb - k0;
      s += (double)u + nb * d;
      ss += (double)v + 2.0 * d * (double)u + nb * d * d;
    };
    int b = lane;
    for (; b + 16 * 7 < nblk; b += 16 * 8) {
      float k[8], u[8], v[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const float* q = p + (size_t)(b + 16 * t) * stride;
        k[t] = q[0];
        u[t] = q[c];
        v[t] = q[2 * c];
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) add(b + 16 * t, k[t], u[t], v[t]);
    }
    for (; b < nblk; b += 16) {
      const float* q = p + (size_t)b * stride;
      add(b, q[0], q[c], q[2 * c]);
    }
  }
  sm[0][cl][lane] = s;
  sm[1][cl][lane] = ss;
  __syncthreads();
  if (lane != 0 || ch >= c) return -1;
  s = 0;
  ss = 0;
  for (int j = 0; j < 16; ++j) {
    s += sm[0][cl][j];
    ss += sm[1][cl][j];
  }
  *s_out = s;
  *ss_out = ss;
  *k0_out = k0;
  return ch;
}

// mean / invstd from the partials (fp64 combine), running-stat update
// (torch semantics: running_var takes the unbiased variance).
// T = double: bn_fwd_partial's [sum (x - K)][sum (x - K)^2] slots about K = x0 = row 0 of x;
// float: the conv epilogue's [K_b][..][..] slots about a pivot per row tile of `rows` rows
template <typename T>
__global__ __launch_bounds__(256) void bn_fwd_finalize(const T* __restrict__ part, int nblk,
                                                       int rows, const float* __restrict__ x0,
                                                       int n, int c, float eps, float momentum,
                                                       float* running_mean, float* running_var,
                                                       float* __restrict__ mean,
                                                       float* __restrict__ invstd) {
  constexpr bool kTilePivots = sizeof(T) == sizeof(float);
  double s, ss, k0;
  int ch;
  if constexpr (kTilePivots) {
    ch = combine_tile_partials(part, nblk, c, n, rows, &s, &ss, &k0);
    if (ch < 0) return;
  } else {
    double o[2];
    ch = combine_sums<2>(part, nblk, c, o);
    if (ch < 0) return;
    s = o[0], ss = o[1], k0 = x0[ch];
  }
  const double dm = s / n;              // mean - K_0: of the order of the channel's spread
  const double m = k0 + dm;
  double var = ss / n - dm * dm;
  if (var < 0) var = 0;                 // (rounding only: a constant channel gives 0 exactly)
  mean[ch] = (float)m;
  invstd[ch] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    double unbiased = n > 1 ? var * n / (n - 1) : var;
    const double mo = (double)momentum;      // (one rounding each, not three)
    running_mean[ch] = (float)((1.0 - mo) * (double)running_mean[ch] + mo * m);
    running_var[ch] = (float)((1.0 - mo) * (double)running_var[ch] + mo * unbiased);
  }
}

// EVAL: `mean` / `invstd` are the running mean and VARIANCE; every block takes the channels'
// 1 / sqrt(var + eps) into LDS first (fp64, rounded once: the value the backward gets too) and
// block 0 leaves the per-channel mean / invstd in save_mean / save_invstd for the backward pass
// -- one launch per BatchNorm in eval mode instead of two.
template <bool EVAL>
__global__ __launch_bounds__(256) void bn_fwd_apply(const float* __restrict__ x,
                                                    const float* __restrict__ res, long total4,
                                                    int c4, const float* __restrict__ mean,
                                                    const float* __restrict__ invstd,
                                                    const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, int relu,
                                                    float* __restrict__ y, float eps,
                                                    float* __restrict__ save_mean,
                                                    float* __restrict__ save_invstd) {
  __shared__ __attribute__((aligned(16))) float s_is[EVAL ? 1024 : 4];      // c <= 1024
  if (EVAL) {
    for (int ch = threadIdx.x; ch < 4 * c4; ch += 256) {
      s_is[ch] = (float)(1.0 / sqrt((double)invstd[ch] + (double)eps));
      if (blockIdx.x == 0) {
        save_mean[ch] = mean[ch];
        save_invstd[ch] = s_is[ch];
      }
    }
    __syncthreads();
  }
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total4; e += (long)gridDim.x * 256) {
    const int g = (int)(e % c4);
    f32x4 v = ((const f32x4*)x)[e];
    const f32x4 m = ((const f32x4*)mean)[g];
    const f32x4 is = EVAL ? ((const f32x4*)s_is)[g] : ((const f32x4*)invstd)[g];
    const f32x4 ga = ((const f32x4*)gamma)[g], be = ((const f32x4*)beta)[g];
    // fp64 from the loads to the one rounding of the result: the float32 chain's four
    // roundings show where the product and beta (or the residual) cancel
    f64x4 t = bn_affine(v, m, is, ga, be);
    if (res) t += widen(((const f32x4*)res)[e]);
    v = narrow(t);
    if (relu) {
#pragma unroll
      for (int s = 0; s < 4; ++s) v[s] = v[s] > 0.f ? v[s] : 0.f;
    }
    ((f32x4*)y)[e] = v;
  }
}

// Backward sums, about the forward's float32 mean m: dy_eff, dy_eff * (x - m), and x - m,
// (x - m)^2 -- from the last two the finalize kernel takes the batch mean and variance again
// in fp64 (this pass reads x anyway): working from the ROUNDED save_mean / save_invstd moves
// dgamma by invstd * dbeta * the mean's rounding, and at two rows dx hangs on invstd's last bit.
struct BwdStat {
  static constexpr bool kPivot = false;
  static constexpr int kSums = 4;
  __device__ void pivot(int) {}
  const f32x4 *x, *y, *dy, *mean, *invstd;
  int relu;
  __device__ void operator()(long e, int g, f64x4* o) const {
    f32x4 d = dy[e];
    if (relu) {
      f32x4 yy = y[e];
#pragma unroll
      for (int s = 0; s < 4; ++s) d[s] = yy[s] > 0.f ? d[s] : 0.f;
    }
    o[0] = widen(d);
    o[2] = widen(x[e]) - widen(mean[g]);
    o[1] = o[0] * o[2];
    o[3] = o[2] * o[2];
  }
};
// The same with the ReLU mask recomputed from x instead of read from y (BN + ReLU without a
// residual): y > 0 <=> (x - mean) * invstd * gamma + beta > 0, evaluated exactly as the
// forward pass evaluated it (bn_xhat / bn_affine: same operations in the same order, no
// contraction: the build flags) -- one array less to stream in a pass that does nothing but
// stream.
struct BwdStatRecompute {
  static constexpr bool kPivot = false;
  static constexpr int kSums = 4;
  __device__ void pivot(int) {}
  const f32x4 *x, *dy, *mean, *invstd, *gamma, *beta;
  __device__ void operator()(long e, int g, f64x4* o) const {
    const f32x4 t = narrow(bn_affine(x[e], mean[g], invstd[g], gamma[g], beta[g]));
    f32x4 d = dy[e];
#pragma unroll
    for (int s = 0; s < 4; ++s) d[s] = t[s] > 0.f ? d[s] : 0.f;
    o[0] = widen(d);
    o[2] = widen(x[e]) - widen(mean[g]);
    o[1] = o[0] * o[2];
    o[3] = o[2] * o[2];
  }
};
__global__ __launch_bounds__(256) void bn_bwd_partial(const float* x, const float* y,
                                                      const float* dy, int n, int c,
                                                      const float* mean, const float* invstd,
                                                      int relu, double* __restrict__ part) {
  block_channel_sums(BwdStat{(const f32x4*)x, (const f32x4*)y, (const f32x4*)dy,
                             (const f32x4*)mean, (const f32x4*)invstd, relu},
                     n, c, part);
}
__global__ __launch_bounds__(256) void bn_bwd_partial_recompute(
    const float* x, const float* dy, int n, int c, const float* mean, const float* invstd,
    const float* gamma, const float* beta, double* __restrict__ part) {
  block_channel_sums(BwdStatRecompute{(const f32x4*)x, (const f32x4*)dy, (const f32x4*)mean,
                                      (const f32x4*)invstd, (const f32x4*)gamma,
                                      (const f32x4*)beta},
                     n, c, part);
}
// st64[4][c] for the apply pass, unrounded: dgamma, dbeta, and what the apply pass must use
// for the statistics: dm = mean - save_mean and invstd.  refine (training, the forward's eps
// known): both from this pass's own fp64 sums; else dm = 0, invstd = save_invstd.
__global__ __launch_bounds__(256) void bn_bwd_finalize(const double* __restrict__ part, int nblk,
                                                       int n, int c,
                                                       const float* __restrict__ invstd,
                                                       int refine, float eps,
                                                       float* __restrict__ dgamma,
                                                       float* __restrict__ dbeta,
                                                       double* __restrict__ st64) {
  double o[4];
  const int ch = combine_sums<4>(part, nblk, c, o);
  if (ch < 0) return;
  double is = invstd[ch], dm = 0;
  if (refine) {
    dm = o[2] / n;
    double var = o[3] / n - dm * dm;
    if (var < 0) var = 0;
    is = 1.0 / sqrt(var + (double)eps);
  }
  const double dg = is * (o[1] - dm * o[0]);      // sum dy_eff * (x - mean) * invstd
  dbeta[ch] = (float)o[0];
  dgamma[ch] = (float)dg;
  st64[ch] = dg;
  st64[c + ch] = o[0];
  st64[2 * c + ch] = dm;
  st64[3 * c + ch] = is;
}
// training: dx = gamma*invstd*(dy - dbeta/N - xhat*dgamma/N); eval: gamma*invstd*dy
__global__ __launch_bounds__(256) void bn_bwd_apply(const float* __restrict__ x,
                                                    const float* __restrict__ y,
                                                    const float* __restrict__ dy, long total4,
                                                    int c4, double inv_n,
                                                    const float* __restrict__ mean,
                                                    const float* __restrict__ invstd,
                                                    const float* __restrict__ gamma,
                                                    const double* __restrict__ st64, int relu,
                                                    int training, float* __restrict__ dx,
                                                    float* __restrict__ dres) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total4; e += (long)gridDim.x * 256) {
    const int g = (int)(e % c4);
    f32x4 d = ((const f32x4*)dy)[e];
    if (relu) {
      f32x4 yy = ((const f32x4*)y)[e];
#pragma unroll
      for (int s = 0; s < 4; ++s) d[s] = yy[s] > 0.f ? d[s] : 0.f;
    }
    if (dres) ((f32x4*)dres)[e] = d;
    const f64x4* st = (const f64x4*)st64 + g;       // [dgamma][dbeta][dm][invstd], c4 apart
    const f64x4 is = st[3 * c4];
    f64x4 r = widen(d);      // (fp64: the three terms cancel, most of all for a few rows)
    if (training) {
      const f64x4 xh =
          (widen(((const f32x4*)x)[e]) - widen(((const f32x4*)mean)[g]) - st[2 * c4]) * is;
      r = r - st[c4] * inv_n - xh * st[0] * inv_n;
    }
    ((f32x4*)dx)[e] = narrow(r * is * widen(((const f32x4*)gamma)[g]));
  }
}

// BN + ReLU without a residual, mask recomputed from x (see BwdStatRecompute)
__global__ __launch_bounds__(256) void bn_bwd_apply_recompute(
    const float* __restrict__ x, const float* __restrict__ dy, long total4, int c4, double inv_n,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const double* __restrict__ st64, int training, float* __restrict__ dx) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total4; e += (long)gridDim.x * 256) {
    const int g = (int)(e % c4);
    const f32x4 xv = ((const f32x4*)x)[e], m = ((const f32x4*)mean)[g];
    const f32x4 ga = ((const f32x4*)gamma)[g];
    // the mask: the forward's own evaluation, from the float32 statistics it used
    const f32x4 t = narrow(bn_affine(xv, m, ((const f32x4*)invstd)[g], ga, ((const f32x4*)beta)[g]));
    f32x4 d = ((const f32x4*)dy)[e];
#pragma unroll
    for (int s = 0; s < 4; ++s) d[s] = t[s] > 0.f ? d[s] : 0.f;
    const f64x4* st = (const f64x4*)st64 + g;       // [dgamma][dbeta][dm][invstd], c4 apart
    const f64x4 is = st[3 * c4];
    f64x4 r = widen(d);
    if (training) {
      const f64x4 xh = (widen(xv) - widen(m) - st[2 * c4]) * is;
      r = r - st[c4] * inv_n - xh * st[0] * inv_n;
    }
    ((f32x4*)dx)[e] = narrow(r * is * widen(ga));
  }
}

inline int bn_blocks(int n) { return ceil_div(n > 0 ? n : 1, kBnRows); }
// workspace: the backward's [blocks][4][c] fp64 block sums (the forward uses [blocks][2][c] of
// them) and its unrounded [4][c] totals / statistics behind them
inline size_t bn_ws_bytes(int n, int c) {
  return sizeof(double) * ((size_t)bn_blocks(n) * 4 + 4) * c;
}
inline int stream_blocks(long total4) {
  long b = (total4 + 255) / 256;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT size_t msmd_bn_workspace_bytes(int n, int c) {
  return align_up(bn_ws_bytes(n, c));
}

MSMD_EXPORT int msmd_bn_act_fwd_f32(const float* x, const float* residual, int n, int c,
                                    const float* gamma, const float* beta, float* running_mean,
                                    float* running_var, int training, float momentum, float eps,
                                    int relu, float* y, float* save_mean, float* save_invstd,
                                    void* workspace, size_t workspace_bytes,
                                    msmd_stream_t stream) {
  if (n < 0 || c < 4 || (c & 3) || c > 1024 || !gamma || !beta || !save_mean || !save_invstd)
    return c > 0 && ((c & 3) || c > 1024) ? MSMD_ERR_UNSUPPORTED : MSMD_ERR_INVALID_ARG;
  if (!training && (!running_mean || !running_var)) return MSMD_ERR_INVALID_ARG;
  if (n == 0) return MSMD_OK;
  if (!x || !y) return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = bn_blocks(n);
  if (training) {
    if (workspace_bytes < bn_ws_bytes(n, c) || ((uintptr_t)workspace & 255))
      return MSMD_ERR_WORKSPACE;
    double* part = (double*)workspace;
    MSMD_LAUNCH(bn_fwd_partial, dim3(nblk), dim3(256), 0, st, x, n, c, part);
    MSMD_LAUNCH(bn_fwd_finalize<double>, dim3(ceil_div(c, 16)), dim3(256), 0, st, part, nblk,
                kBnRows, x, n, c, eps, momentum, running_mean, running_var, save_mean, save_invstd);
  }
  const long total4 = (long)n * (c >> 2);
  if (training)
    MSMD_LAUNCH(bn_fwd_apply<false>, dim3(stream_blocks(total4)), dim3(256), 0, st, x, residual,
                total4, c >> 2, save_mean, save_invstd, gamma, beta, relu, y, eps,
                (float*)nullptr, (float*)nullptr);
  else
    MSMD_LAUNCH(bn_fwd_apply<true>, dim3(stream_blocks(total4)), dim3(256), 0, st, x, residual,
                total4, c >> 2, running_mean, running_var, gamma, beta, relu, y, eps, save_mean,
                save_invstd);
  return launch_status();
}

// Training-mode forward with the statistics pass already done: `partials` =
// [n_partials][3][c]: per block of `rows_per_partial` rows of x (the last block the rest;
// n_partials = ceil(n / rows_per_partial)) and per channel a pivot K, sum (x - K) and
// sum (x - K)^2 (msmd_spconv_fwd_split_stats writes them from its accumulators).
MSMD_EXPORT int msmd_bn_act_fwd_from_partials_f32(const float* x, const float* residual, int n,
                                                  int c, const float* gamma, const float* beta,
                                                  float* running_mean, float* running_var,
                                                  float momentum, float eps, int relu, float* y,
                                                  float* save_mean, float* save_invstd,
                                                  const float* partials, int n_partials,
                                                  int rows_per_partial, msmd_stream_t stream) {
  if (n < 0 || c < 4 || (c & 3) || c > 1024 || !gamma || !beta || !save_mean || !save_invstd)
    return c > 0 && ((c & 3) || c > 1024) ? MSMD_ERR_UNSUPPORTED : MSMD_ERR_INVALID_ARG;
  if (n == 0) return MSMD_OK;
  if (!x || !y || !partials || n_partials < 1 || rows_per_partial < 1 ||
      n_partials != ceil_div(n, rows_per_partial))
    return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  MSMD_LAUNCH(bn_fwd_finalize<float>, dim3(ceil_div(c, 16)), dim3(256), 0, st, partials, n_partials,
              rows_per_partial, (const float*)nullptr, n, c, eps, momentum, running_mean, running_var, save_mean, save_invstd);
  const long total4 = (long)n * (c >> 2);
  MSMD_LAUNCH(bn_fwd_apply<false>, dim3(stream_blocks(total4)), dim3(256), 0, st, x, residual,
              total4, c >> 2, save_mean, save_invstd, gamma, beta, relu, y, eps, (float*)nullptr,
              (float*)nullptr);
  return launch_status();
}

MSMD_EXPORT int msmd_bn_act_bwd_f32(const float* x, const float* y, const float* dy, int n, int c,
                                    const float* gamma, const float* save_mean,
                                    const float* save_invstd, int training, float eps, int relu,
                                    float* dx, float* dresidual, float* dgamma, float* dbeta,
                                    void* workspace, size_t workspace_bytes,
                                    msmd_stream_t stream) {
  if (n < 0 || c < 4 || (c & 3) || c > 1024 || !gamma || !save_mean || !save_invstd || !dgamma ||
      !dbeta)
    return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    hipMemsetAsync(dgamma, 0, sizeof(float) * c, st);
    hipMemsetAsync(dbeta, 0, sizeof(float) * c, st);
    return MSMD_OK;
  }
  if (!x || !dy || !dx || (relu && !y)) return MSMD_ERR_INVALID_ARG;
  const int nblk = bn_blocks(n);
  if (workspace_bytes < bn_ws_bytes(n, c) || ((uintptr_t)workspace & 255))
    return MSMD_ERR_WORKSPACE;
  double* part = (double*)workspace;
  MSMD_LAUNCH(bn_bwd_partial, dim3(nblk), dim3(256), 0, st, x, y, dy, n, c, save_mean,
              save_invstd, relu, part);
  double* st64 = part + (size_t)nblk * 4 * c;
  MSMD_LAUNCH(bn_bwd_finalize, dim3(ceil_div(c, 16)), dim3(256), 0, st, part, nblk, n, c,
              save_invstd, (int)(training && eps > 0.f), eps, dgamma, dbeta, st64);
  const long total4 = (long)n * (c >> 2);
  MSMD_LAUNCH(bn_bwd_apply, dim3(stream_blocks(total4)), dim3(256), 0, st, x, y, dy, total4,
              c >> 2, 1.0 / (double)n, save_mean, save_invstd, gamma, st64, relu, training, dx,
              dresidual);
  return launch_status();
}

// BatchNorm + ReLU (no residual) backward without reading y: the mask is recomputed from x
// (bit-identical decision, see BwdStatRecompute).  Same results as msmd_bn_act_bwd_f32 with
// relu = 1 and the forward pass's y; the two streaming passes read 2 and 2 arrays instead of
// 3 and 3 (+1 write).
MSMD_EXPORT int msmd_bn_relu_bwd_f32(const float* x, const float* dy, int n, int c,
                                     const float* gamma, const float* beta,
                                     const float* save_mean, const float* save_invstd,
                                     int training, float eps, float* dx, float* dgamma,
                                     float* dbeta, void* workspace, size_t workspace_bytes,
                                     msmd_stream_t stream) {
  if (n < 0 || c < 4 || (c & 3) || c > 1024 || !gamma || !beta || !save_mean || !save_invstd ||
      !dgamma || !dbeta)
    return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    hipMemsetAsync(dgamma, 0, sizeof(float) * c, st);
    hipMemsetAsync(dbeta, 0, sizeof(float) * c, st);
    return MSMD_OK;
  }
  if (!x || !dy || !dx) return MSMD_ERR_INVALID_ARG;
  const int nblk = bn_blocks(n);
  if (workspace_bytes < bn_ws_bytes(n, c) || ((uintptr_t)workspace & 255))
    return MSMD_ERR_WORKSPACE;
  double* part = (double*)workspace;
  MSMD_LAUNCH(bn_bwd_partial_recompute, dim3(nblk), dim3(256), 0, st, x, dy, n, c, save_mean,
              save_invstd, gamma, beta, part);
  double* st64 = part + (size_t)nblk * 4 * c;
  MSMD_LAUNCH(bn_bwd_finalize, dim3(ceil_div(c, 16)), dim3(256), 0, st, part, nblk, n, c,
              save_invstd, (int)(training && eps > 0.f), eps, dgamma, dbeta, st64);
  const long total4 = (long)n * (c >> 2);
  MSMD_LAUNCH(bn_bwd_apply_recompute, dim3(stream_blocks(total4)), dim3(256), 0, st, x, dy, total4,
              c >> 2, 1.0 / (double)n, save_mean, save_invstd, gamma, beta, st64, training, dx);
  return launch_status();
}
