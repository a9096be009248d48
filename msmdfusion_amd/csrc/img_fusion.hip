// img_fusion.hip -- the image stage of TransFusionHead (COVERAGE f3-img): what the reference
// computes in a Python double loop over samples and views
// (mmdet3d/models/dense_heads/transfusion_head.py:930-1004).
//
// msmd_img_query_geometry_f32   one launch for the batch, one block per sample, the views looped
//   inside.  Per (sample, view, query): the eight box corners (lidar_box3d.py:46-84), centre
//   and corners through the 3x4 matrix (lidar2img times the reversed 3-D flow, composed on the
//   host in float64), depth clamped at 1e-5, scale / crop / flip, the strict on-image test, the
//   float centre on the feature map, its truncation, radius = ceil(|max - min| / osf / 2)
//   saturating at INT32_MAX (also for NaN), sigma = (2 radius + 1) / 6.  Then, in the same
//   block: the member count of every view (an integer LDS counter), group validity (count > 1,
//   :985), the winning view of every query (the HIGHEST valid view that sees it: later views
//   overwrite earlier ones, :987 and :1004) and on_the_image_mask.  Nothing is read back.
//
// msmd_gauss_attn_fwd_f32 / _bwd_f32   cross-attention with the reference's Gaussian log-mask
//   (:996-1003) without the [n, H W] mask: per (row, head)
//       softmax_j( q.k_j / sqrt(d) - d2_j / (2 sigma^2) )   over the keys with
//       exp(-d2_j / (2 sigma^2)) >= FLT_EPSILON,
//   d2 the squared distance of the integer centre to the key's cell.  Only the bounding box of
//   that disc, clipped to the map, is visited; the softmax is online.  Forward and the dQ pass
//   are query-stationary: one wave per (row, head), lane <-> key, every lane keeps its own
//   running (max, sum, accumulator[d]) and the 64 states are merged by a butterfly at the end.
//   dK / dV are key-stationary: one thread per key of one (sample, view, head) holds K_j, V_j
//   and both accumulators in registers and walks the sample's rows in ASCENDING order, kChunk
//   rows at a time through LDS, keeping the rows of its view whose window covers the key.  No
//   atomics: every result is a fixed-order sum, bitwise reproducible.
//
//   Dropout (on the attention weights, after the softmax, as torch's attention does): key j of
//   (row, head) is kept iff mix(seed, row, head, j) >= threshold, threshold = floor(p 2^32),
//   kept weights times 1 / (1 - p).  mix is stateless (below); the backward regenerates it.
//
//   Backward with dropout D_ij (0 or 1/(1-p)): O_i = sum_j D_ij P_ij V_j, so dP_ij = D_ij
//   dO_i.V_j and sum_j P_ij dP_ij = dO_i . O_i: the row term of the softmax gradient is still
//   delta_i = dO_i . O_i.  dS_ij = P_ij (dP_ij - delta_i), dQ_i = sum_j dS_ij K_j / sqrt(d),
//   dK_j = sum_i dS_ij Q_i / sqrt(d), dV_j = sum_i D_ij P_ij dO_i, P_ij = exp(S_ij - lse_i).
//
// About 0.2 GFLOP at the nuScenes shape (400 rows, 8 heads, windows of a few hundred keys of
// 16 floats): latency and traffic, not arithmetic, so plain VALU with 16-byte loads.
#include <float.h>
#include <math.h>

#include "common.hpp"

namespace msmd {
namespace {

constexpr int kGeoBlock = 256;
constexpr int kGeoPerThread = 4;             // P <= kGeoBlock * kGeoPerThread
constexpr int kGeoMaxViews = 8;
constexpr int kAttnKeyTile = 256;            // keys per block of the key-stationary pass
constexpr int kAttnRowChunk = 64;            // rows staged per LDS round of that pass

__device__ __forceinline__ float proj4(const float* m, float x, float y, float z) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)),
                             __fmul_rn(m[2], z)), m[3]);
}

struct Pixel {
  float x, y;
};

// :954-973 for one point
__device__ __forceinline__ Pixel to_pixel(const msmd_point_sample_params& p, float x, float y,
                                          float z) {
  const float qx = proj4(p.m, x, y, z), qy = proj4(p.m + 4, x, y, z);
  float qz = proj4(p.m + 8, x, y, z);
  qz = qz < 1e-5f ? 1e-5f : qz;                      // clamp(min=1e-5); NaN stays NaN
  Pixel o;
  o.x = __fsub_rn(__fmul_rn(__fdiv_rn(qx, qz), p.scale_x), p.crop_x);
  o.y = __fsub_rn(__fmul_rn(__fdiv_rn(qy, qz), p.scale_y), p.crop_y);
  if (p.flip != 0.f) o.x = __fsub_rn(p.img_w, o.x);
  return o;
}

__device__ __forceinline__ int saturating_int(float v) {   // NaN -> INT32_MAX as well
  if (!(v < 2147483520.f)) return 2147483647;
  if (v < -2147483520.f) return -2147483647 - 1;
  return (int)v;
}

// grid (B), kGeoBlock threads
__global__ __launch_bounds__(kGeoBlock) void img_query_geometry_kernel(
    const float* __restrict__ pos3d, const float* __restrict__ boxes,
    const msmd_point_sample_params* __restrict__ params, int P, int V, float osf,
    uint8_t* __restrict__ on, float* __restrict__ pos, int32_t* __restrict__ centre,
    int32_t* __restrict__ radius, float* __restrict__ sigma, int32_t* __restrict__ count,
    uint8_t* __restrict__ valid, int32_t* __restrict__ winner, uint8_t* __restrict__ mask,
    float* __restrict__ win_pos, int32_t* __restrict__ win_centre, float* __restrict__ win_sigma) {
  __shared__ int cnt[kGeoMaxViews];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < kGeoMaxViews) cnt[tid] = 0;
  __syncthreads();
  uint32_t onbits[kGeoPerThread];
#pragma unroll
  for (int j = 0; j < kGeoPerThread; ++j) {
    onbits[j] = 0;
    const int p = tid + j * kGeoBlock;
    if (p >= P) continue;
    const float* q3 = pos3d + (size_t)b * 3 * P + p;
    const float x = q3[0], y = q3[P], z = q3[2 * (size_t)P];
    const float* bx = boxes + ((size_t)b * P + p) * 7;
    const float ox = bx[0], oy = bx[1], oz = bx[2], dx = bx[3], dy = bx[4], dz = bx[5];
    const float sn = sinf(bx[6]), cs = cosf(bx[6]);
    float cxs[8], cys[8], czs[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      // (x0y0z0, x0y0z1, x0y1z1, x0y1z0, x1y0z0, x1y0z1, x1y1z1, x1y1z0)
      const float ux = (i & 4) ? 0.5f : -0.5f;
      const float uy = (i & 2) ? 0.5f : -0.5f;
      const float uz = ((i ^ (i >> 1)) & 1) ? 1.f : 0.f;
      const float lx = __fmul_rn(dx, ux), ly = __fmul_rn(dy, uy), lz = __fmul_rn(dz, uz);
      cxs[i] = __fadd_rn(__fadd_rn(__fmul_rn(lx, cs), __fmul_rn(ly, sn)), ox);
      cys[i] = __fadd_rn(__fsub_rn(__fmul_rn(ly, cs), __fmul_rn(lx, sn)), oy);
      czs[i] = __fadd_rn(lz, oz);
    }
    for (int v = 0; v < V; ++v) {
      const msmd_point_sample_params prm = params[(size_t)b * V + v];
      const Pixel c = to_pixel(prm, x, y, z);
      const bool is_on = c.x > 0.f && c.x < prm.pad_w && c.y > 0.f && c.y < prm.pad_h;
      float mxx = -INFINITY, mnx = INFINITY, mxy = -INFINITY, mny = INFINITY;
      bool bad = false;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const Pixel k = to_pixel(prm, cxs[i], cys[i], czs[i]);
        bad = bad || isnan(k.x) || isnan(k.y);
        mxx = fmaxf(mxx, k.x), mnx = fminf(mnx, k.x);
        mxy = fmaxf(mxy, k.y), mny = fminf(mny, k.y);
      }
      const float ex = __fdiv_rn(__fsub_rn(mxx, mnx), osf), ey = __fdiv_rn(__fsub_rn(mxy, mny), osf);
      const float nrm = __fsqrt_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)));
      const int rad = bad ? 2147483647 : saturating_int(ceilf(__fdiv_rn(nrm, 2.f)));
      const float px = __fdiv_rn(c.x, osf), py = __fdiv_rn(c.y, osf);
      const size_t o = ((size_t)b * V + v) * P + p;
      on[o] = is_on ? 1 : 0;
      pos[2 * o] = px, pos[2 * o + 1] = py;
      centre[2 * o] = is_on ? saturating_int(truncf(px)) : 0;
      centre[2 * o + 1] = is_on ? saturating_int(truncf(py)) : 0;
      radius[o] = rad;
      sigma[o] = __fdiv_rn(__fadd_rn(__fmul_rn((float)rad, 2.f), 1.f), 6.f);
      if (is_on) {
        onbits[j] |= 1u << v;
        atomicAdd(&cnt[v], 1);
      }
    }
  }
  __syncthreads();
  if (tid < V) {
    count[(size_t)b * V + tid] = cnt[tid];
    valid[(size_t)b * V + tid] = cnt[tid] > 1 ? 1 : 0;
  }
#pragma unroll
  for (int j = 0; j < kGeoPerThread; ++j) {
    const int p = tid + j * kGeoBlock;
    if (p >= P) continue;
    int win = -1;
    for (int v = 0; v < V; ++v)
      if (((onbits[j] >> v) & 1u) && cnt[v] > 1) win = v;
    const size_t r = (size_t)b * P + p;
    winner[r] = win;
    mask[r] = win >= 0 ? 1 : 0;
    float wx = 0.f, wy = 0.f, ws = 0.f;
    int cx = 0, cy = 0;
    if (win >= 0) {          // this thread's own stores above
      const size_t o = ((size_t)b * V + win) * P + p;
      wx = pos[2 * o], wy = pos[2 * o + 1], ws = sigma[o];
      cx = centre[2 * o], cy = centre[2 * o + 1];
    }
    win_pos[2 * r] = wx, win_pos[2 * r + 1] = wy;
    win_centre[2 * r] = cx, win_centre[2 * r + 1] = cy;
    win_sigma[r] = ws;
  }
}

// ---- dropout ------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t fmix32(uint32_t x) {      // murmur3's finaliser
  x ^= x >> 16, x *= 0x85EBCA6Bu, x ^= x >> 13, x *= 0xC2B2AE35u, x ^= x >> 16;
  return x;
}
// mix(seed, row, head, key): see include/msmd_hip.h; restated in tests/img_fusion_ref.py
__device__ __forceinline__ uint32_t drop_mix(uint32_t seed_lo, uint32_t seed_hi, uint32_t row,
                                             uint32_t head, uint32_t key) {
  uint32_t x = fmix32(seed_lo ^ (row * 0x9E3779B1u));
  x = fmix32((x + head * 0x85EBCA77u) ^ seed_hi);
  return fmix32(x ^ (key * 0xC2B2AE3Du));
}

struct Window {
  int x0, x1, y0, y1;
  float two_s2;
};

// the bounding box of the disc exp(-d2 / two_s2) >= eps, i.e. d2 <= 15.95 two_s2, clipped
__device__ __forceinline__ Window window_of(int cx, int cy, float sg, int H, int W) {
  Window w;
  w.two_s2 = __fmul_rn(__fmul_rn(sg, sg), 2.f);
  const float rbf = __fadd_rn(__fsqrt_rn(__fmul_rn(16.f, w.two_s2)), 1.f);
  const long long rb = rbf < (float)(H + W) ? (long long)rbf : (long long)(H + W);   // NaN: all
  const long long lx = (long long)cx - rb, hx = (long long)cx + rb;
  const long long ly = (long long)cy - rb, hy = (long long)cy + rb;
  w.x0 = (int)(lx < 0 ? 0 : (lx > W ? W : lx));
  w.x1 = (int)(hx > W - 1 ? W - 1 : (hx < -1 ? -1 : hx));
  w.y0 = (int)(ly < 0 ? 0 : (ly > H ? H : ly));
  w.y1 = (int)(hy > H - 1 ? H - 1 : (hy < -1 ? -1 : hy));
  return w;
}

// -d2 / (2 sigma^2) for key (kx, ky); member iff exp(.) >= eps
__device__ __forceinline__ bool gauss_arg(int cx, int cy, int kx, int ky, float two_s2,
                                          float* arg) {
  const float dx = __fsub_rn((float)cx, (float)kx), dy = __fsub_rn((float)cy, (float)ky);
  const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
  *arg = __fdiv_rn(-d2, two_s2);
  return expf(*arg) >= FLT_EPSILON;
}

template <int D>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float* r) {
#pragma unroll
  for (int i = 0; i < D; i += 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + i);
    r[i] = t.x, r[i + 1] = t.y, r[i + 2] = t.z, r[i + 3] = t.w;
  }
}
template <int D>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float* r) {
#pragma unroll
  for (int i = 0; i < D; i += 4)
    *reinterpret_cast<float4*>(p + i) = make_float4(r[i], r[i + 1], r[i + 2], r[i + 3]);
}
template <int D>
__device__ __forceinline__ float dot_row(const float* a, const float* b) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < D; ++i) s = fmaf(a[i], b[i], s);
  return s;
}

// grid (rows, heads), 64 threads
template <int D>
__global__ __launch_bounds__(64) void gauss_attn_fwd_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const int32_t* __restrict__ view, const int32_t* __restrict__ centre,
    const float* __restrict__ sigma, int P, int V, int H, int W, int heads, float scale,
    uint32_t drop_thresh, float inv_keep, uint32_t seed_lo, uint32_t seed_hi,
    float* __restrict__ out, float* __restrict__ lse) {
  const int row = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
  const int C = heads * D;
  const int vw = view[row];
  float acc[D];
#pragma unroll
  for (int i = 0; i < D; ++i) acc[i] = 0.f;
  float m = -INFINITY, l = 0.f;
  if (vw >= 0 && vw < V) {
    const size_t g = (size_t)(row / P) * V + vw;
    const float* kb = k + g * H * W * C + h * D;
    const float* vb = v + g * H * W * C + h * D;
    float qv[D];
    load_row<D>(q + (size_t)row * C + h * D, qv);
#pragma unroll
    for (int i = 0; i < D; ++i) qv[i] *= scale;
    const int cx = centre[2 * row], cy = centre[2 * row + 1];
    const Window w = window_of(cx, cy, sigma[row], H, W);
    const int ww = w.x1 - w.x0 + 1, wh = w.y1 - w.y0 + 1;
    const int n = (ww > 0 && wh > 0) ? ww * wh : 0;
    for (int idx = lane; idx < n; idx += 64) {
      const int ky = w.y0 + idx / ww, kx = w.x0 + idx % ww;
      float arg;
      if (!gauss_arg(cx, cy, kx, ky, w.two_s2, &arg)) continue;
      const int key = ky * W + kx;
      float kr[D];
      load_row<D>(kb + (size_t)key * C, kr);
      const float s = dot_row<D>(qv, kr) + arg;
      float pj = 1.f;
      if (s > m) {
        const float c = expf(m - s);        // m = -inf: 0
        l *= c;
#pragma unroll
        for (int i = 0; i < D; ++i) acc[i] *= c;
        m = s;
      } else {
        pj = expf(s - m);
      }
      l += pj;
      if (drop_thresh != 0u) {
        if (drop_mix(seed_lo, seed_hi, (uint32_t)row, (uint32_t)h, (uint32_t)key) < drop_thresh)
          continue;
        pj *= inv_keep;
      }
      load_row<D>(vb + (size_t)key * C, kr);
#pragma unroll
      for (int i = 0; i < D; ++i) acc[i] = fmaf(pj, kr[i], acc[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float m2 = __shfl_xor(m, o, 64), l2 = __shfl_xor(l, o, 64);
      const float mm = fmaxf(m, m2);
      const float a = m == -INFINITY ? 0.f : expf(m - mm);
      const float b2 = m2 == -INFINITY ? 0.f : expf(m2 - mm);
      l = l * a + l2 * b2;
#pragma unroll
      for (int i = 0; i < D; ++i) acc[i] = acc[i] * a + __shfl_xor(acc[i], o, 64) * b2;
      m = mm;
    }
  }
  if (lane == 0) {
    const bool some = l > 0.f;
    const float inv = some ? 1.f / l : 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i) acc[i] = some ? acc[i] * inv : 0.f;
    store_row<D>(out + (size_t)row * C + h * D, acc);
    lse[(size_t)row * heads + h] = some ? m + logf(l) : 0.f;
  }
}

// grid (rows, heads), 64 threads: dQ and delta = dO . O
template <int D>
__global__ __launch_bounds__(64) void gauss_attn_bwd_q_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const float* __restrict__ o, const float* __restrict__ d_o, const float* __restrict__ lse,
    const int32_t* __restrict__ view, const int32_t* __restrict__ centre,
    const float* __restrict__ sigma, int P, int V, int H, int W, int heads, float scale,
    uint32_t drop_thresh, float inv_keep, uint32_t seed_lo, uint32_t seed_hi,
    float* __restrict__ dq, float* __restrict__ delta) {
  const int row = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
  const int C = heads * D;
  const int vw = view[row];
  float acc[D];
#pragma unroll
  for (int i = 0; i < D; ++i) acc[i] = 0.f;
  float dl = 0.f;
  if (vw >= 0 && vw < V) {
    const size_t g = (size_t)(row / P) * V + vw;
    const float* kb = k + g * H * W * C + h * D;
    const float* vb = v + g * H * W * C + h * D;
    float qv[D], dov[D], tmp[D];
    load_row<D>(q + (size_t)row * C + h * D, qv);
    load_row<D>(d_o + (size_t)row * C + h * D, dov);
    load_row<D>(o + (size_t)row * C + h * D, tmp);
    dl = dot_row<D>(dov, tmp);
#pragma unroll
    for (int i = 0; i < D; ++i) qv[i] *= scale;
    const float ls = lse[(size_t)row * heads + h];
    const int cx = centre[2 * row], cy = centre[2 * row + 1];
    const Window w = window_of(cx, cy, sigma[row], H, W);
    const int ww = w.x1 - w.x0 + 1, wh = w.y1 - w.y0 + 1;
    const int n = (ww > 0 && wh > 0) ? ww * wh : 0;
    for (int idx = lane; idx < n; idx += 64) {
      const int ky = w.y0 + idx / ww, kx = w.x0 + idx % ww;
      float arg;
      if (!gauss_arg(cx, cy, kx, ky, w.two_s2, &arg)) continue;
      const int key = ky * W + kx;
      float kr[D];
      load_row<D>(kb + (size_t)key * C, kr);
      const float pj = expf(dot_row<D>(qv, kr) + arg - ls);
      float wgt = 1.f;
      if (drop_thresh != 0u)
        wgt = drop_mix(seed_lo, seed_hi, (uint32_t)row, (uint32_t)h, (uint32_t)key) < drop_thresh
                  ? 0.f : inv_keep;
      load_row<D>(vb + (size_t)key * C, tmp);
      const float ds = pj * (wgt * dot_row<D>(dov, tmp) - dl);
#pragma unroll
      for (int i = 0; i < D; ++i) acc[i] = fmaf(ds, kr[i], acc[i]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int i = 0; i < D; ++i) acc[i] += __shfl_xor(acc[i], off, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < D; ++i) acc[i] *= scale;
    store_row<D>(dq + (size_t)row * C + h * D, acc);
    delta[(size_t)row * heads + h] = dl;
  }
}

// grid (ceil(H W / kAttnKeyTile), B V, heads), kAttnKeyTile threads: dK and dV
template <int D>
__global__ __launch_bounds__(kAttnKeyTile) void gauss_attn_bwd_kv_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const float* __restrict__ d_o, const float* __restrict__ lse, const float* __restrict__ delta,
    const int32_t* __restrict__ view, const int32_t* __restrict__ centre,
    const float* __restrict__ sigma, int P, int V, int H, int W, int heads, float scale,
    uint32_t drop_thresh, float inv_keep, uint32_t seed_lo, uint32_t seed_hi,
    float* __restrict__ dk, float* __restrict__ dv) {
  __shared__ float s_q[kAttnRowChunk][D], s_do[kAttnRowChunk][D];
  __shared__ float s_two[kAttnRowChunk], s_lse[kAttnRowChunk], s_delta[kAttnRowChunk];
  __shared__ int s_cx[kAttnRowChunk], s_cy[kAttnRowChunk], s_act[kAttnRowChunk];
  const int tid = threadIdx.x, g = blockIdx.y, h = blockIdx.z;
  const int C = heads * D, HW = H * W;
  const int b = g / V, vw = g - b * V;
  const int key0 = blockIdx.x * kAttnKeyTile;
  const int key = key0 + tid;
  const bool live = key < HW;
  const int ky = live ? key / W : 0, kx = live ? key - ky * W : 0;
  const int ty0 = key0 / W, ty1 = min(HW - 1, key0 + kAttnKeyTile - 1) / W;
  float kr[D], vr[D], dka[D], dva[D];
#pragma unroll
  for (int i = 0; i < D; ++i) kr[i] = vr[i] = dka[i] = dva[i] = 0.f;
  const size_t koff = ((size_t)g * HW + (live ? key : 0)) * C + h * D;
  if (live) {
    load_row<D>(k + koff, kr);
    load_row<D>(v + koff, vr);
  }
  for (int base = 0; base < P; base += kAttnRowChunk) {
    const int cnt = min(P - base, kAttnRowChunk);
    __syncthreads();
    if (tid < cnt) {
      const int row = b * P + base + tid;
      const int cx = centre[2 * row], cy = centre[2 * row + 1];
      const Window w = window_of(cx, cy, sigma[row], H, W);
      s_act[tid] = view[row] == vw && w.y0 <= ty1 && w.y1 >= ty0 && w.x0 <= w.x1;
      s_cx[tid] = cx, s_cy[tid] = cy, s_two[tid] = w.two_s2;
      s_lse[tid] = lse[(size_t)row * heads + h];
      s_delta[tid] = delta[(size_t)row * heads + h];
    }
    for (int i = tid; i < cnt * D; i += kAttnKeyTile) {
      const int r = i / D, c = i - r * D;
      const size_t off = (size_t)(b * P + base + r) * C + h * D + c;
      s_q[r][c] = q[off] * scale;
      s_do[r][c] = d_o[off];
    }
    __syncthreads();
    for (int r = 0; r < cnt; ++r) {
      if (!s_act[r]) continue;                      // uniform over the block
      float arg;
      if (!live || !gauss_arg(s_cx[r], s_cy[r], kx, ky, s_two[r], &arg)) continue;
      float sc = 0.f, dov = 0.f;
#pragma unroll
      for (int i = 0; i < D; ++i) sc = fmaf(s_q[r][i], kr[i], sc), dov = fmaf(s_do[r][i], vr[i], dov);
      const float pj = expf(sc + arg - s_lse[r]);
      float wgt = 1.f;
      if (drop_thresh != 0u)
        wgt = drop_mix(seed_lo, seed_hi, (uint32_t)(b * P + base + r), (uint32_t)h,
                       (uint32_t)key) < drop_thresh ? 0.f : inv_keep;
      const float pw = pj * wgt;
      const float ds = pj * (wgt * dov - s_delta[r]);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        dva[i] = fmaf(pw, s_do[r][i], dva[i]);
        dka[i] = fmaf(ds, s_q[r][i], dka[i]);       // s_q carries 1 / sqrt(d)
      }
    }
  }
  if (live) {
    store_row<D>(dk + koff, dka);
    store_row<D>(dv + koff, dva);
  }
}

inline int head_dim(int channels, int heads) {
  if (heads < 1 || channels < 1 || channels > 256 || channels % heads) return 0;
  const int d = channels / heads;
  return (d == 8 || d == 16 || d == 32) ? d : 0;
}

struct AttnArgs {
  const float *q, *k, *v;
  const int32_t *view, *centre;
  const float* sigma;
  int rows, P, V, H, W, heads;
  float scale, inv_keep;
  uint32_t thresh, seed_lo, seed_hi;
};

template <int D>
void launch_fwd(const AttnArgs& a, float* out, float* lse, hipStream_t st) {
  MSMD_LAUNCH(gauss_attn_fwd_kernel<D>, dim3(a.rows, a.heads), dim3(64), 0, st, a.q, a.k, a.v,
              a.view, a.centre, a.sigma, a.P, a.V, a.H, a.W, a.heads, a.scale, a.thresh,
              a.inv_keep, a.seed_lo, a.seed_hi, out, lse);
}
template <int D>
void launch_bwd(const AttnArgs& a, const float* o, const float* d_o, const float* lse, float* dq,
                float* dk, float* dv, float* delta, hipStream_t st) {
  MSMD_LAUNCH(gauss_attn_bwd_q_kernel<D>, dim3(a.rows, a.heads), dim3(64), 0, st, a.q, a.k, a.v,
              o, d_o, lse, a.view, a.centre, a.sigma, a.P, a.V, a.H, a.W, a.heads, a.scale,
              a.thresh, a.inv_keep, a.seed_lo, a.seed_hi, dq, delta);
  MSMD_LAUNCH(gauss_attn_bwd_kv_kernel<D>,
              dim3(ceil_div((long)a.H * a.W, kAttnKeyTile), (a.rows / a.P) * a.V, a.heads),
              dim3(kAttnKeyTile), 0, st, a.q, a.k, a.v, d_o, lse, delta, a.view, a.centre,
              a.sigma, a.P, a.V, a.H, a.W, a.heads, a.scale, a.thresh, a.inv_keep, a.seed_lo,
              a.seed_hi, dk, dv);
}

// 0: launch; 1: nothing to do; < 0: refusal
int check_attn(int batch, int P, int V, int H, int W, int channels, int heads, float dropout,
               uint64_t seed, AttnArgs* a) {
  if (batch < 0 || P < 0 || V < 1 || H < 1 || W < 1 || !(dropout >= 0.f) || !(dropout < 1.f))
    return MSMD_ERR_INVALID_ARG;
  const int d = head_dim(channels, heads);
  if (!d) return MSMD_ERR_UNSUPPORTED;
  if (V > kGeoMaxViews || heads > 65535 || (long)batch * V > 65535) return MSMD_ERR_UNSUPPORTED;
  if ((long)batch * P * channels >= 2147483647L ||
      (long)batch * V * H * W * channels >= 2147483647L)
    return MSMD_ERR_RANGE;
  a->rows = batch * P, a->P = P, a->V = V, a->H = H, a->W = W, a->heads = heads;
  a->scale = 1.f / sqrtf((float)d);
  const double t = floor((double)dropout * 4294967296.0);
  a->thresh = dropout > 0.f ? (uint32_t)(t > 4294967295.0 ? 4294967295.0 : t) : 0u;
  a->inv_keep = 1.f / (1.f - dropout);
  a->seed_lo = (uint32_t)seed, a->seed_hi = (uint32_t)(seed >> 32);
  return (batch == 0 || P == 0) ? 1 : 0;
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_img_query_geometry_max_queries(void) { return kGeoBlock * kGeoPerThread; }
MSMD_EXPORT int msmd_img_query_geometry_max_views(void) { return kGeoMaxViews; }

MSMD_EXPORT int msmd_img_query_geometry_f32(
    const float* pos3d, const float* boxes, const msmd_point_sample_params* params, int batch,
    int num_queries, int num_views, float out_size_factor_img, uint8_t* on, float* pos,
    int32_t* centre, int32_t* radius, float* sigma, int32_t* count, uint8_t* valid,
    int32_t* winner, uint8_t* mask, float* win_pos, int32_t* win_centre, float* win_sigma,
    msmd_stream_t stream) {
  if (batch < 0 || num_queries < 0 || num_views < 1 || !(out_size_factor_img > 0.f))
    return MSMD_ERR_INVALID_ARG;
  if (num_queries > kGeoBlock * kGeoPerThread || num_views > kGeoMaxViews)
    return MSMD_ERR_UNSUPPORTED;
  if ((long)batch * num_views * num_queries * 2 >= 2147483647L) return MSMD_ERR_RANGE;
  if (batch == 0) return MSMD_OK;
  if (!params || !count || !valid) return MSMD_ERR_INVALID_ARG;
  if (num_queries > 0 && (!pos3d || !boxes || !on || !pos || !centre || !radius || !sigma ||
                          !winner || !mask || !win_pos || !win_centre || !win_sigma))
    return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(img_query_geometry_kernel, dim3(batch), dim3(kGeoBlock), 0, (hipStream_t)stream,
              pos3d, boxes, params, num_queries, num_views, out_size_factor_img, on, pos, centre,
              radius, sigma, count, valid, winner, mask, win_pos, win_centre, win_sigma);
  return launch_status();
}

MSMD_EXPORT int msmd_gauss_attn_supported(int channels, int heads) {
  return head_dim(channels, heads) != 0;
}
MSMD_EXPORT int msmd_gauss_attn_key_tile(void) { return kAttnKeyTile; }
MSMD_EXPORT int msmd_gauss_attn_row_chunk(void) { return kAttnRowChunk; }

MSMD_EXPORT int msmd_gauss_attn_fwd_f32(
    const float* q, const float* k, const float* v, const int32_t* view, const int32_t* centre,
    const float* sigma, int batch, int num_queries, int num_views, int h, int w, int channels,
    int heads, float dropout, uint64_t seed, float* out, float* lse, msmd_stream_t stream) {
  AttnArgs a;
  const int rc = check_attn(batch, num_queries, num_views, h, w, channels, heads, dropout, seed, &a);
  if (rc) return rc < 0 ? rc : MSMD_OK;
  if (!q || !k || !v || !view || !centre || !sigma || !out || !lse) return MSMD_ERR_INVALID_ARG;
  a.q = q, a.k = k, a.v = v, a.view = view, a.centre = centre, a.sigma = sigma;
  hipStream_t st = (hipStream_t)stream;
  switch (channels / heads) {
    case 8: launch_fwd<8>(a, out, lse, st); break;
    case 16: launch_fwd<16>(a, out, lse, st); break;
    default: launch_fwd<32>(a, out, lse, st); break;
  }
  return launch_status();
}

MSMD_EXPORT int msmd_gauss_attn_bwd_f32(
    const float* q, const float* k, const float* v, const float* out, const float* grad_out,
    const float* lse, const int32_t* view, const int32_t* centre, const float* sigma, int batch,
    int num_queries, int num_views, int h, int w, int channels, int heads, float dropout,
    uint64_t seed, float* grad_q, float* grad_k, float* grad_v, float* delta,
    msmd_stream_t stream) {
  AttnArgs a;
  const int rc = check_attn(batch, num_queries, num_views, h, w, channels, heads, dropout, seed, &a);
  if (rc < 0) return rc;
  if (batch == 0) return MSMD_OK;
  if (!grad_k || !grad_v) return MSMD_ERR_INVALID_ARG;
  a.q = q, a.k = k, a.v = v, a.view = view, a.centre = centre, a.sigma = sigma;
  hipStream_t st = (hipStream_t)stream;
  if (rc == 1) {       // no rows: every key's gradient is zero
    const size_t bytes = sizeof(float) * (size_t)batch * num_views * h * w * channels;
    if (hipMemsetAsync(grad_k, 0, bytes, st) != hipSuccess ||
        hipMemsetAsync(grad_v, 0, bytes, st) != hipSuccess)
      return MSMD_ERR_LAUNCH;
    return MSMD_OK;
  }
  if (!q || !k || !v || !out || !grad_out || !lse || !view || !centre || !sigma || !grad_q ||
      !delta)
    return MSMD_ERR_INVALID_ARG;
  switch (channels / heads) {
    case 8: launch_bwd<8>(a, out, grad_out, lse, grad_q, grad_k, grad_v, delta, st); break;
    case 16: launch_bwd<16>(a, out, grad_out, lse, grad_q, grad_k, grad_v, delta, st); break;
    default: launch_bwd<32>(a, out, grad_out, lse, grad_q, grad_k, grad_v, delta, st); break;
  }
  return launch_status();
}
