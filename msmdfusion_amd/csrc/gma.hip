// gma.hip -- the feature assembly of one GMA-Conv stage as ONE launch each way.
//
// SparseMultiModalEncoderPaint.grouped_sparse_conv
// (mmdet3d/models/middle_encoders/sparse_encoder_multimodal_encoderpaint_double_aware.py:325-430)
// builds the unified voxel set's features from three row groups:
//     only-3D rows:  [ conv3D(only-3D voxels)            | 0 (c2) ]
//     only-2D rows:  [ 0 (c3) | cross_gate[nearest 3D voxel] * feat2D[row]   ]
//     mixed rows:    [ feat3D[row3] | gate(feat3D[row3]) * feat2D[row2]      ]
// -- in the reference (and in this repo until round 3) a dozen indexing / cat / pad / mul
// launches per stage and twice that in backward (three index_add_ with their zero fills:
// 0.63 ms of the 14.5 ms LC step).  Everything around the two Linear+ReLU gates is HBM-bound
// row copying: one thread per 16-byte piece of an output row.  (The gates themselves -- skinny
// fp32 GEMMs that hipBLASLt ran at a few TF -- are the row-streaming kernels at the end of
// this file: msmd_rows_linear_*.)
//
// backward: d conv3D = the left block of the only-3D rows; d gate = right block of the mixed
// rows * feat2D; d cross_gate[t] = sum over the only-2D rows whose nearest voxel is t of
// right block * feat2D -- a segmented sum over rows sorted by nearest voxel (`order` /
// `starts` from the index pass: one wave per target row, fixed order, deterministic; the
// dummy row that all unmatched rows share is spread over kDummyBlocks blocks and reduced);
// without the sorted lists: float atomics, as torch's index_add_ (the one it replaces).
// feat3D / feat2D get no gradient (frozen LiDAR encoder, raw virtual-point voxels): the
// Python wrapper falls back to the unfused ops when they ask for one.
#include "common.hpp"

namespace msmd {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct GmaArgs {
  const float* conv3;     // [n_o3, c3]
  const float* cross;     // [n3 + 1, c2]   (row n3 = the dummy embedding's gate)
  const float* feat2;     // [n2, c2]
  const float* feat3;     // [n3, c3]
  const float* gate;      // [n_mix, c2]
  const int64_t* nn3;     // [n_o2]  nearest 3D voxel of an only-2D row, -1 = none
  const int64_t* rows_o2; // [n_o2]  row of feat2
  const int64_t* rows_m3; // [n_mix] row of feat3
  const int64_t* rows_m2; // [n_mix] row of feat2
  int n_o3, n_o2, n_o2_pad, n_mix, n_mix_pad, n3, c3, c2;
};

__global__ __launch_bounds__(256) void gma_assemble_fwd_kernel(GmaArgs A, float* __restrict__ out) {
  const int c = A.c3 + A.c2, c4 = c >> 2, k3 = A.c3 >> 2;
  const long rows = (long)A.n_o3 + A.n_o2 + A.n_o2_pad + A.n_mix + A.n_mix_pad;
  const long total = rows * c4;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long row = e / c4;
    const int q = (int)(e - row * c4);        // 16-byte piece inside the row
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < A.n_o3) {
      if (q < k3) v = ((const f32x4*)(A.conv3 + (size_t)row * A.c3))[q];
    } else if (row < (long)A.n_o3 + A.n_o2) {
      if (q >= k3) {
        const long i = row - A.n_o3;
        long t = A.nn3[i];
        t = t >= 0 ? t : A.n3;
        v = ((const f32x4*)(A.cross + (size_t)t * A.c2))[q - k3] *
            ((const f32x4*)(A.feat2 + (size_t)A.rows_o2[i] * A.c2))[q - k3];
      }
    } else if (row >= (long)A.n_o3 + A.n_o2 + A.n_o2_pad &&
               row < (long)A.n_o3 + A.n_o2 + A.n_o2_pad + A.n_mix) {
      const long i = row - A.n_o3 - A.n_o2 - A.n_o2_pad;
      if (q < k3)
        v = ((const f32x4*)(A.feat3 + (size_t)A.rows_m3[i] * A.c3))[q];
      else
        v = ((const f32x4*)(A.gate + (size_t)i * A.c2))[q - k3] *
            ((const f32x4*)(A.feat2 + (size_t)A.rows_m2[i] * A.c2))[q - k3];
    }
    ((f32x4*)out)[e] = v;
  }
}

__global__ __launch_bounds__(256) void gma_assemble_bwd_kernel(GmaArgs A,
                                                               const float* __restrict__ dout,
                                                               float* __restrict__ d_conv3,
                                                               float* __restrict__ d_cross,
                                                               float* __restrict__ d_gate) {
  const int c = A.c3 + A.c2, c4 = c >> 2, k3 = A.c3 >> 2;
  const long rows = (long)A.n_o3 + A.n_o2 + A.n_o2_pad + A.n_mix + A.n_mix_pad;
  const long total = rows * c4;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long row = e / c4;
    const int q = (int)(e - row * c4);
    if (row < A.n_o3) {
      if (q < k3) ((f32x4*)(d_conv3 + (size_t)row * A.c3))[q] = ((const f32x4*)dout)[e];
    } else if (row < (long)A.n_o3 + A.n_o2) {
      if (q >= k3 && d_cross) {   // (no sorted row lists: float atomics)
        const long i = row - A.n_o3;
        long t = A.nn3[i];
        t = t >= 0 ? t : A.n3;
        const f32x4 g = ((const f32x4*)dout)[e] *
                        ((const f32x4*)(A.feat2 + (size_t)A.rows_o2[i] * A.c2))[q - k3];
        float* d = d_cross + (size_t)t * A.c2 + 4 * (q - k3);
#pragma unroll
        for (int s = 0; s < 4; ++s) unsafeAtomicAdd(d + s, g[s]);   // hardware float add (atomicAdd is a CAS loop without -munsafe-fp-atomics)
      }
    } else if (row >= (long)A.n_o3 + A.n_o2 + A.n_o2_pad &&
               row < (long)A.n_o3 + A.n_o2 + A.n_o2_pad + A.n_mix) {
      if (q >= k3 && d_gate) {
        const long i = row - A.n_o3 - A.n_o2 - A.n_o2_pad;
        ((f32x4*)(d_gate + (size_t)i * A.c2))[q - k3] =
            ((const f32x4*)dout)[e] *
            ((const f32x4*)(A.feat2 + (size_t)A.rows_m2[i] * A.c2))[q - k3];
      }
    }
  }
}

// d cross_gate without atomics: the only-2D rows sorted by their nearest voxel (order[],
// starts[t] .. starts[t + 1] = the rows of target t; built once per batch by the index pass).
// Targets t < n3: one wave each -- its four 16-lane groups take every fourth row of the
// segment (a lane = one 16-byte piece of the c2-wide row), the four partial sums are added
// in group order.  Target n3 -- the dummy embedding's row, which gates EVERY only-2D voxel
// without a LiDAR neighbour: thousands of rows, 1.1 ms when one wave walked them alone -- is
// spread over kDummyBlocks extra workgroups of 16 groups (block partials in group order,
// then gma_cross_dummy_kernel adds the block partials in block order).  Fixed order
// throughout: deterministic, unlike the index_add_ this replaces; every target row is
// written (no zero fill).  c2 <= 64.
constexpr int kDummyBlocks = 64;
__device__ __forceinline__ f32x4 cross_term(const GmaArgs& A, const float* __restrict__ dout,
                                            long i, int c, int l) {
  return ((const f32x4*)(dout + (size_t)(A.n_o3 + i) * c + A.c3))[l] *
         ((const f32x4*)(A.feat2 + (size_t)A.rows_o2[i] * A.c2))[l];
}
__global__ __launch_bounds__(256) void gma_cross_grad_kernel(GmaArgs A, const float* __restrict__ dout,
                                                             const int64_t* __restrict__ order,
                                                             const int64_t* __restrict__ starts,
                                                             float* __restrict__ d_cross,
                                                             float* __restrict__ dummy_part,
                                                             int target_blocks) {
  const int lane = threadIdx.x & 63, g = lane >> 4, l = lane & 15, wave = threadIdx.x >> 6;
  const int c = A.c3 + A.c2, q2 = A.c2 >> 2;
  if ((int)blockIdx.x >= target_blocks) {   // a slice of the dummy row's segment
    __shared__ f32x4 sm[16][16];
    const int db = blockIdx.x - target_blocks, grp = wave * 4 + g;
    const long s0 = starts[A.n3], s1 = starts[A.n3 + 1];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (l < q2)
      for (long p = s0 + db * 16 + grp; p < s1; p += 16 * kDummyBlocks)
        acc += cross_term(A, dout, order[p], c, l);
    sm[grp][l] = acc;
    __syncthreads();
    if (threadIdx.x < q2) {
      f32x4 r = sm[0][threadIdx.x];
      for (int k = 1; k < 16; ++k) r += sm[k][threadIdx.x];
      ((f32x4*)(dummy_part + (size_t)db * A.c2))[threadIdx.x] = r;
    }
    return;
  }
  const long t = (long)blockIdx.x * 4 + wave;
  if (t >= A.n3) return;
  const long s0 = starts[t], s1 = starts[t + 1];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (l < q2)
    for (long p = s0 + g; p < s1; p += 4) acc += cross_term(A, dout, order[p], c, l);
  f32x4 r = acc;   // groups 1..3 -> group 0, in group order
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    f32x4 o;
#pragma unroll
    for (int s = 0; s < 4; ++s) o[s] = __shfl(acc[s], l + 16 * k, 64);
    r += o;
  }
  if (g == 0 && l < q2) ((f32x4*)(d_cross + (size_t)t * A.c2))[l] = r;
}
__global__ __launch_bounds__(64) void gma_cross_dummy_kernel(const float* __restrict__ dummy_part,
                                                             int c2, float* __restrict__ d_row) {
  const int l = threadIdx.x;
  if (l >= (c2 >> 2)) return;
  f32x4 r = ((const f32x4*)dummy_part)[l];
  for (int k = 1; k < kDummyBlocks; ++k) r += ((const f32x4*)(dummy_part + (size_t)k * c2))[l];
  ((f32x4*)d_row)[l] = r;
}

inline int grid_for(long total) {
  long b = (total + 255) / 256;
  return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}

bool fill_args(GmaArgs& A, const float* conv3, int n_o3, int c3, const float* cross, int n3,
               int c2, const int64_t* nn3, const float* feat2, const int64_t* rows_o2, int n_o2,
               int n_o2_pad, const float* feat3, const int64_t* rows_m3, const float* gate,
               const int64_t* rows_m2, int n_mix, int n_mix_pad) {
  if (c3 < 4 || c2 < 4 || (c3 & 3) || (c2 & 3) || n_o3 < 0 || n_o2 < 0 || n_mix < 0 ||
      n_o2_pad < 0 || n_mix_pad < 0 || n3 < 0)
    return false;
  if ((n_o3 && !conv3) || (n_o2 && (!cross || !nn3 || !feat2 || !rows_o2)) ||
      (n_mix && (!feat3 || !rows_m3 || !gate || !rows_m2 || !feat2)))
    return false;
  A = GmaArgs{conv3, cross, feat2, feat3, gate, nn3, rows_o2, rows_m3, rows_m2,
              n_o3,  n_o2,  n_o2_pad, n_mix, n_mix_pad, n3, c3, c2};
  return true;
}


// ---------------------------------------------------------------- gate linears --
// gate_control / cross_gate_control: nn.Sequential(nn.Linear(c3, 64), nn.ReLU()) over the
// rows of a stage's 3-D voxels (sparse_multimodal_encoder_painting.py:83-96, applied at
// :398-417).  hipBLASLt's fp32 GEMM took 170-230 us per call on these skinny shapes
// ([75k..150k] x [16..128] x 64: under 1 GFLOP, 57 MB of traffic) and the step makes 16 of
// them; they are row-streaming passes: y = relu(x W^T + b) with W in LDS, and for backward
// per-block partial sums of dW = g^T x, db = sum g (g = dy where y > 0), added in block
// order (fixed: deterministic).  fp32 FMAs in k order; results differ from the GEMM's by
// its different summation order only (~1e-7 relative).
// rows per block, forward (whole passes of 32..128) / backward (one partial each).  128 / 128:
// with 256 the 60-150 k-row tables gave every CU ONE 4-wave workgroup -- a single wave per SIMD
// waiting out its own LDS latencies -- and the 128-channel backward pass took 75 us; at 128
// rows it takes 49 (the partials' reduction 6 -> 11 us).
constexpr int kLinRowsPerBlock = 128;
constexpr int kLinBwdRows = 128;
constexpr int kLinBwdTile = 32;         // ... staged in LDS this many at a time

__global__ __launch_bounds__(256) void rows_linear_fwd_kernel(
    const float* __restrict__ x, int n, const float* __restrict__ x_tail, int n_tail, int cin,
    const float* __restrict__ w, const float* __restrict__ b, int cout, int relu,
    float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float lin_smem[];
  constexpr int RT = 4;                      // rows per thread: a W piece read from LDS serves 4
  float* wt = lin_smem;                      // [cin][cout]: W transposed
  const int xs_ld = cin + 4;                 // (+4: rows of a pass land in different banks)
  float* xs = wt + cin * cout;               // [rows per pass][xs_ld]
  const int cg = cout >> 2, rg = 256 / cg;   // column groups of 4, row groups per pass
  const int rpp = rg * RT;                   // rows per pass
  const int tid = threadIdx.x;
  // (LDS writes in address order; w is a few KB and comes from L1/L2 either way)
  for (int e = tid; e < cin * cout; e += 256) {
    const int k = e / cout, co = e - k * cout;
    wt[e] = w[co * cin + k];
  }
  const int g = tid % cg, r = tid / cg;
  f32x4 bias = {0.f, 0.f, 0.f, 0.f};
  if (b) bias = *(const f32x4*)(b + 4 * g);
  const long total = (long)n + n_tail;
  const long row0 = (long)blockIdx.x * kLinRowsPerBlock;
  const int c4 = cin >> 2;
  // a pass's x tile = rpp * c4 16-byte pieces, at most kLinFwdPre per thread (cin <= 4 cout);
  // the next pass's pieces are loaded into registers while this one is multiplied
  constexpr int kLinFwdPre = 4 * RT;
  f32x4 pre[kLinFwdPre];
  auto fetch = [&](int p0) {
#pragma unroll
    for (int u = 0; u < kLinFwdPre; ++u) {
      const int e = tid + 256 * u;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (e < rpp * c4) {
        const int rr = e / c4, k4 = e - rr * c4;
        const long row = row0 + p0 + rr;
        if (row < n) v = *(const f32x4*)(x + row * cin + 4 * k4);
        else if (row < total) v = *(const f32x4*)(x_tail + (row - n) * cin + 4 * k4);
      }
      pre[u] = v;
    }
  };
  fetch(0);
  for (int p0 = 0; p0 < kLinRowsPerBlock; p0 += rpp) {
    if (row0 + p0 >= total) break;
    __syncthreads();   // wt filled (first pass) / the previous pass's xs consumed
#pragma unroll
    for (int u = 0; u < kLinFwdPre; ++u) {
      const int e = tid + 256 * u;
      if (e < rpp * c4) {
        const int rr = e / c4, k4 = e - rr * c4;
        *(f32x4*)(xs + rr * xs_ld + 4 * k4) = pre[u];
      }
    }
    __syncthreads();
    if (p0 + rpp < kLinRowsPerBlock) fetch(p0 + rpp);
    f32x4 acc[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[t] = bias;
    for (int k = 0; k < cin; k += 4) {
      f32x4 xv[RT];
#pragma unroll
      for (int t = 0; t < RT; ++t) xv[t] = *(const f32x4*)(xs + (r + rg * t) * xs_ld + k);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 wv = *(const f32x4*)(wt + (k + j) * cout + 4 * g);
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t] += xv[t][j] * wv;
      }
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const long row = row0 + p0 + r + rg * t;
      if (row >= total) continue;
      f32x4 a = acc[t];
      if (relu) {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = a[j] > 0.f ? a[j] : 0.f;
      }
      *(f32x4*)(y + row * cout + 4 * g) = a;
    }
  }
}

// part[blk][cout * cin + cout]: this block's dW (as [cout][cin]) and db
template <int CPT>
__global__ __launch_bounds__(256) void rows_linear_bwd_partial_kernel(
    const float* __restrict__ x, int n, const float* __restrict__ x_tail, int n_tail, int cin,
    const float* __restrict__ y, const float* __restrict__ dy, int cout, int relu,
    float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float lin_smem[];
  const int xs_ld = cin + 4;
  float* gs = lin_smem;                         // [tile][cout]
  float* xs = gs + kLinBwdTile * cout;          // [tile][xs_ld]
  const int tid = threadIdx.x;
  const int co = tid % cout, grp = tid / cout;  // this thread: dW[co][grp * CPT .. + CPT)
  float acc[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) acc[j] = 0.f;
  float accb = 0.f;
  const long total = (long)n + n_tail;
  const long row0 = (long)blockIdx.x * kLinBwdRows;
  const int c4 = cin >> 2, o4 = cout >> 2;
  // the next tile's pieces travel in registers while this one is accumulated
  constexpr int kPreG = kLinBwdTile * 32 / 256, kPreX = kLinBwdTile * 64 / 256;   // cout <= 128, cin <= 256
  f32x4 pg[kPreG], px[kPreX];
  auto fetch = [&](int p0) {
#pragma unroll
    for (int u = 0; u < kPreG; ++u) {
      const int e = tid + 256 * u;
      f32x4 gv = {0.f, 0.f, 0.f, 0.f};
      if (e < kLinBwdTile * o4) {
        const int rr = e / o4, q = e - rr * o4;
        const long row = row0 + p0 + rr;
        if (row < total) {
          gv = *(const f32x4*)(dy + row * cout + 4 * q);
          if (relu) {
            const f32x4 yv = *(const f32x4*)(y + row * cout + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) gv[j] = yv[j] > 0.f ? gv[j] : 0.f;
          }
        }
      }
      pg[u] = gv;
    }
#pragma unroll
    for (int u = 0; u < kPreX; ++u) {
      const int e = tid + 256 * u;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (e < kLinBwdTile * c4) {
        const int rr = e / c4, k4 = e - rr * c4;
        const long row = row0 + p0 + rr;
        if (row < n) v = *(const f32x4*)(x + row * cin + 4 * k4);
        else if (row < total) v = *(const f32x4*)(x_tail + (row - n) * cin + 4 * k4);
      }
      px[u] = v;
    }
  };
  fetch(0);
  for (int p0 = 0; p0 < kLinBwdRows; p0 += kLinBwdTile) {
    if (row0 + p0 >= total) break;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPreG; ++u) {
      const int e = tid + 256 * u;
      if (e < kLinBwdTile * o4) *(f32x4*)(gs + (e / o4) * cout + 4 * (e % o4)) = pg[u];
    }
#pragma unroll
    for (int u = 0; u < kPreX; ++u) {
      const int e = tid + 256 * u;
      if (e < kLinBwdTile * c4) *(f32x4*)(xs + (e / c4) * xs_ld + 4 * (e % c4)) = px[u];
    }
    __syncthreads();
    if (p0 + kLinBwdTile < kLinBwdRows) fetch(p0 + kLinBwdTile);
#pragma unroll 4
    for (int rr = 0; rr < kLinBwdTile; ++rr) {
      const float gv = gs[rr * cout + co];
      const float* xr = xs + rr * xs_ld + grp * CPT;
#pragma unroll
      for (int j = 0; j < CPT; j += 4) {
        const f32x4 xv = *(const f32x4*)(xr + j);
        acc[j] += gv * xv[0];
        acc[j + 1] += gv * xv[1];
        acc[j + 2] += gv * xv[2];
        acc[j + 3] += gv * xv[3];
      }
      accb += gv;
    }
  }
  float* out = part + (size_t)blockIdx.x * ((size_t)cout * cin + cout);
#pragma unroll
  for (int j = 0; j < CPT; ++j) out[(size_t)co * cin + grp * CPT + j] = acc[j];
  if (grp == 0) out[(size_t)cout * cin + co] = accb;
}

// d[e] = sum over blocks of part[blk][e] in a fixed order: a workgroup owns 64 entries, its
// four waves each add up every fourth block (8 loads in flight), the four sums are added in
// wave order.  (One thread per entry walking all blocks was 33 workgroups for the 128 x 64
// layer's 8256 entries: 17 us for 7.8 MB.)
__global__ __launch_bounds__(256) void rows_linear_bwd_reduce_kernel(
    const float* __restrict__ part, int nblk, int entries, int per_w, float* __restrict__ dw,
    float* __restrict__ db) {
  __shared__ float sm[4][64];
  const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (e < entries) {
    int bk = slice;
    for (; bk + 28 < nblk; bk += 32) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(bk + 4 * u) * entries + e];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; bk < nblk; bk += 4) s += part[(size_t)bk * entries + e];
  }
  sm[slice][lane] = s;
  __syncthreads();
  if (slice || e >= entries) return;
  s = ((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane];
  if (e < per_w) dw[e] = s;
  else if (db) db[e - per_w] = s;
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_gma_assemble_fwd_f32(const float* conv3, int n_o3, int c3,
                                          const float* cross_gate, int n3, int c2,
                                          const int64_t* nn3, const float* feat2,
                                          const int64_t* rows_o2, int n_o2, int n_o2_pad,
                                          const float* feat3, const int64_t* rows_m3,
                                          const float* gate, const int64_t* rows_m2, int n_mix,
                                          int n_mix_pad, float* out, msmd_stream_t stream) {
  GmaArgs A;
  if (!fill_args(A, conv3, n_o3, c3, cross_gate, n3, c2, nn3, feat2, rows_o2, n_o2, n_o2_pad,
                 feat3, rows_m3, gate, rows_m2, n_mix, n_mix_pad))
    return MSMD_ERR_INVALID_ARG;
  const long rows = (long)n_o3 + n_o2 + n_o2_pad + n_mix + n_mix_pad;
  if (rows == 0) return MSMD_OK;
  if (!out) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(gma_assemble_fwd_kernel, dim3(grid_for(rows * ((c3 + c2) >> 2))), dim3(256), 0,
              (hipStream_t)stream, A, out);
  return launch_status();
}

MSMD_EXPORT size_t msmd_gma_assemble_bwd_workspace_floats(int c2) {
  return (size_t)kDummyBlocks * (c2 > 0 ? c2 : 0);
}

MSMD_EXPORT int msmd_gma_assemble_bwd_f32(const float* d_out, int n_o3, int c3, int n3, int c2,
                                          const int64_t* nn3, const float* feat2,
                                          const int64_t* rows_o2, int n_o2, int n_o2_pad,
                                          const int64_t* rows_m2, int n_mix, int n_mix_pad,
                                          float* d_conv3 /* [n_o3,c3] */,
                                          float* d_cross_gate /* [n3+1,c2] or NULL */,
                                          float* d_gate /* [n_mix,c2] or NULL */,
                                          const int64_t* order /* [n_o2] or NULL */,
                                          const int64_t* starts /* [n3+2] or NULL */,
                                          float* workspace /* msmd_gma_assemble_bwd_workspace_floats */,
                                          msmd_stream_t stream) {
  GmaArgs A;
  // (the forward-only operands are not read in backward)
  if (!fill_args(A, d_conv3, n_o3, c3, d_cross_gate ? d_cross_gate : (const float*)d_out, n3, c2,
                 nn3, feat2, rows_o2, n_o2, n_o2_pad, d_out, rows_m2, d_out, rows_m2, n_mix,
                 n_mix_pad))
    return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const bool csr = d_cross_gate && order && starts && workspace && c2 <= 64;
  if (d_cross_gate && !csr)
    hipMemsetAsync(d_cross_gate, 0, sizeof(float) * ((size_t)n3 + 1) * c2, st);
  const long rows = (long)n_o3 + n_o2 + n_o2_pad + n_mix + n_mix_pad;
  if (!d_out && rows) return MSMD_ERR_INVALID_ARG;
  if (csr) {
    const int tb = ceil_div(n3 > 0 ? n3 : 1, 4);
    MSMD_LAUNCH(gma_cross_grad_kernel, dim3(tb + kDummyBlocks), dim3(256), 0, st, A, d_out, order,
                starts, d_cross_gate, workspace, tb);
    MSMD_LAUNCH(gma_cross_dummy_kernel, dim3(1), dim3(64), 0, st, (const float*)workspace, c2,
                d_cross_gate + (size_t)n3 * c2);
  }
  if (rows == 0) return launch_status();
  if (n_o3 && !d_conv3) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(gma_assemble_bwd_kernel, dim3(grid_for(rows * ((c3 + c2) >> 2))), dim3(256), 0, st,
              A, d_out, d_conv3, csr ? (float*)nullptr : d_cross_gate, d_gate);
  return launch_status();
}


namespace {
inline size_t rows_linear_fwd_smem(int cin, int cout) {
  const int rpp = 4 * (256 / (cout >> 2));    // (RT rows per thread)
  return sizeof(float) * ((size_t)cin * cout + (size_t)rpp * (cin + 4));
}
}  // namespace

// y[(n + n_tail), cout] = relu?(cat(x, x_tail) @ w^T + b); w is nn.Linear's [cout, cin].
MSMD_EXPORT int msmd_rows_linear_supported(int cin, int cout) {
  // channel groups of 4; cout threads per row group; the backward's thread layout: it is
  // instantiated for 4, 8, 16, 32 and 64 input channels per thread -- a shape the forward
  // would take and the backward refuse (cin = 48 with cout = 64) is not supported at all;
  // the forward's W + row tile must fit the CU's 160 KB of LDS
  if (!(cout == 32 || cout == 64 || cout == 128) || cin < 4 || cin > 256 || cin > 4 * cout ||
      cin % (256 / cout) != 0)
    return 0;
  const int cpt = cin / (256 / cout);
  if (!(cpt == 4 || cpt == 8 || cpt == 16 || cpt == 32 || cpt == 64)) return 0;
  return rows_linear_fwd_smem(cin, cout) <= 160 * 1024;
}

MSMD_EXPORT int msmd_rows_linear_fwd_f32(const float* x, int n, const float* x_tail, int n_tail,
                                         int cin, const float* w, const float* b, int cout,
                                         int relu, float* y, msmd_stream_t stream) {
  if (!msmd_rows_linear_supported(cin, cout)) return MSMD_ERR_UNSUPPORTED;
  if (n < 0 || n_tail < 0 || !w || (n && !x) || (n_tail && !x_tail)) return MSMD_ERR_INVALID_ARG;
  const long total = (long)n + n_tail;
  if (total == 0) return MSMD_OK;
  if (!y) return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t smem = rows_linear_fwd_smem(cin, cout);
  static LdsGrant granted;
  const int rc = optin_dynamic_lds((const void*)rows_linear_fwd_kernel, smem, granted);
  if (rc != MSMD_OK) return rc;
  MSMD_LAUNCH(rows_linear_fwd_kernel, dim3(ceil_div(total, kLinRowsPerBlock)), dim3(256), smem, st,
              x, n, x_tail, n_tail, cin, w, b, cout, relu, y);
  return launch_status();
}

MSMD_EXPORT size_t msmd_rows_linear_bwd_workspace_bytes(int n_total, int cin, int cout) {
  const size_t nblk = ceil_div(n_total > 0 ? n_total : 1, kLinBwdRows);
  return align_up(sizeof(float) * nblk * ((size_t)cout * cin + cout));
}

// dw[cout, cin] = g^T cat(x, x_tail), db[cout] = column sums of g, g = dy (where y > 0 if relu)
MSMD_EXPORT int msmd_rows_linear_bwd_f32(const float* x, int n, const float* x_tail, int n_tail,
                                         int cin, const float* y, const float* dy, int cout,
                                         int relu, float* dw, float* db, void* workspace,
                                         size_t workspace_bytes, msmd_stream_t stream) {
  if (!msmd_rows_linear_supported(cin, cout)) return MSMD_ERR_UNSUPPORTED;
  if (n < 0 || n_tail < 0 || !dw || (n && !x) || (n_tail && !x_tail)) return MSMD_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)n + n_tail;
  const int per_w = cout * cin, entries = per_w + cout;
  if (total == 0) {
    (void)hipMemsetAsync(dw, 0, sizeof(float) * per_w, st);
    if (db) (void)hipMemsetAsync(db, 0, sizeof(float) * cout, st);
    return launch_status();
  }
  if (!dy || (relu && !y)) return MSMD_ERR_INVALID_ARG;
  const int nblk = ceil_div(total, kLinBwdRows);
  if (workspace_bytes < sizeof(float) * (size_t)nblk * entries || ((uintptr_t)workspace & 255))
    return MSMD_ERR_WORKSPACE;
  float* part = (float*)workspace;
  const int cpt = cin / (256 / cout);
  const size_t smem = sizeof(float) * ((size_t)kLinBwdTile * cout + (size_t)kLinBwdTile * (cin + 4));
#define MSMD_LIN_BWD(C_)                                                                       \
  MSMD_LAUNCH(rows_linear_bwd_partial_kernel<C_>, dim3(nblk), dim3(256), smem, st, x, n, x_tail, \
              n_tail, cin, y, dy, cout, relu, part)
  switch (cpt) {
    case 4: MSMD_LIN_BWD(4); break;
    case 8: MSMD_LIN_BWD(8); break;
    case 16: MSMD_LIN_BWD(16); break;
    case 32: MSMD_LIN_BWD(32); break;
    case 64: MSMD_LIN_BWD(64); break;
    default: return MSMD_ERR_UNSUPPORTED;
  }
#undef MSMD_LIN_BWD
  MSMD_LAUNCH(rows_linear_bwd_reduce_kernel, dim3(ceil_div(entries, 64)), dim3(256), 0, st,
              (const float*)part, nblk, entries, per_w, dw, db);
  return launch_status();
}
