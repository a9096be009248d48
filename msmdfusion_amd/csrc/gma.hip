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
//
// msmd_gma_stage_* (behind the gate kernels): both gates computed INSIDE the assembly, per
// output row -- no gate table is built, and backward visits only the table rows an only-2D
// row refers to.  Same arithmetic and summation order as the two steps above: same bits.
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
// the sum of one 16-lane group's rows p, p + step, .. < p1 of `order`, in that order; four
// rows' dependent loads (order -> rows_o2 -> feat2) travel together
__device__ __forceinline__ f32x4 cross_chain(const GmaArgs& A, const float* __restrict__ dout,
                                             const int64_t* __restrict__ order, long p, long p1,
                                             long step, int c, int l) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (; p + 3 * step < p1; p += 4 * step) {
    long i[4], r2[4];
    f32x4 a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) i[u] = order[p + u * step];
#pragma unroll
    for (int u = 0; u < 4; ++u) r2[u] = A.rows_o2[i[u]];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = ((const f32x4*)(dout + (size_t)(A.n_o3 + i[u]) * c + A.c3))[l];
      b[u] = ((const f32x4*)(A.feat2 + (size_t)r2[u] * A.c2))[l];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += a[u] * b[u];
  }
  for (; p < p1; p += step) acc += cross_term(A, dout, order[p], c, l);
  return acc;
}
// slice db of the dummy row's segment (a 256-thread workgroup = 16 groups of 16 lanes)
__device__ __forceinline__ void cross_dummy_slice(const GmaArgs& A, const float* __restrict__ dout,
                                                  const int64_t* __restrict__ order,
                                                  const int64_t* __restrict__ starts,
                                                  float* __restrict__ dummy_part, int db) {
  __shared__ f32x4 sm[16][16];
  const int l = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int c = A.c3 + A.c2, q2 = A.c2 >> 2;
  const long s0 = starts[A.n3], s1 = starts[A.n3 + 1];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (l < q2) acc = cross_chain(A, dout, order, s0 + db * 16 + grp, s1, 16 * kDummyBlocks, c, l);
  sm[grp][l] = acc;
  __syncthreads();
  if (threadIdx.x < q2) {
    f32x4 r = sm[0][threadIdx.x];
    for (int k = 1; k < 16; ++k) r += sm[k][threadIdx.x];
    ((f32x4*)(dummy_part + (size_t)db * A.c2))[threadIdx.x] = r;
  }
}
// one target's segment sum, by one wave: the value of lanes 0..15 (group 0) is the row
__device__ __forceinline__ f32x4 cross_segment_sum(const GmaArgs& A, const float* __restrict__ dout,
                                                   const int64_t* __restrict__ order, long s0,
                                                   long s1) {
  const int lane = threadIdx.x & 63, g = lane >> 4, l = lane & 15;
  const int c = A.c3 + A.c2, q2 = A.c2 >> 2;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (l < q2) acc = cross_chain(A, dout, order, s0 + g, s1, 4, c, l);
  f32x4 r = acc;   // groups 1..3 -> group 0, in group order
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    f32x4 o;
#pragma unroll
    for (int s = 0; s < 4; ++s) o[s] = __shfl(acc[s], l + 16 * k, 64);
    r += o;
  }
  return r;
}
__global__ __launch_bounds__(256) void gma_cross_grad_kernel(GmaArgs A, const float* __restrict__ dout,
                                                             const int64_t* __restrict__ order,
                                                             const int64_t* __restrict__ starts,
                                                             float* __restrict__ d_cross,
                                                             float* __restrict__ dummy_part,
                                                             int target_blocks) {
  const int lane = threadIdx.x & 63, g = lane >> 4, l = lane & 15, wave = threadIdx.x >> 6;
  const int q2 = A.c2 >> 2;
  if ((int)blockIdx.x >= target_blocks) {   // a slice of the dummy row's segment
    cross_dummy_slice(A, dout, order, starts, dummy_part, blockIdx.x - target_blocks);
    return;
  }
  const long t = (long)blockIdx.x * 4 + wave;
  if (t >= A.n3) return;
  const f32x4 r = cross_segment_sum(A, dout, order, starts[t], starts[t + 1]);
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

// The gates' arithmetic, in ONE place (the forward tables, the fused stage assembly and the
// ReLU masks its backward recomputes must agree to the bit): RT rows x0 + t * x_stride against
// the column(s) V of W at w_col + k * w_stride; the accumulator starts at the bias, k ascends,
// each step a multiply, then an add (the build has -ffp-contract=off).
template <int RT, typename V>
__device__ __forceinline__ void lin_rows_dot(const float* __restrict__ w_col, int w_stride, int cin,
                                             const float* __restrict__ x0, int x_stride, V bias,
                                             V (&acc)[RT]) {
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t] = bias;
  for (int k = 0; k < cin; k += 4) {
    f32x4 xv[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) xv[t] = *(const f32x4*)(x0 + t * x_stride + k);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const V wv = *(const V*)(w_col + (k + j) * w_stride);
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] += xv[t][j] * wv;
    }
  }
}

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
    lin_rows_dot<RT, f32x4>(wt + 4 * g, cout, cin, xs + r * xs_ld, rg * xs_ld, bias, acc);
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

// ------------------------------------------------------------- the fused stage --
// The two gates computed where the assembly uses them: per only-2D row from its nearest
// voxel's (or the dummy embedding's) feat3 row, per mixed row from its own -- the
// [n3 + 1, c2] cross-gate table, of which the assembly read 1-10 % of the rows, is never
// built, and backward visits only the table rows some only-2D row refers to.  The values are
// the op chain's to the bit: lin_rows_dot is the tables' arithmetic, the sums below keep the
// chain's order, and what is skipped are terms 0 * x and all-zero partials.  c2 = 64.
struct GmaStageArgs {
  GmaArgs A;                             // (A.cross / A.gate: unused, no table exists)
  const float *w_c, *b_c, *w_g, *b_g;    // nn.Linear's [c2, c3] / [c2] (or NULL)
  const float* dummy;                    // [c3]
};
constexpr int kStageRows = 128;          // rows per workgroup = the tables' block size
static_assert(kStageRows == kLinBwdRows, "the partial slots follow rows_linear's blocks");
constexpr int kStageC2 = 64;

__device__ __forceinline__ void stage_fill_wt(float* __restrict__ wt, const float* __restrict__ w,
                                              int cin) {
  // W [c2][cin] in 16-byte pieces, all of a thread's loads in flight at once (cin <= 256)
  const int pieces = cin * kStageC2 / 4;
  f32x4 v[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int e = threadIdx.x + 256 * u;
    if (e < pieces) v[u] = ((const f32x4*)w)[e];
  }
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int e = threadIdx.x + 256 * u;
    if (e < pieces) {
      const int co = 4 * e / cin, k = 4 * e - co * cin;
#pragma unroll
      for (int j = 0; j < 4; ++j) wt[(k + j) * kStageC2 + co] = v[u][j];
    }
  }
}

// blocks [0, nb_o2): 128 only-2D (+ pad) rows each; [nb_o2, nb_o2 + nb_mix): mixed (+ pad)
// rows; the rest: the only-3D rows' [conv3 | 0], one thread per 16-byte piece.
constexpr int kStageCopy = 8;            // 16-byte pieces a copying thread keeps in flight
inline int stage_copy_blocks(long pieces) {
  const long b = (pieces + 256 * kStageCopy - 1) / (256 * kStageCopy);
  return (int)(b > 2048 ? 2048 : b);
}
template <int CPT>
__global__ __launch_bounds__(256) void gma_stage_fwd_kernel(GmaStageArgs S, float* __restrict__ out,
                                                            int nb_o2, int nb_mix) {
  const GmaArgs& A = S.A;
  constexpr int cin = 4 * CPT, c4 = CPT;
  const int c = cin + A.c2, tid = threadIdx.x;
  if ((int)blockIdx.x >= nb_o2 + nb_mix) {
    const int cq = c >> 2;
    const long total = (long)A.n_o3 * cq;
    const long nb = gridDim.x - nb_o2 - nb_mix;
    for (long e0 = (long)(blockIdx.x - nb_o2 - nb_mix) * 256 * kStageCopy + tid; e0 < total;
         e0 += nb * 256 * kStageCopy) {
      f32x4 v[kStageCopy];
#pragma unroll
      for (int u = 0; u < kStageCopy; ++u) {
        const long e = e0 + 256 * u, row = e / cq;
        const int q = (int)(e - row * cq);
        v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (e < total && q < c4) v[u] = ((const f32x4*)(A.conv3 + (size_t)row * cin))[q];
      }
#pragma unroll
      for (int u = 0; u < kStageCopy; ++u)
        if (e0 + 256 * u < total) ((f32x4*)out)[e0 + 256 * u] = v[u];
    }
    return;
  }
  extern __shared__ __attribute__((aligned(16))) float lin_smem[];
  constexpr int RT = 4, cg = kStageC2 >> 2, rg = 256 / cg, rpp = rg * RT;   // as rows_linear_fwd
  constexpr int xs_ld = cin + 4;
  float* wt = lin_smem;                        // [cin][c2]
  float* xs = wt + cin * kStageC2;             // [rpp][xs_ld]
  int* xrow = (int*)(xs + rpp * xs_ld);        // [128] feat3 row, -1 = the dummy, -2 = none
  int* frow = xrow + kStageRows;               // [128] feat2 row
  const bool mix = (int)blockIdx.x >= nb_o2;
  const long row0 = (long)(mix ? blockIdx.x - nb_o2 : blockIdx.x) * kStageRows;
  const long n = mix ? A.n_mix : A.n_o2, total = n + (mix ? A.n_mix_pad : A.n_o2_pad);
  const long base = mix ? (long)A.n_o3 + A.n_o2 + A.n_o2_pad : (long)A.n_o3;
  const float* b = mix ? S.b_g : S.b_c;
  stage_fill_wt(wt, mix ? S.w_g : S.w_c, cin);
  if (tid < kStageRows) {
    const long i = row0 + tid;
    int xr = -2, fr = 0;
    if (i < n) {
      if (mix) {
        xr = (int)A.rows_m3[i];
        fr = (int)A.rows_m2[i];
      } else {
        const long t = A.nn3[i];
        xr = t >= 0 ? (int)t : -1;
        fr = (int)A.rows_o2[i];
      }
    }
    xrow[tid] = xr;
    frow[tid] = fr;
  }
  const int g = tid % cg, r = tid / cg;
  f32x4 bias = {0.f, 0.f, 0.f, 0.f};
  if (b) bias = *(const f32x4*)(b + 4 * g);
  __syncthreads();
  // a pass's x tile = rpp * c4 16-byte pieces, kPre per thread; the next
  // pass's pieces and this pass's feat2 rows are loaded while this one is multiplied
  constexpr int kPre = rpp * c4 / 256;
  f32x4 pre[kPre];
  auto fetch = [&](int p0) {
#pragma unroll
    for (int u = 0; u < kPre; ++u) {
      const int e = tid + 256 * u;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (e < rpp * c4) {
        const int rr = e / c4, k4 = e - rr * c4;
        const int xr = xrow[p0 + rr];
        if (xr >= 0) v = *(const f32x4*)(A.feat3 + (size_t)xr * cin + 4 * k4);
        else if (xr == -1) v = *(const f32x4*)(S.dummy + 4 * k4);
      }
      pre[u] = v;
    }
  };
  fetch(0);
  for (int p0 = 0; p0 < kStageRows; p0 += rpp) {
    if (row0 + p0 >= total) break;
    if (p0) __syncthreads();     // the previous pass's xs consumed
#pragma unroll
    for (int u = 0; u < kPre; ++u) {
      const int e = tid + 256 * u;
      if (e < rpp * c4) {
        const int rr = e / c4, k4 = e - rr * c4;
        *(f32x4*)(xs + rr * xs_ld + 4 * k4) = pre[u];
        const long i = row0 + p0 + rr;
        if (i < total)      // the left block: feat3's row (mixed), zeros (only-2D, pad rows)
          *(f32x4*)(out + (size_t)(base + i) * c + 4 * k4) =
              mix ? pre[u] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    __syncthreads();
    if (p0 + rpp < kStageRows) fetch(p0 + rpp);
    f32x4 f2[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int rr = p0 + r + rg * t;
      f2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (row0 + rr < n) f2[t] = ((const f32x4*)(A.feat2 + (size_t)frow[rr] * kStageC2))[g];
    }
    f32x4 acc[RT];
    lin_rows_dot<RT, f32x4>(wt + 4 * g, kStageC2, A.c3, xs + r * xs_ld, rg * xs_ld, bias, acc);
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const long i = row0 + p0 + r + rg * t;
      if (i >= total) continue;
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if (i < n) {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = acc[t][j] > 0.f ? acc[t][j] : 0.f;
        a = a * f2[t];
      }
      *(f32x4*)(out + (size_t)(base + i) * c + cin + 4 * g) = a;
    }
  }
}

// One 128-row block of a gate's dW / db partial: its rows with a gradient (the cross table:
// the targets some only-2D row refers to, ascending; the gate: all of them) in tiles of
// kLinBwdTile -- x rows and the incoming gradient into LDS, the gradient masked by the
// recomputed gate, then rows_linear_bwd_partial_kernel's accumulation (thread = output
// channel co x CPT input channels, rows in order).  false: no row of the block had one.
template <int CPT>
__device__ __forceinline__ bool stage_bwd_block(const GmaStageArgs& S, const float* __restrict__ dout,
                                                const int64_t* __restrict__ order,
                                                const int64_t* __restrict__ starts, bool mix,
                                                int blk, float* __restrict__ slot) {
  extern __shared__ __attribute__((aligned(16))) float lin_smem[];
  const GmaArgs& A = S.A;
  constexpr int cin = 4 * CPT, c4 = CPT, xs_ld = cin + 4;
  const int c = cin + kStageC2, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* wt = lin_smem;                                  // [cin][c2]
  float* xs = wt + cin * kStageC2;                       // [tile][xs_ld]
  float* gs = xs + kLinBwdTile * xs_ld;                  // [tile][c2]
  long* sst = (long*)(gs + kLinBwdTile * kStageC2);      // [129] the block's starts
  int* items = (int*)(sst + kStageRows + 2);             // [128] rows of the block, compacted
  int* cnt = items + kStageRows;                         // [2]
  const int co = tid % kStageC2, grp = tid / kStageC2;
  const long row0 = (long)blk * kStageRows;
  const float* b = mix ? S.b_g : S.b_c;
  const float bias = b ? b[co] : 0.f;
  int count;
  if (mix) {
    count = (int)(A.n_mix - row0 < kStageRows ? A.n_mix - row0 : kStageRows);
  } else {
    if (tid <= kStageRows) {
      const long t = row0 + tid;
      sst[tid] = starts[t < A.n3 ? t : A.n3];    // (the dummy row n3 is the reduction's)
    }
    __syncthreads();
    bool ref = false;
    int pre = 0;
    if (tid < kStageRows) {
      ref = sst[tid + 1] > sst[tid];
      const unsigned long long m = __ballot(ref);
      if (lane == 0) cnt[wave] = __popcll(m);
      pre = __popcll(m & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (ref) items[(wave ? cnt[0] : 0) + pre] = tid;
    count = cnt[0] + cnt[1];
    if (count == 0) return false;
  }
  stage_fill_wt(wt, mix ? S.w_g : S.w_c, cin);
  const long base = (long)A.n_o3 + A.n_o2 + A.n_o2_pad;
  float acc[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) acc[j] = 0.f;
  float accb = 0.f;
  for (int p0 = 0; p0 < count; p0 += kLinBwdTile) {
    const int nt = count - p0 < kLinBwdTile ? count - p0 : kLinBwdTile;
    __syncthreads();     // items / wt written; the previous tile consumed
    {   // (all of a thread's loads in flight at once)
      constexpr int kPreX = kLinBwdTile * c4 / 256 > 0 ? kLinBwdTile * c4 / 256 : 1;
      f32x4 px[kPreX];
#pragma unroll
      for (int u = 0; u < kPreX; ++u) {
        const int e = tid + 256 * u, rr = e / c4, k4 = e - rr * c4;
        px[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (rr < nt) {
          const long src = mix ? (long)A.rows_m3[row0 + p0 + rr] : row0 + items[p0 + rr];
          px[u] = *(const f32x4*)(A.feat3 + (size_t)src * cin + 4 * k4);
        }
      }
#pragma unroll
      for (int u = 0; u < kPreX; ++u) {
        const int e = tid + 256 * u, rr = e / c4, k4 = e - rr * c4;
        if (rr < kLinBwdTile) *(f32x4*)(xs + rr * xs_ld + 4 * k4) = px[u];
      }
    }
    if (mix) {
      constexpr int kPreG = kLinBwdTile * (kStageC2 >> 2) / 256;
      f32x4 pa[kPreG], pb[kPreG];
#pragma unroll
      for (int u = 0; u < kPreG; ++u) {
        const int e = tid + 256 * u, rr = e >> 4, q = e & 15;
        pa[u] = pb[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (rr < nt) {
          const long i = row0 + p0 + rr;
          pa[u] = ((const f32x4*)(dout + (size_t)(base + i) * c + cin))[q];
          pb[u] = ((const f32x4*)(A.feat2 + (size_t)A.rows_m2[i] * kStageC2))[q];
        }
      }
#pragma unroll
      for (int u = 0; u < kPreG; ++u) ((f32x4*)gs)[tid + 256 * u] = pa[u] * pb[u];
    } else {
      for (int rr = wave; rr < kLinBwdTile; rr += 4) {     // a wave per target, as the chain
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (rr < nt) {
          const int lt = items[p0 + rr];
          v = cross_segment_sum(A, dout, order, sst[lt], sst[lt + 1]);
        }
        if (lane < 16) ((f32x4*)gs)[rr * 16 + lane] = v;
      }
    }
    __syncthreads();
    {   // the ReLU mask: the gate of each tile row, recomputed
      constexpr int RM = kLinBwdTile / 4;
      float y[RM];
      // (A.c3, not the constant: the k loop stays a loop -- unrolled whole it spills)
      lin_rows_dot<RM, float>(wt + co, kStageC2, A.c3, xs + grp * xs_ld, 4 * xs_ld, bias, y);
#pragma unroll
      for (int t = 0; t < RM; ++t)
        if (!(y[t] > 0.f)) gs[(grp + 4 * t) * kStageC2 + co] = 0.f;
    }
    __syncthreads();
    for (int rr = 0; rr < nt; ++rr) {
      const float gv = gs[rr * kStageC2 + co];
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
#pragma unroll
  for (int j = 0; j < CPT; ++j) slot[(size_t)co * cin + grp * CPT + j] = acc[j];
  if (grp == 0) slot[(size_t)kStageC2 * cin + co] = accb;
  return true;
}

// blocks [0, kDummyBlocks): slices of the dummy row's segment; then nb_c: the cross table's
// 128-row blocks (a flag each: did it write its slot); then nb_g blocks of mixed rows; the
// rest: d conv3 = the left block of the only-3D rows.
template <int CPT>
__global__ __launch_bounds__(256) void gma_stage_bwd_kernel(
    GmaStageArgs S, const float* __restrict__ dout, const int64_t* __restrict__ order,
    const int64_t* __restrict__ starts, float* __restrict__ d_conv3, float* __restrict__ part_c,
    int* __restrict__ flags, float* __restrict__ dummy_part, float* __restrict__ dummy_gate,
    float* __restrict__ part_g, int nb_c, int nb_g) {
  const GmaArgs& A = S.A;
  constexpr int entries = kStageC2 * 4 * CPT + kStageC2;
  int blk = blockIdx.x;
  if (blk < kDummyBlocks) {      // (first: the longest chains of the launch)
    cross_dummy_slice(A, dout, order, starts, dummy_part, blk);
    if (blk == 0 && threadIdx.x < kStageC2) {   // the dummy embedding's gate, for its mask
      const int co = threadIdx.x;
      float y[1];
      lin_rows_dot<1, float>(S.w_c + (size_t)co * 4 * CPT, 1, 4 * CPT, S.dummy, 0,
                             S.b_c ? S.b_c[co] : 0.f, y);
      dummy_gate[co] = y[0];
    }
    return;
  }
  blk -= kDummyBlocks;
  if (blk < nb_c) {
    const bool wrote = stage_bwd_block<CPT>(S, dout, order, starts, false, blk,
                                            part_c + (size_t)blk * entries);
    if (threadIdx.x == 0) flags[blk] = wrote ? 1 : 0;
    return;
  }
  blk -= nb_c;
  if (blk < nb_g) {
    stage_bwd_block<CPT>(S, dout, order, starts, true, blk, part_g + (size_t)blk * entries);
    return;
  }
  blk -= nb_g;
  const int c4 = (A.c3 + A.c2) >> 2, k3 = A.c3 >> 2;
  const long total = (long)A.n_o3 * k3;
  const long nb = (long)gridDim.x - nb_c - kDummyBlocks - nb_g;
  for (long e0 = (long)blk * 256 * kStageCopy + threadIdx.x; e0 < total;
       e0 += nb * 256 * kStageCopy) {
    f32x4 v[kStageCopy];
#pragma unroll
    for (int u = 0; u < kStageCopy; ++u) {
      const long e = e0 + 256 * u, row = e / k3;
      if (e < total) v[u] = ((const f32x4*)dout)[row * c4 + (e - row * k3)];
    }
#pragma unroll
    for (int u = 0; u < kStageCopy; ++u)
      if (e0 + 256 * u < total) ((f32x4*)d_conv3)[e0 + 256 * u] = v[u];
  }
}

// Both gates' dW / db from the block slots, rows_linear_bwd_reduce_kernel's order (block bk
// in slice bk % 4, ascending; the slices added in order).  An unflagged cross block counts
// as the zeros the chain's partial held.  The dummy row -- the LAST row of the cross
// table's last block -- is added to that block's slot here, where the chain's partial
// kernel added it: its gradient = the kDummyBlocks slices in block order, masked by the
// dummy embedding's gate (computed by the partial launch).  Workgroups [0, rb): the cross linear; [rb, 2 rb): the gate.
__global__ __launch_bounds__(256) void gma_stage_reduce_kernel(
    GmaStageArgs S, const float* __restrict__ part_c, const int* __restrict__ flags, int nb_c,
    const float* __restrict__ dummy_part, const float* __restrict__ dummy_gate,
    const float* __restrict__ part_g, int nb_g, int rb,
    float* __restrict__ dw_c, float* __restrict__ db_c, float* __restrict__ dw_g,
    float* __restrict__ db_g) {
  __shared__ float sm[4][64];
  const int cin = S.A.c3, per_w = kStageC2 * cin, entries = per_w + kStageC2;
  const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const bool gate = (int)blockIdx.x >= rb;
  const int e = ((int)blockIdx.x - (gate ? rb : 0)) * 64 + lane;
  const float* part = gate ? part_g : part_c;
  const int nblk = gate ? nb_g : nb_c, last = nb_c - 1;
  float s = 0.f;
  {
    const int e_own = e;
    const int e = e_own < entries ? e_own : entries - 1;   // (every lane takes part in the ballots)
    const bool has_d = !gate && slice == (last & 3);
    float dterm = 0.f;
    if (has_d) {
      const int co = e < per_w ? e / cin : e - per_w;
      float dv[kDummyBlocks];
#pragma unroll
      for (int k = 0; k < kDummyBlocks; ++k) dv[k] = dummy_part[k * kStageC2 + co];
      float d = dv[0];
#pragma unroll
      for (int k = 1; k < kDummyBlocks; ++k) d += dv[k];
      const float gv = dummy_gate[co] > 0.f ? d : 0.f;
      dterm = e < per_w ? gv * S.dummy[e - co * cin] : gv;
    }
    // this slice's blocks bk = slice, slice + 4, ..: 64 candidates at a time, one lane reads
    // one flag, the set bits (wave-uniform, ascending) are walked eight loads at a time; a
    // missing one of the eight re-reads the first and adds an exact 0.  The dummy row's
    // block -- the last of its slice -- is added behind the loop with the dummy term.
    for (int b0 = slice; b0 < nblk; b0 += 256) {
      const int cand = b0 + 4 * lane;
      bool f = cand < nblk && !(has_d && cand == last);
      if (f && !gate) f = flags[cand] != 0;
      unsigned long long m = __ballot(f);
      while (m) {
        int idx[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          idx[u] = m ? __builtin_ctzll(m) : -1;
          m &= m - 1;       // (0 stays 0)
        }
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          v[u] = part[(size_t)(b0 + 4 * (idx[u] >= 0 ? idx[u] : idx[0])) * entries + e];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += idx[u] >= 0 ? v[u] : 0.f;
      }
    }
    if (has_d) s += (flags[last] ? part[(size_t)last * entries + e] : 0.f) + dterm;
  }
  sm[slice][lane] = s;
  __syncthreads();
  if (slice || e >= entries) return;
  s = ((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane];
  float* dw = gate ? dw_g : dw_c;
  float* db = gate ? db_g : db_c;
  if (e < per_w) dw[e] = s;
  else if (db) db[e - per_w] = s;
}

inline size_t stage_fwd_smem(int c3) {
  return sizeof(float) * ((size_t)c3 * kStageC2 + 64 * (size_t)(c3 + 4)) +
         sizeof(int) * 2 * kStageRows;
}
inline size_t stage_bwd_smem(int c3) {
  return sizeof(float) * ((size_t)c3 * kStageC2 + (size_t)kLinBwdTile * (c3 + 4) +
                          (size_t)kLinBwdTile * kStageC2) +
         sizeof(long) * (kStageRows + 2) + sizeof(int) * (kStageRows + 2);
}
struct StageWs {
  float *part_c, *part_g, *dummy_part, *dummy_gate;
  int* flags;
  int nb_c, nb_g;
};
template <typename Arena>
StageWs stage_ws(Arena& ar, int n3, int n_mix, int c3) {
  StageWs w;
  const size_t entries = (size_t)kStageC2 * c3 + kStageC2;
  w.nb_c = ceil_div((long)n3 + 1, kStageRows);
  w.nb_g = ceil_div(n_mix, kStageRows);
  w.part_c = ar.template take<float>(w.nb_c * entries);
  w.part_g = ar.template take<float>((w.nb_g ? w.nb_g : 1) * entries);
  w.dummy_part = ar.template take<float>((size_t)kDummyBlocks * kStageC2);
  w.dummy_gate = ar.template take<float>(kStageC2);
  w.flags = ar.template take<int>(w.nb_c);
  return w;
}
bool stage_args(GmaStageArgs& S, const float* conv3, int n_o3, int c3, const float* feat3, int n3,
                int c2, const float* dummy, const float* w_c, const float* b_c, const float* w_g,
                const float* b_g, const int64_t* nn3, const float* feat2, const int64_t* rows_o2,
                int n_o2, int n_o2_pad, const int64_t* rows_m3, const int64_t* rows_m2, int n_mix,
                int n_mix_pad) {
  if (n_o3 < 0 || n_o2 < 0 || n_mix < 0 || n_o2_pad < 0 || n_mix_pad < 0 || n3 < 0) return false;
  if ((n_o3 && !conv3) || !dummy || !w_c || !w_g || (n3 && !feat3) ||
      (n_o2 && (!feat2 || !rows_o2)) || (n_mix && (!feat3 || !rows_m3 || !rows_m2 || !feat2)))
    return false;
  S.A = GmaArgs{conv3, nullptr, feat2, feat3, nullptr, nn3, rows_o2, rows_m3, rows_m2,
                n_o3,  n_o2,    n_o2_pad, n_mix, n_mix_pad, n3, c3, c2};
  S.w_c = w_c, S.b_c = b_c, S.w_g = w_g, S.b_g = b_g, S.dummy = dummy;
  return true;
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

// ---- the fused stage: gates + assembly, one launch forward, two backward ----
MSMD_EXPORT int msmd_gma_stage_supported(int c3, int c2) {
  // the gates' thread layouts at c2 = 64: 4 input-channel groups of c3 / 4 channels each
  return c2 == kStageC2 && (c3 == 16 || c3 == 32 || c3 == 64 || c3 == 128 || c3 == 256) &&
         msmd_rows_linear_supported(c3, c2);
}

template <int CPT>
static int stage_fwd_launch(const GmaStageArgs& S, float* out, int nb_o2, int nb_mix, int nb_o3,
                            hipStream_t st) {
  const size_t smem = stage_fwd_smem(4 * CPT);
  static LdsGrant granted;
  const int rc = optin_dynamic_lds((const void*)gma_stage_fwd_kernel<CPT>, smem, granted);
  if (rc != MSMD_OK) return rc;
  MSMD_LAUNCH(gma_stage_fwd_kernel<CPT>, dim3(nb_o2 + nb_mix + nb_o3), dim3(256), smem, st, S, out,
              nb_o2, nb_mix);
  return launch_status();
}

MSMD_EXPORT int msmd_gma_stage_fwd_f32(const float* conv3, int n_o3, int c3, const float* feat3,
                                       int n3, int c2, const float* dummy, const float* w_cross,
                                       const float* b_cross, const float* w_gate,
                                       const float* b_gate, const int64_t* nn3, const float* feat2,
                                       const int64_t* rows_o2, int n_o2, int n_o2_pad,
                                       const int64_t* rows_m3, const int64_t* rows_m2, int n_mix,
                                       int n_mix_pad, float* out, msmd_stream_t stream) {
  if (!msmd_gma_stage_supported(c3, c2)) return MSMD_ERR_UNSUPPORTED;
  GmaStageArgs S;
  if (!stage_args(S, conv3, n_o3, c3, feat3, n3, c2, dummy, w_cross, b_cross, w_gate, b_gate, nn3,
                  feat2, rows_o2, n_o2, n_o2_pad, rows_m3, rows_m2, n_mix, n_mix_pad) ||
      (n_o2 && !nn3))
    return MSMD_ERR_INVALID_ARG;
  const long rows = (long)n_o3 + n_o2 + n_o2_pad + n_mix + n_mix_pad;
  if (rows == 0) return MSMD_OK;
  if (!out) return MSMD_ERR_INVALID_ARG;
  const int nb_o2 = ceil_div((long)n_o2 + n_o2_pad, kStageRows);
  const int nb_mix = ceil_div((long)n_mix + n_mix_pad, kStageRows);
  const int nb_o3 = stage_copy_blocks((long)n_o3 * ((c3 + c2) >> 2));
  hipStream_t st = (hipStream_t)stream;
  switch (c3 / 4) {
    case 4: return stage_fwd_launch<4>(S, out, nb_o2, nb_mix, nb_o3, st);
    case 8: return stage_fwd_launch<8>(S, out, nb_o2, nb_mix, nb_o3, st);
    case 16: return stage_fwd_launch<16>(S, out, nb_o2, nb_mix, nb_o3, st);
    case 32: return stage_fwd_launch<32>(S, out, nb_o2, nb_mix, nb_o3, st);
    case 64: return stage_fwd_launch<64>(S, out, nb_o2, nb_mix, nb_o3, st);
    default: return MSMD_ERR_UNSUPPORTED;
  }
}

MSMD_EXPORT size_t msmd_gma_stage_bwd_workspace_bytes(int n3, int n_mix, int c3, int c2) {
  (void)c2;
  ArenaSize ar;
  stage_ws(ar, n3 > 0 ? n3 : 0, n_mix > 0 ? n_mix : 0, c3 > 0 ? c3 : 0);
  return ar.off;
}

template <int CPT>
static int stage_bwd_launch(const GmaStageArgs& S, const float* d_out, const int64_t* order,
                            const int64_t* starts, float* d_conv3, const StageWs& w, int nb_o3,
                            hipStream_t st) {
  const size_t smem = stage_bwd_smem(4 * CPT);
  static LdsGrant granted;
  const int rc = optin_dynamic_lds((const void*)gma_stage_bwd_kernel<CPT>, smem, granted);
  if (rc != MSMD_OK) return rc;
  MSMD_LAUNCH(gma_stage_bwd_kernel<CPT>, dim3(w.nb_c + kDummyBlocks + w.nb_g + nb_o3), dim3(256),
              smem, st, S, d_out, order, starts, d_conv3, w.part_c, w.flags, w.dummy_part,
              w.dummy_gate, w.part_g, w.nb_c, w.nb_g);
  return MSMD_OK;
}

MSMD_EXPORT int msmd_gma_stage_bwd_f32(const float* d_out, int n_o3, int c3, const float* feat3,
                                       int n3, int c2, const float* dummy, const float* w_cross,
                                       const float* b_cross, const float* w_gate,
                                       const float* b_gate, const float* feat2,
                                       const int64_t* rows_o2, int n_o2, int n_o2_pad,
                                       const int64_t* rows_m3, const int64_t* rows_m2, int n_mix,
                                       int n_mix_pad, const int64_t* order, const int64_t* starts,
                                       float* d_conv3, float* dw_cross, float* db_cross,
                                       float* dw_gate, float* db_gate, void* workspace,
                                       size_t workspace_bytes, msmd_stream_t stream) {
  if (!msmd_gma_stage_supported(c3, c2)) return MSMD_ERR_UNSUPPORTED;
  GmaStageArgs S;
  if (!stage_args(S, d_conv3, n_o3, c3, feat3, n3, c2, dummy, w_cross, b_cross, w_gate, b_gate,
                  nullptr, feat2, rows_o2, n_o2, n_o2_pad, rows_m3, rows_m2, n_mix, n_mix_pad) ||
      !starts || (n_o2 && !order) || !dw_cross || !dw_gate)
    return MSMD_ERR_INVALID_ARG;
  const long rows = (long)n_o3 + n_o2 + n_o2_pad + n_mix + n_mix_pad;
  if (rows && !d_out) return MSMD_ERR_INVALID_ARG;
  Arena ar{(char*)workspace, workspace_bytes};
  const StageWs w = stage_ws(ar, n3, n_mix, c3);
  if (!workspace || !ar.ok()) return MSMD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nb_o3 = stage_copy_blocks((long)n_o3 * (c3 >> 2));
  int rc;
  switch (c3 / 4) {
    case 4: rc = stage_bwd_launch<4>(S, d_out, order, starts, d_conv3, w, nb_o3, st); break;
    case 8: rc = stage_bwd_launch<8>(S, d_out, order, starts, d_conv3, w, nb_o3, st); break;
    case 16: rc = stage_bwd_launch<16>(S, d_out, order, starts, d_conv3, w, nb_o3, st); break;
    case 32: rc = stage_bwd_launch<32>(S, d_out, order, starts, d_conv3, w, nb_o3, st); break;
    case 64: rc = stage_bwd_launch<64>(S, d_out, order, starts, d_conv3, w, nb_o3, st); break;
    default: return MSMD_ERR_UNSUPPORTED;
  }
  if (rc != MSMD_OK) return rc;
  const int rb = ceil_div((long)kStageC2 * c3 + kStageC2, 64);
  MSMD_LAUNCH(gma_stage_reduce_kernel, dim3(2 * rb), dim3(256), 0, st, S, (const float*)w.part_c,
              (const int*)w.flags, w.nb_c, (const float*)w.dummy_part,
              (const float*)w.dummy_gate, (const float*)w.part_g, w.nb_g, rb, dw_cross, db_cross, dw_gate, db_gate);
  return launch_status();
}
