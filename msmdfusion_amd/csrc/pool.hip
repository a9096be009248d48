// pool.hip -- sparse max-pool forward / backward (fp32) for gfx950.
//
// Replaces SparseMaxPoolForwardFunctor / SparseMaxPoolBackwardFunctor (mmdet3d/ops/spconv/src/
// maxpool.cc:20-62, driven per offset by pool_ops.h:34,71) over the pool's rulebook, which is
// the strided conv rulebook of the same geometry (rulebook.hip).  The contract, element by
// element:
//   forward   out[o] = 0; for every pair (k, i, o): if (out[o] < in[i]) out[o] = in[i]
//   backward  din[i] = 0; for k ascending, every pair (k, i, o): if (out[o] == in[i])
//             din[i] += dout[o]
// so an all-negative window gives 0 and a NaN input never wins.
//
// Both passes are INPUT-STATIONARY over nbr_bwd[K, n_in] (input row -> output row per offset):
// that table is complete -- every input row, repeated coordinates included, has its pair --
// while nbr_fwd keeps one input row per (offset, output cell).
//   forward: the result is max(+0, the non-NaN inputs), >= +0.  Only inputs > 0 can move an
//     output, and on non-negative floats the order of the bit patterns (as integers) is the
//     order of the values: one integer atomicMax per (input element, offset) into an output
//     zeroed up front gives exactly the loop's value, whatever the order of the atomics.
//   backward: each (i, c) thread walks k in ascending order and writes its element once --
//     the functor's summation order, no float atomics: bitwise equal to the loop.
#include "common.hpp"

namespace msmd {
namespace {

inline int grid_of(long work) {
  long b = (work + 255) / 256;
  if (b > 8192) b = 8192;
  return (int)(b > 0 ? b : 1);
}

__global__ __launch_bounds__(256) void maxpool_fwd(const float* __restrict__ in, int n, int c,
                                                   const int32_t* __restrict__ nbr_bwd, int kvol,
                                                   int n_out, uint32_t* __restrict__ out_bits) {
  const long total = (long)n * c;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const float v = in[t];
    if (!(v > 0.f)) continue;  // <= 0 and NaN never replace the zero start
    const int i = (int)(t / c), ch = (int)(t - (long)i * c);
    const uint32_t bits = __float_as_uint(v);
    for (int k = 0; k < kvol; ++k) {
      const int o = nbr_bwd[(size_t)k * n + i];
      if ((unsigned)o < (unsigned)n_out) atomicMax(&out_bits[(size_t)o * c + ch], bits);
    }
  }
}

__global__ __launch_bounds__(256) void maxpool_bwd(const float* __restrict__ in,
                                                   const float* __restrict__ out,
                                                   const float* __restrict__ dout, int n, int c,
                                                   const int32_t* __restrict__ nbr_bwd, int kvol,
                                                   int n_out, float* __restrict__ din) {
  const long total = (long)n * c;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int i = (int)(t / c), ch = (int)(t - (long)i * c);
    const float v = in[t];
    float acc = 0.f;
    for (int k = 0; k < kvol; ++k) {
      const int o = nbr_bwd[(size_t)k * n + i];
      if ((unsigned)o < (unsigned)n_out) {
        const size_t e = (size_t)o * c + ch;
        if (out[e] == v) acc += dout[e];
      }
    }
    din[t] = acc;
  }
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT int msmd_sparse_maxpool_fwd_f32(const float* in, int n_in, int num_channels,
                                            const int32_t* nbr_bwd, int kvol, int n_out,
                                            float* out, msmd_stream_t stream) {
  if (n_in < 0 || n_out < 0 || num_channels < 1 || kvol < 1) return MSMD_ERR_INVALID_ARG;
  if ((n_out > 0 && !out) || (n_in > 0 && n_out > 0 && (!in || !nbr_bwd)))
    return MSMD_ERR_INVALID_ARG;
  if (n_out == 0) return MSMD_OK;
  hipStream_t st = (hipStream_t)stream;
  hipMemsetAsync(out, 0, sizeof(float) * (size_t)n_out * num_channels, st);
  if (n_in > 0)
    MSMD_LAUNCH(maxpool_fwd, dim3(grid_of((long)n_in * num_channels)), dim3(256), 0, st, in, n_in,
                num_channels, nbr_bwd, kvol, n_out, (uint32_t*)out);
  return launch_status();
}

MSMD_EXPORT int msmd_sparse_maxpool_bwd_f32(const float* in, const float* out, const float* dout,
                                            int n_in, int num_channels, const int32_t* nbr_bwd,
                                            int kvol, int n_out, float* din,
                                            msmd_stream_t stream) {
  if (n_in < 0 || n_out < 0 || num_channels < 1 || kvol < 1) return MSMD_ERR_INVALID_ARG;
  if (n_in == 0) return MSMD_OK;
  if (!in || !din || !nbr_bwd || (n_out > 0 && (!out || !dout))) return MSMD_ERR_INVALID_ARG;
  MSMD_LAUNCH(maxpool_bwd, dim3(grid_of((long)n_in * num_channels)), dim3(256), 0,
              (hipStream_t)stream, in, out, dout, n_in, num_channels, nbr_bwd, kvol, n_out, din);
  return launch_status();
}
