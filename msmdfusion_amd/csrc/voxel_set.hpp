// voxel_set.hpp -- a voxel set as an occupancy bitmap of its grid: what the strided and
// transposed rulebooks (rulebook.hip), the union set of sparse_add and the modality split
// (dense.hip) are built from.  Mark the cells (1 bit each), scan the popcounts of the words
// (scan.hpp): the rank of a set bit is the cell's row in ascending linear id.  One workspace
// layout for all of them, so a region sized and carved by one entry point is read by another
// (the fusion chain counts a union set in rulebook.hip and fills it through
// msmd_sparse_add_fill) without either knowing more than this header.
#pragma once
#include "common.hpp"
#include "scan.hpp"

namespace msmd {

struct Shape3 {
  int s[3];   // (z, y, x) extents of the grid
};

// linear cell id of (b, z, y, x) in a grid of extents s
__device__ __forceinline__ uint32_t cell_id(int b, int z, int y, int x, const int* s) {
  return (((uint32_t)b * s[0] + z) * s[1] + y) * s[2] + x;
}

// A grid whose cell ids fit 32 bits (0xffffffff stays free); dst <- its extents.
inline int check_grid(int batch, const int* shape, int* dst) {
  if (batch < 1 || !shape) return MSMD_ERR_INVALID_ARG;
  double cells = batch;
  for (int i = 0; i < 3; ++i) {
    if (shape[i] < 1) return MSMD_ERR_INVALID_ARG;
    dst[i] = shape[i];
    cells *= shape[i];
  }
  return cells >= 4294967295.0 ? MSMD_ERR_RANGE : MSMD_OK;
}

struct SetWs {
  uint32_t *bits, *bits2;   // bits2: the second set of the modality split, else null
  int *prefix, *tiles;
  size_t words;
};
// two = false is the layout every *_workspace_bytes query of a single set reports
template <typename A>
void carve_set(A& a, SetWs* w, int batch, const int* shape, bool two = false) {
  size_t cells = (size_t)batch * shape[0] * shape[1] * shape[2];
  size_t words = (cells + 31) / 32;
  uint32_t* b0 = a.template take<uint32_t>(words);
  uint32_t* b1 = two ? a.template take<uint32_t>(words) : nullptr;
  int* pf = a.template take<int>(words);
  int* tl = a.template take<int>(scan_num_tiles((long)words) + 1);
  if (w) *w = SetWs{b0, b1, pf, tl, words};
}
inline size_t set_workspace_bytes(int batch, const int* shape, bool two = false) {
  ArenaSize a;
  carve_set(a, (SetWs*)nullptr, batch, shape, two);
  return a.off;
}
// false: the region is too small or not 256-byte aligned
inline bool carve_set_at(void* region, size_t bytes, SetWs* w, int batch, const int* shape,
                         bool two = false) {
  Arena a(region, bytes);
  carve_set(a, w, batch, shape, two);
  return a.ok();
}

static __global__ __launch_bounds__(256) void set_mark_rows(const int32_t* __restrict__ idx, int n,
                                                            Shape3 sh, uint32_t* bits) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int4 r = ((const int4*)idx)[i];
  bitmap_set(bits, cell_id(r.x, r.y, r.z, r.w, sh.s));
}
inline void mark_rows(const int32_t* idx, int n, const Shape3& sh, uint32_t* bits,
                      hipStream_t st) {
  if (n > 0) MSMD_LAUNCH(set_mark_rows, dim3(ceil_div(n, 256)), dim3(256), 0, st, idx, n, sh, bits);
}

// w.prefix <- set cells in front of each word of w.bits, *count (device) <- cells of the set
inline void scan_set(const SetWs& w, int32_t* count, hipStream_t st) {
  device_scan(PopcCount{w.bits}, StorePrefix{w.prefix}, (int)w.words, w.tiles, count, -1, st);
}

}  // namespace msmd
