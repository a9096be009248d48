// scan.hpp -- device-wide exclusive prefix sum in two small kernels (tile sums -> apply),
// generic over where the per-element count comes from and what is done with the prefix.
// (Round 3: the single-block scan of the tile sums between the two is gone -- every apply
// block adds up the tile sums in front of it itself, a few KB from L2.  The index pass of
// an LC step runs 44 scans on a stream whose launches queue behind the feature pass's
// persistent kernels: a launch there costs far more than the few microseconds of its work.)
//   Count: int operator()(int i) const          -- value of element i
//   Emit : void operator()(int i, int prefix, int value) const
// Used for: popcount ranks of occupancy bitmaps (strided rulebook,
// sparse_add, modality split), first-point flags (voxelization) and per-offset
// pair compaction.  All HBM-bound streaming passes with coalesced access.
// segmented_scan() below runs the same two kernels over several independent sequences at
// once (the launch sets of voxelize.hip, rulebook.hip and dense.hip).
#pragma once
#include "common.hpp"

namespace msmd {

constexpr int kScanBlock = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kScanBlock * kScanItems;

inline int scan_num_tiles(long n) { return ceil_div(n, kScanTile); }
// Rows of a table padded to whole scan tiles (the pair compaction: each offset's rows are a
// run of whole tiles, so no tile straddles two offsets).
inline int rows_padded(int n_rows) { return scan_num_tiles(n_rows > 0 ? n_rows : 1) * kScanTile; }

// Sum of the tile's counts -> *out.  The tile covers elements [base, base + kScanTile) of
// a sequence of n.
template <typename Count>
__device__ __forceinline__ void tile_sum(const Count& count, int base, int n,
                                         int* __restrict__ out) {
  __shared__ int smem[kScanBlock / 64];
  int s = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    int i = base + j * kScanBlock + threadIdx.x;  // coalesced
    if (i < n) s += count(i);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int i = 0; i < kScanBlock / 64; ++i) t += smem[i];
    *out = t;
  }
}

template <typename Count>
__global__ __launch_bounds__(kScanBlock) void scan_tile_sums(Count count, int n,
                                                             int* __restrict__ tile_sums) {
  tile_sum(count, blockIdx.x * kScanTile, n, tile_sums + blockIdx.x);
}

// Sum of a[lo .. hi) by the whole block (same value in every thread).  smem: BLOCK/64 ints.
template <int BLOCK>
__device__ __forceinline__ int block_range_sum(const int* __restrict__ a, int lo, int hi,
                                               int* smem) {
  int s = 0;
  for (int i = lo + (int)threadIdx.x; i < hi; i += BLOCK) s += a[i];
  s = wave_sum(s);
  __syncthreads();   // smem may still be read from a previous use
  if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = s;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int i = 0; i < BLOCK / 64; ++i) t += smem[i];
  // ... and the next user of smem (block_excl_scan writes it without a barrier in front) must
  // not overtake a wave still reading here.  Without this barrier a block now and then took
  // a wrong carry: garbage positions in pair lists / row ranks, only under load (round 3:
  // memory faults in one bench leg out of ~6 -- found by bisecting, a bisection script of round 3, since pruned: git history)
  __syncthreads();
  return t;
}

// Exclusive prefixes of a tile: kScanItems values per thread, item-major (item j of every
// thread precedes item j + 1 of any thread, the order of the coalesced loads), across the
// block with ONE barrier pair for all items -- the values are loaded up front (kScanItems
// independent loads in flight instead of a load -> two barriers -> load chain per item: the
// index pass runs ~50 of these scans per LC step as short kernels whose time is that chain).
// smem: kScanItems * kScanBlock / 64 ints.  ex[j] <- prefix inside the tile; returns the total.
constexpr int kScanSmem = kScanItems * (kScanBlock / 64);
__device__ __forceinline__ int tile_excl_scan(const int (&v)[kScanItems], int (&ex)[kScanItems],
                                              int* smem) {
  constexpr int NW = kScanBlock / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    ex[j] = wave_excl_scan(v[j], lane);
    if (lane == 63) smem[j * NW + w] = ex[j] + v[j];
  }
  __syncthreads();
  int run = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int s = smem[j * NW + i];
      base += i < w ? s : 0;
      tot += s;
    }
    ex[j] += run + base;
    run += tot;
  }
  __syncthreads();      // smem may be written again
  return run;
}

// In place, by ONE block of 1024 threads: a[0..n) values -> a[0..n] exclusive prefix (a has
// n + 1 entries; the stream-K tile weights of a table).  part: 1024 ints of LDS.
__device__ __forceinline__ void block_prefix_in_place(int32_t* __restrict__ a, int n, int* part) {
  const int per = (n + 1023) / 1024, t = threadIdx.x;
  const int b = t * per, e = b + per < n ? b + per : n;
  int s = 0;
  for (int i = b; i < e; ++i) s += a[i];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;    // exclusive prefix of this thread's slice
  for (int i = b; i < e; ++i) {
    const int w = a[i];
    a[i] = run;
    run += w;
  }
  if (t == 1023) a[n] = part[1023];
}

// total <- 0 for an empty input
static __global__ void scan_empty_total(int* __restrict__ total) {
  if (total) *total = 0;
}

// The tile at [base, base + kScanTile) of a sequence of n: emit(i, exclusive prefix, value) for
// its elements, the prefix starting from the sum of tile_sums[lo .. hi), the tiles of the
// sequence in front of this one.  Returns the inclusive total at the tile's end.
template <typename Count, typename Emit>
__device__ __forceinline__ int tile_apply(const Count& count, const Emit& emit, int base, int n,
                                          const int* __restrict__ tile_sums, int lo, int hi) {
  __shared__ int smem[kScanSmem];
  int v[kScanItems], ex[kScanItems];
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    const int i = base + j * kScanBlock + threadIdx.x;
    v[j] = i < n ? count(i) : 0;
  }
  const int carry = block_range_sum<kScanBlock>(tile_sums, lo, hi, smem);
  const int tot = tile_excl_scan(v, ex, smem);
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    const int i = base + j * kScanBlock + threadIdx.x;
    if (i < n) emit(i, carry + ex[j], v[j]);
  }
  return carry + tot;
}

template <typename Count, typename Emit>
__global__ __launch_bounds__(kScanBlock) void scan_apply(Count count, Emit emit, int n,
                                                         const int* __restrict__ tile_sums,
                                                         int* __restrict__ total, int clamp) {
  const int sum = tile_apply(count, emit, blockIdx.x * kScanTile, n, tile_sums, 0, blockIdx.x);
  if (total && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
    *total = (clamp >= 0 && sum > clamp) ? clamp : sum;
}

// ---- several sequences in one launch ----------------------------------------
// The launch sets (msmd_hard_voxelize_many, msmd_rulebook_subm3d_many, msmd_rows_where_eq_many,
// msmd_rulebook_plan_many) pack the blocks of several jobs into one grid; `first` holds each
// job's first block (n + 1 entries, the unused tail at INT_MAX) and travels as a kernel
// argument.  -> the job that owns block b.  A table with room for one job needs no look-up:
// its blocks read the job's fields at fixed offsets, without waiting for `first`.
template <int M>
__device__ __forceinline__ int segment_of(const int (&first)[M], int n, int b) {
  if (M == 2) return 0;
  int s = 0;
  while (s + 1 < n && b >= first[s + 1]) ++s;     // uniform: scalar loads of kernel arguments
  return s;
}

// The scan above over several independent segments, each owning whole tiles (the scan restarts
// at every segment).  Tab, a launch table passed by value, supplies
//   int n;                                   -- number of segments
//   const int (&seg_tile0() const)[]         -- first tile of segment s (n + 1 entries)
//   int seg_len(int s) const                 -- its number of elements
//   Count seg_count(int s), Emit seg_emit(int s) const   -- the contracts at the top
//   void seg_done(int s, int total) const    -- run by every thread of the block that holds the
//                                               segment's last tile, with the segment's sum
template <typename Tab>
__global__ __launch_bounds__(kScanBlock) void seg_scan_tile_sums(const Tab tab,
                                                                 int* __restrict__ tile_sums) {
  const int s = segment_of(tab.seg_tile0(), tab.n, blockIdx.x);
  tile_sum(tab.seg_count(s), (blockIdx.x - tab.seg_tile0()[s]) * kScanTile, tab.seg_len(s),
           tile_sums + blockIdx.x);
}
template <typename Tab>
__global__ __launch_bounds__(kScanBlock) void seg_scan_apply(const Tab tab,
                                                             const int* __restrict__ tile_sums) {
  const int s = segment_of(tab.seg_tile0(), tab.n, blockIdx.x);
  const int t0 = tab.seg_tile0()[s];
  const int sum = tile_apply(tab.seg_count(s), tab.seg_emit(s), (blockIdx.x - t0) * kScanTile,
                             tab.seg_len(s), tile_sums, t0, (int)blockIdx.x);
  if ((int)blockIdx.x == tab.seg_tile0()[s + 1] - 1) tab.seg_done(s, sum);
}
template <typename Tab>
inline void segmented_scan(const Tab& tab, int n_tiles, int* tile_sums, hipStream_t st) {
  MSMD_LAUNCH(seg_scan_tile_sums<Tab>, dim3(n_tiles), dim3(kScanBlock), 0, st, tab, tile_sums);
  MSMD_LAUNCH(seg_scan_apply<Tab>, dim3(n_tiles), dim3(kScanBlock), 0, st, tab,
              (const int*)tile_sums);
}

// Host driver.  tile_sums: scratch of scan_num_tiles(n) ints (raw tile sums afterwards).
template <typename Count, typename Emit>
inline void device_scan(Count count, Emit emit, int n, int* tile_sums, int* total, int clamp,
                        hipStream_t st) {
  const int nt = scan_num_tiles(n);
  if (nt == 0) {
    MSMD_LAUNCH(scan_empty_total, dim3(1), dim3(1), 0, st, total);
    return;
  }
  MSMD_LAUNCH(scan_tile_sums<Count>, dim3(nt), dim3(kScanBlock), 0, st, count, n,
                     tile_sums);
  MSMD_LAUNCH((scan_apply<Count, Emit>), dim3(nt), dim3(kScanBlock), 0, st, count, emit, n,
                     (const int*)tile_sums, total, clamp);
}

// ---- occupancy bitmap + popcount rank ---------------------------------------
// A set of 32-bit cell ids in [0, cells) is a bitmap of ceil(cells/32) words;
// after device_scan(PopcCount, StorePrefix) the row of a present cell, in
// ascending cell order, is prefix[cell>>5] + popc(bits[cell>>5] & low mask).
struct PopcCount {
  const uint32_t* bits;
  __device__ int operator()(int i) const { return __popc(bits[i]); }
};
struct StorePrefix {
  int* prefix;
  __device__ void operator()(int i, int p, int) const { prefix[i] = p; }
};
__device__ __forceinline__ void bitmap_set(uint32_t* bits, uint32_t cell) {
  atomicOr(&bits[cell >> 5], 1u << (cell & 31));
}
__device__ __forceinline__ bool bitmap_test(const uint32_t* __restrict__ bits, uint32_t cell) {
  return (bits[cell >> 5] >> (cell & 31)) & 1u;
}
__device__ __forceinline__ int bitmap_rank(const uint32_t* __restrict__ bits,
                                           const int* __restrict__ prefix, uint32_t cell) {
  return prefix[cell >> 5] + __popc(bits[cell >> 5] & ((1u << (cell & 31)) - 1u));
}

}  // namespace msmd
