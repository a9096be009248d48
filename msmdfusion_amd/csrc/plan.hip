// plan.hip -- everything the conv kernels derive from a neighbour table: the tiling order,
// the table in tile order, the stream-K prefixes, the reference pair lists, the one-chunk
// wgrad segment table.  ONE set of kernels, for one table or for all tables of an index pass.
//
// The conv kernels tile the output rows of a table in an order that puts rows with similar
// offset masks into the same wave / 128-row tile (spconv.hip: row_mask_kernel has the
// reasoning and the measured effect; tiling_key.hpp the key).  No re-sequencing of whole
// tiles: stream-K, the split kernels' schedule, cuts the sequence into equal cost shares
// wherever the tiles lie, so a heaviest-first order (a cost pass and a second sort) bought
// nothing.
//
// One LC step plans ~21 tables.  Table by table that is ~13 launches each -- the 27-bit radix
// sort alone 7-8 -- of kernels that finish in 5-20 us on 20k-170k rows: ~280 launches and
// 3.2 ms of the index queue's 8.5 ms (profiles/r04_lc_stream_summary.txt), and the index
// queue's length IS the step.  Nothing in the index chain reads a plan (only
// the feature pass does), so the plans can wait until every table exists and run together as
// a GROUP of up to 32 tables described by one kernel argument (PlanTab):
//   keys of all rows (table id above the mask key) -> ONE radix sort -> order + tiled
//   tables -> tile weights -> prefixes -> pair tile sums -> pair lists -> segment tables,
// 7 kernels + one sort whatever the number of tables.  The sort is stable and the table id
// is the key's top bits, so a table's rows come out in the order a sort of its own gives
// them: a group of one IS the single-table plan, and msmd_rulebook_tiling / _plan / _pairs
// are groups of one.  Integer work, exact; any order gives the same conv results.
#include <hipcub/hipcub.hpp>

#include "common.hpp"
#include "scan.hpp"
#include "tiling_key.hpp"

namespace msmd {
int stream_k_c1();                                   // spconv_split.hip

namespace {

constexpr int kPlanMax = 32;      // tables per group (5 key bits)

struct PlanTab {
  int n, shift;              // tables; bit of the key the table id starts at
  int row0[kPlanMax + 1];    // first row of table s in the concatenation of all sorted rows
  int blk0[kPlanMax + 1];    // ... first 256-row block
  int tile0[kPlanMax + 1];   // ... first tile-weight block (128-row tiles, then 256-row ones)
  int pblk0[kPlanMax + 1];   // ... first pair-scan block (kvol * tiles-per-offset each)
  msmd_plan_desc d[kPlanMax];
};

__global__ __launch_bounds__(256) void keys_many_kernel(const PlanTab tab,
                                                        uint32_t* __restrict__ keys,
                                                        int32_t* __restrict__ vals) {
  const int s = segment_of(tab.blk0, tab.n, blockIdx.x);
  const msmd_plan_desc& d = tab.d[s];
  const int o = (blockIdx.x - tab.blk0[s]) * 256 + threadIdx.x;
  if (o >= d.n_rows) return;
  const int g = tab.row0[s] + o;
  // (a 32-bit key leaves no room for an id: such a table is a group of its own, id 0)
  const uint32_t id = tab.shift < 32 ? (uint32_t)s << tab.shift : 0u;
  // (the Gray code of the ranked mask simulates 1.3 % better, 1.299 -> 1.282 items / useful
  // work; measured within noise, not used)
  keys[g] = id | row_key32(d.nbr, d.kvol, (size_t)d.n_rows, o);
  vals[g] = o;
}

// order[p] = the row at tile position p; tiled[k][p] = nbr[k][order[p]]
__global__ __launch_bounds__(256) void finish_many_kernel(const PlanTab tab,
                                                          const int32_t* __restrict__ sorted) {
  const int s = segment_of(tab.blk0, tab.n, blockIdx.x);
  const msmd_plan_desc& d = tab.d[s];
  const int p = (blockIdx.x - tab.blk0[s]) * 256 + threadIdx.x;
  const int n = d.n_rows;
  if (p >= n) return;
  const int row = sorted[tab.row0[s] + p];
  d.order[p] = row;
  if (d.tiled) {
    const int32_t* __restrict__ nbr = d.nbr;
    int32_t* __restrict__ tiled = d.tiled;
    for (int k = 0; k < d.kvol; ++k) tiled[(size_t)k * n + p] = nbr[(size_t)k * n + row];
  }
}

// spconv_split.hip: tile_weight_kernel for every (table, tile height, tile) -- from the SORTED
// KEYS instead of the tile-ordered table: position p of table s holds the row whose key is
// keys[row0[s] + p], and the key's low bits are the row's offset mask (ranked for 3x3x3: a
// permutation of the bits, which the weight -- a sum over the offsets -- does not see).  4
// bytes per row instead of 4 K: weight = c1 * |union of the tile's masks| + sum over its
// 32-row groups of |union of the group's masks|, rows past the table's end standing for the
// last row exactly as the table-reading kernel has it.  One wave per tile.
__global__ __launch_bounds__(256) void tile_weight_many_kernel(const PlanTab tab, int c1,
                                                               const uint32_t* __restrict__ keys,
                                                               int n_tiles) {
  const int vt = blockIdx.x * 4 + (threadIdx.x >> 6);        // tile of this wave
  if (vt >= n_tiles) return;
  const int lane = threadIdx.x & 63;
  const int s = segment_of(tab.tile0, tab.n, vt);
  const msmd_plan_desc& d = tab.d[s];
  const int n = d.n_rows, kvol = d.kvol;
  int t = vt - tab.tile0[s];
  const int t128 = d.prefix128 ? (n + 127) / 128 : 0;
  int rows = 128;
  int32_t* weight = d.prefix128;
  if (t >= t128) {
    t -= t128;
    rows = 256;
    weight = d.prefix256;
  }
  const uint32_t low = kvol >= 32 ? 0xffffffffu : ((1u << kvol) - 1u);
  const uint32_t* __restrict__ k = keys + tab.row0[s];
  uint32_t all = 0;
  int groups = 0;
  for (int g0 = 0; g0 < rows; g0 += 64) {                    // two 32-row groups per pass
    int p = t * rows + g0 + lane;
    p = p < n ? p : n - 1;
    uint32_t m = k[p] & low;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) m |= __shfl_xor(m, o);  // OR inside each 32-lane half
    const uint32_t m0 = __shfl(m, 0), m1 = __shfl(m, 32);
    all |= m0 | m1;
    groups += __popc(m0) + __popc(m1);
  }
  if (lane == 0) {
    const int w = c1 * __popc(all) + groups;
    weight[t] = w > 0 ? w : 1;
  }
}

// block 2s = table s's 128-row prefix, 2s + 1 its 256-row one
__global__ __launch_bounds__(1024) void tile_prefix_many_kernel(const PlanTab tab) {
  __shared__ int part[1024];
  const msmd_plan_desc& d = tab.d[blockIdx.x >> 1];
  const int rows = (blockIdx.x & 1) ? 256 : 128;
  int32_t* a = (blockIdx.x & 1) ? d.prefix256 : d.prefix128;
  if (a) block_prefix_in_place(a, (d.n_rows + rows - 1) / rows, part);
}

// Compaction of every table's K offsets in one launch set: block b of a table = scan tile
// b % tpk of offset b / tpk (each offset padded to whole tiles: rows_padded).  First the
// tiles' pair counts ...
__global__ __launch_bounds__(kScanBlock) void pair_sums_many_kernel(const PlanTab tab,
                                                                    int* __restrict__ tile_sums) {
  __shared__ int smem[kScanBlock / 64];
  const int s = segment_of(tab.pblk0, tab.n, blockIdx.x);
  const msmd_plan_desc& d = tab.d[s];
  const int n = d.n_rows;
  const int tpk = (n + kScanTile - 1) / kScanTile;
  const int b = blockIdx.x - tab.pblk0[s];
  const int k = b / tpk, base = (b - k * tpk) * kScanTile;
  const int32_t* __restrict__ nbr = d.nbr + (size_t)k * n;
  int c = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    const int o = base + j * kScanBlock + threadIdx.x;
    if (o < n) c += nbr[o] >= 0;
  }
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int i = 0; i < kScanBlock / 64; ++i) t += smem[i];
    tile_sums[blockIdx.x] = t;
  }
}

// ... then one offset's neighbours into the reference's pair lists, with the tail of both
// rows filled with -1 (the reference allocates indicePairs as full(-1), spconv_ops.h:55-59)
// by the table's EMPTY entries: entry o of offset k without a neighbour, the r-th such,
// writes position num_k + r.  No 0xFF fill of the whole [K,2,ld] tensor in front (19 MB per
// table at 90k rows, 12 tables per LC step), no scan of the tile sums, no separate count
// kernel: a block adds up the tile sums it needs.  The blocks of an offset also share the -1
// fill of the lists' entries past the padded table (ld > rows_pad: the strided convs, whose
// input side is the longer one).
__global__ __launch_bounds__(kScanBlock) void pairs_apply_many_kernel(
    const PlanTab tab, const int* __restrict__ tile_sums_all) {
  __shared__ int smem[kScanSmem];
  const int s = segment_of(tab.pblk0, tab.n, blockIdx.x);
  const msmd_plan_desc& d = tab.d[s];
  const int n_rows = d.n_rows, ld = d.ld;
  const int tpk = (n_rows + kScanTile - 1) / kScanTile, rows_pad = tpk * kScanTile;
  const int* __restrict__ tile_sums = tile_sums_all + tab.pblk0[s];
  const int b = blockIdx.x - tab.pblk0[s];
  const int k = b / tpk, tile_in_k = b - k * tpk;
  // pairs of this offset in front of this tile, and in the whole offset
  int carry = block_range_sum<kScanBlock>(tile_sums, k * tpk, b, smem);
  const int num_k = carry + block_range_sum<kScanBlock>(tile_sums, b, (k + 1) * tpk, smem);
  if (tile_in_k == 0 && threadIdx.x == 0) d.indice_num[k] = num_k;
  int32_t* __restrict__ pin = d.indice_pairs + ((size_t)k * 2 + 0) * ld;
  int32_t* __restrict__ pout = pin + ld;
  const int32_t* __restrict__ nbr = d.nbr + (size_t)k * n_rows;
  const int base = tile_in_k * kScanTile;
  int src[kScanItems], v[kScanItems], ex[kScanItems];
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    const int o = base + j * kScanBlock + threadIdx.x;
    src[j] = o < n_rows ? nbr[o] : -1;
    v[j] = src[j] >= 0;
  }
  tile_excl_scan(v, ex, smem);
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    const int o = base + j * kScanBlock + threadIdx.x;
    const int pos = carry + ex[j];         // pairs of offset k in front of entry o
    if (v[j]) {
      if (pos < ld) {
        pin[pos] = src[j];
        pout[pos] = o;
      }
    } else {
      const int tail = num_k + (o - pos);  // o - pos = empty entries in front of o
      if (tail < ld) {
        pin[tail] = -1;
        pout[tail] = -1;
      }
    }
  }
  if (ld > rows_pad) {
    const int per = (ld - rows_pad + tpk - 1) / tpk;
    const int lo = rows_pad + tile_in_k * per, hi = lo + per < ld ? lo + per : ld;
    for (int i = lo + threadIdx.x; i < hi; i += kScanBlock) {
      pin[i] = -1;
      pout[i] = -1;
    }
  }
}

// spconv_wgrad_block.hip: pair_segments_kernel for one chunk (= the whole pair list of every
// offset): prefix[K + 1] | p0[K] = 0 | cnt[K] = num.  One wave per table.
__global__ __launch_bounds__(64) void segtab_many_kernel(const PlanTab tab) {
  const msmd_plan_desc& d = tab.d[blockIdx.x];
  if (!d.segtab) return;
  const int kvol = d.kvol, k = threadIdx.x;
  const int n = k < kvol ? d.indice_num[k] : 0;
  const int steps = (n + 31) >> 5;
  int incl = steps;                                 // wave inclusive scan
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o);
    if (k >= o) incl += v;
  }
  int32_t* __restrict__ t = d.segtab;
  if (k < kvol) {
    t[k] = incl - steps;
    t[kvol + 1 + k] = 0;
    t[2 * kvol + 1 + k] = n;
  }
  if (k == kvol - 1) t[kvol] = incl;
}

// ------------------------------------------------------------------------ host side ---
// What one table adds to a group's launch grids.  Only a table with an order is sorted (and
// only such a table can have a tiled table or prefixes); an empty table adds nothing.
struct Extent {
  long rows, tiles, pblk;
  int key_bits;
};
inline Extent extent(const msmd_plan_desc& d) {
  Extent e{};
  if (d.n_rows <= 0 || d.kvol < 1) return e;
  if (d.order) {
    e.rows = d.n_rows;
    e.tiles = (d.prefix128 ? ceil_div(d.n_rows, 128) : 0) +
              (d.prefix256 ? ceil_div(d.n_rows, 256) : 0);
    e.key_bits = row_key_bits(d.kvol);
  }
  if (d.indice_pairs) e.pblk = (long)d.kvol * scan_num_tiles(d.n_rows);
  return e;
}

// Tables descs[0 .. return) form the next group.  The table id sits above the widest key of
// the group: a group closes when id and key no longer fit into 32 bits together (a table
// whose key needs all 32 -- K = 16..26, 28..31 -- is a group of one), at kPlanMax tables, and
// before 2^31 rows or pair blocks.
int group_size(const msmd_plan_desc* descs, int n_left) {
  int n = 0, shift = 0;
  long rows = 0, pblk = 0;
  for (; n < n_left && n < kPlanMax; ++n) {
    const Extent e = extent(descs[n]);
    const int sh = e.key_bits > shift ? e.key_bits : shift;
    if (n > 0 && (sh + next_pow2_bits(n + 1) > 32 || rows + e.rows >= 2147483647L ||
                  pblk + e.pblk >= 2147483647L))
      break;
    shift = sh;
    rows += e.rows;
    pblk += e.pblk;
  }
  return n;
}

// false: 2^31 rows or pair blocks (in one table: group_size closes a group before that)
bool fill_tab(const msmd_plan_desc* descs, int n, PlanTab* tab) {
  long rows = 0, blk = 0, tiles = 0, pblk = 0;
  tab->n = n;
  tab->shift = 0;
  tab->row0[0] = tab->blk0[0] = tab->tile0[0] = tab->pblk0[0] = 0;
  for (int s = 0; s < n; ++s) {
    const Extent e = extent(descs[s]);
    rows += e.rows;
    blk += ceil_div(e.rows, 256);
    tiles += e.tiles;
    pblk += e.pblk;
    if (rows >= 2147483647L || pblk >= 2147483647L) return false;
    if (e.key_bits > tab->shift) tab->shift = e.key_bits;
    tab->d[s] = descs[s];
    tab->row0[s + 1] = (int)rows;
    tab->blk0[s + 1] = (int)blk;
    tab->tile0[s + 1] = (int)tiles;
    tab->pblk0[s + 1] = (int)pblk;
  }
  return true;
}

struct PlanWs {
  uint32_t *keys, *keys_out;
  int32_t *vals, *sorted;
  int* tile_sums;
  void* cub;
  size_t cub_bytes;
};

template <typename A>
void carve(A& a, PlanWs* w, long rows, long pair_blocks) {
  PlanWs s{};
  if (rows > 0) {                  // (no table wants an order: nothing is sorted)
    hipcub::DeviceRadixSort::SortPairs(nullptr, s.cub_bytes, (uint32_t*)nullptr,
                                       (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                                       (int)rows);
    s.keys = a.template take<uint32_t>(rows);
    s.keys_out = a.template take<uint32_t>(rows);
    s.vals = a.template take<int32_t>(rows);
    s.sorted = a.template take<int32_t>(rows);
    s.cub = a.template take<char>(s.cub_bytes);
  }
  s.tile_sums = a.template take<int>((size_t)pair_blocks + 1);
  if (w) *w = s;
}

size_t group_bytes(const msmd_plan_desc* descs, int n) {
  PlanTab tab;
  if (!fill_tab(descs, n, &tab)) return 0;
  ArenaSize a;
  carve(a, (PlanWs*)nullptr, tab.row0[n], tab.pblk0[n]);
  return a.off;
}

// What msmd_rulebook_plan_many accepts of one table.
int check_desc(const msmd_plan_desc& d) {
  if (d.kvol < 1 || d.kvol > 31) return MSMD_ERR_UNSUPPORTED;
  if (d.n_rows < 0) return MSMD_ERR_INVALID_ARG;
  const bool ordered = d.tiled || d.prefix128 || d.prefix256;
  if (d.n_rows > 0 && (!d.nbr || (ordered && !d.order))) return MSMD_ERR_INVALID_ARG;
  if ((d.prefix128 || d.prefix256) && d.n_rows > 0 && !d.tiled) return MSMD_ERR_INVALID_ARG;
  if (d.indice_pairs && (!d.indice_num || d.ld < d.n_rows)) return MSMD_ERR_INVALID_ARG;
  if (d.segtab && !d.indice_pairs) return MSMD_ERR_INVALID_ARG;
  if ((double)d.kvol * rows_padded(d.n_rows) >= 2147483647.0) return MSMD_ERR_RANGE;
  return MSMD_OK;
}

// A table without rows: no kernel has a block for it.
void plan_empty(const msmd_plan_desc& d, hipStream_t st) {
  if (d.prefix128) hipMemsetAsync(d.prefix128, 0, sizeof(int32_t), st);
  if (d.prefix256) hipMemsetAsync(d.prefix256, 0, sizeof(int32_t), st);
  if (d.indice_pairs && d.ld > 0)
    hipMemsetAsync(d.indice_pairs, 0xFF, sizeof(int32_t) * (size_t)d.kvol * 2 * d.ld, st);
  if (d.indice_num) hipMemsetAsync(d.indice_num, 0, sizeof(int32_t) * d.kvol, st);
}

// One group (group_size) of tables whose descriptors the caller has validated: checks what
// only the group decides (size, workspace) and launches.  Nothing is enqueued on an error.
int run_group(const msmd_plan_desc* descs, int n, void* workspace, size_t workspace_bytes,
              hipStream_t st) {
  PlanTab tab;
  if (!fill_tab(descs, n, &tab)) return MSMD_ERR_RANGE;
  const int rows = tab.row0[n], nblk = tab.blk0[n], tiles = tab.tile0[n], pblk = tab.pblk0[n];
  Arena a(workspace, workspace_bytes);
  PlanWs w;
  carve(a, &w, rows, pblk);
  if (!workspace || !a.ok()) return MSMD_ERR_WORKSPACE;
  bool any_prefix = false, any_seg = false;
  for (int s = 0; s < n; ++s) {
    const msmd_plan_desc& d = descs[s];
    if (d.n_rows == 0) plan_empty(d, st);
    any_prefix |= d.prefix128 || d.prefix256;
    any_seg |= d.segtab != nullptr;
  }
  if (rows > 0) {
    MSMD_LAUNCH(keys_many_kernel, dim3(nblk), dim3(256), 0, st, tab, w.keys, w.vals);
    size_t cb = w.cub_bytes;
    const int end_bit = tab.shift + next_pow2_bits(n);   // the key's significant bits + the id's
    if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, w.keys, w.keys_out, w.vals, w.sorted, rows,
                                           0, end_bit, st) != hipSuccess)
      return MSMD_ERR_LAUNCH;
    MSMD_LAUNCH(finish_many_kernel, dim3(nblk), dim3(256), 0, st, tab, (const int32_t*)w.sorted);
  }
  if (tiles > 0)
    MSMD_LAUNCH(tile_weight_many_kernel, dim3(ceil_div(tiles, 4)), dim3(256), 0, st, tab,
                stream_k_c1(), (const uint32_t*)w.keys_out, tiles);
  if (any_prefix) MSMD_LAUNCH(tile_prefix_many_kernel, dim3(2 * n), dim3(1024), 0, st, tab);
  if (pblk > 0) {
    MSMD_LAUNCH(pair_sums_many_kernel, dim3(pblk), dim3(kScanBlock), 0, st, tab, w.tile_sums);
    MSMD_LAUNCH(pairs_apply_many_kernel, dim3(pblk), dim3(kScanBlock), 0, st, tab,
                (const int*)w.tile_sums);
  }
  if (any_seg) MSMD_LAUNCH(segtab_many_kernel, dim3(n), dim3(64), 0, st, tab);
  return launch_status();
}

// descriptor of the single-table entry points
msmd_plan_desc one_table(const int32_t* nbr, int kvol, int n_rows) {
  msmd_plan_desc d{};
  d.nbr = nbr;
  d.kvol = kvol;
  d.n_rows = n_rows;
  return d;
}
// ... and their workspace: a one-table group's, through the same carve
size_t one_table_bytes(int kvol, int n_rows, bool order, bool pairs) {
  if (kvol < 1 || n_rows < 0) return 0;
  ArenaSize a;
  carve(a, (PlanWs*)nullptr, order ? n_rows : 0, pairs ? (long)kvol * scan_num_tiles(n_rows) : 0);
  return a.off;
}

}  // namespace
}  // namespace msmd

using namespace msmd;

MSMD_EXPORT size_t msmd_rulebook_plan_many_workspace_bytes(const msmd_plan_desc* descs,
                                                           int n_desc) {
  if (!descs || n_desc < 0) return 0;
  size_t most = 0;
  for (int i = 0, g; i < n_desc; i += g) {                    // the groups plan_many runs
    g = group_size(descs + i, n_desc - i);
    const size_t b = group_bytes(descs + i, g);
    most = b > most ? b : most;
  }
  return most;
}

MSMD_EXPORT int msmd_rulebook_plan_many(const msmd_plan_desc* descs, int n_desc, void* workspace,
                                        size_t workspace_bytes, msmd_stream_t stream) {
  if (n_desc < 0 || (n_desc > 0 && !descs)) return MSMD_ERR_INVALID_ARG;
  if (n_desc == 0) return MSMD_OK;
  if (!workspace || ((uintptr_t)workspace & 255)) return MSMD_ERR_WORKSPACE;
  for (int i = 0; i < n_desc; ++i) {
    const int rc = check_desc(descs[i]);
    if (rc != MSMD_OK) return rc;
  }
  if (workspace_bytes < msmd_rulebook_plan_many_workspace_bytes(descs, n_desc))
    return MSMD_ERR_WORKSPACE;
  for (int i = 0, g; i < n_desc; i += g) {
    g = group_size(descs + i, n_desc - i);
    const int rc = run_group(descs + i, g, workspace, workspace_bytes, (hipStream_t)stream);
    if (rc != MSMD_OK) return rc;
  }
  return MSMD_OK;
}

// ------------------------------------------------ one table: a group of one ------------
MSMD_EXPORT size_t msmd_rulebook_tiling_workspace_bytes(int n_rows, int rows_per_tile) {
  return rows_per_tile < 1 ? 0 : one_table_bytes(1, n_rows, true, false);
}

MSMD_EXPORT int msmd_rulebook_tiling(const int32_t* nbr, int kernel_volume, int n_rows,
                                     int rows_per_tile, int32_t* order, int32_t* tiled,
                                     void* workspace, size_t workspace_bytes,
                                     msmd_stream_t stream) {
  if (kernel_volume < 1 || kernel_volume > 31) return MSMD_ERR_UNSUPPORTED;
  if (n_rows < 0 || rows_per_tile < 1 || (n_rows > 0 && (!nbr || !order)))
    return MSMD_ERR_INVALID_ARG;
  if (n_rows == 0) return MSMD_OK;
  msmd_plan_desc d = one_table(nbr, kernel_volume, n_rows);
  d.order = order;
  d.tiled = tiled;
  return run_group(&d, 1, workspace, workspace_bytes, (hipStream_t)stream);
}

MSMD_EXPORT size_t msmd_rulebook_plan_workspace_bytes(int kernel_volume, int n_rows,
                                                      int rows_per_tile) {
  return rows_per_tile < 1 ? 0 : one_table_bytes(kernel_volume, n_rows, true, true);
}

MSMD_EXPORT int msmd_rulebook_plan(const int32_t* nbr, int kernel_volume, int n_rows,
                                   int rows_per_tile, int32_t* order, int32_t* tiled,
                                   int32_t* prefix128, int32_t* prefix256, int32_t* indice_pairs,
                                   int ld, int32_t* indice_num, void* workspace,
                                   size_t workspace_bytes, msmd_stream_t stream) {
  if (!nbr || kernel_volume < 1 || n_rows < 1 || rows_per_tile < 1 || !order || !tiled)
    return MSMD_ERR_INVALID_ARG;
  msmd_plan_desc d = one_table(nbr, kernel_volume, n_rows);
  d.order = order;
  d.tiled = tiled;
  d.prefix128 = prefix128;
  d.prefix256 = prefix256;
  d.indice_pairs = indice_pairs;
  d.indice_num = indice_num;
  d.ld = ld;
  const int rc = check_desc(d);
  return rc != MSMD_OK ? rc : run_group(&d, 1, workspace, workspace_bytes, (hipStream_t)stream);
}

MSMD_EXPORT size_t msmd_rulebook_pairs_workspace_bytes(int kernel_volume, int n_rows) {
  return one_table_bytes(kernel_volume, n_rows, false, true);
}

// (no order: any kernel volume)
MSMD_EXPORT int msmd_rulebook_pairs(const int32_t* nbr, int kernel_volume, int n_rows,
                                    int32_t* indice_pairs, int ld, int32_t* indice_num,
                                    void* workspace, size_t workspace_bytes,
                                    msmd_stream_t stream) {
  if (kernel_volume < 1 || n_rows < 0 || ld < 0 || !indice_num ||
      (n_rows > 0 && (!nbr || !indice_pairs)))
    return MSMD_ERR_INVALID_ARG;
  if ((double)kernel_volume * rows_padded(n_rows) >= 2147483647.0) return MSMD_ERR_RANGE;
  msmd_plan_desc d = one_table(nbr, kernel_volume, n_rows);
  d.indice_pairs = indice_pairs;
  d.indice_num = indice_num;
  d.ld = ld;
  return run_group(&d, 1, workspace, workspace_bytes, (hipStream_t)stream);
}
