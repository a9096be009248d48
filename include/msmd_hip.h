/*
 * msmd_hip.h -- C ABI of libmsmd_hip.so: the MI355X (gfx950) implementation of
 * MSMDFusion's sparse-voxel fusion hot path.
 *
 * The reference has no C ABI for this path; its boundary is pybind11 torch
 * extensions plus the spconv-2.x Python package.  Every entry point below
 * names the reference interface it replaces (paths relative to the reference
 * checkout).  INTEGRATION.md shows the binding a reference maintainer adds.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless the
 *     parameter is documented "host";
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it,
 *     nothing synchronises the device, nothing allocates;
 *   - outputs and scratch are caller-allocated; scratch sizes come from the
 *     matching *_workspace_bytes() query; workspace base must be 256-B aligned;
 *   - the return value is an msmd_status (0 = ok, <0 = error, nothing was
 *     enqueued on error); msmd_status_string() names it;
 *   - re-entrant: no global mutable state; two streams may call concurrently
 *     with distinct workspaces.
 *   - tensors are dense row-major; `indices` rows are (batch, z, y, x) int32.
 */
#ifndef MSMD_HIP_H_
#define MSMD_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* msmd_stream_t; /* hipStream_t */

enum msmd_status {
  MSMD_OK = 0,
  MSMD_ERR_INVALID_ARG = -1,
  MSMD_ERR_WORKSPACE = -2,   /* workspace too small or misaligned            */
  MSMD_ERR_UNSUPPORTED = -3, /* shape / parameter outside the built kernels  */
  MSMD_ERR_LAUNCH = -4,      /* hipGetLastError() != hipSuccess after launch */
  MSMD_ERR_RANGE = -5        /* linear voxel id would not fit 32 bits        */
};

const char* msmd_status_string(int status);
/* hipGetErrorString() of the launch that made the calling thread's most recent
 * MSMD_ERR_LAUNCH. */
const char* msmd_last_launch_error(void);
/* ABI version: bumped whenever a signature below changes or is added (2: the n1 section). */
int msmd_abi_version(void);
/* 1 when a gfx950 device is visible to this process, else 0 (host call). */
int msmd_device_ok(void);

/* ------------------------------------------------------------------------ *
 * a1/a3  Hard voxelization (+ fused mean VFE)
 * replaces: voxel_layer.hard_voxelize  mmdet3d/ops/voxel/src/voxelization.h:51-69
 *           (CPU mmdet3d/ops/voxel/src/voxelization_cpu.cpp:44-142,
 *            CUDA mmdet3d/ops/voxel/src/voxelization_cuda.cu:184-326)
 *           HardSimpleVFE.forward  mmdet3d/models/voxel_encoders/voxel_encoder.py:29-46
 * Semantics kept bit-for-bit: float32 floor((p-min)/size) coordinates, grid =
 * round((max-min)/size), voxel id = rank of the voxel's first point in input
 * order, slot = number of earlier same-voxel points (< max_points kept), the
 * `break` at the point that would open voxel number max_voxels.
 * Only rows [0, *voxel_num) of voxels/coors/num_points_per_voxel are written
 * (padding slots inside a written voxel row are zero-filled); the caller
 * reads *voxel_num (device int32) after the stream reaches this point.
 * ------------------------------------------------------------------------ */
size_t msmd_voxelize_workspace_bytes(int num_points, int max_voxels,
                                     int max_points);

int msmd_hard_voxelize(const float* points, int num_points, int num_features,
                       const float* voxel_size /* host[3] x,y,z */,
                       const float* coors_range /* host[6] xyzxyz min,max */,
                       int max_points, int max_voxels,
                       float* voxels /* [max_voxels,max_points,C] or NULL */,
                       int32_t* coors /* [max_voxels,3] (z,y,x) */,
                       int32_t* num_points_per_voxel /* [max_voxels] */,
                       float* voxel_mean /* [max_voxels,C] or NULL: fused VFE */,
                       int32_t* voxel_num /* [1] */, void* workspace,
                       size_t workspace_bytes, msmd_stream_t stream);

/* The same for SEVERAL clouds in one launch set (the B LiDAR sweeps of a batch and the
 * virtual points of its four image scales: MSMDFusion.py:462-491 calls the voxel layer once
 * per sample and scale, each call its own voxel size): blocks find their cloud, the scan
 * restarts per cloud, one fill initialises every cloud's tables.  msmd_hard_voxelize is the
 * one-descriptor case of this call: the same kernels, a workspace of
 * msmd_voxelize_workspace_bytes (for an empty cloud, which only has *voxel_num = 0 written,
 * that is one 256-byte unit whatever max_voxels is).  The workspace is shared by the descriptors of a call.
 * Every descriptor, then the workspace (against the largest launch set of 12 clouds), is
 * checked before the first fill or launch: a call that returns an error has enqueued nothing
 * and leaves every output untouched. */
typedef struct msmd_voxelize_desc {
  const float* points;             /* [num_points, num_features] */
  int32_t num_points, num_features;
  float voxel_size[3];
  float coors_range[6];
  int32_t max_points, max_voxels;
  float* voxels;                   /* [max_voxels, max_points, num_features] or NULL */
  int32_t* coors;                  /* [max_voxels, 3] (z, y, x) */
  int32_t* num_points_per_voxel;   /* [max_voxels] */
  float* voxel_mean;               /* [max_voxels, num_features] or NULL */
  int32_t* voxel_num;              /* [1], device */
} msmd_voxelize_desc;
size_t msmd_hard_voxelize_many_workspace_bytes(const msmd_voxelize_desc* descs, int n_desc);
int msmd_hard_voxelize_many(const msmd_voxelize_desc* descs /* host */, int n_desc,
                            void* workspace, size_t workspace_bytes, msmd_stream_t stream);

/* HardSimpleVFE on an already materialised voxel tensor (unfused form). */
int msmd_voxel_mean(const float* voxels /* [M,max_points,C] */,
                    const int32_t* num_points_per_voxel, int num_voxels,
                    int max_points, int num_features, int out_features,
                    float* out /* [M,out_features] */, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a1d  Dynamic voxelization + DynamicScatter (sum / mean / max, fwd + bwd)
 * replaces: voxel_layer.dynamic_voxelize  mmdet3d/ops/voxel/src/voxelization.h:71-83
 *           (CUDA mmdet3d/ops/voxel/src/voxelization_cuda.cu:25-61, 328-371)
 *           voxel_layer.dynamic_point_to_voxel_forward  voxelization.h:96-108
 *           (CUDA mmdet3d/ops/voxel/src/scatter_points_cuda.cu:246-306)
 *           voxel_layer.dynamic_point_to_voxel_backward  voxelization.h:110-128
 *           (CUDA mmdet3d/ops/voxel/src/scatter_points_cuda.cu:308-383)
 *           DynamicVFE.map_voxel_center_to_point
 *           mmdet3d/models/voxel_encoders/voxel_encoder.py:176-218
 * ------------------------------------------------------------------------ */
/* One (z, y, x) row per point, float32 floor((p-min)/size), grid = round((max-min)/size);
 * out-of-range points get the reference kernel's pattern: x out of range writes -1 to slot
 * 0 only, y to slots 0-1, z to slots 0-2; unwritten slots keep the caller's values.
 * coors rows are `ndim` (>= 3) ints apart; slots 0-2 are the only ones touched. */
int msmd_dynamic_voxelize(const float* points, int num_points, int num_features,
                          const float* voxel_size /* host[3] x,y,z */,
                          const float* coors_range /* host[6] */, int ndim,
                          int32_t* coors /* [N, ndim] */, msmd_stream_t stream);

/* Index half of a scatter: depends on the coordinates only.  A row is invalid when any of
 * its ndim (1..8) entries is negative.  The M unique valid rows in lexicographic order go to
 * voxel_coors rows [0, M); point2voxel[i] = row of point i or -1; the points of voxel v are
 * seg_points[seg_start[v] .. seg_start[v+1]) in ascending point index; counts[v] = their
 * number.  info[0] = M, info[1] = 1 when the packed 64-bit row key would not hold the
 * columns' bit widths (then M = 0).  The caller reads info after the stream reaches here. */
size_t msmd_scatter_index_workspace_bytes(int num_points);
int msmd_scatter_index(const int32_t* coors /* [N, ndim] */, int num_points, int ndim,
                       int32_t* voxel_coors /* [N, ndim] */, int32_t* point2voxel /* [N] */,
                       int32_t* seg_points /* [N] */, int32_t* seg_start /* [N+1] */,
                       int32_t* counts /* [N] */, int32_t* info /* [2] */, void* workspace,
                       size_t workspace_bytes, msmd_stream_t stream);
/* out[v, c] = sum (reduce 0) / mean (1) / max (2) of feats over segment v, accumulated in
 * fp32 in ascending point index (no atomics: bitwise reproducible).  max also writes
 * argmax[v, c] = the smallest point index attaining the maximum (argmax may be NULL). */
int msmd_scatter_reduce_f32(const float* feats /* [N, C] */, int num_points, int num_channels,
                            const int32_t* seg_points, const int32_t* seg_start, int num_voxels,
                            int reduce, float* out /* [M, C] */, int32_t* argmax /* [M, C] */,
                            msmd_stream_t stream);
/* grad_in[i, c]: reduce 0 -> grad_out[v, c]; 1 -> grad_out[v, c] / counts[v]; 2 ->
 * grad_out[v, c] where argmax[v, c] == i; 0 for other points and for point2voxel < 0. */
int msmd_scatter_reduce_bwd_f32(const float* grad_out /* [M, C] */, int num_voxels,
                                int num_points, int num_channels, const int32_t* point2voxel,
                                const int32_t* counts, const int32_t* argmax, int reduce,
                                float* grad_in /* [N, C] */, msmd_stream_t stream);
/* The reference backward's traceback: argmax[v, c] = smallest point i of voxel v with
 * feats[i, c] == reduced[v, c] (num_points where there is none). */
int msmd_scatter_max_argmax_f32(const float* feats /* [N, C] */, int num_points,
                                int num_channels, const int32_t* point2voxel,
                                const float* reduced /* [M, C] */, int num_voxels,
                                int32_t* argmax /* [M, C] */, msmd_stream_t stream);
/* out[i, c] = voxel_feats[point2voxel[i], c], 0 where point2voxel[i] < 0.  Its backward is
 * msmd_scatter_reduce_f32 (sum) on the same segments. */
int msmd_scatter_gather_f32(const float* voxel_feats /* [M, C] */, int num_voxels,
                            int num_channels, const int32_t* point2voxel, int num_points,
                            float* out /* [N, C] */, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * r1  RoI-aware 3-D pooling (max / avg, fwd + bwd) and points-in-boxes
 * replaces: roiaware_pool3d_ext.forward  mmdet3d/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:49-90
 *           (CUDA roiaware_pool3d_kernel.cu:17-275: generate_pts_mask_for_box3d,
 *            collect_inside_pts_for_box3d, roiaware_maxpool3d / _avgpool3d)
 *           roiaware_pool3d_ext.backward  roiaware_pool3d.cpp:92-124
 *           (CUDA roiaware_pool3d_kernel.cu:277-366)
 *           roiaware_pool3d_ext.points_in_boxes_gpu / _batch
 *           (CUDA mmdet3d/ops/roiaware_pool3d/src/points_in_boxes_cuda.cu:24-203)
 * Boxes / RoIs are rows of 7 floats (x, y, z of the bottom centre, w, l, h, rz), points rows
 * of 3.  The predicate, the voxel of a point and the pooling semantics are pinned in
 * csrc/roiaware.hip.  out_x/y/z must be 1..256 (MSMD_ERR_UNSUPPORTED otherwise).  A cell is
 * one (RoI, voxel): cell = r * (out_x*out_y*out_z) + (ix*out_y + iy)*out_z + iz.
 * ------------------------------------------------------------------------ */
/* Index half, phase 1: tile_start[0 .. T) <- exclusive offsets of the hits of every (RoI,
 * 2048-point tile), tile_start[T] <- the total number of hits H, the one value the caller
 * reads; T = msmd_roiaware_num_tiles().  roi_batch / pts_batch (NULL: all 0): a point is
 * tested only against the RoIs of its own batch id. */
size_t msmd_roiaware_num_tiles(int num_rois, int num_points);
size_t msmd_roiaware_count_workspace_bytes(int num_rois, int num_points);
int msmd_roiaware_count(const float* rois /* [R, 7] */, const int32_t* roi_batch /* [R] */,
                        int num_rois, const float* pts /* [P, 3] */,
                        const int32_t* pts_batch /* [P] */, int num_points,
                        int32_t* tile_start /* [T + 1] */, void* workspace,
                        size_t workspace_bytes, msmd_stream_t stream);
/* Phase 2 (the same geometry, tile_start and H of phase 1): the compact point-list index.
 * hit_pts[vox_start[cell] ..) = the points of the cell in ascending point index, of which the
 * first min(size, max_pts_per_voxel - 1) are kept; vox_start has R*V + 1 entries.  The
 * inverse: inv_cell[pt_start[p] .. pt_start[p+1]) = the cells of p's kept hits in ascending
 * RoI order.  Nothing is read back. */
size_t msmd_roiaware_index_workspace_bytes(int num_hits);
int msmd_roiaware_index(const float* rois, const int32_t* roi_batch, int num_rois,
                        const float* pts, const int32_t* pts_batch, int num_points, int out_x,
                        int out_y, int out_z, int max_pts_per_voxel, const int32_t* tile_start,
                        int num_hits, int32_t* hit_pts /* [H] */,
                        int32_t* vox_start /* [R*V + 1] */, int64_t* inv_cell /* [H] */,
                        int32_t* pt_start /* [P + 1] */, void* workspace, size_t workspace_bytes,
                        msmd_stream_t stream);
/* Feature half: pooled[cell, c] (mode 0 max + argmax[cell, c], 1 avg) over the index.
 * ref_writes = 0: every element written (no winner / empty -> 0, argmax -1, argmax may be
 * NULL); 1: only where the reference writes (max: pooled where a point won, argmax always;
 * avg: pooled where the count is > 0).  hit_pts may be NULL when the index has no hits. */
int msmd_roiaware_pool_f32(const float* pts_feature /* [P, C] */, int num_points,
                           int num_channels, const int32_t* hit_pts, const int32_t* vox_start,
                           int64_t num_cells, int max_pts_per_voxel, int mode, int ref_writes,
                           float* pooled /* [cells, C] */, int32_t* argmax /* [cells, C] */,
                           msmd_stream_t stream);
/* grad_in[p, c] (= when accumulate is 0, += otherwise) the sum of p's contributions in
 * ascending RoI order, float32, written once per element (no float atomics). */
int msmd_roiaware_pool_bwd_f32(const float* grad_out /* [cells, C] */, int64_t num_cells,
                               int num_channels, const int32_t* vox_start, int max_pts_per_voxel,
                               const int64_t* inv_cell, const int32_t* pt_start, int num_points,
                               const int32_t* argmax /* [cells, C], max only */, int mode,
                               int accumulate, float* grad_in /* [P, C] */, msmd_stream_t stream);
/* The reference's pts_idx_of_voxels [cells, max_pts_per_voxel]: slot 0 = count, slots
 * 1..count = the points; other slots keep the caller's values. */
int msmd_roiaware_write_table(const int32_t* hit_pts, const int32_t* vox_start,
                              int64_t num_cells, int max_pts_per_voxel,
                              int32_t* pts_idx_of_voxels, msmd_stream_t stream);
/* The index rebuilt from a caller's padded table (the shim's backward): phase 1 writes
 * vox_start[0 .. cells] from the counts (clamped to 0 .. max_pts_per_voxel - 1; the total E
 * at vox_start[cells], read by the caller); phase 2 fills hit_pts[E] and the inverse.  Table
 * entries outside [0, num_points) are left out of the inverse.  One workspace query for both
 * phases (phase 1: num_entries = 0). */
size_t msmd_roiaware_table_workspace_bytes(int64_t num_cells, int num_entries);
int msmd_roiaware_table_count(const int32_t* pts_idx_of_voxels, int64_t num_cells,
                              int max_pts_per_voxel, int32_t* vox_start /* [cells + 1] */,
                              void* workspace, size_t workspace_bytes, msmd_stream_t stream);
int msmd_roiaware_table_index(const int32_t* pts_idx_of_voxels, int64_t num_cells,
                              int max_pts_per_voxel, int num_points, int num_entries,
                              const int32_t* vox_start, int32_t* hit_pts /* [E] */,
                              int64_t* inv_cell /* [E] */, int32_t* pt_start /* [P + 1] */,
                              void* workspace, size_t workspace_bytes, msmd_stream_t stream);
/* points_in_boxes_gpu (all_hits 0): out[b, i] = first box k holding point i, else -1 (every
 * element written); points_in_boxes_batch (all_hits 1): out[b, i, k] = 0 / 1. */
int msmd_points_in_boxes_f32(const float* boxes /* [B, T, 7] */, const float* pts /* [B, M, 3] */,
                             int batch_size, int num_boxes, int num_points, int all_hits,
                             int32_t* out, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a5  Submanifold rulebook (hash-based voxel index)
 * replaces: sparse_conv_ext.get_indice_pairs_3d(..., subM=1)
 *           mmdet3d/ops/spconv/src/all.cc:21-27,
 *           mmdet3d/ops/spconv/include/spconv/spconv_ops.h:28-107,
 *           algorithm geometry.h:247-297 (getIndicePairsSubM), CUDA
 *           indice.cu.h:148-203; spconv-2.x ops.get_indice_pairs_implicit_gemm
 *           (bug_fix/conv.py:382-396).
 * Output is output-stationary: nbr[k*n + o] = input row feeding output row o
 * through kernel offset k ((kz*KH+ky)*KW+kx, geometry.h:62-73), or -1.
 * msmd_rulebook_pairs() converts it to the reference's indicePairs/indiceNum.
 * ------------------------------------------------------------------------ */
size_t msmd_rulebook_subm_workspace_bytes(int n);

int msmd_rulebook_subm3d(const int32_t* indices /* [n,4] */, int n,
                         int batch_size, const int* spatial_shape /* host[3] */,
                         const int* ksize /* host[3] */,
                         int32_t* nbr /* [K,n] */, void* workspace,
                         size_t workspace_bytes, msmd_stream_t stream);

/* The same table through an occupancy bitmap of the grid instead of the hash (1 bit per
 * cell, a popcount prefix per 256-cell block, a rank -> row table): cost = a clear and a
 * counting pass over batch_size * D*H*W / 8 bytes plus ~9 word reads per voxel, against 27
 * random slot reads per voxel for the hash -- the better choice for large voxel sets and
 * for the small grids of the deeper stages.  Identical output (duplicates keep the last
 * row). */
size_t msmd_rulebook_subm_bitmap_workspace_bytes(int n, int batch_size,
                                                 const int* spatial_shape);
int msmd_rulebook_subm3d_bitmap(const int32_t* indices, int n, int batch_size,
                                const int* spatial_shape, const int* ksize,
                                int32_t* nbr, void* workspace, size_t workspace_bytes,
                                msmd_stream_t stream);

/* msmd_rulebook_subm3d / _bitmap for MANY voxel sets in one launch set (2 fills + at most 7
 * kernels whatever the number of tables): an index pass builds the SubM tables of all its
 * voxel sets together at its end -- nothing in the index chain reads one.  descs: HOST
 * array; method 0 = hash index, 1 = occupancy bitmap; tables with n = 0 are skipped.
 * msmd_rulebook_subm3d (method 0) and msmd_rulebook_subm3d_bitmap (method 1) are the
 * one-descriptor case of this call: the same kernels, their *_workspace_bytes the size of
 * that one descriptor.  Every descriptor, then the workspace (against the largest launch set
 * of 16 tables), is checked before the first fill or launch: a call that returns an error
 * has enqueued nothing and leaves every table untouched. */
typedef struct msmd_subm_desc {
  const int32_t* indices;      /* [n,4] (b,z,y,x) */
  int32_t n, batch_size;
  int32_t spatial_shape[3], ksize[3];
  int32_t method, reserved;
  int32_t* nbr;                /* [K, n] */
} msmd_subm_desc;
size_t msmd_rulebook_subm3d_many_workspace_bytes(const msmd_subm_desc* descs, int n_desc);
int msmd_rulebook_subm3d_many(const msmd_subm_desc* descs, int n_desc, void* workspace,
                              size_t workspace_bytes, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a6  Strided (regular) sparse conv rulebook, two phases with one host read
 * replaces: sparse_conv_ext.get_indice_pairs_3d(..., subM=0)
 *           spconv_ops.h:108-137, geometry.h:144-194 (getIndicePairsConv),
 *           CUDA indice.cu.h:22-65,112-145 + torch::_unique.
 * Output rows are in ascending linear (b,z,y,x) id, the order of the
 * reference's CUDA path (spconv_ops.h:130).  Phase 1 marks the occupied
 * output cells and counts them (*n_out, device); the caller reads it,
 * allocates, then phase 2 fills out_indices / nbr_fwd / nbr_bwd.  The same
 * workspace must be passed, untouched, to both phases.
 * An input set that repeats a coordinate (only the reference_quirks unified sets can): the
 * table is output-stationary, one input row per (offset, output row) -- the LAST row of the
 * coordinate, deterministically, as every SubM look-up; nbr_bwd still lists the output row
 * for every input row (the earlier rows receive the gradient of a contribution the forward
 * pass did not take from them: INTEGRATION.md).
 * ------------------------------------------------------------------------ */
size_t msmd_rulebook_conv_workspace_bytes(int batch_size,
                                          const int* out_shape /* host[3] */);

int msmd_rulebook_conv3d_count(const int32_t* indices /* [n,4] */, int n,
                               int batch_size, const int* out_shape,
                               const int* ksize, const int* stride,
                               const int* padding, int32_t* n_out /* [1] */,
                               void* workspace, size_t workspace_bytes,
                               msmd_stream_t stream);

int msmd_rulebook_conv3d_fill(const int32_t* indices, int n, int batch_size,
                              const int* out_shape, const int* ksize,
                              const int* stride, const int* padding, int n_out,
                              int32_t* out_indices /* [n_out,4] */,
                              int32_t* nbr_fwd /* [K,n_out] in-row or -1 */,
                              int32_t* nbr_bwd /* [K,n]    out-row or -1 */,
                              void* workspace, size_t workspace_bytes,
                              msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a6t  Transposed sparse conv rulebook (SparseConvTranspose3d), same two phases
 * replaces: sparse_conv_ext.get_indice_pairs_3d(..., transpose=1)
 *           spconv_ops.h:108-137, geometry.h:87-140,196-245 (getValidOutPosTranspose,
 *           getIndicePairsDeConv).
 * Input coordinate c reaches output c*stride - padding + k (dilation 1); k is the
 * row-major index of the offset; cells outside [0, out_shape) are dropped.  out_shape is
 * the deconv size (in-1)*stride - 2*padding + ksize + output_padding (ops.py:33-43) and
 * the workspace is msmd_rulebook_conv_workspace_bytes(batch_size, out_shape).  Output
 * rows in ascending linear id; tables as msmd_rulebook_conv3d_fill's (at most one input
 * coordinate reaches an (offset, output row); a repeated coordinate: its LAST row).
 * ------------------------------------------------------------------------ */
int msmd_rulebook_deconv3d_count(const int32_t* indices /* [n,4] */, int n,
                                 int batch_size, const int* out_shape,
                                 const int* ksize, const int* stride,
                                 const int* padding, int32_t* n_out /* [1] */,
                                 void* workspace, size_t workspace_bytes,
                                 msmd_stream_t stream);

int msmd_rulebook_deconv3d_fill(const int32_t* indices, int n, int batch_size,
                                const int* out_shape, const int* ksize,
                                const int* stride, const int* padding, int n_out,
                                int32_t* out_indices /* [n_out,4] */,
                                int32_t* nbr_fwd /* [K,n_out] in-row or -1 */,
                                int32_t* nbr_bwd /* [K,n]    out-row or -1 */,
                                void* workspace, size_t workspace_bytes,
                                msmd_stream_t stream);

/* A chain of strided convs whose input set is the previous one's output set
 * (SparseEncoder: sparse_encoder.py:175-187, only SubM convs in between): all levels
 * counted back to back -- level l+1 is marked from level l's occupancy bitmap -- so the
 * host reads n_out[0..levels) ONCE instead of once per level (the reference's
 * getIndicePairs syncs per conv).  out_shapes / ksizes / strides / paddings: [levels][3].
 * The workspace is the concatenation of the per-level msmd_rulebook_conv_workspace_bytes
 * blocks (each rounded up to 256 bytes): afterwards msmd_rulebook_conv3d_fill runs per
 * level on its own block, level l's input rows being level l-1's out_indices. */
size_t msmd_rulebook_conv_chain_workspace_bytes(int batch_size, int levels,
                                                const int* out_shapes);
int msmd_rulebook_conv3d_count_chain(const int32_t* indices, int n, int batch_size,
                                     int levels, const int* out_shapes, const int* ksizes,
                                     const int* strides, const int* paddings,
                                     int32_t* n_out /* [levels] */, void* workspace,
                                     size_t workspace_bytes, msmd_stream_t stream);

/* The same idea for the fusion stack's stage chain (sparse_multimodal_encoder_painting.py:
 * 413-428): level l's strided conv takes the UNION (sparse_add) of an extra voxel set
 * extra[l] (host array of device pointers, [n_extra[l], 4] each) and the previous level's
 * output set; level 0 takes extra[0] as it is.  counts[2l] = |union_l| (l >= 1),
 * counts[2l + 1] = |out_l|, all counted back to back: ONE host read for the whole chain.
 * After the read the caller fills level by level with msmd_sparse_add_fill (workspace =
 * level l's union region) and msmd_rulebook_conv3d_fill (its conv region): the regions lie
 * in `workspace` in the order conv_0, union_1, conv_1, union_2, ..., each
 * align256(msmd_rulebook_conv_workspace_bytes(batch, its grid)) bytes
 * (msmd_sparse_add_workspace_bytes is the same layout).  in_shapes[l] = out_shapes[l - 1]. */
size_t msmd_rulebook_add_conv_chain_workspace_bytes(int batch_size, int levels,
                                                    const int* in_shapes, const int* out_shapes);
int msmd_rulebook_add_conv_count_chain(const int32_t* const* extra, const int* n_extra,
                                       int batch_size, int levels, const int* in_shapes,
                                       const int* out_shapes, const int* ksizes,
                                       const int* strides, const int* paddings, int32_t* counts,
                                       void* workspace, size_t workspace_bytes,
                                       msmd_stream_t stream);

/* nbr table -> reference rulebook format: indice_pairs[K,2,ld] (-1 padded,
 * pairs of one offset sorted by output row) and indice_num[K]
 * (spconv_ops.h:55-59).  n_rows = number of output rows of `nbr`. */
size_t msmd_rulebook_pairs_workspace_bytes(int kernel_volume, int n_rows);

int msmd_rulebook_pairs(const int32_t* nbr /* [K,n_rows] */, int kernel_volume,
                        int n_rows, int32_t* indice_pairs /* [K,2,ld] */,
                        int ld, int32_t* indice_num /* [K] */, void* workspace,
                        size_t workspace_bytes, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a7/a8  Sparse convolution arithmetic (implicit GEMM on MFMA)
 * replaces: sparse_conv_ext.indice_conv_fp32 / indice_conv_backward_fp32
 *           all.cc:28-51, spconv_ops.h:260-456 (+ reordering.cc:20-50);
 *           spconv-2.x Fsp.implicit_gemm (bug_fix/conv.py:441-447).
 *   out[o,:] = sum_k in[nbr[k,o],:] @ W[k]          (W[k] is [c_in,c_out])
 * `weight` is plain [K,c_in,c_out] fp32; msmd_spconv_pack_weight() converts
 * it (optionally transposing each W[k]) to the MFMA fragment order the
 * kernels read; packed size is K*round16(c_in)*round16(c_out) floats.
 * dgrad = the same kernel on the backward table with transposed weights.
 * `weight_flip` != 0 pairs table row k with weight K-1-k: a SubM (odd kernel)
 * forward table read that way IS its backward table, so SubM dgrad needs no
 * second rulebook.
 * ------------------------------------------------------------------------ */
size_t msmd_spconv_packed_weight_elems(int kernel_volume, int c_in, int c_out);

int msmd_spconv_pack_weight(const float* weight, int kernel_volume, int c_in,
                            int c_out,
                            int flags /* bit0: pack W[k]^T (dgrad);
                                         bit1: weight is KRSC [c_out,K,c_in]
                                               (bug_fix/conv.py:114-117) instead
                                               of [K,c_in,c_out] */,
                            float* packed, msmd_stream_t stream);

/* `row_order` (NULL or a permutation of [0,n_out)): the order in which output
 * rows are tiled.  Any permutation gives bit-identical results; sorting rows
 * by msmd_rulebook_row_masks() lets whole waves / workgroups skip the kernel
 * offsets none of their rows is connected through. */
int msmd_spconv_fwd_f32(const float* in_feat /* [n_in,c_in] */, int n_in,
                        int c_in, const float* packed_weight,
                        const int32_t* nbr /* [K,ld] */, int ld, int n_out,
                        int kernel_volume, int weight_flip,
                        const int32_t* row_order /* [n_out] or NULL */,
                        int32_t* tile_counter /* [1] scratch or NULL */,
                        float* out_feat /* [n_out,c_out] */, int c_out,
                        msmd_stream_t stream);
/* tile_counter != NULL selects the persistent form: a fixed number of resident
 * workgroups draw row tiles from *tile_counter -- with a heaviest-first
 * row_order this balances the very uneven per-tile cost.  *tile_counter must
 * be 0 on entry; the kernel's last draw puts it back to 0, so one zeroed word
 * per stream serves every launch (no memset between launches). */

/* ---- the same convolution at bf16 MFMA rate, fp32-equivalent results -------
 * Every fp32 operand is the exact sum of three bf16 values (h + m + l); six
 * bf16 products accumulated in fp32 reproduce the fp32 product to ~2^-23 (the
 * dropped cross terms are below fp32's own rounding), at 2.7x fewer matrix-core
 * cycles than the fp32 MFMA.  `planes` = 3 is that mode; 2 keeps three products
 * (relative error ~2^-17); 1 is plain bf16 operands.  Features are read as fp32
 * and split in registers; weights are split by the pack call.
 * Non-finite operands: a NaN stays NaN.  An INFINITE operand becomes NaN with planes >= 2,
 * where msmd_spconv_fwd_f32 returns inf: the first plane is bf16(inf) = inf and the
 * residual plane inf - inf = NaN.  planes = 1 has no residual and returns inf like the fp32
 * kernel.  Either way exactly the output rows connected to the operand's row change (every
 * element of them: a zero weight does not mask a NaN); all other rows are bit-identical to
 * the clean run under every scheduling mode, and a row that no table entry refers to is
 * never read.  The same holds for msmd_spconv_wgrad_split per kernel offset
 * (tests/test_gpu_conv_edges.py pins both).
 * Covers c_in % 8 == 0 and c_out % 4 == 0, both >= 32, K <= 32 (ask
 * msmd_spconv_fwd_split_supported; c_out > 128 runs in column passes); other
 * layers use msmd_spconv_fwd_f32.
 * With `row_order`, `nbr` must be in TILE order: nbr[k][p] refers to output row
 * row_order[p] (msmd_rulebook_permute_cols).  `tile_counter` is required.      */
int msmd_spconv_fwd_split_supported(int c_in, int c_out, int kernel_volume);

size_t msmd_spconv_packed_split_bytes(int kernel_volume, int c_in /* contraction */,
                                      int c_out /* outputs */, int planes);

int msmd_spconv_pack_weight_split(const float* weight, int kernel_volume, int c_in,
                                  int c_out, int flags /* as msmd_spconv_pack_weight */,
                                  int planes, void* packed, msmd_stream_t stream);
/* The same plus the image of the opposite transposition (flags ^ 1), one launch:
 * forward and dgrad of a conv read one each. */
int msmd_spconv_pack_weight_split_pair(const float* weight, int kernel_volume, int c_in,
                                       int c_out, int flags, int planes, void* packed,
                                       void* packed_transposed, msmd_stream_t stream);

/* Several weights in one launch (a training step repacks every trained conv's weight after
 * the optimizer has moved it: one launch instead of one per conv).  descs: n_desc descriptors
 * in DEVICE memory, 48 bytes each
 *   { const float* weight; void* packed; void* packed_transposed (or NULL); int64_t start;
 *     int32_t kernel_volume, c_in, c_out, flags; }
 * with start = the running count of work units in front of this weight (descriptor order; a
 * weight's units = msmd_spconv_packed_split_bytes / (16 * planes) of each image it writes) and
 * total_units their sum.  Images as msmd_spconv_pack_weight_split[_pair]. */
int msmd_spconv_pack_weight_split_many(const void* descs, int n_desc, long total_units,
                                       int planes, msmd_stream_t stream);

/* `tile_counter`: `sync_ints` zeroed int32 owned by the stream ([0] = the tile
 * counter, [1 + t] = exchange flag of row tile t); every launch leaves all of them
 * at 0 again.  `workspace` (msmd_spconv_fwd_split_workspace_bytes; may be NULL):
 * exchange buffer that lets the heaviest 128-row tiles run as two scheduling units
 * -- used when sync_ints >= 1 + ceil(n_out / 128) and the row tiles alone would
 * leave the workgroup slots unbalanced; without it every tile is one unit.  The
 * sum order per output element is fixed either way (deterministic), but differs
 * between the two modes in the last bit.                                        */
size_t msmd_spconv_fwd_split_workspace_bytes(int n_out, int c_out);

int msmd_spconv_fwd_split(const float* in_feat /* [n_in,c_in] */, int n_in, int c_in,
                          const void* packed_weight, const int32_t* nbr /* [K,ld] */,
                          int ld, int n_out, int kernel_volume, int weight_flip,
                          const int32_t* row_order /* [n_out] or NULL */,
                          int32_t* tile_counter /* [sync_ints] */, int sync_ints,
                          float* out_feat /* [n_out,c_out] */, int c_out, int planes,
                          void* workspace, size_t workspace_bytes,
                          const int32_t* tile_prefix /* msmd_rulebook_tile_prefix of `nbr`,
                                                        or NULL: dynamic tile scheduler */,
                          msmd_stream_t stream);

/* The same call that also leaves, per row tile of the output (128 or 256 rows:
 * msmd_spconv_fwd_split_tile_rows(c_out)), the pivoted column statistics of the rows it
 * wrote: bn_partials[msmd_spconv_fwd_split_stats_blocks(n_out, c_out)][3][c_out] = per channel a
 * pivot K (the tile's first row), sum (x - K) and sum (x - K)^2 over the tile's rows (raw
 * float32 sums of x and x^2 cancel for a channel far from zero) -- the statistics
 * pass of the BatchNorm1d that follows a conv in make_sparse_convmodule / SparseBasicBlock
 * (mmdet3d/ops/sparse_block.py:87-117,161-190) without reading the output again
 * (msmd_bn_act_fwd_from_partials_f32 takes them).  bn_partials = NULL: msmd_spconv_fwd_split. */
int msmd_spconv_fwd_split_stats(const float* in_feat, int n_in, int c_in,
                                const void* packed_weight, const int32_t* nbr, int ld,
                                int n_out, int kernel_volume, int weight_flip,
                                const int32_t* row_order, int32_t* tile_counter, int sync_ints,
                                float* out_feat, int c_out, int planes, void* workspace,
                                size_t workspace_bytes, const int32_t* tile_prefix,
                                float* bn_partials, msmd_stream_t stream);
int msmd_spconv_fwd_split_stats_blocks(int n_out, int c_out);

/* Rows per tile the split kernel uses for a layer of c_out output channels: 256 (the
 * ping-pong form: 8 waves, one workgroup and one weight stream per CU; 161..192 channels as
 * one 12-tile pass) from 161 channels up, 128 below -- the rows_per_tile to compute its
 * tile_prefix with. */
int msmd_spconv_fwd_split_tile_rows(int c_out);

/* Which instantiation of the split kernel msmd_spconv_fwd_split launches for a layer of c_out
 * output channels: params[7] = {NT column tiles per pass,
 * UB units per item, waves per workgroup, weight buffers, ping-pong 0|1, table buffers,
 * column passes = kernel launches per call}.  rocprofv3 names the kernel
 * spconv_fwd_split_kernel<NT, UB, planes, waves, buffers, pingpong, tables>.  For tools
 * (bench.py's roofline grouping, tools/split_bench.py); replaces nothing in the reference. */
int msmd_spconv_fwd_split_instantiation(int c_out, int* params);

/* Stream-K work table of a neighbour table (in the order the conv kernel tiles it):
 * prefix[t] = number of (row tile, active offset) work items before tile t, prefix[n_tiles]
 * = all of them (n_tiles = ceil(n_rows / rows_per_tile); an empty tile counts 1).  With it
 * msmd_spconv_fwd_split gives every workgroup the same share of the launch (see
 * csrc/spconv_split.hip); no reference counterpart. */
int msmd_rulebook_tile_prefix(const int32_t* nbr /* [K,ld] */, int kernel_volume, int ld,
                              int n_rows, int rows_per_tile,
                              int32_t* prefix /* [n_tiles + 1] */, msmd_stream_t stream);

/* wgrad with the same operand splitting (both operands are read as fp32 and split
 * into bf16 planes on the way to the matrix cores); c_in, c_out >= 64 and multiples of 4.
 * Widths that are multiples of 16 take the whole-block kernel (csrc/spconv_wgrad_block.hip:
 * one workgroup owns up to 128 x 128 channels of an offset, producer waves fetch and split
 * each pair's rows once, consumer waves only multiply); the others 64 x 64 slabs.
 * replaces: sparse_conv_ext.indice_conv_backward_fp32's filter-gradient half
 *           (mmdet3d/ops/spconv/include/spconv/spconv_ops.h:363-456).
 * Workspace as msmd_spconv_wgrad_workspace_bytes. */
int msmd_spconv_wgrad_split_supported(int c_in, int c_out);

int msmd_spconv_wgrad_split(const float* in_feat, int c_in, const float* d_out, int c_out,
                            const int32_t* indice_pairs /* [K,2,ld] */,
                            const int32_t* indice_num /* [K] device */, int ld,
                            int kernel_volume, int planes,
                            float* d_weight /* [K,c_in,c_out] */,
                            int krsc_out /* != 0: d_weight is [c_out,K,c_in] */,
                            void* workspace, size_t workspace_bytes, msmd_stream_t stream);

/* The same with the whole-block kernel's step sequence in ROW-CHUNK-major order: the pairs of
 * every offset are cut where their OUTPUT row crosses a multiple of chunk_rows, and the 27
 * pieces of a chunk are processed next to each other (same XCD, same time), so that a chunk's
 * d_out rows are fetched from HBM once for all offsets instead of once per offset
 * (csrc/spconv_wgrad_block.hip).  seg_table = msmd_rulebook_pair_segments' output for these
 * pair lists (index data: once per rulebook), n_chunks its chunk count; NULL = one chunk (the
 * plain offset-major sequence, what msmd_spconv_wgrad_split runs).  Same sums per (offset,
 * channel pair) in another fixed order: results agree to fp32 rounding, run to run identical.
 * Workspace: msmd_spconv_wgrad_segments_workspace_bytes.
 * msmd_rulebook_pair_segments_ints returns 0 for kernel volumes the whole-block kernel does
 * not take (> 64, e.g. 5x5x5): build no table, pass seg_table = NULL, the slab kernel runs. */
size_t msmd_rulebook_pair_segments_ints(int kernel_volume, int n_chunks);
int msmd_rulebook_pair_segments(const int32_t* indice_pairs /* [K,2,ld] */,
                                const int32_t* indice_num /* [K] device */, int ld,
                                int kernel_volume, int chunk_rows, int n_chunks /* <= 256,
                                chunk_rows * n_chunks >= ld */,
                                int32_t* table /* [msmd_rulebook_pair_segments_ints] */,
                                msmd_stream_t stream);
size_t msmd_spconv_wgrad_segments_workspace_bytes(int kernel_volume, int ld, int c_in, int c_out,
                                                  int n_chunks);
int msmd_spconv_wgrad_split_segments(const float* in_feat, int c_in, const float* d_out,
                                     int c_out, const int32_t* indice_pairs,
                                     const int32_t* indice_num, int ld, int kernel_volume,
                                     int planes, float* d_weight, int krsc_out,
                                     const int32_t* seg_table, int n_chunks, void* workspace,
                                     size_t workspace_bytes, msmd_stream_t stream);

/* out[k][p] = nbr[k][order[p]] for p < n: the neighbour table in tile order. */
int msmd_rulebook_permute_cols(const int32_t* nbr, int kernel_volume, int ld, int n,
                               const int32_t* order, int32_t* out /* [K,n] */,
                               msmd_stream_t stream);

/* masks[o] = bitset over k of (nbr[k][o] >= 0); sort_keys[o]: ascending order makes
 * rows with similar masks adjacent (3x3x3: the mask with its bits ranked centre <
 * faces < edges < corners; other volumes: heaviest mask first).  Either output may be
 * NULL.  kernel_volume <= 64.
 * msmd_rulebook_tile_costs: cost[t] = K - |union of the masks of rows
 * order[t*rows_per_tile ..)| -- ascending = the tile sequence (heaviest first) the
 * persistent conv kernels balance best on; `order` may be NULL (natural order).
 * Both only choose a tiling: conv results do not depend on it. */
/* The whole tiling of a table in one call: order[p] = output row at tile position p
 * (rows sorted by msmd_rulebook_row_masks' key) and, if `tiled` is not NULL,
 * tiled[k][p] = nbr[k][order[p]] (= msmd_rulebook_permute_cols).  An in-library radix sort
 * over the key's significant bits; kernel_volume <= 31, nbr is [K,n_rows]. */
size_t msmd_rulebook_tiling_workspace_bytes(int n_rows, int rows_per_tile);
int msmd_rulebook_tiling(const int32_t* nbr, int kernel_volume, int n_rows,
                         int rows_per_tile, int32_t* order /* [n_rows] */,
                         int32_t* tiled /* [K,n_rows] or NULL */, void* workspace,
                         size_t workspace_bytes, msmd_stream_t stream);

/* msmd_rulebook_tiling + msmd_rulebook_tile_prefix (128- and/or 256-row tiles; NULL to
 * skip) + msmd_rulebook_pairs (indice_pairs NULL to skip) of one table in one call: same
 * results, one host call instead of four (the index pass is host-bound). */
size_t msmd_rulebook_plan_workspace_bytes(int kernel_volume, int n_rows, int rows_per_tile);
int msmd_rulebook_plan(const int32_t* nbr, int kernel_volume, int n_rows,
                       int rows_per_tile, int32_t* order, int32_t* tiled,
                       int32_t* prefix128, int32_t* prefix256, int32_t* indice_pairs,
                       int ld, int32_t* indice_num, void* workspace,
                       size_t workspace_bytes, msmd_stream_t stream);

/* msmd_rulebook_plan (+ the one-chunk msmd_rulebook_pair_segments table) for MANY tables in
 * one launch set: an index pass plans every table of the step at its end -- nothing in the
 * index chain reads a plan -- with 7 kernels and one radix sort whatever the number of
 * tables (table id = the key's top bits; stable, so each table's order is its own sort's).
 * descs: HOST array.  Per table everything is optional (NULL): order / tiled / prefix128 /
 * prefix256 / indice_pairs (+ indice_num) / segtab; tiled and the prefixes need order, the
 * prefixes need tiled, segtab needs indice_pairs; ld >= n_rows.  Tables that ask for no order
 * are not sorted.  The single-table entry points above run the same kernels on a launch set
 * of one table, so the results are theirs.  Up to 32 tables share a launch set as long as
 * table id and sort key fit into 32 bits together (a kernel volume of 16..26 or 28..31 has
 * a 32-bit key: a set of its own). */
typedef struct msmd_plan_desc {
  const int32_t* nbr;        /* [K, n_rows] */
  int32_t kvol, n_rows;
  int32_t* order;            /* [n_rows]; required by tiled and the prefixes only */
  int32_t* tiled;            /* [K, n_rows] */
  int32_t* prefix128;        /* [ceil(n_rows / 128) + 1] */
  int32_t* prefix256;        /* [ceil(n_rows / 256) + 1] */
  int32_t* indice_pairs;     /* [K, 2, ld] */
  int32_t* indice_num;       /* [K] */
  int32_t* segtab;           /* [msmd_rulebook_pair_segments_ints(K, 1)] */
  int32_t ld, reserved;
} msmd_plan_desc;
size_t msmd_rulebook_plan_many_workspace_bytes(const msmd_plan_desc* descs, int n_desc);
int msmd_rulebook_plan_many(const msmd_plan_desc* descs, int n_desc, void* workspace,
                            size_t workspace_bytes, msmd_stream_t stream);

int msmd_rulebook_tile_costs(const int32_t* nbr /* [K,n_rows] */, int kernel_volume,
                             int n_rows, const int32_t* order, int rows_per_tile,
                             int32_t* cost /* [ceil(n_rows / rows_per_tile)] */,
                             msmd_stream_t stream);

int msmd_rulebook_row_masks(const int32_t* nbr /* [K,n_rows] */,
                            int kernel_volume, int n_rows, uint64_t* masks,
                            int64_t* sort_keys, msmd_stream_t stream);

/* dW[k] = sum over pairs p of offset k: in[pairs[k,0,p],:]^T (x) dout[pairs[k,1,p],:]
 * (spconv_ops.h:399,438).  Deterministic two-pass reduction. */
size_t msmd_spconv_wgrad_workspace_bytes(int kernel_volume, int ld, int c_in,
                                         int c_out);

int msmd_spconv_wgrad_f32(const float* in_feat, int c_in, const float* d_out,
                          int c_out, const int32_t* indice_pairs /* [K,2,ld] */,
                          const int32_t* indice_num /* [K] device */, int ld,
                          int kernel_volume, float* d_weight /* [K,c_in,c_out] */,
                          int krsc_out /* != 0: d_weight is [c_out,K,c_in] */,
                          void* workspace, size_t workspace_bytes,
                          msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a9/a10  BatchNorm1d (+ residual) (+ ReLU) on sparse-tensor features [n,c]
 * replaces: the nn.BatchNorm1d + nn.ReLU(inplace) pair make_sparse_convmodule
 *           appends to every sparse conv (mmdet3d/ops/sparse_block.py:161-190)
 *           and SparseBasicBlock's relu(bn2(conv2(x)) + identity) (:103-126).
 * training != 0: batch statistics (biased variance for normalisation,
 * running_var updated with the unbiased one, torch semantics; running_* may be
 * NULL = track_running_stats False, tools/train.py:205-211); else running stats.
 * save_mean / save_invstd [c] are outputs the backward needs.  c % 4 == 0.
 * ------------------------------------------------------------------------ */
size_t msmd_bn_workspace_bytes(int n, int c);

int msmd_bn_act_fwd_f32(const float* x /* [n,c] */, const float* residual /* or NULL */,
                        int n, int c, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, int training,
                        float momentum, float eps, int relu, float* y,
                        float* save_mean, float* save_invstd, void* workspace,
                        size_t workspace_bytes, msmd_stream_t stream);

/* Training-mode forward whose statistics pass was done by the producer of x:
 * partials[n_partials][3][c] = per block of rows_per_partial consecutive rows (the last block the
 * rest; n_partials = ceil(n / rows_per_partial), anything else is MSMD_ERR_INVALID_ARG) and per
 * channel a pivot K (any value near the block's, e.g. its first row), sum (x - K), sum (x - K)^2
 * (msmd_spconv_fwd_split_stats; there the blocks are the row tiles in tile order).  Same outputs
 * and running-stat update as msmd_bn_act_fwd_f32. */
int msmd_bn_act_fwd_from_partials_f32(const float* x, const float* residual, int n, int c,
                                      const float* gamma, const float* beta,
                                      float* running_mean, float* running_var, float momentum,
                                      float eps, int relu, float* y, float* save_mean,
                                      float* save_invstd, const float* partials, int n_partials,
                                      int rows_per_partial, msmd_stream_t stream);

int msmd_bn_act_bwd_f32(const float* x, const float* y /* fwd output, for the ReLU mask */,
                        const float* dy, int n, int c, const float* gamma,
                        const float* save_mean, const float* save_invstd,
                        int training,
                        float eps /* the forward's; training != 0 and eps > 0: the pass, which
                                     reads x anyway, takes the batch mean and variance again in
                                     fp64 instead of working from the float32 roundings in
                                     save_mean / save_invstd; <= 0: from those */,
                        int relu, float* dx,
                        float* dresidual /* or NULL */, float* dgamma, float* dbeta,
                        void* workspace, size_t workspace_bytes, msmd_stream_t stream);
/* BatchNorm + ReLU WITHOUT a residual, backward without y: the ReLU mask is recomputed from x
 * with the forward pass's own arithmetic (bit-identical decision), so the two streaming passes
 * read one array less each.  Results = msmd_bn_act_bwd_f32(relu = 1) given the forward's y. */
int msmd_bn_relu_bwd_f32(const float* x, const float* dy, int n, int c, const float* gamma,
                         const float* beta, const float* save_mean, const float* save_invstd,
                         int training, float eps /* as above */, float* dx, float* dgamma,
                         float* dbeta, void* workspace, size_t workspace_bytes,
                         msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a6p  Sparse max-pool (SparseMaxPool3d), fp32, any channel count
 * replaces: sparse_conv_ext.indice_maxpool_fp32 / indice_maxpool_backward_fp32
 *           (pool_ops.h:34,71; functors src/maxpool.cc:20-62)
 * Over the pool's rulebook (the strided conv rulebook of the same geometry), read
 * input-stationary through nbr_bwd[K, n_in] (output row or -1), which lists every
 * pair, repeated input coordinates included.
 * fwd: out [n_out,C] is zeroed here; an input value replaces the output only when
 *      out < in -- an all-negative window gives 0, a NaN never wins.  Exact.
 * bwd: din [n_in,C] = sum over k ascending of dout[o] where out[o] == in[i]; every
 *      element written once, no float atomics (the functor's order: bitwise equal).
 * ------------------------------------------------------------------------ */
int msmd_sparse_maxpool_fwd_f32(const float* in /* [n_in,C] */, int n_in, int num_channels,
                                const int32_t* nbr_bwd /* [K,n_in] */, int kvol, int n_out,
                                float* out /* [n_out,C] */, msmd_stream_t stream);
int msmd_sparse_maxpool_bwd_f32(const float* in /* [n_in,C] */,
                                const float* out /* [n_out,C] */,
                                const float* dout /* [n_out,C] */, int n_in,
                                int num_channels, const int32_t* nbr_bwd, int kvol,
                                int n_out, float* din /* [n_in,C] */,
                                msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a12  SparseConvTensor.dense(): BEV scatter
 * replaces: scatter_nd + permute + contiguous
 *           mmdet3d/ops/spconv/structure.py:5-18,55-64
 * out is [B,C,D,H,W] contiguous (channels-first) and is fully written
 * (zero-filled then scattered) by this call.  The backward gathers.
 * ------------------------------------------------------------------------ */
int msmd_dense_scatter_f32(const float* feat /* [n,c] */,
                           const int32_t* indices /* [n,4] */, int n, int c,
                           int batch_size, const int* spatial_shape,
                           float* out, msmd_stream_t stream);
int msmd_dense_gather_f32(const float* dense /* [B,C,D,H,W] */,
                          const int32_t* indices, int n, int c, int batch_size,
                          const int* spatial_shape, float* feat /* [n,c] */,
                          msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a12 -> f1  channels-last BEV hand-over
 * replaces: stage_outs[-1].dense(); .view(N, C*D, H, W); torch.cat([x, x_mm], 1)
 *           mmdet3d/models/detectors/MSMDFusion.py:436-440 (and
 *           mmdet3d/models/middle_encoders/sparse_encoder.py:187-190 for x)
 * bev is ONE [B,H,W,total_channels] buffer (the NHWC image of the reference's
 * [B, total_channels, H, W] tensor) the caller has zero-filled; a tensor with c
 * channels and depth D fills channels [channel_offset, channel_offset + c*D),
 * channel index c_i*D + z as .view(N, C*D, H, W) orders them.  gather = backward.
 * ------------------------------------------------------------------------ */
int msmd_bev_scatter_nhwc_f32(const float* feat /* [n,c] */,
                              const int32_t* indices /* [n,4] b,z,y,x */,
                              int n, int c, int batch_size,
                              const int* spatial_shape /* D,H,W */, float* bev,
                              int total_channels, int channel_offset,
                              msmd_stream_t stream);
int msmd_bev_gather_nhwc_f32(const float* bev, const int32_t* indices, int n,
                             int c, int batch_size, const int* spatial_shape,
                             float* feat /* [n,c] */, int total_channels,
                             int channel_offset, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a13 (image half)  MSMDFusionDetector.get_foreground2D, gather part
 * replaces: the per-(sample, camera) loop -- (fg_pxl * downscale).long(),
 *           img_feat.permute(1,2,0)[coord_h, coord_w], the torch.cat calls
 *           mmdet3d/models/detectors/MSMDFusion.py:195-224
 * All cameras of all samples in one call.  img_feat is [planes, c, h, w] with
 * arbitrary element strides (strides[4] = plane, channel, row, column), planes =
 * B * cameras.  pixels is [n,3] (x, y, depth) in float32 or float64, the numpy
 * dtype the loader produced: the product with `downscale` is taken in that
 * dtype and truncated toward zero like .long().  Negative cells wrap like
 * torch indexing; cells outside [-size, size) are COUNTED in *n_bad (the
 * reference raises IndexError there; the Python mirror raises on n_bad != 0)
 * and read as zeros.
 *   fg_pcd   [n, pts_dim + c]  = [pts | feat]
 *   score_in [n, c + 17]       = [feat | depth | lidar2img[plane] (16)]
 *   cells    [n] (optional)    = linear (plane, h, w) cell per point, -1 = bad;
 *                                input of msmd_fg_scatter_add_f32 (the backward)
 * ------------------------------------------------------------------------ */
int msmd_fg_gather_f32(const float* img_feat, const int64_t* strides,
                       int planes, int c, int h, int w, const void* pixels,
                       int pixel_is_f64, const int32_t* plane /* [n] */,
                       double downscale, const float* pts /* [n,pts_dim] */,
                       int pts_dim, const float* lidar2img /* [planes,16] */,
                       int n, float* fg_pcd, float* score_in, int32_t* cells,
                       int32_t* n_bad, msmd_stream_t stream);
/* The same gather with get_foreground2D's tail folded in, for the no-gradient case (the
 * reference's own training step: the result feeds voxelize(), which is @torch.no_grad(),
 * MSMDFusion.py:462): score = ReLU([feat | depth | lidar2img[plane]] . score_weight +
 * score_bias) (score_net = Linear(c + 17, 1) + ReLU, :125-128, :225-227) and
 *   fg_pcd [n, pts_dim + c] = [pts | feat * score]   for points [0, n_scaled),
 *                             [pts | feat]           for the rest (:229-234 copies the
 * scaled channels back for sample 0, and sample 1 when B == 2, only: reference_quirks).
 * score_in is never materialised.  c <= 64.  The dot product is summed in a fixed order. */
int msmd_fg_gather_scored_f32(const float* img_feat, const int64_t* strides,
                              int planes, int c, int h, int w, const void* pixels,
                              int pixel_is_f64, const int32_t* plane /* [n] */,
                              double downscale, const float* pts /* [n,pts_dim] */,
                              int pts_dim, const float* lidar2img /* [planes,16] */,
                              const float* score_weight /* [c + 17] */,
                              const float* score_bias /* [1] */, int n, int n_scaled,
                              float* fg_pcd, int32_t* n_bad, msmd_stream_t stream);
/* grad_img[plane, :, h, w] += grad[i, col0 : col0 + c]   (atomic fp32 adds: the
 * order, hence the last bit, is not fixed -- as index_put(accumulate) on a GPU) */
int msmd_fg_scatter_add_f32(const float* grad, int grad_stride, int col0,
                            const int32_t* cells, int n, int planes, int c,
                            int h, int w, const int64_t* strides,
                            float* grad_img, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * f2  depth_aware_channel_compression, sparse depth canvas
 * replaces: canvas[i,j].index_put_((y, x), depth) for B x 6 cameras
 *           mmdet3d/models/detectors/MSMDFusion.py:336-356
 * canvas is [planes, h, w], fully written.  Where several pixels land on one
 * cell the row with the highest index wins (what a sequential index_put_
 * leaves; the reference's CUDA index_put_ is unordered there).
 * ------------------------------------------------------------------------ */
size_t msmd_depth_canvas_workspace_bytes(int planes, int h, int w);
int msmd_depth_canvas_f32(const void* pixels /* [n,3] x,y,depth */,
                          int pixel_is_f64, const int32_t* plane, int n,
                          int planes, int h, int w, float* canvas,
                          int32_t* n_bad, void* workspace,
                          size_t workspace_bytes, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a17  spconv.pytorch.functional.sparse_add(a, b)
 * call site: mmdet3d/models/middle_encoders/sparse_multimodal_encoder_painting.py:455
 * Union of two coordinate sets on one grid, rows in ascending linear id,
 * features summed where both are present.  Two phases like the strided
 * rulebook; map_a/map_b give each input row's output row (for autograd).
 * ------------------------------------------------------------------------ */
size_t msmd_sparse_add_workspace_bytes(int batch_size, const int* spatial_shape);

int msmd_sparse_add_count(const int32_t* idx_a, int n_a, const int32_t* idx_b,
                          int n_b, int batch_size, const int* spatial_shape,
                          int32_t* n_out /* [1] */, void* workspace,
                          size_t workspace_bytes, msmd_stream_t stream);

int msmd_sparse_add_fill(const float* feat_a, const int32_t* idx_a, int n_a,
                         const float* feat_b, const int32_t* idx_b, int n_b,
                         int c, int batch_size, const int* spatial_shape,
                         int n_out, int32_t* out_indices /* [n_out,4] */,
                         float* out_feat /* [n_out,c] */,
                         int32_t* map_a /* [n_a] */, int32_t* map_b /* [n_b] */,
                         void* workspace, size_t workspace_bytes,
                         msmd_stream_t stream);
/* c == 0 makes msmd_sparse_add_fill an index-only pass (out_indices + maps; the
 * feature pointers may be NULL).  msmd_sparse_add_rows is then the feature half
 * on its own: out_feat[map_a[i]] += feat_a[i], out_feat[map_b[j]] += feat_b[j]
 * over a zeroed out_feat -- the same sums as the fused call, bit for bit (at
 * most two addends per element).  Together they let a caller that knows the
 * coordinate sets ahead of the features (step pipelining) keep the host read of
 * n_out off the feature pass. */
int msmd_sparse_add_rows(const float* feat_a, const int32_t* map_a, int n_a,
                         const float* feat_b, const int32_t* map_b, int n_b,
                         int c, int n_out, float* out_feat /* [n_out,c] */,
                         msmd_stream_t stream);

/* The same feature half as a gather, without a zero fill and without float atomics on the
 * common path: inv_x[j] = the last row of x that lands on output row j (msmd_rows_inverse of
 * map_x, once per batch); out[j] = a[inv_a[j]] + b[inv_b[j]].  Rows of one tensor that share
 * their coordinates (sparse_add sums those too) are added by a fix-up pass.  c % 4 == 0. */
int msmd_rows_inverse(const int32_t* map, int n, int n_out, int32_t* inv /* [n_out] */,
                      msmd_stream_t stream);
int msmd_sparse_add_rows_gather(const float* feat_a, const int32_t* map_a, const int32_t* inv_a,
                                int n_a, const float* feat_b, const int32_t* map_b,
                                const int32_t* inv_b, int n_b, int c, int n_out, float* out_feat,
                                msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a16  GMA-Conv stage assembly (one launch each way)
 * replaces: the index / cat / pad / mul chain of
 *           SparseMultiModalEncoderPaint.grouped_sparse_conv
 *           mmdet3d/models/middle_encoders/sparse_encoder_multimodal_encoderpaint_double_aware.py:349-421
 * out rows, in this order ([c3 | c2] columns):
 *   n_o3      only-3D rows   [ conv3[i]                       | 0 ]
 *   n_o2      only-2D rows   [ 0 | cross_gate[nn3[i] < 0 ? n3 : nn3[i]] * feat2[rows_o2[i]] ]
 *   n_o2_pad  zero rows (samples without an only-2D voxel, :208-225)
 *   n_mix     mixed rows     [ feat3[rows_m3[i]] | gate[i] * feat2[rows_m2[i]] ]
 *   n_mix_pad zero rows
 * backward: d_conv3 = left block of the only-3D rows, d_gate = right block of the
 * mixed rows * feat2, d_cross_gate[t] = sum over the only-2D rows whose nearest voxel is t
 * of right block * feat2.  With `order` (the only-2D rows sorted by nearest voxel, -1 as
 * n3) and `starts` (starts[t] .. starts[t+1] = target t's slice of `order`) the sum runs
 * in a fixed order, one wave per target (c2 <= 64); without them: a zero fill + float
 * atomics, like the index_add_ it replaces.  feat3 / feat2 receive no gradient.
 * c3, c2 multiples of 4. */
int msmd_gma_assemble_fwd_f32(const float* conv3, int n_o3, int c3, const float* cross_gate,
                              int n3, int c2, const int64_t* nn3, const float* feat2,
                              const int64_t* rows_o2, int n_o2, int n_o2_pad,
                              const float* feat3, const int64_t* rows_m3, const float* gate,
                              const int64_t* rows_m2, int n_mix, int n_mix_pad,
                              float* out /* [rows, c3 + c2] */, msmd_stream_t stream);
int msmd_gma_assemble_bwd_f32(const float* d_out, int n_o3, int c3, int n3, int c2,
                              const int64_t* nn3, const float* feat2, const int64_t* rows_o2,
                              int n_o2, int n_o2_pad, const int64_t* rows_m2, int n_mix,
                              int n_mix_pad, float* d_conv3 /* [n_o3,c3] */,
                              float* d_cross_gate /* [n3+1,c2] or NULL */,
                              float* d_gate /* [n_mix,c2] or NULL */,
                              const int64_t* order /* [n_o2] or NULL */,
                              const int64_t* starts /* [n3+2] or NULL */,
                              float* workspace /* ..._workspace_floats(c2) floats, with order */,
                              msmd_stream_t stream);
size_t msmd_gma_assemble_bwd_workspace_floats(int c2);

/* a16  the stage's gate tables: gate_control / cross_gate_control =
 * nn.Sequential(nn.Linear(c3, 64), nn.ReLU()) applied to the rows of the 3-D voxels
 * replaces: torch's Linear + ReLU (hipBLASLt GEMM + elementwise) at
 *           sparse_multimodal_encoder_painting.py:83-96 (definition), :398-417 (use)
 * y[n + n_tail, c_out] = relu?(cat(x, x_tail) w^T + b), w = nn.Linear's [c_out, c_in]
 * (x_tail: the dummy embedding row the reference concatenates, no copy of x needed);
 * backward: dw = g^T x, db = column sums of g, g = dy where y > 0 -- per-block partials
 * added in block order (deterministic).  c_out in {32, 64, 128}, c_in % 4 = 0
 * (msmd_rows_linear_supported). */
int msmd_rows_linear_supported(int c_in, int c_out);
int msmd_rows_linear_fwd_f32(const float* x, int n, const float* x_tail, int n_tail, int c_in,
                             const float* w, const float* b /* or NULL */, int c_out, int relu,
                             float* y, msmd_stream_t stream);
size_t msmd_rows_linear_bwd_workspace_bytes(int n_total, int c_in, int c_out);
int msmd_rows_linear_bwd_f32(const float* x, int n, const float* x_tail, int n_tail, int c_in,
                             const float* y, const float* dy, int c_out, int relu,
                             float* dw /* [c_out,c_in] */, float* db /* [c_out] or NULL */,
                             void* workspace, size_t workspace_bytes, msmd_stream_t stream);

/* a16b  both gates computed inside the stage assembly (a15 + a16 in one call each way)
 * out = msmd_gma_assemble_fwd_f32's, with cross_gate[t] = relu(w_cross feat3[t] + b_cross)
 * (t = n3: the dummy row) and gate[i] = relu(w_gate feat3[rows_m3[i]] + b_gate) computed
 * per output row -- the [n3 + 1, c2] table, of which the assembly reads a few per cent, is
 * never built.  backward: d_conv3 and the weight / bias gradients of both linears, from
 * per-block partials over the table rows that `order` / `starts` (as a15) refer to; the
 * ReLU masks are recomputed.  Every value equals the a16 -> a15 chain's to the bit (same
 * arithmetic, same summation order).  c2 = 64, c3 in {16, 32, 64, 128, 256}
 * (msmd_gma_stage_supported); weights are nn.Linear's [c2, c3]; biases may be NULL. */
int msmd_gma_stage_supported(int c3, int c2);
int msmd_gma_stage_fwd_f32(const float* conv3, int n_o3, int c3, const float* feat3, int n3,
                           int c2, const float* dummy /* [c3] */, const float* w_cross,
                           const float* b_cross, const float* w_gate, const float* b_gate,
                           const int64_t* nn3, const float* feat2, const int64_t* rows_o2,
                           int n_o2, int n_o2_pad, const int64_t* rows_m3,
                           const int64_t* rows_m2, int n_mix, int n_mix_pad,
                           float* out /* [rows, c3 + c2] */, msmd_stream_t stream);
size_t msmd_gma_stage_bwd_workspace_bytes(int n3, int n_mix, int c3, int c2);
int msmd_gma_stage_bwd_f32(const float* d_out, int n_o3, int c3, const float* feat3, int n3,
                           int c2, const float* dummy, const float* w_cross,
                           const float* b_cross, const float* w_gate, const float* b_gate,
                           const float* feat2, const int64_t* rows_o2, int n_o2, int n_o2_pad,
                           const int64_t* rows_m3, const int64_t* rows_m2, int n_mix,
                           int n_mix_pad, const int64_t* order /* [n_o2] */,
                           const int64_t* starts /* [n3+2] */, float* d_conv3 /* [n_o3,c3] */,
                           float* dw_cross /* [c2,c3] */, float* db_cross /* [c2] or NULL */,
                           float* dw_gate, float* db_gate, void* workspace,
                           size_t workspace_bytes, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a14  voxel_modality_split: LiDAR voxels vs virtual-point voxels
 * replaces: MSMDFusionDetector.voxel_modality_split + numba type_assign
 *           mmdet3d/models/detectors/MSMDFusion.py:27-45,251-325
 * mix3d[i]/mix2d[j] = 1 when the voxel exists in both sets (same b,z,y,x).
 * pair_3d/pair_2d list the matched rows, aligned, in ascending linear id;
 * *n_mixed (device) is their count.  Keys are exact integers (the reference's
 * float32 keys alias, SURVEY Appendix B.3 -- deliberate, documented fix).
 * ------------------------------------------------------------------------ */
size_t msmd_modality_split_workspace_bytes(int batch_size,
                                           const int* spatial_shape);

int msmd_modality_split(const int32_t* idx_3d /* [n3,4] */, int n3,
                        const int32_t* idx_2d /* [n2,4] */, int n2,
                        int batch_size, const int* spatial_shape,
                        int32_t* mix3d /* [n3] */, int32_t* mix2d /* [n2] */,
                        int32_t* pair_3d /* [min(n3,n2)] */,
                        int32_t* pair_2d /* [min(n3,n2)] */,
                        int32_t* n_mixed /* [1] */, void* workspace,
                        size_t workspace_bytes, msmd_stream_t stream);
/* The same, plus per-sample row counts in the same pass (what the detector and
 * the fusion stack otherwise obtain from boolean masks with a host round trip
 * each: only_3D / only_2D selections MSMDFusion.py:251-325 callers,
 * pad_missing_batch_id sparse_multimodal_encoder_painting.py:208-225, the
 * per-sample split of fps_NN_fast :349-369).
 * sample_stats[4*batch_size] = rows per sample of [3D unmatched | 3D matched |
 * 2D unmatched | 2D matched]; rows of a sample need not be contiguous. */
int msmd_modality_split_stats(const int32_t* idx_3d, int n3,
                              const int32_t* idx_2d, int n2, int batch_size,
                              const int* spatial_shape, int32_t* mix3d,
                              int32_t* mix2d, int32_t* pair_3d, int32_t* pair_2d,
                              int32_t* n_mixed, int32_t* sample_stats,
                              void* workspace, size_t workspace_bytes,
                              msmd_stream_t stream);

/* a14 with the REFERENCE's float32 keys (`reference_quirks=True` of the detector): key =
 * fl(fl(fl(z) * 1e6 + fl(y) * 1e3) + fl(x)) (MSMDFusion.py:271-272: int tensor * python float
 * promotes to float32), both sets sorted per sample, the r-th occurrence of a key in one list
 * matched with the r-th in the other (type_assign's two-pointer walk, :27-45; ties in row
 * order).  Keys alias for z >= 17 (2^24 < 17e6) and for x >= 1000: voxels that merely share a
 * rounded key are marked mixed -- what a checkpoint trained with the reference has seen.
 * pair_3d / pair_2d: matched rows in key order per sample, samples concatenated (:262-318).
 * reference_offsets != 0: pair rows numbered as the reference does (:288-289,313-314:
 * position in the sample + the PREVIOUS sample's count only; identical to global rows for
 * batch <= 2; needs each set's rows grouped by sample, ascending).  sample_stats (or NULL) as
 * msmd_modality_split_stats.  Grids whose largest key (in the kernel's own float32
 * arithmetic) reaches 2^26, or batch_size > 64: MSMD_ERR_RANGE.  Checked on the device, as the
 * rows are keyed: a row outside the grid or the batch (negative coordinates included), and --
 * with reference_offsets -- a row whose sample id is below its predecessor's; either sets
 * *n_mixed = -1 (every other output is then unspecified) instead of a count. */
size_t msmd_modality_split_float_keys_workspace_bytes(int n3, int n2, int batch_size);
int msmd_modality_split_float_keys(const int32_t* idx_3d, int n3, const int32_t* idx_2d, int n2,
                                   int batch_size, const int* spatial_shape, int32_t* mix3d,
                                   int32_t* mix2d, int32_t* pair_3d, int32_t* pair_2d,
                                   int32_t* n_mixed, int32_t* sample_stats /* or NULL */,
                                   int reference_offsets, void* workspace,
                                   size_t workspace_bytes, msmd_stream_t stream);

/* rows[r] = the r-th i, ascending, with flags[i * stride] == value (at most `capacity` are
 * written; total, if not NULL, receives the count): the row lists `mask.nonzero()` gives the
 * reference (sparse_multimodal_encoder_painting.py:332-340: only_3D / only_2D masks) without
 * the host waiting for the size -- the caller has it from msmd_modality_split_stats.
 * rows[count .. capacity) are set to -1 (torch.nonzero_static's padding). */
size_t msmd_rows_where_workspace_bytes(int n);
int msmd_rows_where_eq(const int32_t* flags, int stride, int n, int value, int64_t* rows,
                       int capacity, int32_t* total, void* workspace, size_t workspace_bytes,
                       msmd_stream_t stream);
/* The same for n_lists (flag vector, value) pairs in one scan: the only-3D and only-2D row lists
 * of all four image scales of a step (host arrays of n_lists pointers / ints).  Per list as
 * msmd_rows_where_eq, the -1 tail included; a list of capacity 0 is skipped.  Every list is
 * checked before the first launch: a call that returns an error has enqueued nothing. */
size_t msmd_rows_where_eq_many_workspace_bytes(const int* lens, int n_lists);
int msmd_rows_where_eq_many(const int32_t* const* flags, const int* strides, const int* lens,
                            const int* values, int64_t* const* rows, const int* capacities,
                            int n_lists, void* workspace, size_t workspace_bytes,
                            msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * a15  GMA-Conv neighbour search helpers
 * replaces: furthest_point_sample_ext.furthest_point_sampling_wrapper
 *           mmdet3d/ops/furthest_point_sample/src/furthest_point_sample_cuda.cu:25-141
 *           ball_query_ext.ball_query_wrapper
 *           mmdet3d/ops/ball_query/src/ball_query_cuda.cu:11-54
 *           and the dense torch.norm/min/index_put_ glue of fps_NN_fast
 *           sparse_multimodal_encoder_painting.py:276-323
 * FPS reproduces the reference block reduction's tie order exactly.
 * ------------------------------------------------------------------------ */
int msmd_furthest_point_sample(const float* xyz /* [b,n,3] */, int b, int n,
                               int m, float* temp /* [b,n] scratch */,
                               int32_t* idx /* [b,m] */, msmd_stream_t stream);

/* Ragged batch: element i owns points [offsets[i], offsets[i+1]) of xyz
 * ([total,3]); idx[i, :] are indices local to the element; n_max = the largest
 * element (host).  One workgroup per element, all elements run concurrently. */
int msmd_furthest_point_sample_ragged(const float* xyz, const int32_t* offsets /* [b+1] device */,
                                      int b, int n_max, int m, float* temp /* [total] */,
                                      int32_t* idx /* [b,m] */, msmd_stream_t stream);

int msmd_ball_query(const float* center_xyz /* [b,m,3] */,
                    const float* xyz /* [b,n,3] */, int b, int n, int m,
                    float min_radius, float max_radius, int nsample,
                    int32_t* idx /* [b,m,nsample] */, msmd_stream_t stream);

/* nearest key per query: out_idx[q] = argmin_k |query_q - key_k| (lowest k on
 * ties) when sqrt(d2) < dist_thresh, else -1.  Integer voxel coordinates.
 * scratch: nq * 8 bytes. */
int msmd_nn_search(const int32_t* query_zyx /* [nq,3] */, int nq,
                   const int32_t* key_zyx /* [nk,3] */, int nk,
                   float dist_thresh, int32_t* out_idx /* [nq] */,
                   void* scratch, msmd_stream_t stream);

/* fps_NN_fast's last step: every query inside the ball of a valid
 * representative inherits that representative's nearest key; when several
 * balls cover a query the highest representative index wins (the order a
 * sequential index_put_ leaves, sparse_multimodal_encoder_painting.py:321). */
int msmd_nn_assign(const int32_t* group_idx /* [m,nsample] ball-query out */,
                   const int32_t* rep_nn /* [m] nearest key or -1 */, int m,
                   int nsample, int nq, int32_t* query_nn /* [nq], -1 init by callee */,
                   int32_t* scratch /* [nq] */, msmd_stream_t stream);

/* The whole chain behind FPS for all samples of a stage in one ragged launch set:
 * nearest key of the representatives (or of the queries themselves) -> ball query ->
 * assignment -> batch offsets -> pad rows.
 * replaces: sparse_multimodal_encoder_painting.py:276-323 (fps_NN_fast behind its FPS call)
 *           as SparseMultiModalEncoderPaint.grouped_sparse_conv composes it per sample
 *           (:349-369), and the -1 rows of the padded only-2D voxels (:208-225)
 * desc (device, int32 [4*b + 2]): query offsets [b+1] | key offsets [b+1] | mode [b] |
 * base [b].  Sample s owns rows [q_off[s], q_off[s+1]) of query_bzyx and
 * [k_off[s], k_off[s+1]) of key_bzyx (both (b,z,y,x) rows, 16-byte aligned; the batch
 * column is skipped).  Modes: SKIP = every row -1; DIRECT = every query searches the
 * keys itself (at most nq_max queries); CLUSTERED = the fps_num representatives
 * fps_idx[s, :] (sample-local rows) search the keys, every query within `radius` of a
 * representative that found a key (only the first max_cluster_samples hits in row order
 * count) inherits it, the highest representative winning.  A valid row is
 * base[s] + the key's sample-local index.  out: int64 [n_query + n_pad], the tail -1.
 * nq_max / nk_max: the largest searching set (fps_num for a CLUSTERED sample) and the
 * largest key set of the batch (host).  Exact for coordinates in [0, 32767] (the
 * caller's contract) and dist_thresh, radius <= 2048 (else MSMD_ERR_UNSUPPORTED): see
 * csrc/gma_nn.hip.  One fill and three kernels. */
#define MSMD_NN_CHAIN_SKIP 0
#define MSMD_NN_CHAIN_DIRECT 1
#define MSMD_NN_CHAIN_CLUSTERED 2
size_t msmd_gma_nn_chain_scratch_bytes(int b, int nq_max, int n_query);
int msmd_gma_nn_chain(const int32_t* query_bzyx /* [n_query,4] */, int n_query,
                      const int32_t* key_bzyx /* [n_key,4] */, int n_key,
                      const int32_t* desc /* [4*b+2] device */, int b,
                      const int32_t* fps_idx /* [b,fps_num] or NULL */, int fps_num,
                      int nq_max, int nk_max, float dist_thresh, float radius,
                      int max_cluster_samples, int n_pad, int64_t* out /* [n_query+n_pad] */,
                      void* scratch, size_t scratch_bytes, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * f3 (training half)  TransFusionHead.loss: target assignment and heat-map loss
 * replaces: iou3d_cuda.boxes_overlap_bev_gpu(boxes_a, boxes_b, ans_overlap)
 *           (mmdet3d/ops/iou3d/src/iou3d.cpp:70-98, kernel iou3d_kernel.cu:36-264) and
 *           its caller BaseInstance3DBoxes.overlaps
 *           (mmdet3d/core/bbox/structures/base_box3d.py:384-438), reached from
 *           HungarianAssigner3D.assign (core/bbox/assigners/hungarian_assigner.py:125)
 * ------------------------------------------------------------------------ */
/* Overlap AREA of rotated BEV rectangles (x1, y1, x2, y2, angle), out[na, nb]. */
int msmd_boxes_overlap_bev_f32(const float* boxes_a /* [na,5] */, int na,
                               const float* boxes_b /* [nb,5] */, int nb,
                               float* out /* [na,nb] */, msmd_stream_t stream);
/* 3-D IoU (mode 0) / IoF over boxes_a (mode 1) of LiDAR boxes
 * (x, y, z_bottom, dx, dy, dz, yaw, ...) for a whole batch: sample s compares its na
 * rows of boxes_a with its first nb_valid[s] rows of boxes_b (nb_valid NULL: all nb);
 * columns past nb_valid[s] are written as 0.  out[batch, na, nb]. */
int msmd_boxes_iou3d_f32(const float* boxes_a /* [batch,na,lda] */, int lda,
                         const float* boxes_b /* [batch,nb,ldb] */, int ldb,
                         const int32_t* nb_valid /* [batch] or NULL */, int batch,
                         int na, int nb, int mode, float* out, msmd_stream_t stream);

/* replaces: the per-box loop gaussian_radius -> draw_heatmap_gaussian of
 *           TransFusionHead.get_targets_single
 *           (mmdet3d/models/dense_heads/transfusion_head.py:1186-1210;
 *           mmdet3d/core/utils/gaussian.py:5-53)
 * heatmap[planes, h, w] (caller zero-fills; plane = sample * classes + class) takes the
 * maximum with exp(-(dx^2 + dy^2) / (2 (d/6)^2)), d = 2 radius + 1, evaluated in double
 * and rounded to float, clipped to the map.  plane < 0 or radius < 0: box skipped. */
int msmd_heatmap_gaussian_f32(const int32_t* plane /* [n] */,
                              const int32_t* center_x /* [n] */,
                              const int32_t* center_y /* [n] */,
                              const int32_t* radius /* [n] */, int n, int planes, int h,
                              int w, float* heatmap, msmd_stream_t stream);

/* replaces: clip_sigmoid (mmdet3d/models/utils/clip_sigmoid.py) + mmdet's
 *           GaussianFocalLoss(alpha=2, gamma=4) as called at transfusion_head.py:1247-1249.
 * p = clamp(sigmoid(logit), clip, 1 - clip);
 * loss_i = -log(p + 1e-12) (1-p)^2 [target == 1] - log(1 - p + 1e-12) p^2 (1-target)^4.
 * sums[0] = sum of loss_i, sums[1] = number of cells with target == 1 (the avg_factor the
 * reference reads back with .item()); grad (optional) = d loss_i / d logit_i.
 * Deterministic: per-block partials in double, summed in block order. */
size_t msmd_gaussian_focal_workspace_bytes(int64_t n);
int msmd_gaussian_focal_f32(const float* logits, const float* target, int64_t n,
                            float clip, float* grad /* [n] or NULL */,
                            float* sums /* [2] */, void* workspace,
                            size_t workspace_bytes, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * n2  iou3d: BEV IoU and rotated / axis-aligned / circle NMS, batched over segments
 * replaces: iou3d_cuda.boxes_iou_bev_gpu  (mmdet3d/ops/iou3d/src/iou3d.cpp:100-126, kernel
 *           iou3d_kernel.cu:244-281)
 *           iou3d_cuda.nms_gpu / nms_normal_gpu  (iou3d.cpp:128-232: mask kernel
 *           iou3d_kernel.cu:283-419, device -> host copy of the mask, host reduction)
 *           circle_nms  (mmdet3d/core/post_processing/box3d_nms.py:141-181, a numba loop
 *           over host copies of the boxes)
 * and their per-task, per-sample call sites CenterHead.get_task_detections
 * (models/dense_heads/centerpoint_head.py:737-852) and TransFusionHead.get_bboxes
 * (transfusion_head.py:1334-1367).
 * ------------------------------------------------------------------------ */
/* IoU of rotated BEV rectangles (x1, y1, x2, y2, angle): overlap / max(sa + sb - overlap,
 * 1e-8), out[na, nb]. */
int msmd_boxes_iou_bev_f32(const float* boxes_a /* [na,5] */, int na,
                           const float* boxes_b /* [nb,5] */, int nb,
                           float* out /* [na,nb] */, msmd_stream_t stream);
/* Greedy NMS of num_segments lists in one call, nothing read back.  Segment s is rows
 * offsets[s] .. offsets[s+1] of boxes (row stride ld floats), already in descending score
 * order; only its first max_segment rows take part (the pre-NMS cut; max_segment <= 16384,
 * else MSMD_ERR_INVALID_ARG before anything is enqueued).  Row i suppresses a later row j when
 *   kind 0 (rotated): iou_bev(i, j) > thresh[s]      columns x1, y1, x2, y2, angle
 *   kind 1 (normal):  iou_normal(i, j) > thresh[s]   columns x1, y1, x2, y2
 *   kind 2 (circle):  dx*dx + dy*dy <= thresh[s]     columns x, y; float32, no contraction
 * NaN follows these expressions as written.  Kinds 0 and 2: every test is false, the box is
 * kept and suppresses nothing.  Kind 1: iou_normal's fmaxf / fminf drop the NaN and its union
 * becomes fmaxf(NaN, 1e-8) = 1e-8, so a NaN box counts as overlapping, as in the reference.
 * keep[s * keep_stride + p] = the p-th kept row of segment s for p < num_keep[s] =
 * min(kept, post_max, keep_stride), -1 after that: the row's position in the segment, or
 * order[offsets[s] + position] when order is given (the caller's sort permutation).
 * workspace: the suppression mask, total_boxes * ceil(max_segment / 64) words.
 * Bitwise reproducible: no atomics on floats, launch sizes depend on the arguments only. */
size_t msmd_nms_workspace_bytes(int total_boxes, int max_segment);
int msmd_nms_batched_f32(int kind, const float* boxes /* [total_boxes, ld] */, int ld,
                         const int32_t* offsets /* [num_segments + 1] */, int num_segments,
                         int total_boxes, int max_segment,
                         const float* thresh /* [num_segments] */, int post_max,
                         const int64_t* order /* [total_boxes] or NULL */,
                         int64_t* keep /* [num_segments, keep_stride] */, int keep_stride,
                         int32_t* num_keep /* [num_segments] */, void* workspace,
                         size_t workspace_bytes, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * p1  Pillar feature net: decoration + Linear + BatchNorm1d + ReLU + max / mean over the slots
 * replaces: PillarFeatureNet.forward  mmdet3d/models/voxel_encoders/pillar_encoder.py:91-150
 *           PFNLayer.forward          mmdet3d/models/voxel_encoders/utils.py:191-227
 * (one PFN layer; the encoder has no gradient to its input).
 * voxels[N, M, C] float32 (the padded table of hard voxelization, never written), num_points[N]
 * (>= 1, may exceed M), coors[N, 4] (batch, z, y, x).  flags: 1 with_cluster_center,
 * 2 with_voxel_center, 4 with_distance, 8 legacy.  Decorated row of slot m (K = C + 3 + 2 + 1
 * channels for the flags set, in this order): raw channels (legacy with voxel centre: channels
 * 0, 1 hold x - cx, y - cy, as the reference's in-place view leaves them), xyz minus
 * (sum over all M slots) / num_points, x - (coors[3] vx + x_offset), y - (coors[2] vy +
 * y_offset), |xyz|; rows with m >= num_points are zero rows (and count in the statistics).
 * Built shapes: K <= 16, U <= 128, M <= 64, C >= 3 (else MSMD_ERR_UNSUPPORTED).  N == 0: ok,
 * nothing is launched.  All sums: fp64 per workgroup, workgroups added in order (no atomics). */
size_t msmd_pillar_workspace_bytes(int num_pillars, int max_points, int out_channels);
/* moments[0..16) = column sums s of the decorated rows, moments[16 + 16 i + j] = G[i][j] =
 * sum f_i f_j over all N * M rows (entries past K are 0): the batch statistics of W f follow
 * as mean = W s / n, var = w^T (G / n - s s^T / n^2) w. */
int msmd_pillar_moments_f32(const float* voxels, const int32_t* num_points,
                            const int32_t* coors, int num_pillars, int max_points,
                            int num_features, int flags, float vx, float vy, float x_offset,
                            float y_offset, double* moments /* [272] */, void* workspace,
                            size_t workspace_bytes, msmd_stream_t stream);
/* out[n, u] = max over the M slots (mode_max) or (sum over the M slots) / num_points of
 * relu(scale[u] * (weight[u] . f) + shift[u]); argmax[n, u] (mode_max): the smallest slot
 * attaining the maximum. */
int msmd_pillar_pfn_fwd_f32(const float* voxels, const int32_t* num_points,
                            const int32_t* coors, int num_pillars, int max_points,
                            int num_features, int flags, float vx, float vy, float x_offset,
                            float y_offset, const float* weight /* [U, K] */,
                            const float* scale /* [U] */, const float* shift /* [U] */,
                            int out_channels, int mode_max, float* out /* [N, U] */,
                            uint8_t* argmax /* [N, U] or NULL */, msmd_stream_t stream);
/* g = grad_out [y > 0] at the argmax slot (mode_max) or grad_out / num_points [y > 0] at every
 * slot; sums[u * 17 + k] = sum g f_k (k < 16), sums[u * 17 + 16] = sum g. */
int msmd_pillar_pfn_bwd_f32(const float* voxels, const int32_t* num_points,
                            const int32_t* coors, int num_pillars, int max_points,
                            int num_features, int flags, float vx, float vy, float x_offset,
                            float y_offset, const float* weight, const float* scale,
                            const float* shift, int out_channels, int mode_max,
                            const float* grad_out /* [N, U] */, const uint8_t* argmax,
                            double* sums /* [U, 17] */, void* workspace,
                            size_t workspace_bytes, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * p2  HardVFE with one or two VFELayers: decoration + (Linear + BatchNorm1d + ReLU + max over
 *     the slots) twice, the second layer on [h1; max h1] (csrc/hard_vfe.hip)
 * replaces: HardVFE.forward   mmdet3d/models/voxel_encoders/voxel_encoder.py (HardVFE)
 *           VFELayer.forward  mmdet3d/models/voxel_encoders/utils.py:34-106
 * (the encoder has no gradient to its input).
 * voxels / num_points / coors as for p1.  flags: 1 with_cluster_center, 2 with_voxel_center.
 * Decorated row of slot m (K = C + 3 + 3): raw channels, xyz minus (sum over all M slots) /
 * num_points, x - (coors[3] vx + x_offset), y - (coors[2] vy + y_offset), z - (coors[1] vz +
 * z_offset); rows with m >= num_points are zero rows and count in both layers' statistics.
 * Per row: y1 = W1 f, h1 = relu(scale1 y1 + shift1), m1 = max over the slots of h1,
 * y2 = W2 [h1; m1], out = max over the slots of relu(scale2 y2 + shift2).  u2 == 0: one layer,
 * out = m1.  Built shapes: K <= 16, u1, u2 <= 64, M <= 64, C >= 3 (else MSMD_ERR_UNSUPPORTED).
 * N == 0: ok, nothing is launched.  All sums: fp64, added in a fixed order (no atomics). */
size_t msmd_hard_vfe_workspace_bytes(int num_voxels, int max_points);
/* The moments of the decorated rows, laid out as msmd_pillar_moments_f32's. */
int msmd_hard_vfe_moments_f32(const float* voxels, const int32_t* num_points,
                              const int32_t* coors, int num_voxels, int max_points,
                              int num_features, int flags, float vx, float vy, float vz,
                              float x_offset, float y_offset, float z_offset,
                              double* moments /* [272] */, void* workspace,
                              size_t workspace_bytes, msmd_stream_t stream);
/* Layer 2's batch statistics: pivot[u] = y2 of (voxel 0, slot 0), sums[2 u] = sum y2,
 * sums[2 u + 1] = sum (y2 - pivot)^2 over all N * M rows (u < 64; entries past u2 are 0). */
int msmd_hard_vfe_stats_f32(const float* voxels, const int32_t* num_points,
                            const int32_t* coors, int num_voxels, int max_points,
                            int num_features, int flags, float vx, float vy, float vz,
                            float x_offset, float y_offset, float z_offset,
                            const float* w1 /* [u1, K] */, const float* scale1,
                            const float* shift1, int u1, const float* w2 /* [u2, 2 u1] */,
                            int u2, float* pivot /* [64] */, double* sums /* [128] */,
                            void* workspace, size_t workspace_bytes, msmd_stream_t stream);
/* out[N, U], argmax[N, U] (the smallest slot attaining the maximum of the last layer) and,
 * with two layers, ymax[N, u2]: y2 at that slot.  U = u2, or u1 when u2 == 0. */
int msmd_hard_vfe_fwd_f32(const float* voxels, const int32_t* num_points, const int32_t* coors,
                          int num_voxels, int max_points, int num_features, int flags, float vx,
                          float vy, float vz, float x_offset, float y_offset, float z_offset,
                          const float* w1, const float* scale1, const float* shift1, int u1,
                          const float* w2, const float* scale2, const float* shift2, int u2,
                          float* out, uint8_t* argmax, float* ymax /* or NULL (u2 == 0) */,
                          msmd_stream_t stream);
/* g2[N, U]: the gradient at the last BatchNorm's output, placed at (n, argmax[n, u]).  Two
 * layers: dy2 = scale2 g2 - (dp + dq y2) per row (dp, dq [u2]: the batch statistics' terms,
 * zeros in eval mode); sums[u * 128 + j] = dW2[u][j] for the h1 columns j < u1 and
 * sums[u * 128 + 64 + j] for the m1 columns, then from sums[8192]: [u1 * 17 + k] = sum g1 f_k
 * (k < 16) and [u1 * 17 + 16] = sum g1, g1 the gradient at the first BatchNorm's output.
 * One layer: only the [u1][17] block, at sums[0]. */
int msmd_hard_vfe_bwd_f32(const float* voxels, const int32_t* num_points, const int32_t* coors,
                          int num_voxels, int max_points, int num_features, int flags, float vx,
                          float vy, float vz, float x_offset, float y_offset, float z_offset,
                          const float* w1, const float* scale1, const float* shift1, int u1,
                          const float* w2, const float* scale2, int u2, const float* g2,
                          const uint8_t* argmax, const float* dp, const float* dq,
                          double* sums /* [9280] or [u1 = 64][17] */, void* workspace,
                          size_t workspace_bytes, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * n1  PointNet++ op family (csrc/pointnet.hip)
 * replaces: gather_points_ext.gather_points_wrapper / gather_points_grad_wrapper
 *           mmdet3d/ops/gather_points/src/gather_points_cuda.cu:9-94
 *           group_points_ext.forward / backward
 *           mmdet3d/ops/group_points/src/group_points_cuda.cu:12-101
 *           interpolate_ext.three_nn_wrapper
 *           mmdet3d/ops/interpolate/src/three_nn_cuda.cu:11-89
 *           interpolate_ext.three_interpolate_wrapper / three_interpolate_grad_wrapper
 *           mmdet3d/ops/interpolate/src/three_interpolate_cuda.cu:11-108
 *           knn_ext.knn_wrapper  mmdet3d/ops/knn/src/knn_cuda.cu:26-268
 *           furthest_point_sample_ext.furthest_point_sampling_with_dist_wrapper
 *           mmdet3d/ops/furthest_point_sample/src/furthest_point_sample_cuda.cu:214-400
 * Features are (B, C, N) channel-major, xyz (B, N, 3), indices int32.  An index outside
 * [0, N) reads as 0 in the forward ops and is left out of the backward (the reference reads
 * and adds out of bounds).  B <= 65535, C <= 4 * 65535.
 * ------------------------------------------------------------------------ */
/* out[b, c, j] = features[b, c, idx[b, j]] */
int msmd_gather_points_f32(const float* features /* [b,c,n] */, const int32_t* idx /* [b,npoint] */,
                           int b, int c, int n, int npoint, float* out /* [b,c,npoint] */,
                           msmd_stream_t stream);
/* out[b, c, p, s] = features[b, c, idx[b, p, s]]; npoint * nsample < 2^31 */
int msmd_group_points_f32(const float* features /* [b,c,n] */,
                          const int32_t* idx /* [b,npoint,nsample] */, int b, int c, int n,
                          int npoint, int nsample, float* out /* [b,c,npoint,nsample] */,
                          msmd_stream_t stream);
/* The three nearest known points of every unknown point: float32
 * d = (dx*dx + dy*dy) + dz*dz, strict <, lowest index on ties; dist2 is the SQUARED distance
 * (three_nn.py takes the root).  m < 3: the missing entries are index 0, distance +inf. */
int msmd_three_nn_f32(const float* unknown /* [b,n,3] */, const float* known /* [b,m,3] */,
                      int b, int n, int m, float* dist2 /* [b,n,3] */, int32_t* idx /* [b,n,3] */,
                      msmd_stream_t stream);
/* out[b, c, j] = (w0 f[i0] + w1 f[i1]) + w2 f[i2], i = idx[b, j, :], w = weight[b, j, :] */
int msmd_three_interpolate_f32(const float* features /* [b,c,m] */,
                               const int32_t* idx /* [b,n,3] */,
                               const float* weight /* [b,n,3] */, int b, int c, int m, int n,
                               float* out /* [b,c,n] */, msmd_stream_t stream);
/* idx[b, j, p] = the j-th nearest of the n points to centre p, 0-based, ordered by
 * (d2, index) ascending (the order the reference's stable insertion sort leaves); d2 as in
 * three_nn -- the reference's chained ssd += tmp*tmp may be contracted by its compiler, so d2
 * itself is not claimed bit-equal.  No [n x npoint] matrix is written.  Built for
 * 1 <= k <= 128: k > 128 returns MSMD_ERR_UNSUPPORTED, k < 1 or k > n MSMD_ERR_INVALID_ARG. */
int msmd_knn_f32(const float* xyz /* [b,n,3] */, const float* center_xyz /* [b,npoint,3] */,
                 int b, int n, int npoint, int k, int64_t* idx /* [b,k,npoint] */,
                 msmd_stream_t stream);
/* Furthest point sampling on a distance matrix: idx[b, 0] = 0, the running minimum is taken
 * against row `old`; the reference block reduction's tie order, as msmd_furthest_point_sample.
 * n < 2^21. */
int msmd_furthest_point_sample_with_dist(const float* dist /* [b,n,n] */, int b, int n, int m,
                                         float* temp /* [b,n] scratch */,
                                         int32_t* idx /* [b,m] */, msmd_stream_t stream);
/* By-source inverse of an index tensor, for the backward of the three ops above: the
 * destinations j in [0, m) of batch element b whose idx[b, j] == s are
 * dest[src_start[b*n + s] .. src_start[b*n + s + 1]), in ASCENDING j (stable radix sort; no
 * dependence on atomic arrival order).  b*m and b*n < 2^31. */
size_t msmd_point_inverse_index_workspace_bytes(int b, int m);
int msmd_point_inverse_index(const int32_t* idx /* [b,m] */, int b, int n, int m,
                             int32_t* src_start /* [b*n+1] */, int32_t* dest /* [b*m] */,
                             void* workspace, size_t workspace_bytes, msmd_stream_t stream);
/* grad_in[b, c, s] (+)= sum over the source's destinations j, in list order, float32 with a
 * Kahan compensation term (y = term - comp; sum = acc + y; comp = (sum - acc) - y), of
 * weight[b, j] * grad_out[b, c, j / dest_per_out] (weight NULL: 1).  dest_per_out = 1 for
 * gather / group, 3 for three_interpolate (destinations are its (point, slot) pairs);
 * grad_out is [b, c, m / dest_per_out].  No float atomics: bitwise reproducible. */
int msmd_point_scatter_bwd_f32(const float* grad_out, const float* weight /* [b,m] or NULL */,
                               const int32_t* src_start, const int32_t* dest, int b, int c,
                               int n, int m, int dest_per_out, int accumulate,
                               float* grad_in /* [b,c,n] */, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * n3  Anchor3DHead: matrix-free target assignment and the sigmoid focal loss (csrc/anchor.hip)
 * replaces: MaxIoUAssigner.assign / assign_wrt_overlaps (mmdet 2.x
 *           mmdet/core/bbox/assigners/max_iou_assigner.py) over BboxOverlapsNearest3D
 *           (mmdet3d/core/bbox/iou_calculators/iou3d_calculator.py:94-150 -> mmdet
 *           bbox_overlaps): a [num_gt, num_anchors] matrix per sample and per assigner,
 *           reduced along both axes, then a Python loop over the ground truths
 *           AnchorTrainMixin.anchor_target_3d_single / anchor_target_single_assigner
 *           (mmdet3d/models/dense_heads/train_mixins.py:101-314), get_direction_target
 *           (:317-346), DeltaXYZWLHRBBoxCoder.encode
 *           (mmdet3d/core/bbox/coders/delta_xyzwhlr_bbox_coder.py:20-54)
 *           mmdet FocalLoss(use_sigmoid=True) as Anchor3DHead.loss_single calls it
 *           (mmdet3d/models/dense_heads/anchor3d_head.py:217-218)
 * A segment is one (sample, assigner group): output rows anchor_offsets[s] ..
 * anchor_offsets[s+1] (a HOST array, ascending from 0: the anchors' layout follows from the
 * feature-map sizes) and the ground truths gt_index[gt_offsets[s] .. gt_offsets[s+1]) (DEVICE
 * arrays: under assign_per_class they depend on the labels; gt_index NULL: the entries are the
 * rows themselves).  Output row r uses anchor row r % anchor_rows, so the samples of a batch
 * share one copy of the anchors.  At most msmd_anchor_max_segments() segments per call
 * (MSMD_ERR_RANGE beyond).  Nothing is read back; bad arguments, offsets that do not ascend
 * included, are refused before anything is enqueued.
 * ------------------------------------------------------------------------ */
int msmd_anchor_max_segments(void);
/* ground-truth boxes staged in LDS at a time (a test crosses it on purpose) */
int msmd_anchor_gt_chunk(void);
/* mmdet 2.x MaxIoUAssigner with match_low_quality, gt_max_assign_all, ignore_iof_thr < 0 and a
 * scalar neg_iou_thr, on axis-aligned BEV boxes (x1, y1, x2, y2):
 *   iou = overlap / max(area_gt + area_anchor - overlap, 1e-6), wh = clamp(rb - lt, 0), float32
 *   1. every anchor starts at -1 (ignored)
 *   2. 0 <= max < neg_iou_thr[s]: 0 (negative)
 *   3. max >= pos_iou_thr[s]: argmax + 1, ties to the LOWEST ground-truth index
 *   4. for ground truths i in ascending order whose best IoU over the segment's anchors is
 *      >= min_pos_iou[s]: every anchor whose IoU with i EQUALS that best value gets i + 1 (a
 *      later i overrides an earlier one and rule 3)
 * with i local to the segment's list.  A segment without ground truths: every anchor 0,
 * max_overlaps 0.  num_pos[s] = anchors of segment s with assigned_gt > 0.  An entry of
 * gt_index outside [0, num_gt) is never assigned.  Bitwise reproducible: the only atomics are
 * integer ones (a max on the bits of the non-negative IoU, a count). */
size_t msmd_anchor_assign_workspace_bytes(int gt_entries);
int msmd_anchor_assign_f32(const float* anchor_bev /* [anchor_rows,4] */, int anchor_rows,
                           const int32_t* anchor_offsets /* HOST [num_segments+1] */,
                           int num_segments, const float* gt_bev /* [num_gt,4] */, int num_gt,
                           const int32_t* gt_index /* [gt_entries] or NULL */,
                           const int32_t* gt_offsets /* [num_segments+1] */, int gt_entries,
                           const float* pos_iou_thr /* HOST [num_segments] */,
                           const float* neg_iou_thr /* HOST [num_segments] */,
                           const float* min_pos_iou /* HOST [num_segments] */,
                           int32_t* assigned_gt /* [rows] */, float* max_overlaps /* [rows] */,
                           int32_t* num_pos /* [num_segments] */, void* workspace,
                           size_t workspace_bytes, msmd_stream_t stream);
/* From assigned_gt, for input row r of sample r / anchor_rows, written at row
 * dest[r % anchor_rows] of that sample (dest NULL: in place; a permutation of [0, anchor_rows),
 * the reference's [..., size, rotation] interleaving when the segments are the anchor sizes):
 *   positive: bbox_targets = DeltaXYZWLHRBBoxCoder.encode(anchor, gt) (columns past 7:
 *     gt - anchor), bbox_weights = 1, dir_targets = floor(limit_period(rot_gt - dir_offset, 0,
 *     2 pi) / pi) clamped to {0, 1} with rot_gt = (gt_r - anchor_r) + anchor_r, dir_weights = 1,
 *     labels = gt_labels[gt], label_weights = pos_weight > 0 ? pos_weight : 1
 *   otherwise: labels = num_classes, zeros; label_weights = 1 for a negative, 0 for an ignored
 *     anchor.
 * 7 <= code_size <= 16 (else MSMD_ERR_UNSUPPORTED). */
int msmd_anchor_targets_f32(const int32_t* assigned_gt /* [rows] */,
                            const float* anchors /* [anchor_rows,code_size] */, int anchor_rows,
                            int code_size,
                            const int32_t* anchor_offsets /* HOST [num_segments+1] */,
                            int num_segments, const float* gt_boxes /* [num_gt,code_size] */,
                            const int64_t* gt_labels /* [num_gt] */, int num_gt,
                            const int32_t* gt_index /* [gt_entries] or NULL */,
                            const int32_t* gt_offsets /* [num_segments+1] */, int gt_entries,
                            const int32_t* dest /* [anchor_rows] or NULL */, int num_classes,
                            float pos_weight, float dir_offset, int64_t* labels /* [rows] */,
                            float* label_weights /* [rows] */,
                            float* bbox_targets /* [rows,code_size] */,
                            float* bbox_weights /* [rows,code_size] */,
                            int64_t* dir_targets /* [rows] */, float* dir_weights /* [rows] */,
                            msmd_stream_t stream);
/* sum[0] = sum over i, c of weights[i] * BCE_with_logits(x, t) * (alpha t + (1 - alpha)(1 - t))
 * * pt^gamma with t = [labels[i] == c] (background: labels[i] == num_classes), pt = (1 - p) t +
 * p (1 - t), p = sigmoid(x); grad (optional) = d of that sum / d logit.  The avg_factor division
 * stays with the caller.  Deterministic: per-block partials in double, summed in block order. */
size_t msmd_sigmoid_focal_workspace_bytes(int64_t n, int num_classes);
int msmd_sigmoid_focal_f32(const float* logits /* [n,num_classes] */,
                           const int64_t* labels /* [n] */, const float* weights /* [n] */,
                           int64_t n, int num_classes, float gamma, float alpha,
                           float* grad /* [n,num_classes] or NULL */, float* sum /* [1] */,
                           void* workspace, size_t workspace_bytes, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * n4  VoteNet: matrix-free Chamfer distance, vote targets, points per box (csrc/vote.hip) and
 *     the class-aware axis-aligned 3-D NMS (csrc/nms.hip)
 * replaces: chamfer_distance  (mmdet3d/models/losses/chamfer_distance.py:50-55: two
 *           [B, N, M, 3] expansions, a [B, N, M] matrix, two torch.min) and autograd through it
 *           VoteHead.get_targets_single  (models/dense_heads/vote_head.py:472-501: a Python loop
 *           over ground truths with a torch.nonzero per box and per slot)
 *           VoteHead.multiclass_nms_single  (vote_head.py:617-625: an [N, T] inclusion table,
 *           only summed over N)
 *           aligned_3d_nms  (mmdet3d/core/post_processing/box3d_nms.py:91-138: a Python while
 *           loop with one host read per kept box)
 * Nothing here uses float atomics; every result is bitwise reproducible; nothing is read back.
 * ------------------------------------------------------------------------ */
/* Chamfer forward.  c(s, t) = (cx + cy) + cz in float32, every operation rounded on its own,
 * with the per-coordinate criterion on d = s - t: mode 0 (l2) d * d, 1 (l1) |d|, 2 (smooth_l1,
 * beta 1) (0.5 |d|) |d| for |d| < 1 else |d| - 0.5.
 *   d1[b, n] = min over m of c(src[b, n], dst[b, m]), i1[b, n] = its index; d2 / i2 likewise
 *   over n for every dst[b, m].
 * The minimum is torch.min's over a dimension: ties go to the lowest index, a NaN distance is
 * the minimum and the first NaN is reported.  channels != 3, n == 0 or m == 0 are refused
 * (MSMD_ERR_INVALID_ARG).  No buffer of size N x M exists; no workspace. */
int msmd_chamfer_fwd_f32(const float* src /* [batch,n,3] */, const float* dst /* [batch,m,3] */,
                         int batch, int n, int m, int channels, int mode,
                         float* d1 /* [batch,n] */, int64_t* i1 /* [batch,n] */,
                         float* d2 /* [batch,m] */, int64_t* i2 /* [batch,m] */,
                         msmd_stream_t stream);
/* Chamfer backward for upstream g1 [batch, n] (of d1) and g2 [batch, m] (of d2), with
 * c'(d) = 2 d (l2), sign(d) with sign(0) = 0 (l1), d for |d| < 1 else sign(d) (smooth_l1):
 *   grad_src[b, n] = g1[b, n] c'(src_n - dst_{i1[n]}), then + g2[b, m] c'(src_n - dst_m) for
 *   every m with i2[b, m] == n in ascending m;
 *   grad_dst[b, m] = g2[b, m] c'(dst_m - src_{i2[m]}), then + g1[b, n] c'(dst_m - src_n) for
 *   every n with i1[b, n] == m in ascending n.
 * The differences are float32; the products and the running sum (a left fold in that order) are
 * double, rounded to float32 once at the end.
 * One lane per output point scans the other side's index array; no atomics, no sort.  An index
 * outside its set contributes nothing.  Either gradient may be NULL (not computed). */
int msmd_chamfer_bwd_f32(const float* src /* [batch,n,3] */, const float* dst /* [batch,m,3] */,
                         const float* g1 /* [batch,n] */, const float* g2 /* [batch,m] */,
                         const int64_t* i1 /* [batch,n] */, const int64_t* i2 /* [batch,m] */,
                         int batch, int n, int m, int channels, int mode,
                         float* grad_src /* [batch,n,3] or NULL */,
                         float* grad_dst /* [batch,m,3] or NULL */, msmd_stream_t stream);
/* Vote targets of the box form (bbox_coder.with_rot).  Sample s owns point rows
 * point_offsets[s] .. point_offsets[s+1] and box rows box_offsets[s] .. box_offsets[s+1]; boxes
 * are in the frame of msmd_points_in_boxes_f32 (x, y, z bottom, w, l, h, rz) and tested with
 * its predicate; centers are their gravity centres.  With k = the boxes of the point's sample
 * that hold it, in ascending box order, and vote(box) = center - point[:3]:
 *   vote_mask = (k > 0); slot 0 = vote(first); slot 1 = vote(second) if k >= 2 else
 *   vote(first); slot 2 = vote(LAST) if k >= 3 else vote(first) -- the reference clamps its
 *   slot counter at 2, so every later box overwrites slot 2; all zero when k == 0.
 * Every row of both outputs that the offsets cover is written.  gt_per_seed must be 3.
 * max_points (a bound on a sample's points known to the host) only sizes the grid. */
int msmd_vote_targets_f32(const float* points /* [total_points,ld] */, int ld,
                          const int32_t* point_offsets /* [num_samples+1] */,
                          const float* boxes /* [total_boxes,7] */,
                          const float* centers /* [total_boxes,3] */,
                          const int32_t* box_offsets /* [num_samples+1] */, int num_samples,
                          int total_points, int total_boxes, int max_points, int gt_per_seed,
                          float* vote_targets /* [total_points,9] */,
                          int64_t* vote_mask /* [total_points] */, msmd_stream_t stream);
/* count[b, t] = the points of sample b inside box t (the predicate of
 * msmd_points_in_boxes_f32), summed in integers; no [M, T] table. */
int msmd_points_in_boxes_count_f32(const float* boxes /* [B,T,7] */,
                                   const float* pts /* [B,M,ld] */, int ld, int batch_size,
                                   int num_boxes, int num_points, int32_t* count /* [B,T] */,
                                   msmd_stream_t stream);
/* Class-aware axis-aligned 3-D NMS over segments; rows (x1, y1, z1, x2, y2, z2, class) in
 * descending score order.  offsets, max_segment, thresh, post_max, order, keep, keep_stride,
 * num_keep and the workspace are those of msmd_nms_batched_f32.  A kept row i suppresses a
 * later row j when !((iou * same) <= thresh[s]) with inter = the product of the three
 * fmaxf(0, min(hi) - max(lo)) extents, iou = inter / (vol_i + vol_j - inter) and
 * same = (class_i == class_j) ? 1 : 0, all float32 and rounded one operation at a time.  That
 * is the reference's `score_sorted[iou <= thresh]` as written: a NaN IoU (0 / 0, two disjoint
 * zero-volume boxes) suppresses, and across classes, because NaN * 0 is NaN. */
size_t msmd_nms_aligned3d_workspace_bytes(int total_boxes, int max_segment);
int msmd_nms_aligned3d_f32(const float* boxes /* [total_boxes, ld >= 7] */, int ld,
                           const int32_t* offsets /* [num_segments + 1] */, int num_segments,
                           int total_boxes, int max_segment,
                           const float* thresh /* [num_segments] */, int post_max,
                           const int64_t* order /* [total_boxes] or NULL */,
                           int64_t* keep /* [num_segments, keep_stride] */, int keep_stride,
                           int32_t* num_keep /* [num_segments] */, void* workspace,
                           size_t workspace_bytes, msmd_stream_t stream);

/* ---- 3DSSD (COVERAGE n5) ------------------------------------------------------------------
 * Candidate targets of SSD3DHead for the whole batch in one launch: what
 * SSD3DHead.get_targets_single and _assign_targets_by_points_inside compute per sample
 * (mmdet3d/models/dense_heads/ssd_3d_head.py:307-437, 545-572: about sixty tensor ops, two
 * points_in_boxes_gpu launches, a gt[valid] compaction and a host read per sample).
 * Sample s owns candidate rows s * num_candidates .. and box rows box_offsets[s] ..
 * box_offsets[s+1] of gt_boxes / vote_boxes / labels / box_table / dir_class.  Both box tables are
 * in the frame of msmd_points_in_boxes_f32 and tested with its predicate; a row whose label is
 * -1 does not exist.  box_table row (table_width must be 33): gravity centre (3), half sizes
 * (3), direction residual (1), sin and cos of -yaw (2), the 8 x 3 corners (24), all computed by
 * the caller.  seeds: sample s starts at seeds + s * seed_stride floats, 3 per candidate.
 * Per candidate, with `a` = the first existing box (ascending) holding the aggregated point, or
 * the sample's LAST existing box when none does (inside = a box holds it):
 *   center_targets / size_targets / dir_class_targets / dir_res_targets / mask_targets / corners
 *     = copies from box a (centre absolute);
 *   positive = inside && |p - (centre + (0, 0, half_z))| < pos_distance_thr; negative = !inside;
 *   centerness[k] = c * (k == label ? 1 : 0), c = clamp(cbrt(clamp(l * w * h, 0)), 0, 1) with the
 *     min / max ratios of the six clamped face distances of the point turned by -yaw, float32,
 *     one rounding per operation, NaN propagated as torch.clamp / min / max do;
 *   vote_mask / vote_targets: the same rule with vote_boxes on the seed point,
 *     vote_targets = centre(box) - seed.
 * A sample without an existing row gets zeros everywhere and negative = 1.  Masks are bytes
 * (0 / 1).  Every output row is written; nothing is read back; the launch shape depends on the
 * arguments only. */
int msmd_ssd3d_gt_chunk(void); /* boxes per LDS chunk */
int msmd_ssd3d_targets_f32(const float* aggregated /* [batch,num_candidates,3] */,
                           const float* seeds, int64_t seed_stride,
                           const float* gt_boxes /* [total_boxes,7] */,
                           const float* vote_boxes /* [total_boxes,7] */,
                           const int64_t* labels /* [total_boxes] */,
                           const int32_t* box_offsets /* [batch+1] */,
                           const float* box_table /* [total_boxes,table_width] */,
                           int table_width, const int64_t* dir_class /* [total_boxes] */,
                           int batch, int num_candidates, int total_boxes, int num_classes,
                           float pos_distance_thr, float* vote_targets /* [batch,n,3] */,
                           float* center_targets /* [batch,n,3] */,
                           float* size_targets /* [batch,n,3] */,
                           int64_t* dir_class_targets /* [batch,n] */,
                           float* dir_res_targets /* [batch,n] */,
                           int64_t* mask_targets /* [batch,n] */,
                           float* centerness /* [batch,n,num_classes] */,
                           float* corners /* [batch,n,8,3] */, uint8_t* vote_mask /* [batch,n] */,
                           uint8_t* positive_mask /* [batch,n] */,
                           uint8_t* negative_mask /* [batch,n] */, msmd_stream_t stream);
/* mmcv.ops.nms's pair test (mmcv 1.x nms_cuda_kernel.cuh, offset 0) over segments, the kernel
 * behind batched_nms (ssd_3d_head.py:512-515).  Rows (x1, y1, x2, y2), already shifted by
 * class * (max coordinate + 1) as batched_nms does, in descending score order.  A kept row i
 * suppresses a later row j when inter > thresh[s] * (area_i + area_j - inter), inter = the
 * product of the two fmaxf(min(hi) - max(lo), 0) extents, float32, one rounding per operation:
 * no division and no floor on the union.  Everything else is msmd_nms_batched_f32's; the
 * workspace is msmd_nms_workspace_bytes. */
int msmd_nms_mmcv_f32(const float* boxes /* [total_boxes, ld >= 4] */, int ld,
                      const int32_t* offsets /* [num_segments + 1] */, int num_segments,
                      int total_boxes, int max_segment, const float* thresh /* [num_segments] */,
                      int post_max, const int64_t* order /* [total_boxes] or NULL */,
                      int64_t* keep /* [num_segments, keep_stride] */, int keep_stride,
                      int32_t* num_keep /* [num_segments] */, void* workspace,
                      size_t workspace_bytes, msmd_stream_t stream);

/* ---- FreeAnchor3DHead (COVERAGE n6, csrc/free_anchor.hip) -----------------------------------
 * The training loss of mmdet3d/models/dense_heads/free_anchor3d_head.py:72-242 without its two
 * [num_gt, num_anchors] IoU matrices per sample.  Boxes are nearest-BEV boxes (x1, y1, x2, y2)
 * and the IoU is msmd_anchor_assign_f32's.  No [G, A] array exists in global memory, nothing is
 * read back, there are no float atomics: every result is bitwise reproducible. */
/* replaces: DeltaXYZWLHRBBoxCoder.decode (mmdet3d/core/bbox/coders/delta_xyzwhlr_bbox_coder.py:
 * 56-91) followed by LiDARInstance3DBoxes.nearest_bev (core/bbox/structures/lidar_box3d.py:93-111)
 * as free_anchor3d_head.py:112-116 applies them to every anchor of every sample.  Row r of
 * deltas uses anchor r % num_anchors; only x, y, w, l and the rotation are decoded.
 * code_size < 7 is refused (MSMD_ERR_INVALID_ARG). */
int msmd_decode_nearest_bev_f32(const float* anchors /* [num_anchors,code_size] */,
                                int num_anchors, int code_size,
                                const float* deltas /* [batch*num_anchors,code_size] */,
                                int batch, float* pred_bev /* [batch*num_anchors,4] */,
                                msmd_stream_t stream);
/* replaces: free_anchor3d_head.py:115-161 (the [G, A] IoU matrix of ground truths x decoded
 * predictions, its row maximum, and sparse_coo_tensor / sparse.sum / nonzero per sample).
 * Sample b owns prediction rows b * num_anchors .. and ground truths gt_offsets[b] ..
 * gt_offsets[b+1] (a DEVICE array).  With t1 = bbox_thr and t2[i] = max over the sample's
 * anchors of IoU(gt i, pred j):
 *   box_prob[j, c] = max over the sample's i with gt_labels[i] == c of
 *                    clamp((IoU(i, j) - t1) / (max(t2[i], t1) - t1), 0, 1), else 0,
 * float32 with a true division.  A ground truth with t2 <= t1 contributes nothing (the
 * reference gives 0 there as well, except NaN where an IoU equals t1 bit for bit).  A pair with
 * a NaN coordinate in either box has a NaN IoU (tested explicitly: fmaxf / fminf would drop the
 * NaN): it contributes nothing and stays out of t2, so a NaN prediction keeps a zero row and a
 * NaN ground truth is ignored (the reference's row maximum would make t2 NaN instead).  A label
 * outside [0, num_classes) is skipped.  Every row is written. */
size_t msmd_free_anchor_box_prob_workspace_bytes(int num_gt);
int msmd_free_anchor_box_prob_f32(const float* pred_bev /* [batch*num_anchors,4] */, int batch,
                                  int num_anchors, const float* gt_bev /* [num_gt,4] */,
                                  const int64_t* gt_labels /* [num_gt] */, int num_gt,
                                  const int32_t* gt_offsets /* [batch+1] */, int num_classes,
                                  float bbox_thr, float* box_prob /* [batch*num_anchors,C] */,
                                  void* workspace, size_t workspace_bytes, msmd_stream_t stream);
/* replaces: free_anchor3d_head.py:167-173 (the [G, A] matrix of ground truths x anchors and
 * torch.topk over each row), for all ground truths of a batch at once: the anchors are shared by
 * the samples.  Row i of matched holds the k anchors with the largest IoU to ground truth i:
 * a larger IoU first, among equal IoUs the LOWER anchor index first, NaN as the largest value
 * (torch.topk's order) -- and a pair with a NaN coordinate in either box has a NaN IoU, as the
 * same expression has in torch, so a NaN ground truth gets the first k anchors by index and a
 * NaN anchor is in every bag; the row itself is written in ascending anchor index.  Exact: a radix
 * select on the IoU's 32 bits, then an ordered compaction.  k < 1, k >
 * msmd_free_anchor_max_topk() and k > num_anchors (where the reference's topk raises too) are
 * refused with MSMD_ERR_INVALID_ARG. */
int msmd_free_anchor_max_topk(void);
size_t msmd_free_anchor_topk_workspace_bytes(int num_anchors, int num_gt);
int msmd_free_anchor_topk(const float* anchor_bev /* [num_anchors,4] */, int num_anchors,
                          const float* gt_bev /* [num_gt,4] */, int num_gt, int k,
                          int32_t* matched /* [num_gt,k] */, void* workspace,
                          size_t workspace_bytes, msmd_stream_t stream);
/* replaces: FreeAnchor3DHead.negative_bag_loss (free_anchor3d_head.py:266-282) and autograd
 * through it.  sum[0] = sum over all entries of (1 - alpha) p^gamma BCE(p, 0) with
 * p = clamp(sigmoid(logit) (1 - box_prob), 0, 1) and torch's binary_cross_entropy (the log
 * clamped at -100, backward p / max((1 - p) p, 1e-12)); grad (optional) = d sum / d logits.
 * Deterministic: per-block partials in double, summed in block order.  gamma < 1 is refused
 * (MSMD_ERR_INVALID_ARG): the gradient at p = 0 is unbounded there. */
size_t msmd_free_anchor_negative_workspace_bytes(int64_t n, int num_classes);
int msmd_free_anchor_negative_f32(const float* logits /* [n,num_classes] */,
                                  const float* box_prob /* [n,num_classes] */, int64_t n,
                                  int num_classes, float gamma, float alpha,
                                  float* grad /* [n,num_classes] or NULL */, float* sum /* [1] */,
                                  void* workspace, size_t workspace_bytes, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * p3  PointFusion's multi-level image sampler, forward + backward (csrc/point_sample.hip)
 * replaces: point_sample()  mmdet3d/models/fusion_layers/point_fusion.py:10-95
 *           PointFusion.obtain_mlvl_feats / sample_single  point_fusion.py:239-306 (the loop
 *           over samples and levels, one cat per sample and one per batch)
 *           apply_3d_transformation  mmdet3d/models/fusion_layers/coord_transform.py:7-90
 *           F.grid_sample(mode='bilinear', padding_mode='zeros') and its backward to the map
 *           (float atomics in torch)
 * One call covers all samples and all levels.  points [N, >= 3] are the concatenated clouds
 * (row stride point_stride floats), sample b owns rows sample_start[b] .. sample_start[b+1]
 * (the array is given twice: on the DEVICE for the kernels, on the HOST for validation -- 0
 * first, N last, non-decreasing; an empty sample is fine).  Level l is a channels-last map
 * [B, H_l, W_l, C_l] and fills columns offset_l .. offset_l + C_l of the [N, sum C_l] output
 * row; the offsets tile the row in level order.
 * Per point: q = m [x y z 1]; z = max(q.z, 1e-5); px = q.x / z * scale_x - crop_x (py likewise);
 * flip != 0: px = img_w - px; per level grid_sample's bilinear unnormalisation of
 * (px / pad_w * 2 - 1, py / pad_h * 2 - 1) for either align_corners, zero padding (a corner
 * outside the map contributes nothing; bounds are tested in floating point, coordinates of
 * 1e30 are fine), corners accumulated nw, ne, sw, se.  float32, no contraction.
 * Deviation: a point whose pixel coordinate is not finite reads zeros in every level and takes
 * no part in the backward (torch's result there depends on the backend's float -> int
 * conversion).  Every output element is written.  N == 0: ok, nothing is launched.
 * Total cells (B * sum H_l W_l) and N * L * 4 must be below 2^31 (MSMD_ERR_UNSUPPORTED).
 * ------------------------------------------------------------------------ */
#define MSMD_POINT_SAMPLE_MAX_LEVELS 8
typedef struct msmd_point_sample_params { /* one per sample, DEVICE array */
  float m[12];                            /* 3x4, row-major: detector frame -> homogeneous pixel */
  float scale_x, scale_y, crop_x, crop_y;
  float flip;                             /* 0 or 1 */
  float img_w;                            /* before padding: the flip axis */
  float pad_h, pad_w;
} msmd_point_sample_params;
typedef struct msmd_point_sample_level { /* HOST array, copied into the launch by value */
  const float* map;                      /* DEVICE [B, h, w, c]; the gradient buffer in bwd */
  int32_t h, w, c;
  int32_t offset;                        /* first column of the level in the output row */
} msmd_point_sample_level;
int msmd_point_sample_fwd_f32(const float* points, int point_stride, int num_points,
                              const int32_t* sample_start /* [batch+1] */,
                              const int32_t* sample_start_host /* host [batch+1] */, int batch,
                              const msmd_point_sample_params* params /* [batch] */,
                              const msmd_point_sample_level* levels /* host [num_levels] */,
                              int num_levels, int align_corners,
                              float* out /* [num_points, sum c] */, msmd_stream_t stream);
/* The index of the backward; it depends on the points and the map shapes only.  A contribution
 * is (point p, level l, corner k), id t = (p L + l) 4 + k: cell[t] = cell_base[l] +
 * (b H_l + y) W_l + x with cell_base the running sum of B H_l W_l, or -1 for a corner outside
 * the map or a point that is not finite; weight[t] its bilinear weight (0 where cell is -1).
 * start [cells + 1] / order [N L 4]: the by-cell inverse, every list in ASCENDING t (built on
 * msmd_point_inverse_index's stable radix sort).  piece_start [cells + 1]: the exclusive scan of
 * the number of msmd_point_sample_bwd_chunk()-sized pieces of the lists LONGER than one chunk.
 * levels[].map is not read (NULL is fine here and in the workspace queries). */
int msmd_point_sample_bwd_chunk(void);
size_t msmd_point_sample_index_workspace_bytes(const msmd_point_sample_level* levels,
                                               int num_levels, int batch, int num_points);
int msmd_point_sample_index(const float* points, int point_stride, int num_points,
                            const int32_t* sample_start, const int32_t* sample_start_host,
                            int batch, const msmd_point_sample_params* params,
                            const msmd_point_sample_level* levels, int num_levels,
                            int align_corners, int32_t* cell /* [N L 4] */,
                            float* weight /* [N L 4] */, int32_t* start /* [cells+1] */,
                            int32_t* order /* [N L 4] */, int32_t* piece_start /* [cells+1] */,
                            void* workspace, size_t workspace_bytes, msmd_stream_t stream);
/* grad_levels[l].map [B, H_l, W_l, C_l] (written, every cell; an empty list gives exact zeros) =
 * sum over the cell's list, in list order, of weight[t] * grad_out[p, offset_l .. + C_l].
 * float32; a list longer than one chunk is cut into chunks summed by separate waves into the
 * workspace, and the partial sums are added in chunk order: no float atomics, the result depends
 * on the index alone (bitwise reproducible).  There is no gradient to the points. */
size_t msmd_point_sample_bwd_workspace_bytes(const msmd_point_sample_level* levels,
                                             int num_levels, int batch, int num_points);
int msmd_point_sample_bwd_f32(const float* grad_out /* [num_points, sum c] */, int num_points,
                              int batch, const msmd_point_sample_level* grad_levels,
                              int num_levels, const float* weight, const int32_t* start,
                              const int32_t* order, const int32_t* piece_start, void* workspace,
                              size_t workspace_bytes, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * p4  ImVoteNet's VoteFusion for the whole batch in one launch (csrc/vote_fusion.hip)
 * replaces: VoteFusion.forward  mmdet3d/models/fusion_layers/vote_fusion.py:40-212 (the loop
 *           over samples, the [seed_num, bbox_num, 5 + num_classes] tensors, about sixty
 *           launches per sample and the topk over the box axis)
 *           apply_3d_transformation ('DEPTH', both directions), coord_2d_transform,
 *           bbox_2d_transform  mmdet3d/models/fusion_layers/coord_transform.py:7-214
 *           Coord3DMode.convert_point (DEPTH <-> CAM with Rt)  core/bbox/structures/
 *           coord_3d_mode.py:181-257; points_cam2img  core/bbox/structures/utils.py:114-144
 * seeds [batch, num_seeds, 3] in the detector's depth frame; boxes [total_boxes, 6] = (l, t, r,
 * b, conf, class) in the rescaled image frame, sample s owning rows box_offsets[s] ..
 * box_offsets[s+1] (given twice: on the DEVICE for the kernel, on the HOST for validation -- 0
 * first, total_boxes last, non-decreasing); imgs [batch, 3, pad_h, pad_w] (read only).
 * Per seed: cam = m_cam [x y z 1]; (u, v) = rint((K cam).xy / (K cam).z - 1), half to even.
 * Each box is un-rescaled with bbox_2d_transform(ori2new=False)'s float32 operations in its
 * order (flip, minus crop, divide by scale).  in_box = l < u < r && t < v < b (strict); score =
 * float(in_box) + conf.  The max_imvote largest scores are kept in descending order, EQUAL SCORES
 * TO THE LOWER BOX INDEX; a list shorter than max_imvote is filled with score-0 pairs.  Slot k of
 * seed s is column k * num_seeds + s.  For the chosen boxes: rows 0-1 xz, rows 2-4 ray_angle
 * (vote_fusion.py:110-150, the offset lifted by m_vote, which includes the forward flow's
 * translation as the reference does), rows 5 .. 5 + num_classes conf at the class row, all
 * times float(in_box); mask = floor(score) != 0.  Rows 5 + num_classes .. + 3: the image at
 * rint(coord_2d_transform(uv, ori2new=True)) divided by 255, the same in every slot of the
 * seed.  An empty box list gives zero cue rows, mask 1 in slot 0 and 0 in the others.
 * Deviations: a pixel outside img_h x img_w (or the padded image) or not finite gives a zero
 * texture cue and is not read; a class outside [0, num_classes) gives no semantic cue; the
 * image is never written.  Every output element is written, nothing is read back, no atomics.
 * max_imvote < 1 or > msmd_vote_fusion_max_k(), num_classes < 1 and host offsets that do not
 * start at 0 / end at total_boxes / decrease are refused (MSMD_ERR_INVALID_ARG).
 * ------------------------------------------------------------------------ */
typedef struct msmd_vote_fusion_params { /* one per sample, DEVICE array */
  float m_cam[12];  /* 3x4, row-major: detector depth frame -> camera frame */
  float k[9];       /* calib K, row-major */
  float m_vote[12]; /* 3x4, row-major: camera-frame offset -> detector depth frame */
  float scale_x, scale_y, crop_x, crop_y;
  float flip;         /* 0 or 1 */
  float img_h, img_w; /* img_shape, before padding */
  float fx;           /* K[0][0], used for both image axes as in the reference */
} msmd_vote_fusion_params;
int msmd_vote_fusion_max_k(void); /* largest max_imvote of the fused path */
int msmd_vote_fusion_f32(const float* seeds /* [batch,num_seeds,3] */, int batch, int num_seeds,
                         const float* boxes /* [total_boxes,6] */, int total_boxes,
                         const int32_t* box_offsets /* [batch+1] */,
                         const int32_t* box_offsets_host /* host [batch+1] */,
                         const float* imgs /* [batch,3,pad_h,pad_w] */, int pad_h, int pad_w,
                         const msmd_vote_fusion_params* params /* [batch] */, int num_classes,
                         int max_imvote,
                         float* feat /* [batch,5+num_classes+3,max_imvote*num_seeds] */,
                         uint8_t* mask /* [batch,max_imvote*num_seeds] */, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * f3-img  TransFusionHead's image stage (csrc/img_fusion.hip)
 * replaces: the double loop over samples and views of TransFusionHead.forward_single
 *           mmdet3d/models/dense_heads/transfusion_head.py:930-1004 -- the projection of the
 *           queries and their box corners (:943-979), the on-image test and the host read of its
 *           count (:981-987), centres, radius and sigma (:990-995), the [n, H W] Gaussian mask,
 *           its threshold and logarithm (:996-999) and the masked attention they feed (:1003,
 *           multi_head_attention_forward :286-504); LiDARInstance3DBoxes.corners
 *           core/bbox/structures/lidar_box3d.py:46-84
 *
 * msmd_img_query_geometry_f32: one launch for the batch, the views looped inside.  pos3d
 * [batch, 3, P] = (x, y, height) of the queries; boxes [batch, P, 7] = (x, y, z_bottom, dx, dy,
 * dz, yaw); params [batch * V] in the layout of msmd_point_sample_params, m = lidar2img[view]
 * times the reversed 3-D flow (or lidar2img[view] alone where the reference skips the flow).
 * Per (sample, view, query), float32 without contraction: the eight corners in the reference's
 * order; q = m [p 1], z = max(q.z, 1e-5), px = q.x / z * scale_x - crop_x (py likewise), flip:
 * px = img_w - px; on = 0 < px < pad_w && 0 < py < pad_h (strict); pos = (px, py) / osf; centre =
 * trunc(pos) (0 where not on); radius = ceil(|max - min of the corner pixels| / osf / 2),
 * INT32_MAX where that is not below 2^31 or any corner pixel is NaN; sigma = (2 radius + 1) / 6.
 * count [batch, V] = members of the view, valid = count > 1 (:985); winner [batch, P] = the
 * highest valid view that sees the query or -1; mask = winner >= 0 (on_the_image_mask);
 * win_pos / win_centre / win_sigma: the winner's values, 0 without one.  Every output element is
 * written, nothing is read back.  P <= msmd_img_query_geometry_max_queries() (1024), V <=
 * msmd_img_query_geometry_max_views() (8), else MSMD_ERR_UNSUPPORTED.
 *
 * msmd_gauss_attn_fwd_f32: q [batch * P, C] (projected, unscaled), k, v [batch * V, h * w, C]
 * (projected), view [batch * P] (the row's view or -1), centre [batch * P, 2] (x, y), sigma
 * [batch * P].  Per (row, head), d = C / heads, key j at cell (jx, jy) = (j % w, j / w):
 *   arg_j = -((cx - jx)^2 + (cy - jy)^2) / (2 sigma^2)            (float32)
 *   window = { j : expf(arg_j) >= FLT_EPSILON }
 *   out = sum_window D_j softmax_window(q.k_j / sqrt(d) + arg_j) v_j,  lse = log sum exp
 * Only the disc's bounding box, clipped to the map, is visited; the softmax is online.  A row
 * with view -1 (or >= V) or an empty window gives out = 0, lse = 0.  Dropout 0 <= p < 1 on the
 * weights: D_j = 0 where mix(seed, row, head, j) < floor(p 2^32), else 1 / (1 - p); p = 0: D = 1.
 *   fmix(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
 *   mix = fmix(fmix((fmix(lo(seed) ^ row * 0x9E3779B1) + head * 0x85EBCA77) ^ hi(seed))
 *              ^ j * 0xC2B2AE3D)                                   (all uint32, wrapping)
 * msmd_gauss_attn_bwd_f32: grad_q [batch * P, C], grad_k, grad_v [batch * V, h * w, C] (every
 * element written), delta [batch * P, heads] (scratch: grad_out . out).  The mask is
 * regenerated.  dQ is query-stationary; dK / dV key-stationary: a thread per key walks the
 * sample's rows in ascending order, msmd_gauss_attn_row_chunk() rows per LDS round,
 * msmd_gauss_attn_key_tile() keys per block.  No atomics; bitwise reproducible.
 * Built: C / heads of 8, 16, 32 with C <= 256 (msmd_gauss_attn_supported), V <= 8; anything
 * else MSMD_ERR_UNSUPPORTED.  h, w >= 1.
 * ------------------------------------------------------------------------ */
int msmd_img_query_geometry_max_queries(void);
int msmd_img_query_geometry_max_views(void);
int msmd_img_query_geometry_f32(const float* pos3d /* [batch,3,P] */,
                                const float* boxes /* [batch,P,7] */,
                                const msmd_point_sample_params* params /* [batch*V] */, int batch,
                                int num_queries, int num_views, float out_size_factor_img,
                                uint8_t* on /* [batch,V,P] */, float* pos /* [batch,V,P,2] */,
                                int32_t* centre /* [batch,V,P,2] */,
                                int32_t* radius /* [batch,V,P] */, float* sigma /* [batch,V,P] */,
                                int32_t* count /* [batch,V] */, uint8_t* valid /* [batch,V] */,
                                int32_t* winner /* [batch,P] */, uint8_t* mask /* [batch,P] */,
                                float* win_pos /* [batch,P,2] */,
                                int32_t* win_centre /* [batch,P,2] */,
                                float* win_sigma /* [batch,P] */, msmd_stream_t stream);
int msmd_gauss_attn_supported(int channels, int heads);
int msmd_gauss_attn_key_tile(void);
int msmd_gauss_attn_row_chunk(void);
int msmd_gauss_attn_fwd_f32(const float* q, const float* k, const float* v, const int32_t* view,
                            const int32_t* centre, const float* sigma, int batch, int num_queries,
                            int num_views, int h, int w, int channels, int heads, float dropout,
                            uint64_t seed, float* out /* [batch*P,C] */,
                            float* lse /* [batch*P,heads] */, msmd_stream_t stream);
int msmd_gauss_attn_bwd_f32(const float* q, const float* k, const float* v, const float* out,
                            const float* grad_out, const float* lse, const int32_t* view,
                            const int32_t* centre, const float* sigma, int batch, int num_queries,
                            int num_views, int h, int w, int channels, int heads, float dropout,
                            uint64_t seed, float* grad_q, float* grad_k, float* grad_v,
                            float* delta /* [batch*P,heads] */, msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * n7  H3DNet primitive targets (csrc/primitive.hip)
 * replaces: PrimitiveHead.get_targets_single and its helpers
 *           mmdet3d/models/roi_heads/mask_heads/primitive_head.py:327-601 (the loop over the
 *           instances of a sample, with its nonzero, unique and ~14 host reads per instance),
 *           match_point2line :676-715, match_point2plane :717-733, point2line_dist :657-674,
 *           _assign_primitive_line_targets :803-866, _assign_primitive_surface_targets
 *           :868-950, _get_plane_fomulation :952-967, check_horizon / check_dist :631-655
 *
 * Sample s owns point rows point_offsets[s] .. point_offsets[s+1] and box rows
 * box_offsets[s] .. box_offsets[s+1] (device int32 arrays, as msmd_vote_targets_f32 takes
 * them).  Boxes are their eight corners in DepthBoxes.corners order.
 *
 * msmd_primitive_index (mode independent; the three heads of a step share one): a point is
 * foreground when sem != num_classes; the instances of a sample are the distinct instance
 * labels of its foreground points in ascending order, rank = position in that order
 * (torch.unique).  The index holds, per (sample, rank), the number of points, the lowest
 * foreground point (its sem is the instance's class: pts_semantic_mask[indices][0]) and the
 * instance's points in ascending point order.  DEVIATION: labels outside [0, label_bound) take
 * no part (the reference accepts any label); label_bound <= msmd_primitive_max_labels() (1024).
 * max_points and max_instances are host-known bounds that only size grids.
 *
 * msmd_primitive_targets_f32: mode 0 = 'z' (num_dims 2), 1 = 'xy' (num_dims 1), 2 = 'line'
 * (num_dims 0).  One workgroup per (sample, instance) sweeps the instance's list three times in
 * steps of msmd_primitive_point_chunk() entries: minima, then counts / moments / sums, then
 * decisions and writes.  Per instance, all float32 and rounded one operation at a time:
 *   box = corners[rank] -- the RANK, not the label: the reference indexes with its enumerate
 *     counter (:376-383).  DEVIATION: an instance whose rank is not below the sample's box count
 *     (the reference raises IndexError) gets no targets.
 *   planes (n, d): lower (0, 0, 1, -corners[7].z); upper (0, 0, 1, -mean z of corners 1, 2, 5,
 *     6); left = cross(c2 - c3, c3 - c0) through c0, divided by its norm; right: that normal,
 *     d = -mean(n . c) over corners 4, 5, 7, 6; front = cross(c0 - c4, c4 - c5) through c5;
 *     back: that normal over corners 3, 2, 7, 6.
 *   DEVIATION: where the reference raises NotImplementedError (check_horizon, check_dist, a
 *     normal's z not below lower_thresh -- none can fire for a finite box rotated about z, the
 *     normals' z components are exactly 0) the instance gets no targets; a degenerate or NaN box
 *     fails these comparisons and so gets none either.
 *   plane matching: dist = |p . n + d|; selected = |dist - min over the instance| < dist_thresh;
 *     the minimum is torch.min's (a NaN distance is the minimum, then nothing is selected).
 *   surfaces (modes z, xy): on when count(selected) > num_point and the unbiased variance of
 *     dist[selected] < var_thresh; the variance is accumulated in double, pivoted on the
 *     minimum, from the float32 distances.
 *   lines (mode line) are matched among the plane's selected points: with_yaw, point2line_dist
 *     in its own form sqrt(|a2p|^2 - length^2) < line_thresh (a negative radicand is NaN and
 *     selects nothing); else |x - xmin|, |x - xmax|, |y - ymin|, |y - ymax| < line_thresh.  A
 *     line is on when count > num_point_line.
 *   centres and sizes: every branch of the two _assign_* helpers (both yaw forms, center_axises
 *     [1,1,0,0] and [2,2], the left / right calls on point2line_matching[2:]).  Means over
 *     selected points are double sums in a fixed order over the instance's list, rounded to
 *     float32 once.
 *   write order: line: 4 bottom, 4 top, 2 left, 2 right; z: bottom, top; xy: left, right, front,
 *     back.  A later primitive overwrites point_offset / point_sem of a point an earlier one
 *     wrote, point_mask is the OR: each lane evaluates its own point in that order.  No atomics
 *     on outputs, no write races, bitwise reproducible.
 * point_mask [total_points], point_offset [total_points, 3], point_sem [total_points, 3 +
 * num_dims + 1] (centre, sizes, class as float): every row the offsets cover is written, rows
 * the reference leaves untouched as zeros.  Nothing is read back.
 * Null pointers, negative counts, label_bound outside 1 .. 1024, an unknown mode, num_dims not
 * matching the mode and a too-small index return MSMD_ERR_INVALID_ARG.
 * ------------------------------------------------------------------------ */
int msmd_primitive_max_labels(void);  /* largest label_bound */
int msmd_primitive_point_chunk(void); /* list entries per sweep step */
size_t msmd_primitive_index_workspace_bytes(int num_samples, int total_points, int label_bound);
int msmd_primitive_index(const int64_t* pts_semantic_mask /* [total_points] */,
                         const int64_t* pts_instance_mask /* [total_points] */,
                         const int32_t* point_offsets /* [num_samples+1] */, int num_samples,
                         int total_points, int max_points, int num_classes, int label_bound,
                         int max_instances, void* index, size_t index_bytes,
                         msmd_stream_t stream);
int msmd_primitive_targets_f32(const float* points /* [total_points,ld] */, int ld,
                               const int64_t* pts_semantic_mask /* [total_points] */,
                               const int32_t* point_offsets /* [num_samples+1] */,
                               const float* corners /* [total_boxes,8,3] */,
                               const int32_t* box_offsets /* [num_samples+1] */, int num_samples,
                               int total_points, int total_boxes, int max_points, int max_boxes,
                               int with_yaw, int mode, int num_dims, float dist_thresh,
                               float var_thresh, float lower_thresh, int num_point,
                               int num_point_line, float line_thresh, int label_bound,
                               const void* index, size_t index_bytes,
                               float* point_mask /* [total_points] */,
                               float* point_offset /* [total_points,3] */,
                               float* point_sem /* [total_points,3+num_dims+1] */,
                               msmd_stream_t stream);

/* ------------------------------------------------------------------------ *
 * n8  H3DNet second stage: box cue centres and fused cue targets (csrc/h3d.hip)
 * replaces: DepthInstance3DBoxes.get_surface_line_center
 *           mmdet3d/core/bbox/structures/depth_box3d.py:277-330 (about thirty small ops)
 *           H3DBboxHead.get_targets_single under multi_apply
 *           mmdet3d/models/roi_heads/bbox_heads/h3d_bbox_head.py:761-932 (per sample: three
 *           chamfer_distance calls that expand [1, N, M, 3], two get_surface_line_center
 *           calls, about sixty small ops, seven of them boolean-mask assignments)
 *
 * Boxes are rows (cx, cy, cz, sx, sy, sz, yaw) with the GRAVITY centre.
 *
 * msmd_box_cue_centers_f32: surface row b * 6 + f (f: +z, -z, +y, -y, +x, -x) and line row
 * b * 12 + l (the order of depth_box3d.py:305-308) = centre[b] + Rz(-yaw[r % n]) (offset *
 * size[b] / 2), r the row's own number and n the number of boxes of the call.  r % n, not b, is
 * the reference's: it repeats its n rotation matrices 6 (12) times against box-major rows.
 * With every yaw 0 the two readings agree.  Double arithmetic on the float32 inputs, one
 * rounding per coordinate.  msmd_box_cue_centers_bwd_f32 gives the gradient of the seven
 * columns: one lane per box gathers its 18 rows (centre, sizes) and the 6 + 12 rows
 * r = b (mod n) it rotates (yaw), in ascending order, without atomics.
 *
 * msmd_h3d_cue_targets_f32: every output of H3DBboxHead.get_targets for the batch in one
 * launch, nothing read back.  Sample b has gt_counts[b] boxes in gt_boxes[b] (device int32; a
 * count outside 1 .. max_gt is clipped into it -- an empty sample is the reference's single
 * zero box with label 0, which is what zero padding holds).  Per (sample, proposal p, cue):
 *   the nearest ground-truth centre to aggregated[b, p] (squared L2, torch.min's rule: lowest
 *   index on ties, the first NaN wins -- the selection of msmd_chamfer_fwd_f32, bit for bit);
 *   that box's cue centre as above with n = the sample's count -> obj_surface_line_center;
 *   the nearest predicted surface (cues 0-5) or line (cues 6-17) centre to it, same rule;
 *   the argmax of that primitive's class scores (lowest index among maxima, NaN is a maximum);
 *   d_center = sqrt(d2 + 1e-6) and likewise d_prim (cue centre to selected primitive) and
 *   d_own (the proposal's own cue centre, surface_obj / line_obj, to the selected primitive);
 *   label = d_own < label_*_threshold && d_prim < mask_*_threshold;
 *   sem = label && argmax == gt_labels[nearest];  near = d_center < near_threshold;
 *   cues_objectness_label = label, cues_sem_label = sem (both BEFORE the reference's in-place
 *   multiplication), cues_matching_label = label * near, cues_mask = proposal_objectness_mask =
 *   near || d_center > far_threshold, proposal_objectness_label = near, cues_match_mask = any
 *   of the proposal's 18 unmultiplied labels.
 * Cue rows are the reference's: surface f * P + p, line 6 P + l * P + p; surface_obj is
 * [B, 6 P, 3] and line_obj [B, 12 P, 3] in that order (the two halves of the [B, 18 P, 3]
 * cue centres the head's forward leaves).  No atomics, one writer per element, bitwise
 * reproducible.  No workspace.
 * Null pointers, a negative size, max_gt / num_surface / num_line / num_classes < 1 (with work
 * to do) and a NaN threshold return MSMD_ERR_INVALID_ARG; num_classes > 4096 or an element
 * count that does not fit 31 bits MSMD_ERR_RANGE.  batch == 0 or num_proposals == 0: ok.
 *
 * Deviation of the Python head that calls these (h3d_head.H3DBboxHead.loss): the reference
 * unpacks 13 rpn targets (:348-351) where VoteHead.get_targets returns 14, so its
 * H3DNet.forward_train raises as written; the head here takes 13 or 14 and drops
 * assigned_center_targets, the eighth, when 14 arrive.
 * ------------------------------------------------------------------------ */
int msmd_h3d_cue_gt_chunk(void);   /* ground-truth centres per LDS chunk */
int msmd_h3d_cue_pred_chunk(void); /* predicted centres per LDS chunk */
int msmd_h3d_cue_proposals(void);  /* proposals per workgroup */
int msmd_box_cue_centers_f32(const float* boxes /* [n,7] */, int n,
                             float* surface /* [n*6,3] */, float* line /* [n*12,3] */,
                             msmd_stream_t stream);
int msmd_box_cue_centers_bwd_f32(const float* boxes /* [n,7] */, int n,
                                 const float* grad_surface /* [n*6,3] */,
                                 const float* grad_line /* [n*12,3] */,
                                 float* grad_boxes /* [n,7] */, msmd_stream_t stream);
int msmd_h3d_cue_targets_f32(const float* aggregated /* [B,P,3] */,
                             const float* gt_boxes /* [B,G,7] */,
                             const int32_t* gt_counts /* [B] */,
                             const int64_t* gt_labels /* [B,G] */,
                             const float* surface_pred /* [B,Ns,3] */,
                             const float* line_pred /* [B,Nl,3] */,
                             const float* surface_sem /* [B,Ns,C] */,
                             const float* line_sem /* [B,Nl,C] */,
                             const float* surface_obj /* [B,6P,3] */,
                             const float* line_obj /* [B,12P,3] */, int batch,
                             int num_proposals, int max_gt, int num_surface, int num_line,
                             int num_classes, float near_threshold, float far_threshold,
                             float label_surface_threshold, float label_line_threshold,
                             float mask_surface_threshold, float mask_line_threshold,
                             int64_t* cues_objectness_label /* [B,18P] */,
                             int64_t* cues_sem_label /* [B,18P] */,
                             int64_t* cues_matching_label /* [B,18P] */,
                             float* cues_mask /* [B,18P] */,
                             int64_t* proposal_objectness_label /* [B,P] */,
                             float* proposal_objectness_mask /* [B,P] */,
                             float* cues_match_mask /* [B,P] */,
                             float* obj_surface_line_center /* [B,18P,3] */,
                             msmd_stream_t stream);

/* ---- Part-A2, first stage (COVERAGE n9) ---------------------------------------------------
 * Semantic and part targets of PointwiseSemanticHead for the whole batch in one launch: what
 * get_targets / get_targets_single compute per sample
 * (mmdet3d/models/roi_heads/mask_heads/pointwise_semantic_head.py:78-157: two
 * points_in_boxes_gpu launches, then per ground-truth box a boolean mask, a host read, a
 * gather, an einsum rotation and a masked write, and a torch.cat per batch).
 * Row i is voxel centre voxel_centers[i] of sample batch_ids[i] (coors[:, 0]); rows may be in
 * any order.  Sample b has gt_counts[b] boxes (device int32, clipped into 0 .. max_gt) in
 * gt_boxes[b] and enlarged_boxes[b], both in the frame of msmd_points_in_boxes_f32 (LiDAR,
 * bottom centre) and tested with its predicate; enlarged_boxes is the caller's
 * LiDARInstance3DBoxes.enlarged_box(extra_width) of gt_boxes.  labels is int64 (labels_int64
 * = 1) or int32 (0).  Per row, k = the first box of its sample holding the centre, or none:
 *   seg_targets  = labels[k] verbatim, num_classes when there is no k; -1 when (a k exists) !=
 *                  (any enlarged box holds the centre);
 *   part_targets = max(rot_z(-yaw[k]) (centre - bottom_centre[k]) / dims[k] + (0.5, 0.5, 0), 0)
 *                  in the row-vector convention of rotation_3d_in_axis(axis=2), float32, one
 *                  rounding per operation, NaN kept as torch.clamp keeps it; 0 when there is
 *                  no k.
 * A row whose batch id is outside [0, batch) gets seg = -1 and part = 0 (the reference drops
 * such rows).  Output is in input row order, which is the reference's torch.cat whenever the
 * ids do not decrease.  A NaN centre or box fails the predicate.  Every output element is
 * written; no atomics, no workspace, nothing read back; the launch shape depends on num_rows
 * only.  Null pointers (with work to do), a negative size and num_classes < 1 return
 * MSMD_ERR_INVALID_ARG before anything is enqueued; batch * max_gt * 7 >= 2^31 MSMD_ERR_RANGE.
 * num_rows == 0, batch == 0 and max_gt == 0 are valid. */
int msmd_semantic_gt_chunk(void); /* boxes per LDS chunk */
int msmd_semantic_targets_f32(const float* voxel_centers /* [num_rows,3] */,
                              const int32_t* batch_ids /* [num_rows] */,
                              const float* gt_boxes /* [batch,max_gt,7] */,
                              const float* enlarged_boxes /* [batch,max_gt,7] */,
                              const void* labels /* [batch,max_gt] */, int labels_int64,
                              const int32_t* gt_counts /* [batch] */, int num_rows, int batch,
                              int max_gt, int num_classes, int64_t* seg_targets /* [num_rows] */,
                              float* part_targets /* [num_rows,3] */, msmd_stream_t stream);

/* ---- Part-A2, second stage (COVERAGE n10) -------------------------------------------------
 * PartAggregationROIHead._assign_and_sample (mmdet3d/models/roi_heads/
 * part_aggregation_roi_head.py:222-294) and PartA2BboxHead.get_targets (bbox_heads/
 * parta2_bbox_head.py:356-460) for every sample of the batch, nothing read back.
 *
 * Both calls take the batch as flat lists: proposals [P, 7] and gt_boxes [G, 7] (LiDAR rows x, y,
 * z_bottom, dx, dy, dz, yaw) with HOST offset tables of batch + 1 ascending entries from 0
 * (list lengths are tensor shapes; the tables travel by value in the kernel arguments).
 *
 * msmd_roi_assign3d_f32: class-aware MaxIoUAssigner (mmdet core/bbox/assigners/
 * max_iou_assigner.py, gt_max_assign_all = match_low_quality = True, no ignore set) over the
 * 3-D IoU of BboxOverlaps3D(coordinate='lidar'); the pair value is the one
 * msmd_boxes_iou3d_f32 writes, bit for bit.  single = 0: an IoU is formed only where
 * proposal_labels[p] == gt_labels[g] and that label lies in [0, num_classes); thresholds are
 * per class (host arrays of num_classes floats).  single = 1: no label test, thresholds are
 * element 0, proposal_labels may be null.  Per proposal:
 *   gt_inds       -1 ignored, 0 background, i + 1 with i the index in the sample's ground-truth
 *                 list (the merged convention of :263-275); ties of the arg-max go to the lowest
 *                 index, of rule 4 (low-quality matches) to the highest, as in the reference;
 *   max_overlaps  the largest IoU over the ground truths of the proposal's class, 0 when the
 *                 class has none or the label is outside [0, num_classes);
 *   labels        gt_labels of the assigned ground truth, else -1.
 * A row with a NaN coordinate takes part in no pair: a NaN proposal gets gt_inds = -1 and
 * max_overlaps = NaN, and no other row depends on it.  The per-ground-truth maximum is an
 * integer atomicMax on the bits of the non-negative IoU, so the result is bitwise reproducible.
 * Three enqueued operations (memset, two launches).  batch > msmd_roi_assign_max_samples() or
 * num_classes > msmd_roi_assign_max_classes(): MSMD_ERR_RANGE.
 *
 * msmd_roi_sample_targets_f32: IoUNegPiecewiseSampler.sample (core/bbox/samplers/
 * iou_neg_piecewise_sampler.py, add_gt_as_proposals = False, return_iou = True) followed by
 * _get_target_single, one workgroup per sample, no atomics, one launch.  random_choice(gallery,
 * n) is "the n entries with the smallest keys (one float32 per proposal), ties to the lower
 * proposal index".  Quotas as the reference computes them: int(n * fraction) is (int)((double)
 * n * fraction); extend_num, the last-piece rule, neg_pos_ub (< 0: none) and both early returns
 * included.  Piece k holds max_overlaps in [thrs[k+1], thrs[k]) (the last: [0, thrs[k])); the
 * bounds must not ascend, the fractions of all but the last piece lie in [0, 1] and sum to at
 * most 1, and num_expected_pos <= num (else MSMD_ERR_INVALID_ARG): that keeps a sample's rows
 * within `num`.
 * Outputs are padded to `num` rows per sample: row r of sample s at s * num + r, positives in
 * ascending proposal order, then negatives in ascending order, then zero rows (sampled_inds
 * -1).  Per row: rois (s, box), ious, label (1 above cls_pos_thr, 0 below cls_neg_thr, else
 * iou * 2 - 0.5 in two roundings), label_weights (label >= 0), reg_mask / bbox_weights (1 for
 * positives), pos_gt_bboxes and bbox_targets (positives; zero otherwise): the canonical
 * transform of :428-448 and DeltaXYZWLHRBBoxCoder.encode against the zero-centred, zero-yaw
 * RoI, float32 as written.  counts[s] = (positives, negatives).  Every output element is
 * written.  More than msmd_roi_sample_max_proposals() proposals in a sample, num >
 * msmd_roi_sample_max_num() or num_pieces > msmd_roi_sample_max_pieces(): MSMD_ERR_RANGE. */
int msmd_roi_assign_max_samples(void);
int msmd_roi_assign_max_classes(void);
int msmd_roi_assign_gt_chunk(void); /* ground truths per LDS chunk */
int msmd_roi_sample_max_proposals(void);
int msmd_roi_sample_max_num(void);
int msmd_roi_sample_max_pieces(void);
size_t msmd_roi_assign3d_workspace_bytes(int num_gt);
int msmd_roi_assign3d_f32(const float* proposals /* [P,7] */,
                          const int64_t* proposal_labels /* [P] */,
                          const int32_t* proposal_offsets /* host [batch+1] */,
                          const float* gt_boxes /* [G,7] */, const int64_t* gt_labels /* [G] */,
                          const int32_t* gt_offsets /* host [batch+1] */, int batch,
                          int num_classes, int single, const float* pos_iou_thr /* host */,
                          const float* neg_iou_thr /* host */,
                          const float* min_pos_iou /* host */, int32_t* gt_inds /* [P] */,
                          float* max_overlaps /* [P] */, int64_t* labels /* [P] */,
                          void* workspace, size_t workspace_bytes, msmd_stream_t stream);
int msmd_roi_sample_targets_f32(const float* proposals /* [P,7] */,
                                const int32_t* proposal_offsets /* host [batch+1] */,
                                const int32_t* gt_inds /* [P] */,
                                const float* max_overlaps /* [P] */, const float* keys /* [P] */,
                                const float* gt_boxes /* [G,7] */,
                                const int32_t* gt_offsets /* host [batch+1] */, int batch,
                                int num, int num_expected_pos, double neg_pos_ub,
                                int num_pieces, const double* neg_piece_fractions /* host */,
                                const float* neg_iou_piece_thrs /* host */, float cls_pos_thr,
                                float cls_neg_thr, float* rois /* [batch,num,8] */,
                                float* ious /* [batch,num] */, float* label /* [batch,num] */,
                                float* label_weights /* [batch,num] */,
                                int64_t* reg_mask /* [batch,num] */,
                                float* bbox_weights /* [batch,num] */,
                                float* pos_gt_bboxes /* [batch,num,7] */,
                                float* bbox_targets /* [batch,num,7] */,
                                int32_t* sampled_inds /* [batch,num] */,
                                int32_t* counts /* [batch,2] */, msmd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MSMD_HIP_H_ */
