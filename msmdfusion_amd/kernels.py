"""Tensor-level wrappers over the C ABI (include/msmd_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every
computation is a call into libmsmd_hip.so on torch's current stream.  All
functions require CUDA (ROCm) tensors and raise otherwise -- no CPU path.
"""
import ctypes as C
import os

import torch

from ._lib import check, float_arr, int3, lib


def _raw_stream(device_index=None):
    """Handle of torch's current stream (an int).  torch.cuda.current_stream() builds a
    Python Stream object per call -- 8 us each, 85 calls per training step."""
    if device_index is None:
        device_index = torch._C._cuda_getDevice()     # (torch.cuda.current_device() minus its
    return torch._C._cuda_getCurrentRawStream(device_index)   # lazy-init check: 1 us a call)


def _stream():
    return C.c_void_p(_raw_stream())


def _p(t):
    # (the address as a Python int: ctypes converts it for a c_void_p parameter itself, and
    # building a c_void_p object per argument was a quarter of a 17-argument call's 3.5 us)
    return None if t is None else t.data_ptr()


def _need_cuda(*ts):
    """Every operand on the GPU, and on the CURRENT one: the C ABI launches on the
    current HIP device and on torch's current stream of that device, so a tensor
    living elsewhere (single-process multi-GPU, a forgotten set_device) would be
    touched from the wrong device and stream -- refuse instead."""
    cur = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("msmdfusion_amd kernels need CUDA/ROCm tensors "
                               "(there is no CPU fallback)")
        if cur is None:
            cur = torch._C._cuda_getDevice()
        if t.device.index != cur:
            raise RuntimeError("tensor on cuda:%d but the current device is cuda:%d: wrap the "
                               "call in torch.cuda.device(tensor.device)" % (t.device.index, cur))


def _need_bzyx(*index_tensors):
    """The index kernels read rows as one int4 (b,z,y,x): anything else (the
    5-column tensors voxel_modality_split leaves, MSMDFusion.py:322-323) would be
    read misaligned and past the end."""
    for t in index_tensors:
        if t.dim() != 2 or t.shape[1] != 4:
            raise ValueError("expected [N,4] (b,z,y,x) voxel indices, got %s" % (tuple(t.shape),))


_WS_CACHE = {}
_WS_CACHE_MAX = 1 << 30


def _ws(nbytes, device):
    """Scratch for one library call (or a count -> host read -> fill pair).  Grow-only
    buffer per (device, stream): every user is stream-ordered behind the previous one, a
    stream is driven by one thread at a time, and nothing returned to callers aliases the
    scratch -- so ~250 allocator calls per LC step (two threads contending for the caching
    allocator's lock) become dictionary look-ups."""
    nbytes = max(int(nbytes), 256)
    if nbytes > _WS_CACHE_MAX:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    key = (device.index, _raw_stream(device.index))
    buf = _WS_CACHE.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _WS_CACHE[key] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8,
                                           device=device)
    return buf


class _Count:
    """Where a counting kernel puts its total and how the host gets it: a device int read
    with .item().  (Round 2 also tried pinned, device-mapped host slots the host spins on:
    134.2-134.3 against 134.4 samples/s -- what a read costs next to the feature pass is the
    counting kernels' turn on a busy GPU, not the copy; removed.)"""

    def __init__(self, device):
        self.tensor = torch.empty((1,), dtype=torch.int32, device=device)
        self.ptr = _p(self.tensor)

    def read(self):
        return int(self.tensor.item())


def _expand3(v):
    return [int(v)] * 3 if isinstance(v, int) else [int(x) for x in v]


def kernel_volume(ksize):
    k = _expand3(ksize)
    return k[0] * k[1] * k[2]


# ------------------------------------------------------------------ voxelization
def hard_voxelize(points, voxel_size, coors_range, max_points, max_voxels,
                  want_voxels=True, want_mean=False):
    """voxel_layer.hard_voxelize (mmdet3d/ops/voxel/src/voxelization.h:51-69).

    Returns (voxels[M,max_points,C] | None, coors[M,3], num_points[M],
    mean[M,C] | None).  One host read (the voxel count), like the reference.
    """
    _need_cuda(points)
    pts = points.contiguous().float()
    n, c = pts.shape
    dev = pts.device
    voxels = torch.empty((max_voxels, max_points, c), dtype=torch.float32, device=dev) \
        if want_voxels else None
    mean = torch.empty((max_voxels, c), dtype=torch.float32, device=dev) if want_mean else None
    coors = torch.empty((max_voxels, 3), dtype=torch.int32, device=dev)
    npv = torch.empty((max_voxels,), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    nbytes = lib.msmd_voxelize_workspace_bytes(n, max_voxels, max_points)
    ws = _ws(nbytes, dev)
    check(lib.msmd_hard_voxelize(_p(pts), n, c, float_arr(voxel_size), float_arr(coors_range),
                                 int(max_points), int(max_voxels), _p(voxels), _p(coors), _p(npv),
                                 _p(mean), _p(count), _p(ws), nbytes, _stream()),
          "msmd_hard_voxelize")
    m = int(count.item())
    return (voxels[:m] if want_voxels else None, coors[:m], npv[:m],
            mean[:m] if want_mean else None)


class _VoxDesc(C.Structure):        # include/msmd_hip.h: msmd_voxelize_desc
    _fields_ = [("points", C.c_void_p), ("num_points", C.c_int32), ("num_features", C.c_int32),
                ("voxel_size", C.c_float * 3), ("coors_range", C.c_float * 6),
                ("max_points", C.c_int32), ("max_voxels", C.c_int32), ("voxels", C.c_void_p),
                ("coors", C.c_void_p), ("num_points_per_voxel", C.c_void_p),
                ("voxel_mean", C.c_void_p), ("voxel_num", C.c_void_p)]


def hard_voxelize_batch(points_list, voxel_size, coors_range, max_points, max_voxels,
                        want_voxels=True, want_mean=False):
    """hard_voxelize for every sample of a batch in ONE launch set and with ONE host read
    (msmd_hard_voxelize_many: the reference syncs 4 times per sample,
    voxelization_cuda.cu:231-323, and is called once per sample and scale).
    voxel_size: one size for all clouds, or one size per cloud (the LiDAR sweep
    and the four scales of virtual points of a step go out in a single call)."""
    per_cloud = len(voxel_size) > 0 and isinstance(voxel_size[0], (list, tuple))
    if per_cloud and len(voxel_size) != len(points_list):
        raise ValueError("need one voxel size per cloud")
    if not points_list:
        return []
    pending = []
    descs = (_VoxDesc * len(points_list))()
    counts_all = None
    for ci, points in enumerate(points_list):
        _need_cuda(points)
        pts = points.contiguous().float()
        n, c = pts.shape
        dev = pts.device
        if counts_all is None:
            counts_all = torch.empty((len(points_list),), dtype=torch.int32, device=dev)
        voxels = torch.empty((max_voxels, max_points, c), dtype=torch.float32, device=dev) \
            if want_voxels else None
        mean = torch.empty((max_voxels, c), dtype=torch.float32, device=dev) if want_mean else None
        coors = torch.empty((max_voxels, 3), dtype=torch.int32, device=dev)
        npv = torch.empty((max_voxels,), dtype=torch.int32, device=dev)
        count = counts_all[ci:ci + 1]
        vs = voxel_size[ci] if per_cloud else voxel_size
        d = descs[ci]
        d.points, d.num_points, d.num_features = _p(pts), n, c
        d.voxel_size = (C.c_float * 3)(*[float(v) for v in vs])
        d.coors_range = (C.c_float * 6)(*[float(v) for v in coors_range])
        d.max_points, d.max_voxels = int(max_points), int(max_voxels)
        d.voxels, d.coors, d.num_points_per_voxel = _p(voxels), _p(coors), _p(npv)
        d.voxel_mean, d.voxel_num = _p(mean), _p(count)
        pending.append((voxels, coors, npv, mean, pts))
    nbytes = lib.msmd_hard_voxelize_many_workspace_bytes(descs, len(points_list))
    ws = _ws(nbytes, counts_all.device)
    check(lib.msmd_hard_voxelize_many(descs, len(points_list), _p(ws), nbytes, _stream()),
          "msmd_hard_voxelize_many")
    counts = counts_all.tolist()
    return [(v[:m] if want_voxels else None, c[:m], n[:m], mu[:m] if want_mean else None)
            for (v, c, n, mu, _), m in zip(pending, counts)]


def voxel_mean(voxels, num_points, out_features=None):
    _need_cuda(voxels, num_points)
    v = voxels.contiguous().float()
    m, mp, c = v.shape
    of = c if out_features is None else int(out_features)
    out = torch.empty((m, of), dtype=torch.float32, device=v.device)
    check(lib.msmd_voxel_mean(_p(v), _p(num_points.contiguous().int()), m, mp, c, of, _p(out),
                              _stream()), "msmd_voxel_mean")
    return out


# ------------------------------------------------------------------ dynamic voxelization
REDUCE_TYPES = {"sum": 0, "mean": 1, "max": 2}


def _need_dtype(t, dtype, what):
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s, got %s" % (what, dtype, t.dtype))


def _reduce_code(reduce_type):
    if reduce_type not in REDUCE_TYPES:
        raise RuntimeError("do not support reduce type %r (sum, mean, max)" % (reduce_type,))
    return REDUCE_TYPES[reduce_type]


def dynamic_voxelize(points, voxel_size, coors_range, coors=None):
    """voxel_layer.dynamic_voxelize (voxelization_cuda.cu:25-61): coors[N,3] (z,y,x) int32,
    written in place when given (out-of-range points get the reference's -1 pattern, slots
    it does not write keep their values); a zero-filled tensor otherwise."""
    _need_cuda(points, coors)
    _need_dtype(points, torch.float32, "points")
    if points.dim() != 2 or points.shape[1] < 3 or not points.is_contiguous():
        raise RuntimeError("points must be a contiguous [N, >=3] tensor")
    n = points.shape[0]
    if coors is None:
        coors = torch.zeros((n, 3), dtype=torch.int32, device=points.device)
    _need_dtype(coors, torch.int32, "coors")
    if coors.dim() != 2 or coors.shape[0] != n or coors.shape[1] < 3 or not coors.is_contiguous():
        raise RuntimeError("coors must be a contiguous [N, >=3] int32 tensor")
    check(lib.msmd_dynamic_voxelize(_p(points), n, points.shape[1], float_arr(voxel_size),
                                    float_arr(coors_range), coors.shape[1], _p(coors), _stream()),
          "msmd_dynamic_voxelize")
    return coors


class ScatterIndex:
    """The index half of a dynamic scatter, a function of the coordinates alone:
    voxel_coors[M, NDim] (unique valid rows, lexicographic), point2voxel[N] (-1: invalid),
    counts[M], and the segment table seg_points[N] / seg_start[M+1] (the points of voxel v in
    ascending point index).  Every scatter / gather on the same coordinates reuses it."""

    __slots__ = ("voxel_coors", "point2voxel", "seg_points", "seg_start", "counts",
                 "num_points", "num_voxels")

    def __init__(self, voxel_coors, point2voxel, seg_points, seg_start, counts):
        self.voxel_coors, self.point2voxel = voxel_coors, point2voxel
        self.seg_points, self.seg_start, self.counts = seg_points, seg_start, counts
        self.num_points, self.num_voxels = point2voxel.shape[0], voxel_coors.shape[0]


def scatter_index(coors):
    """coors[N, NDim] int32 (NDim 1..8; 4 = batch, z, y, x) -> ScatterIndex.  One host read
    (the voxel count), as hard_voxelize."""
    _need_cuda(coors)
    _need_dtype(coors, torch.int32, "coors")
    if coors.dim() != 2 or not 1 <= coors.shape[1] <= 8 or not coors.is_contiguous():
        raise RuntimeError("coors must be a contiguous [N, NDim] int32 tensor (NDim 1..8)")
    n, nd = coors.shape
    dev = coors.device
    vc = torch.empty((n, nd), dtype=torch.int32, device=dev)
    p2v = torch.empty((n,), dtype=torch.int32, device=dev)
    seg = torch.empty((n,), dtype=torch.int32, device=dev)
    start = torch.empty((n + 1,), dtype=torch.int32, device=dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    info = torch.empty((2,), dtype=torch.int32, device=dev)
    nbytes = lib.msmd_scatter_index_workspace_bytes(n)
    ws = _ws(nbytes, dev)
    check(lib.msmd_scatter_index(_p(coors), n, nd, _p(vc), _p(p2v), _p(seg), _p(start),
                                 _p(counts), _p(info), _p(ws), nbytes, _stream()),
          "msmd_scatter_index")
    m, overflow = info.tolist()
    if overflow:
        raise RuntimeError("scatter_index: the coordinate columns need more than 63 key bits")
    return ScatterIndex(vc[:m], p2v, seg, start[:m + 1], counts[:m])


def _need_feats(feats, n, what="feats"):
    _need_dtype(feats, torch.float32, what)
    if feats.dim() != 2 or feats.shape[0] != n or not feats.is_contiguous():
        raise RuntimeError("%s must be a contiguous [%d, C] float32 tensor" % (what, n))


def scatter_reduce(feats, index, reduce_type):
    """feats[N, C] -> (out[M, C], argmax[M, C] int32 | None): the segment reduce of
    dynamic_point_to_voxel_forward, in ascending point index (bitwise reproducible)."""
    code = _reduce_code(reduce_type)
    _need_cuda(feats, index.point2voxel)
    _need_feats(feats, index.num_points)
    m, c = index.num_voxels, feats.shape[1]
    out = torch.empty((m, c), dtype=torch.float32, device=feats.device)
    arg = torch.empty((m, c), dtype=torch.int32, device=feats.device) if code == 2 else None
    check(lib.msmd_scatter_reduce_f32(_p(feats), index.num_points, c, _p(index.seg_points),
                                      _p(index.seg_start), m, code, _p(out), _p(arg), _stream()),
          "msmd_scatter_reduce_f32")
    return out, arg


def scatter_reduce_backward(grad_out, point2voxel, reduce_type, counts=None, argmax=None,
                            out=None):
    """d feats[N, C] of scatter_reduce from d out[M, C] (0 for invalid points); written into
    `out` (contiguous [N, C] float32) when given."""
    code = _reduce_code(reduce_type)
    _need_cuda(grad_out, point2voxel, counts, argmax)
    _need_dtype(grad_out, torch.float32, "grad")
    _need_dtype(point2voxel, torch.int32, "point2voxel")
    g = grad_out.contiguous()
    m, c = g.shape
    n = point2voxel.shape[0]
    if code == 1 and (counts is None or counts.dtype != torch.int32 or counts.shape[0] != m):
        raise RuntimeError("mean backward needs counts[M] int32")
    if code == 2 and (argmax is None or argmax.dtype != torch.int32 or tuple(argmax.shape) != (m, c)):
        raise RuntimeError("max backward needs argmax[M, C] int32")
    if out is None:
        out = torch.empty((n, c), dtype=torch.float32, device=g.device)
    else:
        _need_cuda(out)
        _need_feats(out, n, "grad_feats")
        if out.shape[1] != c:
            raise RuntimeError("grad_feats has %d channels, the voxel gradient %d" % (out.shape[1], c))
    check(lib.msmd_scatter_reduce_bwd_f32(_p(g), m, n, c, _p(point2voxel.contiguous()),
                                          _p(None if counts is None else counts.contiguous()),
                                          _p(None if argmax is None else argmax.contiguous()),
                                          code, _p(out), _stream()),
          "msmd_scatter_reduce_bwd_f32")
    return out


def scatter_max_argmax(feats, point2voxel, reduced):
    """The reference backward's traceback (max_reduce_traceback_scatter_idx_kernel):
    argmax[M, C] = smallest point whose value equals the voxel's maximum."""
    _need_cuda(feats, point2voxel, reduced)
    n = point2voxel.shape[0]
    _need_feats(feats, n)
    _need_dtype(reduced, torch.float32, "reduced_feats")
    r = reduced.contiguous()
    m, c = r.shape
    arg = torch.empty((m, c), dtype=torch.int32, device=r.device)
    check(lib.msmd_scatter_max_argmax_f32(_p(feats), n, c, _p(point2voxel.contiguous()), _p(r), m,
                                          _p(arg), _stream()), "msmd_scatter_max_argmax_f32")
    return arg


def scatter_gather(voxel_feats, point2voxel):
    """out[i] = voxel_feats[point2voxel[i]], 0 for invalid points."""
    _need_cuda(voxel_feats, point2voxel)
    _need_dtype(voxel_feats, torch.float32, "voxel_feats")
    _need_dtype(point2voxel, torch.int32, "point2voxel")
    vf = voxel_feats.contiguous()
    m, c = vf.shape
    n = point2voxel.shape[0]
    out = torch.empty((n, c), dtype=torch.float32, device=vf.device)
    check(lib.msmd_scatter_gather_f32(_p(vf), m, c, _p(point2voxel.contiguous()), n, _p(out),
                                      _stream()), "msmd_scatter_gather_f32")
    return out


# ------------------------------------------------------------------ RoI-aware pooling
ROIAWARE_MODES = {"max": 0, "avg": 1}
ROIAWARE_MAX_OUT = 256


def roiaware_out_size(out_size):
    """int or 3-sequence -> (out_x, out_y, out_z), each 1..256 (the reference packs 8 bits per
    axis and aliases above 256: refused here)."""
    if isinstance(out_size, int):
        o = (out_size,) * 3
    else:
        o = tuple(out_size)
        if len(o) != 3 or not all(isinstance(v, int) for v in o):
            raise ValueError("out_size must be an int or a tuple of 3 ints, got %r" % (out_size,))
    if not all(1 <= v <= ROIAWARE_MAX_OUT for v in o):
        raise ValueError("out_size %r: every axis must be 1..%d" % (out_size, ROIAWARE_MAX_OUT))
    return o


def _need_rows(t, width, what, dtype=torch.float32):
    _need_dtype(t, dtype, what)
    if t.dim() != 2 or t.shape[1] != width or not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous [N, %d] %s tensor, got %s"
                           % (what, width, dtype, tuple(t.shape)))


def _need_ids(t, n, what):
    if t is None:
        return
    _need_dtype(t, torch.int32, what)
    if t.dim() != 1 or t.shape[0] != n or not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous [%d] int32 tensor" % (what, n))


class RoIPointIndex:
    """The index half of RoI-aware pooling, a function of the RoIs and points alone:
    hit_pts[H] (the points of every (RoI, voxel) cell in ascending point index, the first
    min(count, max_pts_per_voxel - 1) of them kept), vox_start[R*V + 1], and the inverse
    inv_cell[H] / pt_start[P + 1] (each point's kept cells in ascending RoI order).  Every
    pooling over the same RoIs and points reuses it, whatever its mode and channels."""

    __slots__ = ("hit_pts", "vox_start", "inv_cell", "pt_start", "num_rois", "num_points",
                 "out_size", "max_pts_per_voxel", "rows")

    def __init__(self, hit_pts, vox_start, inv_cell, pt_start, num_rois, num_points, out_size,
                 max_pts_per_voxel, rows=None):
        self.hit_pts, self.vox_start = hit_pts, vox_start
        self.inv_cell, self.pt_start = inv_cell, pt_start
        self.num_rois, self.num_points = num_rois, num_points
        self.out_size, self.max_pts_per_voxel = tuple(out_size), max_pts_per_voxel
        self.rows = rows          # the RoI rows an extractor selected, in output order

    @property
    def num_cells(self):
        ox, oy, oz = self.out_size
        return self.num_rois * ox * oy * oz

    def counts(self):
        """Kept points per cell, [R, X, Y, Z] int32."""
        n = (self.vox_start[1:] - self.vox_start[:-1]).clamp_(max=self.max_pts_per_voxel - 1)
        return n.view(self.num_rois, *self.out_size)


def roiaware_index(rois, pts, out_size, max_pts_per_voxel, roi_batch=None, pts_batch=None):
    """rois[R, 7], pts[P, 3] float32 (+ int32 batch ids, None: all 0) -> RoIPointIndex.  One
    launch set for the whole batch and one host read (the hit count)."""
    _need_cuda(rois, pts, roi_batch, pts_batch)
    _need_rows(rois, 7, "rois")
    _need_rows(pts, 3, "pts")
    ox, oy, oz = roiaware_out_size(out_size)
    if int(max_pts_per_voxel) < 1:
        raise ValueError("max_pts_per_voxel must be >= 1")
    r, n = rois.shape[0], pts.shape[0]
    _need_ids(roi_batch, r, "roi_batch")
    _need_ids(pts_batch, n, "pts_batch")
    dev = rois.device
    tiles = int(lib.msmd_roiaware_num_tiles(r, n))
    tile_start = torch.empty((tiles + 1,), dtype=torch.int32, device=dev)
    nbytes = lib.msmd_roiaware_count_workspace_bytes(r, n)
    ws = _ws(nbytes, dev)
    check(lib.msmd_roiaware_count(_p(rois), _p(roi_batch), r, _p(pts), _p(pts_batch), n,
                                  _p(tile_start), _p(ws), nbytes, _stream()), "msmd_roiaware_count")
    h = int(tile_start[tiles].item())
    cells = r * ox * oy * oz
    hit_pts = torch.empty((h,), dtype=torch.int32, device=dev)
    inv_cell = torch.empty((h,), dtype=torch.int64, device=dev)
    vox_start = torch.empty((cells + 1,), dtype=torch.int32, device=dev)
    pt_start = torch.empty((n + 1,), dtype=torch.int32, device=dev)
    nbytes = lib.msmd_roiaware_index_workspace_bytes(h)
    ws = _ws(nbytes, dev)
    check(lib.msmd_roiaware_index(_p(rois), _p(roi_batch), r, _p(pts), _p(pts_batch), n, ox, oy, oz,
                                  int(max_pts_per_voxel), _p(tile_start), h, _p(hit_pts),
                                  _p(vox_start), _p(inv_cell), _p(pt_start), _p(ws), nbytes,
                                  _stream()), "msmd_roiaware_index")
    return RoIPointIndex(hit_pts, vox_start, inv_cell, pt_start, r, n, (ox, oy, oz),
                         int(max_pts_per_voxel))


def _roiaware_mode(mode):
    if mode not in ROIAWARE_MODES:
        raise ValueError("mode must be 'max' or 'avg', got %r" % (mode,))
    return ROIAWARE_MODES[mode]


def roiaware_pool(pts_feature, index, mode, pooled=None, argmax=None):
    """pts_feature[P, C] -> (pooled[R, X, Y, Z, C], argmax[R, X, Y, Z, C] int32 | None).
    With `pooled` (and `argmax` for max) given, writes into them only where the reference
    kernels write (the shim's in-place contract)."""
    code = _roiaware_mode(mode)
    _need_cuda(pts_feature, index.vox_start, pooled, argmax)
    _need_feats(pts_feature, index.num_points, "pts_feature")
    c = pts_feature.shape[1]
    shape = (index.num_rois,) + index.out_size + (c,)
    ref_writes = pooled is not None
    if pooled is None:
        pooled = torch.empty(shape, dtype=torch.float32, device=pts_feature.device)
        if code == 0:
            argmax = torch.empty(shape, dtype=torch.int32, device=pts_feature.device)
    if code == 0 and argmax is None:
        raise RuntimeError("max pooling needs an argmax tensor")
    checks = [(pooled, torch.float32, "pooled_features")]
    if code == 0:
        checks.append((argmax, torch.int32, "argmax"))
    for t, dt, what in checks:
        _need_dtype(t, dt, what)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError("%s must be a contiguous %s tensor" % (what, shape))
    check(lib.msmd_roiaware_pool_f32(_p(pts_feature), index.num_points, c, _p(index.hit_pts),
                                     _p(index.vox_start), index.num_cells,
                                     index.max_pts_per_voxel, code, int(ref_writes), _p(pooled),
                                     _p(argmax if code == 0 else None), _stream()),
          "msmd_roiaware_pool_f32")
    return pooled, (argmax if code == 0 else None)


def roiaware_pool_backward(grad_out, index, mode, argmax=None, grad_in=None):
    """d pts_feature[P, C] from d pooled[R, X, Y, Z, C]: each point's kept hits summed in
    ascending RoI order (bitwise reproducible).  With `grad_in` given, adds into it."""
    code = _roiaware_mode(mode)
    _need_cuda(grad_out, index.vox_start, argmax, grad_in)
    _need_dtype(grad_out, torch.float32, "grad_out")
    g = grad_out.contiguous()
    if g.dim() != 5 or tuple(g.shape[:4]) != (index.num_rois,) + index.out_size:
        raise RuntimeError("grad_out must be [%d, %d, %d, %d, C]"
                           % ((index.num_rois,) + index.out_size))
    c = g.shape[4]
    if code == 0:
        if argmax is None or argmax.dtype != torch.int32 or argmax.shape != g.shape:
            raise RuntimeError("max backward needs argmax[R, X, Y, Z, C] int32")
        argmax = argmax.contiguous()
    accumulate = grad_in is not None
    if grad_in is None:
        grad_in = torch.empty((index.num_points, c), dtype=torch.float32, device=g.device)
    else:
        _need_feats(grad_in, index.num_points, "grad_in")
        if grad_in.shape[1] != c:
            raise RuntimeError("grad_in has %d channels, grad_out %d" % (grad_in.shape[1], c))
    check(lib.msmd_roiaware_pool_bwd_f32(_p(g), index.num_cells, c, _p(index.vox_start),
                                         index.max_pts_per_voxel, _p(index.inv_cell),
                                         _p(index.pt_start), index.num_points,
                                         _p(argmax if code == 0 else None), code, int(accumulate),
                                         _p(grad_in), _stream()), "msmd_roiaware_pool_bwd_f32")
    return grad_in


def roiaware_write_table(index, table):
    """Fill the reference's pts_idx_of_voxels[R, X, Y, Z, max_pts_per_voxel] int32 in place:
    slot 0 = count, slots 1..count = the points, the rest untouched."""
    _need_cuda(table, index.vox_start)
    _need_dtype(table, torch.int32, "pts_idx_of_voxels")
    shape = (index.num_rois,) + index.out_size + (index.max_pts_per_voxel,)
    if tuple(table.shape) != shape or not table.is_contiguous():
        raise RuntimeError("pts_idx_of_voxels must be a contiguous %s int32 tensor" % (shape,))
    check(lib.msmd_roiaware_write_table(_p(index.hit_pts), _p(index.vox_start), index.num_cells,
                                        index.max_pts_per_voxel, _p(table), _stream()),
          "msmd_roiaware_write_table")
    return table


def roiaware_index_from_table(table, num_points):
    """RoIPointIndex of a padded pts_idx_of_voxels[R, X, Y, Z, M] table (one host read: the
    number of entries)."""
    _need_cuda(table)
    _need_dtype(table, torch.int32, "pts_idx_of_voxels")
    if table.dim() != 5 or not table.is_contiguous():
        raise RuntimeError("pts_idx_of_voxels must be a contiguous [N, X, Y, Z, M] int32 tensor")
    r, ox, oy, oz, m = (int(v) for v in table.shape)
    roiaware_out_size((ox, oy, oz))
    if m < 1:
        raise ValueError("max_pts_per_voxel must be >= 1")
    dev = table.device
    cells = r * ox * oy * oz
    vox_start = torch.empty((cells + 1,), dtype=torch.int32, device=dev)
    nbytes = lib.msmd_roiaware_table_workspace_bytes(cells, 0)
    ws = _ws(nbytes, dev)
    check(lib.msmd_roiaware_table_count(_p(table), cells, m, _p(vox_start), _p(ws), nbytes,
                                        _stream()), "msmd_roiaware_table_count")
    e = int(vox_start[cells].item())
    hit_pts = torch.empty((e,), dtype=torch.int32, device=dev)
    inv_cell = torch.empty((e,), dtype=torch.int64, device=dev)
    pt_start = torch.empty((int(num_points) + 1,), dtype=torch.int32, device=dev)
    nbytes = lib.msmd_roiaware_table_workspace_bytes(cells, e)
    ws = _ws(nbytes, dev)
    check(lib.msmd_roiaware_table_index(_p(table), cells, m, int(num_points), e, _p(vox_start),
                                        _p(hit_pts), _p(inv_cell), _p(pt_start), _p(ws), nbytes,
                                        _stream()), "msmd_roiaware_table_index")
    return RoIPointIndex(hit_pts, vox_start, inv_cell, pt_start, r, int(num_points), (ox, oy, oz), m)


def points_in_boxes(boxes, pts, all_hits, out=None):
    """boxes[B, T, 7], pts[B, M, 3] float32 -> [B, M] first box or -1 (all_hits False) or
    [B, M, T] 0/1 flags (True), int32; written into `out` when given."""
    _need_cuda(boxes, pts, out)
    for t, w, what in ((boxes, 7, "boxes"), (pts, 3, "points")):
        _need_dtype(t, torch.float32, what)
        if t.dim() != 3 or t.shape[2] != w or not t.is_contiguous():
            raise RuntimeError("%s must be a contiguous [B, N, %d] float32 tensor, got %s"
                               % (what, w, tuple(t.shape)))
    if boxes.shape[0] != pts.shape[0]:
        raise RuntimeError("points and boxes need the same batch size, got %d and %d"
                           % (pts.shape[0], boxes.shape[0]))
    b, m, t = pts.shape[0], pts.shape[1], boxes.shape[1]
    shape = (b, m, t) if all_hits else (b, m)
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=pts.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != shape or not out.is_contiguous():
        raise RuntimeError("box_idxs_of_pts must be a contiguous %s int32 tensor" % (shape,))
    check(lib.msmd_points_in_boxes_f32(_p(boxes), _p(pts), b, t, m, int(bool(all_hits)), _p(out),
                                       _stream()), "msmd_points_in_boxes_f32")
    return out


# ------------------------------------------------------------------ rulebooks
def conv_output_size(in_shape, ksize, stride, padding, dilation=(1, 1, 1)):
    """mmdet3d/ops/spconv/ops.py:20-30."""
    return [(in_shape[i] + 2 * padding[i] - dilation[i] * (ksize[i] - 1) - 1) // stride[i] + 1
            for i in range(3)]


# SubM index: "hash" (2N-slot table, cost ~ voxels), "bitmap" (occupancy words of the grid,
# cost ~ grid cells + a third of the hash's per-voxel cost) or "auto" by size
_SUBM_INDEX = os.environ.get("MSMD_SUBM_INDEX", "auto")
_SUBM_BITMAP_WORDS_PER_VOXEL = float(os.environ.get("MSMD_SUBM_BITMAP_WORDS_PER_VOXEL", "100"))
_SUBM_BITMAP_MIN_VOXELS = int(os.environ.get("MSMD_SUBM_BITMAP_MIN_VOXELS", "60000"))


def subm_index_method(n, batch_size, spatial_shape, method=None):
    method = method or _SUBM_INDEX
    if method != "auto":
        return method
    # the bitmap is laid out in 4 x 8 x 8 bricks (csrc/rulebook.hip): the grid padded to
    # whole bricks is what it clears and counts, and the entry point takes fewer than 2^24
    # bricks -- a thin grid (D = 1..3 pads 4x along z) or a huge one takes the hash index
    d, h, w = (int(v) for v in spatial_shape)
    bricks = int(batch_size) * ((d + 3) // 4) * ((h + 7) // 8) * ((w + 7) // 8)
    if bricks >= 1 << 24:
        return "hash"
    words = bricks * 8          # 256 cells per brick
    # the bitmap's clear + count (~3 ps per 32-cell word) against what it saves per voxel
    # (~0.3 ns), and not below the size where either is launch-bound anyway
    return "bitmap" if n >= _SUBM_BITMAP_MIN_VOXELS and words <= _SUBM_BITMAP_WORDS_PER_VOXEL * n \
        else "hash"


def rulebook_subm(indices, batch_size, spatial_shape, ksize, method=None):
    """-> nbr[K,N] int32 (output-stationary neighbour table)."""
    _need_bzyx(indices)
    _need_cuda(indices)
    idx = indices.contiguous().int()
    n = idx.shape[0]
    ks = _expand3(ksize)
    nbr = torch.empty((kernel_volume(ks), n), dtype=torch.int32, device=idx.device)
    if subm_index_method(n, batch_size, spatial_shape, method) == "bitmap":
        nbytes = lib.msmd_rulebook_subm_bitmap_workspace_bytes(n, int(batch_size),
                                                               int3(spatial_shape))
        ws = _ws(nbytes, idx.device)
        check(lib.msmd_rulebook_subm3d_bitmap(_p(idx), n, int(batch_size), int3(spatial_shape),
                                              int3(ks), _p(nbr), _p(ws), nbytes, _stream()),
              "msmd_rulebook_subm3d_bitmap")
        return nbr
    nbytes = lib.msmd_rulebook_subm_workspace_bytes(n)
    ws = _ws(nbytes, idx.device)
    check(lib.msmd_rulebook_subm3d(_p(idx), n, int(batch_size), int3(spatial_shape), int3(ks),
                                   _p(nbr), _p(ws), nbytes, _stream()), "msmd_rulebook_subm3d")
    return nbr


_INT3 = C.c_int * 3


class _StridedGeometry:
    """[(ksize, stride, padding), ...] expanded against a grid, level l over level l - 1's
    output grid: per level ks, st, pd, in_shape, out_shape, and the same as the flat c_int arrays
    (f_ks, f_st, f_pd, f_in, f_out) the chain entry points take."""

    def __init__(self, in_shape, geoms, out_size=conv_output_size):
        self.ks, self.st, self.pd, self.in_shape, self.out_shape = [], [], [], [], []
        shape = [int(v) for v in in_shape]
        for ksize, stride, padding in geoms:
            ks, st, pd = _expand3(ksize), _expand3(stride), _expand3(padding)
            self.in_shape.append(list(shape))
            shape = out_size(shape, ks, st, pd)
            self.out_shape.append(list(shape))
            self.ks.append(ks)
            self.st.append(st)
            self.pd.append(pd)
        flat = lambda rows: (C.c_int * (3 * len(rows)))(*[v for r in rows for v in r])  # noqa: E731
        self.f_ks, self.f_st, self.f_pd = flat(self.ks), flat(self.st), flat(self.pd)
        self.f_in, self.f_out = flat(self.in_shape), flat(self.out_shape)

    def level(self, l):
        """(out_shape, ks, st, pd) of level l as the library takes one level's: its three ints
        of the flat arrays, in place."""
        return tuple(_INT3.from_buffer(f, 12 * l)
                     for f in (self.f_out, self.f_ks, self.f_st, self.f_pd))


def _region_bytes(batch_size, shape):
    """The 256-byte-aligned workspace region of one voxel set on the grid `shape`: what the
    chain entry points lay out per level, and what a fill of that level is handed."""
    return (lib.msmd_rulebook_conv_workspace_bytes(int(batch_size), int3(shape)) + 255) // 256 * 256


def _strided_fill(fill, idx, batch_size, geo, l, m, need_bwd, ws_addr, ws_bytes):
    """Level l of geo over the rows idx, whose output set (m rows) has been counted into the
    workspace at ws_addr -> (out_indices[m,4], nbr_fwd[K,m], nbr_bwd[K,n] | None)."""
    n, dev, kvol = idx.shape[0], idx.device, kernel_volume(geo.ks[l])
    out_idx = torch.empty((m, 4), dtype=torch.int32, device=dev)
    nbr_fwd = torch.empty((kvol, m), dtype=torch.int32, device=dev)
    nbr_bwd = torch.empty((kvol, n), dtype=torch.int32, device=dev) if need_bwd else None
    check(fill(_p(idx), n, int(batch_size), *geo.level(l), m, _p(out_idx), _p(nbr_fwd),
               _p(nbr_bwd), ws_addr, ws_bytes, _stream()), fill.__name__)
    return out_idx, nbr_fwd, nbr_bwd


def add_conv_chain(extras, batch_size, in_shape, geoms, need_bwd=True):
    """The fusion stack's stage chain with ONE host read: level l's strided conv (geoms[l] =
    (ksize, stride, padding)) runs over total_l = extras[0] for l = 0 and
    sparse_add(extras[l], out_{l-1}) after that (a = the extra set, b = the previous level's
    output set, as sparse_add_index(extras[l], out_prev)).  All union and output sets are
    counted on the device back to back (msmd_rulebook_add_conv_count_chain), read together,
    then filled level by level.  -> per level dict(total_indices, map_a, map_b (None at level
    0), out_indices, nbr_fwd, nbr_bwd, in_shape, out_shape): tensor for tensor what
    sparse_add_index + rulebook_conv give stage by stage."""
    levels = len(geoms)
    if len(extras) != levels or levels < 1:
        raise ValueError("add_conv_chain: one extra voxel set per level")
    idx = []
    for e in extras:
        _need_bzyx(e)
        _need_cuda(e)
        idx.append(e if (e.dtype == torch.int32 and e.is_contiguous()) else e.contiguous().int())
    dev = idx[0].device
    geo = _StridedGeometry(in_shape, geoms)
    nbytes = lib.msmd_rulebook_add_conv_chain_workspace_bytes(int(batch_size), levels, geo.f_in,
                                                              geo.f_out)
    # (not the per-stream scratch: the fills below run after other library calls may have
    # used that one)
    ws = torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=dev)
    ptrs = (C.c_void_p * levels)(*[t.data_ptr() for t in idx])
    ns = (C.c_int * levels)(*[int(t.shape[0]) for t in idx])
    counts = torch.empty((2 * levels,), dtype=torch.int32, device=dev)
    check(lib.msmd_rulebook_add_conv_count_chain(ptrs, ns, int(batch_size), levels, geo.f_in,
                                                 geo.f_out, geo.f_ks, geo.f_st, geo.f_pd,
                                                 _p(counts), _p(ws), nbytes, _stream()),
          "msmd_rulebook_add_conv_count_chain")
    ms = counts.tolist()                                    # the chain's one host read
    out, at, prev = [], ws.data_ptr(), None
    for l in range(levels):
        total, ma, mb = idx[0], None, None
        if l > 0:                        # the union region, then the level's conv region
            ub = _region_bytes(batch_size, geo.in_shape[l])
            total, _, ma, mb = _sparse_add_fill(None, idx[l], None, prev, batch_size,
                                                geo.in_shape[l], int(ms[2 * l]), at, ub)
            at += ub
        cb = _region_bytes(batch_size, geo.out_shape[l])
        out_idx, nbr_fwd, nbr_bwd = _strided_fill(lib.msmd_rulebook_conv3d_fill, total, batch_size,
                                                  geo, l, int(ms[2 * l + 1]), need_bwd, at, cb)
        at += cb
        out.append(dict(total_indices=total, map_a=ma, map_b=mb, out_indices=out_idx,
                        nbr_fwd=nbr_fwd, nbr_bwd=nbr_bwd, in_shape=geo.in_shape[l],
                        out_shape=geo.out_shape[l]))
        prev = out_idx
    return out


class _SubmDesc(C.Structure):      # include/msmd_hip.h: msmd_subm_desc
    _fields_ = [("indices", C.c_void_p), ("n", C.c_int32), ("batch_size", C.c_int32),
                ("spatial_shape", C.c_int32 * 3), ("ksize", C.c_int32 * 3),
                ("method", C.c_int32), ("reserved", C.c_int32), ("nbr", C.c_void_p)]


def subm_table(indices, ksize):
    """The empty [K, N] table rulebook_subm_many fills for a voxel set."""
    return torch.empty((kernel_volume(_expand3(ksize)), indices.shape[0]), dtype=torch.int32,
                       device=indices.device)


def rulebook_subm_many(jobs):
    """rulebook_subm for MANY voxel sets in one library call and one launch set
    (csrc/rulebook.hip: msmd_rulebook_subm3d_many).  jobs: dicts with indices [N,4] int32
    (b,z,y,x) contiguous, batch_size, spatial_shape, ksize, nbr (= subm_table(...), filled
    here) and optionally method.  The index method of each set is chosen as rulebook_subm
    chooses it; the tables are those of the single calls."""
    if not jobs:
        return
    descs = (_SubmDesc * len(jobs))()
    keep = []
    for d, j in zip(descs, jobs):
        idx = j["indices"]
        _need_bzyx(idx)
        _need_cuda(idx, j["nbr"])
        if idx.dtype != torch.int32 or not idx.is_contiguous():
            idx = idx.contiguous().int()
        keep.append(idx)
        n = idx.shape[0]
        ks = _expand3(j["ksize"])
        if tuple(j["nbr"].shape) != (kernel_volume(ks), n) or not j["nbr"].is_contiguous():
            raise ValueError("rulebook_subm_many: nbr must be the contiguous [K, N] table")
        d.indices, d.n, d.batch_size = idx.data_ptr(), n, int(j["batch_size"])
        d.spatial_shape[:] = [int(v) for v in j["spatial_shape"]]
        d.ksize[:] = ks
        d.method = int(subm_index_method(n, j["batch_size"], j["spatial_shape"],
                                         j.get("method")) == "bitmap")
        d.nbr = j["nbr"].data_ptr()
    dev = jobs[0]["nbr"].device
    nbytes = lib.msmd_rulebook_subm3d_many_workspace_bytes(descs, len(jobs))
    ws = _ws(nbytes, dev)
    check(lib.msmd_rulebook_subm3d_many(descs, len(jobs), _p(ws), nbytes, _stream()),
          "msmd_rulebook_subm3d_many")


def _rulebook_strided(indices, batch_size, spatial_shape, geom, out_size, count, fill, need_bwd):
    """One strided or transposed level (geom = (ksize, stride, padding), out_size its output
    grid): count the output set, read the count, fill."""
    _need_bzyx(indices)
    _need_cuda(indices)
    idx = indices.contiguous().int()
    geo = _StridedGeometry(spatial_shape, [geom], out_size)
    nbytes = lib.msmd_rulebook_conv_workspace_bytes(int(batch_size), geo.f_out)
    ws = _ws(nbytes, idx.device)
    m = _Count(idx.device)
    check(count(_p(idx), idx.shape[0], int(batch_size), geo.f_out, geo.f_ks, geo.f_st, geo.f_pd,
                m.ptr, _p(ws), nbytes, _stream()), count.__name__)
    return _strided_fill(fill, idx, batch_size, geo, 0, m.read(), need_bwd, _p(ws), nbytes) \
        + (geo.out_shape[0],)


def rulebook_conv(indices, batch_size, spatial_shape, ksize, stride, padding, need_bwd=True):
    """-> (out_indices[M,4], nbr_fwd[K,M], nbr_bwd[K,N] | None, out_shape)"""
    return _rulebook_strided(indices, batch_size, spatial_shape, (ksize, stride, padding),
                             conv_output_size, lib.msmd_rulebook_conv3d_count,
                             lib.msmd_rulebook_conv3d_fill, need_bwd)


def rulebook_conv_chain(indices, batch_size, spatial_shape, geoms, need_bwd=True):
    """A chain of strided convs, each over the previous one's output set: geoms = [(ksize,
    stride, padding), ...].  All output sets are counted on the device back to back and the
    counts read ONCE.  -> [(out_indices, nbr_fwd, nbr_bwd | None, out_shape), ...], tensor for
    tensor what rulebook_conv gives level by level."""
    _need_bzyx(indices)
    _need_cuda(indices)
    idx = indices.contiguous().int()
    dev = idx.device
    levels = len(geoms)
    geo = _StridedGeometry(spatial_shape, geoms)
    nbytes = lib.msmd_rulebook_conv_chain_workspace_bytes(int(batch_size), levels, geo.f_out)
    ws = _ws(nbytes, dev)
    counts = torch.empty((levels,), dtype=torch.int32, device=dev)
    check(lib.msmd_rulebook_conv3d_count_chain(_p(idx), idx.shape[0], int(batch_size), levels,
                                               geo.f_out, geo.f_ks, geo.f_st, geo.f_pd, _p(counts),
                                               _p(ws), nbytes, _stream()),
          "msmd_rulebook_conv3d_count_chain")
    ms = counts.tolist()                                    # the chain's one host read
    out, at = [], ws.data_ptr()
    for l in range(levels):
        lvl_bytes = _region_bytes(batch_size, geo.out_shape[l])
        tables = _strided_fill(lib.msmd_rulebook_conv3d_fill, idx, batch_size, geo, l, int(ms[l]),
                               need_bwd, at, lvl_bytes)
        out.append(tables + (geo.out_shape[l],))
        at += lvl_bytes
        idx = tables[0]
    return out


def deconv_output_size(in_shape, ksize, stride, padding, output_padding=(0, 0, 0),
                       dilation=(1, 1, 1)):
    """mmdet3d/ops/spconv/ops.py:33-43: (in - 1) * s - 2p + k + output_padding (the
    reference's formula: dilation does not enter it)."""
    ks, st, pd, op = _expand3(ksize), _expand3(stride), _expand3(padding), _expand3(output_padding)
    for k in ks:
        if k == -1:
            raise ValueError("deconv don't support kernel_size < 0")
    return [(int(in_shape[i]) - 1) * st[i] - 2 * pd[i] + ks[i] + op[i] for i in range(3)]


def rulebook_deconv(indices, batch_size, spatial_shape, ksize, stride, padding,
                    output_padding=(0, 0, 0), need_bwd=True):
    """Transposed-conv rulebook (geometry.h:196-245): input c reaches c*s - p + k.
    -> (out_indices[M,4] in ascending linear id, nbr_fwd[K,M], nbr_bwd[K,N] | None, out_shape);
    one host read (the output count)."""
    def out_size(*geom):
        out_shape = deconv_output_size(*geom, output_padding)
        if any(s < 1 for s in out_shape):
            raise ValueError("transposed conv output shape %s is empty" % (out_shape,))
        return out_shape
    return _rulebook_strided(indices, batch_size, spatial_shape, (ksize, stride, padding), out_size,
                             lib.msmd_rulebook_deconv3d_count, lib.msmd_rulebook_deconv3d_fill,
                             need_bwd)


def rulebook_pairs(nbr, ld=None):
    """nbr[K,M] -> (indice_pairs[K,2,ld], indice_num[K]): the reference's
    rulebook format (spconv_ops.h:55-59), pairs sorted by output row."""
    _need_cuda(nbr)
    kvol, m = nbr.shape
    ld = m if ld is None else int(ld)
    dev = nbr.device
    pairs = torch.empty((kvol, 2, ld), dtype=torch.int32, device=dev)
    num = torch.empty((kvol,), dtype=torch.int32, device=dev)
    nbytes = lib.msmd_rulebook_pairs_workspace_bytes(kvol, m)
    ws = _ws(nbytes, dev)
    check(lib.msmd_rulebook_pairs(_p(nbr.contiguous()), kvol, m, _p(pairs), ld, _p(num), _p(ws),
                                  nbytes, _stream()), "msmd_rulebook_pairs")
    return pairs, num


# ------------------------------------------------------------------ max-pool
def _need_pool_args(feat, nbr_bwd):
    _need_cuda(feat, nbr_bwd)
    _need_dtype(feat, torch.float32, "features")
    _need_dtype(nbr_bwd, torch.int32, "nbr_bwd")
    if feat.dim() != 2 or nbr_bwd.dim() != 2 or nbr_bwd.shape[1] != feat.shape[0]:
        raise ValueError("max-pool: features [N,C] and nbr_bwd [K,N] expected, got %s and %s"
                         % (tuple(feat.shape), tuple(nbr_bwd.shape)))
    if feat.shape[1] < 1:
        raise ValueError("max-pool: at least one channel")


def maxpool_fwd(feat, nbr_bwd, n_out):
    """Sparse max-pool over a strided rulebook's input-side table nbr_bwd[K, N] (every pair
    listed): out[o] starts at 0 and takes in[i] where out < in (maxpool.cc:20-40).
    -> [n_out, C]."""
    _need_pool_args(feat, nbr_bwd)
    feat, nbr_bwd = feat.contiguous(), nbr_bwd.contiguous()
    n, c = feat.shape
    out = torch.empty((int(n_out), c), dtype=torch.float32, device=feat.device)
    check(lib.msmd_sparse_maxpool_fwd_f32(_p(feat), n, c, _p(nbr_bwd), nbr_bwd.shape[0],
                                          int(n_out), _p(out), _stream()),
          "msmd_sparse_maxpool_fwd_f32")
    return out


def maxpool_bwd(feat, out, grad_out, nbr_bwd):
    """din[i] = sum over k ascending of dout[o] where out[o] == in[i] (maxpool.cc:42-62).
    -> [N, C], bitwise the functor's loop."""
    _need_pool_args(feat, nbr_bwd)
    _need_cuda(out, grad_out)
    _need_dtype(out, torch.float32, "out")
    _need_dtype(grad_out, torch.float32, "grad_out")
    n, c = feat.shape
    if out.shape != grad_out.shape or (out.dim() == 2 and out.shape[1] != c):
        raise ValueError("max-pool backward: out / grad_out must both be [n_out, %d]" % c)
    feat, out, grad_out = feat.contiguous(), out.contiguous(), grad_out.contiguous()
    din = torch.empty_like(feat)
    check(lib.msmd_sparse_maxpool_bwd_f32(_p(feat), _p(out), _p(grad_out), n, c,
                                          _p(nbr_bwd.contiguous()), nbr_bwd.shape[0],
                                          out.shape[0], _p(din), _stream()),
          "msmd_sparse_maxpool_bwd_f32")
    return din


# ------------------------------------------------------------------ convolution
def pack_weight(weight, transpose=False, krsc=False):
    """weight -> MFMA-fragment order (see spconv.hip).  weight is [K,Cin,Cout]
    or, with krsc=True, the modules' KRSC parameter [Cout,kd,kh,kw,Cin]."""
    _need_cuda(weight)
    w = weight.contiguous().float()
    if krsc:
        cout, cin = w.shape[0], w.shape[-1]
        kvol = w.numel() // (cout * cin)
    else:
        kvol, cin, cout = w.shape
    packed = torch.empty((lib.msmd_spconv_packed_weight_elems(kvol, cin, cout),),
                         dtype=torch.float32, device=w.device)
    check(lib.msmd_spconv_pack_weight(_p(w), kvol, cin, cout, int(bool(transpose)) | (2 if krsc else 0),
                                      _p(packed), _stream()), "msmd_spconv_pack_weight")
    return packed


# bench.py sets this to a list to time individual launches with events recorded
# on the launch stream: entries are (kind, start_event, end_event, meta).
PROFILE = None


def _prof_begin():
    if PROFILE is None:
        return None
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()
    return ev


def _prof_end(kind, start, **meta):
    if start is not None:
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        PROFILE.append((kind, start, end, meta))


# tools/split_bench.py --lc-b2 sets this to a list: every conv launch of a step is kept as
# (kind, meta, relaunch) -- relaunch() issues the same library call on the same operands
# again, alone on the chip -- to separate a layer's own time from what the step costs it.
CAPTURE = None


def _launch(kind, call, **meta):
    """One conv library call, bracketed by PROFILE's events and kept for CAPTURE."""
    ev = _prof_begin()
    call()
    _prof_end(kind, ev, **meta)
    if CAPTURE is not None:
        CAPTURE.append((kind, meta, call))


TILE_ROWS = 128     # rows per workgroup tile of the conv kernels


def row_mask_order(nbr, tile_lpt=True):
    """Tiling order of the rows of nbr[K,n]: rows sorted by (rank-permuted) neighbour
    mask so that the rows of a wave / a 128-row tile share their empty offsets, then
    -- tile_lpt -- whole tiles re-sequenced heaviest first for the persistent
    scheduler.  Masks and tile costs come from the C ABI; the sorts are torch's
    device radix sort.  It only chooses a tiling: results do not depend on it."""
    _need_cuda(nbr)
    kvol, n = nbr.shape
    if kvol > 64 or n == 0:
        return None
    keys = torch.empty((n,), dtype=torch.int64, device=nbr.device)
    check(lib.msmd_rulebook_row_masks(_p(nbr), kvol, n, None, _p(keys), _stream()),
          "msmd_rulebook_row_masks")
    if 2 * kvol <= 32 or (kvol <= 27):   # key fits 32 bits: half the radix passes
        keys = (keys - 2147483648).int()   # unsigned order under a signed compare
    order = torch.sort(keys, stable=False)[1].int()
    full = n // TILE_ROWS
    if tile_lpt and full > 1:
        cost = torch.empty(((n + TILE_ROWS - 1) // TILE_ROWS,), dtype=torch.int32,
                           device=nbr.device)
        check(lib.msmd_rulebook_tile_costs(_p(nbr), kvol, n, _p(order), TILE_ROWS, _p(cost),
                                           _stream()), "msmd_rulebook_tile_costs")
        seq = torch.sort(cost[:full], stable=True)[1]      # the partial last tile stays last
        head = order[:full * TILE_ROWS].view(full, TILE_ROWS).index_select(0, seq).reshape(-1)
        order = torch.cat([head, order[full * TILE_ROWS:]]) if n % TILE_ROWS else head
    return order


def rulebook_tiling(nbr, want_table=True):
    """(order[n], table in tile order | None) of nbr[K,n] in one library call: what
    row_mask_order + permute_cols compute through torch, with the sorts done in the
    library (K <= 31; falls back to those two otherwise)."""
    _need_cuda(nbr)
    kvol, n = nbr.shape
    if n == 0:
        return None, nbr
    if kvol > 31:
        order = row_mask_order(nbr)
        return order, (permute_cols(nbr, order) if want_table and order is not None else nbr)
    t = nbr.contiguous()
    order = torch.empty((n,), dtype=torch.int32, device=t.device)
    tiled = torch.empty_like(t) if want_table else None
    nbytes = lib.msmd_rulebook_tiling_workspace_bytes(n, TILE_ROWS)
    ws = _ws(nbytes, t.device)
    check(lib.msmd_rulebook_tiling(_p(t), kvol, n, TILE_ROWS, _p(order), _p(tiled), _p(ws), nbytes,
                                   _stream()), "msmd_rulebook_tiling")
    return order, tiled


def rulebook_plan(nbr, tile_rows=(), want_pairs=False, ld=None):
    """rulebook_tiling + tile_prefix (for each height in tile_rows, 128 / 256) +
    rulebook_pairs of one table in ONE library call.
    -> dict(order, tiled, prefix={rows: tensor}, pairs=(pairs, num) | None)"""
    _need_cuda(nbr)
    kvol, n = nbr.shape
    t = nbr.contiguous()
    dev = t.device
    order = torch.empty((n,), dtype=torch.int32, device=dev)
    tiled = torch.empty_like(t)
    pre = {r: torch.empty(((n + r - 1) // r + 1,), dtype=torch.int32, device=dev)
           for r in set(tile_rows)}
    if any(r not in (128, 256) for r in pre):
        raise ValueError("tile heights are 128 or 256 rows")
    pairs = num = None
    ld = n if ld is None else int(ld)
    if want_pairs:
        pairs = torch.empty((kvol, 2, ld), dtype=torch.int32, device=dev)
        num = torch.empty((kvol,), dtype=torch.int32, device=dev)
    nbytes = lib.msmd_rulebook_plan_workspace_bytes(kvol, n, TILE_ROWS)
    ws = _ws(nbytes, dev)
    check(lib.msmd_rulebook_plan(_p(t), kvol, n, TILE_ROWS, _p(order), _p(tiled), _p(pre.get(128)),
                                 _p(pre.get(256)), _p(pairs), ld, _p(num), _p(ws), nbytes,
                                 _stream()), "msmd_rulebook_plan")
    return dict(order=order, tiled=tiled, prefix=pre,
                pairs=(pairs, num) if want_pairs else None)


class _PlanDesc(C.Structure):      # include/msmd_hip.h: msmd_plan_desc (80 bytes)
    _fields_ = [("nbr", C.c_void_p), ("kvol", C.c_int32), ("n_rows", C.c_int32),
                ("order", C.c_void_p), ("tiled", C.c_void_p), ("prefix128", C.c_void_p),
                ("prefix256", C.c_void_p), ("indice_pairs", C.c_void_p),
                ("indice_num", C.c_void_p), ("segtab", C.c_void_p), ("ld", C.c_int32),
                ("reserved", C.c_int32)]


def rulebook_plan_many(jobs):
    """rulebook_plan (+ the one-chunk pair_segments table) of MANY tables in one library call
    and one launch set (csrc/plan.hip).  jobs: dicts with nbr [K,n] and optionally
    tile_rows (heights, 128 / 256; implies the tile-ordered table), want_table, want_pairs,
    want_segments (implies pairs), ld.  -> one dict per job:
    order, tiled | None, prefix {rows: tensor}, pairs (pairs, num) | None,
    segments (table, 1) | None -- the values the single calls give.
    All outputs of a call live in ONE int32 allocation (views; 256-byte aligned pieces)."""
    if not jobs:
        return []
    dev = jobs[0]["nbr"].device
    _need_cuda(*[j["nbr"] for j in jobs])
    descs = (_PlanDesc * len(jobs))()
    lay, total = [], 0

    def take(n):            # offset (int32 units) of an n-int piece
        nonlocal total
        o = total
        total += (n + 63) & ~63
        return o
    keep = []
    for d, j in zip(descs, jobs):
        t = j["nbr"]
        if not t.is_contiguous():
            t = t.contiguous()
        keep.append(t)
        kvol, n = t.shape
        rows = set(j.get("tile_rows") or ())
        if any(r not in (128, 256) for r in rows):
            raise ValueError("tile heights are 128 or 256 rows")
        want_seg = bool(j.get("want_segments"))
        want_pairs = bool(j.get("want_pairs")) or want_seg
        want_table = bool(j.get("want_table")) or bool(rows)
        ld = n if j.get("ld") is None else int(j["ld"])
        if want_seg and (WGRAD_CHUNK_ROWS > 0 or ld <= 0):
            want_seg = False            # chunked tables: pair_segments() after the call
        o = dict(kvol=kvol, n=n, ld=ld, order=take(n), tiled=take(kvol * n) if want_table else None,
                 prefix={r: take((n + r - 1) // r + 1) for r in sorted(rows)},
                 pairs=take(kvol * 2 * ld) if want_pairs else None,
                 num=take(kvol) if want_pairs else None,
                 seg=take(int(lib.msmd_rulebook_pair_segments_ints(kvol, 1))) if want_seg else None)
        lay.append(o)
        d.nbr, d.kvol, d.n_rows, d.ld = t.data_ptr(), kvol, n, ld
    slab = torch.empty((max(total, 1),), dtype=torch.int32, device=dev)
    base = slab.data_ptr()
    at = lambda off: None if off is None else base + 4 * off
    for d, o in zip(descs, lay):
        d.order, d.tiled = at(o["order"]), at(o["tiled"])
        d.prefix128, d.prefix256 = at(o["prefix"].get(128)), at(o["prefix"].get(256))
        d.indice_pairs, d.indice_num, d.segtab = at(o["pairs"]), at(o["num"]), at(o["seg"])
    nbytes = lib.msmd_rulebook_plan_many_workspace_bytes(descs, len(jobs))
    ws = _ws(nbytes, dev)
    check(lib.msmd_rulebook_plan_many(descs, len(jobs), _p(ws), nbytes, _stream()),
          "msmd_rulebook_plan_many")
    def view(off, *shape):
        size = 1
        for v in shape:
            size *= v
        return slab[off:off + size].view(*shape)
    out = []
    for o in lay:
        kvol, n, ld = o["kvol"], o["n"], o["ld"]
        pairs = None
        if o["pairs"] is not None:
            pairs = (view(o["pairs"], kvol, 2, ld), view(o["num"], kvol))
        seg = None
        if o["seg"] is not None:
            seg = (slab[o["seg"]:o["seg"] + 3 * kvol + 1], 1)
        out.append(dict(order=view(o["order"], n),
                        tiled=None if o["tiled"] is None else view(o["tiled"], kvol, n),
                        prefix={r: slab[off:off + (n + r - 1) // r + 1]
                                for r, off in o["prefix"].items()},
                        pairs=pairs, segments=seg))
    return out


_TILE_COUNTERS = {}


_SYNC_INTS = 1 + 8192       # tile counter + one stream-K exchange flag per workgroup ticket


def _tile_counter(device):
    """Zeroed int32s per (device, stream): [0] is the counter the persistent conv
    kernels draw tiles from, the rest are the split kernels' exchange flags; every
    launch leaves all of them at 0 again (see msmd_spconv_fwd_f32 / _fwd_split)."""
    key = (device, _raw_stream(device.index))
    c = _TILE_COUNTERS.get(key)
    if c is None:
        c = _TILE_COUNTERS[key] = torch.zeros((_SYNC_INTS,), dtype=torch.int32, device=device)
    return c


_EXCHANGE = {}


def _exchange_buffer(device, nbytes):
    """Grow-only scratch per (device, stream) for the split kernels' tile halves:
    launches on one stream are ordered, so one buffer serves them all."""
    key = (device, _raw_stream(device.index))
    b = _EXCHANGE.get(key)
    if b is None or b.numel() < nbytes:
        b = _EXCHANGE[key] = torch.empty((max(int(nbytes), 256),), dtype=torch.uint8,
                                         device=device)
    return b


def conv_forward(feat, packed_weight, nbr, n_out, c_out, weight_flip=False, row_order=None):
    """out[o] = sum_k feat[nbr[k,o]] @ W[k]  (implicit GEMM on MFMA)."""
    _need_cuda(feat, packed_weight, nbr)
    f = feat.contiguous().float()
    n_in, c_in = f.shape
    kvol, ld = nbr.shape
    out = torch.empty((n_out, c_out), dtype=torch.float32, device=f.device)
    # persistent tile scheduler whenever a (heaviest-first) order is supplied
    counter = _tile_counter(f.device) if row_order is not None else None
    _launch("spconv_fwd", lambda: check(
        lib.msmd_spconv_fwd_f32(_p(f), n_in, c_in, _p(packed_weight), _p(nbr), ld, int(n_out),
                                kvol, int(bool(weight_flip)), _p(row_order), _p(counter),
                                _p(out), int(c_out), _stream()), "msmd_spconv_fwd_f32"),
            nbr=nbr, c_in=c_in, c_out=int(c_out), n_in=n_in, n_out=int(n_out))
    return out


# ---------------------------------------------- split-bf16 ("fp32-equivalent") conv path
_SPLIT_SUPPORTED = {}


def split_supported(c_in, c_out, kvol=27):
    """Does the bf16-split implicit GEMM cover (contraction c_in, outputs c_out)?"""
    key = (c_in, c_out, kvol)
    v = _SPLIT_SUPPORTED.get(key)
    if v is None:
        v = _SPLIT_SUPPORTED[key] = bool(
            lib.msmd_spconv_fwd_split_supported(int(c_in), int(c_out), int(kvol)))
    return v


def pack_weight_split(weight, planes=3, transpose=False, krsc=False):
    """weight -> split bf16 planes in MFMA 16x16x32 fragment order."""
    _need_cuda(weight)
    w = weight.contiguous().float()
    if krsc:
        cout, cin = w.shape[0], w.shape[-1]
        kvol = w.numel() // (cout * cin)
    else:
        kvol, cin, cout = w.shape
    ci, co = (cout, cin) if transpose else (cin, cout)
    packed = torch.empty((lib.msmd_spconv_packed_split_bytes(kvol, ci, co, planes),),
                         dtype=torch.uint8, device=w.device)
    check(lib.msmd_spconv_pack_weight_split(_p(w), kvol, cin, cout,
                                            int(bool(transpose)) | (2 if krsc else 0), planes,
                                            _p(packed), _stream()),
          "msmd_spconv_pack_weight_split")
    return packed


def pack_weight_split_pair(weight, planes=3, krsc=False):
    """(pack_weight_split(w), pack_weight_split(w, transpose=True)) in one launch."""
    _need_cuda(weight)
    w = weight.contiguous().float()
    if krsc:
        cout, cin = w.shape[0], w.shape[-1]
        kvol = w.numel() // (cout * cin)
    else:
        kvol, cin, cout = w.shape
    a = torch.empty((lib.msmd_spconv_packed_split_bytes(kvol, cin, cout, planes),),
                    dtype=torch.uint8, device=w.device)
    b = torch.empty((lib.msmd_spconv_packed_split_bytes(kvol, cout, cin, planes),),
                    dtype=torch.uint8, device=w.device)
    check(lib.msmd_spconv_pack_weight_split_pair(_p(w), kvol, cin, cout, 2 if krsc else 0, planes,
                                                 _p(a), _p(b), _stream()),
          "msmd_spconv_pack_weight_split_pair")
    return a, b


class _PackDesc(C.Structure):      # csrc/spconv_split.hip: PackDesc (48 bytes)
    _fields_ = [("w", C.c_void_p), ("packed_a", C.c_void_p), ("packed_b", C.c_void_p),
                ("start", C.c_int64), ("kvol", C.c_int32), ("cin", C.c_int32),
                ("cout", C.c_int32), ("flags", C.c_int32)]


def pack_weight_split_many(jobs, planes=3):
    """pack_weight_split / pack_weight_split_pair of several weights in ONE launch.
    jobs: [(weight, krsc, packed, packed_transposed | None)] with `packed*` preallocated uint8
    tensors of msmd_spconv_packed_split_bytes each (same device).  The descriptor table goes to
    the device through a pinned staging copy (no host wait)."""
    if not jobs:
        return
    descs = (_PackDesc * len(jobs))()
    start = 0
    keep = []
    for i, (weight, krsc, packed, packed_t) in enumerate(jobs):
        _need_cuda(weight, packed, packed_t)
        w = weight.detach()
        if not (w.is_contiguous() and w.dtype == torch.float32):
            w = w.contiguous().float()
        keep.append(w)
        if krsc:
            cout, cin = w.shape[0], w.shape[-1]
            kvol = w.numel() // (cout * cin)
        else:
            kvol, cin, cout = w.shape
        d = descs[i]
        d.w, d.packed_a = w.data_ptr(), packed.data_ptr()
        d.packed_b = packed_t.data_ptr() if packed_t is not None else None
        d.start, d.kvol, d.cin, d.cout, d.flags = start, kvol, cin, cout, 2 if krsc else 0
        # one work unit = the `planes` 16-byte pieces of one (offset, k-block, tile, lane)
        start += lib.msmd_spconv_packed_split_bytes(kvol, cin, cout, planes) // (16 * planes)
        if packed_t is not None:
            start += lib.msmd_spconv_packed_split_bytes(kvol, cout, cin, planes) // (16 * planes)
    dev = jobs[0][0].device
    host = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).pin_memory()
    table = host.to(dev, non_blocking=True)
    check(lib.msmd_spconv_pack_weight_split_many(_p(table), len(jobs), start, int(planes),
                                                 _stream()), "msmd_spconv_pack_weight_split_many")
    # (the pinned buffer and the descriptor table must outlive the copy / the launch: they are
    # referenced by the stream until it has passed them)
    table.record_stream(torch.cuda.current_stream(dev))
    return host, table, keep


def permute_cols(nbr, order):
    """nbr[K,n] -> the table in tile order: out[k][p] = nbr[k][order[p]]."""
    _need_cuda(nbr, order)
    kvol, n = nbr.shape
    out = torch.empty_like(nbr)
    check(lib.msmd_rulebook_permute_cols(_p(nbr), kvol, n, n, _p(order), _p(out), _stream()),
          "msmd_rulebook_permute_cols")
    return out


_TILE_ROWS = {}


def split_tile_rows(c_out):
    """Rows per tile of the split kernel for a layer with c_out output channels."""
    v = _TILE_ROWS.get(c_out)
    if v is None:
        v = _TILE_ROWS[c_out] = int(lib.msmd_spconv_fwd_split_tile_rows(int(c_out)))
    return v


def split_instantiation(c_out):
    """dict(nt, ub, waves, buffers, pingpong, tables, passes): the template arguments
    msmd_spconv_fwd_split runs a layer of c_out output channels with (asked of the library:
    msmd_spconv_fwd_split_instantiation)."""
    p = (C.c_int * 7)()
    check(lib.msmd_spconv_fwd_split_instantiation(int(c_out), p),
          "msmd_spconv_fwd_split_instantiation")
    return dict(nt=p[0], ub=p[1], waves=p[2], buffers=p[3], pingpong=bool(p[4]), tables=p[5],
                passes=p[6])


def tile_prefix(nbr, rows=TILE_ROWS):
    """Stream-K work table of a neighbour table given in the order the conv kernel tiles
    it (tile order when a row order is used), for tiles of `rows` rows
    (split_tile_rows(c_out) of the layer): int32 [n_tiles + 1], see
    msmd_rulebook_tile_prefix."""
    _need_cuda(nbr)
    kvol, n = nbr.shape
    t = nbr.contiguous()
    out = torch.empty(((n + rows - 1) // rows + 1,), dtype=torch.int32, device=t.device)
    check(lib.msmd_rulebook_tile_prefix(_p(t), kvol, n, n, int(rows), _p(out), _stream()),
          "msmd_rulebook_tile_prefix")
    return out


def conv_forward_split(feat, packed_weight, nbr, n_out, c_out, planes=3, weight_flip=False,
                       row_order=None, split_tiles=True, tile_prefix=None, bn_stats=False):
    """conv_forward at bf16 MFMA rate with fp32-equivalent results: fp32 features
    are split into `planes` bf16 planes in registers, weights are pre-split
    (pack_weight_split).  With row_order, `nbr` must be in tile order (permute_cols).
    split_tiles=False withholds the exchange buffer: every 128-row tile is then one
    scheduling unit and the result does not depend on the tiling order at all (with
    it, tiles that a scheduling boundary cuts are summed in pieces: same value to the
    last bit or two).  tile_prefix (tile_prefix(nbr), with the exchange buffer): stream-K
    scheduling -- every workgroup gets the same share of the launch's work."""
    _need_cuda(feat, packed_weight, nbr)
    f = feat.contiguous().float()
    n_in, c_in = f.shape
    kvol, ld = nbr.shape
    out = torch.empty((n_out, c_out), dtype=torch.float32, device=f.device)
    counter = _tile_counter(f.device)
    nbytes = lib.msmd_spconv_fwd_split_workspace_bytes(int(n_out), int(c_out))
    ws = _exchange_buffer(f.device, nbytes) if split_tiles else None
    if tile_prefix is not None and split_tiles:
        rows = split_tile_rows(c_out)
        if tile_prefix.numel() != (int(n_out) + rows - 1) // rows + 1:
            raise ValueError("tile_prefix was not computed for %d-row tiles (K.tile_prefix(nbr, "
                             "K.split_tile_rows(c_out)))" % rows)
    # bn_stats: also the per-tile pivoted column statistics of the output ([tiles, 3, c_out]:
    # pivot, sum (x - pivot), sum (x - pivot)^2), for the BatchNorm that follows
    # (bn_act_forward(partials=...)) -> (out, partials)
    part = None
    if bn_stats and int(n_out) > 0:
        part = torch.empty((int(lib.msmd_spconv_fwd_split_stats_blocks(int(n_out), int(c_out))), 3,
                            int(c_out)), dtype=torch.float32, device=f.device)
    _launch("spconv_fwd_split", lambda: check(
        lib.msmd_spconv_fwd_split_stats(_p(f), n_in, c_in, _p(packed_weight), _p(nbr), ld,
                                        int(n_out), kvol, int(bool(weight_flip)),
                                        _p(row_order), _p(counter), counter.numel(), _p(out),
                                        int(c_out), int(planes), _p(ws),
                                        0 if ws is None else ws.numel(),
                                        _p(tile_prefix) if split_tiles else None, _p(part),
                                        _stream()), "msmd_spconv_fwd_split_stats"),
            nbr=nbr, c_in=c_in, c_out=int(c_out), n_in=n_in, n_out=int(n_out))
    return (out, part) if bn_stats else out


def conv_wgrad(feat, d_out, pairs, num, krsc_shape=None):
    """dW from the compact pair lists: [K,Cin,Cout], or laid out as the KRSC
    parameter when krsc_shape (= weight.shape) is given."""
    _need_cuda(feat, d_out, pairs, num)
    f, g = feat.contiguous().float(), d_out.contiguous().float()
    kvol, _, ld = pairs.shape
    c_in, c_out = f.shape[1], g.shape[1]
    dw = torch.empty((kvol, c_in, c_out) if krsc_shape is None else tuple(krsc_shape),
                     dtype=torch.float32, device=f.device)
    nbytes = lib.msmd_spconv_wgrad_workspace_bytes(kvol, ld, c_in, c_out)
    ws = _ws(nbytes, f.device)
    _launch("spconv_wgrad", lambda: check(
        lib.msmd_spconv_wgrad_f32(_p(f), c_in, _p(g), c_out, _p(pairs), _p(num), ld, kvol,
                                  _p(dw), int(krsc_shape is not None), _p(ws), nbytes,
                                  _stream()), "msmd_spconv_wgrad_f32"),
            num=num, c_in=c_in, c_out=c_out, n_in=f.shape[0], n_out=g.shape[0])
    return dw


def wgrad_split_supported(c_in, c_out):
    return bool(lib.msmd_spconv_wgrad_split_supported(int(c_in), int(c_out)))


# Rows per chunk of the wgrad kernel's row-chunk-major sequence; 0 (default) = offset-major.
# Measured (MI355X, tools/wgrad_ablate.py since pruned, 128 x 128 at 89.7 k rows): offset-major 263 us;
# 8192 / 4096 / 2048 / 1024-row chunks 270 / 278 / 308 / 367 us -- every (chunk, offset)
# boundary is another 64 KB partial slot for the reduction pass to read, and the main kernel
# does not get faster with its rows in L2: it is not the bandwidth-bound kernel the PMC
# traffic figure (651 MB per launch) suggested.
WGRAD_CHUNK_ROWS = int(os.environ.get("MSMD_WGRAD_CHUNK_ROWS", "0"))
WGRAD_MAX_CHUNKS = 256


def pair_segments(pairs, num, chunk_rows=None):
    """Row-chunk segment table of pair lists (pairs[K,2,ld], num[K]) for conv_wgrad_split:
    -> (table int32, n_chunks); MSMD_WGRAD_CHUNK_ROWS=0 (default) = one chunk.
    Index data: computed once per rulebook (IndiceData.pair_segments)."""
    _need_cuda(pairs, num)
    chunk_rows = WGRAD_CHUNK_ROWS if chunk_rows is None else int(chunk_rows)
    kvol, _, ld = pairs.shape
    if ld <= 0:
        return None
    if chunk_rows <= 0:          # one chunk: the offset-major sequence, its table built HERE
        chunk_rows = ld          # (index pass) instead of by every wgrad launch
    n_chunks = (ld + chunk_rows - 1) // chunk_rows
    if n_chunks > WGRAD_MAX_CHUNKS:          # very large sets: larger chunks
        chunk_rows = (ld + WGRAD_MAX_CHUNKS - 1) // WGRAD_MAX_CHUNKS
        n_chunks = (ld + chunk_rows - 1) // chunk_rows
    n_ints = int(lib.msmd_rulebook_pair_segments_ints(kvol, n_chunks))
    if n_ints == 0:      # kernel volume > 64 (5x5x5 ...): the slab wgrad kernel, which takes no table
        return None
    table = torch.empty((n_ints,),
                        dtype=torch.int32, device=pairs.device)
    check(lib.msmd_rulebook_pair_segments(_p(pairs), _p(num), ld, kvol, chunk_rows, n_chunks,
                                          _p(table), _stream()), "msmd_rulebook_pair_segments")
    return table, n_chunks


def conv_wgrad_split(feat, d_out, pairs, num, planes=3, krsc_shape=None, segments=None):
    """conv_wgrad at bf16 MFMA rate (operands split into `planes` bf16 planes in
    registers; planes=3 is fp32-equivalent).  c_in, c_out >= 64, multiples of 4.
    segments = pair_segments(pairs, num): the whole-block kernel walks the pairs row chunk by
    row chunk (all offsets of a chunk together: its rows stay in L2) instead of offset by
    offset; same sums in another fixed order."""
    _need_cuda(feat, d_out, pairs, num)
    f, g = feat.contiguous().float(), d_out.contiguous().float()
    kvol, _, ld = pairs.shape
    c_in, c_out = f.shape[1], g.shape[1]
    dw = torch.empty((kvol, c_in, c_out) if krsc_shape is None else tuple(krsc_shape),
                     dtype=torch.float32, device=f.device)
    table, n_chunks = segments if segments is not None else (None, 1)
    nbytes = lib.msmd_spconv_wgrad_segments_workspace_bytes(kvol, ld, c_in, c_out, n_chunks)
    ws = _ws(nbytes, f.device)
    _launch("spconv_wgrad_split", lambda: check(
        lib.msmd_spconv_wgrad_split_segments(_p(f), c_in, _p(g), c_out, _p(pairs), _p(num), ld,
                                             kvol, int(planes), _p(dw),
                                             int(krsc_shape is not None), _p(table),
                                             int(n_chunks), _p(ws), nbytes, _stream()),
        "msmd_spconv_wgrad_split_segments"),
            num=num, c_in=c_in, c_out=c_out, n_in=f.shape[0], n_out=g.shape[0])
    return dw


# ------------------------------------------------------------------ BN (+residual)(+ReLU)
def bn_act_forward(x, residual, gamma, beta, running_mean, running_var, training, momentum, eps,
                   relu, partials=None):
    """-> (y, save_mean, save_invstd).  partials (training only): [blocks, 3, c] pivot /
    sum (x - pivot) / sum (x - pivot)^2 per block of split_tile_rows(c) rows of x, from the
    kernel that produced x (conv_forward_split(bn_stats=True)): the statistics pass is skipped."""
    _need_cuda(x, gamma, beta)
    xx = x.contiguous().float()
    n, c = xx.shape
    dev = xx.device
    y = torch.empty_like(xx)
    stats = torch.empty((2, c), dtype=torch.float32, device=dev)
    mean, invstd = stats[0], stats[1]
    nbytes = lib.msmd_bn_workspace_bytes(n, c)
    ws = _ws(nbytes, dev)
    res = None if residual is None else residual.contiguous().float()
    if partials is not None and training:
        assert partials.shape[1:] == (3, c) and partials.is_contiguous()
    if partials is not None and training and n > 0:
        check(lib.msmd_bn_act_fwd_from_partials_f32(
            _p(xx), _p(res), n, c, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
            float(momentum), float(eps), int(bool(relu)), _p(y), _p(mean), _p(invstd),
            _p(partials), int(partials.shape[0]), split_tile_rows(c), _stream()),
            "msmd_bn_act_fwd_from_partials_f32")
        return y, mean, invstd
    check(lib.msmd_bn_act_fwd_f32(_p(xx), _p(res), n, c, _p(gamma), _p(beta), _p(running_mean),
                                  _p(running_var), int(bool(training)), float(momentum),
                                  float(eps), int(bool(relu)), _p(y), _p(mean), _p(invstd), _p(ws),
                                  nbytes, _stream()), "msmd_bn_act_fwd_f32")
    return y, mean, invstd


def bn_act_backward(x, y, dy, gamma, save_mean, save_invstd, training, relu, want_residual,
                    eps=0.0):
    """-> (dx, dresidual | None, dgamma, dbeta).  eps: the forward's -- in training mode the
    pass then takes the batch statistics again in fp64 instead of working from the float32
    save_mean / save_invstd (0: from those)."""
    _need_cuda(x, dy)
    xx, g = x.contiguous().float(), dy.contiguous().float()
    n, c = xx.shape
    dev = xx.device
    dx = torch.empty_like(xx)
    dres = torch.empty_like(xx) if want_residual else None
    dgb = torch.empty((2, c), dtype=torch.float32, device=dev)
    dgamma, dbeta = dgb[0], dgb[1]
    nbytes = lib.msmd_bn_workspace_bytes(n, c)
    ws = _ws(nbytes, dev)
    check(lib.msmd_bn_act_bwd_f32(_p(xx), _p(y), _p(g), n, c, _p(gamma), _p(save_mean),
                                  _p(save_invstd), int(bool(training)), float(eps),
                                  int(bool(relu)), _p(dx),
                                  _p(dres), _p(dgamma), _p(dbeta), _p(ws), nbytes, _stream()),
          "msmd_bn_act_bwd_f32")
    return dx, dres, dgamma, dbeta


def bn_relu_backward(x, dy, gamma, beta, save_mean, save_invstd, training, eps=0.0):
    """bn_act_backward for BatchNorm + ReLU without a residual, without reading y (the mask is
    recomputed from x: csrc/bn.hip BwdStatRecompute).  -> (dx, dgamma, dbeta)"""
    _need_cuda(x, dy)
    xx, g = x.contiguous().float(), dy.contiguous().float()
    n, c = xx.shape
    dev = xx.device
    dx = torch.empty_like(xx)
    dgb = torch.empty((2, c), dtype=torch.float32, device=dev)
    nbytes = lib.msmd_bn_workspace_bytes(n, c)
    ws = _ws(nbytes, dev)
    check(lib.msmd_bn_relu_bwd_f32(_p(xx), _p(g), n, c, _p(gamma), _p(beta), _p(save_mean),
                                   _p(save_invstd), int(bool(training)), float(eps), _p(dx),
                                   _p(dgb[0]),
                                   _p(dgb[1]), _p(ws), nbytes, _stream()), "msmd_bn_relu_bwd_f32")
    return dx, dgb[0], dgb[1]


# ------------------------------------------------------------------ dense / sets
def dense_scatter(feat, indices, batch_size, spatial_shape):
    _need_bzyx(indices)
    _need_cuda(feat, indices)
    f = feat.contiguous().float()
    n, c = f.shape
    d, h, w = [int(x) for x in spatial_shape]
    out = torch.empty((int(batch_size), c, d, h, w), dtype=torch.float32, device=f.device)
    check(lib.msmd_dense_scatter_f32(_p(f), _p(indices.contiguous().int()), n, c, int(batch_size),
                                     int3(spatial_shape), _p(out), _stream()),
          "msmd_dense_scatter_f32")
    return out


def dense_gather(dense, indices, spatial_shape):
    _need_bzyx(indices)
    _need_cuda(dense, indices)
    dn = dense.contiguous().float()
    b, c = dn.shape[0], dn.shape[1]
    n = indices.shape[0]
    feat = torch.empty((n, c), dtype=torch.float32, device=dn.device)
    check(lib.msmd_dense_gather_f32(_p(dn), _p(indices.contiguous().int()), n, c, b,
                                    int3(spatial_shape), _p(feat), _stream()),
          "msmd_dense_gather_f32")
    return feat


def bev_scatter_nhwc(feat, indices, batch_size, spatial_shape, bev, channel_offset):
    """feat rows -> channels [channel_offset, +c*D) of the zero-filled NHWC buffer
    bev [B,H,W,Ctot] (in place)."""
    _need_bzyx(indices)
    _need_cuda(feat, indices, bev)
    f = feat.contiguous().float()
    n, c = f.shape
    d, h, w = [int(x) for x in spatial_shape]
    if bev.dtype != torch.float32 or not bev.is_contiguous() or \
            tuple(bev.shape[:3]) != (int(batch_size), h, w):
        raise ValueError("bev must be a contiguous float32 [B,H,W,Ctot] buffer, got %s"
                         % (tuple(bev.shape),))
    check(lib.msmd_bev_scatter_nhwc_f32(_p(f), _p(indices.contiguous().int()), n, c,
                                        int(batch_size), int3(spatial_shape), _p(bev),
                                        int(bev.shape[3]), int(channel_offset), _stream()),
          "msmd_bev_scatter_nhwc_f32")
    return bev


def bev_gather_nhwc(bev, indices, c, batch_size, spatial_shape, channel_offset):
    _need_bzyx(indices)
    _need_cuda(bev, indices)
    if bev.dtype != torch.float32 or not bev.is_contiguous() or bev.dim() != 4:
        raise ValueError("bev must be a contiguous float32 [B,H,W,Ctot] buffer")
    n = indices.shape[0]
    feat = torch.empty((n, int(c)), dtype=torch.float32, device=bev.device)
    check(lib.msmd_bev_gather_nhwc_f32(_p(bev), _p(indices.contiguous().int()), n, int(c),
                                       int(batch_size), int3(spatial_shape), _p(feat),
                                       int(bev.shape[3]), int(channel_offset), _stream()),
          "msmd_bev_gather_nhwc_f32")
    return feat


# ------------------------------------------------------------ image-side glue
def _strides4(t):
    return (C.c_int64 * 4)(*[int(s) for s in t.stride()])


def _pixels(pixels):
    if pixels.dim() != 2 or pixels.shape[1] != 3 or \
            pixels.dtype not in (torch.float32, torch.float64):
        raise ValueError("pixels must be [n,3] float32/float64 (x, y, depth)")
    return pixels.contiguous(), int(pixels.dtype == torch.float64)


def fg_gather(img_feat, pixels, plane, downscale, pts, lidar2img, want_cells=True):
    """-> (fg_pcd [n, pts_dim+C], score_in [n, C+17], cells [n] | None, n_bad [1])"""
    _need_cuda(img_feat, pixels, plane, pts, lidar2img)
    if img_feat.dim() != 4 or img_feat.dtype != torch.float32:
        raise ValueError("img_feat must be float32 [planes, C, H, W]")
    px, is64 = _pixels(pixels)
    n = px.shape[0]
    planes, c, h, w = img_feat.shape
    pts = pts.contiguous().float()
    if pts.shape[0] != n or plane.shape[0] != n:
        raise ValueError("pixels / points / plane ids disagree on the number of points")
    l2i = lidar2img.contiguous().float().view(-1, 16)
    if l2i.shape[0] != planes:
        raise ValueError("need one 4x4 lidar2img per (sample, camera) plane")
    dev = img_feat.device
    fg = torch.empty((n, pts.shape[1] + c), dtype=torch.float32, device=dev)
    sc = torch.empty((n, c + 17), dtype=torch.float32, device=dev)
    cells = torch.empty((n,), dtype=torch.int32, device=dev) if want_cells else None
    bad = torch.empty((1,), dtype=torch.int32, device=dev)
    check(lib.msmd_fg_gather_f32(_p(img_feat), _strides4(img_feat), planes, c, h, w, _p(px), is64,
                                 _p(plane.contiguous().int()), float(downscale), _p(pts),
                                 int(pts.shape[1]), _p(l2i), n, _p(fg), _p(sc), _p(cells), _p(bad),
                                 _stream()), "msmd_fg_gather_f32")
    return fg, sc, cells, bad


def fg_gather_scored(img_feat, pixels, plane, downscale, pts, lidar2img, score_weight,
                     score_bias, n_scaled=None):
    """get_foreground2D without gradients, one launch: -> (fg_pcd [n, pts_dim+C] = [pts |
    feat * ReLU(score_net row)] for the first n_scaled points (default all), [pts | feat]
    for the rest; n_bad [1]).  score_weight [C+17] (or [1, C+17]), score_bias [1]."""
    _need_cuda(img_feat, pixels, plane, pts, lidar2img, score_weight, score_bias)
    if img_feat.dim() != 4 or img_feat.dtype != torch.float32:
        raise ValueError("img_feat must be float32 [planes, C, H, W]")
    px, is64 = _pixels(pixels)
    n = px.shape[0]
    planes, c, h, w = img_feat.shape
    pts = pts.contiguous().float()
    if pts.shape[0] != n or plane.shape[0] != n:
        raise ValueError("pixels / points / plane ids disagree on the number of points")
    l2i = lidar2img.contiguous().float().view(-1, 16)
    if l2i.shape[0] != planes:
        raise ValueError("need one 4x4 lidar2img per (sample, camera) plane")
    sw = score_weight.detach().contiguous().float().view(-1)
    sb = score_bias.detach().contiguous().float().view(-1)
    if sw.numel() != c + 17 or sb.numel() != 1:
        raise ValueError("score_net is Linear(%d, 1): got weight %s, bias %s"
                         % (c + 17, tuple(score_weight.shape), tuple(score_bias.shape)))
    dev = img_feat.device
    fg = torch.empty((n, pts.shape[1] + c), dtype=torch.float32, device=dev)
    bad = torch.empty((1,), dtype=torch.int32, device=dev)
    check(lib.msmd_fg_gather_scored_f32(_p(img_feat), _strides4(img_feat), planes, c, h, w, _p(px),
                                        is64, _p(plane.contiguous().int()), float(downscale),
                                        _p(pts), int(pts.shape[1]), _p(l2i), _p(sw), _p(sb), n,
                                        n if n_scaled is None else int(n_scaled), _p(fg), _p(bad),
                                        _stream()), "msmd_fg_gather_scored_f32")
    return fg, bad


def fg_scatter_add(grad, col0, c, cells, like):
    """Backward of fg_gather w.r.t. the feature map: zeros_like(like) + scatter."""
    _need_cuda(grad, cells, like)
    g = grad.contiguous().float()
    out = torch.zeros_like(like)
    planes, cc, h, w = like.shape
    check(lib.msmd_fg_scatter_add_f32(_p(g), int(g.shape[1]), int(col0), _p(cells),
                                      int(g.shape[0]), planes, int(c), h, w, _strides4(out),
                                      _p(out), _stream()), "msmd_fg_scatter_add_f32")
    return out


def depth_canvas(pixels, plane, planes, h, w):
    """-> (canvas [planes,h,w] float32, n_bad [1])"""
    _need_cuda(pixels, plane)
    px, is64 = _pixels(pixels)
    dev = px.device
    canvas = torch.empty((int(planes), int(h), int(w)), dtype=torch.float32, device=dev)
    bad = torch.empty((1,), dtype=torch.int32, device=dev)
    nbytes = lib.msmd_depth_canvas_workspace_bytes(int(planes), int(h), int(w))
    ws = _ws(nbytes, dev)
    check(lib.msmd_depth_canvas_f32(_p(px), is64, _p(plane.contiguous().int()), int(px.shape[0]),
                                    int(planes), int(h), int(w), _p(canvas), _p(bad), _p(ws),
                                    nbytes, _stream()), "msmd_depth_canvas_f32")
    return canvas, bad


# ------------------------------------------------ head targets / loss (row f3)
def boxes_overlap_bev(boxes_a, boxes_b):
    """iou3d_cuda.boxes_overlap_bev_gpu: rotated rectangles (x1, y1, x2, y2, angle) ->
    overlap AREAS [na, nb]."""
    _need_cuda(boxes_a, boxes_b)
    a, b = boxes_a.contiguous().float(), boxes_b.contiguous().float()
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != 5 or b.shape[1] != 5:
        raise ValueError("boxes must be [n,5] (x1, y1, x2, y2, angle)")
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    check(lib.msmd_boxes_overlap_bev_f32(_p(a), a.shape[0], _p(b), b.shape[0], _p(out), _stream()),
          "msmd_boxes_overlap_bev_f32")
    return out


def boxes_iou3d(boxes_a, boxes_b, nb_valid=None, mode="iou"):
    """BaseInstance3DBoxes.overlaps for LiDAR boxes (x, y, z_bottom, dx, dy, dz, yaw, ...).
    [na, ca] x [nb, cb] -> [na, nb], or batched [B, na, ca] x [B, nb, cb] (+ nb_valid [B]:
    rows of boxes_b in use per sample) -> [B, na, nb]."""
    _need_cuda(boxes_a, boxes_b)
    if mode not in ("iou", "iof"):
        raise ValueError("mode must be 'iou' or 'iof'")
    a, b = boxes_a.contiguous().float(), boxes_b.contiguous().float()
    single = a.dim() == 2
    if single:
        a, b = a[None], b[None]
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[2] < 7 or b.shape[2] < 7:
        raise ValueError("boxes must be [B,n,>=7] with equal B (or [n,>=7])")
    batch, na, nb = a.shape[0], a.shape[1], b.shape[1]
    if nb_valid is not None:
        _need_cuda(nb_valid)
        nb_valid = nb_valid.contiguous().int()
        if nb_valid.numel() != batch:
            raise ValueError("nb_valid must hold one count per sample")
    out = torch.empty((batch, na, nb), dtype=torch.float32, device=a.device)
    check(lib.msmd_boxes_iou3d_f32(_p(a), a.shape[2], _p(b), b.shape[2],
                                   _p(nb_valid) if nb_valid is not None else None, batch, na, nb,
                                   0 if mode == "iou" else 1, _p(out), _stream()),
          "msmd_boxes_iou3d_f32")
    return out[0] if single else out


def heatmap_gaussian(heatmap, plane, center_x, center_y, radius):
    """heatmap [planes, H, W] (or [B, C, H, W]) float32, updated in place: maximum with one
    Gaussian bump per box (plane = sample * C + class; plane < 0 or radius < 0 skips)."""
    _need_cuda(heatmap, plane, center_x, center_y, radius)
    if heatmap.dtype != torch.float32 or not heatmap.is_contiguous() or heatmap.dim() < 3:
        raise ValueError("heatmap must be a contiguous float32 [..., H, W] buffer")
    h, w = heatmap.shape[-2:]
    planes = heatmap.numel() // (h * w)
    n = plane.numel()
    args = [t.contiguous().int() for t in (plane, center_x, center_y, radius)]
    if any(t.numel() != n for t in args):
        raise ValueError("plane / center / radius must have one entry per box")
    check(lib.msmd_heatmap_gaussian_f32(_p(args[0]), _p(args[1]), _p(args[2]), _p(args[3]), n,
                                        planes, h, w, _p(heatmap), _stream()),
          "msmd_heatmap_gaussian_f32")
    return heatmap


def gaussian_focal(logits, target, clip=1e-4, want_grad=True):
    """clip_sigmoid + GaussianFocalLoss(alpha=2, gamma=4), unreduced sums.
    -> (sums [2] = (sum of losses, cells with target == 1), grad like logits | None)"""
    _need_cuda(logits, target)
    x, t = logits.contiguous().float(), target.contiguous().float()
    if x.shape != t.shape:
        raise ValueError("logits and target must have the same shape")
    n = x.numel()
    sums = torch.empty((2,), dtype=torch.float32, device=x.device)
    grad = torch.empty_like(x) if want_grad else None
    nbytes = lib.msmd_gaussian_focal_workspace_bytes(n)
    ws = _ws(nbytes, x.device)
    check(lib.msmd_gaussian_focal_f32(_p(x), _p(t), n, float(clip),
                                      _p(grad) if grad is not None else None, _p(sums), _p(ws),
                                      nbytes, _stream()), "msmd_gaussian_focal_f32")
    return sums, grad


# ------------------------------------------------ iou3d: BEV IoU and NMS (row n2)
def boxes_iou_bev(boxes_a, boxes_b):
    """iou3d_cuda.boxes_iou_bev_gpu: rotated rectangles (x1, y1, x2, y2, angle) -> IoU [na, nb]."""
    _need_cuda(boxes_a, boxes_b)
    a, b = boxes_a.contiguous().float(), boxes_b.contiguous().float()
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != 5 or b.shape[1] != 5:
        raise ValueError("boxes must be [n,5] (x1, y1, x2, y2, angle)")
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    check(lib.msmd_boxes_iou_bev_f32(_p(a), a.shape[0], _p(b), b.shape[0], _p(out), _stream()),
          "msmd_boxes_iou_bev_f32")
    return out


NMS_KINDS = {"rotate": 0, "rotated": 0, "normal": 1, "circle": 2}
NMS_ALIGNED3D = "aligned3d"      # its own entry point (msmd_nms_aligned3d_f32), not a kind code
NMS_MMCV = "mmcv"                # likewise (msmd_nms_mmcv_f32): mmcv.ops.nms's pair test
NMS_MAX_SEGMENT = 16384


def nms_workspace_bytes(total_boxes, max_segment):
    return lib.msmd_nms_workspace_bytes(int(total_boxes), int(max_segment))


def nms_segments(kind, boxes, offsets, thresh, max_segment, post_max=None, order=None,
                 keep=None, num_keep=None, workspace=None):
    """Greedy NMS of every segment in one call (two launches, nothing read back).
    boxes [total, >= 5 | 4 | 2] float32 ('aligned3d': [total, >= 7] rows x1, y1, z1, x2, y2, z2,
    class; 'mmcv': [total, >= 4] rows x1, y1, x2, y2 already shifted by class), each segment
    (rows offsets[s] .. offsets[s+1], int32 [S + 1] on the device) already in descending score
    order; only the first `max_segment`
    rows of a segment take part.  thresh: float32 [S] on the device.  order (optional, long
    [total]): the caller's sort permutation -- kept rows are then reported as order[row].
    -> (keep long [S, min(post_max, max_segment)], -1 past num_keep[s]; num_keep int32 [S]).
    keep / num_keep / workspace (uint8, nms_workspace_bytes) may be passed in: with all three
    the call allocates nothing."""
    _need_cuda(boxes, offsets, thresh, order, keep, num_keep, workspace)
    code = None if kind in (NMS_ALIGNED3D, NMS_MMCV) else NMS_KINDS[kind]
    if boxes.dtype != torch.float32 or boxes.dim() != 2 or not boxes.is_contiguous():
        raise ValueError("boxes must be a contiguous float32 [total, columns] tensor")
    if offsets.dtype != torch.int32 or thresh.dtype != torch.float32:
        raise ValueError("offsets must be int32 and thresh float32")
    segments = offsets.numel() - 1
    if segments < 0 or thresh.numel() != segments:
        raise ValueError("offsets holds S + 1 entries and thresh S")
    total, max_segment = boxes.shape[0], int(max_segment)
    if max_segment > NMS_MAX_SEGMENT:
        raise ValueError("NMS handles at most %d boxes per segment (got %d): set pre_max"
                         % (NMS_MAX_SEGMENT, max_segment))
    stride = max_segment if post_max is None else min(int(post_max), max_segment)
    post = stride
    if order is not None and (order.dtype != torch.long or order.numel() != total):
        raise ValueError("order must be a long tensor with one entry per box")
    if keep is None:
        keep = torch.empty((segments, stride), dtype=torch.long, device=boxes.device)
    elif keep.dtype != torch.long or tuple(keep.shape) != (segments, stride) \
            or not keep.is_contiguous():
        raise ValueError("keep must be a contiguous long [%d, %d] tensor" % (segments, stride))
    if num_keep is None:
        num_keep = torch.empty((segments,), dtype=torch.int32, device=boxes.device)
    elif num_keep.dtype != torch.int32 or num_keep.numel() != segments:
        raise ValueError("num_keep must be an int32 [%d] tensor" % segments)
    nbytes = lib.msmd_nms_workspace_bytes(total, max_segment)
    ws = _ws(nbytes, boxes.device) if workspace is None else workspace
    if ws.numel() * ws.element_size() < nbytes:
        raise ValueError("workspace holds %d bytes, %d needed" % (ws.numel(), nbytes))
    if kind == NMS_MMCV:
        check(lib.msmd_nms_mmcv_f32(_p(boxes), boxes.shape[1], _p(offsets.contiguous()), segments,
                                    total, max_segment, _p(thresh.contiguous()), post, _p(order),
                                    _p(keep), stride, _p(num_keep), _p(ws), nbytes, _stream()),
              "msmd_nms_mmcv_f32")
        return keep, num_keep
    if code is None:
        check(lib.msmd_nms_aligned3d_f32(_p(boxes), boxes.shape[1], _p(offsets.contiguous()),
                                         segments, total, max_segment, _p(thresh.contiguous()),
                                         post, _p(order), _p(keep), stride, _p(num_keep), _p(ws),
                                         nbytes, _stream()), "msmd_nms_aligned3d_f32")
        return keep, num_keep
    check(lib.msmd_nms_batched_f32(code, _p(boxes), boxes.shape[1], _p(offsets.contiguous()),
                                   segments, total, max_segment, _p(thresh.contiguous()), post,
                                   _p(order), _p(keep), stride, _p(num_keep), _p(ws), nbytes,
                                   _stream()), "msmd_nms_batched_f32")
    return keep, num_keep


# ------------------------------------------------ VoteNet ops (row n4)
CHAMFER_MODES = {"l2": 0, "l1": 1, "smooth_l1": 2}


def _chamfer_sets(src, dst):
    _need_cuda(src, dst)
    for t, what in ((src, "src"), (dst, "dst")):
        _need_dtype(t, torch.float32, what)
        if t.dim() != 3 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float32 [B, N, 3] tensor, got %s"
                             % (what, tuple(t.shape)))
    if src.shape[0] != dst.shape[0] or src.shape[2] != dst.shape[2]:
        raise ValueError("src %s and dst %s need the same batch size and channels"
                         % (tuple(src.shape), tuple(dst.shape)))
    return src.shape[0], src.shape[1], dst.shape[1], src.shape[2]


def chamfer_forward(src, dst, mode):
    """src [B, N, 3], dst [B, M, 3] float32 -> (d1 [B, N], i1 long [B, N], d2 [B, M], i2 long
    [B, M]): each point's smallest criterion distance to the other set and where it is
    (torch.min's tie and NaN rules).  Two launches, no [N, M] buffer."""
    b, n, m, c = _chamfer_sets(src, dst)
    dev = src.device
    d1 = torch.empty((b, n), dtype=torch.float32, device=dev)
    d2 = torch.empty((b, m), dtype=torch.float32, device=dev)
    i1 = torch.empty((b, n), dtype=torch.long, device=dev)
    i2 = torch.empty((b, m), dtype=torch.long, device=dev)
    check(lib.msmd_chamfer_fwd_f32(_p(src), _p(dst), b, n, m, c, CHAMFER_MODES[mode], _p(d1),
                                   _p(i1), _p(d2), _p(i2), _stream()), "msmd_chamfer_fwd_f32")
    return d1, i1, d2, i2


def chamfer_backward(src, dst, g1, g2, i1, i2, mode, want_src=True, want_dst=True):
    """-> (grad_src [B, N, 3] | None, grad_dst [B, M, 3] | None) for upstream g1 [B, N] and
    g2 [B, M]; fixed summation order, no atomics."""
    b, n, m, c = _chamfer_sets(src, dst)
    _need_cuda(g1, g2, i1, i2)
    for t, dt, shape, what in ((g1, torch.float32, (b, n), "g1"), (g2, torch.float32, (b, m), "g2"),
                               (i1, torch.long, (b, n), "i1"), (i2, torch.long, (b, m), "i2")):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s %s tensor" % (what, dt, shape))
    if not (want_src or want_dst):
        return None, None
    grad_src = torch.empty_like(src) if want_src else None
    grad_dst = torch.empty_like(dst) if want_dst else None
    check(lib.msmd_chamfer_bwd_f32(_p(src), _p(dst), _p(g1), _p(g2), _p(i1), _p(i2), b, n, m, c,
                                   CHAMFER_MODES[mode], _p(grad_src), _p(grad_dst), _stream()),
          "msmd_chamfer_bwd_f32")
    return grad_src, grad_dst


def vote_targets(points, point_offsets, boxes, centers, box_offsets, max_points=None,
                 gt_per_seed=3):
    """VoteHead.get_targets_single's box-form vote targets for every sample in one launch.
    points float32 [P, >= 3] rows, sample s = rows point_offsets[s] .. point_offsets[s+1] (int32
    [S + 1] on the device); boxes float32 [T, 7] in the points_in_boxes frame with gravity
    `centers` [T, 3] and box_offsets likewise.  max_points: a host-known bound on a sample's
    points (sizes the grid only).  -> (vote_targets float32 [P, 9], vote_mask long [P])."""
    _need_cuda(points, point_offsets, boxes, centers, box_offsets)
    for t, w, what in ((points, None, "points"), (boxes, 7, "boxes"), (centers, 3, "centers")):
        _need_dtype(t, torch.float32, what)
        if t.dim() != 2 or not t.is_contiguous() or (w is not None and t.shape[1] != w):
            raise ValueError("%s must be a contiguous float32 [rows, %s] tensor, got %s"
                             % (what, w or ">= 3", tuple(t.shape)))
    if boxes.shape[0] != centers.shape[0]:
        raise ValueError("one gravity centre per box")
    for t in (point_offsets, box_offsets):
        _need_dtype(t, torch.int32, "offsets")
    samples = point_offsets.numel() - 1
    if samples < 0 or box_offsets.numel() != samples + 1:
        raise ValueError("point_offsets and box_offsets hold S + 1 entries each")
    total = points.shape[0]
    targets = torch.empty((total, 3 * int(gt_per_seed)), dtype=torch.float32, device=points.device)
    mask = torch.empty((total,), dtype=torch.long, device=points.device)
    check(lib.msmd_vote_targets_f32(_p(points), points.shape[1], _p(point_offsets.contiguous()),
                                    _p(boxes), _p(centers), _p(box_offsets.contiguous()), samples,
                                    total, boxes.shape[0],
                                    total if max_points is None else int(max_points),
                                    int(gt_per_seed), _p(targets), _p(mask), _stream()),
          "msmd_vote_targets_f32")
    return targets, mask


def points_in_boxes_count(boxes, pts):
    """boxes [B, T, 7], pts [B, M, >= 3] float32 -> int32 [B, T]: the sample's points inside
    each box (the points_in_boxes predicate), without the [B, M, T] table."""
    _need_cuda(boxes, pts)
    for t, what in ((boxes, "boxes"), (pts, "points")):
        _need_dtype(t, torch.float32, what)
        if t.dim() != 3 or not t.is_contiguous():
            raise RuntimeError("%s must be a contiguous [B, N, C] float32 tensor" % what)
    if boxes.shape[2] != 7 or pts.shape[2] < 3 or boxes.shape[0] != pts.shape[0]:
        raise RuntimeError("boxes [B, T, 7] and points [B, M, >= 3] expected, got %s and %s"
                           % (tuple(boxes.shape), tuple(pts.shape)))
    b, t, m = boxes.shape[0], boxes.shape[1], pts.shape[1]
    count = torch.empty((b, t), dtype=torch.int32, device=pts.device)
    check(lib.msmd_points_in_boxes_count_f32(_p(boxes), _p(pts), pts.shape[2], b, t, m, _p(count),
                                             _stream()), "msmd_points_in_boxes_count_f32")
    return count


# ------------------------------------------------ 3DSSD candidate targets (row n5)
SSD3D_GT_CHUNK = lib.msmd_ssd3d_gt_chunk()
SSD3D_TABLE_WIDTH = 33      # centre 3, half sizes 3, direction residual 1, sin / cos 2, corners 24
SSD3D_TARGET_NAMES = ("vote_targets", "center_targets", "size_res_targets", "dir_class_targets",
                      "dir_res_targets", "mask_targets", "centerness_targets", "corner3d_targets",
                      "vote_mask", "positive_mask", "negative_mask")


def ssd3d_targets(aggregated, seeds, gt_boxes, vote_boxes, labels, box_offsets, box_table,
                  dir_class, num_classes, pos_distance_thr):
    """SSD3DHead.get_targets_single for every sample in one launch (msmd_ssd3d_targets_f32).
    aggregated float32 [B, N, 3]; seeds float32 [B, >= N, 3] (the first N of each sample are
    read; a view with a sample stride is taken as it is); gt_boxes / vote_boxes float32 [T, 7] in
    the points_in_boxes frame, labels long [T] (-1: the row does not exist), box_offsets int32
    [B + 1] on the device; box_table float32 [T, 33] and dir_class long [T] as msmd_hip.h lays
    them out.  -> the reference's eleven per-sample results stacked, in its order
    (SSD3D_TARGET_NAMES); center_targets are absolute; the three masks are bool."""
    _need_cuda(aggregated, seeds, gt_boxes, vote_boxes, labels, box_offsets, box_table, dir_class)
    _need_dtype(aggregated, torch.float32, "aggregated")
    _need_dtype(seeds, torch.float32, "seeds")
    if aggregated.dim() != 3 or aggregated.shape[2] != 3 or not aggregated.is_contiguous():
        raise ValueError("aggregated must be a contiguous float32 [B, N, 3] tensor, got %s"
                         % (tuple(aggregated.shape),))
    batch, n = aggregated.shape[:2]
    if seeds.dim() != 3 or seeds.shape[0] != batch or seeds.shape[1] < n or seeds.shape[2] != 3:
        raise ValueError("seeds must be [B, >= N, 3], got %s" % (tuple(seeds.shape),))
    if seeds.numel() and (seeds.stride(2) != 1 or seeds.stride(1) != 3 or
                          (batch > 1 and seeds.stride(0) < n * 3)):
        seeds = seeds[:, :n].contiguous()
    seed_stride = seeds.stride(0) if batch > 1 else max(seeds.shape[1], n) * 3
    total = gt_boxes.shape[0]
    for t, w, what in ((gt_boxes, 7, "gt_boxes"), (vote_boxes, 7, "vote_boxes"),
                       (box_table, SSD3D_TABLE_WIDTH, "box_table")):
        _need_dtype(t, torch.float32, what)
        if t.dim() != 2 or tuple(t.shape) != (total, w) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float32 [%d, %d] tensor, got %s"
                             % (what, total, w, tuple(t.shape)))
    for t, what in ((labels, "labels"), (dir_class, "dir_class")):
        _need_dtype(t, torch.long, what)
        if t.dim() != 1 or t.numel() != total or not t.is_contiguous():
            raise ValueError("%s must be a contiguous long [%d] tensor" % (what, total))
    _need_dtype(box_offsets, torch.int32, "box_offsets")
    if box_offsets.numel() != batch + 1:
        raise ValueError("box_offsets holds B + 1 entries")
    dev, classes = aggregated.device, int(num_classes)
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)       # noqa: E731
    l = lambda *shape: torch.empty(shape, dtype=torch.long, device=dev)          # noqa: E731,E741
    u = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)         # noqa: E731
    vote, center, size = f(batch, n, 3), f(batch, n, 3), f(batch, n, 3)
    dcls, dres, mask = l(batch, n), f(batch, n), l(batch, n)
    cness, corners = f(batch, n, classes), f(batch, n, 8, 3)
    vmask, pos, neg = u(batch, n), u(batch, n), u(batch, n)
    check(lib.msmd_ssd3d_targets_f32(
        _p(aggregated), _p(seeds), seed_stride, _p(gt_boxes), _p(vote_boxes), _p(labels),
        _p(box_offsets.contiguous()), _p(box_table), SSD3D_TABLE_WIDTH, _p(dir_class), batch, n,
        total, classes, float(pos_distance_thr), _p(vote), _p(center), _p(size), _p(dcls),
        _p(dres), _p(mask), _p(cness), _p(corners), _p(vmask), _p(pos), _p(neg), _stream()),
        "msmd_ssd3d_targets_f32")
    return (vote, center, size, dcls, dres, mask, cness, corners, vmask.view(torch.bool),
            pos.view(torch.bool), neg.view(torch.bool))


# ------------------------------------------------ Anchor3DHead targets / loss (row n3)
ANCHOR_MAX_SEGMENTS = lib.msmd_anchor_max_segments()
ANCHOR_GT_CHUNK = lib.msmd_anchor_gt_chunk()


def _host_ints(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def _gt_lists(gt_index, gt_offsets, segments, num_gt):
    _need_cuda(gt_index, gt_offsets)
    if gt_offsets.dtype != torch.int32 or gt_offsets.numel() != segments + 1:
        raise ValueError("gt_offsets must be an int32 tensor of one entry per segment plus one")
    if gt_index is None:
        return None, int(num_gt)
    if gt_index.dtype != torch.int32:
        raise ValueError("gt_index must be int32")
    return gt_index.contiguous(), int(gt_index.numel())


def anchor_assign(anchor_bev, anchor_offsets, gt_bev, gt_offsets, pos_iou_thr, neg_iou_thr,
                  min_pos_iou, gt_index=None):
    """MaxIoUAssigner over nearest-BEV boxes for every (sample, assigner group) segment in one
    call, without the IoU matrix and with nothing read back (include/msmd_hip.h, row n3).
    anchor_bev [rows, 4] float32 (x1, y1, x2, y2), shared by the samples: output row r uses
    anchor row r % rows.  anchor_offsets: a HOST sequence [S + 1], ascending from 0.  gt_bev
    [G, 4]; gt_offsets int32 [S + 1] on the device, into gt_index (int32, device) or, without
    it, into gt_bev itself.  Thresholds: one float per segment (host).
    -> assigned_gt int32 [total] (-1 ignored, 0 negative, i + 1 positive with i local to the
       segment's list), max_overlaps float32 [total], num_pos int32 [S]."""
    _need_cuda(anchor_bev, gt_bev)
    offs = [int(v) for v in anchor_offsets]
    segments = len(offs) - 1
    if segments < 0 or not (len(pos_iou_thr) == len(neg_iou_thr) == len(min_pos_iou) == segments):
        raise ValueError("anchor_offsets holds S + 1 entries and every threshold list S")
    a, g = anchor_bev.contiguous(), gt_bev.contiguous()
    if a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != 4 or g.dtype != torch.float32 \
            or g.dim() != 2 or g.shape[1] != 4:
        raise ValueError("anchor_bev and gt_bev must be float32 [n, 4] (x1, y1, x2, y2)")
    gt_index, entries = _gt_lists(gt_index, gt_offsets, segments, g.shape[0])
    total = offs[-1] if segments >= 0 and offs else 0
    dev = a.device
    assigned = torch.empty((max(total, 0),), dtype=torch.int32, device=dev)
    overlaps = torch.empty((max(total, 0),), dtype=torch.float32, device=dev)
    num_pos = torch.empty((segments,), dtype=torch.int32, device=dev)
    nbytes = lib.msmd_anchor_assign_workspace_bytes(entries)
    ws = _ws(nbytes, dev)
    check(lib.msmd_anchor_assign_f32(_p(a), a.shape[0], _host_ints(offs), segments, _p(g),
                                     g.shape[0], _p(gt_index), _p(gt_offsets.contiguous()),
                                     entries, float_arr(pos_iou_thr), float_arr(neg_iou_thr),
                                     float_arr(min_pos_iou), _p(assigned), _p(overlaps),
                                     _p(num_pos), _p(ws), nbytes, _stream()),
          "msmd_anchor_assign_f32")
    return assigned, overlaps, num_pos


def anchor_targets(assigned_gt, anchors, anchor_offsets, gt_boxes, gt_labels, gt_offsets,
                   num_classes, pos_weight=-1.0, dir_offset=0.0, gt_index=None, dest=None):
    """The tensors anchor_target_single_assigner writes, for every segment at once, from
    anchor_assign's assigned_gt.  anchors [rows, code], gt_boxes [G, code] float32, gt_labels
    long [G]; dest (int32 [rows], device): where row r of a sample lands in that sample's
    output (the reference's size-interleaved order).
    -> labels long [total], label_weights, bbox_targets [total, code], bbox_weights,
       dir_targets long [total], dir_weights."""
    _need_cuda(assigned_gt, anchors, gt_boxes, gt_labels, dest)
    offs = [int(v) for v in anchor_offsets]
    segments = len(offs) - 1
    a, g = anchors.contiguous(), gt_boxes.contiguous()
    if a.dtype != torch.float32 or g.dtype != torch.float32 or a.dim() != 2 or g.dim() != 2 \
            or a.shape[1] != g.shape[1]:
        raise ValueError("anchors and gt_boxes must be float32 [n, code] with one code size")
    if gt_labels.dtype != torch.long or gt_labels.numel() != g.shape[0]:
        raise ValueError("gt_labels must be a long tensor with one entry per box")
    total = offs[-1]
    if assigned_gt.dtype != torch.int32 or assigned_gt.numel() != total:
        raise ValueError("assigned_gt must be int32 with one entry per output row")
    if dest is not None and (dest.dtype != torch.int32 or dest.numel() != a.shape[0]):
        raise ValueError("dest must be int32 with one entry per anchor row")
    gt_index, entries = _gt_lists(gt_index, gt_offsets, segments, g.shape[0])
    dev, code = a.device, a.shape[1]
    labels = torch.empty((total,), dtype=torch.long, device=dev)
    label_weights = torch.empty((total,), dtype=torch.float32, device=dev)
    bbox_targets = torch.empty((total, code), dtype=torch.float32, device=dev)
    bbox_weights = torch.empty((total, code), dtype=torch.float32, device=dev)
    dir_targets = torch.empty((total,), dtype=torch.long, device=dev)
    dir_weights = torch.empty((total,), dtype=torch.float32, device=dev)
    check(lib.msmd_anchor_targets_f32(
        _p(assigned_gt.contiguous()), _p(a), a.shape[0], code, _host_ints(offs), segments, _p(g),
        _p(gt_labels.contiguous()), g.shape[0], _p(gt_index), _p(gt_offsets.contiguous()), entries,
        _p(dest), int(num_classes), float(pos_weight), float(dir_offset), _p(labels),
        _p(label_weights), _p(bbox_targets), _p(bbox_weights), _p(dir_targets), _p(dir_weights),
        _stream()), "msmd_anchor_targets_f32")
    return labels, label_weights, bbox_targets, bbox_weights, dir_targets, dir_weights


def sigmoid_focal(logits, labels, weights, gamma=2.0, alpha=0.25, want_grad=True):
    """mmdet FocalLoss(use_sigmoid=True), weighted and summed: logits [N, C] float32, labels
    long [N] (background = C), weights float32 [N].
    -> (sum float32 [1], grad like logits | None)"""
    _need_cuda(logits, labels, weights)
    x = logits.contiguous()
    if x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError("logits must be float32 [N, C]")
    n, c = x.shape
    if labels.dtype != torch.long or labels.numel() != n or weights.dtype != torch.float32 \
            or weights.numel() != n:
        raise ValueError("labels (long) and weights (float32) hold one entry per row of logits")
    total = torch.empty((1,), dtype=torch.float32, device=x.device)
    grad = torch.empty_like(x) if want_grad else None
    nbytes = lib.msmd_sigmoid_focal_workspace_bytes(n, c)
    ws = _ws(nbytes, x.device)
    check(lib.msmd_sigmoid_focal_f32(_p(x), _p(labels.contiguous()), _p(weights.contiguous()), n, c,
                                     float(gamma), float(alpha), _p(grad), _p(total), _p(ws),
                                     nbytes, _stream()), "msmd_sigmoid_focal_f32")
    return total, grad


# ------------------------------------------------ FreeAnchor3DHead loss (row n6)
FREE_ANCHOR_MAX_TOPK = lib.msmd_free_anchor_max_topk()


def _f32_rows(t, cols, what):
    t = t.contiguous()
    if t.dtype != torch.float32 or t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        raise ValueError("%s must be float32 [n, %s]" % (what, cols if cols else "c"))
    return t


def decode_nearest_bev(anchors, deltas):
    """DeltaXYZWLHRBBoxCoder.decode followed by nearest_bev for every (sample, anchor):
    anchors [A, code] float32 shared by the samples, deltas [B * A, code] -> pred_bev [B * A, 4]
    (x1, y1, x2, y2).  Only the five decoded members the BEV box needs are computed."""
    _need_cuda(anchors, deltas)
    a, d = _f32_rows(anchors, None, "anchors"), _f32_rows(deltas, None, "deltas")
    if a.shape[1] != d.shape[1] or a.shape[0] == 0 or d.shape[0] % a.shape[0]:
        raise ValueError("deltas holds a whole number of samples of the anchors' rows and code")
    out = torch.empty((d.shape[0], 4), dtype=torch.float32, device=d.device)
    check(lib.msmd_decode_nearest_bev_f32(_p(a), a.shape[0], a.shape[1], _p(d),
                                          d.shape[0] // a.shape[0], _p(out), _stream()),
          "msmd_decode_nearest_bev_f32")
    return out


def free_anchor_box_prob(pred_bev, gt_bev, gt_labels, gt_offsets, num_classes, bbox_thr):
    """P{anchor j in A+} of FreeAnchor for a whole batch, without the [G, A] IoU matrix
    (include/msmd_hip.h, row n6).  pred_bev [B * A, 4]; gt_bev [G, 4], gt_labels long [G];
    gt_offsets int32 [B + 1] on the device.  -> box_prob float32 [B * A, num_classes]."""
    _need_cuda(pred_bev, gt_bev, gt_labels, gt_offsets)
    p, g = _f32_rows(pred_bev, 4, "pred_bev"), _f32_rows(gt_bev, 4, "gt_bev")
    if gt_offsets.dtype != torch.int32 or gt_offsets.numel() < 2:
        raise ValueError("gt_offsets must be an int32 tensor of one entry per sample plus one")
    batch = gt_offsets.numel() - 1
    if p.shape[0] % batch:
        raise ValueError("pred_bev holds a whole number of anchors per sample")
    if gt_labels.dtype != torch.long or gt_labels.numel() != g.shape[0]:
        raise ValueError("gt_labels must be a long tensor with one entry per box")
    out = torch.empty((p.shape[0], int(num_classes)), dtype=torch.float32, device=p.device)
    nbytes = lib.msmd_free_anchor_box_prob_workspace_bytes(g.shape[0])
    ws = _ws(nbytes, p.device)
    check(lib.msmd_free_anchor_box_prob_f32(
        _p(p), batch, p.shape[0] // batch, _p(g), _p(gt_labels.contiguous()), g.shape[0],
        _p(gt_offsets.contiguous()), int(num_classes), float(bbox_thr), _p(out), _p(ws), nbytes,
        _stream()), "msmd_free_anchor_box_prob_f32")
    return out


def free_anchor_topk(anchor_bev, gt_bev, k):
    """The bags of FreeAnchor: for every ground truth the k anchors of largest nearest-BEV IoU
    (ties to the lower anchor index, NaN largest), each row in ascending anchor index, without
    the [G, A] matrix.  anchor_bev [A, 4], gt_bev [G, 4] -> matched int32 [G, k]."""
    _need_cuda(anchor_bev, gt_bev)
    a, g = _f32_rows(anchor_bev, 4, "anchor_bev"), _f32_rows(gt_bev, 4, "gt_bev")
    k = int(k)
    if k > a.shape[0]:
        raise ValueError("free_anchor_topk: k = %d exceeds the %d anchors (the reference's "
                         "torch.topk raises there too)" % (k, a.shape[0]))
    if k < 1 or k > FREE_ANCHOR_MAX_TOPK:
        raise ValueError("free_anchor_topk: k = %d outside [1, %d]" % (k, FREE_ANCHOR_MAX_TOPK))
    out = torch.empty((g.shape[0], k), dtype=torch.int32, device=a.device)
    nbytes = lib.msmd_free_anchor_topk_workspace_bytes(a.shape[0], g.shape[0])
    ws = _ws(nbytes, a.device)
    check(lib.msmd_free_anchor_topk(_p(a), a.shape[0], _p(g), g.shape[0], k, _p(out), _p(ws),
                                    nbytes, _stream()), "msmd_free_anchor_topk")
    return out


def free_anchor_negative(logits, box_prob, gamma=2.0, alpha=0.5, want_grad=True):
    """FreeAnchor's negative bag loss, summed: (1 - alpha) p^gamma BCE(p, 0) with
    p = clamp(sigmoid(logits) (1 - box_prob), 0, 1); logits and box_prob float32 [N, C].
    -> (sum float32 [1], grad like logits | None)"""
    _need_cuda(logits, box_prob)
    x, q = _f32_rows(logits, None, "logits"), _f32_rows(box_prob, None, "box_prob")
    if x.shape != q.shape:
        raise ValueError("logits and box_prob must have one shape")
    if not gamma >= 1:
        raise ValueError("free_anchor_negative: gamma = %r < 1 (the gradient at p = 0 is "
                         "unbounded)" % (gamma,))
    n, c = x.shape
    total = torch.empty((1,), dtype=torch.float32, device=x.device)
    grad = torch.empty_like(x) if want_grad else None
    nbytes = lib.msmd_free_anchor_negative_workspace_bytes(n, c)
    ws = _ws(nbytes, x.device)
    check(lib.msmd_free_anchor_negative_f32(_p(x), _p(q), n, c, float(gamma), float(alpha),
                                            _p(grad), _p(total), _p(ws), nbytes, _stream()),
          "msmd_free_anchor_negative_f32")
    return total, grad


def _sparse_add_fill(feat_a, idx_a, feat_b, idx_b, batch_size, spatial_shape, m, ws_addr,
                     ws_bytes):
    """The union set (m rows) counted into the workspace at ws_addr -> (out_indices, out_feat,
    map_a, map_b) in ONE fill launch set; without features (None) the index half alone."""
    na, nb, dev = idx_a.shape[0], idx_b.shape[0], idx_a.device
    c = 0 if feat_a is None else feat_a.shape[1]
    oi = torch.empty((m, 4), dtype=torch.int32, device=dev)
    of = None if feat_a is None else torch.empty((m, c), dtype=torch.float32, device=dev)
    ma = torch.empty((na,), dtype=torch.int32, device=dev)
    mb = torch.empty((nb,), dtype=torch.int32, device=dev)
    check(lib.msmd_sparse_add_fill(_p(feat_a), _p(idx_a), na, _p(feat_b), _p(idx_b), nb, c,
                                   int(batch_size), int3(spatial_shape), m, _p(oi), _p(of), _p(ma),
                                   _p(mb), ws_addr, ws_bytes, _stream()), "msmd_sparse_add_fill")
    return oi, of, ma, mb


def sparse_add(feat_a, idx_a, feat_b, idx_b, batch_size, spatial_shape):
    """-> (out_indices, out_feat, map_a, map_b); without features (None, as sparse_add_index
    calls it) the index half alone, out_feat = None."""
    _need_bzyx(idx_a, idx_b)
    _need_cuda(feat_a, idx_a, feat_b, idx_b)
    if feat_a is not None:
        feat_a, feat_b = feat_a.contiguous().float(), feat_b.contiguous().float()
    ia, ib = idx_a.contiguous().int(), idx_b.contiguous().int()
    nbytes = lib.msmd_sparse_add_workspace_bytes(int(batch_size), int3(spatial_shape))
    ws = _ws(nbytes, ia.device)
    count = _Count(ia.device)
    check(lib.msmd_sparse_add_count(_p(ia), ia.shape[0], _p(ib), ib.shape[0], int(batch_size),
                                    int3(spatial_shape), count.ptr, _p(ws), nbytes, _stream()),
          "msmd_sparse_add_count")
    return _sparse_add_fill(feat_a, ia, feat_b, ib, batch_size, spatial_shape, count.read(),
                            _p(ws), nbytes)


def sparse_add_index(idx_a, idx_b, batch_size, spatial_shape):
    """Index half of sparse_add -> (out_indices[m,4], map_a[na], map_b[nb])."""
    oi, _, ma, mb = sparse_add(None, idx_a, None, idx_b, batch_size, spatial_shape)
    return oi, ma, mb


def sparse_add_rows(feat_a, map_a, feat_b, map_b, n_out):
    """Feature half of sparse_add with the maps of sparse_add_index (no host read)."""
    _need_cuda(feat_a, map_a, feat_b, map_b)
    fa, fb = feat_a.contiguous().float(), feat_b.contiguous().float()
    assert fa.shape[1] == fb.shape[1] and map_a.dtype == map_b.dtype == torch.int32
    assert map_a.shape[0] == fa.shape[0] and map_b.shape[0] == fb.shape[0]
    of = torch.empty((int(n_out), fa.shape[1]), dtype=torch.float32, device=fa.device)
    check(lib.msmd_sparse_add_rows(_p(fa), _p(map_a.contiguous()), fa.shape[0], _p(fb),
                                   _p(map_b.contiguous()), fb.shape[0], fa.shape[1], int(n_out),
                                   _p(of), _stream()), "msmd_sparse_add_rows")
    return of


def rows_inverse(row_map, n_out):
    """inv[j] = the last row i with row_map[i] == j, -1 where none (int32 [n_out])."""
    _need_cuda(row_map)
    m = row_map if (row_map.dtype == torch.int32 and row_map.is_contiguous()) \
        else row_map.contiguous().int()
    inv = torch.empty((int(n_out),), dtype=torch.int32, device=m.device)
    check(lib.msmd_rows_inverse(_p(m), m.shape[0], int(n_out), _p(inv), _stream()),
          "msmd_rows_inverse")
    return inv


def sparse_add_rows_gather(feat_a, map_a, inv_a, feat_b, map_b, inv_b, n_out):
    """sparse_add_rows as a gather through the inverse maps (rows_inverse of map_a / map_b):
    every output row written once, no zero fill, no float atomics unless a tensor repeats a
    coordinate."""
    _need_cuda(feat_a, feat_b, inv_a, inv_b)
    fa, fb = feat_a.contiguous().float(), feat_b.contiguous().float()
    assert fa.shape[1] == fb.shape[1] and fa.shape[1] % 4 == 0
    assert map_a.shape[0] == fa.shape[0] and map_b.shape[0] == fb.shape[0]
    assert inv_a.shape[0] == inv_b.shape[0] == int(n_out)
    of = torch.empty((int(n_out), fa.shape[1]), dtype=torch.float32, device=fa.device)
    check(lib.msmd_sparse_add_rows_gather(_p(fa), _p(map_a), _p(inv_a), fa.shape[0], _p(fb),
                                          _p(map_b), _p(inv_b), fb.shape[0], fa.shape[1],
                                          int(n_out), _p(of), _stream()),
          "msmd_sparse_add_rows_gather")
    return of


class _GmaAssemble(torch.autograd.Function):
    """Feature assembly of a GMA-Conv stage, one launch each way (csrc/gma.hip)."""

    @staticmethod
    def forward(ctx, conv3, cross_gate, gate, feat3, feat2, nn3, rows_o2, rows_m3, rows_m2,
                n_o2_pad, n_mix_pad, order, starts):
        n_o3, c3 = conv3.shape
        n3, c2 = cross_gate.shape[0] - 1, cross_gate.shape[1]
        n_o2, n_mix = rows_o2.shape[0], rows_m3.shape[0]
        rows = n_o3 + n_o2 + n_o2_pad + n_mix + n_mix_pad
        out = torch.empty((rows, c3 + c2), dtype=torch.float32, device=conv3.device)
        check(lib.msmd_gma_assemble_fwd_f32(
            _p(conv3), n_o3, c3, _p(cross_gate), n3, c2, _p(nn3), _p(feat2), _p(rows_o2), n_o2,
            int(n_o2_pad), _p(feat3), _p(rows_m3), _p(gate), _p(rows_m2), n_mix, int(n_mix_pad),
            _p(out), _stream()), "msmd_gma_assemble_fwd_f32")
        ctx.save_for_backward(feat2, nn3, rows_o2, rows_m2)
        ctx.csr = (order, starts)
        ctx.dims = (n_o3, c3, n3, c2, n_o2, int(n_o2_pad), n_mix, int(n_mix_pad))
        return out

    @staticmethod
    def backward(ctx, d_out):
        feat2, nn3, rows_o2, rows_m2 = ctx.saved_tensors
        n_o3, c3, n3, c2, n_o2, n_o2_pad, n_mix, n_mix_pad = ctx.dims
        d = d_out.contiguous().float()
        need = ctx.needs_input_grad
        d_conv3 = torch.empty((n_o3, c3), dtype=torch.float32, device=d.device)
        d_cross = torch.empty((n3 + 1, c2), dtype=torch.float32, device=d.device) if need[1] else None
        d_gate = torch.empty((n_mix, c2), dtype=torch.float32, device=d.device) if need[2] else None
        ws = None
        if ctx.csr[0] is not None and d_cross is not None:
            ws = _ws(4 * lib.msmd_gma_assemble_bwd_workspace_floats(c2), d.device)
        check(lib.msmd_gma_assemble_bwd_f32(
            _p(d), n_o3, c3, n3, c2, _p(nn3), _p(feat2), _p(rows_o2), n_o2, n_o2_pad,
            _p(rows_m2), n_mix, n_mix_pad, _p(d_conv3), _p(d_cross), _p(d_gate),
            _p(ctx.csr[0]), _p(ctx.csr[1]), _p(ws), _stream()), "msmd_gma_assemble_bwd_f32")
        return (d_conv3 if need[0] else None, d_cross, d_gate) + (None,) * 10


def gma_nn_segments(nn3, n3):
    """(order, starts) for gma_assemble's backward: the only-2D rows sorted by their nearest
    3D voxel (-1 -> n3, stable) and, per target t in 0..n3, its slice starts[t]:starts[t+1] of
    `order`.  Index-only (no host read): the index pass builds it ahead of the feature pass."""
    key = torch.where(nn3 >= 0, nn3, torch.full_like(nn3, n3))
    skey, order = torch.sort(key, stable=True)
    starts = torch.searchsorted(skey, torch.arange(n3 + 2, device=nn3.device, dtype=skey.dtype))
    return order.contiguous(), starts.contiguous()


def gma_assemble(conv3, cross_gate, gate, feat3, feat2, nn3, rows_o2, rows_m3, rows_m2,
                 n_o2_pad=0, n_mix_pad=0, segments=None):
    """Unified features of a GMA-Conv stage (mmdet3d/models/middle_encoders/
    sparse_encoder_multimodal_encoderpaint_double_aware.py:349-421): rows
    [conv3 | 0], [0 | cross_gate[nn3] * feat2[rows_o2]], zero pad rows,
    [feat3[rows_m3] | gate * feat2[rows_m2]], zero pad rows.  Gradients flow to conv3,
    cross_gate and gate; feat3 / feat2 must not require one (the caller falls back to the
    unfused ops otherwise).  segments = gma_nn_segments(nn3, n3): d cross_gate is then summed
    in a fixed order (deterministic); without it by float atomics."""
    _need_cuda(conv3, cross_gate, gate, feat3, feat2, nn3, rows_o2, rows_m3, rows_m2)
    assert not feat3.requires_grad and not feat2.requires_grad
    assert nn3.dtype == rows_o2.dtype == rows_m3.dtype == rows_m2.dtype == torch.int64
    assert nn3.shape[0] == rows_o2.shape[0] and rows_m3.shape[0] == rows_m2.shape[0] == gate.shape[0]
    assert conv3.shape[1] == feat3.shape[1] and cross_gate.shape[1] == gate.shape[1] == feat2.shape[1]
    f = lambda t: t.contiguous().float()
    order, starts = segments if segments is not None else (None, None)
    if order is not None:
        assert order.dtype == starts.dtype == torch.int64 and order.shape[0] == nn3.shape[0]
        assert starts.shape[0] == cross_gate.shape[0] + 1
    return _GmaAssemble.apply(f(conv3), f(cross_gate), f(gate), f(feat3), f(feat2),
                              nn3.contiguous(), rows_o2.contiguous(), rows_m3.contiguous(),
                              rows_m2.contiguous(), int(n_o2_pad), int(n_mix_pad), order, starts)


def gma_stage_supported(c3, c2):
    return bool(lib.msmd_gma_stage_supported(int(c3), int(c2)))


class _GmaStage(torch.autograd.Function):
    """Both gate linears inside the stage assembly (csrc/gma.hip): one launch forward, a
    partial and a reduce launch backward; no gate table is built."""

    @staticmethod
    def forward(ctx, conv3, w_c, b_c, w_g, b_g, feat3, dummy, feat2, nn3, rows_o2, rows_m3,
                rows_m2, n_o2_pad, n_mix_pad, order, starts):
        n_o3, c3 = conv3.shape
        n3, c2 = feat3.shape[0], feat2.shape[1]
        n_o2, n_mix = rows_o2.shape[0], rows_m3.shape[0]
        rows = n_o3 + n_o2 + n_o2_pad + n_mix + n_mix_pad
        out = torch.empty((rows, c3 + c2), dtype=torch.float32, device=conv3.device)
        check(lib.msmd_gma_stage_fwd_f32(
            _p(conv3), n_o3, c3, _p(feat3), n3, c2, _p(dummy), _p(w_c), _p(b_c), _p(w_g), _p(b_g),
            _p(nn3), _p(feat2), _p(rows_o2), n_o2, n_o2_pad, _p(rows_m3), _p(rows_m2), n_mix,
            n_mix_pad, _p(out), _stream()), "msmd_gma_stage_fwd_f32")
        ctx.save_for_backward(w_c, b_c, w_g, b_g, feat3, dummy, feat2, rows_o2, rows_m3, rows_m2,
                              order, starts)
        ctx.dims = (n_o3, c3, n3, c2, n_o2, n_o2_pad, n_mix, n_mix_pad)
        return out

    @staticmethod
    def backward(ctx, d_out):
        w_c, b_c, w_g, b_g, feat3, dummy, feat2, rows_o2, rows_m3, rows_m2, order, starts = \
            ctx.saved_tensors
        n_o3, c3, n3, c2, n_o2, n_o2_pad, n_mix, n_mix_pad = ctx.dims
        d = d_out.contiguous().float()
        dev = d.device
        d_conv3 = torch.empty((n_o3, c3), dtype=torch.float32, device=dev)
        dw_c, dw_g = torch.empty_like(w_c), torch.empty_like(w_g)
        db_c = None if b_c is None else torch.empty_like(b_c)
        db_g = None if b_g is None else torch.empty_like(b_g)
        nbytes = lib.msmd_gma_stage_bwd_workspace_bytes(n3, n_mix, c3, c2)
        ws = _ws(nbytes, dev)
        check(lib.msmd_gma_stage_bwd_f32(
            _p(d), n_o3, c3, _p(feat3), n3, c2, _p(dummy), _p(w_c), _p(b_c), _p(w_g), _p(b_g),
            _p(feat2), _p(rows_o2), n_o2, n_o2_pad, _p(rows_m3), _p(rows_m2), n_mix, n_mix_pad,
            _p(order), _p(starts), _p(d_conv3), _p(dw_c), _p(db_c), _p(dw_g), _p(db_g), _p(ws),
            nbytes, _stream()), "msmd_gma_stage_bwd_f32")
        return (d_conv3, dw_c, db_c, dw_g, db_g) + (None,) * 11


def gma_stage(conv3, w_cross, b_cross, w_gate, b_gate, feat3, dummy, feat2, nn3, rows_o2, rows_m3,
              rows_m2, n_o2_pad, n_mix_pad, segments):
    """gma_assemble with both gates computed inside it: cross_gate = relu(Linear(w_cross,
    b_cross)) of feat3's rows and the `dummy` row [1, c3] behind them, gate = relu(Linear(
    w_gate, b_gate)) of feat3[rows_m3] -- evaluated per output row, so only the table rows the
    assembly reads cost anything, forward and backward.  Gradients: conv3 and the four
    parameters; feat3 / feat2 / dummy get none.  segments = gma_nn_segments(nn3, n3).  The
    values are those of rows_linear -> gma_assemble to the bit."""
    _need_cuda(conv3, w_cross, w_gate, feat3, dummy, feat2, nn3, rows_o2, rows_m3, rows_m2)
    assert not (feat3.requires_grad or feat2.requires_grad or dummy.requires_grad)
    assert nn3.dtype == rows_o2.dtype == rows_m3.dtype == rows_m2.dtype == torch.int64
    assert nn3.shape[0] == rows_o2.shape[0] and rows_m3.shape[0] == rows_m2.shape[0]
    c3, c2 = feat3.shape[1], feat2.shape[1]
    if not gma_stage_supported(c3, c2):
        raise ValueError(f"gma_stage: unsupported channels c3 = {c3}, c2 = {c2}")
    assert conv3.shape[1] == c3 and dummy.numel() == c3
    assert tuple(w_cross.shape) == tuple(w_gate.shape) == (c2, c3)
    order, starts = segments
    assert order.dtype == starts.dtype == torch.int64 and order.shape[0] == nn3.shape[0]
    assert starts.shape[0] == feat3.shape[0] + 2
    f = lambda t: None if t is None else t.contiguous().float()
    return _GmaStage.apply(f(conv3), f(w_cross), f(b_cross), f(w_gate), f(b_gate), f(feat3),
                           f(dummy), f(feat2), nn3.contiguous(), rows_o2.contiguous(),
                           rows_m3.contiguous(), rows_m2.contiguous(), int(n_o2_pad),
                           int(n_mix_pad), order.contiguous(), starts.contiguous())


def _modality_split_launch(idx_3d, idx_2d, batch_size, spatial_shape, float_keys,
                           reference_offsets, want_stats):
    """Enqueue one split -> (mix3d, mix2d, pair_3d, pair_2d, out) with out = int32
    [count | 4 * batch stats] on the device (capacity-sized pair lists: the caller trims)."""
    _need_bzyx(idx_3d, idx_2d)
    _need_cuda(idx_3d, idx_2d)
    a, b = idx_3d.contiguous().int(), idx_2d.contiguous().int()
    n3, n2 = a.shape[0], b.shape[0]
    dev = a.device
    B = int(batch_size)
    cap = max(min(n3, n2), 1)
    mix3 = torch.empty((n3,), dtype=torch.int32, device=dev)
    mix2 = torch.empty((n2,), dtype=torch.int32, device=dev)
    p3 = torch.empty((cap,), dtype=torch.int32, device=dev)
    p2 = torch.empty((cap,), dtype=torch.int32, device=dev)
    out = torch.empty((1 + 4 * B,), dtype=torch.int32, device=dev)   # count | stats
    stats_p = C.c_void_p(out.data_ptr() + 4) if want_stats else None
    if float_keys:
        nbytes = lib.msmd_modality_split_float_keys_workspace_bytes(n3, n2, B)
        ws = _ws(nbytes, dev)
        check(lib.msmd_modality_split_float_keys(_p(a), n3, _p(b), n2, B, int3(spatial_shape),
                                                 _p(mix3), _p(mix2), _p(p3), _p(p2), _p(out),
                                                 stats_p, int(bool(reference_offsets)), _p(ws),
                                                 nbytes, _stream()),
              "msmd_modality_split_float_keys")
    else:
        nbytes = lib.msmd_modality_split_workspace_bytes(B, int3(spatial_shape))
        ws = _ws(nbytes, dev)
        if want_stats:
            check(lib.msmd_modality_split_stats(_p(a), n3, _p(b), n2, B, int3(spatial_shape),
                                                _p(mix3), _p(mix2), _p(p3), _p(p2), _p(out),
                                                stats_p, _p(ws), nbytes, _stream()),
                  "msmd_modality_split_stats")
        else:
            check(lib.msmd_modality_split(_p(a), n3, _p(b), n2, B, int3(spatial_shape), _p(mix3),
                                          _p(mix2), _p(p3), _p(p2), _p(out), _p(ws), nbytes,
                                          _stream()), "msmd_modality_split")
    return mix3, mix2, p3, p2, out, (a, b, ws)


def _check_split_count(m):
    """msmd_modality_split_float_keys reports bad input through a count of -1."""
    if m < 0:
        raise ValueError("modality_split(float_keys=True): a voxel row lies outside the grid / "
                         "the batch, or (reference_offsets) the rows are not grouped by sample "
                         "in ascending order (include/msmd_hip.h)")


def modality_split(idx_3d, idx_2d, batch_size, spatial_shape, float_keys=False,
                   reference_offsets=False):
    """-> (mix3d[n3], mix2d[n2], pair_3d[m], pair_2d[m]).
    float_keys: the reference's float32 keys and two-pointer merge (csrc/modality_float.hip;
    MSMDFusion.py:271-272, 27-45) instead of exact integer keys; reference_offsets: pair rows
    numbered with the reference's non-cumulative batch offsets (:288-289,313-314) -- this
    needs each set's rows grouped by sample in ascending order (what voxelize() returns; the
    reference selects by mask and has no such requirement, nor has the exact-key path).
    Rows outside the grid and ungrouped rows raise ValueError (checked on the device)."""
    mix3, mix2, p3, p2, out, _keep = _modality_split_launch(
        idx_3d, idx_2d, batch_size, spatial_shape, float_keys, reference_offsets, False)
    m = int(out[0].item())
    _check_split_count(m)
    return mix3, mix2, p3[:m], p2[:m]


def modality_split_many(jobs, batch_size, float_keys=False, reference_offsets=False):
    """Several independent modality splits (the four image scales of a step) with ONE
    host read.  jobs: [(idx_3d, idx_2d, spatial_shape), ...] -> per job
    (mix3d, mix2d, pair_3d, pair_2d, stats) with stats = dict of per-sample row
    counts as python lists: c3_plain, c3_mixed, c2_plain, c2_mixed."""
    B = int(batch_size)
    pending = [_modality_split_launch(i3, i2, B, shape, float_keys, reference_offsets, True)
               for i3, i2, shape in jobs]
    if not pending:
        return []
    host = torch.stack([p[4] for p in pending]).tolist()
    res = []
    for (mix3, mix2, p3, p2, _, _), h in zip(pending, host):
        m = h[0]
        _check_split_count(m)
        stats = dict(c3_plain=h[1:1 + B], c3_mixed=h[1 + B:1 + 2 * B],
                     c2_plain=h[1 + 2 * B:1 + 3 * B], c2_mixed=h[1 + 3 * B:1 + 4 * B])
        res.append((mix3, mix2, p3[:m], p2[:m], stats))
    return res


CHECK_COUNTS = os.environ.get("MSMD_CHECK_COUNTS", "0") == "1"


def rows_where_eq(flags, value, count):
    """Row numbers i (int64, ascending) with flags[i] == value for a 1-D int32 tensor (any
    stride: a column of an index tensor) whose number of such rows the host already knows:
    one scan (two launches, csrc/dense.hip) instead of a compare + nonzero_static."""
    count = int(count)
    if count == 0 or flags.shape[0] == 0:
        return torch.empty((0,), dtype=torch.long, device=flags.device)
    if not flags.is_cuda or flags.dtype != torch.int32 or flags.dim() != 1:
        return rows_where(flags == value, count)
    n = flags.shape[0]
    # `count` is the host's number (msmd_modality_split_stats).  The kernel never leaves a
    # row of the output unwritten: rows past the device's own total are set to -1
    # (rows_tail_fill, csrc/dense.hip), so a stale host count cannot hand uninitialised row
    # ids to index_select -- it hands it -1, which torch's bounds check rejects.
    # MSMD_CHECK_COUNTS=1 (tests, debugging) reads the device total back and compares.
    rows = torch.empty((count,), dtype=torch.long, device=flags.device)
    nbytes = lib.msmd_rows_where_workspace_bytes(n)
    ws = _ws(nbytes, flags.device)
    total = torch.empty((1,), dtype=torch.int32, device=flags.device) if CHECK_COUNTS else None
    check(lib.msmd_rows_where_eq(_p(flags), int(flags.stride(0)), n, int(value), _p(rows), count,
                                 _p(total), _p(ws), nbytes, _stream()), "msmd_rows_where_eq")
    if total is not None and int(total.item()) != count:
        raise RuntimeError("rows_where_eq: the host expects %d rows with flag %d, the device "
                           "found %d (stale per-sample statistics?)"
                           % (count, int(value), int(total.item())))
    return rows


def rows_where_eq_many(jobs):
    """rows_where_eq for several (flags, value, count) triples in ONE scan (two launches):
    -> list of int64 row tensors.  flags: 1-D int32 CUDA tensors (any stride)."""
    if not jobs:
        return []
    dev = jobs[0][0].device
    n = len(jobs)
    outs, ptr_f, ptr_r = [], (C.c_void_p * n)(), (C.c_void_p * n)()
    strides, lens, values, caps = ((C.c_int * n)() for _ in range(4))
    for i, (flags, value, count) in enumerate(jobs):
        _need_cuda(flags)
        if flags.dtype != torch.int32 or flags.dim() != 1:
            raise ValueError("rows_where_eq_many: 1-D int32 flag vectors")
        count = int(count)
        out = torch.empty((count,), dtype=torch.long, device=dev)
        outs.append(out)
        ptr_f[i], ptr_r[i] = _p(flags), (_p(out) if count else None)
        strides[i] = int(flags.stride(0)) if flags.shape[0] else 1
        lens[i], values[i], caps[i] = flags.shape[0], int(value), count
    nbytes = lib.msmd_rows_where_eq_many_workspace_bytes(lens, n)
    ws = _ws(nbytes, dev)
    check(lib.msmd_rows_where_eq_many(ptr_f, strides, lens, values, ptr_r, caps, n, _p(ws), nbytes,
                                      _stream()), "msmd_rows_where_eq_many")
    return outs


def rows_where(mask, count):
    """Row numbers where a 1-D bool tensor is set, ascending, when their number is
    already known on the host: mask.nonzero() would wait for the device to size its
    output."""
    count = int(count)
    if count == 0:
        return torch.empty((0,), dtype=torch.long, device=mask.device)
    if _nonzero_static_ok(mask.device):
        return torch.nonzero_static(mask, size=count).flatten()
    # stable sort of the inverted mask: the selected rows come first, in order
    return torch.sort((~mask).to(torch.uint8), stable=True)[1][:count]


_NONZERO_STATIC = {}      # device type -> whether torch.nonzero_static works there


def _nonzero_static_ok(device):
    """Probed ONCE per device type on a tiny tensor: the hot path never swallows a
    RuntimeError (an asynchronous HIP error surfacing at that call would be hidden and the
    slow fallback taken for the rest of the process)."""
    ok = _NONZERO_STATIC.get(device.type)
    if ok is None:
        ok = False
        if hasattr(torch, "nonzero_static"):
            try:
                probe = torch.tensor([True, False, True], device=device)
                ok = torch.nonzero_static(probe, size=2).flatten().tolist() == [0, 2]
            except (NotImplementedError, RuntimeError):
                ok = False
        _NONZERO_STATIC[device.type] = ok
    return ok


# ------------------------------------------------------------------ GMA-Conv helpers
def furthest_point_sample(points_xyz, num_points):
    """mmdet3d/ops/furthest_point_sample/furthest_point_sample.py:14-35."""
    _need_cuda(points_xyz)
    x = points_xyz.contiguous().float()
    b, n, _ = x.shape
    out = torch.empty((b, num_points), dtype=torch.int32, device=x.device)
    tmp = torch.empty((b, n), dtype=torch.float32, device=x.device)
    check(lib.msmd_furthest_point_sample(_p(x), b, n, int(num_points), _p(tmp), _p(out),
                                         _stream()), "msmd_furthest_point_sample")
    return out


def furthest_point_sample_ragged(xyz, offsets, n_max, num_points):
    """FPS over a ragged batch: xyz [total,3], offsets int32 [b+1] (device),
    n_max = largest element (host int).  -> int32 [b, num_points], indices local
    to each element.  All elements run concurrently, one workgroup each."""
    _need_cuda(xyz, offsets)
    x = xyz.contiguous().float()
    b = offsets.shape[0] - 1
    out = torch.empty((b, num_points), dtype=torch.int32, device=x.device)
    tmp = torch.empty((max(x.shape[0], 1),), dtype=torch.float32, device=x.device)
    check(lib.msmd_furthest_point_sample_ragged(_p(x), _p(offsets.contiguous().int()), b,
                                                int(n_max), int(num_points), _p(tmp), _p(out),
                                                _stream()), "msmd_furthest_point_sample_ragged")
    return out


def ball_query(min_radius, max_radius, sample_num, xyz, center_xyz):
    """mmdet3d/ops/ball_query/ball_query.py:14-40 (same argument order)."""
    _need_cuda(xyz, center_xyz)
    assert min_radius < max_radius
    x, cx = xyz.contiguous().float(), center_xyz.contiguous().float()
    b, n, _ = x.shape
    m = cx.shape[1]
    idx = torch.empty((b, m, int(sample_num)), dtype=torch.int32, device=x.device)
    check(lib.msmd_ball_query(_p(cx), _p(x), b, n, m, float(min_radius), float(max_radius),
                              int(sample_num), _p(idx), _stream()), "msmd_ball_query")
    return idx


def nn_search(query_zyx, key_zyx, dist_thresh):
    _need_cuda(query_zyx, key_zyx)
    q, k = query_zyx.contiguous().int(), key_zyx.contiguous().int()
    nq, nk = q.shape[0], k.shape[0]
    out = torch.empty((nq,), dtype=torch.int32, device=q.device)
    scratch = torch.empty((max(nq, 1),), dtype=torch.int64, device=q.device)
    check(lib.msmd_nn_search(_p(q), nq, _p(k), nk, float(dist_thresh), _p(out), _p(scratch),
                             _stream()), "msmd_nn_search")
    return out


def nn_assign(group_idx, rep_nn, nq):
    _need_cuda(group_idx, rep_nn)
    g, r = group_idx.contiguous().int(), rep_nn.contiguous().int()
    m, ns = g.shape
    out = torch.empty((nq,), dtype=torch.int32, device=g.device)
    scratch = torch.empty((max(nq, 1),), dtype=torch.int32, device=g.device)
    check(lib.msmd_nn_assign(_p(g), _p(r), m, ns, int(nq), _p(out), _p(scratch), _stream()),
          "msmd_nn_assign")
    return out


NN_CHAIN_SKIP, NN_CHAIN_DIRECT, NN_CHAIN_CLUSTERED = 0, 1, 2      # msmd_hip.h: MSMD_NN_CHAIN_*
NN_CHAIN_KEYS = 256      # csrc/gma_nn.hip: kChainKeys, the keys one workgroup visits


def gma_nn_chain_supported(coord_bound, dist_thresh, radius):
    """Whether gma_nn_chain's integer distance order is exact (csrc/gma_nn.hip): every
    coordinate below `coord_bound` <= 32768, dist_thresh and radius at most 2048 (radius > 0)."""
    return (coord_bound is not None and int(coord_bound) <= 32768
            and float(dist_thresh) <= 2048.0 and 0.0 < float(radius) <= 2048.0)


def gma_nn_chain_desc(q_offsets, k_offsets, modes, bases, device):
    """The per-sample descriptors of gma_nn_chain as one int32 device vector (one pinned,
    non-blocking copy): query offsets [B+1] | key offsets [B+1] | mode [B] | base [B].
    Its first B+1 entries are what furthest_point_sample_ragged takes as offsets."""
    desc = torch.tensor(list(q_offsets) + list(k_offsets) + list(modes) + list(bases),
                        dtype=torch.int32)
    return desc.pin_memory().to(device, non_blocking=True)


def _rows16(t):
    """(b,z,y,x) rows as contiguous int32 whose first row is 16-byte aligned."""
    t = t.contiguous().int()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def gma_nn_chain(query_bzyx, key_bzyx, desc, batch_size, fps_idx, fps_num, nq_max, nk_max,
                 dist_thresh, radius, max_cluster_samples, n_pad=0):
    """The neighbour search behind FPS for all samples of a stage (msmd_gma_nn_chain):
    -> int64 [n_query + n_pad] rows of key_bzyx (base + sample-local nearest key), -1 = none.
    desc: gma_nn_chain_desc(); fps_idx: int32 [B, fps_num] sample-local representatives
    (None when no sample is CLUSTERED); nq_max / nk_max: host ints, the largest searching
    set (fps_num for a CLUSTERED sample, its query count for a DIRECT one) and key set."""
    _need_cuda(query_bzyx, key_bzyx, desc, fps_idx)
    if not gma_nn_chain_supported(0, dist_thresh, radius):
        raise ValueError("gma_nn_chain needs dist_thresh <= 2048 and radius <= 2048")
    q, k = _rows16(query_bzyx), _rows16(key_bzyx)
    nq, nk, b = q.shape[0], k.shape[0], int(batch_size)
    assert q.shape[1:] == (4,) and k.shape[1:] == (4,) and desc.numel() == 4 * b + 2
    assert desc.dtype == torch.int32 and desc.is_contiguous()
    if fps_idx is not None:
        assert fps_idx.dtype == torch.int32 and tuple(fps_idx.shape) == (b, int(fps_num))
        fps_idx = fps_idx.contiguous()
    out = torch.empty((nq + int(n_pad),), dtype=torch.long, device=q.device)
    nbytes = lib.msmd_gma_nn_chain_scratch_bytes(b, int(nq_max), nq)
    scratch = torch.empty((max(nbytes // 8 + 1, 1),), dtype=torch.int64, device=q.device)
    check(lib.msmd_gma_nn_chain(_p(q), nq, _p(k), nk, _p(desc), b, _p(fps_idx), int(fps_num),
                                int(nq_max), int(nk_max), float(dist_thresh), float(radius),
                                int(max_cluster_samples), int(n_pad), _p(out), _p(scratch),
                                scratch.numel() * 8, _stream()), "msmd_gma_nn_chain")
    return out


# ------------------------------------------------------------------ PointNet++ op family (n1)
KNN_MAX_K = 128      # csrc/pointnet.hip: kKnnMaxK


def _need_f32(t, shape, what):
    """A contiguous float32 tensor of the given shape (None = any size on that axis)."""
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (what, t.dtype))
    if t.dim() != len(shape) or any(w is not None and int(v) != int(w)
                                    for v, w in zip(t.shape, shape)):
        raise ValueError("%s must be %s, got %s" % (what, list(shape), tuple(t.shape)))
    return t.contiguous()


def _need_i32(t, shape, what):
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError("%s must be an integer tensor, got %s" % (what, t.dtype))
    if t.dim() != len(shape) or any(w is not None and int(v) != int(w)
                                    for v, w in zip(t.shape, shape)):
        raise ValueError("%s must be %s, got %s" % (what, list(shape), tuple(t.shape)))
    return t.contiguous().int()


def gather_points(features, indices, out=None):
    """gather_points_ext.gather_points_wrapper: features (B, C, N), indices (B, M) ->
    (B, C, M)."""
    _need_cuda(features, indices, out)
    f = _need_f32(features, (None, None, None), "features")
    b, c, n = f.shape
    idx = _need_i32(indices, (b, None), "indices")
    m = idx.shape[1]
    if out is None:
        out = torch.empty((b, c, m), dtype=torch.float32, device=f.device)
    check(lib.msmd_gather_points_f32(_p(f), _p(idx), b, c, n, m, _p(out), _stream()),
          "msmd_gather_points_f32")
    return out


def group_points(features, indices, out=None):
    """group_points_ext.forward: features (B, C, N), indices (B, npoint, nsample) ->
    (B, C, npoint, nsample)."""
    _need_cuda(features, indices, out)
    f = _need_f32(features, (None, None, None), "features")
    b, c, n = f.shape
    idx = _need_i32(indices, (b, None, None), "indices")
    npoint, nsample = idx.shape[1:]
    if out is None:
        out = torch.empty((b, c, npoint, nsample), dtype=torch.float32, device=f.device)
    check(lib.msmd_group_points_f32(_p(f), _p(idx), b, c, n, npoint, nsample, _p(out),
                                    _stream()), "msmd_group_points_f32")
    return out


def three_nn(unknown, known, dist2=None, idx=None):
    """interpolate_ext.three_nn_wrapper: unknown (B, N, 3), known (B, M, 3) -> SQUARED
    distances (B, N, 3) float32 and indices (B, N, 3) int32."""
    _need_cuda(unknown, known, dist2, idx)
    u = _need_f32(unknown, (None, None, 3), "unknown")
    b, n, _ = u.shape
    k = _need_f32(known, (b, None, 3), "known")
    if dist2 is None:
        dist2 = torch.empty((b, n, 3), dtype=torch.float32, device=u.device)
    if idx is None:
        idx = torch.empty((b, n, 3), dtype=torch.int32, device=u.device)
    check(lib.msmd_three_nn_f32(_p(u), _p(k), b, n, k.shape[1], _p(dist2), _p(idx), _stream()),
          "msmd_three_nn_f32")
    return dist2, idx


def three_interpolate(features, indices, weight, out=None):
    """interpolate_ext.three_interpolate_wrapper: features (B, C, M), indices / weight
    (B, N, 3) -> (B, C, N)."""
    _need_cuda(features, indices, weight, out)
    f = _need_f32(features, (None, None, None), "features")
    b, c, m = f.shape
    idx = _need_i32(indices, (b, None, 3), "indices")
    n = idx.shape[1]
    w = _need_f32(weight, (b, n, 3), "weight")
    if out is None:
        out = torch.empty((b, c, n), dtype=torch.float32, device=f.device)
    check(lib.msmd_three_interpolate_f32(_p(f), _p(idx), _p(w), b, c, m, n, _p(out), _stream()),
          "msmd_three_interpolate_f32")
    return out


def knn(k, xyz, center_xyz):
    """The k nearest of xyz (B, N, 3) to every centre (B, npoint, 3): int64 (B, k, npoint),
    0-based, ordered by (squared distance, index)."""
    _need_cuda(xyz, center_xyz)
    x = _need_f32(xyz, (None, None, 3), "xyz")
    b, n, _ = x.shape
    cx = _need_f32(center_xyz, (b, None, 3), "center_xyz")
    k = int(k)
    if k < 1:
        raise ValueError("knn: k must be positive, got %d" % k)
    if k > KNN_MAX_K:
        raise ValueError("knn: k = %d, but the kernel is built for k <= %d" % (k, KNN_MAX_K))
    if k > n:
        raise ValueError("knn: k = %d neighbours asked of %d points" % (k, n))
    npoint = cx.shape[1]
    idx = torch.empty((b, k, npoint), dtype=torch.int64, device=x.device)
    check(lib.msmd_knn_f32(_p(x), _p(cx), b, n, npoint, k, _p(idx), _stream()), "msmd_knn_f32")
    return idx


def furthest_point_sample_with_dist(points_dist, num_points, out=None):
    """furthest_point_sample.py:41-66: points_dist (B, N, N) -> int32 (B, num_points)."""
    _need_cuda(points_dist, out)
    d = _need_f32(points_dist, (None, None, None), "points_dist")
    b, n, n2 = d.shape
    if n != n2:
        raise ValueError("points_dist must be (B, N, N), got %s" % (tuple(d.shape),))
    if out is None:
        out = torch.empty((b, int(num_points)), dtype=torch.int32, device=d.device)
    tmp = torch.empty((b, n), dtype=torch.float32, device=d.device)
    check(lib.msmd_furthest_point_sample_with_dist(_p(d), b, n, int(num_points), _p(tmp), _p(out),
                                                   _stream()),
          "msmd_furthest_point_sample_with_dist")
    return out


class PointInverseIndex:
    """By-source inverse of an index tensor (B, M) over N source points: the destinations of
    source (b, s) are dest[src_start[b*N + s] : src_start[b*N + s + 1]], ascending."""
    __slots__ = ("src_start", "dest", "b", "n", "m")

    def __init__(self, src_start, dest, b, n, m):
        self.src_start, self.dest, self.b, self.n, self.m = src_start, dest, b, n, m


def point_inverse_index(indices, num_src):
    """indices: (B, ...) integer tensor, flattened per batch element to (B, M)."""
    _need_cuda(indices)
    b = indices.shape[0]
    m, n = (indices[0].numel() if b else 0), int(num_src)
    idx = indices.contiguous().int().view(b, m)
    nbytes = lib.msmd_point_inverse_index_workspace_bytes(b, m)
    if nbytes == 0:
        raise ValueError("point_inverse_index: %d x %d destinations do not fit 31 bits" % (b, m))
    ws = _ws(nbytes, idx.device)
    src_start = torch.empty((b * n + 1,), dtype=torch.int32, device=idx.device)
    dest = torch.empty((max(b * m, 1),), dtype=torch.int32, device=idx.device)
    check(lib.msmd_point_inverse_index(_p(idx), b, n, m, _p(src_start), _p(dest), _p(ws),
                                       ws.numel(), _stream()), "msmd_point_inverse_index")
    return PointInverseIndex(src_start, dest, b, n, m)


def point_scatter_backward(grad_out, inverse, weight=None, dest_per_out=1, grad_in=None):
    """grad_in[b, c, s] = sum over the source's destinations, in ascending position, of
    weight * grad_out (float32, no atomics).  grad_out: (B, C, ...) with
    M / dest_per_out positions per (b, c); grad_in given: added to (the shims' contract)."""
    _need_cuda(grad_out, weight, grad_in)
    if grad_out.dtype != torch.float32:
        raise TypeError("grad_out must be float32, got %s" % grad_out.dtype)
    b, n, m = inverse.b, inverse.n, inverse.m
    g = grad_out.contiguous()
    c = g.shape[1]
    if g.shape[0] != b or g.numel() != b * c * (m // dest_per_out):
        raise ValueError("grad_out %s does not match the index (B %d, %d destinations)"
                         % (tuple(g.shape), b, m))
    if weight is not None:
        weight = _need_f32(weight.view(b, -1) if weight.is_contiguous() else
                           weight.contiguous().view(b, -1), (b, m), "weight")
    accumulate = grad_in is not None
    if accumulate:
        if tuple(grad_in.shape) != (b, c, n) or grad_in.dtype != torch.float32 or \
                not grad_in.is_contiguous():
            raise ValueError("grad_in must be a contiguous float32 (%d, %d, %d)" % (b, c, n))
    else:
        grad_in = torch.empty((b, c, n), dtype=torch.float32, device=g.device)
    check(lib.msmd_point_scatter_bwd_f32(_p(g), _p(weight), _p(inverse.src_start),
                                         _p(inverse.dest), b, c, n, m, int(dest_per_out),
                                         int(accumulate), _p(grad_in), _stream()),
          "msmd_point_scatter_bwd_f32")
    return grad_in


# ------------------------------------------------------------------ gate tables (a16)
def rows_linear_supported(c_in, c_out):
    return bool(lib.msmd_rows_linear_supported(int(c_in), int(c_out)))


class _RowsLinear(torch.autograd.Function):
    """relu?(cat(x, x_tail) @ w^T + b) over feature rows (csrc/gma.hip); the weight and bias
    gradients come from per-block partial sums added in block order (deterministic); the
    input gradient, when something upstream wants it, is one matmul."""

    @staticmethod
    def forward(ctx, x, x_tail, w, b, relu):
        xx = x.contiguous().float()
        n, c_in = xx.shape
        tail = None if x_tail is None else x_tail.contiguous().float()
        n_tail = 0 if tail is None else tail.shape[0]
        ww = w.contiguous().float()
        bb = None if b is None else b.contiguous().float()
        c_out = ww.shape[0]
        y = torch.empty((n + n_tail, c_out), dtype=torch.float32, device=xx.device)
        check(lib.msmd_rows_linear_fwd_f32(_p(xx), n, _p(tail), n_tail, c_in, _p(ww), _p(bb), c_out,
                                           int(bool(relu)), _p(y), _stream()),
              "msmd_rows_linear_fwd_f32")
        ctx.save_for_backward(xx, tail, ww, y)
        ctx.relu, ctx.has_bias = bool(relu), b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        xx, tail, ww, y = ctx.saved_tensors
        g = dy.contiguous().float()
        n, c_in = xx.shape
        n_tail = 0 if tail is None else tail.shape[0]
        c_out = ww.shape[0]
        dx = dtail = dw = db = None
        if ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3]):
            dw = torch.empty_like(ww)
            db = torch.empty((c_out,), dtype=torch.float32, device=ww.device) if ctx.has_bias else None
            nbytes = lib.msmd_rows_linear_bwd_workspace_bytes(n + n_tail, c_in, c_out)
            ws = _ws(nbytes, ww.device)
            check(lib.msmd_rows_linear_bwd_f32(_p(xx), n, _p(tail), n_tail, c_in, _p(y), _p(g),
                                               c_out, int(ctx.relu), _p(dw), _p(db), _p(ws), nbytes,
                                               _stream()), "msmd_rows_linear_bwd_f32")
        if ctx.needs_input_grad[0] or (tail is not None and ctx.needs_input_grad[1]):
            gm = g * (y > 0) if ctx.relu else g
            if ctx.needs_input_grad[0]:
                dx = gm[:n] @ ww
            if tail is not None and ctx.needs_input_grad[1]:
                dtail = gm[n:] @ ww
        return dx, dtail, dw, db, None


def rows_linear(x, weight, bias=None, relu=False, x_tail=None):
    """nn.Linear (+ ReLU) over feature rows, optionally with extra rows appended (x_tail)
    without materialising the concatenation."""
    _need_cuda(x, weight)
    return _RowsLinear.apply(x, x_tail, weight, bias, relu)


# ------------------------------------------------------------------ pillar feature net
PILLAR_MAX_K, PILLAR_MAX_U, PILLAR_MAX_M = 16, 128, 64


class PillarGeometry:
    """The decoration a PillarFeatureNet applies (csrc/pillar.hip): flags, pillar size and the
    centre offsets, as the float32 values the reference's tensor arithmetic rounds them to."""

    def __init__(self, with_cluster_center, with_voxel_center, with_distance, legacy, vx, vy,
                 x_offset, y_offset):
        self.flags = (1 if with_cluster_center else 0) | (2 if with_voxel_center else 0) | \
            (4 if with_distance else 0) | (8 if legacy else 0)
        self.vx, self.vy = float(vx), float(vy)
        self.x_offset, self.y_offset = float(x_offset), float(y_offset)

    def decorated(self, c):
        return c + 3 * (self.flags & 1) + (self.flags & 2) + ((self.flags & 4) >> 2)

    def args(self):
        return self.flags, self.vx, self.vy, self.x_offset, self.y_offset


def pillar_supported(m, c, k, u):
    return 1 <= m <= PILLAR_MAX_M and c >= 3 and k <= PILLAR_MAX_K and 1 <= u <= PILLAR_MAX_U


def _pillar_inputs(voxels, num_points, coors):
    _need_cuda(voxels, num_points, coors)
    _need_dtype(voxels, torch.float32, "voxels")
    _need_dtype(num_points, torch.int32, "num_points")
    _need_dtype(coors, torch.int32, "coors")
    if voxels.dim() != 3 or not voxels.is_contiguous():
        raise ValueError("voxels must be a contiguous [N, M, C] table, got %s" % (tuple(voxels.shape),))
    n = voxels.shape[0]
    if tuple(num_points.shape) != (n,) or tuple(coors.shape) != (n, 4) or \
            not num_points.is_contiguous() or not coors.is_contiguous():
        raise ValueError("num_points must be [N] and coors [N, 4] (batch, z, y, x), contiguous")
    return n, int(voxels.shape[1]), int(voxels.shape[2])


def pillar_moments(voxels, num_points, coors, geom):
    """-> (s[K], G[K, K]) float64: column sums and Gram matrix of the decorated rows of all
    N * M slots."""
    n, m, c = _pillar_inputs(voxels, num_points, coors)
    k = geom.decorated(c)
    dev = voxels.device
    mom = torch.zeros(272, dtype=torch.float64, device=dev) if n == 0 else \
        torch.empty(272, dtype=torch.float64, device=dev)
    nbytes = lib.msmd_pillar_workspace_bytes(n, m, 1)
    ws = _ws(nbytes, dev)
    check(lib.msmd_pillar_moments_f32(_p(voxels), _p(num_points), _p(coors), n, m, c,
                                      *geom.args(), _p(mom), _p(ws), nbytes, _stream()),
          "msmd_pillar_moments_f32")
    return mom[:k], mom[16:].view(16, 16)[:k, :k]


def pillar_pfn_forward(voxels, num_points, coors, geom, weight, scale, shift, mode):
    """-> (out[N, U], argmax[N, U] uint8 | None)."""
    n, m, c = _pillar_inputs(voxels, num_points, coors)
    _need_cuda(weight, scale, shift)
    u = int(weight.shape[0])
    if tuple(weight.shape) != (u, geom.decorated(c)) or not weight.is_contiguous():
        raise ValueError("weight must be a contiguous [U, K=%d] matrix, got %s"
                         % (geom.decorated(c), tuple(weight.shape)))
    mode_max = {"max": 1, "avg": 0}[mode]
    out = torch.empty((n, u), dtype=torch.float32, device=voxels.device)
    arg = torch.empty((n, u), dtype=torch.uint8, device=voxels.device) if mode_max else None
    check(lib.msmd_pillar_pfn_fwd_f32(_p(voxels), _p(num_points), _p(coors), n, m, c,
                                      *geom.args(), _p(weight), _p(scale), _p(shift), u, mode_max,
                                      _p(out), _p(arg), _stream()), "msmd_pillar_pfn_fwd_f32")
    return out, arg


def pillar_pfn_backward(voxels, num_points, coors, geom, weight, scale, shift, mode, grad_out,
                        argmax):
    """-> (A[U, K], sg[U]) float64: sum g f and sum g over the slots the gradient reaches."""
    n, m, c = _pillar_inputs(voxels, num_points, coors)
    _need_cuda(weight, scale, shift, grad_out, argmax)
    u, k = int(weight.shape[0]), geom.decorated(c)
    _need_dtype(grad_out, torch.float32, "grad_out")
    if tuple(grad_out.shape) != (n, u) or not grad_out.is_contiguous():
        raise ValueError("grad_out must be a contiguous [N, U] tensor")
    dev = voxels.device
    sums = torch.zeros((u, 17), dtype=torch.float64, device=dev) if n == 0 else \
        torch.empty((u, 17), dtype=torch.float64, device=dev)
    nbytes = lib.msmd_pillar_workspace_bytes(n, m, u)
    ws = _ws(nbytes, dev)
    mode_max = {"max": 1, "avg": 0}[mode]
    check(lib.msmd_pillar_pfn_bwd_f32(_p(voxels), _p(num_points), _p(coors), n, m, c,
                                      *geom.args(), _p(weight), _p(scale), _p(shift), u, mode_max,
                                      _p(grad_out), _p(argmax), _p(sums), _p(ws), nbytes,
                                      _stream()), "msmd_pillar_pfn_bwd_f32")
    return sums[:, :k], sums[:, 16]


# ------------------------------------------------------------------ HardVFE (csrc/hard_vfe.hip)
HARD_VFE_MAX_K, HARD_VFE_MAX_U, HARD_VFE_MAX_M = 16, 64, 64
HARD_VFE_VOXELS_PER_STEP, HARD_VFE_BLOCKS = 4, 512     # kVox, kBlocks of the kernels


class HardVFEGeometry:
    """The decoration a HardVFE applies: flags (1 cluster centre, 2 the three-channel voxel
    centre), voxel size and centre offsets."""

    def __init__(self, with_cluster_center, with_voxel_center, vx, vy, vz, x_offset, y_offset,
                 z_offset):
        self.flags = (1 if with_cluster_center else 0) | (2 if with_voxel_center else 0)
        self.size = (float(vx), float(vy), float(vz))
        self.offset = (float(x_offset), float(y_offset), float(z_offset))

    def decorated(self, c):
        return c + 3 * (self.flags & 1) + 3 * ((self.flags & 2) >> 1)

    def args(self):
        return (self.flags, *self.size, *self.offset)


def hard_vfe_supported(m, c, k, widths):
    return 1 <= m <= HARD_VFE_MAX_M and c >= 3 and k <= HARD_VFE_MAX_K and \
        1 <= len(widths) <= 2 and all(1 <= u <= HARD_VFE_MAX_U for u in widths)


def _hard_vfe_layers(layers, k):
    """layers: [(weight, scale, shift)] of one or two layers (scale / shift may be None where
    the call does not read them) -> (w1, s1, t1, u1, w2, s2, t2, u2)."""
    if not 1 <= len(layers) <= 2:
        raise ValueError("the fused HardVFE runs one or two layers, got %d" % len(layers))
    w1, s1, t1 = layers[0]
    u1 = int(w1.shape[0])
    if tuple(w1.shape) != (u1, k) or not w1.is_contiguous():
        raise ValueError("layer 1 weight must be a contiguous [U1, K=%d] matrix, got %s"
                         % (k, tuple(w1.shape)))
    w2 = s2 = t2 = None
    u2 = 0
    if len(layers) == 2:
        w2, s2, t2 = layers[1]
        u2 = int(w2.shape[0])
        if tuple(w2.shape) != (u2, 2 * u1) or not w2.is_contiguous():
            raise ValueError("layer 2 weight must be a contiguous [U2, 2 * U1 = %d] matrix, got %s"
                             % (2 * u1, tuple(w2.shape)))
    for t, u, what in ((w1, u1, "weight"), (s1, u1, "scale1"), (t1, u1, "shift1"),
                       (w2, u2, "weight"), (s2, u2, "scale2"), (t2, u2, "shift2")):
        if t is None:
            continue
        _need_cuda(t)
        _need_dtype(t, torch.float32, what)
        if t.dim() == 1 and (t.shape[0] != u or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous [%d] vector" % (what, u))
    if u1 > HARD_VFE_MAX_U or u2 > HARD_VFE_MAX_U or k > HARD_VFE_MAX_K:
        raise ValueError("the fused HardVFE is built for K <= 16 and widths <= 64, got K=%d, "
                         "widths %s" % (k, (u1, u2)))
    return w1, s1, t1, u1, w2, s2, t2, u2


def _hard_vfe_inputs(voxels, num_points, coors, geom):
    n, m, c = _pillar_inputs(voxels, num_points, coors)
    if m > HARD_VFE_MAX_M or c < 3:
        raise ValueError("the fused HardVFE is built for M <= 64 slots and C >= 3, got M=%d C=%d"
                         % (m, c))
    return n, m, c, geom.decorated(c)


def hard_vfe_moments(voxels, num_points, coors, geom):
    """-> (s[K], G[K, K]) float64 of the decorated rows of all N * M slots (pillar_moments with
    the three-channel centre)."""
    n, m, c, k = _hard_vfe_inputs(voxels, num_points, coors, geom)
    dev = voxels.device
    mom = torch.zeros(272, dtype=torch.float64, device=dev) if n == 0 else \
        torch.empty(272, dtype=torch.float64, device=dev)
    nbytes = lib.msmd_hard_vfe_workspace_bytes(n, m)
    ws = _ws(nbytes, dev)
    check(lib.msmd_hard_vfe_moments_f32(_p(voxels), _p(num_points), _p(coors), n, m, c,
                                        *geom.args(), _p(mom), _p(ws), nbytes, _stream()),
          "msmd_hard_vfe_moments_f32")
    return mom[:k], mom[16:].view(16, 16)[:k, :k]


def hard_vfe_stats(voxels, num_points, coors, geom, w1, scale1, shift1, w2):
    """Layer 2's pre-BatchNorm sums -> (pivot[U2] float32, sum y2 [U2], sum (y2 - pivot)^2 [U2],
    float64) over all N * M rows."""
    n, m, c, k = _hard_vfe_inputs(voxels, num_points, coors, geom)
    w1, s1, t1, u1, w2, _, _, u2 = _hard_vfe_layers([(w1, scale1, shift1), (w2, None, None)], k)
    dev = voxels.device
    pivot = torch.zeros(64, dtype=torch.float32, device=dev)
    sums = torch.zeros(128, dtype=torch.float64, device=dev)
    nbytes = lib.msmd_hard_vfe_workspace_bytes(n, m)
    ws = _ws(nbytes, dev)
    check(lib.msmd_hard_vfe_stats_f32(_p(voxels), _p(num_points), _p(coors), n, m, c,
                                      *geom.args(), _p(w1), _p(s1), _p(t1), u1, _p(w2), u2,
                                      _p(pivot), _p(sums), _p(ws), nbytes, _stream()),
          "msmd_hard_vfe_stats_f32")
    sums = sums.view(64, 2)
    return pivot[:u2], sums[:u2, 0], sums[:u2, 1]


def hard_vfe_forward(voxels, num_points, coors, geom, layers):
    """layers: [(weight, scale, shift)] -> (out[N, U], argmax[N, U] uint8, ymax[N, U] | None):
    the last layer's maximum, the smallest slot attaining it and (two layers) the
    pre-BatchNorm y2 there."""
    n, m, c, k = _hard_vfe_inputs(voxels, num_points, coors, geom)
    w1, s1, t1, u1, w2, s2, t2, u2 = _hard_vfe_layers(layers, k)
    u, dev = (u2 or u1), voxels.device
    out = torch.empty((n, u), dtype=torch.float32, device=dev)
    arg = torch.empty((n, u), dtype=torch.uint8, device=dev)
    ymax = torch.empty((n, u), dtype=torch.float32, device=dev) if u2 else None
    check(lib.msmd_hard_vfe_fwd_f32(_p(voxels), _p(num_points), _p(coors), n, m, c, *geom.args(),
                                    _p(w1), _p(s1), _p(t1), u1, _p(w2), _p(s2), _p(t2), u2,
                                    _p(out), _p(arg), _p(ymax), _stream()),
          "msmd_hard_vfe_fwd_f32")
    return out, arg, ymax


def hard_vfe_backward(voxels, num_points, coors, geom, layers, g2, argmax, dp=None, dq=None):
    """g2[N, U]: the gradient at the last BatchNorm's output, placed at the argmax slots; dp,
    dq[U2]: the dense terms of a batch-statistics BatchNorm (dy2 = scale2 g2 - dp - dq y2).
    -> (dW2[U2, 2 U1] | None, A1[U1, K], sg1[U1]) float64."""
    n, m, c, k = _hard_vfe_inputs(voxels, num_points, coors, geom)
    w1, s1, t1, u1, w2, s2, _, u2 = _hard_vfe_layers(layers, k)
    u, dev = (u2 or u1), voxels.device
    _need_cuda(g2, argmax, dp, dq)
    _need_dtype(g2, torch.float32, "g2")
    _need_dtype(argmax, torch.uint8, "argmax")
    if tuple(g2.shape) != (n, u) or not g2.is_contiguous() or tuple(argmax.shape) != (n, u) or \
            not argmax.is_contiguous():
        raise ValueError("g2 and argmax must be contiguous [N, U] tensors")
    if u2:
        for t, what in ((dp, "dp"), (dq, "dq")):
            _need_dtype(t, torch.float32, what)
            if tuple(t.shape) != (u2,) or not t.is_contiguous():
                raise ValueError("%s must be a contiguous [U2] vector" % what)
    entries = 64 * 128 + 64 * 17 if u2 else 64 * 17
    sums = torch.zeros(entries, dtype=torch.float64, device=dev)
    nbytes = lib.msmd_hard_vfe_workspace_bytes(n, m)
    ws = _ws(nbytes, dev)
    check(lib.msmd_hard_vfe_bwd_f32(_p(voxels), _p(num_points), _p(coors), n, m, c, *geom.args(),
                                    _p(w1), _p(s1), _p(t1), u1, _p(w2), _p(s2), u2, _p(g2),
                                    _p(argmax), _p(dp), _p(dq), _p(sums), _p(ws), nbytes,
                                    _stream()), "msmd_hard_vfe_bwd_f32")
    dw2 = None
    if u2:
        dw = sums[:8192].view(64, 128)
        dw2 = torch.cat([dw[:u2, :u1], dw[:u2, 64:64 + u1]], dim=1)
        sums = sums[8192:]
    a1 = sums.view(64, 17)
    return dw2, a1[:u1, :k], a1[:u1, 16]


# ------------------------------------------------------------------ PointFusion's sampler (csrc/point_sample.hip)
POINT_SAMPLE_MAX_LEVELS = 8
POINT_SAMPLE_BWD_CHUNK = lib.msmd_point_sample_bwd_chunk()     # kChunk of the kernels


class _PointSampleLevel(C.Structure):      # include/msmd_hip.h: msmd_point_sample_level
    _fields_ = [("map", C.c_void_p), ("h", C.c_int32), ("w", C.c_int32), ("c", C.c_int32),
                ("offset", C.c_int32)]


class PointSampleBatch:
    """What one batch of clouds hands the sampler besides the points: sample_start (the host
    list and its device copy) and the per-sample parameter block [B, 20] float32 on the device
    (the layout of msmd_point_sample_params)."""
    __slots__ = ("starts", "sample_start", "params", "batch", "num_points")

    def __init__(self, starts, sample_start, params):
        self.starts = (C.c_int32 * len(starts))(*starts)
        self.sample_start, self.params = sample_start, params
        self.batch, self.num_points = len(starts) - 1, int(starts[-1])


def _point_sample_levels(maps):
    """maps: channels-last contiguous [B, H, W, C] float32 tensors -> (the level array, sum C)."""
    if not 1 <= len(maps) <= POINT_SAMPLE_MAX_LEVELS:
        raise ValueError("point_sample: 1..%d levels, got %d" % (POINT_SAMPLE_MAX_LEVELS, len(maps)))
    levels = (_PointSampleLevel * len(maps))()
    row = 0
    for lv, m in zip(levels, maps):
        _need_cuda(m)
        _need_dtype(m, torch.float32, "map")
        if m.dim() != 4 or not m.is_contiguous() or m.shape[0] != maps[0].shape[0]:
            raise ValueError("point_sample: every map must be a contiguous [B, H, W, C] tensor")
        lv.map, lv.h, lv.w, lv.c, lv.offset = m.data_ptr(), m.shape[1], m.shape[2], m.shape[3], row
        row += m.shape[3]
    return levels, row


def _point_sample_shapes(shapes):
    """The level array of maps known by their (B, H, W, C) only (index, workspace queries)."""
    levels = (_PointSampleLevel * len(shapes))()
    row = 0
    for lv, (_, h, w, c) in zip(levels, shapes):
        lv.map, lv.h, lv.w, lv.c, lv.offset = None, h, w, c, row
        row += c
    return levels


def _point_sample_points(points, batch):
    _need_cuda(points, batch.sample_start, batch.params)
    _need_dtype(points, torch.float32, "points")
    if points.dim() != 2 or points.shape[1] < 3 or points.shape[0] != batch.num_points or \
            (points.shape[0] > 0 and points.stride(1) != 1):
        raise ValueError("point_sample: points must be [N = %d, >= 3] with unit column stride, got "
                         "%s" % (batch.num_points, tuple(points.shape)))
    return points.stride(0) if points.shape[0] > 1 else points.shape[1]


def point_sample_forward(points, batch, maps, align_corners):
    """points [N, >= 3], batch: PointSampleBatch, maps: [B, H_l, W_l, C_l] -> out [N, sum C_l]."""
    stride = _point_sample_points(points, batch)
    levels, row = _point_sample_levels(maps)
    if maps[0].shape[0] != batch.batch:
        raise ValueError("point_sample: %d samples but maps of batch %d" % (batch.batch,
                                                                           maps[0].shape[0]))
    out = torch.empty((batch.num_points, row), dtype=torch.float32, device=points.device)
    check(lib.msmd_point_sample_fwd_f32(_p(points), stride, batch.num_points,
                                        _p(batch.sample_start), batch.starts, batch.batch,
                                        _p(batch.params), levels, len(maps), int(align_corners),
                                        _p(out), _stream()), "msmd_point_sample_fwd_f32")
    return out


class PointSampleIndex:
    """The backward's index: per contribution (point, level, corner) its cell and weight, the
    by-cell lists (start / order) and the scan of the long lists' pieces."""
    __slots__ = ("cell", "weight", "start", "order", "piece_start", "cells", "num_points")

    def __init__(self, cell, weight, start, order, piece_start, cells, num_points):
        self.cell, self.weight, self.start, self.order = cell, weight, start, order
        self.piece_start, self.cells, self.num_points = piece_start, cells, num_points


def point_sample_index(points, batch, shapes, align_corners):
    """The index of point_sample_backward; depends on the points and the maps' (B, H, W, C)
    shapes only."""
    stride = _point_sample_points(points, batch)
    if not 1 <= len(shapes) <= POINT_SAMPLE_MAX_LEVELS:
        raise ValueError("point_sample: 1..%d levels, got %d" % (POINT_SAMPLE_MAX_LEVELS,
                                                                 len(shapes)))
    levels = _point_sample_shapes(shapes)
    n, nl, dev = batch.num_points, len(shapes), points.device
    nbytes = lib.msmd_point_sample_index_workspace_bytes(levels, nl, batch.batch, n)
    if nbytes == 0:
        raise ValueError("point_sample_index: the cells or the %d x %d x 4 contributions do not "
                         "fit 31 bits" % (n, nl))
    cells = sum(int(s[0] * s[1] * s[2]) for s in shapes)
    t = max(n * nl * 4, 1)
    cell = torch.empty(t, dtype=torch.int32, device=dev)
    weight = torch.empty(t, dtype=torch.float32, device=dev)
    order = torch.empty(t, dtype=torch.int32, device=dev)
    start = torch.empty(cells + 1, dtype=torch.int32, device=dev)
    piece_start = torch.empty(cells + 1, dtype=torch.int32, device=dev)
    ws = _ws(nbytes, dev)
    check(lib.msmd_point_sample_index(_p(points), stride, n, _p(batch.sample_start), batch.starts,
                                      batch.batch, _p(batch.params), levels, nl,
                                      int(align_corners), _p(cell), _p(weight), _p(start),
                                      _p(order), _p(piece_start), _p(ws), ws.numel(), _stream()),
          "msmd_point_sample_index")
    return PointSampleIndex(cell, weight, start, order, piece_start, cells, n)


def point_sample_backward(grad_out, index, shapes, grads=None):
    """grad_out [N, sum C_l] -> the maps' gradients, channels-last [B, H_l, W_l, C_l] (every
    cell written; `grads`: buffers to write into).  shapes: the maps' (B, H, W, C)."""
    _need_cuda(grad_out)
    _need_dtype(grad_out, torch.float32, "grad_out")
    if grads is None:
        grads = [torch.empty(tuple(s), dtype=torch.float32, device=grad_out.device)
                 for s in shapes]
    levels, row = _point_sample_levels(grads)
    if tuple(grad_out.shape) != (index.num_points, row) or not grad_out.is_contiguous():
        raise ValueError("grad_out must be a contiguous [%d, %d] tensor, got %s"
                         % (index.num_points, row, tuple(grad_out.shape)))
    b = grads[0].shape[0]
    nbytes = lib.msmd_point_sample_bwd_workspace_bytes(levels, len(grads), b, index.num_points)
    ws = _ws(nbytes, grad_out.device)
    check(lib.msmd_point_sample_bwd_f32(_p(grad_out), index.num_points, b, levels, len(grads),
                                        _p(index.weight), _p(index.start), _p(index.order),
                                        _p(index.piece_start), _p(ws), ws.numel(), _stream()),
          "msmd_point_sample_bwd_f32")
    return grads


# ------------------------------------------------------------------ ImVoteNet's VoteFusion (csrc/vote_fusion.hip)
VOTE_FUSION_MAX_K = lib.msmd_vote_fusion_max_k()
VOTE_FUSION_PARAMS = 41         # floats of msmd_vote_fusion_params


def vote_fusion(seeds, boxes, box_offsets, box_offsets_host, imgs, params, num_classes,
                max_imvote):
    """VoteFusion.forward for the whole batch in one launch (msmd_vote_fusion_f32).  seeds
    float32 [B, S, 3]; boxes float32 [T, 6] (l, t, r, b, conf, class), the samples' lists
    concatenated; box_offsets int32 [B + 1] on the device and the same numbers as a host
    sequence; imgs float32 [B, 3, Hpad, Wpad]; params float32 [B, 41] on the device (the layout
    of msmd_vote_fusion_params) -> (feat float32 [B, 5 + num_classes + 3, K S], mask bool
    [B, K S]), slot k of seed s in column k S + s."""
    _need_cuda(seeds, boxes, box_offsets, imgs, params)
    for t, what in ((seeds, "seeds"), (boxes, "boxes"), (imgs, "imgs"), (params, "params")):
        _need_dtype(t, torch.float32, what)
    _need_dtype(box_offsets, torch.int32, "box_offsets")
    if seeds.dim() != 3 or seeds.shape[2] != 3 or not seeds.is_contiguous():
        raise ValueError("seeds must be a contiguous float32 [B, S, 3] tensor, got %s"
                         % (tuple(seeds.shape),))
    batch, s = seeds.shape[:2]
    if boxes.dim() != 2 or boxes.shape[1] != 6 or not boxes.is_contiguous():
        raise ValueError("boxes must be a contiguous float32 [T, 6] tensor, got %s"
                         % (tuple(boxes.shape),))
    if imgs.dim() != 4 or imgs.shape[0] != batch or imgs.shape[1] != 3 or not imgs.is_contiguous():
        raise ValueError("imgs must be a contiguous float32 [B = %d, 3, H, W] tensor, got %s"
                         % (batch, tuple(imgs.shape)))
    if tuple(params.shape) != (batch, VOTE_FUSION_PARAMS) or not params.is_contiguous():
        raise ValueError("params must be a contiguous float32 [%d, %d] tensor, got %s"
                         % (batch, VOTE_FUSION_PARAMS, tuple(params.shape)))
    if box_offsets.numel() != batch + 1 or len(box_offsets_host) != batch + 1 or \
            not box_offsets.is_contiguous():
        raise ValueError("box_offsets holds B + 1 entries, on the device and on the host")
    k, classes = int(max_imvote), int(num_classes)
    host = (C.c_int * (batch + 1))(*[int(v) for v in box_offsets_host])
    feat = torch.empty((batch, 5 + classes + 3, max(k, 0) * s), dtype=torch.float32,
                       device=seeds.device)
    mask = torch.empty((batch, max(k, 0) * s), dtype=torch.uint8, device=seeds.device)
    check(lib.msmd_vote_fusion_f32(_p(seeds), batch, s, _p(boxes), boxes.shape[0],
                                   _p(box_offsets), host, _p(imgs), imgs.shape[2], imgs.shape[3],
                                   _p(params), classes, k, _p(feat), _p(mask), _stream()),
          "msmd_vote_fusion_f32")
    return feat, mask.view(torch.bool)


# ------------------------------------------------------------------ TransFusionHead's image stage (csrc/img_fusion.hip)
IMG_GEOMETRY_MAX_QUERIES = lib.msmd_img_query_geometry_max_queries()
IMG_GEOMETRY_MAX_VIEWS = lib.msmd_img_query_geometry_max_views()
IMG_GEOMETRY_PARAMS = 20        # floats of msmd_point_sample_params
GAUSS_ATTN_KEY_TILE = lib.msmd_gauss_attn_key_tile()       # keys per block of the dK / dV pass
GAUSS_ATTN_ROW_CHUNK = lib.msmd_gauss_attn_row_chunk()     # rows per LDS round of that pass


class ImgQueryGeometry:
    """What img_query_geometry leaves on the device (shapes in include/msmd_hip.h)."""
    __slots__ = ("on", "pos", "centre", "radius", "sigma", "count", "valid", "winner", "mask",
                 "win_pos", "win_centre", "win_sigma")


def img_query_geometry(pos3d, boxes, params, out_size_factor_img):
    """transfusion_head.py:943-995 and the bookkeeping of :985-987 / :1004-1006 for the whole
    batch in one launch (msmd_img_query_geometry_f32).  pos3d float32 [B, 3, P]; boxes float32
    [B, P, 7]; params float32 [B, V, 20] (msmd_point_sample_params per (sample, view))."""
    _need_cuda(pos3d, boxes, params)
    for t, what in ((pos3d, "pos3d"), (boxes, "boxes"), (params, "params")):
        _need_dtype(t, torch.float32, what)
    if pos3d.dim() != 3 or pos3d.shape[1] != 3 or not pos3d.is_contiguous():
        raise ValueError("pos3d must be a contiguous float32 [B, 3, P] tensor, got %s"
                         % (tuple(pos3d.shape),))
    b, _, p = pos3d.shape
    if tuple(boxes.shape) != (b, p, 7) or not boxes.is_contiguous():
        raise ValueError("boxes must be a contiguous float32 [%d, %d, 7] tensor, got %s"
                         % (b, p, tuple(boxes.shape)))
    if params.dim() != 3 or params.shape[0] != b or params.shape[2] != IMG_GEOMETRY_PARAMS or \
            not params.is_contiguous():
        raise ValueError("params must be a contiguous float32 [%d, V, %d] tensor, got %s"
                         % (b, IMG_GEOMETRY_PARAMS, tuple(params.shape)))
    v = params.shape[1]
    if not 1 <= v <= IMG_GEOMETRY_MAX_VIEWS:
        raise ValueError("img_query_geometry: 1..%d views, got %d" % (IMG_GEOMETRY_MAX_VIEWS, v))
    if p > IMG_GEOMETRY_MAX_QUERIES:
        raise ValueError("img_query_geometry: at most %d queries, got %d"
                         % (IMG_GEOMETRY_MAX_QUERIES, p))
    if not float(out_size_factor_img) > 0:
        raise ValueError("out_size_factor_img must be positive")
    dev = pos3d.device

    def new(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)
    g = ImgQueryGeometry()
    g.on, g.pos = new((b, v, p), torch.uint8), new((b, v, p, 2), torch.float32)
    g.centre, g.radius = new((b, v, p, 2), torch.int32), new((b, v, p), torch.int32)
    g.sigma = new((b, v, p), torch.float32)
    g.count, g.valid = new((b, v), torch.int32), new((b, v), torch.uint8)
    g.winner, g.mask = new((b, p), torch.int32), new((b, p), torch.uint8)
    g.win_pos, g.win_centre = new((b, p, 2), torch.float32), new((b, p, 2), torch.int32)
    g.win_sigma = new((b, p), torch.float32)
    check(lib.msmd_img_query_geometry_f32(
        _p(pos3d), _p(boxes), _p(params), b, p, v, float(out_size_factor_img), _p(g.on), _p(g.pos),
        _p(g.centre), _p(g.radius), _p(g.sigma), _p(g.count), _p(g.valid), _p(g.winner),
        _p(g.mask), _p(g.win_pos), _p(g.win_centre), _p(g.win_sigma), _stream()),
        "msmd_img_query_geometry_f32")
    g.on, g.valid, g.mask = g.on.view(torch.bool), g.valid.view(torch.bool), g.mask.view(torch.bool)
    return g


def gauss_attn_supported(channels, heads):
    """Whether the window-attention kernels are built for this width (C / heads of 8, 16, 32,
    C <= 256)."""
    return bool(lib.msmd_gauss_attn_supported(int(channels), int(heads)))


def _gauss_attn_args(q, k, v, view, centre, sigma, num_views, h, w, heads, dropout):
    _need_cuda(q, k, v, view, centre, sigma)
    for t, what in ((q, "q"), (k, "k"), (v, "v"), (sigma, "sigma")):
        _need_dtype(t, torch.float32, what)
    _need_dtype(view, torch.int32, "view")
    _need_dtype(centre, torch.int32, "centre")
    if q.dim() != 2 or not q.is_contiguous():
        raise ValueError("q must be a contiguous float32 [B P, C] tensor, got %s" % (tuple(q.shape),))
    rows, c = q.shape
    num_views, h, w, heads = int(num_views), int(h), int(w), int(heads)
    if not gauss_attn_supported(c, heads):
        raise ValueError("gauss_attn: C / heads must be 8, 16 or 32 with C <= 256, got %d / %d"
                         % (c, heads))
    if not 1 <= num_views <= IMG_GEOMETRY_MAX_VIEWS or h < 1 or w < 1:
        raise ValueError("gauss_attn: 1..%d views and a map of at least 1 x 1, got V = %d, %d x %d"
                         % (IMG_GEOMETRY_MAX_VIEWS, num_views, h, w))
    if k.dim() != 3 or k.shape[1:] != (h * w, c) or k.shape[0] % num_views or \
            k.shape != v.shape or not k.is_contiguous() or not v.is_contiguous():
        raise ValueError("k and v must be contiguous float32 [B V, %d, %d] tensors, got %s and %s"
                         % (h * w, c, tuple(k.shape), tuple(v.shape)))
    batch = k.shape[0] // num_views
    if batch == 0 or rows % batch:
        raise ValueError("gauss_attn: %d rows do not divide over %d samples" % (rows, batch))
    if tuple(view.shape) != (rows,) or tuple(centre.shape) != (rows, 2) or \
            tuple(sigma.shape) != (rows,) or not view.is_contiguous() or \
            not centre.is_contiguous() or not sigma.is_contiguous():
        raise ValueError("view [R], centre [R, 2] and sigma [R] must be contiguous with R = %d"
                         % rows)
    if not 0.0 <= float(dropout) < 1.0:
        raise ValueError("dropout must be in [0, 1), got %r" % (dropout,))
    for t, what in ((q, "q"), (k, "k"), (v, "v")):
        if t.data_ptr() % 16:
            raise ValueError("gauss_attn: %s must start on a 16-byte boundary (the kernels load "
                             "four floats at a time)" % what)
    return batch, rows // batch, c


def _aligned16(t):
    """t contiguous and on a 16-byte boundary (a copy where a view is not)."""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def gauss_attn_forward(q, k, v, view, centre, sigma, num_views, h, w, heads, dropout=0.0, seed=0):
    """msmd_gauss_attn_fwd_f32 -> (out [B P, C], lse [B P, heads])."""
    batch, p, c = _gauss_attn_args(q, k, v, view, centre, sigma, num_views, h, w, heads, dropout)
    out = torch.empty_like(q)
    lse = torch.empty((q.shape[0], int(heads)), dtype=torch.float32, device=q.device)
    check(lib.msmd_gauss_attn_fwd_f32(_p(q), _p(k), _p(v), _p(view), _p(centre), _p(sigma), batch,
                                      p, int(num_views), int(h), int(w), c, int(heads),
                                      float(dropout), int(seed) & (2 ** 64 - 1), _p(out), _p(lse),
                                      _stream()), "msmd_gauss_attn_fwd_f32")
    return out, lse


def gauss_attn_backward(q, k, v, out, grad_out, lse, view, centre, sigma, num_views, h, w, heads,
                        dropout=0.0, seed=0):
    """msmd_gauss_attn_bwd_f32 -> (grad_q, grad_k, grad_v); the dropout mask is regenerated."""
    batch, p, c = _gauss_attn_args(q, k, v, view, centre, sigma, num_views, h, w, heads, dropout)
    _need_cuda(out, grad_out, lse)
    for t, what in ((out, "out"), (grad_out, "grad_out"), (lse, "lse")):
        _need_dtype(t, torch.float32, what)
    if out.shape != q.shape or grad_out.shape != q.shape or not out.is_contiguous() or \
            not grad_out.is_contiguous() or tuple(lse.shape) != (q.shape[0], int(heads)) or \
            not lse.is_contiguous():
        raise ValueError("out and grad_out must be contiguous like q, lse [R, heads]")
    if out.data_ptr() % 16 or grad_out.data_ptr() % 16:
        raise ValueError("gauss_attn: out and grad_out must start on a 16-byte boundary")
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty_like(lse)
    check(lib.msmd_gauss_attn_bwd_f32(_p(q), _p(k), _p(v), _p(out), _p(grad_out), _p(lse), _p(view),
                                      _p(centre), _p(sigma), batch, p, int(num_views), int(h),
                                      int(w), c, int(heads), float(dropout),
                                      int(seed) & (2 ** 64 - 1), _p(gq), _p(gk), _p(gv), _p(delta),
                                      _stream()), "msmd_gauss_attn_bwd_f32")
    return gq, gk, gv


class _GaussAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, view, centre, sigma, num_views, h, w, heads, dropout, seed):
        q, k, v = _aligned16(q), _aligned16(k), _aligned16(v)
        out, lse = gauss_attn_forward(q, k, v, view, centre, sigma, num_views, h, w, heads,
                                      dropout, seed)
        ctx.save_for_backward(q, k, v, out, lse, view, centre, sigma)
        ctx.args = (num_views, h, w, heads, dropout, seed)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, out, lse, view, centre, sigma = ctx.saved_tensors
        gq, gk, gv = gauss_attn_backward(q, k, v, out, _aligned16(grad_out), lse, view, centre,
                                         sigma, *ctx.args)
        return (gq, gk, gv) + (None,) * 9


def gauss_attn(q, k, v, view, centre, sigma, num_views, h, w, heads, dropout=0.0, seed=0):
    """Gaussian-window cross-attention with autograd (q, k, v); see gauss_attn_forward."""
    return _GaussAttn.apply(q, k, v, view, centre, sigma, num_views, h, w, heads, dropout, seed)


# ------------------------------------------------------------------ H3DNet primitive targets
PRIMITIVE_MODES = {"z": 0, "xy": 1, "line": 2}
PRIMITIVE_NUM_DIMS = {"z": 2, "xy": 1, "line": 0}
# labels outside [0, label_bound) take no part (a deviation from the reference, which accepts
# any label); the default is the library's limit, msmd_primitive_max_labels()
PRIMITIVE_MAX_LABELS = 1024


def _primitive_offsets(point_offsets, total):
    _need_dtype(point_offsets, torch.int32, "offsets")
    samples = point_offsets.numel() - 1
    if samples < 0 or point_offsets.dim() != 1 or not point_offsets.is_contiguous():
        raise ValueError("offsets hold S + 1 contiguous int32 entries")
    return samples


def primitive_index(pts_semantic_mask, pts_instance_mask, point_offsets, num_classes,
                    label_bound=None, max_points=None, max_instances=None):
    """The mode-independent index of msmd_primitive_targets_f32 for a batch: the instances of
    every sample (distinct instance labels of the points with sem != num_classes, ascending),
    their class point and their points in ascending order.  Masks long [P], sample s = rows
    point_offsets[s] .. point_offsets[s+1] (int32 [S + 1] on the device).  Labels outside
    [0, label_bound) take no part; label_bound defaults to PRIMITIVE_MAX_LABELS.  max_points /
    max_instances: host-known bounds that size grids only.  -> an opaque uint8 tensor; build it
    once per step and hand it to the three heads."""
    _need_cuda(pts_semantic_mask, pts_instance_mask, point_offsets)
    total = pts_semantic_mask.numel()
    for t, what in ((pts_semantic_mask, "pts_semantic_mask"),
                    (pts_instance_mask, "pts_instance_mask")):
        _need_dtype(t, torch.long, what)
        if t.dim() != 1 or t.numel() != total or not t.is_contiguous():
            raise ValueError("%s must be a contiguous long [P] tensor" % what)
    samples = _primitive_offsets(point_offsets, total)
    bound = PRIMITIVE_MAX_LABELS if label_bound is None else int(label_bound)
    nbytes = lib.msmd_primitive_index_workspace_bytes(samples, total, bound)
    if nbytes == 0:
        raise ValueError("primitive_index: label_bound must be in 1 .. %d" % PRIMITIVE_MAX_LABELS)
    index = torch.empty((nbytes,), dtype=torch.uint8, device=pts_semantic_mask.device)
    check(lib.msmd_primitive_index(_p(pts_semantic_mask), _p(pts_instance_mask),
                                   _p(point_offsets), samples, total,
                                   total if max_points is None else int(max_points),
                                   int(num_classes), bound,
                                   bound if max_instances is None else int(max_instances),
                                   _p(index), nbytes, _stream()), "msmd_primitive_index")
    return index


def primitive_targets(points, pts_semantic_mask, point_offsets, corners, box_offsets, index, mode,
                      with_yaw, train_cfg, label_bound=None, max_points=None, max_boxes=None):
    """PrimitiveHead.get_targets_single for every sample in one launch, nothing read back.
    points float32 [P, >= 3]; corners float32 [T, 8, 3] in DepthBoxes.corners order with
    box_offsets like point_offsets; index from primitive_index (same offsets and label_bound);
    mode 'z' | 'xy' | 'line'; train_cfg holds dist_thresh, var_thresh, lower_thresh, num_point,
    num_point_line, line_thresh.  The box of an instance is corners[rank of its label], as in
    the reference.  -> (point_mask float32 [P], point_offset [P, 3], point_sem
    [P, 3 + num_dims + 1])."""
    _need_cuda(points, pts_semantic_mask, point_offsets, corners, box_offsets, index)
    _need_dtype(points, torch.float32, "points")
    _need_dtype(corners, torch.float32, "corners")
    _need_dtype(pts_semantic_mask, torch.long, "pts_semantic_mask")
    _need_dtype(index, torch.uint8, "index")
    if points.dim() != 2 or points.shape[1] < 3 or not points.is_contiguous():
        raise ValueError("points must be a contiguous float32 [P, >= 3] tensor")
    if corners.dim() != 3 or tuple(corners.shape[1:]) != (8, 3) or not corners.is_contiguous():
        raise ValueError("corners must be a contiguous float32 [T, 8, 3] tensor")
    total = points.shape[0]
    if pts_semantic_mask.dim() != 1 or pts_semantic_mask.numel() != total or \
            not pts_semantic_mask.is_contiguous():
        raise ValueError("pts_semantic_mask must be a contiguous long [P] tensor")
    if mode not in PRIMITIVE_MODES:
        raise ValueError("primitive mode must be one of 'z', 'xy', 'line'")
    samples = _primitive_offsets(point_offsets, total)
    if _primitive_offsets(box_offsets, corners.shape[0]) != samples:
        raise ValueError("point_offsets and box_offsets hold S + 1 entries each")
    bound = PRIMITIVE_MAX_LABELS if label_bound is None else int(label_bound)
    dims = PRIMITIVE_NUM_DIMS[mode]
    dev = points.device
    mask = torch.empty((total,), dtype=torch.float32, device=dev)
    offset = torch.empty((total, 3), dtype=torch.float32, device=dev)
    sem = torch.empty((total, 4 + dims), dtype=torch.float32, device=dev)
    check(lib.msmd_primitive_targets_f32(
        _p(points), points.shape[1], _p(pts_semantic_mask), _p(point_offsets), _p(corners),
        _p(box_offsets), samples, total, corners.shape[0],
        total if max_points is None else int(max_points),
        corners.shape[0] if max_boxes is None else int(max_boxes), 1 if with_yaw else 0,
        PRIMITIVE_MODES[mode], dims, float(train_cfg["dist_thresh"]),
        float(train_cfg["var_thresh"]), float(train_cfg["lower_thresh"]),
        int(train_cfg["num_point"]), int(train_cfg["num_point_line"]),
        float(train_cfg["line_thresh"]), bound, _p(index), index.numel(), _p(mask), _p(offset),
        _p(sem), _stream()), "msmd_primitive_targets_f32")
    return mask, offset, sem


# ------------------------------------------------------------------ H3DNet second stage (row n8)
H3D_CUE_GT_CHUNK = lib.msmd_h3d_cue_gt_chunk()
H3D_CUE_PRED_CHUNK = lib.msmd_h3d_cue_pred_chunk()
H3D_CUE_PROPOSALS = lib.msmd_h3d_cue_proposals()
H3D_CUE_THRESHOLDS = ("near_threshold", "far_threshold", "label_surface_threshold",
                      "label_line_threshold", "mask_surface_threshold", "mask_line_threshold")
H3D_CUE_TARGET_NAMES = ("cues_objectness_label", "cues_sem_label", "proposal_objectness_label",
                        "cues_mask", "cues_match_mask", "proposal_objectness_mask",
                        "cues_matching_label", "obj_surface_line_center")


def _need_boxes7(boxes):
    _need_cuda(boxes)
    _need_dtype(boxes, torch.float32, "boxes")
    if boxes.dim() != 2 or boxes.shape[1] != 7 or not boxes.is_contiguous():
        raise ValueError("boxes must be a contiguous float32 [n, 7] tensor, got %s"
                         % (tuple(boxes.shape),))
    return boxes.shape[0]


def box_cue_centers_forward(boxes):
    """boxes float32 [n, 7] = (gravity centre, sizes, yaw) -> (surface [n * 6, 3], line
    [n * 12, 3]): get_surface_line_center (depth_box3d.py:277-330), its rotation-index quirk
    included (msmd_box_cue_centers_f32)."""
    n = _need_boxes7(boxes)
    surface = torch.empty((n * 6, 3), dtype=torch.float32, device=boxes.device)
    line = torch.empty((n * 12, 3), dtype=torch.float32, device=boxes.device)
    check(lib.msmd_box_cue_centers_f32(_p(boxes), n, _p(surface), _p(line), _stream()),
          "msmd_box_cue_centers_f32")
    return surface, line


def box_cue_centers_backward(boxes, grad_surface, grad_line):
    """-> grad_boxes [n, 7] for upstream [n * 6, 3] and [n * 12, 3]; fixed order, no atomics."""
    n = _need_boxes7(boxes)
    _need_cuda(grad_surface, grad_line)
    for t, rows, what in ((grad_surface, n * 6, "grad_surface"), (grad_line, n * 12, "grad_line")):
        _need_dtype(t, torch.float32, what)
        if tuple(t.shape) != (rows, 3) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float32 [%d, 3] tensor" % (what, rows))
    grad = torch.empty_like(boxes)
    check(lib.msmd_box_cue_centers_bwd_f32(_p(boxes), n, _p(grad_surface), _p(grad_line),
                                           _p(grad), _stream()), "msmd_box_cue_centers_bwd_f32")
    return grad


class _BoxCueCenters(torch.autograd.Function):
    @staticmethod
    def forward(ctx, boxes):
        boxes = boxes.contiguous()
        ctx.save_for_backward(boxes)
        return box_cue_centers_forward(boxes)

    @staticmethod
    def backward(ctx, grad_surface, grad_line):
        boxes, = ctx.saved_tensors
        n = boxes.shape[0]
        gs = boxes.new_zeros((n * 6, 3)) if grad_surface is None else grad_surface.contiguous()
        gl = boxes.new_zeros((n * 12, 3)) if grad_line is None else grad_line.contiguous()
        return box_cue_centers_backward(boxes, gs, gl)


def box_cue_centers(boxes):
    """box_cue_centers_forward, differentiable in all seven columns."""
    return _BoxCueCenters.apply(boxes)


def h3d_cue_targets(aggregated, gt_boxes, gt_counts, gt_labels, surface_pred, line_pred,
                    surface_sem, line_sem, surface_obj, line_obj, train_cfg):
    """H3DBboxHead.get_targets_single (h3d_bbox_head.py:761-932) for every sample in one launch
    (msmd_h3d_cue_targets_f32), nothing read back.  aggregated [B, P, 3]; gt_boxes [B, G, 7]
    in gravity-centre form, zero padded, with gt_counts int32 [B] and gt_labels long [B, G];
    surface_pred [B, Ns, 3], line_pred [B, Nl, 3] with scores [B, Ns, C], [B, Nl, C];
    surface_obj [B, 6 P, 3] and line_obj [B, 12 P, 3], the proposals' own cue centres;
    train_cfg holds H3D_CUE_THRESHOLDS.  -> the reference's eight results stacked, in its
    order (H3D_CUE_TARGET_NAMES)."""
    floats = ((aggregated, "aggregated"), (gt_boxes, "gt_boxes"), (surface_pred, "surface_pred"),
              (line_pred, "line_pred"), (surface_sem, "surface_sem"), (line_sem, "line_sem"),
              (surface_obj, "surface_obj"), (line_obj, "line_obj"))
    _need_cuda(gt_counts, gt_labels, *[t for t, _ in floats])
    for t, what in floats:
        _need_dtype(t, torch.float32, what)
        if t.dim() != 3 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float32 [B, N, C] tensor, got %s"
                             % (what, tuple(t.shape)))
    _need_dtype(gt_counts, torch.int32, "gt_counts")
    _need_dtype(gt_labels, torch.long, "gt_labels")
    b, p = aggregated.shape[:2]
    g, ns, nl, c = gt_boxes.shape[1], surface_pred.shape[1], line_pred.shape[1], \
        surface_sem.shape[2]
    want = ((aggregated, (b, p, 3)), (gt_boxes, (b, g, 7)), (surface_pred, (b, ns, 3)),
            (line_pred, (b, nl, 3)), (surface_sem, (b, ns, c)), (line_sem, (b, nl, c)),
            (surface_obj, (b, 6 * p, 3)), (line_obj, (b, 12 * p, 3)), (gt_labels, (b, g)),
            (gt_counts, (b,)))
    for t, shape in want:
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("h3d_cue_targets: expected a contiguous %s tensor, got %s"
                             % (shape, tuple(t.shape)))
    dev = aggregated.device
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)       # noqa: E731
    l = lambda *shape: torch.empty(shape, dtype=torch.long, device=dev)          # noqa: E731,E741
    obj_label, sem_label, match_label, cues_mask = l(b, 18 * p), l(b, 18 * p), l(b, 18 * p), \
        f(b, 18 * p)
    prop_label, prop_mask, match_mask, centers = l(b, p), f(b, p), f(b, p), f(b, 18 * p, 3)
    check(lib.msmd_h3d_cue_targets_f32(
        _p(aggregated), _p(gt_boxes), _p(gt_counts), _p(gt_labels), _p(surface_pred),
        _p(line_pred), _p(surface_sem), _p(line_sem), _p(surface_obj), _p(line_obj), b, p, g, ns,
        nl, c, *[float(train_cfg[k]) for k in H3D_CUE_THRESHOLDS], _p(obj_label), _p(sem_label),
        _p(match_label), _p(cues_mask), _p(prop_label), _p(prop_mask), _p(match_mask),
        _p(centers), _stream()), "msmd_h3d_cue_targets_f32")
    return (obj_label, sem_label, prop_label, cues_mask, match_mask, prop_mask, match_label,
            centers)


# ------------------------------------------------ Part-A2 semantic / part targets (row n9)
SEMANTIC_GT_CHUNK = lib.msmd_semantic_gt_chunk()


def semantic_targets(voxel_centers, batch_ids, gt_boxes, enlarged_boxes, gt_labels, gt_counts,
                     num_classes):
    """PointwiseSemanticHead.get_targets (pointwise_semantic_head.py:78-157) for every sample
    in one launch (msmd_semantic_targets_f32), nothing read back.  voxel_centers float32 [N, 3];
    batch_ids int32 [N] (coors[:, 0], any order); gt_boxes / enlarged_boxes float32 [B, G, 7]
    (LiDAR, bottom centre; the second is enlarged_box(extra_width) of the first), gt_labels long
    or int32 [B, G], gt_counts int32 [B] on the device.
    -> (seg_targets long [N], part_targets float32 [N, 3]), both written in full by the kernel,
    in input row order."""
    _need_cuda(voxel_centers, batch_ids, gt_boxes, enlarged_boxes, gt_labels, gt_counts)
    for t, what in ((voxel_centers, "voxel_centers"), (gt_boxes, "gt_boxes"),
                    (enlarged_boxes, "enlarged_boxes")):
        _need_dtype(t, torch.float32, what)
    _need_dtype(batch_ids, torch.int32, "batch_ids")
    _need_dtype(gt_counts, torch.int32, "gt_counts")
    if gt_labels.dtype not in (torch.long, torch.int32):
        raise ValueError("gt_labels must be long or int32, got %s" % gt_labels.dtype)
    if voxel_centers.dim() != 2 or voxel_centers.shape[1] != 3:
        raise ValueError("voxel_centers must be [N, 3], got %s" % (tuple(voxel_centers.shape),))
    n = voxel_centers.shape[0]
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 7:
        raise ValueError("gt_boxes must be [B, G, 7], got %s" % (tuple(gt_boxes.shape),))
    b, g = gt_boxes.shape[:2]
    want = ((voxel_centers, (n, 3)), (batch_ids, (n,)), (gt_boxes, (b, g, 7)),
            (enlarged_boxes, (b, g, 7)), (gt_labels, (b, g)), (gt_counts, (b,)))
    for t, shape in want:
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("semantic_targets: expected a contiguous %s tensor, got %s"
                             % (shape, tuple(t.shape)))
    dev = voxel_centers.device
    seg = torch.empty((n,), dtype=torch.long, device=dev)
    part = torch.empty((n, 3), dtype=torch.float32, device=dev)
    check(lib.msmd_semantic_targets_f32(
        _p(voxel_centers), _p(batch_ids), _p(gt_boxes), _p(enlarged_boxes), _p(gt_labels),
        int(gt_labels.dtype == torch.long), _p(gt_counts), n, b, g, int(num_classes), _p(seg),
        _p(part), _stream()), "msmd_semantic_targets_f32")
    return seg, part


# ------------------------------------------------ Part-A2 RoI assignment / sampling (row n10)
ROI_ASSIGN_MAX_SAMPLES = lib.msmd_roi_assign_max_samples()
ROI_ASSIGN_MAX_CLASSES = lib.msmd_roi_assign_max_classes()
ROI_ASSIGN_GT_CHUNK = lib.msmd_roi_assign_gt_chunk()
ROI_SAMPLE_MAX_PROPOSALS = lib.msmd_roi_sample_max_proposals()
ROI_SAMPLE_MAX_NUM = lib.msmd_roi_sample_max_num()
ROI_SAMPLE_MAX_PIECES = lib.msmd_roi_sample_max_pieces()


def _roi_lists(proposals, proposal_offsets, gt_boxes, gt_offsets):
    _need_cuda(proposals, gt_boxes)
    poffs, goffs = [int(v) for v in proposal_offsets], [int(v) for v in gt_offsets]
    if len(poffs) != len(goffs) or len(poffs) < 1:
        raise ValueError("proposal_offsets and gt_offsets hold one entry per sample plus one")
    for t, offs, what in ((proposals, poffs, "proposals"), (gt_boxes, goffs, "gt_boxes")):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 7 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float32 [n, 7] tensor, got %s %s"
                             % (what, t.dtype, tuple(t.shape)))
        if offs[0] != 0 or offs[-1] != t.shape[0] or any(b < a for a, b in zip(offs, offs[1:])):
            raise ValueError("%s: the offsets must ascend from 0 to %d, got %s"
                             % (what, t.shape[0], offs))
    return poffs, goffs


def roi_assign3d(proposals, proposal_labels, proposal_offsets, gt_boxes, gt_labels, gt_offsets,
                 pos_iou_thr, neg_iou_thr, min_pos_iou, single=False):
    """Class-aware MaxIoUAssigner over the 3-D IoU for every sample of the batch
    (msmd_roi_assign3d_f32): no IoU matrix, nothing read back.  proposals float32 [P, 7],
    proposal_labels long [P] (None with single=True), gt_boxes float32 [G, 7], gt_labels long
    [G]; proposal_offsets / gt_offsets: HOST sequences [B + 1].  Thresholds: one float per class
    (host), one in all with single=True.
    -> gt_inds int32 [P] (-1 ignored, 0 background, i + 1 with i local to the sample's list),
       max_overlaps float32 [P], labels long [P] (-1 where unassigned)."""
    poffs, goffs = _roi_lists(proposals, proposal_offsets, gt_boxes, gt_offsets)
    _need_cuda(proposal_labels, gt_labels)
    batch, p, g = len(poffs) - 1, proposals.shape[0], gt_boxes.shape[0]
    classes = len(pos_iou_thr)
    if not (len(neg_iou_thr) == len(min_pos_iou) == classes) or classes < 1:
        raise ValueError("every threshold list holds one entry per class")
    if single and classes != 1:
        raise ValueError("the single-assigner form takes one threshold triple")
    if not single and (proposal_labels is None or proposal_labels.dtype != torch.long
                       or proposal_labels.numel() != p or not proposal_labels.is_contiguous()):
        raise ValueError("proposal_labels must be a contiguous long tensor, one per proposal")
    if gt_labels.dtype != torch.long or gt_labels.numel() != g or not gt_labels.is_contiguous():
        raise ValueError("gt_labels must be a contiguous long tensor with one entry per box")
    dev = proposals.device
    gt_inds = torch.empty((p,), dtype=torch.int32, device=dev)
    overlaps = torch.empty((p,), dtype=torch.float32, device=dev)
    labels = torch.empty((p,), dtype=torch.long, device=dev)
    nbytes = lib.msmd_roi_assign3d_workspace_bytes(g)
    ws = _ws(nbytes, dev)
    check(lib.msmd_roi_assign3d_f32(
        _p(proposals), None if single else _p(proposal_labels), _host_ints(poffs), _p(gt_boxes),
        _p(gt_labels), _host_ints(goffs), batch, classes, int(bool(single)),
        float_arr(pos_iou_thr), float_arr(neg_iou_thr), float_arr(min_pos_iou), _p(gt_inds),
        _p(overlaps), _p(labels), _p(ws), nbytes, _stream()), "msmd_roi_assign3d_f32")
    return gt_inds, overlaps, labels


def roi_sample_targets(proposals, proposal_offsets, gt_inds, max_overlaps, keys, gt_boxes,
                       gt_offsets, num, num_expected_pos, neg_pos_ub, neg_piece_fractions,
                       neg_iou_piece_thrs, cls_pos_thr, cls_neg_thr):
    """IoUNegPiecewiseSampler.sample + PartA2BboxHead._get_target_single for every sample in one
    launch (msmd_roi_sample_targets_f32), nothing read back.  gt_inds int32 / max_overlaps
    float32 [P] as roi_assign3d returns them, keys float32 [P]: random_choice takes the smallest
    keys, ties to the lower index.
    -> dict of tensors padded to `num` rows per sample: rois [B, num, 8], iou, label,
       label_weights, reg_mask (long), bbox_weights [B, num], pos_gt_bboxes, bbox_targets
       [B, num, 7], inds int32 [B, num] (proposal index in its sample, -1 padding), counts int32
       [B, 2] = (positives, negatives); a sample's rows are its positives, then its negatives,
       each ascending."""
    poffs, goffs = _roi_lists(proposals, proposal_offsets, gt_boxes, gt_offsets)
    _need_cuda(gt_inds, max_overlaps, keys)
    batch, p = len(poffs) - 1, proposals.shape[0]
    for t, dtype, what in ((gt_inds, torch.int32, "gt_inds"),
                           (max_overlaps, torch.float32, "max_overlaps"),
                           (keys, torch.float32, "keys")):
        if t.dtype != dtype or t.numel() != p or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor with one entry per proposal"
                             % (what, dtype))
    pieces = len(neg_piece_fractions)
    if pieces != len(neg_iou_piece_thrs) or pieces < 1:
        raise ValueError("neg_piece_fractions and neg_iou_piece_thrs hold one entry per piece")
    num = int(num)
    dev = proposals.device

    def out(shape, dtype=torch.float32):
        return torch.empty((batch, num) + shape, dtype=dtype, device=dev)

    res = dict(rois=out((8,)), iou=out(()), label=out(()), label_weights=out(()),
               reg_mask=out((), torch.long), bbox_weights=out(()), pos_gt_bboxes=out((7,)),
               bbox_targets=out((7,)), inds=out((), torch.int32),
               counts=torch.empty((batch, 2), dtype=torch.int32, device=dev))
    fractions = (C.c_double * pieces)(*[float(v) for v in neg_piece_fractions])
    check(lib.msmd_roi_sample_targets_f32(
        _p(proposals), _host_ints(poffs), _p(gt_inds), _p(max_overlaps), _p(keys), _p(gt_boxes),
        _host_ints(goffs), batch, num, int(num_expected_pos), float(neg_pos_ub), pieces, fractions,
        float_arr(neg_iou_piece_thrs), float(cls_pos_thr), float(cls_neg_thr), _p(res["rois"]),
        _p(res["iou"]), _p(res["label"]), _p(res["label_weights"]), _p(res["reg_mask"]),
        _p(res["bbox_weights"]), _p(res["pos_gt_bboxes"]), _p(res["bbox_targets"]),
        _p(res["inds"]), _p(res["counts"]), _stream()), "msmd_roi_sample_targets_f32")
    return res
