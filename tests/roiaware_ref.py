"""numpy restatement of RoI-aware pooling and points-in-boxes (the contract pinned in
msmdfusion_amd/csrc/roiaware.hip, after mmdet3d/ops/roiaware_pool3d/src/*.cu): the float /
double point-in-box predicate, the capped point lists in point order, the max / avg loops and
the backward summed per point in ascending RoI order in float32."""
import math

import numpy as np

F32 = np.float32


def local_coords(pts, boxes):
    """-> (inside[T, M] bool, local_x[T, M], local_y[T, M]) float32, the reference's mix of
    float and double (check_pt_in_box3d)."""
    p = np.asarray(pts, F32).reshape(-1, 3)
    b = np.asarray(boxes, F32).reshape(-1, 7)
    x, y, z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    cx, cy, zb, w, l, h, rz = (b[:, j:j + 1] for j in range(7))
    h2 = h.astype(np.float64) / 2.0
    cz = (zb.astype(np.float64) + h2).astype(F32)
    rot = (rz.astype(np.float64) + math.pi / 2).astype(F32)
    ca, sa = np.cos(rot).astype(F32), np.sin(rot).astype(F32)
    sx, sy = x - cx, y - cy
    lx = (sx * ca + sy * (-sa)).astype(F32)
    ly = (sx * sa + sy * ca).astype(F32)
    hl, hw = l.astype(np.float64) / 2.0, w.astype(np.float64) / 2.0
    with np.errstate(invalid="ignore"):
        zin = ~(np.abs(z - cz).astype(np.float64) > h2)
        inside = zin & (lx > -hl) & (lx < hl) & (ly > -hw) & (ly < hw)
    return inside, lx, ly


def points_in_boxes_first(pts_b, boxes_b):
    """[B, M, 3], [B, T, 7] -> [B, M] int32 first box or -1."""
    out = []
    for pts, boxes in zip(pts_b, boxes_b):
        inside, _, _ = local_coords(pts, boxes)
        any_ = inside.any(0)
        first = np.where(any_, inside.argmax(0), -1)
        out.append(first)
    return np.asarray(out, np.int32).reshape(len(out), -1)


def points_in_boxes_all(pts_b, boxes_b):
    """[B, M, 3], [B, T, 7] -> [B, M, T] int32 0 / 1."""
    return np.asarray([local_coords(p, b)[0].T for p, b in zip(pts_b, boxes_b)], np.int32)


def _clamp_idx(q, n):
    with np.errstate(invalid="ignore"):
        i = np.where(q > 0, q, 0).astype(np.int64)
    return np.clip(i, 0, n - 1)


def point_lists(rois, pts, out_size, max_pts_per_voxel, roi_batch=None, pts_batch=None):
    """-> {cell: kept point ids (ascending)} with cell = r * V + (ix*oy + iy)*oz + iz, and
    {cell: full count}.  Cells without points are absent."""
    ox, oy, oz = (out_size,) * 3 if isinstance(out_size, int) else tuple(out_size)
    vol = ox * oy * oz
    rois = np.asarray(rois, F32).reshape(-1, 7)
    pts = np.asarray(pts, F32).reshape(-1, 3)
    inside, lx, ly = local_coords(pts, rois)
    if roi_batch is not None or pts_batch is not None:
        rb = np.zeros(len(rois), np.int64) if roi_batch is None else np.asarray(roi_batch)
        pb = np.zeros(len(pts), np.int64) if pts_batch is None else np.asarray(pts_batch)
        inside &= rb[:, None] == pb[None, :]
    cap = max_pts_per_voxel - 1
    kept, full = {}, {}
    for r in range(len(rois)):
        idx = np.nonzero(inside[r])[0]
        if idx.size == 0:
            continue
        _, _, zb, w, l, h, _ = rois[r]
        ix = _clamp_idx((lx[r, idx] + l / F32(2)) / (l / F32(ox)), ox)
        iy = _clamp_idx((ly[r, idx] + w / F32(2)) / (w / F32(oy)), oy)
        iz = _clamp_idx((pts[idx, 2] - zb) / (h / F32(oz)), oz)
        cell = r * vol + (ix * oy + iy) * oz + iz
        order = np.argsort(cell, kind="stable")
        cell, idx = cell[order], idx[order]
        uniq, start, cnt = np.unique(cell, return_index=True, return_counts=True)
        for c, s, n in zip(uniq, start, cnt):
            full[int(c)] = int(n)
            kept[int(c)] = idx[s:s + min(n, cap)]
    return kept, full


def pool(feats, kept, num_cells, mode):
    """-> (pooled[cells, C] float32, argmax[cells, C] int32 | None): max from -inf, strictly
    greater wins, no winner -> 0 / -1; avg a float32 sum in point order, / count, empty 0."""
    feats = np.asarray(feats, F32)
    c = feats.shape[1]
    pooled = np.zeros((num_cells, c), F32)
    argmax = np.full((num_cells, c), -1, np.int32) if mode == "max" else None
    for cell, ids in kept.items():
        if mode == "max":
            mx = np.full(c, -np.inf, F32)
            arg = np.full(c, -1, np.int32)
            for p in ids:
                x = feats[p]
                with np.errstate(invalid="ignore"):
                    win = x > mx
                mx = np.where(win, x, mx)
                arg = np.where(win, p, arg)
            pooled[cell] = np.where(arg >= 0, mx, F32(0))
            argmax[cell] = arg
        elif len(ids):
            s = np.zeros(c, F32)
            for p in ids:
                s = (s + feats[p]).astype(F32)
            pooled[cell] = (s / F32(len(ids))).astype(F32)
    return pooled, argmax


def backward(grad_out, kept, num_points, mode, argmax=None, dtype=F32):
    """grad_in[P, C]: every point's contributions added in ascending RoI order (cells are
    visited in ascending order, and a point sits in at most one cell per RoI)."""
    g = np.asarray(grad_out).astype(dtype).reshape(-1, np.asarray(grad_out).shape[-1])
    out = np.zeros((num_points, g.shape[1]), dtype)
    for cell in sorted(kept):
        ids = kept[cell]
        if mode == "max":
            for p in ids:
                hit = argmax[cell] == p
                out[p] = np.where(hit, out[p] + g[cell], out[p]).astype(dtype)
        else:
            scale = dtype(1) / dtype(max(len(ids), 1))
            for p in ids:
                out[p] = (out[p] + g[cell] * scale).astype(dtype)
    return out
