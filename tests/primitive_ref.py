"""The per-sample loop of H3DNet's PrimitiveHead.get_targets_single (reference
mmdet3d/models/roi_heads/mask_heads/primitive_head.py:327-601 with its helpers), restated in
plain torch as the yardstick of the primitive-target kernels.  Table driven, written for this
project; it runs in float32 (the reference's arithmetic, operation by operation) or float64 (the
truth the float32 error is measured against), on the CPU or -- for the timing record -- on a
device, where every `if` on a tensor is the host read the reference has.

Three behaviours differ from the reference on purpose, as the kernel's do (include/msmd_hip.h):
an instance whose rank is not below the box count gets no targets (IndexError there), an
instance whose box fails one of the reference's NotImplementedError checks gets none either,
and labels outside [0, label_bound) take no part when a label_bound is given.
"""
import torch

NUM_DIMS = {"z": 2, "xy": 1, "line": 0}
# corner pairs of the lines, in the reference's write order
LINE_PAIRS = {"bottom": ((0, 3), (4, 7), (0, 4), (3, 7)), "top": ((1, 2), (5, 6), (1, 5), (2, 6)),
              "left": ((0, 1), (3, 2)), "right": ((4, 5), (7, 6))}
SURFACE_PAIRS = {"bottom": (0, 7), "top": (1, 6), "left": (0, 1), "right": (4, 5),
                 "front": (0, 1), "back": (3, 2)}


class Trace:
    """What the margin assertions need: every discrete decision and the figures behind it."""

    def __init__(self):
        self.reads = 0          # host reads (tensor -> bool) the loop made
        self.items = []         # (tag, dict) in evaluation order

    def add(self, tag, **kw):
        self.items.append((tag, kw))


def _decide(value, trace):
    if trace is not None:
        trace.reads += 1
    return bool(value)


def _plane(v1, v2, point):
    normal = torch.cross(v1, v2, dim=0)
    return torch.cat((normal, (-(normal * point).sum()).reshape(1)))


def _box_planes(c, lower_thresh, trace):
    """-> dict of the six planes (n, d), or None where the reference raises."""
    dtype = c.dtype
    top = c[[1, 2, 5, 6]]
    lower = c.new_tensor([0, 0, 1, -float(c[7, 2])]).to(dtype)
    lower[3] = -c[7, 2]
    horizon = (top[0, 2] == top[1, 2]) & (top[1, 2] == top[2, 2]) & (top[2, 2] == top[3, 2])
    if not (_decide(horizon, trace) and _decide(lower[0] + lower[1] < lower_thresh, trace)):
        return None
    refined = (top * lower[:3]).sum(dim=1)
    upper = lower.clone()
    upper[3] = -refined.mean()
    if not _decide((top[:, 2] + upper[3]).sum() / 4.0 < lower_thresh, trace):
        return None
    planes = {"bottom": lower, "top": upper}
    for near, far, (a, b, p), others in (("left", "right", ((2, 3), (3, 0), 0), [4, 5, 7, 6]),
                                         ("front", "back", ((0, 4), (4, 5), 5), [3, 2, 7, 6])):
        eq = _plane(c[a[0]] - c[a[1]], c[b[0]] - c[b[1]], c[p])
        eq = eq / torch.norm(eq[:3])
        if not _decide(eq[2] < lower_thresh, trace):
            return None
        other = eq.clone()
        other[3] = -((c[others] * eq[:3]).sum(dim=1)).mean()
        planes[near], planes[far] = eq, other
    return planes


def _line_select(pts, c, pair, kind, with_yaw, cfg, trace, tag):
    if with_yaw:
        a, b = c[pair[0]], c[pair[1]]
        a2b, a2p = b - a, pts - a
        length = (a2p * a2b.view(1, 3)).sum(1) / a2b.norm()
        radicand = a2p.norm(dim=1) ** 2 - length ** 2
        dist = radicand.sqrt()
    else:
        lo, hi = c.min(0)[0], c.max(0)[0]
        ref = (lo[0], hi[0], lo[1], hi[1])[kind]
        dist = torch.abs(pts[:, 0 if kind < 2 else 1] - ref)
        radicand = None
    sel = dist < cfg["line_thresh"]
    if trace is not None:
        trace.add("line", name=tag, dist=dist.detach().cpu(), selected=sel.cpu(),
                  radicand=None if radicand is None else radicand.detach().cpu())
    return sel


def primitive_targets_ref(points, sem, inst, corners, with_yaw, mode, num_classes, cfg,
                          dtype=torch.float32, label_bound=None, trace=None):
    """points [N, >= 3] float32, sem / inst long [N], corners [G, 8, 3] float32 ->
    (point_mask [N], point_offset [N, 3], point_sem [N, 3 + num_dims + 1]) in `dtype`."""
    pts = points[:, :3].to(dtype)
    corners = corners.to(dtype)
    n, width = pts.shape[0], 4 + NUM_DIMS[mode]
    mask = pts.new_zeros(n)
    offset = pts.new_zeros((n, 3))
    out = pts.new_zeros((n, width))
    fg = sem != num_classes
    if label_bound is not None:
        fg = fg & (inst >= 0) & (inst < label_bound)
    fg_idx = torch.nonzero(fg, as_tuple=False).squeeze(1)
    labels = inst[fg_idx].unique()
    if trace is not None:
        trace.reads += 1                      # nonzero / unique size the loop on the host
    for rank, label in enumerate(labels):
        if rank >= corners.shape[0]:
            break
        idx = fg_idx[inst[fg_idx] == label]
        xyz = pts[idx]
        cls = sem[idx][0].to(dtype)
        c = corners[rank]
        planes = _box_planes(c, cfg["lower_thresh"], trace)
        if planes is None:
            continue
        lo, hi, mean = c.min(0)[0], c.max(0)[0], c.mean(0)

        def write(sel_idx, sel_xyz, centre, sizes):
            mask[sel_idx] = 1.0
            offset[sel_idx] = centre - sel_xyz
            out[sel_idx] = torch.cat((centre, pts.new_tensor(sizes) if not sizes else
                                      torch.stack(sizes), cls.reshape(1)))

        def match(face):
            eq = planes[face]
            dist = torch.abs((xyz * eq[:3]).sum(dim=1) + eq[3])
            gap = torch.abs(dist - dist.min())
            sel = gap < cfg["dist_thresh"]
            if trace is not None:
                trace.add("plane", name="%d/%s" % (rank, face), gap=gap.detach().cpu(),
                          selected=sel.cpu())
            return dist, sel

        def surface(face):
            dist, sel = match(face)
            count, var = sel.sum(), dist[sel].var()
            if trace is not None:
                trace.add("surface", name="%d/%s" % (rank, face), count=int(count),
                          var=float(var))
            if not (_decide(count > cfg["num_point"], trace) and
                    _decide(var < cfg["var_thresh"], trace)):
                return
            a, b = SURFACE_PAIRS[face]
            sel_xyz = xyz[sel]
            if mode == "z":
                z = sel_xyz[:, 2].mean()
                if with_yaw:
                    mid = (c[a] + c[b]) / 2.0
                    centre = torch.stack((mid[0], mid[1], z))
                    sizes = [(c[4] - c[0]).norm(), (c[3] - c[0]).norm()]
                else:
                    centre = torch.stack((mean[0], mean[1], z))
                    sizes = [hi[0] - lo[0], hi[1] - lo[1]]
            else:
                m = sel_xyz.mean(0)
                if with_yaw:
                    centre = torch.stack((m[0], m[1], (c[a, 2] + c[b, 2]) / 2.0))
                    sizes = [c[b, 2] - c[a, 2]]
                else:
                    centre = torch.stack((m[0], m[1], mean[2]))
                    sizes = [hi[2] - lo[2]]
            write(idx[sel], sel_xyz, centre, sizes)

        def lines(face):
            _, sel = match(face)
            sel_idx, sel_xyz = idx[sel], xyz[sel]
            side = face in ("left", "right")
            kinds, axes = ((2, 3), (2, 2)) if side else ((0, 1, 2, 3), (1, 1, 0, 0))
            for pair, kind, axis in zip(LINE_PAIRS[face], kinds, axes):
                on = _line_select(sel_xyz, c, pair, kind, with_yaw, cfg, trace,
                                  "%d/%s/%d-%d" % ((rank, face) + pair))
                if trace is not None:
                    trace.add("line_count", name="%d/%s/%d-%d" % ((rank, face) + pair),
                              count=int(on.sum()))
                if not _decide(on.sum() > cfg["num_point_line"], trace):
                    continue
                if with_yaw:
                    centre = (c[pair[0]] + c[pair[1]]) / 2
                else:
                    centre = sel_xyz[on].mean(dim=0)
                    centre[axis] = mean[axis]
                write(sel_idx[on], sel_xyz[on], centre, [])

        if mode == "line":
            for face in ("bottom", "top", "left", "right"):
                lines(face)
        elif mode == "z":
            surface("bottom"), surface("top")
        else:
            for face in ("left", "right", "front", "back"):
                surface(face)
    return mask, offset, out


def batch_targets_ref(points, sems, insts, corners, with_yaw, mode, num_classes, cfg,
                      dtype=torch.float32, label_bound=None, trace=None):
    """Lists per sample -> the three outputs concatenated over the samples' rows."""
    outs = [primitive_targets_ref(p, s, i, c, with_yaw, mode, num_classes, cfg, dtype,
                                  label_bound, trace)
            for p, s, i, c in zip(points, sems, insts, corners)]
    return tuple(torch.cat([o[k] for o in outs]) for k in range(3))


def assert_margins(trace32, trace64, cfg):
    """The discrete outcomes are decided by float32 comparisons; an input is a fair test only
    where they are well defined: the same decisions in float32 and float64, no distance within
    1e-3 (relative) of dist_thresh / line_thresh, no variance within a factor 2 of var_thresh,
    no on-line radicand that changes sign between the precisions."""
    assert len(trace32.items) == len(trace64.items), "the two precisions took different paths"
    for (tag, a), (tag64, b) in zip(trace32.items, trace64.items):
        assert tag == tag64 and a["name"] == b["name"], (tag, a["name"], tag64, b["name"])
        if tag == "plane":
            assert torch.equal(a["selected"], b["selected"]), a["name"]
            rel = torch.abs(b["gap"] - cfg["dist_thresh"]) / cfg["dist_thresh"]
            assert not bool((rel < 1e-3).any()), "distance at dist_thresh: %s" % a["name"]
        elif tag == "line":
            assert torch.equal(a["selected"], b["selected"]), a["name"]
            if a["radicand"] is not None:
                assert torch.equal(a["radicand"] < 0, b["radicand"] < 0), \
                    "radicand changes sign: %s" % a["name"]
            d = b["dist"][~torch.isnan(b["dist"])]
            rel = torch.abs(d - cfg["line_thresh"]) / cfg["line_thresh"]
            assert not bool((rel < 1e-3).any()), "distance at line_thresh: %s" % a["name"]
        elif tag == "surface":
            assert a["count"] == b["count"], a["name"]
            if a["count"] > max(cfg["num_point"], 1):
                v = b["var"]
                assert not (cfg["var_thresh"] / 2 < v < cfg["var_thresh"] * 2), \
                    "variance %g at var_thresh: %s" % (v, a["name"])
                assert (a["var"] < cfg["var_thresh"]) == (v < cfg["var_thresh"]), a["name"]
        elif tag == "line_count":
            assert a["count"] == b["count"], a["name"]
