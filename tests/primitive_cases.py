"""Generated inputs of the primitive-target tests: boxes with points on a lattice in the box
frame, so that every comparison the reference makes has a wide margin by construction (the
tests still re-check the margins on the restatement, primitive_ref.assert_margins).

Along each box axis of length 0.3 K the points sit at levels k = 0 .. K: level 0 and K lie
0.005 .. 0.02 inside the two faces, an interior level at 0.3 k +- 0.01.  With dist_thresh 0.1
and line_thresh 0.2 a distance to a face or an edge is then either below 0.03 or above 0.25,
and radicands of on-line distances are at least 5e-5, far above float32 rounding of |a2p|^2.
(With the config's dist_thresh 0.2 the nearest other level is still 0.26 away.)
A `bimodal` face puts half of its level-0 points 0.083 .. 0.087 inside instead: still selected
(gap 0.075 < 0.1), variance about 1.4e-3.
"""
import numpy as np
import torch

STEP = 0.3
SMALL_CFG = dict(dist_thresh=0.1, var_thresh=5e-3, lower_thresh=1e-6, num_point=5,
                 num_point_line=2, line_thresh=0.2)
# the bimodal face's variance (about 1.4e-3) fails this one, a plain face (< 6e-5) passes
VAR_CFG = dict(SMALL_CFG, var_thresh=5e-4)
# train_cfg of configs/_base_/models/h3dnet.py
CONFIG_CFG = dict(dist_thresh=0.2, var_thresh=1e-2, lower_thresh=1e-6, num_point=100,
                  num_point_line=10, line_thresh=0.2)
YAWS = (0.0, np.pi / 2, -np.pi / 2, 0.3, -1.1, 2.5, np.pi, 0.7853981)


def level_coords(rng, levels, k_max, bimodal=False):
    """levels int [m] in 0 .. k_max -> positions along an axis of length 0.3 k_max."""
    m = levels.shape[0]
    edge = rng.uniform(0.005, 0.02, m)
    if bimodal:
        deep = rng.uniform(0.083, 0.087, m)
        edge = np.where((np.arange(m) % 2 == 1) & (levels == 0), deep, edge)
    inner = STEP * levels + rng.uniform(-0.01, 0.01, m)
    length = STEP * k_max
    return np.where(levels == 0, edge, np.where(levels == k_max, length - edge, inner))


def random_levels(rng, m, k_max, p_edge=0.7):
    edge = rng.random(m) < p_edge
    side = rng.integers(0, 2, m) * k_max
    inner = rng.integers(1, k_max, m) if k_max > 1 else side
    return np.where(edge, side, inner)


def instance_points(rng, box, levels, ks, bimodal_axis=None):
    """box (x, y, z_bottom, dx, dy, dz, yaw) float64, levels int [m, 3] -> world points [m, 3]
    by DepthBoxes.corners' own transform (row vector times the transposed rotation)."""
    t = np.stack([level_coords(rng, levels[:, a], ks[a], bimodal=(bimodal_axis == a))
                  for a in range(3)], axis=1)
    local = t - np.array([box[3] / 2, box[4] / 2, 0.0])
    c, s = np.cos(box[6]), np.sin(box[6])
    x = local[:, 0] * c + local[:, 1] * s
    y = -local[:, 0] * s + local[:, 1] * c
    return np.stack([x + box[0], y + box[1], local[:, 2] + box[2]], axis=1)


def make_box(rng, slot, yaw, ks=None):
    ks = tuple(rng.integers(2, 5, 3)) if ks is None else ks
    centre = np.array([6.0 * (slot % 6), 6.0 * (slot // 6), rng.uniform(-1, 1)])
    return np.array([centre[0], centre[1], centre[2], STEP * ks[0], STEP * ks[1], STEP * ks[2],
                     yaw]), ks


def make_sample(seed, n_points, inst_sizes, with_yaw=True, num_classes=18, yaws=YAWS,
                label_stride=3, extra_dims=1, level_fn=None, bimodal=()):
    """A sample of n_points rows: instance r (r-th smallest label, label = 2 + stride r) owns
    inst_sizes[r] points of box r, the rest is background (sem == num_classes) shuffled in.
    level_fn(r, rng, m, ks) may give the instance's levels explicitly.  -> dict of tensors."""
    rng = np.random.default_rng(seed)
    assert sum(inst_sizes) <= n_points
    pts, sem, inst, boxes = [], [], [], []
    for r, m in enumerate(inst_sizes):
        box, ks = make_box(rng, r, yaws[r % len(yaws)] if with_yaw else 0.0)
        levels = None if level_fn is None else level_fn(r, rng, m, ks)
        if levels is None:
            levels = np.stack([random_levels(rng, m, ks[a]) for a in range(3)], axis=1)
        pts.append(instance_points(rng, box, levels, ks, bimodal_axis=2 if r in bimodal else None))
        sem.append(np.full(m, (5 * r + 1) % num_classes))
        inst.append(np.full(m, 2 + label_stride * r))
        boxes.append(box)
    n_bg = n_points - sum(inst_sizes)
    pts.append(rng.uniform(-3, 30, (n_bg, 3)))
    sem.append(np.full(n_bg, num_classes))
    inst.append(rng.integers(0, 40, n_bg))           # background labels collide: they must not count
    pts, sem, inst = np.concatenate(pts), np.concatenate(sem), np.concatenate(inst)
    perm = rng.permutation(n_points)
    pts, sem, inst = pts[perm], sem[perm], inst[perm]
    points = np.concatenate([pts, rng.uniform(0, 1, (n_points, extra_dims))], axis=1)
    box_t = torch.tensor(np.array(boxes).reshape(-1, 7), dtype=torch.float32)
    return dict(points=torch.tensor(points, dtype=torch.float32),
                sem=torch.tensor(sem, dtype=torch.long), inst=torch.tensor(inst, dtype=torch.long),
                boxes=box_t, with_yaw=with_yaw, num_classes=num_classes)


def exact_count_levels(counts):
    """level_fn: instance r gets exactly counts[r][0] points on the bottom face, of which
    counts[r][1] on its x-low edge, exactly counts[r][2] on the top face (counts[r][3] on its
    x-low edge); the rest on interior z levels.  Needs ks[2] >= 2."""
    def fn(r, rng, m, ks):
        if r >= len(counts):
            return None
        nb, nbl, nt, ntl = counts[r]
        assert nb + nt <= m
        lev = np.stack([random_levels(rng, m, ks[a], p_edge=0.0) for a in range(3)], axis=1)
        lev[:nb, 2] = 0
        lev[nb:nb + nt, 2] = ks[2]
        lev[:nbl, 0] = 0
        lev[nb:nb + ntl, 0] = 0
        return lev
    return fn
