"""Inputs for the Part-A2 first-stage tests and golden vectors: the shared case builder, the
margin assertion and numpy restatements (tests/h3d_cases.py is the model).

A case is built so that its discrete outcomes (which box holds a voxel centre, whether an
enlarged box does) are well defined by construction: every centre lies at least MARGIN from
every face of every box and of every enlarged box of its sample, measured in the box frame in
float64 -- an offending centre is drawn again, and assert_margins fails on a case that still
violates it.  Everything is float32 data; the float64 restatement reads the same numbers.

  face_margin      the distance of each centre to the nearest face of any box (float64)
  enlarge          LiDARInstance3DBoxes.enlarged_box on float32 numpy rows
  targets_ref      PointwiseSemanticHead.get_targets_single restated: the discrete part on the
                   float32 predicate (tests/roiaware_ref.py), the part targets in `dtype`
  make_case        boxes, labels, centres and batch ids of a batch
  rpn_loop         PartA2RPNHead.get_bboxes_single / class_agnostic_nms restated per sample on
                   the numpy NMS of tests/iou3d_ref.py
"""
import math

import numpy as np
import torch

import iou3d_ref as IR
import roiaware_ref as RR

MARGIN = 1e-3
EXTRA_WIDTH = 0.2
YAWS = (0.0, math.pi / 2, -math.pi / 2, math.pi, 7.0, -7.0, 0.3, -1.1, 2.0)
F32 = np.float32


def enlarge(boxes, extra_width):
    """lidar_box3d.py:227-240 in float32, torch's arithmetic (in-place adds of a Python scalar)."""
    t = torch.from_numpy(np.asarray(boxes, F32).reshape(-1, 7)).clone()
    t[:, 3:6] += extra_width * 2
    t[:, 2] -= extra_width
    return t.numpy()


def face_margin(centres, boxes):
    """[M, 3], [T, 7] -> [M] float64: min over boxes and faces of the distance between the
    centre and the face's plane, in the box frame (the predicate's: z against the middle
    height, x / y turned by rz + pi / 2 against l / 2 and w / 2).  inf without boxes."""
    p = np.asarray(centres, np.float64).reshape(-1, 3)
    b = np.asarray(boxes, np.float64).reshape(-1, 7)
    if b.shape[0] == 0 or p.shape[0] == 0:
        return np.full((p.shape[0],), np.inf)
    cx, cy, zb, w, l, h, rz = (b[None, :, j] for j in range(7))
    rot = rz + math.pi / 2
    sx, sy = p[:, 0:1] - cx, p[:, 1:2] - cy
    lx = sx * np.cos(rot) - sy * np.sin(rot)
    ly = sx * np.sin(rot) + sy * np.cos(rot)
    dz = np.abs(np.abs(p[:, 2:3] - (zb + h / 2)) - h / 2)
    dx = np.abs(np.abs(lx) - l / 2)
    dy = np.abs(np.abs(ly) - w / 2)
    return np.minimum(np.minimum(dx, dy), dz).min(1)


def assert_margins(centres, ids, boxes_list, extra_width=EXTRA_WIDTH, margin=MARGIN):
    """Every finite centre of sample b is at least `margin` from every face of b's boxes and
    enlarged boxes (NaN boxes and centres are outside every predicate and are skipped)."""
    centres, ids = np.asarray(centres), np.asarray(ids)
    for b, boxes in enumerate(boxes_list):
        boxes = np.asarray(boxes, F32).reshape(-1, 7)
        boxes = boxes[np.isfinite(boxes).all(1)]
        mine = centres[(ids == b) & np.isfinite(centres).all(1)]
        for table in (boxes, enlarge(boxes, extra_width)):
            m = face_margin(mine, table)
            assert m.size == 0 or m.min() >= margin, (b, float(m.min()))


def targets_ref(centres, boxes, labels, num_classes, extra_width=EXTRA_WIDTH, dtype=np.float64):
    """One sample.  centres [n, 3] float32, boxes [G, 7] float32, labels [G] ->
    (seg int64 [n], part `dtype` [n, 3], box_idx int32 [n], in_enlarged bool [n])."""
    centres = np.asarray(centres, F32).reshape(-1, 3)
    boxes = np.asarray(boxes, F32).reshape(-1, 7)
    n, g = centres.shape[0], boxes.shape[0]
    if g == 0 or n == 0:
        return (np.full((n,), num_classes, np.int64), np.zeros((n, 3), dtype),
                np.full((n,), -1, np.int32), np.zeros((n,), bool))
    box_idx = RR.points_in_boxes_first(centres[None], boxes[None])[0]
    in_big = RR.points_in_boxes_first(centres[None], enlarge(boxes, extra_width)[None])[0] > -1
    padded = np.concatenate([[num_classes], np.asarray(labels, np.int64)])
    seg = padded[box_idx.astype(np.int64) + 1]
    seg[(box_idx > -1) ^ in_big] = -1
    part = np.zeros((n, 3), dtype)
    fg = box_idx > -1
    k = box_idx[fg].astype(np.int64)
    bx = boxes.astype(dtype)
    d = centres[fg].astype(dtype) - bx[k, :3]
    angle = -bx[k, 6]
    sn, cs = np.sin(angle).astype(dtype), np.cos(angle).astype(dtype)
    rx = d[:, 0] * cs + d[:, 1] * sn
    ry = d[:, 0] * (-sn) + d[:, 1] * cs
    rot = np.stack([rx, ry, d[:, 2]], 1).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        part[fg] = rot / bx[k, 3:6] + np.asarray([0.5, 0.5, 0], dtype)
    part = np.where(part < 0, dtype(0), part)                   # torch.clamp(min=0): NaN stays
    return seg, part, box_idx, in_big


def batch_targets_ref(centres, ids, boxes_list, labels_list, num_classes,
                      extra_width=EXTRA_WIDTH, dtype=np.float64):
    """The batch in INPUT ROW order; a row whose id is outside [0, B) gets seg -1, part 0."""
    centres, ids = np.asarray(centres, F32), np.asarray(ids)
    seg = np.full((centres.shape[0],), -1, np.int64)
    part = np.zeros((centres.shape[0], 3), dtype)
    for b, (boxes, labels) in enumerate(zip(boxes_list, labels_list)):
        rows = np.nonzero(ids == b)[0]
        s, p, _, _ = targets_ref(centres[rows], boxes, labels, num_classes, extra_width, dtype)
        seg[rows], part[rows] = s, p
    return seg, part


def make_boxes(rng, count, cell=0.0):
    """[count, 7] float32 LiDAR boxes (bottom centre), centres on a lattice 10 apart so that
    boxes of different slots never touch; yaws cycle through YAWS."""
    slots = rng.permutation(64)[:count] if count <= 64 else np.arange(count)
    grid = np.stack([slots % 8, (slots // 8) % 8, slots // 64], axis=1).astype(np.float64)
    centre = grid * np.asarray([10.0, 10.0, 6.0]) + rng.uniform(-1.0, 1.0, size=(count, 3)) + cell
    size = rng.uniform(1.5, 4.0, size=(count, 3))
    yaw = np.asarray([YAWS[i % len(YAWS)] for i in range(count)])
    return np.concatenate([centre, size, yaw[:, None]], axis=1).astype(F32)


def draw_centres(rng, n, boxes, extra_width=EXTRA_WIDTH, margin=MARGIN):
    """n float32 centres about `boxes`: a third well inside a box, a third in the shell between a
    box and its enlarged box, a third anywhere; offenders of the margin are drawn again."""
    boxes = np.asarray(boxes, F32).reshape(-1, 7)
    big = enlarge(boxes, extra_width)

    def draw(m):
        if boxes.shape[0] == 0:
            return rng.uniform(-5.0, 80.0, size=(m, 3)).astype(F32)
        k = rng.integers(0, boxes.shape[0], size=m)
        b = boxes[k].astype(np.float64)
        kind = rng.integers(0, 3, size=m)
        scale = np.where(kind[:, None] == 0, rng.uniform(-0.49, 0.49, size=(m, 3)),
                         rng.uniform(-0.75, 0.75, size=(m, 3)))
        shell = kind == 1                    # one coordinate just past a face
        axis = rng.integers(0, 3, size=m)
        sign = rng.choice([-1.0, 1.0], size=m)
        local = scale * b[:, [4, 3, 5]]      # (along l, along w, along h)
        past = 0.5 * b[np.arange(m), [[4, 3, 5][a] for a in axis]] + rng.uniform(
            0.01, extra_width - 0.01, size=m)
        local[shell, axis[shell]] = (sign * past)[shell]
        rot = b[:, 6] + math.pi / 2          # the predicate's frame, inverted
        x = local[:, 0] * np.cos(rot) + local[:, 1] * np.sin(rot)
        y = -local[:, 0] * np.sin(rot) + local[:, 1] * np.cos(rot)
        z = b[:, 2] + b[:, 5] / 2 + local[:, 2]
        return np.stack([b[:, 0] + x, b[:, 1] + y, z], 1).astype(F32)

    out = draw(n)
    for _ in range(64):
        bad = np.minimum(face_margin(out, boxes), face_margin(out, big)) < margin
        if not bad.any():
            break
        out[bad] = draw(int(bad.sum()))
    return out


def make_case(seed, counts, rows_per_sample, num_classes=3, order="sorted"):
    """-> dict(centres float32 [N, 3], ids int32 [N], boxes list of [G_b, 7], labels list of
    int64 [G_b]).  order: 'sorted' (non-decreasing ids) or 'shuffled'."""
    rng = np.random.default_rng(seed)
    boxes = [make_boxes(rng, c, cell=3.0 * b) for b, c in enumerate(counts)]
    labels = [rng.integers(0, num_classes, size=c).astype(np.int64) for c in counts]
    centres = [draw_centres(rng, r, bx) for r, bx in zip(rows_per_sample, boxes)]
    ids = np.concatenate([np.full((r,), b, np.int32) for b, r in enumerate(rows_per_sample)])
    centres = np.concatenate(centres).astype(F32).reshape(-1, 3)
    if order == "shuffled":
        perm = rng.permutation(ids.shape[0])
        centres, ids = centres[perm], ids[perm]
    assert_margins(centres, ids, boxes)
    return dict(centres=centres, ids=ids, boxes=boxes, labels=labels, num_classes=num_classes)


# ------------------------------------------------------------------------------------ RPN
# The RPN head of the golden vectors: the 8 x 6 KITTI-style map of make_anchor_head_golden.py
# (case kc: three sizes x two rotations, one assigner per size, assign_per_class), 32 channels.
RPN_FEAT, RPN_MAP, RPN_DIR_OFFSET = 32, (8, 6), 0.7854
RPN_SIZES = [[0.6, 0.8, 1.73], [0.6, 1.76, 1.73], [1.6, 3.9, 1.56]]
RPN_RANGES = [[0, -8.0, -0.6, 20.0, 8.0, -0.6], [0, -8.0, -0.6, 20.0, 8.0, -0.6],
              [0, -8.0, -1.78, 20.0, 8.0, -1.78]]
RPN_THR = [(0.5, 0.35), (0.5, 0.35), (0.6, 0.45)]
RPN_CFGS = dict(
    train=dict(nms_pre=100, nms_post=12, max_num=12, nms_thr=0.8, score_thr=0,
               use_rotate_nms=False),
    test=dict(nms_pre=100, nms_post=50, max_num=50, nms_thr=0.3, score_thr=0.9,
              use_rotate_nms=True),
    quirk=dict(nms_pre=1000, nms_post=40, max_num=40, nms_thr=0.5, score_thr=0.45,
               use_rotate_nms=True),
    none=dict(nms_pre=100, nms_post=50, max_num=50, nms_thr=0.3, score_thr=0.3,
              use_rotate_nms=True))


def rpn_head_cfg(test_cfg=None):
    """Constructor arguments of the PartA2RPNHead the golden vectors were recorded with."""
    assigner = [dict(type="MaxIoUAssigner", iou_calculator=dict(type="BboxOverlapsNearest3D"),
                     pos_iou_thr=p, neg_iou_thr=n, min_pos_iou=n, ignore_iof_thr=-1)
                for p, n in RPN_THR]
    return dict(
        num_classes=3, in_channels=RPN_FEAT, feat_channels=RPN_FEAT,
        train_cfg=dict(assigner=assigner, allowed_border=0, pos_weight=-1, debug=False),
        test_cfg=dict(RPN_CFGS["test"] if test_cfg is None else test_cfg),
        anchor_generator=dict(type="Anchor3DRangeGenerator", ranges=RPN_RANGES, sizes=RPN_SIZES,
                              rotations=[0, 1.57], reshape_out=False),
        assigner_per_size=True, assign_per_class=True, dir_offset=RPN_DIR_OFFSET,
        dir_limit_offset=0,
        loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
        loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=2.0),
        loss_dir=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.2))


def rpn_loop(head, cls_scores, bbox_preds, dir_cls_preds, cfg, nms=None):
    """parta2_rpn_head.py:126-311 per sample with the head's own generator, coder, limit_period
    and xywhr2xyxyr, and `nms(kind, boxes [n, 5], scores [n], thresh) -> kept indices`, default
    the numpy NMS of tests/iou3d_ref.py on a stable descending order.
    -> per sample dict(boxes_3d tensor, scores_3d, labels_3d, cls_preds)."""
    from msmdfusion_amd.anchor_head import limit_period, xywhr2xyxyr

    def numpy_nms(kind, boxes, scores, thresh):
        order = IR.stable_order(scores.detach().cpu().numpy())
        keep = IR.nms(kind, boxes.detach().cpu().numpy(), thresh, order)
        return torch.as_tensor(keep, dtype=torch.long, device=boxes.device)

    nms = nms or numpy_nms
    code, C = head.box_code_size, head.num_classes
    sizes = [c.shape[-2:] for c in cls_scores]
    anchors = [a.reshape(-1, code) for a in
               head.anchor_generator.grid_anchors(sizes, device=cls_scores[0].device)]
    nms_pre = cfg.get("nms_pre", -1)
    results = []
    for i in range(cls_scores[0].shape[0]):
        boxes, maxes, labels, dirs, carried = [], [], [], [], []
        for cls, reg, dr, anc in zip(cls_scores, bbox_preds, dir_cls_preds, anchors):
            dir_score = torch.max(dr[i].permute(1, 2, 0).reshape(-1, 2), dim=-1)[1]
            cls_score = cls[i].permute(1, 2, 0).reshape(-1, C)
            scores = cls_score.sigmoid()
            reg_i = reg[i].permute(1, 2, 0).reshape(-1, code)
            max_scores, pred_labels = scores.max(dim=1)
            if nms_pre > 0 and scores.shape[0] > nms_pre:
                max_scores, inds = max_scores.topk(nms_pre)
                anc, reg_i, cls_score = anc[inds], reg_i[inds], scores[inds]
                dir_score, pred_labels = dir_score[inds], pred_labels[inds]
            boxes.append(head.bbox_coder.decode(anc, reg_i))
            maxes.append(max_scores), carried.append(cls_score)
            labels.append(pred_labels), dirs.append(dir_score)
        boxes, maxes, carried = torch.cat(boxes), torch.cat(maxes), torch.cat(carried)
        labels, dirs = torch.cat(labels), torch.cat(dirs)
        for_nms = xywhr2xyxyr(boxes[:, [0, 1, 3, 4, 6]])
        passed = maxes > cfg.get("score_thr", 0)
        kind = "rotate" if cfg["use_rotate_nms"] else "normal"
        selected = nms(kind, for_nms[passed], maxes[passed], cfg["nms_thr"])
        if len(selected) == 0:
            results.append(dict(boxes_3d=boxes.new_zeros([0, code]), scores_3d=boxes.new_zeros([0]),
                                labels_3d=boxes.new_zeros([0]),
                                cls_preds=boxes.new_zeros([0, carried.shape[-1]])))
            continue
        b = boxes[passed][selected].clone()
        s, l = maxes[passed][selected], labels[passed][selected]
        c, d = carried[passed][selected], dirs[passed][selected]
        dir_rot = limit_period(b[..., 6] - head.dir_offset, head.dir_limit_offset, np.pi)
        b[..., 6] = dir_rot + head.dir_offset + np.pi * d.to(b.dtype)
        if b.shape[0] > cfg["nms_post"]:
            inds = s.sort(descending=True)[1][:cfg["nms_post"]]
            b, l, s, c = b[inds], l[inds], s[inds], c[inds]
        results.append(dict(boxes_3d=b, scores_3d=s, labels_3d=l, cls_preds=c))
    return results
