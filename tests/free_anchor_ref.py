"""Torch restatements of FreeAnchor3DHead's loss (mmdet3d/models/dense_heads/
free_anchor3d_head.py) in the reference's own shape -- the [G, A] matrices -- for the tests of
csrc/free_anchor.hip and msmdfusion_amd/free_anchor_head.py.  They run on whatever device and in
whatever dtype their inputs have; the whole-loss restatement is the FUNCTIONAL form (every
(ground truth, anchor) pair has its own sin-difference encoding) and serves float64 autograd."""
import numpy as np
import torch
import torch.nn.functional as F

from msmdfusion_amd import anchor_head as A


def topk_restatement(anchor_bev, gt_bev, k):
    """The matrix, a stable descending sort (equal IoUs keep anchor order, NaN first: the order
    torch.topk selects in), the first k, each row then ascending.  -> long [G, k]"""
    ov = A.bbox_overlaps(gt_bev, anchor_bev)
    order = torch.sort(ov, dim=1, descending=True, stable=True)[1][:, :k]
    return torch.sort(order, dim=1)[0]


def box_prob_restatement(pred_bev, gt_bev, gt_labels, counts, num_classes, bbox_thr):
    """free_anchor3d_head.py:115-161 per sample on the [g, A] matrix; a ground truth whose best
    IoU does not exceed the threshold contributes nothing.  pred_bev [B * A, 4]; counts: the
    samples' ground-truth counts (host).  -> [B * A, num_classes]"""
    B = len(counts)
    n = pred_bev.shape[0] // B
    t1 = torch.full((), bbox_thr, dtype=pred_bev.dtype, device=pred_bev.device)
    out = pred_bev.new_zeros((B, n, num_classes))
    start = 0
    for b, g in enumerate(counts):
        if g == 0:
            continue
        iou = A.bbox_overlaps(gt_bev[start:start + g], pred_bev[b * n:(b + 1) * n])
        t2 = iou.max(dim=1, keepdim=True).values
        prob = ((iou - t1) / (torch.max(t2, t1) - t1)).clamp(min=0, max=1)
        prob = torch.where((t2 > t1) & (iou > t1), prob, torch.zeros_like(prob))
        labels = gt_labels[start:start + g]
        for c in range(num_classes):
            rows = labels == c
            if bool(rows.any()):
                out[b, :, c] = prob[rows].max(dim=0).values
        start += g
    return out.reshape(B * n, num_classes)


def negative_restatement(logits, box_prob, gamma, alpha):
    """negative_bag_loss (:266-282), summed."""
    prob = (logits.sigmoid() * (1 - box_prob)).clamp(0, 1)
    loss = prob ** gamma * F.binary_cross_entropy(prob, torch.zeros_like(prob), reduction="none")
    return ((1 - alpha) * loss).sum()


def decode_bev_restatement(anchors, deltas):
    """decode, then nearest_bev, rows of deltas cycling through the anchors."""
    reps = deltas.shape[0] // anchors.shape[0]
    return A.nearest_bev(A.DeltaXYZWLHRBBoxCoder.decode(anchors.repeat(reps, 1), deltas))


def _flatten(maps, c):
    B = maps[0].shape[0]
    return torch.cat([m.permute(0, 2, 3, 1).reshape(B, -1, c) for m in maps], dim=1)


def loss_restatement(head, anchors, cls_scores, bbox_preds, dir_cls_preds, gt_boxes, gt_labels,
                     matched=None):
    """free_anchor3d_head.py:72-242, sample by sample, in the dtype of the predictions, with the
    functional sin-difference.  anchors [A, code]; matched: per sample long [g, k], taken as
    given (float64 must form the float32 bags), else the top-k restatement.
    -> (dict of the two losses, box_prob [B, A, C], list of matched)"""
    dtype = cls_scores[0].dtype
    anchors = anchors.to(dtype)
    code, C, k = head.box_code_size, head.num_classes, head.pre_anchor_topk
    cls = _flatten(cls_scores, C)
    box = _flatten(bbox_preds, code)
    dirs = _flatten(dir_cls_preds, 2)
    cls_prob = cls.sigmoid()
    beta, w_box, w_dir = head.loss_bbox.beta, head.loss_bbox.loss_weight, head.loss_dir.loss_weight
    code_weight = A._get(head.train_cfg, "code_weight", None)
    positive, box_prob, bags, num_pos = [], [], [], 0
    for b in range(cls.shape[0]):
        gt, lab = gt_boxes[b].to(dtype), gt_labels[b]
        g = gt.shape[0]
        with torch.no_grad():
            pred_bev = A.nearest_bev(A.DeltaXYZWLHRBBoxCoder.decode(anchors, box[b]))
            gt_bev = A.nearest_bev(gt) if g else gt.new_zeros((0, 4))
            box_prob.append(box_prob_restatement(pred_bev, gt_bev, lab, [g], C, head.bbox_thr))
        m = matched[b] if matched is not None else topk_restatement(
            A.nearest_bev(anchors), gt_bev, k)
        bags.append(m)
        num_pos += g
        if g == 0:
            continue
        m_cls = cls_prob[b][m].gather(2, lab.view(-1, 1, 1).repeat(1, k, 1)).squeeze(2)
        m_anchors = anchors[m]
        targets = A.DeltaXYZWLHRBBoxCoder.encode(m_anchors, gt.unsqueeze(1).expand_as(m_anchors))
        rot = targets[..., 6] + m_anchors[..., 6]
        offset_rot = A.limit_period(rot - head.dir_offset, 0, 2 * np.pi)
        dir_t = torch.floor(offset_rot / np.pi).long().clamp(0, 1)
        loss_dir = w_dir * F.cross_entropy(dirs[b][m].transpose(-2, -1), dir_t, reduction="none")
        preds = box[b][m]
        if head.diff_rad_by_sin:
            preds, targets = head.add_sin_difference(preds, targets)
        diff = (preds - targets).abs()
        l1 = torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)
        if code_weight:
            l1 = l1 * torch.tensor(code_weight, dtype=dtype, device=l1.device)
        m_box = torch.exp(-((w_box * l1).sum(-1) + loss_dir))
        prob = m_cls * m_box
        weight = 1 / torch.clamp(1 - prob, 1e-12, None)
        weight = weight / weight.sum(dim=1, keepdim=True)
        bag = (weight * prob).sum(dim=1).clamp(0, 1)
        positive.append(head.alpha * F.binary_cross_entropy(bag, torch.ones_like(bag),
                                                            reduction="none"))
    box_prob = torch.stack(box_prob)
    pos = torch.cat(positive).sum() / max(1, num_pos) if positive else cls.sum() * 0
    neg = negative_restatement(cls, box_prob, head.gamma, head.alpha) / max(1, num_pos * k)
    return dict(positive_bag_loss=pos, negative_bag_loss=neg), box_prob, bags


# ---------------------------------------------------------------- heads of the tests
K_RANGES = [[0, -8.0, -0.6, 20.0, 8.0, -0.6], [0, -8.0, -0.6, 20.0, 8.0, -0.6],
            [0, -8.0, -1.78, 20.0, 8.0, -1.78]]
K_SIZES = [[0.6, 0.8, 1.73], [0.6, 1.76, 1.73], [1.6, 3.9, 1.56]]
N_SIZES = [[0.866, 2.5981, 1.0], [0.5774, 1.7321, 1.0], [1.0, 1.0, 1.0]]


def head_cfg(kind, topk=6, bbox_thr=0.6, gamma=2.0, alpha=0.5, feat=16, num_classes=3):
    """The two head styles of tests/golden/make_free_anchor_golden.py: 'k' (KITTI: one 8 x 6
    level, code 7) and 'n' (nuScenes: aligned generator, levels 8 x 6 and 4 x 3, code 9 with
    code_weight).  -> (config dict, feature-map sizes)"""
    common = dict(type="FreeAnchor3DHead", num_classes=num_classes, in_channels=feat,
                  feat_channels=feat, use_direction_classifier=True, pre_anchor_topk=topk,
                  bbox_thr=bbox_thr, gamma=gamma, alpha=alpha, diff_rad_by_sin=True,
                  dir_offset=0.7854, dir_limit_offset=0,
                  loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25,
                                loss_weight=1.0),
                  loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=0.8),
                  loss_dir=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.2),
                  test_cfg=dict(use_rotate_nms=True, nms_across_levels=False, nms_thr=0.2,
                                score_thr=0.3, min_bbox_size=0, nms_pre=30, max_num=12))
    if kind == "k":
        return dict(common, anchor_generator=dict(
            type="Anchor3DRangeGenerator", ranges=K_RANGES, sizes=K_SIZES, rotations=[0, 1.57],
            reshape_out=True), bbox_coder=dict(type="DeltaXYZWLHRBBoxCoder"),
            train_cfg=dict(allowed_border=0, pos_weight=-1, debug=False)), [(8, 6)]
    return dict(common, anchor_generator=dict(
        type="AlignedAnchor3DRangeGenerator", ranges=[[0, -8.0, -1.8, 20.0, 8.0, -1.8]],
        scales=[1, 2], sizes=N_SIZES, custom_values=[0, 0], rotations=[0, 1.57],
        reshape_out=True), bbox_coder=dict(type="DeltaXYZWLHRBBoxCoder", code_size=9),
        train_cfg=dict(allowed_border=0, pos_weight=2.0, debug=False,
                       code_weight=[1.0] * 7 + [0.2, 0.2])), [(8, 6), (4, 3)]


def gold_inputs(gold, tag, levels, device, dtype=torch.float32):
    """(cls, bbox, dir prediction lists, gt boxes, gt labels) of golden case `tag`."""
    preds = [[torch.from_numpy(gold["%s_pred_%s_l%d" % (tag, name, lvl)]).to(device, dtype)
              for lvl in range(levels)] for name in ("cls", "bbox", "dir")]
    boxes = [torch.from_numpy(gold["%s_gt_boxes_%d" % (tag, b)]).to(device) for b in range(2)]
    labels = [torch.from_numpy(gold["%s_gt_labels_%d" % (tag, b)]).to(device) for b in range(2)]
    return preds, boxes, labels


def within_reference_error(ours, ref32, ref64, factor=4.0):
    """|ours - ref64| <= factor * max(|ref32 - ref64|, eps * scale) in the maximum norm: the margin
    is the reference's own float32 error, floored at float32 eps of the scale.
    -> (ok, error, margin)"""
    ours, ref32, ref64 = (np.asarray(v, np.float64) for v in (ours, ref32, ref64))
    scale = max(float(np.abs(ref64).max()) if ref64.size else 0.0, 1e-30)
    err = float(np.abs(ours - ref64).max()) if ref64.size else 0.0
    own = float(np.abs(ref32 - ref64).max()) if ref64.size else 0.0
    margin = factor * max(own, float(np.finfo(np.float32).eps) * scale)
    return err <= margin, err, margin
