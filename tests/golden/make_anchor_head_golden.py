#!/usr/bin/env python
"""Generates tests/golden/anchor_head_vectors.npz by RUNNING the reference's own code:

    Anchor3DHead.loss / loss_single / add_sin_difference / get_bboxes / get_bboxes_single
        mmdet3d/models/dense_heads/anchor3d_head.py:188-510
    AnchorTrainMixin.anchor_target_3d / _single / anchor_target_single_assigner,
    get_direction_target            mmdet3d/models/dense_heads/train_mixins.py
    Anchor3DRangeGenerator, AlignedAnchor3DRangeGenerator
        mmdet3d/core/anchor/anchor_3d_generator.py
    DeltaXYZWLHRBBoxCoder           mmdet3d/core/bbox/coders/delta_xyzwhlr_bbox_coder.py
    BboxOverlapsNearest3D, bbox_overlaps_nearest_3d
        mmdet3d/core/bbox/iou_calculators/iou3d_calculator.py
    box3d_multiclass_nms            mmdet3d/core/post_processing/box3d_nms.py:8-88
    LiDARInstance3DBoxes (.nearest_bev, .bev), limit_period, xywhr2xyxyr
        (as make_head_loss_golden.py takes them)

mmcv / mmdet are absent: the definitions are taken from the reference FILES at run time (ast)
and executed as they stand.  What they import from mmdet 2.x is written out below from its
published definitions -- MaxIoUAssigner (assign / assign_wrt_overlaps), bbox_overlaps,
PseudoSampler / SamplingResult (with pos_bboxes), SmoothL1Loss, CrossEntropyLoss (softmax
form), images_to_levels; FocalLoss's python branch, weight_reduce_loss, multi_apply and
AssignResult are make_head_loss_golden.py's.  nms_gpu / nms_normal_gpu (CUDA only in the
reference) are served by tests/iou3d_ref.py, the oracle of the iou3d tests, with a stable
descending sort.  The head is the reference's class with its attributes set by hand.

Cases (an 8 x 6 map, H != W; 3 sizes x 2 rotations; batch 2):
  k   KITTI style: three assigners, reshape_out=False; samples with 0 and 7 ground truths
  kc  the same with assign_per_class; samples with 7 and 1
  n   nuScenes style: one assigner, aligned generator, reshape_out=True, code size 9,
      custom_values=[0, 0], levels 8 x 6 and 4 x 3; samples with 1 and 7
The seven boxes are constructed, and the script ASSERTS what they are for (main()).  Only
inputs and outputs are stored.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import iou3d_ref as IR  # noqa: E402
import make_head_loss_golden as ML  # noqa: E402

REF = ML.REF
OUT = os.path.join(ROOT, "tests", "golden", "anchor_head_vectors.npz")
DIR_OFFSET = 0.7854
SIZES = [[0.6, 0.8, 1.73], [0.6, 1.76, 1.73], [1.6, 3.9, 1.56]]
K_RANGES = [[0, -8.0, -0.6, 20.0, 8.0, -0.6], [0, -8.0, -0.6, 20.0, 8.0, -0.6],
            [0, -8.0, -1.78, 20.0, 8.0, -1.78]]
N_SIZES = [[0.866, 2.5981, 1.0], [0.5774, 1.7321, 1.0], [1.0, 1.0, 1.0]]
K_THR = [(0.5, 0.35), (0.5, 0.35), (0.6, 0.45)]
N_THR = (0.6, 0.3)
TEST_CFG = dict(use_rotate_nms=True, nms_across_levels=False, nms_thr=0.2, score_thr=0.3,
                min_bbox_size=0, nms_pre=30, max_num=12)


# ------------------------------------------------------------------ mmdet 2.x, written out
def bbox_overlaps(bboxes1, bboxes2, mode="iou", is_aligned=False, eps=1e-6):
    assert mode in ["iou", "iof", "giou"]
    rows, cols = bboxes1.size(-2), bboxes2.size(-2)
    if rows * cols == 0:
        return bboxes1.new(bboxes1.shape[:-2] + ((rows,) if is_aligned else (rows, cols)))
    area1 = (bboxes1[..., 2] - bboxes1[..., 0]) * (bboxes1[..., 3] - bboxes1[..., 1])
    area2 = (bboxes2[..., 2] - bboxes2[..., 0]) * (bboxes2[..., 3] - bboxes2[..., 1])
    if is_aligned:
        lt = torch.max(bboxes1[..., :2], bboxes2[..., :2])
        rb = torch.min(bboxes1[..., 2:], bboxes2[..., 2:])
        wh = (rb - lt).clamp(min=0)
        overlap = wh[..., 0] * wh[..., 1]
        union = area1 + area2 - overlap if mode in ["iou", "giou"] else area1
    else:
        lt = torch.max(bboxes1[..., :, None, :2], bboxes2[..., None, :, :2])
        rb = torch.min(bboxes1[..., :, None, 2:], bboxes2[..., None, :, 2:])
        wh = (rb - lt).clamp(min=0)
        overlap = wh[..., 0] * wh[..., 1]
        union = area1[..., None] + area2[..., None, :] - overlap if mode in ["iou", "giou"] \
            else area1[..., None]
    eps = union.new_tensor([eps])
    union = torch.max(union, eps)
    return overlap / union


class MaxIoUAssigner:
    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=.0, gt_max_assign_all=True,
                 ignore_iof_thr=-1, ignore_wrt_candidates=True, match_low_quality=True,
                 gpu_assign_thr=-1, iou_calculator=None):
        self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou = pos_iou_thr, neg_iou_thr, min_pos_iou
        self.gt_max_assign_all, self.ignore_iof_thr = gt_max_assign_all, ignore_iof_thr
        self.match_low_quality, self.iou_calculator = match_low_quality, iou_calculator
        self.argmax_seen = []                      # (overlaps, argmax) of every call, for main()

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        overlaps = self.iou_calculator(gt_bboxes, bboxes)
        return self.assign_wrt_overlaps(overlaps, gt_labels)

    def assign_wrt_overlaps(self, overlaps, gt_labels=None):
        num_gts, num_bboxes = overlaps.size(0), overlaps.size(1)
        assigned_gt_inds = overlaps.new_full((num_bboxes,), -1, dtype=torch.long)
        if num_gts == 0 or num_bboxes == 0:
            max_overlaps = overlaps.new_zeros((num_bboxes,))
            if num_gts == 0:
                assigned_gt_inds[:] = 0
            assigned_labels = None if gt_labels is None else \
                overlaps.new_full((num_bboxes,), -1, dtype=torch.long)
            return ML.AssignResult(num_gts, assigned_gt_inds, max_overlaps, labels=assigned_labels)
        max_overlaps, argmax_overlaps = overlaps.max(dim=0)
        gt_max_overlaps, gt_argmax_overlaps = overlaps.max(dim=1)
        self.argmax_seen.append((overlaps, argmax_overlaps))
        if isinstance(self.neg_iou_thr, float):
            assigned_gt_inds[(max_overlaps >= 0) & (max_overlaps < self.neg_iou_thr)] = 0
        pos_inds = max_overlaps >= self.pos_iou_thr
        assigned_gt_inds[pos_inds] = argmax_overlaps[pos_inds] + 1
        if self.match_low_quality:
            for i in range(num_gts):
                if gt_max_overlaps[i] >= self.min_pos_iou:
                    if self.gt_max_assign_all:
                        max_iou_inds = overlaps[i, :] == gt_max_overlaps[i]
                        assigned_gt_inds[max_iou_inds] = i + 1
                    else:
                        assigned_gt_inds[gt_argmax_overlaps[i]] = i + 1
        if gt_labels is not None:
            assigned_labels = assigned_gt_inds.new_full((num_bboxes,), -1)
            pos_inds = torch.nonzero(assigned_gt_inds > 0, as_tuple=False).squeeze()
            if pos_inds.numel() > 0:
                assigned_labels[pos_inds] = gt_labels[assigned_gt_inds[pos_inds] - 1]
        else:
            assigned_labels = None
        return ML.AssignResult(num_gts, assigned_gt_inds, max_overlaps, labels=assigned_labels)


class SamplingResult:
    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.pos_bboxes, self.neg_bboxes = bboxes[pos_inds], bboxes[neg_inds]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        self.pos_gt_bboxes = gt_bboxes[self.pos_assigned_gt_inds, :]


class PseudoSampler:
    def sample(self, assign_result, bboxes, gt_bboxes, **kw):
        pos = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        return SamplingResult(pos, neg, bboxes, gt_bboxes, assign_result)


class SmoothL1Loss(torch.nn.Module):
    def __init__(self, beta=1.0, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.beta, self.reduction, self.loss_weight = beta, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        diff = torch.abs(pred - target)
        loss = torch.where(diff < self.beta, 0.5 * diff * diff / self.beta, diff - 0.5 * self.beta)
        return self.loss_weight * ML.weight_reduce_loss(loss, weight, self.reduction, avg_factor)


class CrossEntropyLoss(torch.nn.Module):
    def __init__(self, use_sigmoid=False, reduction="mean", loss_weight=1.0):
        super().__init__()
        assert not use_sigmoid
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, cls_score, label, weight=None, avg_factor=None):
        loss = F.cross_entropy(cls_score, label, reduction="none")
        if weight is not None:
            weight = weight.float()
        return self.loss_weight * ML.weight_reduce_loss(loss, weight, self.reduction, avg_factor)


def images_to_levels(target, num_levels):
    target = torch.stack(target, 0)
    level_targets, start = [], 0
    for n in num_levels:
        level_targets.append(target[:, start:start + n])
        start += n
    return level_targets


class _Mmcv:
    @staticmethod
    def is_list_of(seq, expected_type):
        return isinstance(seq, list) and all(isinstance(s, expected_type) for s in seq)


def _nms(kind):
    def run(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
        order = IR.stable_order(scores.detach().numpy())
        keep = IR.nms(kind, boxes.detach().numpy(), thresh, order)
        return torch.as_tensor(keep, dtype=torch.long)
    return run


def reference_namespace():
    ns = ML.reference_namespace()
    reg = ML.MH._Registry()
    ns.update(mmcv=_Mmcv, ANCHOR_GENERATORS=reg, IOU_CALCULATORS=reg, BBOX_CODERS=reg, HEADS=reg,
              BaseBBoxCoder=object, bbox_overlaps=bbox_overlaps, numba=None,
              images_to_levels=images_to_levels, multi_apply=ML.multi_apply,
              PseudoSampler=PseudoSampler, nms_gpu=_nms("rotate"), nms_normal_gpu=_nms("normal"),
              build_anchor_generator=None, build_assigner=None, build_bbox_coder=None,
              build_sampler=None, build_loss=None, bias_init_with_prob=None, normal_init=None)
    ns["get_box_type"] = lambda coordinate: (ns["LiDARInstance3DBoxes"], None)
    for path, names in (
            ("core/anchor/anchor_3d_generator.py", {"Anchor3DRangeGenerator",
                                                    "AlignedAnchor3DRangeGenerator"}),
            ("core/bbox/coders/delta_xyzwhlr_bbox_coder.py", {"DeltaXYZWLHRBBoxCoder"}),
            ("core/bbox/iou_calculators/iou3d_calculator.py", {"BboxOverlapsNearest3D",
                                                               "bbox_overlaps_nearest_3d"}),
            ("core/post_processing/box3d_nms.py", {"box3d_multiclass_nms"}),
            ("models/dense_heads/train_mixins.py", {"AnchorTrainMixin", "get_direction_target"}),
            ("models/dense_heads/anchor3d_head.py", {"Anchor3DHead"})):
        ML._exec(ML._defs(REF + path, names), REF + path, ns)
    return ns


def build_head(ns, kind, per_class=False):
    head = ns["Anchor3DHead"].__new__(ns["Anchor3DHead"])
    torch.nn.Module.__init__(head)
    calc = ns["BboxOverlapsNearest3D"]()
    mk = lambda p, n: MaxIoUAssigner(pos_iou_thr=p, neg_iou_thr=n, min_pos_iou=n,
                                     ignore_iof_thr=-1, iou_calculator=calc)
    if kind == "k":
        head.anchor_generator = ns["Anchor3DRangeGenerator"](
            ranges=K_RANGES, sizes=SIZES, rotations=[0, 1.57], reshape_out=False)
        head.bbox_coder = ns["DeltaXYZWLHRBBoxCoder"]()
        head.bbox_assigner = [mk(*t) for t in K_THR]
        head.train_cfg = ML.ConfigDict(dict(allowed_border=0, pos_weight=-1, debug=False))
    else:
        head.anchor_generator = ns["AlignedAnchor3DRangeGenerator"](
            ranges=[[0, -8.0, -1.8, 20.0, 8.0, -1.8]], scales=[1, 2], sizes=N_SIZES,
            custom_values=[0, 0], rotations=[0, 1.57], reshape_out=True)
        head.bbox_coder = ns["DeltaXYZWLHRBBoxCoder"](code_size=9)
        head.bbox_assigner = mk(*N_THR)
        head.train_cfg = ML.ConfigDict(dict(allowed_border=0, pos_weight=2.0, debug=False,
                                            code_weight=[1.0] * 7 + [0.2, 0.2]))
    head.num_classes, head.use_sigmoid_cls, head.sampling = 3, True, False
    head.box_code_size = head.bbox_coder.code_size
    head.num_anchors = head.anchor_generator.num_base_anchors
    head.cls_out_channels = head.num_anchors * head.num_classes
    head.assigner_per_size, head.assign_per_class = kind == "k", per_class
    head.diff_rad_by_sin, head.use_direction_classifier = True, True
    head.dir_offset, head.dir_limit_offset = DIR_OFFSET, 0
    head.test_cfg = ML.ConfigDict(TEST_CFG)
    head.bbox_sampler = PseudoSampler()
    head.loss_cls = ML.FocalLoss(use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0)
    head.loss_bbox = SmoothL1Loss(beta=1.0 / 9.0, loss_weight=2.0)
    head.loss_dir = CrossEntropyLoss(use_sigmoid=False, loss_weight=0.2)
    return head


def kitti_seven(anchors):
    """The constructed sample.  anchors: [1, 8, 6, 3, 2, 7]; car anchors are size index 2."""
    car = anchors[0, :, :, 2, 0]                        # [8, 6, 7], rotation 0
    y3, y4 = float(car[3, 0, 1]), float(car[4, 0, 1])
    assert y3 == -y4                                    # rows 3 and 4 mirror each other
    a_twin, a_take, a_left = car[1, 4].tolist(), car[5, 1].tolist(), car[2, 3].tolist()
    boxes = [
        [8.0, 0.0, -1.78, 1.6, 3.9, 1.56, 0.3],         # 0: midway between rows 3 and 4: a tie
        a_twin, a_twin,                                 # 1, 2: identical, exactly an anchor
        [2.0, -5.714, -0.6, 0.6, 0.8, 1.73, 0.2],       # 3: between the columns: overlaps nothing
        [a_take[0] + 0.1] + a_take[1:6] + [0.1],        # 4: IoU 0.88 with its anchor (rule 3)
        [a_take[0] - 0.4] + a_take[1:6] + [-0.2],       # 5: IoU 0.6 with the same one (rule 4)
        [a_left[0], a_left[1] + 1.0] + a_left[2:6] + [0.15]]   # 6: leaves row 3 between thresholds
    return np.asarray(boxes, np.float32), np.asarray([2, 2, 2, 0, 2, 2, 2], np.int64)


def nus_boxes(level0, n, seed):
    rs = np.random.RandomState(seed)
    flat = level0.numpy()
    pick = flat[rs.randint(0, flat.shape[0], n)].copy()
    box = pick.copy()
    box[:, :2] += rs.uniform(-0.4, 0.4, (n, 2))
    box[:, 3:6] *= rs.uniform(0.85, 1.2, (n, 3))
    box[:, 6] = rs.uniform(-3.0, 3.0, n)
    box[:, 7:9] = rs.normal(size=(n, 2))
    box[0, :7] = pick[0, :7]                            # exactly an anchor
    return box.astype(np.float32), rs.randint(0, 3, n).astype(np.int64)


def predictions(head, sizes, batch, seed):
    g = torch.Generator().manual_seed(seed)
    a, c = head.num_anchors, head.box_code_size
    return ([torch.randn((batch, a * 3, *s), generator=g) for s in sizes],
            [torch.randn((batch, a * c, *s), generator=g) * 0.3 for s in sizes],
            [torch.randn((batch, a * 2, *s), generator=g) for s in sizes])


def run_targets(ns, head, levels, boxes, labels, dtype=torch.float32):
    box = ns["LiDARInstance3DBoxes"]
    code = head.box_code_size
    lv = [a.to(dtype) for a in levels]
    gts = [box(torch.from_numpy(b).to(dtype).reshape(-1, code), box_dim=code) for b in boxes]
    labs = [torch.from_numpy(l) for l in labels]
    return head.anchor_target_3d([list(lv) for _ in boxes], gts, [None] * len(boxes),
                                 gt_labels_list=labs, num_classes=3, sampling=False)


NAMES = ("labels", "label_weights", "bbox_targets", "bbox_weights", "dir_targets", "dir_weights")


def main():
    ns = reference_namespace()
    box = ns["LiDARInstance3DBoxes"]
    out = {}
    # ---- generators, coder, overlaps
    hk, hn = build_head(ns, "k"), build_head(ns, "n")
    (ak,) = hk.anchor_generator.grid_anchors([(8, 6)], device="cpu")
    an = hn.anchor_generator.grid_anchors([(8, 6), (4, 3)], device="cpu")
    out["anchors_k"], out["anchors_n0"], out["anchors_n1"] = ak.numpy(), an[0].numpy(), an[1].numpy()
    seven, seven_l = kitti_seven(ak)
    one = np.asarray([[8.3, 1.0, -1.7, 1.7, 4.0, 1.5, -1.2]], np.float32)
    empty, empty_l = np.zeros((0, 7), np.float32), np.zeros((0,), np.int64)
    n7, n7_l = nus_boxes(an[0], 7, 3)
    n1, n1_l = nus_boxes(an[0], 1, 4)
    flat_k = ak.reshape(-1, 7)
    out["overlaps_k7"] = ns["bbox_overlaps_nearest_3d"](torch.from_numpy(seven), flat_k).numpy()
    out["overlaps_n7"] = ns["bbox_overlaps_nearest_3d"](torch.from_numpy(n7), an[1]).numpy()
    out["overlaps_aligned"] = ns["bbox_overlaps_nearest_3d"](
        torch.from_numpy(seven), flat_k[40:47], is_aligned=True).numpy()
    enc = ns["DeltaXYZWLHRBBoxCoder"].encode(an[0][:7], torch.from_numpy(n7))
    out["coder_encode"] = enc.numpy()
    out["coder_decode"] = ns["DeltaXYZWLHRBBoxCoder"].decode(an[0][7:14], enc * 0.5).numpy()

    cases = {"k": (hk, [ak], [(empty, empty_l), (seven, seven_l)]),
             "kc": (build_head(ns, "k", True), [ak], [(seven, seven_l), (one, np.asarray([2]))]),
             "n": (hn, an, [(n1, n1_l), (n7, n7_l)])}
    for tag, (head, levels, samples) in cases.items():
        boxes, labels = [s[0] for s in samples], [s[1].astype(np.int64) for s in samples]
        for b in range(2):
            out["%s_gt_boxes_%d" % (tag, b)], out["%s_gt_labels_%d" % (tag, b)] = boxes[b], labels[b]
        with torch.no_grad():
            tg = run_targets(ns, head, levels, boxes, labels)
            tg64 = run_targets(ns, head, levels, boxes, labels, torch.float64)
        for name, per_level, per_level64 in zip(NAMES, tg[:6], tg64[:6]):
            for lvl, v in enumerate(per_level):
                out["%s_tgt_%s_l%d" % (tag, name, lvl)] = v.numpy()
                if name == "labels":      # the float64 run made the same assignment
                    assert torch.equal(v, per_level64[lvl]), tag
                if name == "bbox_targets":
                    out["%s_tgt_bbox_targets64_l%d" % (tag, lvl)] = per_level64[lvl].numpy()
        out["%s_num_total_pos" % tag] = np.asarray(tg[6], np.int64)
        out["%s_num_total_neg" % tag] = np.asarray(tg[7], np.int64)
        # the assigner alone, per sample and per assigner (segment order), where it is called
        assigners = head.bbox_assigner if isinstance(head.bbox_assigner, list) else [head.bbox_assigner]
        for b in range(2):
            for i, assigner in enumerate(assigners):
                if isinstance(head.bbox_assigner, list):
                    cur = levels[0][..., i, :, :].reshape(-1, 7)
                    m = labels[b] == i if head.assign_per_class else np.ones(len(labels[b]), bool)
                else:
                    cur = torch.cat([a.reshape(-1, head.box_code_size) for a in levels])
                    m = np.ones(len(labels[b]), bool)
                if m.sum() == 0:
                    continue
                res = assigner.assign(cur, torch.from_numpy(boxes[b][m]), None,
                                      torch.from_numpy(labels[b][m]))
                out["%s_assign_gt_inds_s%d_a%d" % (tag, b, i)] = res.gt_inds.numpy()
                out["%s_assign_max_overlaps_s%d_a%d" % (tag, b, i)] = res.max_overlaps.numpy()
        # every positive's direction is at least 1e-3 away from a bin edge
        for lvl in range(len(tg[0])):
            pos = tg[3][lvl][..., 0] > 0
            flat = torch.cat([a.reshape(-1, head.box_code_size) for a in levels])
            start = sum(t.shape[1] for t in tg[0][:lvl])
            anc = flat[start:start + tg[0][lvl].shape[1]][None].expand(2, -1, -1)
            rot = (tg[2][lvl][..., 6] + anc[..., 6])[pos].double() - DIR_OFFSET
            assert pos.sum() == 0 or float((torch.sin(rot)).abs().min()) >= 1e-3, tag

    # ---- the situations the seven boxes are for (car assigner, all boxes visible: case k)
    gi = out["k_assign_gt_inds_s1_a2"].reshape(8, 6, 2)          # [H, W, rot]
    ov = ns["bbox_overlaps_nearest_3d"](torch.from_numpy(seven), ak[..., 2, :, :].reshape(-1, 7))
    ov = ov.reshape(7, 8, 6, 2)
    assert gi[3, 2, 0] == 1 and gi[4, 2, 0] == 1 and ov[0, 3, 2, 0] == ov[0, 4, 2, 0] == ov[0].max()
    assert ov[0].max() < 0.6                                     # ... by rule 4 (a tie, both)
    assert ov[1, 1, 4, 0] == 1.0 and ov[2, 1, 4, 0] == 1.0 and gi[1, 4, 0] == 3   # rule 4: higher
    assert int(ov[:, 1, 4, 0].argmax()) == 1                     # torch on the CPU: lowest index
    ties = [(o, a) for asg in hk.bbox_assigner for o, a in asg.argmax_seen]
    for o, a in ties:                                            # ... on every tie of every call
        first = (o == o.max(0)[0][None]).float().argmax(0)
        assert torch.equal(a, first)
    assert float(ov[3].max()) < 0.45 and not (gi == 4).any()     # low quality: no anchor
    assert out["k_assign_max_overlaps_s1_a2"].reshape(8, 6, 2)[5, 1, 0] >= 0.6
    assert int(ov[:, 5, 1, 0].argmax()) == 4 and gi[5, 1, 0] == 6   # rule 3 said 5, rule 4 took it
    assert gi[3, 3, 0] == -1 and 0.45 <= ov[:, 3, 3, 0].max() < 0.6  # left at -1
    assert (gi == -1).any() and (gi == 0).any()
    assert "kc_assign_gt_inds_s0_a1" not in out and (seven_l != 1).all()   # a class without boxes
    assert (out["kc_tgt_labels_l0"] == 2).any() and (out["k_tgt_labels_l0"][0] == 3).all()

    # ---- loss and gradients (cases k: the sample without ground truth; n: two levels)
    for tag, seed in (("k", 5), ("n", 6)):
        head, levels, samples = cases[tag]
        sizes = [(8, 6)] if tag == "k" else [(8, 6), (4, 3)]
        preds = predictions(head, sizes, 2, seed)
        for name, per_level in zip(("cls", "bbox", "dir"), preds):
            for lvl, v in enumerate(per_level):
                out["%s_pred_%s_l%d" % (tag, name, lvl)] = v.numpy().copy()
        leaves = [[v.clone().requires_grad_() for v in per_level] for per_level in preds]
        code = head.box_code_size
        gts = [box(torch.from_numpy(s[0]).reshape(-1, code), box_dim=code) for s in samples]
        labs = [torch.from_numpy(s[1].astype(np.int64)) for s in samples]
        losses = head.loss(*leaves, gts, labs, [None, None])
        sum(sum(v) for v in losses.values()).backward()
        for k, per_level in losses.items():
            out["%s_%s" % (tag, k)] = np.asarray([float(v.detach()) for v in per_level], np.float32)
        for name, per_level in zip(("cls", "bbox", "dir"), leaves):
            for lvl, v in enumerate(per_level):
                out["%s_grad_%s_l%d" % (tag, name, lvl)] = v.grad.numpy()
        metas = [dict(box_type_3d=box)] * 2
        with torch.no_grad():
            rets = head.get_bboxes(*[[v.clone() for v in per_level] for per_level in preds], metas)
        for i, (b, s, l) in enumerate(rets):
            out["%s_det_s%d_bboxes" % (tag, i)] = b.tensor.numpy()
            out["%s_det_s%d_scores" % (tag, i)], out["%s_det_s%d_labels" % (tag, i)] = \
                s.numpy(), l.numpy()
        print(tag, {k: [float(v.detach()) for v in per] for k, per in losses.items()},
              "kept", [int(r[1].numel()) for r in rets])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays; positives",
          {t: int(out["%s_num_total_pos" % t]) for t in cases})


if __name__ == "__main__":
    main()
