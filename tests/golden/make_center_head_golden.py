#!/usr/bin/env python
"""Generates tests/golden/center_head_vectors.npz by RUNNING the reference's own code:

    CenterHead.get_targets_single / get_targets / loss / get_bboxes (nms_type='circle')
        mmdet3d/models/dense_heads/centerpoint_head.py:389-735
    CenterPointBBoxCoder.decode      mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py
    circle_nms                       mmdet3d/core/post_processing/box3d_nms.py:141-181
    gaussian.py, clip_sigmoid, LiDARInstance3DBoxes   (as make_head_loss_golden.py takes them)

mmcv / mmdet / numba are absent: the definitions are taken from the reference FILES at run
time (ast) and executed as they stand; mmdet's losses and multi_apply are the written-out
definitions of make_head_loss_golden.py, and numba.jit becomes a pass-through.  The head is
the reference's class with its attributes set by hand (no convolutions are needed: targets,
loss and get_bboxes take predictions, which are seeded inputs here).

Cases: 2 samples, 3 tasks (1 / 2 / 2 classes), a 20 x 20 map, max_objs = 4 so that one task
overflows; boxes on the map border, beyond it, with zero width, a label in no task; norm_bbox
both ways with 9- and 7-column boxes (10- and 8-column anno_box).  Only inputs and outputs are
stored.
"""
import ast
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_head_loss_golden as ML  # noqa: E402

REF = ML.REF
HEAD = REF + "models/dense_heads/centerpoint_head.py"
CODER = REF + "core/bbox/coders/centerpoint_bbox_coders.py"
NMS = REF + "core/post_processing/box3d_nms.py"
OUT = os.path.join(ROOT, "tests", "golden", "center_head_vectors.npz")

TASKS = [["car"], ["truck", "construction_vehicle"], ["bus", "trailer"]]
PC_RANGE = [-8.0, -8.0]
MAP = 20


def train_cfg(code):
    return dict(grid_size=[80, 80, 1], voxel_size=[0.2, 0.2, 8], out_size_factor=4, dense_reg=1,
                gaussian_overlap=0.1, max_objs=4, min_radius=2, pc_range=PC_RANGE,
                point_cloud_range=[100.0] * 6,          # must NOT be what the head reads
                code_weights=[1.0] * 8 + ([0.2, 0.2] if code == 10 else []))


TEST_CFG = dict(post_center_limit_range=[-9, -9, -10, 9, 9, 10], max_per_img=500,
                max_pool_nms=False, min_radius=[0.5, 1.5, 0.8], score_threshold=0.1,
                out_size_factor=4, voxel_size=[0.2, 0.2], pc_range=PC_RANGE, nms_type="circle",
                pre_max_size=30, post_max_size=12, nms_thr=0.2)
CODER_CFG = dict(post_center_range=[-9, -9, -10, 9, 9, 10], max_num=40, score_threshold=0.1,
                 out_size_factor=4, voxel_size=[0.2, 0.2], pc_range=PC_RANGE, code_size=9)


class _Numba:
    @staticmethod
    def jit(*a, **kw):
        return lambda f: f


def reference_namespace():
    ns = ML.reference_namespace()
    ns.update(numba=_Numba, BaseModule=torch.nn.Module, builder=None, build_loss=None,
              build_bbox_coder=None, nms_gpu=None)
    ML._exec(ML._defs(NMS, {"circle_nms"}), NMS, ns)
    ML._exec(ML._defs(CODER, {"CenterPointBBoxCoder"}), CODER, ns)
    ML._exec(ML._defs(HEAD, {"CenterHead"}), HEAD, ns)
    return ns


def build_head(ns, norm_bbox, code):
    head = ns["CenterHead"].__new__(ns["CenterHead"])
    torch.nn.Module.__init__(head)
    head.class_names = TASKS
    head.num_classes = [len(t) for t in TASKS]
    head.train_cfg, head.test_cfg = ML.ConfigDict(train_cfg(code)), ML.ConfigDict(TEST_CFG)
    head.norm_bbox = norm_bbox
    head.task_heads = [None] * len(TASKS)                  # enumerated only
    head.loss_cls = ML.GaussianFocalLoss(reduction="mean")
    head.loss_bbox = ML.L1Loss(reduction="mean", loss_weight=0.25)
    head.bbox_coder = ns["CenterPointBBoxCoder"](**dict(CODER_CFG, code_size=code - 1))
    return head


def ground_truth(cols, seed=0):
    rng = np.random.default_rng(seed)
    out_b, out_l = [], []
    for b, n in enumerate((12, 7)):
        box = np.zeros((n, cols), np.float32)
        box[:, :2] = rng.uniform(-7.5, 7.5, (n, 2))
        box[:, 2] = rng.uniform(-2, 0, n)
        box[:, 3:6] = rng.uniform(0.5, 4.0, (n, 3))
        box[:, 6] = rng.uniform(-math.pi, math.pi, n)
        if cols == 9:
            box[:, 7:9] = rng.normal(size=(n, 2))
        lab = rng.integers(0, 5, n)
        if b == 0:
            lab[:7] = [1, 2, 1, 2, 1, 2, 1]                  # 7 objects in task 1 (> max_objs)
            box[1, :2] = [-8.0, -8.0]                        # the map's first cell
            box[2, :2] = [7.99, 7.99]                        # its last cell
            box[3, :2] = [8.3, 0.0]                          # beyond the map: skipped, keeps its slot
            box[4, 3] = 0.0                                  # zero width: skipped
            lab[11] = -1                                     # in no task
        out_b.append(box)
        out_l.append(lab.astype(np.int64))
    return out_b, out_l


def predictions(seed=5, batch=2):
    g = torch.Generator().manual_seed(seed)
    shapes = dict(reg=2, height=1, dim=3, rot=2, vel=2)
    preds = []
    for names in TASKS:
        d = {k: torch.randn((batch, c, MAP, MAP), generator=g) for k, c in shapes.items()}
        d["reg"] = torch.rand((batch, 2, MAP, MAP), generator=g)
        d["dim"] = d["dim"] * 0.3 + 0.6
        d["heatmap"] = torch.randn((batch, len(names), MAP, MAP), generator=g) * 1.5 - 1.0
        preds.append(d)
    return preds


def main():
    ns = reference_namespace()
    out = {}
    for tag, norm_bbox, cols in (("a", True, 9), ("b", False, 7)):
        head = build_head(ns, norm_bbox, cols + 1)
        boxes, labels = ground_truth(cols)
        gts = [ns["LiDARInstance3DBoxes"](torch.from_numpy(b), box_dim=cols) for b in boxes]
        labs = [torch.from_numpy(v) for v in labels]
        with torch.no_grad():
            tg = head.get_targets(gts, labs)
        for b in range(2):
            out["%s_gt_boxes_%d" % (tag, b)], out["%s_gt_labels_%d" % (tag, b)] = boxes[b], labels[b]
        for name, per_task in zip(("heatmap", "anno", "ind", "mask"), tg):
            for t, v in enumerate(per_task):
                out["%s_tgt_%s_t%d" % (tag, name, t)] = v.numpy()

    # loss + gradients, decode, get_bboxes (circle): the 9-column, norm_bbox case
    head = build_head(ns, True, 10)
    boxes, labels = ground_truth(9)
    gts = [ns["LiDARInstance3DBoxes"](torch.from_numpy(b), box_dim=9) for b in boxes]
    labs = [torch.from_numpy(v) for v in labels]
    preds = predictions()
    for t, d in enumerate(preds):
        for k, v in d.items():
            out["pred_t%d_%s" % (t, k)] = v.numpy().copy()
    leaves = [{k: v.clone().requires_grad_() for k, v in d.items()} for d in preds]
    # loss() rebinds the dict's 'heatmap' to clip_sigmoid's in-place result: hand it aliases
    losses = head.loss(gts, labs, tuple([{k: v * 1.0 for k, v in d.items()}] for d in leaves))
    sum(losses.values()).backward()
    for k, v in losses.items():
        out["loss_" + k] = v.detach().numpy()
    for t, d in enumerate(leaves):
        for k, v in d.items():
            out["grad_t%d_%s" % (t, k)] = v.grad.numpy()

    with torch.no_grad():
        for t, d in enumerate(preds):
            dec = head.bbox_coder.decode(d["heatmap"].sigmoid(), d["rot"][:, 0:1], d["rot"][:, 1:2],
                                         d["height"], torch.exp(d["dim"]), d["vel"], reg=d["reg"],
                                         task_id=t)
            for i, r in enumerate(dec):
                for k, v in r.items():
                    out["decode_t%d_s%d_%s" % (t, i, k)] = v.numpy()
        metas = [dict(box_type_3d=ns["LiDARInstance3DBoxes"])] * 2
        rets = head.get_bboxes(tuple([{k: v.clone() for k, v in d.items()}] for d in preds), metas)
        for i, (b, s, l) in enumerate(rets):
            out["bboxes_s%d_bboxes" % i] = b.tensor.numpy()
            out["bboxes_s%d_scores" % i], out["bboxes_s%d_labels" % i] = s.numpy(), l.numpy()

    # circle_nms alone: distinct scores, clustered centres
    rng = np.random.default_rng(9)
    dets = np.concatenate([rng.uniform(-4, 4, (150, 2)), rng.permutation(150)[:, None] / 150.0],
                          1).astype(np.float32)
    out["circle_dets"] = dets
    for th in (0.01, 0.2, 0.7):
        out["circle_keep_%s" % th] = np.asarray(ns["circle_nms"](dets, th), np.int64)
    out["circle_keep_0.7_post5"] = np.asarray(ns["circle_nms"](dets, 0.7, post_max_size=5), np.int64)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays;",
          {k: float(v.detach()) for k, v in losses.items()},
          "kept", [int(r[1].numel()) for r in rets],
          "decoded", [out["decode_t%d_s0_scores" % t].shape[0] for t in range(3)])


if __name__ == "__main__":
    main()
