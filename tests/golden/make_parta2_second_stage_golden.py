#!/usr/bin/env python
"""Generates tests/golden/parta2_second_stage_vectors.npz by RUNNING the reference's own code on
the CPU:

    PartAggregationROIHead._assign_and_sample   mmdet3d/models/roi_heads/part_aggregation_roi_head.py
    IoUNegPiecewiseSampler (sample, _sample_pos, _sample_neg)
                                                mmdet3d/core/bbox/samplers/iou_neg_piecewise_sampler.py
    PartA2BboxHead (get_targets, _get_target_single, loss, get_corner_loss_lidar, get_bboxes,
    multi_class_nms)                            mmdet3d/models/roi_heads/bbox_heads/parta2_bbox_head.py
    LiDARInstance3DBoxes, rotation_3d_in_axis, xywhr2xyxyr, DeltaXYZWLHRBBoxCoder

mmcv / mmdet are absent: the definitions are taken from the reference FILES at run time (ast, the
machinery of make_head_loss_golden.py / make_anchor_head_golden.py) and executed as they stand.
What they import from mmdet is written out from its published definitions: MaxIoUAssigner and
SmoothL1Loss as make_anchor_head_golden.py has them, CrossEntropyLoss as make_ssd3d_head_golden.py
has it, RandomSampler / BaseSampler's constructor and SamplingResult below.  BboxOverlaps3D is
served by the oracle (make_head_loss_golden.OracleOverlaps), the NMS ops by tests/iou3d_ref.py on
a stable descending order.  random_choice is the project's key rule -- "the n entries with the
smallest keys, ties to the lower proposal index" -- with the keys recorded: a uniform subset, as
the reference's randperm[:n] is.  The spconv layers are dense stand-ins: a SubM conv is a dense
conv3d evaluated at the active sites, BatchNorm runs over the active rows only, the max-pool
takes the active inputs of a window from 0 (they follow a ReLU); mmcv's ConvModule, xavier_init
and normal_init are written out.  Only stubs, inputs and recorded outputs are here.

Cases (3 classes with a per-class assigner list; `car`: one class, a single assigner):
  c3    two samples, 60 / 45 proposals, 7 / 5 boxes, one ground truth labelled -1
  car   two samples, 50 / 40 proposals, 6 / 4 boxes
For each: the assignment of every proposal, the sampled rows, get_targets in float32, the
bbox_targets of _get_target_single on float64 boxes, every loss term and the gradients of cls_score / bbox_pred in
float32 and float64, get_corner_loss_lidar, and get_bboxes with rotate and normal NMS.
`head`: the reference's own __init__ / init_weights / forward / loss at roi_feat_size 4 and 16-48
channels on 8 RoIs: the key list, the weights, forward outputs in eval mode and in train mode
with dropout_ratio 0 and every loss term in float32 and float64, and all parameter gradients of
the train-mode run (float64 values and the float32 run's error against them).
tests/parta2_roi_cases.make_case ASSERTS the IoU, tie and yaw margins; main() asserts that keys
and NMS scores are pairwise distinct and that no NMS pair IoU lies within 1e-4 of nms_thr.
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import iou3d_ref as IR  # noqa: E402
import make_anchor_head_golden as MA  # noqa: E402
import make_ssd3d_head_golden as MS  # noqa: E402
import parta2_roi_cases as RC  # noqa: E402

ML = MA.ML
REF = ML.REF
OUT = os.path.join(HERE, "parta2_second_stage_vectors.npz")
CASES = dict(c3=dict(seed=61, props=(60, 45), gts=(7, 5), classes=3, single=False),
             car=dict(seed=62, props=(50, 40), gts=(6, 4), classes=1, single=True))
SAMPLER = dict(num=24, pos_fraction=0.55, neg_piece_fractions=[0.8, 0.2],
               neg_iou_piece_thrs=[0.55, 0.1], neg_pos_ub=-1, add_gt_as_proposals=False,
               return_iou=True)
RCNN = dict(cls_pos_thr=0.75, cls_neg_thr=0.25)
TEST_CFGS = dict(rotate=dict(use_rotate_nms=True, nms_thr=0.1, score_thr=0.3),
                 normal=dict(use_rotate_nms=False, nms_thr=0.1, score_thr=[0.3, 0.4, 0.5]))


# ------------------------------------------------------------------ mmdet 2.x, written out
class SamplingResult:                            # core/bbox/samplers/sampling_result.py
    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.pos_bboxes, self.neg_bboxes = bboxes[pos_inds], bboxes[neg_inds]
        self.pos_is_gt = gt_flags[pos_inds]
        self.num_gts = gt_bboxes.shape[0]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        if gt_bboxes.numel() == 0:
            assert self.pos_assigned_gt_inds.numel() == 0
            self.pos_gt_bboxes = torch.empty_like(gt_bboxes).view(-1, 4)
        else:
            if len(gt_bboxes.shape) < 2:
                gt_bboxes = gt_bboxes.view(-1, 4)
            self.pos_gt_bboxes = gt_bboxes[self.pos_assigned_gt_inds, :]
        self.pos_gt_labels = None if assign_result.labels is None else \
            assign_result.labels[pos_inds]

    @property
    def bboxes(self):
        return torch.cat([self.pos_bboxes, self.neg_bboxes])


class _NegProxy:
    """The sampler's `neg_sampler`: random_choice inside _sample_neg draws among POSITIONS in
    neg_inds, so the keys of those positions are looked up before the reference's body runs."""

    def __init__(self, owner):
        self.owner = owner

    def _sample_neg(self, assign_result, num_expected, **kwargs):
        neg_inds = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).view(-1)
        self.owner.active_keys = self.owner.keys[neg_inds]
        try:
            return self.owner._sample_neg(assign_result, num_expected, **kwargs)
        finally:
            self.owner.active_keys = self.owner.keys


class RandomSampler:                             # base_sampler.py + random_sampler.py
    def __init__(self, num, pos_fraction, neg_pos_ub=-1, add_gt_as_proposals=True, **kwargs):
        self.num, self.pos_fraction, self.neg_pos_ub = num, pos_fraction, neg_pos_ub
        self.add_gt_as_proposals = add_gt_as_proposals
        self.pos_sampler, self.neg_sampler = self, _NegProxy(self)
        self.keys = self.active_keys = None

    def random_choice(self, gallery, num):
        """The key rule (see the module docstring)."""
        assert len(gallery) >= num
        order = torch.sort(self.active_keys[gallery], stable=True)[1]
        return gallery[order[:max(int(num), 0)]]


def _nms(kind):
    def run(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
        order = IR.stable_order(scores.detach().numpy())
        seen.append((kind, boxes.detach().numpy().copy(), scores.detach().numpy().copy(), thresh))
        return torch.as_tensor(IR.nms(kind, boxes.detach().numpy(), thresh, order), dtype=torch.long)
    return run


seen = []                                         # every NMS call, for main()'s margin assertion


def reference_namespace():
    ns = MA.reference_namespace()
    ns.update(torch=torch, nn=nn, F=F, np=np, multi_apply=ML.multi_apply,
              AssignResult=ML.AssignResult, SamplingResult=SamplingResult,
              RandomSampler=RandomSampler, BBOX_SAMPLERS=ML.MH._Registry(),
              nms_gpu=_nms("rotate"), nms_normal_gpu=_nms("normal"),
              make_sparse_convmodule=make_sparse_convmodule, ConvModule=ConvModule,
              xavier_init=xavier_init, normal_init=normal_init, build_loss=build_loss,
              spconv=types.SimpleNamespace(SparseSequential=SparseSequential,
                                           SparseMaxPool3d=SparseMaxPool3d,
                                           SparseConvTensor=DenseTensor))
    ns["build_bbox_coder"] = lambda cfg: ns[cfg["type"]]()
    path = REF + "core/bbox/samplers/iou_neg_piecewise_sampler.py"
    ML._exec(ML._defs(path, {"IoUNegPiecewiseSampler"}), path, ns)
    path = REF + "models/roi_heads/bbox_heads/parta2_bbox_head.py"
    ML._exec(ML._defs(path, {"PartA2BboxHead"}), path, ns)
    path = REF + "models/roi_heads/part_aggregation_roi_head.py"
    cls = next(n for n in ast.parse(open(path).read()).body
               if isinstance(n, ast.ClassDef) and n.name == "PartAggregationROIHead")
    ML._exec([n for n in cls.body if isinstance(n, ast.FunctionDef)
              and n.name == "_assign_and_sample"], path, ns)
    return ns


def _np(t):
    return t.detach().cpu().numpy()

# ------------------------------------------------------------------ spconv / mmcv stand-ins
class DenseTensor:
    """spconv.SparseConvTensor for the stand-ins: rows [N, C] at indices [N, 4] (b, x, y, z)."""

    def __init__(self, features, indices, spatial_shape, batch_size):
        self.features, self.indices = features, indices.long()
        self.spatial_shape, self.batch_size = list(spatial_shape), batch_size

    def dense(self):
        i = self.indices
        out = self.features.new_zeros((self.batch_size, *self.spatial_shape,
                                       self.features.shape[1]))
        out = out.index_put((i[:, 0], i[:, 1], i[:, 2], i[:, 3]), self.features)
        return out.permute(0, 4, 1, 2, 3).contiguous()

    def rows(self, dense, indices):
        return dense[indices[:, 0], :, indices[:, 1], indices[:, 2], indices[:, 3]]


class SubMConv3d(nn.Module):
    """A SubM conv is the dense conv3d evaluated at the active sites.  The weight has this
    project's layout (out, kd, kh, kw, in), so the recorded state dict loads as it is."""

    def __init__(self, in_channels, out_channels, kernel_size, padding):
        super().__init__()
        self.padding = padding
        self.weight = nn.Parameter(torch.randn(out_channels, *[kernel_size] * 3, in_channels)
                                   / np.sqrt(27.0 * in_channels))

    def forward(self, x):
        y = F.conv3d(x.dense(), self.weight.permute(0, 4, 1, 2, 3), padding=self.padding)
        return DenseTensor(x.rows(y, x.indices), x.indices, x.spatial_shape, x.batch_size)


class SparseMaxPool3d(nn.Module):
    """Max over the active inputs of a window, from 0 (the inputs follow a ReLU); an output site
    is active when its window holds an active input."""

    def __init__(self, kernel_size, stride):
        super().__init__()
        self.kernel_size, self.stride = kernel_size, stride

    def forward(self, x):
        ones = x.features.new_ones((x.features.shape[0], 1))
        mask = DenseTensor(ones, x.indices, x.spatial_shape, x.batch_size).dense()
        pooled = F.max_pool3d(x.dense(), self.kernel_size, self.stride)
        indices = F.max_pool3d(mask, self.kernel_size, self.stride)[:, 0].nonzero(as_tuple=False)
        return DenseTensor(x.rows(pooled, indices), indices, list(pooled.shape[2:]), x.batch_size)


class SparseSequential(nn.Module):
    """Sparse children take the tensor, any other module its rows (BatchNorm1d therefore runs
    over the active rows only)."""

    def __init__(self, *children):
        super().__init__()
        for k, child in enumerate(children):
            self.add_module(str(k), child)

    def forward(self, x):
        for child in self._modules.values():
            if isinstance(child, (SubMConv3d, SparseMaxPool3d, SparseSequential)):
                x = child(x)
            else:
                x = DenseTensor(child(x.features), x.indices, x.spatial_shape, x.batch_size)
        return x


def make_sparse_convmodule(in_channels, out_channels, kernel_size, indice_key, stride=1, padding=0,
                           conv_type="SubMConv3d", norm_cfg=None, order=("conv", "norm", "act")):
    assert conv_type == "SubMConv3d" and stride == 1 and norm_cfg["type"] == "BN1d"
    return SparseSequential(SubMConv3d(in_channels, out_channels, kernel_size, padding),
                            nn.BatchNorm1d(out_channels, eps=norm_cfg["eps"],
                                           momentum=norm_cfg["momentum"]),
                            nn.ReLU(inplace=True))


class ConvModule(nn.Module):                      # mmcv.cnn.ConvModule: conv / bn / activate
    def __init__(self, in_channels, out_channels, kernel_size, padding=0, conv_cfg=None,
                 norm_cfg=None, act_cfg=dict(type="ReLU"), inplace=True):
        super().__init__()
        assert conv_cfg["type"] == "Conv1d"
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size, padding=padding,
                              bias=norm_cfg is None)
        if norm_cfg is not None:
            self.bn = nn.BatchNorm1d(out_channels, eps=norm_cfg["eps"],
                                     momentum=norm_cfg["momentum"])
        self.with_norm, self.with_act = norm_cfg is not None, act_cfg is not None
        if self.with_act:
            self.activate = nn.ReLU(inplace=inplace)

    def forward(self, x):
        x = self.conv(x)
        if self.with_norm:
            x = self.bn(x)
        return self.activate(x) if self.with_act else x


def xavier_init(module, gain=1, bias=0, distribution="normal"):
    assert distribution == "uniform"
    nn.init.xavier_uniform_(module.weight, gain=gain)
    if module.bias is not None:
        nn.init.constant_(module.bias, bias)


def normal_init(module, mean=0, std=1, bias=0):
    nn.init.normal_(module.weight, mean, std)
    if module.bias is not None:
        nn.init.constant_(module.bias, bias)


def build_loss(cfg):
    kinds = {"SmoothL1Loss": MA.SmoothL1Loss, "CrossEntropyLoss": MS.CrossEntropyLoss}
    return kinds[cfg["type"]](**{k: v for k, v in cfg.items() if k != "type"})


HEAD_CFG = dict(num_classes=3, seg_in_channels=16, part_in_channels=4, seg_conv_channels=[16, 16],
                part_conv_channels=[16, 16], merge_conv_channels=[32],
                down_conv_channels=[16, 16], shared_fc_channels=[16, 48, 48],
                cls_channels=[32, 32], reg_channels=[32, 32], dropout_ratio=0.0, roi_feat_size=4,
                with_corner_loss=True,
                loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, reduction="sum",
                               loss_weight=1.0),
                loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, reduction="sum",
                              loss_weight=1.0))
HEAD_ROIS, HEAD_POS = 8, 3


def run_head(ns, out):
    """The reference's own __init__, init_weights, forward and loss on the stand-ins above, in
    float32 and float64, eval mode and train mode (dropout_ratio 0)."""
    torch.manual_seed(9)
    head = ns["PartA2BboxHead"](**HEAD_CFG)
    init = {k: v.clone() for k, v in head.state_dict().items()}
    assert float(init["conv_reg.3.conv.weight"].std()) < 0.002 and \
        float(init["conv_reg.3.conv.bias"].abs().sum()) == 0            # init_weights ran
    gen = torch.Generator().manual_seed(10)
    with torch.no_grad():                         # outputs of order one, non-trivial statistics
        for name, prm in head.named_parameters():
            if name in ("conv_cls.3.conv.weight", "conv_reg.3.conv.weight"):
                prm.copy_(torch.randn(prm.shape, generator=gen) * 0.2)
            elif prm.dim() == 1:
                prm.copy_(torch.rand(prm.shape, generator=gen) * 0.5
                          + (0.75 if name.endswith("weight") else -0.25))
        for name, buf in head.named_buffers():
            if name.endswith("running_mean"):
                buf.copy_(torch.randn(buf.shape, generator=gen) * 0.1)
            elif name.endswith("running_var"):
                buf.copy_(torch.rand(buf.shape, generator=gen) * 0.5 + 0.5)
    out["head_state_keys"] = np.asarray(list(head.state_dict().keys()))
    for k, v in head.state_dict().items():
        out["head_weight_" + k] = _np(v)
    seg, part = RC.pooled_features(21, HEAD_ROIS, HEAD_CFG["roi_feat_size"])
    assert (part >= 0).all()
    out["head_seg_feats"], out["head_part_feats"] = seg, part
    rng = np.random.RandomState(22)
    gt, _ = RC.make_gt(rng, HEAD_ROIS, 3)
    rois = np.concatenate([np.zeros((HEAD_ROIS, 1)), gt + rng.uniform(-0.2, 0.2, gt.shape)], 1)
    reg_mask = (np.arange(HEAD_ROIS) < HEAD_POS).astype(np.int64)
    targets = dict(rois=rois.astype(np.float32), labels=rng.uniform(0, 1, HEAD_ROIS).astype(np.float32),
                   bbox_targets=(rng.normal(size=(HEAD_POS, 7)) * 0.2).astype(np.float32),
                   pos_gt_bboxes=gt[:HEAD_POS], reg_mask=reg_mask,
                   label_weights=np.full(HEAD_ROIS, 1.0 / HEAD_ROIS, np.float32),
                   bbox_weights=(reg_mask / float(HEAD_POS)).astype(np.float32))
    for k, v in targets.items():
        out["head_target_" + k] = v
    state = {k: v.clone() for k, v in head.state_dict().items()}
    for dtype, sfx in ((torch.float32, ""), (torch.float64, "64")):
        for mode in ("eval", "train"):
            h = ns["PartA2BboxHead"](**HEAD_CFG)
            h.load_state_dict(state)
            h = h.to(dtype).train(mode == "train")
            cls_score, bbox_pred = h(torch.from_numpy(seg).to(dtype), torch.from_numpy(part).to(dtype))
            q = "head_%s%s_" % (mode, sfx)
            out[q + "cls_score"], out[q + "bbox_pred"] = _np(cls_score), _np(bbox_pred)
            tg = [torch.from_numpy(v).to(dtype) if v.dtype != np.int64 else torch.from_numpy(v)
                  for v in targets.values()]
            losses = h.loss(cls_score, bbox_pred, *tg)
            (losses["loss_cls"] + losses["loss_bbox"] + losses["loss_corner"].mean()).backward()
            out[q + "loss_cls"], out[q + "loss_bbox"] = _np(losses["loss_cls"]), _np(losses["loss_bbox"])
            out[q + "loss_corner_vector"] = _np(losses["loss_corner"])
            for k, prm in h.named_parameters():
                out[q + "grad_" + k] = _np(prm.grad)
        print("head", sfx or "32", {k: float(out["head_train%s_%s" % (sfx, k)])
                                    for k in ("loss_cls", "loss_bbox")})
    # the gradients of the train-mode run: the float64 values (stored rounded to float32, half
    # an ulp) and, per parameter, the float32 run's largest error against them -- the two numbers
    # the tests' criterion reads, at a third of the bytes
    for k in [k for k in out if k.startswith("head_eval") and "_grad_" in k]:
        del out[k]
    for k, _ in head.named_parameters():
        g32, g64 = out.pop("head_train_grad_" + k), out["head_train64_grad_" + k]
        assert np.abs(g64).max() > 0, k
        out["head_train_graderr_" + k] = np.abs(g32.astype(np.float64) - g64).max()
        out["head_train64_grad_" + k] = g64.astype(np.float32)




def build_bbox_head(ns, classes):
    head = ns["PartA2BboxHead"].__new__(ns["PartA2BboxHead"])
    nn.Module.__init__(head)
    head.num_classes, head.with_corner_loss = classes, True
    head.bbox_coder = ns["DeltaXYZWLHRBBoxCoder"]()
    head.loss_bbox = MA.SmoothL1Loss(beta=1.0 / 9.0, reduction="sum", loss_weight=1.0)
    head.loss_cls = MS.CrossEntropyLoss(use_sigmoid=True, reduction="sum", loss_weight=1.0)
    return head


def run_case(ns, tag, spec, out):
    LiDAR = ns["LiDARInstance3DBoxes"]
    case = RC.make_case(spec["seed"], spec["props"], spec["gts"], spec["classes"], spec["single"])
    if not spec["single"]:
        case["gt_labels"][0][1] = -1
    p = tag + "_"
    mk = lambda: MA.MaxIoUAssigner(pos_iou_thr=0.55, neg_iou_thr=0.55, min_pos_iou=0.55,   # noqa: E731
                                   ignore_iof_thr=-1, iou_calculator=ML.OracleOverlaps())
    sampler = ns["IoUNegPiecewiseSampler"](**SAMPLER)
    keys = [RC.make_keys(spec["seed"] * 10 + b, n) for b, n in enumerate(spec["props"])]
    assigns = []
    plain_sample = sampler.sample

    def sample(assign_result, bboxes, gt_bboxes, gt_labels=None, **kw):
        sampler.keys = sampler.active_keys = torch.from_numpy(keys[len(assigns)])
        assigns.append(assign_result)
        return plain_sample(assign_result, bboxes, gt_bboxes, gt_labels, **kw)

    sampler.sample = sample
    roi = types.SimpleNamespace(bbox_assigner=mk() if spec["single"] else
                                [mk() for _ in range(spec["classes"])], bbox_sampler=sampler)
    proposals = [dict(boxes_3d=LiDAR(torch.from_numpy(b)), labels_3d=torch.from_numpy(l))
                 for b, l in zip(case["props"], case["prop_labels"])]
    gts = [LiDAR(torch.from_numpy(g)) for g in case["gt"]]
    gt_labels = [torch.from_numpy(l) for l in case["gt_labels"]]
    results = ns["_assign_and_sample"](roi, proposals, gts, gt_labels)
    for b, (res, a) in enumerate(zip(results, assigns)):
        for name in ("props", "prop_labels", "gt", "gt_labels"):
            out[p + "%s_%d" % (name, b)] = case[name][b]
        out[p + "keys_%d" % b] = keys[b]
        out[p + "gt_inds_%d" % b], out[p + "max_overlaps_%d" % b] = _np(a.gt_inds), _np(a.max_overlaps)
        out[p + "labels_%d" % b] = _np(a.labels)
        out[p + "pos_inds_%d" % b], out[p + "neg_inds_%d" % b] = _np(res.pos_inds), _np(res.neg_inds)
        out[p + "iou_%d" % b] = _np(res.iou)
        assert len(np.unique(keys[b])) == len(keys[b])
        assert res.pos_inds.numel() >= 2 and res.neg_inds.numel() >= 2, (tag, b)
    head = build_bbox_head(ns, spec["classes"])
    cfg = ML.ConfigDict(RCNN)
    names = ("label", "bbox_targets", "pos_gt_bboxes", "reg_mask", "label_weights", "bbox_weights")
    targets = head.get_targets(results, cfg)
    for k, v in zip(names, targets):
        out[p + "targets_" + k] = _np(v)
    for b, res in enumerate(results):
        # float64 boxes with the float32 IoUs: the reference builds `label` as float32 by name
        # (:418) and refuses a float64 masked write into it; bbox_targets follow the boxes
        single = head._get_target_single(res.pos_bboxes.double(), res.pos_gt_bboxes.double(),
                                         res.iou, cfg)
        assert single[1].dtype == torch.float64
        out[p + "single64_bbox_targets_%d" % b] = _np(single[1])
    rois = torch.cat([torch.cat([torch.full((len(r.bboxes), 1), float(b)), r.bboxes], 1)
                      for b, r in enumerate(results)])
    rs = np.random.RandomState(spec["seed"])
    n = rois.shape[0]
    out[p + "rois"] = _np(rois)
    out[p + "cls_score"] = rs.normal(size=(n, 1)).astype(np.float32)
    out[p + "bbox_pred"] = (rs.normal(size=(n, 7)) * 0.1).astype(np.float32)
    for dtype, sfx in ((torch.float32, ""), (torch.float64, "64")):
        cls_score = torch.from_numpy(out[p + "cls_score"]).to(dtype).requires_grad_(True)
        bbox_pred = torch.from_numpy(out[p + "bbox_pred"]).to(dtype).requires_grad_(True)
        tg = [t.to(dtype) if t.is_floating_point() else t for t in targets]
        losses = head.loss(cls_score, bbox_pred, rois.to(dtype), *tg)
        out[p + "loss_cls" + sfx] = _np(losses["loss_cls"])
        out[p + "loss_bbox" + sfx] = _np(losses["loss_bbox"])
        out[p + "loss_corner_vector" + sfx] = _np(losses["loss_corner"])
        (losses["loss_cls"] + losses["loss_bbox"] + losses["loss_corner"].mean()).backward()
        out[p + "grad_cls_score" + sfx] = _np(cls_score.grad)
        out[p + "grad_bbox_pred" + sfx] = _np(bbox_pred.grad)
    # inference: the RoIs of the sampled rows as proposals
    sizes = [len(r.bboxes) for r in results]
    class_labels = [torch.from_numpy(rs.randint(0, spec["classes"], s)) for s in sizes]
    class_pred = [torch.from_numpy((rs.permutation(s * spec["classes"]).reshape(s, spec["classes"])
                                    / float(s * spec["classes"] + 1)).astype(np.float32))
                  for s in sizes]
    metas = [dict(box_type_3d=LiDAR)] * len(sizes)
    for b in range(len(sizes)):
        out[p + "class_labels_%d" % b], out[p + "class_pred_%d" % b] = _np(class_labels[b]), \
            _np(class_pred[b])
    for kind, test_cfg in TEST_CFGS.items():
        test_cfg = dict(test_cfg)
        if spec["classes"] == 1 and isinstance(test_cfg["score_thr"], list):
            test_cfg["score_thr"] = test_cfg["score_thr"][:1]
        del seen[:]
        got = head.get_bboxes(rois, torch.from_numpy(out[p + "cls_score"]),
                              torch.from_numpy(out[p + "bbox_pred"]), class_labels, class_pred,
                              metas, cfg=ML.ConfigDict(test_cfg))
        for nms_kind, boxes, scores, thresh in seen:
            assert len(np.unique(scores)) == len(scores)
            iou = IR.iou_normal(boxes[:, :4], boxes[:, :4]) if nms_kind == "normal" else \
                IR.iou_bev(boxes, boxes, np.float64)
            assert (np.abs(iou - thresh) > 1e-4).all(), (tag, kind)
        for b, (boxes, scores, labels) in enumerate(got):
            out[p + "%s_boxes_%d" % (kind, b)] = _np(boxes.tensor)
            out[p + "%s_scores_%d" % (kind, b)] = _np(scores)
            out[p + "%s_labels_%d" % (kind, b)] = _np(labels)
        print(tag, kind, "kept", [int(g[1].numel()) for g in got], "of", sizes)
    print(tag, "sampled", [(int(r.pos_inds.numel()), int(r.neg_inds.numel())) for r in results],
          {k: float(out[p + k]) for k in ("loss_cls", "loss_bbox")})


def main():
    ns = reference_namespace()
    out = {}
    for tag, spec in CASES.items():
        run_case(ns, tag, spec, out)
    run_head(ns, out)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
