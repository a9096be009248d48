"""CenterPoint's head (mmdet3d/models/dense_heads/centerpoint_head.py) and its box coder
(mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py): the reference's constructor arguments,
attribute names and state-dict keys, plain torch convolutions.

What differs from the reference is where the loops run:

  get_targets   the whole batch and every task at once on the device -- class -> task routing,
                the slot of every object and the max_objs cut are index arithmetic, the heat
                maps are one launch of the Gaussian painter; nothing is read back
                (the reference loops over samples, tasks and boxes in Python, :436-585)
  loss          clip_sigmoid + GaussianFocalLoss through the fused kernel, which also counts
                the positives (the reference reads them back with .item(), :606)
  get_bboxes    one batched NMS call over all tasks x samples on the device (the reference:
                per task and per sample, circle NMS on the host through numpy, rotated NMS
                through a mask copied to the host, :687-713 and :737-852)

This fork's behaviour is kept as written: train_cfg['pc_range'] (not point_cloud_range),
sin / cos of rot + pi, log of the dimensions under norm_bbox, ind = y * W + x, mask as uint8,
and an object whose integer centre is off the map is skipped but keeps its slot.
"""
import copy
import math

import torch
from torch import nn

from . import iou3d
from .head import ConvModule
from .head_loss import HeatmapPainter, build_loss, heatmap_boxes
from .registry import HEADS, build_conv_layer, build_head


def _box_tensor(boxes):
    return boxes.tensor if hasattr(boxes, "tensor") else boxes


def _conv_module(c_in, c_out, kernel_size, padding, bias, conv_cfg, norm_cfg):
    conv_cfg = conv_cfg or dict(type="Conv2d")
    if conv_cfg.get("type") not in ("Conv2d", "Conv", None):
        raise NotImplementedError("CenterHead: conv_cfg %r (Conv2d only)" % (conv_cfg,))
    norm = dict(norm_cfg or {})
    kind = norm.pop("type", None)
    norm.pop("requires_grad", None)
    kind = {"BN": "BN2d", "BN2d": "BN2d", None: None}[kind]
    return ConvModule(c_in, c_out, kernel_size, stride=1, padding=padding, bias=bias,
                      conv=nn.Conv2d, norm=kind, norm_kwargs=norm)


@HEADS.register_module()
class SeparateHead(nn.Module):
    """centerpoint_head.py:14-120: per head name a stack of ConvModules and a final conv."""

    def __init__(self, in_channels, heads, head_conv=64, final_kernel=1, init_bias=-2.19,
                 conv_cfg=dict(type="Conv2d"), norm_cfg=dict(type="BN2d"), bias="auto",
                 init_cfg=None, **kwargs):
        assert init_cfg is None, "To prevent abnormal initialization behavior, init_cfg is " \
            "not allowed to be set"
        super().__init__()
        self.heads = heads
        self.init_bias = init_bias
        for head in self.heads:
            classes, num_conv = self.heads[head]
            layers, c_in = [], in_channels
            for _ in range(num_conv - 1):
                layers.append(_conv_module(c_in, head_conv, final_kernel, final_kernel // 2, bias,
                                           conv_cfg, norm_cfg))
                c_in = head_conv
            layers.append(build_conv_layer(conv_cfg, head_conv, classes, kernel_size=final_kernel,
                                           stride=1, padding=final_kernel // 2, bias=True))
            self.__setattr__(head, nn.Sequential(*layers))
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        for head in self.heads:
            if head == "heatmap":
                self.__getattr__(head)[-1].bias.data.fill_(self.init_bias)

    def forward(self, x):
        return {head: self.__getattr__(head)(x) for head in self.heads}


@HEADS.register_module()
class DCNSeparateHead(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("DCNSeparateHead (deformable convolutions) is not built; "
                                  "use separate_head=dict(type='SeparateHead', ...)")


class CenterPointBBoxCoder:
    """centerpoint_bbox_coders.py.  decode() returns the reference's per-sample dicts;
    decode_padded() is the same arithmetic without the boolean indexing (fixed [B, K] shapes
    and a validity mask), which is what get_bboxes feeds to the batched NMS."""

    def __init__(self, pc_range, out_size_factor, voxel_size, post_center_range=None,
                 max_num=100, score_threshold=None, code_size=9):
        self.pc_range, self.out_size_factor, self.voxel_size = pc_range, out_size_factor, voxel_size
        self.post_center_range, self.max_num = post_center_range, max_num
        self.score_threshold, self.code_size = score_threshold, code_size

    def _gather_feat(self, feats, inds, feat_masks=None):
        dim = feats.size(2)
        inds = inds.unsqueeze(2).expand(inds.size(0), inds.size(1), dim)
        feats = feats.gather(1, inds)
        if feat_masks is not None:
            feats = feats[feat_masks.unsqueeze(2).expand_as(feats)].view(-1, dim)
        return feats

    def _topk(self, scores, K=80):
        batch, cat, height, width = scores.size()
        topk_scores, topk_inds = torch.topk(scores.view(batch, cat, -1), K)
        topk_inds = topk_inds % (height * width)
        topk_ys = (topk_inds.float() / torch.tensor(width, dtype=torch.float)).int().float()
        topk_xs = (topk_inds % width).int().float()
        topk_score, topk_ind = torch.topk(topk_scores.view(batch, -1), K)
        topk_clses = (topk_ind / torch.tensor(K, dtype=torch.float)).int()
        topk_inds = self._gather_feat(topk_inds.view(batch, -1, 1), topk_ind).view(batch, K)
        topk_ys = self._gather_feat(topk_ys.view(batch, -1, 1), topk_ind).view(batch, K)
        topk_xs = self._gather_feat(topk_xs.view(batch, -1, 1), topk_ind).view(batch, K)
        return topk_score, topk_inds, topk_clses, topk_ys, topk_xs

    def _transpose_and_gather_feat(self, feat, ind):
        feat = feat.permute(0, 2, 3, 1).contiguous()
        feat = feat.view(feat.size(0), -1, feat.size(3))
        return self._gather_feat(feat, ind)

    def encode(self):
        pass

    def decode_padded(self, heat, rot_sine, rot_cosine, hei, dim, vel, reg=None, task_id=-1):
        """-> boxes [B, K, code], scores [B, K], labels [B, K] (float, as the reference), mask
        [B, K] bool (score_threshold and post_center_range)."""
        batch, K = heat.size(0), self.max_num
        scores, inds, clses, ys, xs = self._topk(heat, K=K)
        if reg is not None:
            reg = self._transpose_and_gather_feat(reg, inds).view(batch, K, 2)
            xs = xs.view(batch, K, 1) + reg[:, :, 0:1]
            ys = ys.view(batch, K, 1) + reg[:, :, 1:2]
        else:
            xs = xs.view(batch, K, 1) + 0.5
            ys = ys.view(batch, K, 1) + 0.5
        rot_sine = self._transpose_and_gather_feat(rot_sine, inds).view(batch, K, 1)
        rot_cosine = self._transpose_and_gather_feat(rot_cosine, inds).view(batch, K, 1)
        rot = torch.atan2(rot_sine, rot_cosine)
        hei = self._transpose_and_gather_feat(hei, inds).view(batch, K, 1)
        dim = self._transpose_and_gather_feat(dim, inds).view(batch, K, 3)
        clses = clses.view(batch, K).float()
        scores = scores.view(batch, K)
        xs = xs.view(batch, K, 1) * self.out_size_factor * self.voxel_size[0] + self.pc_range[0]
        ys = ys.view(batch, K, 1) * self.out_size_factor * self.voxel_size[1] + self.pc_range[1]
        if vel is None:
            boxes = torch.cat([xs, ys, hei, dim, rot], dim=2)
        else:
            vel = self._transpose_and_gather_feat(vel, inds).view(batch, K, 2)
            boxes = torch.cat([xs, ys, hei, dim, rot, vel], dim=2)
        if self.post_center_range is None:
            raise NotImplementedError("Need to reorganize output as a batch, only support "
                                      "post_center_range is not None for now!")
        rng = torch.as_tensor(self.post_center_range, dtype=boxes.dtype, device=heat.device)
        mask = (boxes[..., :3] >= rng[:3]).all(2)
        mask &= (boxes[..., :3] <= rng[3:]).all(2)
        if self.score_threshold:
            mask &= scores > self.score_threshold
        return boxes, scores, clses, mask

    def decode(self, heat, rot_sine, rot_cosine, hei, dim, vel, reg=None, task_id=-1):
        boxes, scores, labels, mask = self.decode_padded(heat, rot_sine, rot_cosine, hei, dim, vel,
                                                         reg=reg, task_id=task_id)
        return [dict(bboxes=boxes[i, mask[i]], scores=scores[i, mask[i]],
                     labels=labels[i, mask[i]]) for i in range(heat.size(0))]


_BBOX_CODERS = {"CenterPointBBoxCoder": CenterPointBBoxCoder}


def build_bbox_coder(cfg):
    if not isinstance(cfg, dict):
        return cfg
    args = dict(cfg)
    return _BBOX_CODERS[args.pop("type")](**args)


@HEADS.register_module()
class CenterHead(nn.Module):
    """centerpoint_head.py:241-852."""

    def __init__(self, in_channels=[128], tasks=None, train_cfg=None, test_cfg=None,
                 bbox_coder=None, common_heads=dict(),
                 loss_cls=dict(type="GaussianFocalLoss", reduction="mean"),
                 loss_bbox=dict(type="L1Loss", reduction="none", loss_weight=0.25),
                 separate_head=dict(type="SeparateHead", init_bias=-2.19, final_kernel=3),
                 share_conv_channel=64, num_heatmap_convs=2, conv_cfg=dict(type="Conv2d"),
                 norm_cfg=dict(type="BN2d"), bias="auto", norm_bbox=True, init_cfg=None):
        assert init_cfg is None, "To prevent abnormal initialization behavior, init_cfg is " \
            "not allowed to be set"
        super().__init__()
        num_classes = [len(t["class_names"]) for t in tasks]
        self.class_names = [t["class_names"] for t in tasks]
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.in_channels, self.num_classes, self.norm_bbox = in_channels, num_classes, norm_bbox
        self.loss_cls, self.loss_bbox = build_loss(loss_cls), build_loss(loss_bbox)
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.num_anchor_per_locs = [n for n in num_classes]
        self.fp16_enabled = False
        self.shared_conv = _conv_module(in_channels, share_conv_channel, 3, 1, bias, conv_cfg,
                                        norm_cfg)
        self.task_heads = nn.ModuleList()
        separate_head = dict(separate_head)
        for num_cls in num_classes:
            heads = copy.deepcopy(common_heads)
            heads.update(dict(heatmap=(num_cls, num_heatmap_convs)))
            separate_head.update(in_channels=share_conv_channel, heads=heads, num_cls=num_cls)
            self.task_heads.append(build_head(separate_head))
        self.heatmap_painter = HeatmapPainter()
        self._const = {}

    def init_weights(self):
        pass

    def forward_single(self, x):
        x = self.shared_conv(x)
        return [task(x) for task in self.task_heads]

    def forward(self, feats):
        """feats: list of levels -> tuple (per task) of lists (per level) of dicts, as
        multi_apply(self.forward_single, feats) arranges them."""
        per_level = [self.forward_single(x) for x in feats]
        return tuple(list(level[t] for level in per_level) for t in range(len(self.task_heads)))

    def _gather_feat(self, feat, ind, mask=None):
        dim = feat.size(2)
        ind = ind.unsqueeze(2).expand(ind.size(0), ind.size(1), dim)
        feat = feat.gather(1, ind)
        if mask is not None:
            feat = feat[mask.unsqueeze(2).expand_as(feat)].view(-1, dim)
        return feat

    # ------------------------------------------------------------------ targets
    def _tables(self, device):
        """label -> (task, first slot group) tables, on the device, built once."""
        key = ("tables", device)
        if key not in self._const:
            task_of, cls_in_task = [], []
            for t, names in enumerate(self.class_names):
                task_of += [t] * len(names)
                cls_in_task += list(range(len(names)))
            first = [0]
            for n in self.num_classes:
                first.append(first[-1] + n)
            self._const[key] = tuple(torch.tensor(v, dtype=torch.long, device=device)
                                     for v in (task_of, cls_in_task, first[:-1]))
        return self._const[key]

    def _constant(self, key, make):
        """A small device tensor that depends on the configuration only: built once."""
        if key not in self._const:
            self._const[key] = make()
        return self._const[key]

    def get_targets(self, gt_bboxes_3d, gt_labels_3d):
        """:389-585 for the whole batch and every task at once, with no host read.
        -> (heatmaps, anno_boxes, inds, masks): per task [B, C_t, H, W] float32,
        [B, max_objs, 8 | 10] float32, [B, max_objs] int64, [B, max_objs] uint8."""
        cfg = self.train_cfg
        device = gt_labels_3d[0].device
        B, T = len(gt_labels_3d), len(self.task_heads)
        max_objs = cfg["max_objs"] * cfg["dense_reg"]
        code = len(cfg["code_weights"])
        osf = cfg["out_size_factor"]
        W, H = cfg["grid_size"][0] // osf, cfg["grid_size"][1] // osf
        total_cls = sum(self.num_classes)

        boxes, labels, sample = [], [], []
        for b, (bx, lb) in enumerate(zip(gt_bboxes_3d, gt_labels_3d)):
            if hasattr(bx, "gravity_center"):
                t = torch.cat((bx.gravity_center, bx.tensor[:, 3:]), dim=1)
            else:       # a plain tensor: bottom-centre LiDAR boxes (x, y, z, dx, dy, dz, yaw, ...)
                t = _box_tensor(bx)
                t = torch.cat((t[:, :2], t[:, 2:3] + t[:, 5:6] * 0.5, t[:, 3:]), dim=1)
            boxes.append(t.to(device).float())
            labels.append(lb.to(device).long())
            sample.append(torch.full((t.shape[0],), b, dtype=torch.long, device=device))
        boxes, labels, sample = torch.cat(boxes), torch.cat(labels), torch.cat(sample)
        n = boxes.shape[0]
        task_of, cls_in_task, _ = self._tables(device)
        known = (labels >= 0) & (labels < total_cls)       # torch.where(label == c) of :472
        safe = labels.clamp(0, total_cls - 1)
        task, cls = task_of[safe], cls_in_task[safe]

        # slot k: position in the task's class-major concatenation (:477-489) -- objects of one
        # (sample, task) ordered by (class, original index)
        group = sample * T + task
        group = torch.where(known, group, torch.full_like(group, B * T))
        key = (group * total_cls + safe) * max(n, 1) + torch.arange(n, device=device)
        order = torch.sort(key)[1]
        sorted_group = group[order]
        counts = torch.zeros(B * T + 2, dtype=torch.long, device=device)
        counts.index_add_(0, sorted_group + 1, torch.ones_like(sorted_group))
        start = torch.cumsum(counts, 0)[:-1]
        slot = torch.empty(n, dtype=torch.long, device=device)
        slot[order] = torch.arange(n, device=device) - start[sorted_group]

        hcfg = dict(cfg)
        hcfg["point_cloud_range"] = cfg["pc_range"]
        cx, cy, radius = heatmap_boxes(boxes[:, 0:2], boxes[:, 3:5], hcfg)
        vs = boxes.new_tensor(cfg["voxel_size"][:2])
        coor_x = (boxes[:, 0] - cfg["pc_range"][0]) / vs[0] / osf
        coor_y = (boxes[:, 1] - cfg["pc_range"][1]) / vs[1] / osf
        live = known & (slot < max_objs) & (radius >= 0)
        live &= (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)

        # heat maps: one buffer [B, total classes, H, W], one launch, split per task
        heat = boxes.new_zeros((B, total_cls, H, W))
        plane = torch.where(live, sample * total_cls + safe, torch.full_like(safe, -1))
        if n:
            self.heatmap_painter(heat, plane, cx, cy, radius)
        heatmaps = list(torch.split(heat, self.num_classes, dim=1))

        dims = boxes[:, 3:6].log() if self.norm_bbox else boxes[:, 3:6]
        rot = boxes[:, 6]
        cols = [coor_x - cx.float(), coor_y - cy.float(), boxes[:, 2], dims[:, 0], dims[:, 1],
                dims[:, 2], torch.sin(rot + math.pi), torch.cos(rot + math.pi)]
        if code == 10:
            cols += [boxes[:, 7], boxes[:, 8]]
        anno = torch.stack(cols, dim=1)

        # scatter into [B * T * max_objs (+ one dump row for the skipped)]
        dump = B * T * max_objs
        dest = torch.where(live, group * max_objs + slot, torch.full_like(slot, dump))
        anno_all = boxes.new_zeros((dump + 1, code))
        anno_all[dest] = anno
        ind_all = torch.zeros(dump + 1, dtype=torch.int64, device=device)
        ind_all[dest] = cy.long() * W + cx.long()
        mask_all = torch.zeros(dump + 1, dtype=torch.uint8, device=device)
        mask_all[dest] = 1
        anno_all = anno_all[:dump].view(B, T, max_objs, code)
        ind_all = ind_all[:dump].view(B, T, max_objs)
        mask_all = mask_all[:dump].view(B, T, max_objs)
        return (heatmaps, [anno_all[:, t] for t in range(T)], [ind_all[:, t] for t in range(T)],
                [mask_all[:, t] for t in range(T)])

    # ------------------------------------------------------------------ loss
    def loss(self, gt_bboxes_3d, gt_labels_3d, preds_dicts, **kwargs):
        """:588-641 -> dict(task{i}.loss_heatmap, task{i}.loss_bbox)."""
        heatmaps, anno_boxes, inds, masks = self.get_targets(gt_bboxes_3d, gt_labels_3d)
        loss_dict = dict()
        code_weights = self.train_cfg.get("code_weights", None)
        for task_id, preds_dict in enumerate(preds_dicts):
            pred = preds_dict[0]
            # clip_sigmoid + GaussianFocalLoss(avg_factor=max(num_pos, 1)), one fused pass
            loss_heatmap = self.loss_cls.from_logits(pred["heatmap"].float(),
                                                     heatmaps[task_id].contiguous())
            target_box = anno_boxes[task_id]
            parts = [pred["reg"], pred["height"], pred["dim"], pred["rot"]]
            if "vel" in pred:
                parts.append(pred["vel"])
            anno_box = torch.cat(parts, dim=1).float()
            ind = inds[task_id]
            num = masks[task_id].float().sum()
            box = anno_box.permute(0, 2, 3, 1).contiguous()
            box = self._gather_feat(box.view(box.size(0), -1, box.size(3)), ind)
            mask = masks[task_id].unsqueeze(2).expand_as(target_box).float()
            mask = mask * (~torch.isnan(target_box)).float()
            bbox_weights = mask * mask.new_tensor(code_weights)
            loss_bbox = self.loss_bbox(box, target_box, bbox_weights, avg_factor=(num + 1e-4))
            loss_dict[f"task{task_id}.loss_heatmap"] = loss_heatmap
            loss_dict[f"task{task_id}.loss_bbox"] = loss_bbox
        return loss_dict

    # ------------------------------------------------------------------ inference
    def _decode_task(self, task_id, pred):
        heat = pred["heatmap"].sigmoid()
        dim = torch.exp(pred["dim"]) if self.norm_bbox else pred["dim"]
        rots, rotc = pred["rot"][:, 0].unsqueeze(1), pred["rot"][:, 1].unsqueeze(1)
        return self.bbox_coder.decode_padded(heat, rots, rotc, pred["height"], dim,
                                             pred.get("vel"), reg=pred["reg"], task_id=task_id)

    def get_bboxes(self, preds_dicts, img_metas=None, img=None, rescale=False):
        """:643-735 and get_task_detections: decode per task, then ONE batched NMS over all
        tasks x samples, then label offsets and z -= h / 2.  -> per sample [bboxes [n, code]
        (bottom-centre; wrapped in img_metas[i]['box_type_3d'] when that is given), scores,
        labels (int32)], tasks in order, best score first inside a task."""
        cfg = self.test_cfg
        assert cfg["nms_type"] in ["circle", "rotate"]
        T = len(preds_dicts)
        boxes, scores, labels, valid = [], [], [], []
        for task_id, preds_dict in enumerate(preds_dicts):
            b, s, l, m = self._decode_task(task_id, preds_dict[0])
            if cfg["nms_type"] == "rotate":
                # get_task_detections: its own score threshold (>=) before NMS, the centre
                # range after it
                if cfg["score_threshold"] > 0.0:
                    m = m & (s >= cfg["score_threshold"])
            boxes.append(b)
            scores.append(s)
            labels.append(l)
            valid.append(m)
        boxes, scores = torch.stack(boxes), torch.stack(scores)            # [T, B, K, code]
        labels, valid = torch.stack(labels), torch.stack(valid)
        _, B, K, code = boxes.shape
        dev = boxes.device
        # compact the valid rows of every (task, sample) list to its front: stable sort by
        # validity keeps the decode order; the CSR offsets are the prefix of the counts
        flat_valid = valid.view(T * B, K)
        front = torch.sort((~flat_valid).to(torch.uint8), dim=1, stable=True)[1]
        counts = flat_valid.sum(1)
        rows = (torch.arange(T * B, device=dev)[:, None] * K + front).view(-1)
        # lists become contiguous when rows past a list's count sort to the very end
        live = (torch.arange(K, device=dev)[None, :] < counts[:, None]).view(-1)
        rows = rows[torch.sort((~live).to(torch.uint8), stable=True)[1]]
        offsets = torch.zeros(T * B + 1, dtype=torch.int32, device=dev)
        offsets[1:] = torch.cumsum(counts, 0)
        all_boxes = boxes.view(-1, code)[rows]
        all_scores = scores.view(-1)[rows]
        all_labels = labels.view(-1)[rows]
        if cfg["nms_type"] == "circle":
            thresh = self._constant(("min_radius", B, dev), lambda: torch.tensor(
                [float(r) for r in cfg["min_radius"][:T]], dtype=torch.float32,
                device=dev).repeat_interleave(B))
            keep, num = iou3d.nms_batched("circle", all_boxes[:, :2].contiguous(), all_scores,
                                          offsets, thresh, K, cfg["post_max_size"])
        else:
            bev = iou3d.xywhr2xyxyr(all_boxes[:, [0, 1, 3, 4, 6]])
            keep, num = iou3d.nms_batched("rotate", bev, all_scores, offsets, cfg["nms_thr"],
                                          min(cfg["pre_max_size"], K), cfg["post_max_size"])
        # gather [T * B, P] with padding, then per sample concatenate the tasks
        P = keep.shape[1]
        kept = keep >= 0
        safe = keep.clamp(min=0)
        out_boxes = all_boxes[safe.view(-1)].view(T, B, P, code).clone()
        out_scores = all_scores[safe.view(-1)].view(T, B, P)
        first = self._constant(("first_label", T, dev), lambda: torch.tensor(
            [sum(self.num_classes[:t]) for t in range(T)], device=dev))
        out_labels = (all_labels[safe.view(-1)].view(T, B, P) + first[:, None, None]).int()
        kept = kept.view(T, B, P)
        if cfg["nms_type"] == "rotate":
            limit = cfg["post_center_limit_range"]
            if limit is not None and len(limit) > 0:
                rng = torch.as_tensor(limit, dtype=out_boxes.dtype, device=dev)
                kept = kept & (out_boxes[..., :3] >= rng[:3]).all(-1) & \
                    (out_boxes[..., :3] <= rng[3:]).all(-1)
        out_boxes[..., 2] = out_boxes[..., 2] - out_boxes[..., 5] * 0.5
        ret_list = []
        for i in range(B):          # the variable-length lists the caller gets: one sync here
            m = kept[:, i].reshape(-1)
            bboxes = out_boxes[:, i].reshape(-1, code)[m]
            if img_metas is not None and "box_type_3d" in img_metas[i]:
                bboxes = img_metas[i]["box_type_3d"](bboxes, self.bbox_coder.code_size)
            ret_list.append([bboxes, out_scores[:, i].reshape(-1)[m],
                             out_labels[:, i].reshape(-1)[m]])
        return ret_list
