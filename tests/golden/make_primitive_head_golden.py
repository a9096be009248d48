#!/usr/bin/env python
"""Generates tests/golden/primitive_head_vectors.npz by RUNNING the reference's own code:

    PrimitiveHead (get_targets_single, get_targets, loss, compute_primitive_loss,
    primitive_decode_scores, get_primitive_center and the constructor, for its state-dict keys)
                                          mmdet3d/models/roi_heads/mask_heads/primitive_head.py
    MultiBackbone (constructor and the aggregation layers)
                                          mmdet3d/models/backbones/multi_backbone.py
    VoteModule, ChamferDistance, DepthInstance3DBoxes: as make_vote_head_golden.py takes them

mmcv / mmdet are absent: the definitions are taken from the reference FILES at run time and the
mmcv / mmdet pieces are the ones make_vote_head_golden.py writes out (imported from it).  The
set-abstraction layer of the head and the streams of the backbone are CUDA-only there; they are
stood in for by modules with the parameter names of their published definitions (PointSAModule:
mlps.0.layer{j}.{conv,bn}) resp. by empty modules, so the key lists cover everything else.

get_targets_single runs in float32 as it stands, and in float64 with the points and the box
corners raised to float64 (a box stand-in hands the float32 corners over as float64, since
DepthInstance3DBoxes casts to float32).  The inputs come from tests/primitive_cases.py; main()
ASSERTS that the reference's discrete outcomes are well defined on them (the restatement
tests/primitive_ref.py, which must agree with the reference exactly on the discrete outputs,
records every comparison): same decisions in both precisions, no distance within 1e-3 of
dist_thresh / line_thresh, no variance within a factor 2 of var_thresh, no radicand that changes
sign.  Only inputs, weights, key lists and outputs are stored.

    python tests/golden/make_primitive_head_golden.py
"""
import copy
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_vote_head_golden as G  # noqa: E402
import primitive_cases as PC  # noqa: E402
import primitive_ref as R  # noqa: E402

OUT = os.path.join(HERE, "primitive_head_vectors.npz")
MODES = ("z", "xy", "line")
NUM_DIMS = {"z": 2, "xy": 1, "line": 0}
CHANNELS, SEEDS = 16, 32


class _SAStandIn(nn.Module):
    """PointSAModule's parameters (point_sa_module.py): mlps.0.layer{j} = Conv2d without bias +
    BatchNorm2d, the first layer widened by 3 for use_xyz."""

    def __init__(self, mlp_channels, use_xyz=True, **kw):
        super().__init__()
        spec = list(mlp_channels)
        spec[0] += 3 if use_xyz else 0
        mlp = nn.Sequential()
        for j in range(len(spec) - 1):
            layer = nn.Module()
            layer.conv = nn.Conv2d(spec[j], spec[j + 1], 1, bias=False)
            layer.bn = nn.BatchNorm2d(spec[j + 1])
            mlp.add_module("layer%d" % j, layer)
        self.mlps = nn.ModuleList([mlp])


class _Boxes64:
    """What get_targets_single reads of a box set, with the float32 corners as float64."""

    def __init__(self, boxes):
        self.corners, self.with_yaw = boxes.corners.double(), boxes.with_yaw

    def to(self, device):
        return self


def namespace():
    ns = G.reference_namespace()
    ns.update(copy=copy, build_sa_module=lambda cfg: _SAStandIn(**{k: v for k, v in cfg.items()
                                                                  if k != "type"}),
              BACKBONES=G._Registry(), build_backbone=lambda cfg: nn.Module(),
              auto_fp16=lambda **kw: (lambda f: f), load_checkpoint=None)
    for path, names in (("models/roi_heads/mask_heads/primitive_head.py", {"PrimitiveHead"}),
                        ("models/backbones/multi_backbone.py", {"MultiBackbone"})):
        G._exec(G._defs(G.REF + path, names), G.REF + path, ns)
    return ns


def head_cfg(mode, train_cfg):
    side = 1.0 if mode == "line" else 0.5
    chamfer = dict(type="ChamferDistance", mode="l1", reduction="sum", loss_src_weight=side,
                   loss_dst_weight=side)
    return dict(
        num_dims=NUM_DIMS[mode], num_classes=18, primitive_mode=mode,
        vote_module_cfg=dict(in_channels=CHANNELS, vote_per_seed=1, gt_per_seed=1,
                             conv_channels=(CHANNELS, CHANNELS), conv_cfg=dict(type="Conv1d"),
                             norm_cfg=dict(type="BN1d"), norm_feats=True,
                             vote_loss=dict(type="ChamferDistance", mode="l1", reduction="none",
                                            loss_dst_weight=10.0)),
        vote_aggregation_cfg=dict(type="PointSAModule", num_point=SEEDS, radius=0.3,
                                  num_sample=16, mlp_channels=[CHANNELS, 16, 16, 16],
                                  use_xyz=True, normalize_xyz=True),
        feat_channels=(16, 16), conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d"),
        objectness_loss=dict(type="CrossEntropyLoss", class_weight=[0.4, 0.6], reduction="mean",
                             loss_weight=30.0),
        center_loss=dict(chamfer), semantic_reg_loss=dict(chamfer),
        semantic_cls_loss=dict(type="CrossEntropyLoss", reduction="sum",
                               loss_weight=2.0 if mode == "line" else 1.0),
        train_cfg=dict(train_cfg))


def cases():
    """name -> (samples, train_cfg, masks given).  All samples of a case have one length."""
    def corner(r, rng, m, ks):
        lev = np.stack([PC.random_levels(rng, m, ks[a]) for a in range(3)], axis=1)
        lev[:6] = 0                                  # on two faces and three lines
        return lev
    background = PC.make_sample(44, 300, [])
    background["boxes"] = PC.make_sample(45, 300, [40])["boxes"]
    empty = PC.make_sample(46, 300, [])
    out = {
        # label gap (2, 5, 8, 11: rank != label), an instance of 4 points (fails every count
        # test), corner points (overwrite order), eight yaws over the cases
        "yaw": ([PC.make_sample(41, 300, [120, 90, 4, 60], level_fn=corner),
                 PC.make_sample(42, 300, [100, 100, 50], yaws=PC.YAWS[3:])], PC.SMALL_CFG, True),
        "no_yaw": ([PC.make_sample(43, 300, [120, 90, 4, 60], with_yaw=False, level_fn=corner),
                    background], PC.SMALL_CFG, True),
        # a bimodal bottom face: count passes, variance fails
        "bimodal": ([PC.make_sample(47, 300, [140, 120], bimodal=(0,))], PC.VAR_CFG, True),
        # masks None: derived from the boxes; the second sample has no ground truth
        "derived": ([PC.make_sample(48, 300, [120, 100]), empty], PC.SMALL_CFG, False),
        # the config's 100 / 10 straddled: exactly 100 (off) and 101 (on), 10 (off) and 11 (on)
        "config": ([PC.make_sample(49, 400, [330], yaws=(1.2,),
                                   level_fn=PC.exact_count_levels([(100, 10, 101, 11)]))],
                   PC.CONFIG_CFG, True),
    }
    out["no_yaw"][0][1]["with_yaw"] = False
    return out


def main():
    torch.manual_seed(0)
    ns = namespace()
    Head, Depth = ns["PrimitiveHead"], ns["DepthInstance3DBoxes"]
    store = {}

    def put(key, value):
        store[key] = value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)

    # ---- state-dict keys, from the reference constructors
    for mode in MODES:
        head = Head(**head_cfg(mode, PC.SMALL_CFG))
        put("keys/head_" + mode, sorted(head.state_dict()))
    ref_cfg = dict(fp_channels=((8, 8), (8, 8)))
    multi = ns["MultiBackbone"](num_streams=4, backbones=ref_cfg,
                                suffixes=("net0", "net1", "net2", "net3"))
    put("keys/multi_default", sorted(multi.state_dict()))
    multi2 = ns["MultiBackbone"](num_streams=2, backbones=[dict(ref_cfg), dict(ref_cfg)],
                                 aggregation_mlp_channels=[24, 12])
    put("keys/multi_given", sorted(multi2.state_dict()))
    put("multi/channels_default", [m.conv.weight.shape[:2] for m in multi.aggregation_layers])
    put("multi/channels_given", [m.conv.weight.shape[:2] for m in multi2.aggregation_layers])
    hd_in = torch.randn(2, 32, 20)
    multi.train()
    for name, p in multi.state_dict().items():
        put("multi/state/" + name, p)
    put("multi/in", hd_in)
    put("multi/out", multi.aggregation_layers(hd_in.clone()))

    # ---- targets
    for name, (samples, cfg, masks) in cases().items():
        with_yaw = samples[0]["with_yaw"]
        points = torch.stack([s["points"] for s in samples])
        boxes = [Depth(s["boxes"], with_yaw=with_yaw) if len(s["boxes"]) else
                 Depth(torch.zeros((0, 7)), with_yaw=with_yaw) for s in samples]
        labels = [torch.arange(len(s["boxes"])) * 2 + 1 for s in samples]
        put("%s/points" % name, points)
        put("%s/with_yaw" % name, int(with_yaw))
        put("%s/masks" % name, int(masks))
        put("%s/cfg" % name, [cfg[k] for k in ("dist_thresh", "var_thresh", "lower_thresh",
                                               "num_point", "num_point_line", "line_thresh")])
        g = torch.Generator().manual_seed(7)
        seed_indices = torch.stack([torch.randperm(points.shape[1], generator=g)[:SEEDS]
                                    for _ in samples])
        seed_points = torch.gather(points[..., :3], 1, seed_indices[..., None].expand(-1, -1, 3))
        put("%s/seed_indices" % name, seed_indices)
        for b, s in enumerate(samples):
            put("%s/%d/boxes" % (name, b), s["boxes"])
            put("%s/%d/labels" % (name, b), labels[b])
            put("%s/%d/sem" % (name, b), s["sem"])
            put("%s/%d/inst" % (name, b), s["inst"])
        for mode in MODES:
            head = Head.__new__(Head)
            nn.Module.__init__(head)
            head.num_dims, head.num_classes, head.primitive_mode = NUM_DIMS[mode], 18, mode
            head.train_cfg = dict(cfg)
            for b, s in enumerate(samples):
                fake = Depth(torch.zeros((1, 7)), with_yaw=with_yaw)
                box = boxes[b] if len(labels[b]) else fake
                lab = labels[b] if len(labels[b]) else labels[b].new_zeros(1)
                if masks:
                    sem, inst = s["sem"], s["inst"]
                else:                                    # what :358-369 derive, kept for f64
                    hit = box.points_in_boxes(s["points"][:, :3])
                    inst = hit.argmax(1)
                    sem = lab[inst]
                    sem[hit.max(1)[0] == 0], inst[hit.max(1)[0] == 0] = 18, lab.shape[0]
                    put("%s/%d/derived_sem" % (name, b), sem)
                    put("%s/%d/derived_inst" % (name, b), inst)
                got32 = head.get_targets_single(s["points"][:, :3].clone(), box, lab,
                                                None if not masks else sem.clone(),
                                                None if not masks else inst.clone())
                got64 = head.get_targets_single(s["points"][:, :3].double(), _Boxes64(box), lab,
                                                sem.clone(), inst.clone())
                # the restatement records the comparisons: it must reproduce the reference's
                # discrete outputs exactly, then its traces carry the margin assertions
                t32, t64 = R.Trace(), R.Trace()
                args = (s["points"], sem, inst, box.corners, with_yaw, mode, 18, cfg)
                r32 = R.primitive_targets_ref(*args, torch.float32, None, t32)
                R.primitive_targets_ref(*args, torch.float64, None, t64)
                assert torch.equal(r32[0], got32[0]), (name, mode, b)
                assert torch.equal(r32[2][:, -1], got32[1][:, -1]), (name, mode, b)
                assert torch.equal(got32[0].double(), got64[0]), (name, mode, b)
                assert torch.equal(got32[1][:, -1].double(), got64[1][:, -1]), (name, mode, b)
                R.assert_margins(t32, t64, cfg)
                for tag, got in (("f32", got32), ("f64", got64)):
                    put("%s/%d/%s/%s/mask" % (name, b, mode, tag), got[0])
                    put("%s/%d/%s/%s/sem" % (name, b, mode, tag), got[1])
                    put("%s/%d/%s/%s/offset" % (name, b, mode, tag), got[2])
            preds = {"aggregated_points_" + mode: seed_points, "seed_points": seed_points,
                     "seed_indices": seed_indices}
            sems = [s["sem"].clone() for s in samples] if masks else None
            insts = [s["inst"].clone() for s in samples] if masks else None
            targets = head.get_targets([p[:, :3].clone() for p in points], list(boxes),
                                       list(labels), sems, insts, preds)
            for k, t in enumerate(targets):
                put("%s/targets/%s/%d" % (name, mode, k), t)

    # ---- what the cases were built for
    z = store["yaw/0/z/f32/mask"]
    inst = store["yaw/0/inst"]
    assert z[inst == 8].sum() == 0 and z[inst == 2].sum() > 0            # the 4-point instance
    assert store["bimodal/0/z/f32/mask"][store["bimodal/0/inst"] == 2].sum() < \
        store["bimodal/0/z/f32/mask"][store["bimodal/0/inst"] == 5].sum()
    assert store["config/0/z/f32/mask"].sum() == 101
    assert store["no_yaw/1/z/f32/mask"].sum() == 0 and store["derived/1/line/f32/mask"].sum() == 0
    assert store["derived/0/xy/f32/mask"].sum() > 0

    # ---- decode, primitive centre and loss on the "yaw" case
    samples, cfg, _ = cases()["yaw"]
    points = torch.stack([s["points"] for s in samples])
    seed_indices = torch.from_numpy(store["yaw/seed_indices"])
    seed_points = torch.gather(points[..., :3], 1, seed_indices[..., None].expand(-1, -1, 3))
    boxes = [Depth(s["boxes"]) for s in samples]
    labels = [torch.arange(len(s["boxes"])) * 2 + 1 for s in samples]
    for mode in MODES:
        head = Head(**head_cfg(mode, cfg))
        g = torch.Generator().manual_seed(11)
        predictions = torch.randn((2, 3 + NUM_DIMS[mode] + 18, SEEDS), generator=g)
        decoded = head.primitive_decode_scores(predictions, seed_points)
        put("decode/%s/predictions" % mode, predictions)
        for k, v in decoded.items():
            put("decode/%s/%s" % (mode, k), v)
        flag = torch.randn((2, 2, SEEDS), generator=g)
        centre, ind = head.get_primitive_center(flag, decoded["center_" + mode])
        put("decode/%s/flag" % mode, flag)
        put("decode/%s/pred_center" % mode, centre)
        put("decode/%s/pred_ind" % mode, ind)
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            leaves = {"pred_flag_" + mode: flag, "vote_" + mode: seed_points + 0.3 * torch.randn(
                          seed_points.shape, generator=torch.Generator().manual_seed(12)),
                      "center_" + mode: decoded["center_" + mode],
                      "sem_cls_scores_" + mode: decoded["sem_cls_scores_" + mode]}
            if mode != "line":
                leaves["size_residuals_" + mode] = decoded["size_residuals_" + mode]
            leaves = {k: v.detach().clone().to(dtype).requires_grad_() for k, v in leaves.items()}
            preds = dict(leaves, seed_points=seed_points.to(dtype), seed_indices=seed_indices)
            preds["aggregated_points_" + mode] = seed_points
            losses = head.loss(preds, [p[:, :3].clone() for p in points], list(boxes),
                               list(labels), [s["sem"].clone() for s in samples],
                               [s["inst"].clone() for s in samples])
            sum(losses.values()).backward()
            for k, v in losses.items():
                put("loss/%s/%s/%s" % (mode, tag, k), v)
            for k, v in leaves.items():
                put("loss/%s/%s/in/%s" % (mode, tag, k), v)
                put("loss/%s/%s/grad/%s" % (mode, tag, k), v.grad)
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(store), "arrays")


if __name__ == "__main__":
    main()
