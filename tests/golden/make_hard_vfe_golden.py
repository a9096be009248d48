#!/usr/bin/env python
"""Generates tests/golden/hard_vfe_vectors.npz by RUNNING the reference's own Python code:

    HardVFE                  mmdet3d/models/voxel_encoders/voxel_encoder.py
    VFELayer                 mmdet3d/models/voxel_encoders/utils.py:34-106
    get_paddings_indicator   mmdet3d/models/voxel_encoders/utils.py:11-31

mmdet3d itself cannot be imported here (mmcv is not installed), so the definitions are pulled
out of the reference FILES at run time (ast) and compiled as they stand; the mmcv decorators
(force_fp32 / auto_fp16), build_norm_layer, the registry, DynamicScatter and `builder` are
local stand-ins.  Nothing of the reference is written to the repo: the .npz holds seeded
inputs, the layer weights, the outputs the reference code returned on CPU, the running
statistics it left, the outputs and parameter gradients of the same runs in float64
(module.double(), loss = sum(out * grad_out)) and the state-dict key names.  Build container
only (/root/reference).
"""
import ast
import json
import os
import sys

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/mmdet3d/models"
OUT = os.path.join(ROOT, "tests", "golden", "hard_vfe_vectors.npz")

VOXEL_SIZE = (0.25, 0.25, 8)
PC_RANGE = (-50, -50, -5, 50, 50, 3)
GRID = 400


def _passthrough(*a, **kw):          # force_fp32(out_fp16=True) / auto_fp16(apply_to=...)
    return lambda fn: fn


class _Registry:
    def register_module(self, *a, **kw):
        return lambda cls: cls


class _DynamicScatter:               # HardVFE constructs one and never calls it
    def __init__(self, *a, **kw):
        pass


class _Builder:
    @staticmethod
    def build_fusion_layer(cfg):
        raise NotImplementedError


def _build_norm_layer(cfg, num_features, postfix=""):
    cfg = dict(cfg)
    kind = cfg.pop("type")
    cfg.pop("requires_grad", None)
    cls = {"BN1d": nn.BatchNorm1d, "naiveSyncBN1d": nn.BatchNorm1d}[kind]   # one process
    return "bn" + str(postfix), cls(num_features, **cfg)


def reference_defs():
    ns = {"torch": torch, "nn": nn, "F": F, "build_norm_layer": _build_norm_layer,
          "force_fp32": _passthrough, "auto_fp16": _passthrough,
          "VOXEL_ENCODERS": _Registry(), "DynamicScatter": _DynamicScatter,
          "builder": _Builder}

    def pull(path, names):
        tree = ast.parse(open(os.path.join(REF, path)).read())
        body = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef))
                and n.name in names]
        assert len(body) == len(names), (path, names)
        exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)

    pull("voxel_encoders/utils.py", ("get_paddings_indicator", "VFELayer"))
    pull("voxel_encoders/voxel_encoder.py", ("HardVFE",))
    return ns


def make_voxels(rng, n, m, c):
    """Pillars as hard voxelization leaves them: points inside their pillar, slots past
    num_points zero; one-point voxels (padded slots win some maxima), full voxels and two
    voxels whose num_points exceeds M."""
    cells = rng.choice(GRID * GRID, n, replace=False)
    coors = np.stack([rng.randint(0, 2, n), np.zeros(n, np.int64), cells // GRID, cells % GRID], 1)
    feats = np.zeros((n, m, c), np.float32)
    feats[:, :, :2] = (rng.rand(n, m, 2) + coors[:, None, [3, 2]]) * VOXEL_SIZE[0] + PC_RANGE[0]
    feats[:, :, 2] = rng.uniform(-4.5, 2.5, (n, m))
    feats[:, :, 3:] = rng.rand(n, m, c - 3)
    num = rng.randint(1, m + 1, n)
    num[: max(2, n // 8)] = 1
    num[-max(2, n // 8):] = m
    feats *= (np.arange(m)[None, :] < num[:, None])[:, :, None]
    num[-2:] = m + 7
    return feats.astype(np.float32), num.astype(np.int32), coors.astype(np.int32)


def seed_module(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.endswith("norm.weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif name.endswith("norm.bias"):
                p.copy_(torch.rand(p.shape, generator=g) * 0.7 - 0.2)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
        for name, b in mod.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
            elif name.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) + 0.5)


def run_case(ns, out, names, tag, cfg, voxels, training, seed, weights_of=None):
    feats, num, coors = voxels
    args = (torch.from_numpy(num), torch.from_numpy(coors))
    mod = ns["HardVFE"](voxel_size=VOXEL_SIZE, point_cloud_range=PC_RANGE, **cfg)
    seed_module(mod, seed)
    mod.train(training)
    state = {k: v.clone() for k, v in mod.state_dict().items()}
    weights = weights_of or tag          # (train and eval share one seeded state)
    for k, v in state.items():
        if weights_of:
            assert np.array_equal(out[f"{weights}.w.{k}"], v.numpy()), (tag, k)
        else:
            out[f"{tag}.w.{k}"] = v.numpy().copy()
    with torch.no_grad():
        y = mod(torch.from_numpy(feats.copy()), *args)
    assert y.dim() == 2, (tag, y.shape)
    out[f"{tag}.out"] = y.numpy()
    for k, v in mod.state_dict().items():
        if "running" in k or "num_batches" in k:
            out[f"{tag}.after.{k}"] = v.numpy().copy()
    # the same run in float64, with the gradients of sum(out * grad_out)
    gout = torch.from_numpy(np.random.RandomState(seed).randn(*y.shape).astype(np.float32))
    out[f"{tag}.grad_out"] = gout.numpy()
    mod.load_state_dict(state)
    mod.double()
    y64 = mod(torch.from_numpy(feats.copy()).double(), *args)
    (y64 * gout.double()).sum().backward()
    out[f"{tag}.out64"] = y64.detach().numpy()
    for k, p in mod.named_parameters():
        out[f"{tag}.grad64.{k}"] = p.grad.numpy().copy()
    names[tag] = dict(cfg=cfg, training=training, keys=list(mod.state_dict().keys()),
                      weights=weights)


def main():
    ns = reference_defs()
    rng = np.random.RandomState(21)
    out, names = {}, {}
    voxels = make_voxels(rng, 97, 20, 4)
    out["features"], out["num_points"], out["coors"] = voxels
    common = dict(in_channels=4, with_cluster_center=True, with_voxel_center=True,
                  norm_cfg=dict(type="naiveSyncBN1d", eps=1e-3, momentum=0.01))
    for layers, widths in (("two", [64, 64]), ("one", [64])):
        for training in (True, False):
            tag = "%s_%s" % (layers, "train" if training else "eval")
            run_case(ns, out, names, tag, dict(common, feat_channels=widths), voxels, training,
                     300 + len(widths), weights_of=None if training else layers + "_train")
    out["meta"] = np.frombuffer(json.dumps(dict(
        cases=names, voxel_size=VOXEL_SIZE, point_cloud_range=PC_RANGE)).encode(), np.uint8)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    sys.exit(main())
