#!/usr/bin/env python
"""Generates tests/golden/pillar_vectors.npz by RUNNING the reference's own Python code:

    PillarFeatureNet         mmdet3d/models/voxel_encoders/pillar_encoder.py:11-150
    PFNLayer                 mmdet3d/models/voxel_encoders/utils.py:153-227
    get_paddings_indicator   mmdet3d/models/voxel_encoders/utils.py:11-31
    PointPillarsScatter      mmdet3d/models/middle_encoders/pillar_scatter.py

mmdet3d itself cannot be imported here (mmcv is not installed), so the definitions are pulled
out of the reference FILES at run time (ast) and compiled as they stand; the mmcv decorators
(force_fp32 / auto_fp16), build_norm_layer and the registries are local stand-ins.  Nothing of
the reference is written to the repo: the .npz holds seeded inputs, the layer weights, the
outputs the reference code returned on CPU, the running statistics it left and the state-dict
key names.  Build container only (/root/reference).
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
OUT = os.path.join(ROOT, "tests", "golden", "pillar_vectors.npz")

VOXEL_SIZE = (0.2, 0.2, 8)
PC_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)
GRID = 512


def _passthrough(*a, **kw):          # force_fp32(out_fp16=True) / auto_fp16(apply_to=...)
    return lambda fn: fn


class _Registry:
    def register_module(self, *a, **kw):
        return lambda cls: cls


def _build_norm_layer(cfg, num_features, postfix=""):
    cfg = dict(cfg)
    kind = cfg.pop("type")
    cfg.pop("requires_grad", None)
    cls = {"BN1d": nn.BatchNorm1d, "BN": nn.BatchNorm2d}[kind]
    return "bn" + str(postfix), cls(num_features, **cfg)


def reference_defs():
    ns = {"torch": torch, "nn": nn, "F": F, "build_norm_layer": _build_norm_layer,
          "force_fp32": _passthrough, "auto_fp16": _passthrough,
          "VOXEL_ENCODERS": _Registry(), "MIDDLE_ENCODERS": _Registry()}

    def pull(path, names):
        tree = ast.parse(open(os.path.join(REF, path)).read())
        body = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef))
                and n.name in names]
        assert len(body) == len(names), (path, names)
        exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)

    pull("voxel_encoders/utils.py", ("get_paddings_indicator", "PFNLayer"))
    pull("voxel_encoders/pillar_encoder.py", ("PillarFeatureNet",))
    pull("middle_encoders/pillar_scatter.py", ("PointPillarsScatter",))
    return ns


def make_pillars(rng, n, m, c, exceed=False):
    """Pillars as hard voxelization leaves them: points inside their pillar, slots past
    num_points zero.  exceed: the reference unit test's draw (num_points in [1, 100), every
    slot filled)."""
    cells = rng.choice(GRID * GRID, n, replace=False)
    coors = np.stack([rng.randint(0, 2, n), np.zeros(n, np.int64), cells // GRID, cells % GRID], 1)
    feats = np.zeros((n, m, c), np.float32)
    lo = (rng.rand(n, m, 2) + coors[:, None, [3, 2]]) * VOXEL_SIZE[0] + PC_RANGE[0]
    feats[:, :, :2] = lo
    feats[:, :, 2] = rng.uniform(-4.5, 2.5, (n, m))
    feats[:, :, 3:] = rng.rand(n, m, c - 3)
    if exceed:
        num = rng.randint(1, 100, n)
    else:
        num = rng.randint(1, m + 1, n)
        num[: max(2, n // 8)] = 1            # one-point pillars: padded slots win some maxima
        num[-max(2, n // 8):] = m            # full pillars
        feats *= (np.arange(m)[None, :] < num[:, None])[:, :, None]
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


def run_case(ns, out, names, tag, cfg, pillars, training, seed, weights_of=None):
    feats, num, coors = pillars
    mod = ns["PillarFeatureNet"](voxel_size=VOXEL_SIZE, point_cloud_range=PC_RANGE, **cfg)
    seed_module(mod, seed)
    mod.train(training)
    weights = weights_of or tag          # (the eight base cases share one seeded state)
    for k, v in mod.state_dict().items():
        if weights_of:
            assert np.array_equal(out[f"{weights}.w.{k}"], v.numpy()), (tag, k)
        else:
            out[f"{tag}.w.{k}"] = v.numpy().copy()
    with torch.no_grad():
        # a copy: the reference's legacy path writes into its input
        y = mod(torch.from_numpy(feats.copy()), torch.from_numpy(num), torch.from_numpy(coors))
    assert y.dim() == 2, (tag, y.shape)
    out[f"{tag}.out"] = y.numpy()
    for k, v in mod.state_dict().items():
        if "running" in k or "num_batches" in k:
            out[f"{tag}.after.{k}"] = v.numpy().copy()
    names[tag] = dict(cfg=cfg, training=training, keys=list(mod.state_dict().keys()),
                      weights=weights)


def main():
    ns = reference_defs()
    rng = np.random.RandomState(20)
    out, names = {}, {}

    def put(tag, pillars):
        out[f"{tag}.features"], out[f"{tag}.num_points"], out[f"{tag}.coors"] = pillars

    base = make_pillars(rng, 97, 20, 5)
    put("base", base)
    first = None
    for legacy in (True, False):
        for training in (True, False):
            for mode in ("max", "avg"):
                tag = "base_%s_%s_%s" % ("legacy" if legacy else "new",
                                         "train" if training else "eval", mode)
                run_case(ns, out, names, tag, dict(in_channels=5, feat_channels=[64], mode=mode,
                                                   legacy=legacy), base, training, 100,
                         weights_of=first)
                first = first or tag
                names[tag]["input"] = "base"
    extras = [
        ("distance", make_pillars(rng, 31, 20, 5),
         dict(in_channels=5, feat_channels=[64], with_distance=True)),
        ("c4m32", make_pillars(rng, 29, 32, 4), dict(in_channels=4, feat_channels=[32])),
        ("exceed", make_pillars(rng, 23, 20, 5, exceed=True),
         dict(in_channels=5, feat_channels=[64], mode="avg")),
        ("two_layer", make_pillars(rng, 19, 20, 5), dict(in_channels=5, feat_channels=[32, 64])),
    ]
    for i, (tag, pillars, cfg) in enumerate(extras):
        put(tag, pillars)
        run_case(ns, out, names, tag, cfg, pillars, True, 200 + i)
        names[tag]["input"] = tag

    # PointPillarsScatter: B = 2 with sample 0 empty, 16 x 12 canvas; and the single-sample form
    ny, nx, c = 16, 12, 8
    sc = ns["PointPillarsScatter"](in_channels=c, output_shape=[ny, nx])
    cells = rng.choice(ny * nx, 60, replace=False)
    batch = np.ones(60, np.int64)
    coors = np.stack([batch, np.zeros_like(batch), cells // nx, cells % nx], 1).astype(np.int32)
    feats = rng.randn(len(cells), c).astype(np.float32)
    out["scatter.features"], out["scatter.coors"] = feats, coors
    out["scatter.out"] = sc(torch.from_numpy(feats), torch.from_numpy(coors), 2).numpy()
    out["scatter.single_out"] = sc(torch.from_numpy(feats),
                                   torch.from_numpy(coors[:, 1:]))[0].numpy()
    out["meta"] = np.frombuffer(json.dumps(dict(
        cases=names, voxel_size=VOXEL_SIZE, point_cloud_range=PC_RANGE,
        scatter=dict(in_channels=c, output_shape=[ny, nx], batch_size=2))).encode(), np.uint8)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    sys.exit(main())
