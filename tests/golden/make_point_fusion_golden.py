#!/usr/bin/env python
"""Generates tests/golden/point_fusion_vectors.npz by RUNNING the reference's own Python code:

    point_sample, PointFusion    mmdet3d/models/fusion_layers/point_fusion.py
    apply_3d_transformation      mmdet3d/models/fusion_layers/coord_transform.py:7-90
    BasePoints, LiDARPoints      mmdet3d/core/points/{base_points,lidar_points}.py

mmdet3d itself cannot be imported here (mmcv is not installed), so the definitions are pulled
out of the reference FILES at run time (ast) and compiled as they stand; mmcv's ConvModule and
xavier_init, the registry and get_points_type are local stand-ins written by hand.  BasePoints
casts its tensor to float32; for the float64 runs the point classes see a `torch` whose
as_tensor keeps a float64 tensor as it is, so that the float64 results are float64 throughout.
Nothing of the reference is written to the repo: the .npz holds seeded inputs, the layer
weights, the float32 outputs the reference code returned on CPU, the running statistics a
training forward left, the float64 outputs and float64 gradients (loss = sum(out * grad_out))
of the parameters, the maps and pts_feats, and the state-dict key names.  Build container only
(/root/reference).
"""
import ast
import copy
import json
import os
from functools import partial

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/mmdet3d"
OUT = os.path.join(ROOT, "tests", "golden", "point_fusion_vectors.npz")


class _Registry:
    def register_module(self, *a, **kw):
        return lambda cls: cls


class ConvModule(nn.Module):
    """Stand-in for mmcv.cnn.ConvModule as PointFusion uses it: conv -> norm -> act, the conv
    biased only without a norm, the norm under `bn`."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, conv_cfg=None,
                 norm_cfg=None, act_cfg=None, inplace=True):
        super().__init__()
        assert conv_cfg is None
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, padding=padding,
                              bias=norm_cfg is None)
        self.bn = None
        if norm_cfg is not None:
            cfg = {k: v for k, v in norm_cfg.items() if k not in ("type", "requires_grad")}
            cfg.setdefault("eps", 1e-5)
            self.bn = nn.BatchNorm2d(out_channels, **cfg)
        self.activate = None if act_cfg is None else nn.ReLU(inplace=inplace)

    def forward(self, x):
        x = self.conv(x)
        if self.bn is not None:
            x = self.bn(x)
        return x if self.activate is None else self.activate(x)


def xavier_init(module, gain=1, bias=0, distribution="normal"):
    assert distribution in ["uniform", "normal"]
    if hasattr(module, "weight") and module.weight is not None:
        if distribution == "uniform":
            nn.init.xavier_uniform_(module.weight, gain=gain)
        else:
            nn.init.xavier_normal_(module.weight, gain=gain)
    if hasattr(module, "bias") and module.bias is not None:
        nn.init.constant_(module.bias, bias)


class _TorchKeepDouble:
    """`torch` for the point classes: as_tensor leaves a float64 tensor float64."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def as_tensor(data, dtype=None, device=None):
        if isinstance(data, torch.Tensor) and data.dtype == torch.float64:
            return torch.as_tensor(data, device=device)
        return torch.as_tensor(data, dtype=dtype, device=device)


def reference_defs():
    def pull(ns, path, names):
        tree = ast.parse(open(os.path.join(REF, path)).read())
        body = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef))
                and n.name in names]
        assert len(body) == len(names), (path, names)
        exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)

    from abc import abstractmethod
    pts_ns = {"torch": _TorchKeepDouble(), "np": np, "abstractmethod": abstractmethod}
    pull(pts_ns, "core/points/base_points.py", ("BasePoints",))
    pull(pts_ns, "core/points/lidar_points.py", ("LiDARPoints",))

    def get_points_type(points_type):
        assert points_type == "LIDAR"
        return pts_ns["LiDARPoints"]

    ns = {"torch": torch, "nn": nn, "F": F, "partial": partial, "ConvModule": ConvModule,
          "xavier_init": xavier_init, "FUSION_LAYERS": _Registry(),
          "get_points_type": get_points_type}
    pull(ns, "models/fusion_layers/coord_transform.py", ("apply_3d_transformation",))
    pull(ns, "models/fusion_layers/point_fusion.py", ("point_sample", "PointFusion"))
    return ns


# ---- inputs ---------------------------------------------------------------------------------
PAD = (80, 128)                     # padded input shape (h, w)
SIZES = [(20, 32), (10, 16), (5, 8), (3, 4), (2, 3)]


def lidar2img(rng):
    """x forward, y left, z up -> u = cx - f y / x, v = cy - f z / x (slightly perturbed)."""
    f, cx, cy = 64.0, 64.0, 40.0
    m = np.array([[cx, -f, 0, 0], [cy, 0, -f, 0], [1, 0, 0, 0], [0, 0, 0, 1]], np.float64)
    m[:3] += rng.uniform(-0.02, 0.02, (3, 4)) * np.array([[10], [10], [0.01]])
    return m


def cloud(rng, n):
    """Mostly in view, some outside the image, a few behind the camera."""
    x = rng.uniform(2, 40, n)
    y = rng.uniform(-1.3, 1.3, n) * x
    z = rng.uniform(-0.8, 0.8, n) * x
    pts = np.stack([x, y, z, rng.rand(n)], 1)
    pts[: max(1, n // 16), 0] *= -1
    return pts.astype(np.float32)


def metas(rng, kind, b):
    out = []
    for i in range(b):
        m = dict(lidar2img=lidar2img(rng).tolist(), input_shape=list(PAD),
                 img_shape=[76, 120, 3])
        if kind == "augmented" and i == 0:
            m.update(flip=True, img_crop_offset=[3.5, -2.25],
                     scale_factor=[0.9, 0.8, 0.9, 0.8])
        if kind == "augmented" and i == b - 1:
            a = 0.3
            m.update(transformation_3d_flow=["R", "S", "T", "HF", "VF"],
                     pcd_rotation=[[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0],
                                   [0, 0, 1.0]],
                     pcd_scale_factor=1.05, pcd_trans=[0.4, -0.3, 0.1],
                     pcd_horizontal_flip=True, pcd_vertical_flip=i % 2 == 0)
        out.append(m)
    return out


def forward_flow(ns, pts, meta):
    """The cloud as the detector sees it: the 3-D augmentation applied to the sensor's cloud."""
    xyz = ns["apply_3d_transformation"](torch.from_numpy(pts[:, :3].copy()), "LIDAR", meta,
                                        reverse=False)
    return np.concatenate([xyz.numpy(), pts[:, 3:]], 1).astype(np.float32)


CASES = {
    # name: (constructor kwargs, training, meta kind, cloud sizes)
    "eval_lateral_3": (dict(img_channels=8, pts_channels=6, mid_channels=8, out_channels=12,
                            img_levels=[0, 1, 2], norm_cfg=dict(type="BN"),
                            act_cfg=dict(type="ReLU")), False, "plain", (150, 97)),
    "train_lateral_5": (dict(img_channels=[4, 6, 8, 6, 4], pts_channels=6, mid_channels=8,
                             out_channels=12, img_levels=[0, 1, 2, 3, 4], align_corners=False,
                             norm_cfg=dict(type="BN")), True, "augmented", (140, 101)),
    "train_raw_1": (dict(img_channels=[16], pts_channels=5, mid_channels=10, out_channels=10,
                         img_levels=[0], lateral_conv=False, fuse_out=True), True, "augmented",
                    (120, 75)),
    "eval_raw_3": (dict(img_channels=[3, 5, 4], pts_channels=5, mid_channels=9, out_channels=9,
                        img_levels=[0, 1, 2], lateral_conv=False, fuse_out=True,
                        activate_out=False, align_corners=False), False, "augmented", (64, 0, 33)),
}


def seed_module(mod, seed):
    g = torch.Generator().manual_seed(seed)
    """Keeps the Xavier weights of the constructor; non-trivial biases, norm affines and
    running statistics."""
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) * 0.4 - 0.2)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
            elif isinstance(m, (nn.Linear, nn.Conv2d)) and m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)


def run_case(ns, name, kwargs, training, kind, sizes, seed, out):
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)
    fuse = ns["PointFusion"](**kwargs)
    seed_module(fuse, seed)
    b = len(sizes)
    ms = metas(rng, kind, b)
    pts = [forward_flow(ns, cloud(rng, n), m) if n else np.zeros((0, 4), np.float32)
           for n, m in zip(sizes, ms)]
    chans = fuse.img_channels
    feats = [rng.randn(b, c, *SIZES[lv]).astype(np.float32)
             for c, lv in zip(chans, fuse.img_levels)]
    pts_feats = rng.randn(sum(sizes), kwargs["pts_channels"]).astype(np.float32)
    grad_out = rng.randn(sum(sizes), kwargs["out_channels"]).astype(np.float32)
    state = {k: v.clone() for k, v in fuse.state_dict().items()}

    def run(dtype):
        m = copy.deepcopy(fuse).to(dtype)
        m.train(training)
        f = [torch.from_numpy(x).to(dtype).requires_grad_() for x in feats]
        pf = torch.from_numpy(pts_feats).to(dtype).requires_grad_()
        p = [torch.from_numpy(x).to(dtype) for x in pts]
        # obtain_mlvl_feats' result, seen where forward hands it on (a second call would move
        # the lateral norms' running statistics twice)
        seen = []
        m.img_transform.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
        # (the reference cats nothing for an empty cloud: squeeze() breaks there)
        keep = [i for i in range(b) if sizes[i] > 0]
        res = m([x[keep] for x in f] if len(keep) != b else f, [p[i] for i in keep], pf,
                [ms[i] for i in keep])
        img_pts = seen[0]
        return m, f, pf, res, img_pts

    m32, _, _, res32, img32 = run(torch.float32)
    out[name + "/out32"] = res32.detach().numpy()
    out[name + "/img_pts32"] = img32.detach().numpy()
    if training:
        for k, v in m32.state_dict().items():
            if "running" in k or "num_batches" in k:
                out[name + "/after/" + k] = v.numpy()
    m64, f64, pf64, res64, img64 = run(torch.float64)
    (res64 * torch.from_numpy(grad_out).double()).sum().backward()
    out[name + "/out64"] = res64.detach().numpy()
    out[name + "/img_pts64"] = img64.detach().numpy()
    for k, p in m64.named_parameters():
        out[name + "/grad/" + k] = p.grad.numpy()
    for i, x in enumerate(f64):
        out[name + "/grad_map/%d" % i] = x.grad.numpy()
        out[name + "/map/%d" % i] = feats[i]
    out[name + "/grad_pts_feats"] = pf64.grad.numpy()
    for i, x in enumerate(pts):
        out[name + "/pts/%d" % i] = x
    out[name + "/pts_feats"] = pts_feats
    out[name + "/grad_out"] = grad_out
    for k, v in state.items():
        out[name + "/state/" + k] = v.numpy()
    out[name + "/meta"] = np.array(json.dumps(dict(kwargs=kwargs, training=training, metas=ms,
                                                   keys=list(state))))


def main():
    ns = reference_defs()
    out = {}
    for seed, (name, (kwargs, training, kind, sizes)) in enumerate(CASES.items()):
        run_case(ns, name, kwargs, training, kind, sizes, 100 + seed, out)
    # apply_3d_transformation itself, both directions, on the fullest meta
    rng = np.random.RandomState(7)
    meta = metas(rng, "augmented", 1)[0]
    pts = cloud(rng, 40)[:, :3]
    out["flow/pts"] = pts
    out["flow/meta"] = np.array(json.dumps(meta))
    for rev in (False, True):
        for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
            r = ns["apply_3d_transformation"](torch.from_numpy(pts).to(dtype), "LIDAR", meta,
                                              reverse=rev)
            out["flow/%s%s" % ("reverse" if rev else "forward", tag)] = r.numpy()
    out["cases"] = np.array(json.dumps(list(CASES)))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
