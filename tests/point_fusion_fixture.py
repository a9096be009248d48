"""Shared by test_point_fusion_cpu.py and test_gpu_point_fusion.py: the golden cases of
tests/golden/point_fusion_vectors.npz (make_point_fusion_golden.py), synthetic sampler cases and
the float64 restatement (the composition path run in float64)."""
import functools
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def golden():
    z = np.load(os.path.join(HERE, "golden", "point_fusion_vectors.npz"))
    return z, json.loads(str(z["cases"]))


def case_meta(name):
    return json.loads(str(golden()[0][name + "/meta"]))


def golden_case(name, device="cpu", dtype=torch.float32):
    """-> (module with the golden state, (img_feats, pts, pts_feats, img_metas), info)."""
    from msmdfusion_amd.fusion_layers import PointFusion
    z, _ = golden()
    info = case_meta(name)
    mod = PointFusion(**info["kwargs"])
    state = {k: torch.from_numpy(z[name + "/state/" + k]) for k in info["keys"]}
    mod.load_state_dict(state, strict=True)
    mod = mod.to(device=device, dtype=dtype).train(info["training"])
    n_levels, b = len(mod.img_levels), len(info["metas"])
    feats = [torch.from_numpy(z[name + "/map/%d" % i]).to(device=device, dtype=dtype)
             for i in range(n_levels)]
    pts = [torch.from_numpy(z[name + "/pts/%d" % i]).to(device=device, dtype=dtype)
           for i in range(b)]
    pts_feats = torch.from_numpy(z[name + "/pts_feats"]).to(device=device, dtype=dtype)
    return mod, (feats, pts, pts_feats, info["metas"]), info


def arr(name, key, device="cpu"):
    return torch.from_numpy(golden()[0][name + "/" + key]).to(device)


def scaled_err(a, b):
    """max |a - b| over the largest |b| (1 for an all-zero b)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if a.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30)) \
        if float(b.abs().max()) > 0 else float((a - b).abs().max())


def reference_literal_inputs():
    """tests/test_models/test_fusion/test_point_fusion.py::test_sample_single of the reference."""
    lidar2img = torch.tensor([[6.0294e+02, -7.0791e+02, -1.2275e+01, -1.7094e+02],
                              [1.7678e+02, 8.8088e+00, -7.0794e+02, -1.0257e+02],
                              [9.9998e-01, -1.5283e-03, -5.2907e-03, -3.2757e-01],
                              [0.0000e+00, 0.0000e+00, 0.0000e+00, 1.0000e+00]])
    meta = {"transformation_3d_flow": ["R", "S", "T", "HF"], "input_shape": [370, 1224],
            "img_shape": [370, 1224], "lidar2img": lidar2img}
    img_feat = torch.arange(370 * 1224)[None, ...].view(370, 1224)[None, None, ...].float() \
        / (370 * 1224)
    pts = torch.tensor([[8.356, -4.312, -0.445], [11.777, -6.724, -0.564],
                        [6.453, 2.53, -1.612], [6.227, -3.839, -0.563]])
    rot = torch.tensor([[8.660254e-01, 0.5, 0], [-0.5, 8.660254e-01, 0], [0, 0, 1.0e+00]])
    scale, trans = 1.111, torch.tensor([1.0, -1.0, 0.5])
    pts2 = pts @ rot
    pts2 *= scale
    pts2 += trans
    pts2[:, 1] = -pts2[:, 1]
    meta2 = dict(meta, pcd_scale_factor=scale, pcd_rotation=rot, pcd_trans=trans,
                 pcd_horizontal_flip=True)
    expected = torch.tensor([0.5560822, 0.5476625, 0.9687978, 0.6241757])
    return img_feat, ((pts, meta), (pts2, meta2)), expected


def param_grad_errs(name, grads):
    """{key: error} of parameter gradients against the golden float64 ones, each scaled by the
    largest expected entry among the gradients of the same sub-module (`img_transform`,
    `lateral_convs`, ...).  A Linear bias in front of a batch-statistics BatchNorm has an
    exactly zero gradient: what a float32 run leaves there is the rounding of a cancelling sum
    whose terms are of the size of its neighbours' gradients, so that is the scale."""
    exp = {k: arr(name, "grad/" + k) for k in grads}
    scale = {}
    for k, e in exp.items():
        g = k.split(".")[0]
        scale[g] = max(scale.get(g, 0.0), float(e.abs().max()))
    return {k: float((grads[k].detach().double().cpu() - exp[k]).abs().max())
            / max(scale[k.split(".")[0]], 1e-30) for k in grads}


# ---- synthetic sampler cases ----------------------------------------------------------------
def camera(pad_h, pad_w, seed=0):
    """lidar2img of a camera looking along +x: u = cx - f y / x, v = cy - f z / x."""
    rng = np.random.RandomState(seed)
    f, cx, cy = 0.5 * pad_w, 0.5 * pad_w, 0.5 * pad_h
    m = np.array([[cx, -f, 0, 0], [cy, 0, -f, 0], [1, 0, 0, 0], [0, 0, 0, 1]], np.float64)
    m[:2] += rng.uniform(-0.2, 0.2, (2, 4))
    return m


def pixels_to_points(l2i, u, v, depth):
    """Points (float64 [N, 3]) that project to pixel (u, v) at the given depth (plain camera:
    third row of l2i is (1, 0, 0, 0))."""
    a = np.asarray(l2i, np.float64)
    u, v, depth = (np.asarray(t, np.float64) for t in (u, v, depth))
    # rows 0, 1: a[r, :3] . p + a[r, 3] = (u, v) * depth with p.x = depth
    rhs = np.stack([u, v], 1) * depth[:, None] - a[:2, 0] * depth[:, None] - a[:2, 3]
    yz = rhs @ np.linalg.inv(a[:2, 1:3]).T
    return np.concatenate([depth[:, None], yz], 1)


def cloud(n, pad_h, pad_w, l2i, seed=0, margin=0.15):
    """n float32 points, most in view, some outside the image, ~1/16 behind the camera."""
    rng = np.random.RandomState(seed)
    u = rng.uniform(-margin * pad_w, (1 + margin) * pad_w, n)
    v = rng.uniform(-margin * pad_h, (1 + margin) * pad_h, n)
    d = rng.uniform(2, 40, n)
    pts = pixels_to_points(l2i, u, v, d)
    pts[: n // 16] *= -1
    extra = rng.rand(n, 1)
    return np.concatenate([pts, extra], 1).astype(np.float32)


def sampler(channels, align_corners=True, **kw):
    """A PointFusion used for its sampler only: raw maps, one level per entry of channels."""
    from msmdfusion_amd.fusion_layers import PointFusion
    return PointFusion(img_channels=list(channels), pts_channels=4, mid_channels=4,
                       out_channels=4, img_levels=list(range(len(channels))),
                       lateral_conv=False, align_corners=align_corners, **kw)


def restate(mod, maps, pts, metas, dtype):
    """obtain_mlvl_feats by the composition path in `dtype` (float64: the yardstick's truth;
    float32: the torch composition whose error is the yardstick)."""
    return mod.obtain_mlvl_feats_composed([m.to(dtype) for m in maps],
                                          [p.to(dtype) for p in pts], metas)
