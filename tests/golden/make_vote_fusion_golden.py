#!/usr/bin/env python
"""Generates tests/golden/vote_fusion_vectors.npz by RUNNING the reference's own Python code:

    VoteFusion                         mmdet3d/models/fusion_layers/vote_fusion.py
    apply_3d_transformation, extract_2d_info, coord_2d_transform, bbox_2d_transform
                                       mmdet3d/models/fusion_layers/coord_transform.py
    Coord3DMode (convert_point)        mmdet3d/core/bbox/structures/coord_3d_mode.py
    points_cam2img                     mmdet3d/core/bbox/structures/utils.py
    BasePoints, DepthPoints            mmdet3d/core/points/{base_points,depth_points}.py
    sample_valid_seeds                 mmdet3d/models/detectors/imvotenet.py
    MLP                                mmdet3d/models/utils/mlp.py

mmdet3d itself cannot be imported here (mmcv is not installed), so the definitions are pulled
out of the reference FILES at run time (ast) and compiled as they stand; mmcv's ConvModule, the
registry and get_points_type are local stand-ins written by hand.  BasePoints casts its tensor
to float32; for the float64 runs the point classes see a `torch` whose as_tensor keeps a float64
tensor as it is.  VoteFusion creates its zeros in the default dtype, so the float64 runs set
torch's default dtype to float64.  Nothing of the reference is written to the repo: the .npz
holds seeded inputs, the outputs the reference code returned on CPU in float32 and float64, and
key names.  Build container only (/root/reference).

The uv rounding is discontinuous, so the inputs are generated for the reference to be well
defined: seeds are back-projected in float64 from chosen pixels and depths through the inverse
chain, redrawn until u - 1, v - 1 lie within 0.3 of an integer and the rescaled pixel at least
1e-3 from a half-integer (float64, from the float32 seed); the script asserts that the float32
and the float64 runs agree on every rounded pixel, in-box flag, chosen index and the mask, that
in-box scores are pairwise distinct per seed, and that the xz cue is well conditioned (forward
coordinate >= 0.5, |ray_y| >= 0.2).
"""
import ast
import json
import os
from abc import abstractmethod
from enum import IntEnum, unique
from functools import partial

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/mmdet3d"
OUT = os.path.join(ROOT, "tests", "golden", "vote_fusion_vectors.npz")


class _Registry:
    def register_module(self, *a, **kw):
        return lambda cls: cls


class ConvModule(nn.Module):
    """Stand-in for mmcv.cnn.ConvModule as MLP uses it: Conv1d (biased as asked) -> BN1d under
    `bn` -> ReLU."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, conv_cfg=None,
                 norm_cfg=None, act_cfg=None, bias="auto", inplace=True):
        super().__init__()
        assert conv_cfg == dict(type="Conv1d") and norm_cfg == dict(type="BN1d")
        assert act_cfg == dict(type="ReLU")
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size, padding=padding,
                              bias=bias is True)
        self.bn = nn.BatchNorm1d(out_channels)
        self.activate = nn.ReLU(inplace=inplace)

    def forward(self, x):
        return self.activate(self.bn(self.conv(x)))


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

    pts_ns = {"torch": _TorchKeepDouble(), "np": np, "abstractmethod": abstractmethod}
    pull(pts_ns, "core/points/base_points.py", ("BasePoints",))
    pull(pts_ns, "core/points/depth_points.py", ("DepthPoints",))

    def get_points_type(points_type):
        assert points_type == "DEPTH"
        return pts_ns["DepthPoints"]

    ns = {"torch": torch, "nn": nn, "np": np, "partial": partial, "IntEnum": IntEnum,
          "unique": unique, "FUSION_LAYERS": _Registry(), "get_points_type": get_points_type,
          "BasePoints": pts_ns["BasePoints"], "ConvModule": ConvModule, "EPS": 1e-6}
    pull(ns, "models/fusion_layers/coord_transform.py",
         ("apply_3d_transformation", "extract_2d_info", "bbox_2d_transform", "coord_2d_transform"))
    pull(ns, "core/bbox/structures/coord_3d_mode.py", ("Coord3DMode",))
    pull(ns, "core/bbox/structures/utils.py", ("points_cam2img",))
    pull(ns, "models/fusion_layers/vote_fusion.py", ("VoteFusion",))
    pull(ns, "models/detectors/imvotenet.py", ("sample_valid_seeds",))
    pull(ns, "models/utils/mlp.py", ("MLP",))
    return ns


# ---- inputs ---------------------------------------------------------------------------------
PAD = (48, 64)                      # padded image (h, w)
ORI = (36, 50)                      # the image before the augmentation (h, w)
FLOWS = ([], ["HF", "R", "S", "T"], ["R", "S", "T", "HF"])


def calib(rng):
    """SUN RGB-D style: depth frame x right, y forward, z up; Rt a small tilt, K a pinhole."""
    a, b = rng.uniform(-0.08, 0.08, 2)
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    f = rng.uniform(38.0, 44.0)
    k = np.array([[f, 0, ORI[1] / 2 + rng.uniform(-1, 1)], [0, f, ORI[0] / 2 + rng.uniform(-1, 1)],
                  [0, 0, 1.0]])
    return rx @ rz, k


def meta(rng, flow, scaled, flip):
    m = dict(ori_shape=[ORI[0], ORI[1], 3])
    if scaled:
        sx, sy = 1.2, 1.25
        m.update(scale_factor=[sx, sy, sx, sy], img_shape=[int(ORI[0] * sy), int(ORI[1] * sx), 3])
    else:
        m.update(img_shape=[ORI[0], ORI[1], 3])
    if flip:
        m.update(flip=True)
    if flow:
        a = rng.uniform(0.15, 0.35) * rng.choice([-1, 1])
        m.update(transformation_3d_flow=list(flow),
                 pcd_rotation=[[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0], [0, 0, 1.0]],
                 pcd_scale_factor=float(rng.uniform(0.9, 1.1)),
                 pcd_trans=rng.uniform(-0.2, 0.2, 3).tolist(), pcd_horizontal_flip=True)
    return m


def boxes(rng, n, m, one_conf):
    """n boxes (l, t, r, b, conf, class) in the rescaled frame, their original-frame edges off
    the pixel grid; distinct confidences; optionally one conf == 1.0."""
    out = np.zeros((n, 6))
    conf = rng.permutation(np.linspace(0.08, 0.93, max(n, 1)))[:n]
    for j in range(n):
        w, h = rng.randint(12, ORI[1] - 6), rng.randint(10, ORI[0] - 4)
        l, t = rng.randint(0, ORI[1] - w) + 0.37, rng.randint(0, ORI[0] - h) + 0.41
        out[j] = [l, t, l + w + 0.2, t + h + 0.15, conf[j], rng.randint(0, m["num_classes"])]
    if one_conf and n:
        out[n - 1, 4] = 1.0
    sx, sy = m.get("scale_factor", [1.0, 1.0])[:2]
    out[:, [0, 2]] *= sx
    out[:, [1, 3]] *= sy
    if m.get("flip", False):
        w = m["img_shape"][1]
        out[:, [0, 2]] = w - out[:, [2, 0]]
    return out.astype(np.float32)


def chain64(ns, seeds, m, rt, k):
    """The reference's own projection chain on float64 seeds -> (xyz_cam, uv before - 1 and
    round, uv_rescaled before round)."""
    xyz = ns["apply_3d_transformation"](seeds, "DEPTH", m, reverse=True)
    c3 = ns["Coord3DMode"]
    cam = c3.convert_point(xyz, c3.DEPTH, c3.CAM, rt_mat=rt)
    uv = ns["points_cam2img"](cam, k)
    return cam, uv, ns["coord_2d_transform"](m, (uv - 1).round(), True)


def well_defined(ns, seeds32, m, rt, k, bx):
    """Per seed: whether the reference is well defined there (see the module docstring)."""
    with _default_dtype(torch.float64):
        s = torch.from_numpy(seeds32).double()
        cam, uv, resc = chain64(ns, s, m, torch.from_numpy(rt), torch.from_numpy(k))
    pre = (uv - 1).numpy()
    ok = (np.abs(pre - np.rint(pre)) < 0.3).all(1)
    r = resc.numpy()
    ok &= (np.abs(r - np.floor(r) - 0.5) >= 1e-3).all(1)
    rr = np.rint(r)
    ok &= (rr[:, 0] >= 0) & (rr[:, 0] < m["img_shape"][1]) & (rr[:, 1] >= 0) & \
        (rr[:, 1] < m["img_shape"][0])
    ok &= seeds32[:, 1] >= 0.5
    return ok


class _default_dtype:
    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.old = torch.get_default_dtype()
        torch.set_default_dtype(self.dtype)

    def __exit__(self, *a):
        torch.set_default_dtype(self.old)


def make_seeds(ns, rng, n, m, rt, k, bx):
    """Back-project chosen pixels and depths (float64) through the inverse chain, apply the
    forward flow, round to float32; redraw what is not well defined."""
    out = np.zeros((n, 3), np.float32)
    todo = np.arange(n)
    d2c = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]]) @ rt.T
    for _ in range(200):
        if todo.size == 0:
            return out
        c = todo.size
        u = rng.randint(2, ORI[1] - 2, c) + 1 + rng.uniform(-0.25, 0.25, c)
        v = rng.randint(2, ORI[0] - 2, c) + 1 + rng.uniform(-0.25, 0.25, c)
        z = rng.uniform(1.0, 4.0, c)
        cam = (np.linalg.inv(k) @ np.stack([u, v, np.ones(c)])) * z
        depth = (np.linalg.inv(d2c) @ cam).T
        with _default_dtype(torch.float64):
            fwd = ns["apply_3d_transformation"](torch.from_numpy(depth), "DEPTH", m, reverse=False)
        out[todo] = fwd.numpy().astype(np.float32)
        todo = todo[~well_defined(ns, out[todo], m, rt, k, bx)]
    raise AssertionError("could not draw well-defined seeds")


def details(ns, fuse, img, bx, seeds, m, rt, k):
    """What VoteFusion.forward computes on the way, by the same reference calls: rounded
    pixels, in-box flags [S, Nb], the chosen indices [S, K] (topk) and their scores."""
    cam, uv, resc = chain64(ns, seeds, m, rt, k)
    uv0 = (uv - 1).round()
    res = dict(uv_origin=uv0.numpy(), uv_rescaled=resc.round().numpy(), xyz_cam=cam.numpy())
    if bx.shape[0]:
        b0 = ns["bbox_2d_transform"](m, bx, False)
        inb = (uv0[:, None, 0] > b0[None, :, 0]) & (uv0[:, None, 0] < b0[None, :, 2]) & \
            (uv0[:, None, 1] > b0[None, :, 1]) & (uv0[:, None, 1] < b0[None, :, 3])
        score = inb.to(bx.dtype) + bx[None, :, 4]
        kk = fuse.max_imvote_per_pixel
        if bx.shape[0] < kk:
            score = torch.cat([score, score.new_zeros(score.shape[0], kk - bx.shape[0])], 1)
        val, idx = score.topk(kk, dim=1, largest=True, sorted=True)
        res.update(in_box=inb.numpy(), chosen=idx.numpy(), chosen_score=val.numpy(),
                   bbox_origin=b0.numpy())
    return res


CASES = {
    # name: (num_classes, K, seeds per sample, boxes per sample, (scaled, flip) per sample)
    "c10": (10, 3, 100, (7, 0, 2), ((True, True), (False, False), (True, False))),
    # (no box-free sample here: the reference's empty branch hard-codes 15 cue rows, which
    # stacks with the other samples only at num_classes = 10)
    "c3": (3, 3, 77, (2, 7, 2), ((True, False), (True, True), (False, False))),
}


def run_case(ns, name, spec, seed, out):
    num_classes, kk, s, nbs, augs = spec
    rng = np.random.RandomState(seed)
    fuse = ns["VoteFusion"](num_classes=num_classes, max_imvote_per_pixel=kk)
    b = len(nbs)
    order = rng.permutation(3)
    metas, rts, ks, bxs, seeds = [], [], [], [], []
    for i in range(b):
        m = meta(rng, FLOWS[order[i]], *augs[i])
        rt, k = calib(rng)
        bx = boxes(rng, nbs[i], dict(m, num_classes=num_classes), one_conf=nbs[i] == 7)
        metas.append(m), rts.append(rt), ks.append(k), bxs.append(bx)
        seeds.append(make_seeds(ns, rng, s, m, rt, k, bx))
    imgs = np.zeros((b, 3) + PAD, np.float32)
    for i, m in enumerate(metas):
        h, w = m["img_shape"][:2]
        imgs[i, :, :h, :w] = rng.randint(0, 256, (3, h, w))
    seeds = np.stack(seeds)
    rt_all, k_all = np.stack(rts), np.stack(ks)

    def run(dtype):
        with _default_dtype(dtype):
            t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)      # noqa: E731
            calibs = dict(Rt=t(rt_all), K=t(k_all))
            img_in = t(imgs)
            feat, mask = fuse(img_in, [t(x) for x in bxs], t(seeds), metas, calibs)
            det = [details(ns, fuse, img_in[i], t(bxs[i]), t(seeds[i]), metas[i], calibs["Rt"][i],
                           calibs["K"][i]) for i in range(b)]
        return feat.numpy(), mask.numpy(), det

    f32, m32, d32 = run(torch.float32)
    f64, m64, d64 = run(torch.float64)
    assert f32.dtype == np.float32 and f64.dtype == np.float64
    # ---- the reference is well defined on these inputs
    assert np.array_equal(m32, m64), name
    for i in range(b):
        for key in ("uv_origin", "uv_rescaled"):
            assert np.array_equal(d32[i][key], d64[i][key]), (name, i, key)
        if nbs[i]:
            assert np.array_equal(d32[i]["in_box"], d64[i]["in_box"]), (name, i)
            inb = d64[i]["in_box"]
            sc = inb.astype(np.float32) + bxs[i][None, :, 4]
            for r in range(s):
                v = sc[r][inb[r]]
                assert len(np.unique(v)) == len(v), (name, i, r)
            # chosen indices agree wherever the slot is visible (in-box or conf == 1)
            vis = np.floor(d64[i]["chosen_score"]) != 0
            assert np.array_equal(d32[i]["chosen"][vis], d64[i]["chosen"][vis]), (name, i)
            assert np.array_equal(vis, np.floor(d32[i]["chosen_score"]) != 0)
            # |ray_y| of every visible pair (rows 3 of the cue block)
            cols = f64[i, 3].reshape(kk, s).T
            inb_slot = np.take_along_axis(np.concatenate(
                [inb, np.zeros((s, max(kk - nbs[i], 0)), bool)], 1), d64[i]["chosen"], 1)
            assert (np.abs(cols[inb_slot]) >= 0.2).all(), (name, i, np.abs(cols[inb_slot]).min())
        assert (seeds[i][:, 1] >= 0.5).all()
    out[name + "/feat32"], out[name + "/feat64"] = f32, f64
    out[name + "/mask"] = m32
    out[name + "/seeds"], out[name + "/imgs"] = seeds, imgs.astype(np.uint8)
    out[name + "/Rt"], out[name + "/K"] = rt_all, k_all
    for i in range(b):
        out[name + "/boxes/%d" % i] = bxs[i]
        out[name + "/uv_origin/%d" % i] = d64[i]["uv_origin"].astype(np.int32)
        out[name + "/uv_rescaled/%d" % i] = d64[i]["uv_rescaled"].astype(np.int32)
        out[name + "/xyz_cam64/%d" % i] = d64[i]["xyz_cam"]
        if nbs[i]:
            out[name + "/in_box/%d" % i] = d64[i]["in_box"]
            out[name + "/chosen/%d" % i] = d64[i]["chosen"].astype(np.int32)
            out[name + "/chosen_score/%d" % i] = d32[i]["chosen_score"]
            out[name + "/bbox_origin32/%d" % i] = d32[i]["bbox_origin"]
    out[name + "/meta"] = np.array(json.dumps(dict(num_classes=num_classes, max_imvote_per_pixel=kk,
                                                   metas=metas)))
    hits = sum(int(d64[i]["in_box"].sum()) for i in range(b) if nbs[i])
    print(name, "in-box pairs", hits, "valid slots", int(m32.sum()), "of", m32.size)


def main():
    ns = reference_defs()
    out = {}
    for seed, (name, spec) in enumerate(CASES.items()):
        run_case(ns, name, spec, 300 + seed, out)
    # apply_3d_transformation('DEPTH') itself, both directions, both flow orders
    rng = np.random.RandomState(11)
    pts = rng.uniform(-3, 3, (40, 3)).astype(np.float32)
    out["flow/pts"] = pts
    for tag, flow in (("a", FLOWS[1]), ("b", FLOWS[2]), ("vf", ["T", "VF", "S", "R"])):
        m = meta(rng, flow, False, False)
        if tag == "vf":
            m.update(pcd_vertical_flip=True, pcd_horizontal_flip=False)
        out["flow/%s/meta" % tag] = np.array(json.dumps(m))
        for rev in (False, True):
            for dtype, d in ((torch.float32, "32"), (torch.float64, "64")):
                r = ns["apply_3d_transformation"](torch.from_numpy(pts).to(dtype), "DEPTH", m,
                                                  reverse=rev)
                out["flow/%s/%s%s" % (tag, "reverse" if rev else "forward", d)] = r.numpy()
    # the 2-D transforms on a flipped, scaled, cropped meta
    m2 = dict(img_shape=[45, 60, 3], ori_shape=[36, 50, 3], scale_factor=[1.2, 1.25, 1.2, 1.25],
              flip=True, img_crop_offset=[2.0, -1.0])
    bx = boxes(rng, 6, dict(m2, num_classes=4), False)
    uv = rng.randint(0, 50, (12, 2)).astype(np.float32)
    out["t2d/meta"], out["t2d/boxes"], out["t2d/uv"] = np.array(json.dumps(m2)), bx, uv
    for o2n in (False, True):
        out["t2d/boxes_%d" % o2n] = ns["bbox_2d_transform"](m2, torch.from_numpy(bx), o2n).numpy()
        out["t2d/uv_%d" % o2n] = ns["coord_2d_transform"](m2, torch.from_numpy(uv), o2n).numpy()
    # sample_valid_seeds: the reference's draws on seeded masks (S = 16 sampled of 3 S imvotes)
    s = 16
    torch.manual_seed(5)
    masks = np.zeros((6, 3 * s), bool)
    for row, cnt in enumerate((0, 1, s - 1, s, s + 1, 3 * s)):
        masks[row, rng.permutation(3 * s)[:cnt]] = True
    out["svs/mask"] = masks
    out["svs/inds"] = ns["sample_valid_seeds"](torch.from_numpy(masks), s).numpy()
    # MLP: key names and one eval forward
    torch.manual_seed(6)
    mlp = ns["MLP"](in_channel=18, conv_channels=(8, 6))
    with torch.no_grad():
        for mod in mlp.modules():
            if isinstance(mod, nn.BatchNorm1d):
                mod.running_mean.normal_(0, 0.1), mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.5, 1.5), mod.bias.normal_(0, 0.1)
    mlp.eval()
    x = torch.randn(2, 18, 9)
    out["mlp/x"], out["mlp/y"] = x.numpy(), mlp(x).detach().numpy()
    out["mlp/keys"] = np.array(json.dumps(list(mlp.state_dict())))
    for kname, v in mlp.state_dict().items():
        out["mlp/state/" + kname] = v.numpy()
    out["cases"] = np.array(json.dumps(list(CASES)))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
