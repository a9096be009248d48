#!/usr/bin/env python
"""Generates tests/golden/img_fusion_vectors.npz by RUNNING the reference's own code with
fuse_img=True:

    TransFusionHead.forward_single (+ the classes make_head_golden.py takes)
        mmdet3d/models/dense_heads/transfusion_head.py:25-591, 755-1032
    LiDARInstance3DBoxes.corners    mmdet3d/core/bbox/structures/lidar_box3d.py:46-84
    rotation_3d_in_axis             mmdet3d/core/bbox/structures/utils.py:21-61
    apply_3d_transformation         mmdet3d/models/fusion_layers/coord_transform.py:7-90

As in make_head_golden.py the definitions are taken from the reference files at run time (ast)
and the names they import from absent packages get minimal stand-ins: the box class is its
tensor plus the reference's `corners`, the points class of `get_points_type` is the four
in-place operations of BasePoints the flow uses.  The head is assembled by hand from the
reference's classes (:659-745) and gets its parameters from their names
(synthetic.seeded_parameters), so only inputs' seeds, metas and results are stored.

Runs: B = 2 and B = 1, train and eval mode, float32 and float64, dropout 0.  The cameras are
found by a seeded search so that, in the B = 2 training run, sample 0 has two views that share
queries and one view that sees nothing, and sample 1 has a view with exactly one member, one
with exactly two and one with many.  Every run asserts the conditions under which the
reference's discrete results are well defined in float32 (check_margins).
"""
import ast
import copy
import json
import math
import os
import sys
from functools import partial

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import img_fusion_ref as R  # noqa: E402
import make_head_golden as MH  # noqa: E402
from msmdfusion_amd import synthetic as S  # noqa: E402
from msmdfusion_amd.fusion_head import geometry_params  # noqa: E402

REF = "/root/reference/mmdet3d"
OUT = os.path.join(HERE, "img_fusion_vectors.npz")

CFG = dict(num_proposals=24, in_channels=16, hidden_channel=32, num_classes=10,
           num_decoder_layers=1, num_heads=4, nms_kernel_size=3, ffn_channel=48,
           common_heads=dict(center=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2)),
           grid=(12, 12), num_views=3, in_channels_img=8, out_size_factor_img=4, img_hw=(6, 10))
TEST_CFG = dict(dataset="nuScenes", grid_size=[96, 96, 40], out_size_factor=8,
                pc_range=[-6.0, -6.0], voxel_size=[0.075, 0.075], nms_type=None)
CODER_CFG = dict(pc_range=[-6.0, -6.0], out_size_factor=8, voxel_size=[0.075, 0.075],
                 post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], score_threshold=0.0,
                 code_size=10)
SEEN = []                       # the boxes every LiDARInstance3DBoxes was built from


class _Points:                  # BasePoints / LiDARPoints: what apply_3d_transformation calls
    def __init__(self, tensor):
        self.tensor = tensor

    coord = property(lambda self: self.tensor[:, :3])

    def flip(self, bev_direction="horizontal"):
        if bev_direction == "horizontal":
            self.tensor[:, 1] = -self.tensor[:, 1]
        else:
            self.tensor[:, 0] = -self.tensor[:, 0]

    def scale(self, scale_factor):
        self.tensor[:, :3] *= scale_factor

    def translate(self, trans_vector):
        self.tensor[:, :3] += trans_vector

    def rotate(self, rotation):
        self.tensor[:, :3] = self.tensor[:, :3] @ rotation


class _Conv1dAnyInput(nn.Conv1d):
    """nn.Conv1d taking the reference's `one_hot.float()` in a float64 head as well."""

    def forward(self, x):
        return super().forward(x.to(self.weight.dtype))


def _functions(path, names):
    tree = ast.parse(open(path).read())
    return [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name in names]


def reference_namespace():
    ns = MH.reference_namespace()
    ns.update(partial=partial, get_points_type=lambda kind: _Points)
    body = _functions(os.path.join(REF, "core/bbox/structures/utils.py"), {"rotation_3d_in_axis"})
    body += _functions(os.path.join(REF, "models/fusion_layers/coord_transform.py"),
                       {"apply_3d_transformation"})
    exec(compile(ast.Module(body=body, type_ignores=[]), "reference", "exec"), ns)
    (corners,) = _functions(os.path.join(REF, "core/bbox/structures/lidar_box3d.py"), {"corners"})
    corners.decorator_list = []
    exec(compile(ast.Module(body=[corners], type_ignores=[]), "lidar_box3d", "exec"), ns)

    class LiDARInstance3DBoxes:
        def __init__(self, tensor, box_dim=7):
            SEEN.append(tensor.detach().clone())
            self.tensor = tensor

        dims = property(lambda self: self.tensor[:, 3:6])
        corners = property(ns["corners"])
    ns["LiDARInstance3DBoxes"] = LiDARInstance3DBoxes
    return ns


def build_reference_head(ns):
    """TransFusionHead.__init__ (:659-756) with fuse_img=True, from the reference's classes."""
    c = CFG
    head = nn.Module()
    head.num_classes, head.num_proposals, head.auxiliary = c["num_classes"], c["num_proposals"], True
    head.num_decoder_layers, head.fuse_img = c["num_decoder_layers"], True
    head.initialize_by_heatmap, head.nms_kernel_size = True, c["nms_kernel_size"]
    head.num_views, head.out_size_factor_img = c["num_views"], c["out_size_factor_img"]
    head.test_cfg = dict(TEST_CFG)
    head.bbox_coder = ns["TransFusionBBoxCoder"](**CODER_CFG)
    hid = c["hidden_channel"]
    head.shared_conv = nn.Conv2d(c["in_channels"], hid, 3, padding=1, bias=True)
    head.heatmap_head = nn.Sequential(
        MH._ConvModule(hid, hid, 3, padding=1, bias="auto", conv_cfg=dict(type="Conv2d"),
                       norm_cfg=dict(type="BN2d")),
        nn.Conv2d(hid, c["num_classes"], 3, padding=1, bias=True))
    head.class_encoding = _Conv1dAnyInput(c["num_classes"], hid, 1)

    def layer(**kw):
        return ns["TransformerDecoderLayer"](
            hid, c["num_heads"], c["ffn_channel"], 0.0, "relu",
            self_posembed=ns["PositionEmbeddingLearned"](2, hid),
            cross_posembed=ns["PositionEmbeddingLearned"](2, hid), **kw)
    head.decoder = nn.ModuleList([layer() for _ in range(c["num_decoder_layers"])])

    def ffn(cin):
        heads = copy.deepcopy(c["common_heads"])
        heads.update(dict(heatmap=(c["num_classes"], 2)))
        return ns["FFN"](cin, heads, conv_cfg=dict(type="Conv1d"), norm_cfg=dict(type="BN1d"),
                         bias="auto")
    head.prediction_heads = nn.ModuleList([ffn(hid) for _ in range(c["num_decoder_layers"])])
    head.shared_conv_img = nn.Conv2d(c["in_channels_img"], hid, 3, padding=1, bias=True)
    head.heatmap_head_img = copy.deepcopy(head.heatmap_head)
    head.decoder.append(layer())
    for _ in range(c["num_views"]):
        head.decoder.append(layer(cross_only=True))
    head.fc = nn.Sequential(nn.Conv1d(hid, hid, kernel_size=1))
    head.prediction_heads.append(ffn(hid * 2))
    for m in head.modules():                                   # init_bn_momentum (:776-779)
        if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
            m.momentum = 0.1
    head.create_2D_grid = lambda x, y: ns["create_2D_grid"](head, x, y)
    head.bev_pos = head.create_2D_grid(*c["grid"])
    head.img_feat_pos = None
    head.img_feat_collapsed_pos = None
    return head


def inputs(batch, dtype):
    x = np.random.RandomState(31).standard_normal((2, CFG["in_channels"], *CFG["grid"]))
    img = np.random.RandomState(32).standard_normal(
        (2 * CFG["num_views"], CFG["in_channels_img"], *CFG["img_hw"]))
    x, img = x[:batch], img[:batch * CFG["num_views"]]
    return torch.from_numpy(x).to(dtype), torch.from_numpy(img).to(dtype)


def base_metas():
    """Everything of the metas but the cameras: a 3-D flow (rotation, scale, translation,
    flip), and per sample its own image scale / crop / flip."""
    a = 0.3
    rot = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
    pad = (CFG["img_hw"][0] * 4, CFG["img_hw"][1] * 4)            # (24, 40)
    m0 = dict(input_shape=pad, img_shape=(22, 38, 3), scale_factor=[0.5, 0.5, 0.5, 0.5],
              img_crop_offset=[2.0, 1.0], flip=False, pcd_rotation=rot.tolist(),
              pcd_scale_factor=1.05, pcd_trans=[0.2, -0.1, 0.05], pcd_horizontal_flip=True,
              pcd_vertical_flip=False, transformation_3d_flow=["R", "S", "T", "HF"])
    m1 = dict(input_shape=pad, img_shape=(24, 39, 3), scale_factor=[0.4, 0.4, 0.4, 0.4],
              flip=True, pcd_rotation=rot.T.tolist(), pcd_scale_factor=0.95,
              pcd_horizontal_flip=False, pcd_vertical_flip=True,
              transformation_3d_flow=["HF", "R", "S", "VF"])
    return [m0, m1]


def camera(yaw, f, pos, scale):
    """lidar2img [4, 4] of a camera at `pos` looking along (cos yaw, sin yaw, 0); the principal
    point is the centre of the un-rescaled image."""
    c, s = math.cos(yaw), math.sin(yaw)
    rot = np.array([[s, -c, 0], [0, 0, -1.0], [c, s, 0]])
    ext = np.eye(4)
    ext[:3, :3], ext[:3, 3] = rot, -rot @ np.asarray(pos, np.float64)
    k = np.eye(4)
    k[0, 0] = k[1, 1] = f
    k[0, 2], k[1, 2] = 20.0 / scale, 12.0 / scale
    return k @ ext


def check_margins(pos3d, boxes, metas, what):
    """The conditions under which the reference's discrete results are well defined in
    float32; raises if the inputs break any.  -> the float64 geometry."""
    B = pos3d.shape[0]
    osf = CFG["out_size_factor_img"]
    params = geometry_params(metas, CFG["num_views"], skip_flow=B == 1)
    g64 = R.geometry(pos3d, boxes, params, osf, np.float64)
    g32 = R.geometry(pos3d.astype(np.float32), boxes.astype(np.float32),
                     params.astype(np.float32), osf, np.float32)
    h, w = metas[0]["input_shape"]
    for g in (g64, g32):
        px, py = g["pix"][..., 0].astype(np.float64), g["pix"][..., 1].astype(np.float64)
        border = np.minimum.reduce([abs(px), abs(px - w), abs(py), abs(py - h)])
        assert np.all(border[np.isfinite(border)] >= 1e-3), what + ": a query pixel on the border"
        used = g["on"] & g["valid"][:, :, None]
        for c in (px[used], py[used]):
            frac = c / osf - np.round(c / osf)
            assert np.all(abs(frac) * osf >= 1e-3), what + ": a pixel on a multiple of osf"
        arg = g["radius_arg"][used].astype(np.float64)
        assert np.all(abs(arg - np.round(arg)) >= 1e-3), what + ": a radius argument on an integer"
        cut = -math.log(float(R.EPS32))
        hh, ww = CFG["img_hw"]
        d2 = R.key_d2(g["centre"][used], hh, ww).astype(np.float64)
        ratio = d2 / (2.0 * g["sigma"][used].astype(np.float64)[:, None] ** 2)
        assert np.all(abs(ratio / cut - 1.0) >= 1e-4), what + ": a key on the eps cut-off"
    for k in ("on", "valid", "winner"):
        assert np.array_equal(g64[k], g32[k]), what + ": float32 and float64 disagree on " + k
    used = g64["on"] & g64["valid"][:, :, None]
    for k in ("centre", "radius"):          # (of the queries the reference computes them for)
        assert np.array_equal(g64[k][used], g32[k][used]), \
            what + ": float32 and float64 disagree on " + k
    return g64


def boxes_of(seen):
    boxes = np.stack([b.double().numpy() for b in seen])                     # [B, P, 7]
    height = boxes[..., 2] + boxes[..., 5] * 0.5
    pos3d = np.stack([boxes[..., 0], boxes[..., 1], height], 1)              # [B, 3, P]
    return pos3d, boxes


def find_cameras(pos3d, boxes):
    """A seeded search for the cameras of the B = 2 training run (module docstring)."""
    rng = np.random.RandomState(7)
    metas = base_metas()
    V = CFG["num_views"]
    for m in metas:
        m["lidar2img"] = [camera(0.0, 300.0, [0, 0, 40.0], m["scale_factor"][0])
                          for _ in range(V)]                  # (sees nothing)
    want = {(0, 0): lambda n, g: n >= 8, (0, 2): lambda n, g: n == 0,
            (0, 1): lambda n, g: n >= 6 and (g["on"][0, 0] & g["on"][0, 1]).sum() >= 2
            and (g["on"][0, 0] & ~g["on"][0, 1]).sum() >= 2,
            (1, 0): lambda n, g: n == 1, (1, 1): lambda n, g: n == 2, (1, 2): lambda n, g: n >= 8}
    for (b, v) in [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]:
        for _ in range(20000):
            wide = (b, v) in ((0, 0), (0, 1), (1, 2))
            yaw = rng.uniform(0, 2 * math.pi)
            f = rng.uniform(25, 60) if wide else rng.uniform(150, 500)
            pos = [rng.uniform(-9, 9), rng.uniform(-9, 9), rng.uniform(0.5, 2.5)]
            if (b, v) == (0, 2):
                pos[2] = 40.0                               # far above the scene, looking sideways
            metas[b]["lidar2img"][v] = camera(yaw, f, pos, metas[b]["scale_factor"][0])
            try:
                g = check_margins(pos3d, boxes, metas, "search")
            except AssertionError:
                continue
            if want[(b, v)](int(g["count"][b, v]), g):
                break
        else:
            raise RuntimeError("no camera found for sample %d view %d" % (b, v))
    return metas


def loss_weights(res):
    """The scalar the gradients are taken of: sum_k <res[k], cos(0.37 i + k)>."""
    total = 0
    for j, k in enumerate(sorted(res)):
        w = torch.cos(0.37 * torch.arange(res[k].numel(), dtype=res[k].dtype) + j)
        total = total + (res[k].reshape(-1) * w).sum()
    return total


def typed(ns, proto, dtype):
    """A copy of the head in `dtype`, its position grids included (plain attributes)."""
    head = copy.deepcopy(proto).to(dtype)
    head.create_2D_grid = lambda x, y: ns["create_2D_grid"](head, x, y).to(dtype)
    head.bev_pos = head.bev_pos.to(dtype)
    return head


def run(ns, proto, metas, batch, train, dtype, want_grad=False):
    head = typed(ns, proto, dtype).train(train)
    x, img = inputs(batch, dtype)
    x.requires_grad_(want_grad), img.requires_grad_(want_grad)
    del SEEN[:]
    with torch.set_grad_enabled(want_grad):
        (res,) = ns["forward_single"](head, x, img, [copy.deepcopy(m) for m in metas[:batch]])
    pos3d, boxes = boxes_of(SEEN)
    what = "B=%d %s %s" % (batch, "train" if train else "eval", dtype)
    g = check_margins(pos3d, boxes, metas[:batch], what)
    assert np.array_equal(g["mask"], head.on_the_image_mask.numpy()), what
    out = {k: v.detach().numpy() for k, v in res.items()}
    out["on_the_image_mask"] = head.on_the_image_mask.numpy()
    out["query_labels"] = head.query_labels.numpy()
    out["count"] = g["count"]
    if train:
        for k, v in head.state_dict().items():
            if "running_" in k or "num_batches_tracked" in k:
                out["buf/" + k] = v.numpy()
    if want_grad:
        loss_weights(res).backward()
        out["grad_x"], out["grad_img"] = x.grad.numpy(), img.grad.numpy()
        if dtype == torch.float64:
            out["pos3d"], out["boxes"] = pos3d, boxes
    return out, (pos3d, boxes, g)


def main():
    ns = reference_namespace()
    proto = S.seeded_parameters(build_reference_head(ns), seed=41)
    # the queries do not depend on the cameras: take them from a run with placeholder metas
    placeholder = base_metas()
    for m in placeholder:
        m["lidar2img"] = [camera(0.5 * v, 40.0, [0, 0, 1.0], m["scale_factor"][0])
                          for v in range(CFG["num_views"])]
    head = typed(ns, proto, torch.float64).train()
    x, img = inputs(2, torch.float64)
    del SEEN[:]
    with torch.no_grad():
        ns["forward_single"](head, x, img, placeholder)
    metas = find_cameras(*boxes_of(SEEN))

    out = {}
    for batch in (2, 1):
        for train in (True, False):
            labels = None
            for dtype in (torch.float64, torch.float32):
                grad = batch == 2 and train
                got, (pos3d, boxes, g) = run(ns, proto, metas, batch, train, dtype, grad)
                if labels is not None:
                    assert np.array_equal(labels, got["query_labels"])
                labels = got["query_labels"]
                tag = "B%d_%s_%s/" % (batch, "train" if train else "eval",
                                      "f64" if dtype == torch.float64 else "f32")
                for k, v in got.items():
                    if dtype == torch.float32 and (k in ("count",) or k.startswith("buf/")
                                                   and "num_batches" in k):
                        continue
                    out[tag + k] = v
                if grad and dtype == torch.float64:     # the scene the docstring promises
                    c = g["count"]
                    assert c[0, 2] == 0 and c[1, 0] == 1 and c[1, 1] == 2 and c[1, 2] >= 8, c
                    both = g["on"][0, 0] & g["on"][0, 1]
                    assert both.sum() >= 2
                    params = geometry_params(metas, CFG["num_views"], False)
                    m = params[0, 0, :12].reshape(3, 4)
                    depth = m[2, :3] @ pos3d[0] + m[2, 3]
                    assert (depth < 0).any(), "no query behind camera (0, 0)"
    out["metas_json"] = np.array(json.dumps(
        [dict(m, lidar2img=[a.tolist() for a in m["lidar2img"]]) for m in metas]))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
