"""HardVFE, the naiveSync norms, mmdet's FPN, the MVX detectors and their configs without a GPU:
the composition path against the reference's outputs (tests/golden/hard_vfe_vectors.npz),
constructor arithmetic and refusals, the FPN against a functional restatement, registries, the
config fixtures, the neck dispatch of the detector and the C ABI's argument checks."""
import copy
import ctypes
import json
import os
from unittest import mock

import pytest
import torch
from torch import nn
from torch.nn import functional as F

import hard_vfe_fixture as HF

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-4


# ---------------------------------------------------------------- HardVFE, composition
@pytest.mark.parametrize("tag", ["two_train", "two_eval", "one_train", "one_eval"])
def test_composition_matches_the_reference(tag):
    mod, (feats, num, coors), arr = HF.golden_case(tag)
    assert not mod.fused_ok(feats)
    before = feats.clone()
    with torch.no_grad():
        out = mod(feats, num, coors)
    assert out.dtype == torch.float32 and tuple(out.shape) == (97, 64)
    assert HF.scaled_err(out, arr["out"]) <= 1e-6
    assert HF.scaled_err(out, arr["out64"]) <= 2e-6          # float32 against its float64
    assert torch.equal(feats, before), "the input was written"
    state = mod.state_dict()
    for k, v in arr.items():
        if k.startswith("after."):
            if "num_batches" in k:
                assert int(state[k[6:]]) == int(v), k
            else:
                assert HF.scaled_err(state[k[6:]], v) <= 1e-6, k


@pytest.mark.parametrize("tag", ["two_train", "one_eval"])
def test_float64_restatement_reproduces_the_reference_gradients(tag):
    """The yardstick of the GPU tests is the reference: outputs and parameter gradients of the
    reference's own float64 run."""
    mod, inputs, arr = HF.golden_case(tag)
    out, grads = HF.reference_grads(mod, inputs, arr["grad_out"], torch.float64)
    assert HF.scaled_err(out, arr["out64"]) <= 1e-12
    names = [n for n, _ in mod.named_parameters()]
    order = [p for vfe in mod.vfe_layers for p in (vfe.linear.weight, vfe.norm.weight, vfe.norm.bias)]
    for p, g in zip(order, grads):
        name = names[[id(q) for _, q in mod.named_parameters()].index(id(p))]
        assert HF.scaled_err(g, arr["grad64." + name]) <= 1e-10, name


def test_state_dict_keys_and_constructor_arithmetic():
    from msmdfusion_amd.hard_vfe import HardVFE, VFELayer
    _, meta = HF.golden()
    for tag in ("two_train", "one_train"):
        mod, _, _ = HF.golden_case(tag)
        assert list(mod.state_dict()) == meta["cases"][tag]["keys"]
    mod = HardVFE(in_channels=5, feat_channels=[32, 48, 64], with_cluster_center=True,
                  with_voxel_center=True, voxel_size=(0.25, 0.25, 8),
                  point_cloud_range=(-50, -50, -5, 50, 50, 3))
    assert mod.in_channels == 11 and mod.num_vfe == 3 and mod.takes_voxel_table
    assert [tuple(v.linear.weight.shape) for v in mod.vfe_layers] == [(32, 11), (48, 64), (64, 96)]
    assert [(v.max_out, v.cat_max) for v in mod.vfe_layers] == [(True, True), (True, True),
                                                                (True, False)]
    assert (mod.vx, mod.vy, mod.vz) == (0.25, 0.25, 8)
    assert (mod.x_offset, mod.y_offset, mod.z_offset) == (-49.875, -49.875, -1.0)
    assert mod.fusion_layer is None and mod.return_point_feats is False
    plain = HardVFE(feat_channels=[16])
    assert plain.in_channels == 4 and type(plain.vfe_layers[0].norm) is nn.BatchNorm1d
    assert plain.vfe_layers[0].norm.eps == 1e-3 and plain.vfe_layers[0].norm.momentum == 0.01
    layer = VFELayer(6, 8, max_out=False)
    assert tuple(layer(torch.randn(3, 5, 6)).shape) == (3, 5, 8)
    # three layers compose, on the CPU as well
    feats, num, coors = HF.make_voxels(11, 7, 5, seed=1)
    assert tuple(mod(feats, num, coors).shape) == (11, 64)
    with pytest.raises(AssertionError):
        HardVFE(feat_channels=[])


def test_with_distance_keeps_the_shapes_and_names_the_mismatch():
    from msmdfusion_amd.hard_vfe import HardVFE
    mod = HardVFE(in_channels=4, feat_channels=[64], with_distance=True, with_cluster_center=True,
                  with_voxel_center=True)
    assert mod.in_channels == 13 and tuple(mod.vfe_layers[0].linear.weight.shape) == (64, 13)
    feats, num, coors = HF.make_voxels(5, 6, 4, seed=1)
    for call in (mod, mod.forward_composed):
        with pytest.raises(ValueError, match="has 11 channels where vfe_layers.0.linear expects 13"):
            call(feats, num, coors)


def test_fusion_layer_is_refused():
    from msmdfusion_amd.hard_vfe import HardVFE
    with pytest.raises(NotImplementedError, match="fusion_layer"):
        HardVFE(feat_channels=[64], fusion_layer=dict(type="PointFusion"))


# ---------------------------------------------------------------- naiveSync norms
def test_naive_sync_norms_are_plain_batch_norm_in_one_process():
    from msmdfusion_amd.registry import NORM_LAYERS, build_norm_layer
    for kind, base, shape in (("naiveSyncBN1d", nn.BatchNorm1d, (6, 8, 5)),
                              ("naiveSyncBN2d", nn.BatchNorm2d, (3, 8, 4, 5))):
        name, norm = build_norm_layer(dict(type=kind, eps=1e-3, momentum=0.01), 8)
        assert name == "bn" and isinstance(norm, base) and NORM_LAYERS.get(kind) is type(norm)
        plain = base(8, eps=1e-3, momentum=0.01)
        plain.load_state_dict(norm.state_dict())
        assert list(plain.state_dict()) == list(norm.state_dict())
        x = torch.randn(shape)
        for training in (True, False):
            norm.train(training), plain.train(training)
            assert torch.equal(norm(x), plain(x))
        for k, v in plain.state_dict().items():
            assert torch.equal(norm.state_dict()[k], v), k


def test_naive_sync_norms_refuse_multi_rank_training():
    from msmdfusion_amd.registry import build_norm_layer
    norm = build_norm_layer(dict(type="naiveSyncBN2d"), 4)[1]
    x = torch.randn(2, 4, 3, 3)
    with mock.patch("torch.distributed.is_available", return_value=True), \
            mock.patch("torch.distributed.is_initialized", return_value=True), \
            mock.patch("torch.distributed.get_world_size", return_value=2):
        assert not norm.plain_branch()
        with pytest.raises(NotImplementedError, match="all-reduce of the\\s+batch statistics"):
            norm(x)
        norm.eval()
        assert norm.plain_branch() and tuple(norm(x).shape) == (2, 4, 3, 3)
    with mock.patch("torch.distributed.is_available", return_value=True), \
            mock.patch("torch.distributed.is_initialized", return_value=True), \
            mock.patch("torch.distributed.get_world_size", return_value=1):
        norm.train()
        assert norm.plain_branch() and tuple(norm(x).shape) == (2, 4, 3, 3)


# ---------------------------------------------------------------- FPN
def _fpn_functional(fpn, xs):
    """mmdet's FPN written out: conv -> batch_norm -> relu per ConvModule, nearest top-down."""
    def conv_module(m, x, pad):
        x = F.conv2d(x, m.conv.weight, None, padding=pad)
        bn = m.bn
        x = F.batch_norm(x, bn.running_mean.clone(), bn.running_var.clone(), bn.weight, bn.bias,
                         bn.training, bn.momentum, bn.eps)
        return F.relu(x)
    lat = [conv_module(m, x, 0) for m, x in zip(fpn.lateral_convs, xs)]
    for i in range(len(lat) - 1, 0, -1):
        lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode="nearest")
    return [conv_module(m, x, 1) for m, x in zip(fpn.fpn_convs, lat)]


def test_fpn_against_the_functional_restatement():
    from msmdfusion_amd.registry import build_neck
    torch.manual_seed(0)
    fpn = build_neck(dict(type="FPN", norm_cfg=dict(type="naiveSyncBN2d", eps=1e-3, momentum=0.01),
                          act_cfg=dict(type="ReLU"), in_channels=[6, 10, 14], out_channels=8,
                          start_level=0, num_outs=3))
    want_keys = []
    for group in ("lateral_convs", "fpn_convs"):
        for i in range(3):
            want_keys += ["%s.%d.conv.weight" % (group, i)] + [
                "%s.%d.bn.%s" % (group, i, k) for k in ("weight", "bias", "running_mean",
                                                        "running_var", "num_batches_tracked")]
    assert list(fpn.state_dict()) == want_keys
    assert tuple(fpn.lateral_convs[1].conv.weight.shape) == (8, 10, 1, 1)
    assert tuple(fpn.fpn_convs[2].conv.weight.shape) == (8, 8, 3, 3)
    assert fpn.fpn_convs[0].conv.padding == (1, 1) and fpn.lateral_convs[0].conv.bias is None
    assert not fpn.lateral_convs[0].activate.inplace
    bound = (6.0 / (6 + 8)) ** 0.5                            # Xavier-uniform, 1 x 1, 6 -> 8
    w = fpn.lateral_convs[0].conv.weight.detach()
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.5 * bound
    xs = [torch.randn(2, 6, 25, 25), torch.randn(2, 10, 13, 13), torch.randn(2, 14, 7, 7)]
    for training in (True, False):
        fpn.train(training)
        want = _fpn_functional(fpn, xs)
        got = fpn([x.clone().requires_grad_(True) for x in xs])
        assert isinstance(got, tuple) and len(got) == 3
        for a, b in zip(got, want):
            assert a.shape == b.shape and torch.allclose(a, b, atol=1e-6)
    fpn.train()
    sum(o.sum() for o in fpn(xs)).backward()                  # (the top-down add is not in place)
    assert all(p.grad is not None for p in fpn.parameters())
    # start_level / end_level pick the used levels
    sub = build_neck(dict(type="FPN", in_channels=[6, 10, 14], out_channels=8, start_level=1,
                          num_outs=2))
    assert len(sub.lateral_convs) == 2 and sub.lateral_convs[0].conv.bias is not None
    assert [tuple(o.shape) for o in sub(xs)] == [(2, 8, 13, 13), (2, 8, 7, 7)]


def test_fpn_refusals():
    from msmdfusion_amd.bev import FPN
    with pytest.raises(NotImplementedError, match="num_outs"):
        FPN([6, 10, 14], 8, num_outs=5)
    with pytest.raises(NotImplementedError, match="add_extra_convs"):
        FPN([6, 10, 14], 8, num_outs=3, add_extra_convs="on_input")
    with pytest.raises(NotImplementedError, match="upsample_cfg"):
        FPN([6, 10, 14], 8, num_outs=3, upsample_cfg=dict(mode="bilinear"))
    with pytest.raises(NotImplementedError, match="act_cfg"):
        FPN([6, 10, 14], 8, num_outs=3, act_cfg=dict(type="GELU"))
    with pytest.raises(ValueError, match="3 levels"):
        FPN([6, 10, 14], 8, num_outs=3)([torch.zeros(1, 6, 4, 4)])


# ---------------------------------------------------------------- registries, configs
def test_registries_and_config_fixtures():
    from msmdfusion_amd import configs as C
    from msmdfusion_amd import detector  # noqa: F401
    from msmdfusion_amd.registry import (DETECTORS, NECKS, NORM_LAYERS, VOXEL_ENCODERS,
                                         _register_hot_path)
    _register_hot_path()
    assert "HardVFE" in VOXEL_ENCODERS and "FPN" in NECKS
    assert "MVXTwoStageDetector" in DETECTORS and "MVXFasterRCNN" in DETECTORS
    assert "naiveSyncBN1d" in NORM_LAYERS and "naiveSyncBN2d" in NORM_LAYERS
    fx = json.load(open(os.path.join(HERE, "golden", "reference_pointpillars_fpn_configs.json")))
    norm = lambda o: json.loads(json.dumps(o))   # tuples -> lists
    assert norm(C.POINTPILLARS_FPN_NUS) == fx["pointpillars_fpn_nus"]
    assert norm(C.FREE_ANCHOR_POINTPILLARS_FPN_NUS) == fx["free_anchor_pointpillars_fpn_nus"]
    merged = C.FREE_ANCHOR_POINTPILLARS_FPN_NUS
    assert merged["pts_bbox_head"] == C.FREE_ANCHOR_HEAD_NUS
    assert merged["train_cfg"]["pts"]["code_weight"][-1] == 0.25
    assert merged["train_cfg"]["pts"]["assigner"]["type"] == "MaxIoUAssigner"
    assert C.POINTPILLARS_FPN_NUS["train_cfg"]["pts"]["code_weight"][-1] == 0.2


@pytest.mark.parametrize("name,head", [("POINTPILLARS_FPN_NUS", "Anchor3DHead"),
                                       ("FREE_ANCHOR_POINTPILLARS_FPN_NUS", "FreeAnchor3DHead")])
def test_detectors_build_with_the_reference_prefixes(name, head):
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.registry import build_detector
    det = build_detector(getattr(C, name))
    assert type(det).__name__ == "MVXFasterRCNN" and type(det.pts_bbox_head).__name__ == head
    assert type(det.pts_voxel_encoder).__name__ == "HardVFE" and det.voxel_table_encoder
    assert type(det.pts_backbone).__name__ == "SECONDRows" and type(det.pts_neck).__name__ == "FPN"
    keys = list(det.state_dict())
    assert {k.split(".")[0] for k in keys} == {"pts_voxel_encoder", "pts_backbone", "pts_neck",
                                               "pts_bbox_head"}
    assert "pts_neck.fpn_convs.2.bn.running_var" in keys
    assert tuple(det.state_dict()["pts_voxel_encoder.vfe_layers.1.linear.weight"].shape) == (64, 128)
    assert tuple(det.state_dict()["pts_bbox_head.conv_cls.weight"].shape) == (80, 256, 1, 1)
    with pytest.raises(NotImplementedError, match="pts_fusion_layer"):
        build_detector(dict(getattr(C, name), pts_fusion_layer=dict(type="PointFusion")))


def test_neck_dispatch_keeps_the_existing_builds():
    """SECOND / SECONDFPN configs build exactly what they built before the dispatch on `type`:
    the row forms under rows=True, the torch forms otherwise, the same state-dict keys."""
    from msmdfusion_amd import bev, configs as C, grid_conv
    from msmdfusion_amd.registry import build_detector
    for rows, back, neck in ((True, grid_conv.SECONDRows, grid_conv.SECONDFPNRows),
                             (False, bev.SECOND, bev.SECONDFPN)):
        for model in (C.TRANSFUSION_PILLAR_L["model"], C.POINTPILLARS_SECFPN_KITTI["model"]):
            det = build_detector(copy.deepcopy(model), rows=rows)
            assert type(det.pts_backbone) is back and type(det.pts_neck) is neck
            plain_b = bev.SECOND(**{k: v for k, v in (model.get("pts_backbone") or
                                                      model.get("backbone")).items() if k != "type"})
            plain_n = bev.SECONDFPN(**{k: v for k, v in (model.get("pts_neck") or
                                                         model.get("neck")).items() if k != "type"})
            assert list(det.pts_backbone.state_dict()) == list(plain_b.state_dict())
            assert list(det.pts_neck.state_dict()) == list(plain_n.state_dict())
    # a type without a row form goes to the registry, rows or not
    det = build_detector(C.POINTPILLARS_FPN_NUS, rows=True)
    assert type(det.pts_neck) is bev.FPN and type(det.pts_backbone) is grid_conv.SECONDRows
    det = build_detector(C.POINTPILLARS_FPN_NUS, rows=False)
    assert type(det.pts_neck) is bev.FPN and type(det.pts_backbone) is bev.SECOND


# ---------------------------------------------------------------- C ABI
def test_c_abi_refuses_bad_hard_vfe_arguments():
    """Null pointers and shapes outside the built kernels (K > 16, widths > 64, M > 64) return
    a non-zero status before anything is launched."""
    from msmdfusion_amd._lib import lib
    p = ctypes.c_void_p(256)
    geo = (0.25, 0.25, 8.0, -49.875, -49.875, -1.0)

    def moments(n=4, m=20, c=4, flags=3, vox=p, mom=p, ws=p, nbytes=1 << 20):
        return lib.msmd_hard_vfe_moments_f32(vox, p, p, n, m, c, flags, *geo, mom, ws, nbytes, None)

    def stats(n=4, m=20, c=4, flags=3, u1=64, u2=64, w2=p, pivot=p, ws=p, nbytes=1 << 20):
        return lib.msmd_hard_vfe_stats_f32(p, p, p, n, m, c, flags, *geo, p, p, p, u1, w2, u2,
                                           pivot, p, ws, nbytes, None)

    def fwd(n=4, m=20, c=4, flags=3, u1=64, u2=64, w2=p, out=p, arg=p, ymax=p):
        return lib.msmd_hard_vfe_fwd_f32(p, p, p, n, m, c, flags, *geo, p, p, p, u1, w2, p, p, u2,
                                         out, arg, ymax, None)

    def bwd(n=4, m=20, c=4, flags=3, u1=64, u2=64, g2=p, dp=p, sums=p, ws=p, nbytes=1 << 23):
        return lib.msmd_hard_vfe_bwd_f32(p, p, p, n, m, c, flags, *geo, p, p, p, u1, p, p, u2, g2,
                                         p, dp, p, sums, ws, nbytes, None)

    assert lib.msmd_hard_vfe_workspace_bytes(30000, 64) >= 512 * 9280 * 8
    assert lib.msmd_hard_vfe_workspace_bytes(4, 65) == 0
    assert lib.msmd_hard_vfe_workspace_bytes(-1, 64) == 0
    assert moments(vox=None) == -1 and moments(mom=None) == -1 and moments(n=-1) == -1
    assert moments(ws=None) == -2 and moments(nbytes=8) == -2
    assert moments(m=65) == -3 and moments(c=11) == -3 and moments(m=0) == -1
    assert moments(c=2) == -1 and moments(flags=4) == -1
    assert moments(n=0) == 0 and fwd(n=0) == 0 and bwd(n=0) == 0
    assert stats(w2=None) == -1 and stats(pivot=None) == -1 and stats(u2=0) == -1
    assert stats(ws=None) == -2 and stats(u1=65) == -3 and stats(u2=65) == -3
    assert fwd(out=None) == -1 and fwd(arg=None) == -1 and fwd(w2=None) == -1
    assert fwd(ymax=None) == -1 and fwd(u1=0) == -1
    assert fwd(u1=65) == -3 and fwd(u2=65) == -3 and fwd(m=65) == -3 and fwd(c=11) == -3
    assert bwd(g2=None) == -1 and bwd(sums=None) == -1 and bwd(dp=None) == -1
    assert bwd(ws=None) == -2 and bwd(nbytes=1 << 10) == -2 and bwd(u2=65) == -3


def test_wrappers_refuse_cpu_tensors_wrong_dtypes_and_shapes():
    from msmdfusion_amd import kernels as K
    geom = K.HardVFEGeometry(True, True, 0.25, 0.25, 8, -49.875, -49.875, -1.0)
    assert geom.decorated(4) == 10 and geom.flags == 3
    assert K.hard_vfe_supported(64, 4, 10, [64, 64]) and K.hard_vfe_supported(1, 3, 9, [16])
    assert not K.hard_vfe_supported(65, 4, 10, [64]) and not K.hard_vfe_supported(64, 4, 10, [65])
    assert not K.hard_vfe_supported(64, 11, 17, [64]) and not K.hard_vfe_supported(64, 4, 10, [8] * 3)
    assert not K.hard_vfe_supported(64, 2, 8, [64])
    feats, num, coors = HF.make_voxels(5, 6, 4, seed=1)
    w = torch.zeros(64, 10)
    v = torch.zeros(64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.hard_vfe_moments(feats, num, coors, geom)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.hard_vfe_forward(feats, num, coors, geom, [(w, v, v)])
