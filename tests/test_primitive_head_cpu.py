"""CPU-side pins of H3DNet's primitive stage: the restated target loop (tests/primitive_ref.py)
against vectors from the reference's own PrimitiveHead (tests/golden/primitive_head_vectors.npz,
written by make_primitive_head_golden.py), state-dict keys, constructor arithmetic, config
fixtures, decode, the loss on the golden's targets, the C-ABI refusals and PointNet2SASSG's
unchanged default path."""
import copy
import ctypes
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_primitive_head_golden as M  # noqa: E402  (the cases and the small head config)
import primitive_ref as R  # noqa: E402

MODES = ("z", "xy", "line")
CFG_KEYS = ("dist_thresh", "var_thresh", "lower_thresh", "num_point", "num_point_line",
            "line_thresh")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "primitive_head_vectors.npz"))


def _within(got, ref32, ref64, what):
    """|got - float64| <= 4 x the reference's own float32 error, per tensor."""
    bound = 4 * float(np.abs(ref32.astype(np.float64) - ref64).max()) if ref64.size else 0.0
    err = float(np.abs(np.asarray(got, np.float64) - ref64).max()) if ref64.size else 0.0
    assert err <= bound, (what, err, bound)


def test_restatement_equals_the_reference_vectors(gold):
    from msmdfusion_amd.head_loss import DepthBoxes
    seen = 0
    for name in M.cases():
        cfg = dict(zip(CFG_KEYS, gold[name + "/cfg"].tolist()))
        cfg["num_point"], cfg["num_point_line"] = int(cfg["num_point"]), int(cfg["num_point_line"])
        with_yaw, masks = bool(gold[name + "/with_yaw"]), bool(gold[name + "/masks"])
        points = torch.from_numpy(gold[name + "/points"])
        for b in range(points.shape[0]):
            boxes = torch.from_numpy(gold["%s/%d/boxes" % (name, b)]).reshape(-1, 7)
            if boxes.shape[0] == 0:
                boxes = torch.zeros((1, 7))
            corners = DepthBoxes(boxes, with_yaw=with_yaw).corners
            prefix = "%s/%d/" % (name, b)
            sem = torch.from_numpy(gold[prefix + ("sem" if masks else "derived_sem")])
            inst = torch.from_numpy(gold[prefix + ("inst" if masks else "derived_inst")])
            for mode in MODES:
                args = (points[b], sem, inst, corners, with_yaw, mode, 18, cfg)
                r32 = R.primitive_targets_ref(*args, torch.float32)
                r64 = R.primitive_targets_ref(*args, torch.float64)
                g32 = {k: gold["%s%s/f32/%s" % (prefix, mode, k)] for k in ("mask", "sem", "offset")}
                g64 = {k: gold["%s%s/f64/%s" % (prefix, mode, k)] for k in ("mask", "sem", "offset")}
                assert np.array_equal(r32[0].numpy(), g32["mask"]), (name, b, mode)
                assert np.array_equal(r64[0].numpy(), g64["mask"]), (name, b, mode)
                assert np.array_equal(r32[2][:, -1].numpy(), g32["sem"][:, -1]), (name, b, mode)
                written = (g32["sem"] != 0).any(1) | (g32["offset"] != 0).any(1)
                mine = ((r32[2] != 0).any(1) | (r32[1] != 0).any(1)).numpy()
                assert np.array_equal(mine, written), (name, b, mode)
                _within(r32[1].numpy(), g32["offset"], g64["offset"], (name, b, mode, "offset"))
                _within(r32[2].numpy(), g32["sem"], g64["sem"], (name, b, mode, "sem"))
                np.testing.assert_allclose(r64[1].numpy(), g64["offset"], rtol=0, atol=1e-12)
                np.testing.assert_allclose(r64[2].numpy(), g64["sem"], rtol=0, atol=1e-12)
                seen += int(g32["mask"].sum() > 0)
    assert seen >= 12


def test_state_dict_keys_equal_the_reference_lists(gold):
    from msmdfusion_amd import registry
    for mode in MODES:
        head = registry.build_head(dict(type="PrimitiveHead", **M.head_cfg(mode, M.PC.SMALL_CFG)))
        assert sorted(head.state_dict()) == gold["keys/head_" + mode].tolist()
    sassg = dict(type="PointNet2SASSG", in_channels=4, num_points=(16, 8), radius=(0.2, 0.4),
                 num_samples=(4, 4), sa_channels=((8, 8), (8, 8)), fp_channels=((8, 8), (8, 8)))
    multi = registry.build_backbone(dict(type="MultiBackbone", num_streams=4, backbones=sassg,
                                         suffixes=("net0", "net1", "net2", "net3")))
    own = sorted(k for k in multi.state_dict() if not k.startswith("backbone_list."))
    assert own == gold["keys/multi_default"].tolist()
    assert sorted({k.split(".")[1] for k in multi.state_dict() if k.startswith("backbone_list.")}) \
        == ["0", "1", "2", "3"]
    assert [tuple(m.conv.weight.shape[:2]) for m in multi.aggregation_layers] == \
        [tuple(r) for r in gold["multi/channels_default"].tolist()]
    given = [24, 12]
    multi2 = registry.build_backbone(dict(type="MultiBackbone", num_streams=2,
                                          backbones=[copy.deepcopy(sassg), copy.deepcopy(sassg)],
                                          aggregation_mlp_channels=given))
    assert given == [16, 24, 12]                      # insert(0, ...) in place, as the reference
    assert sorted(k for k in multi2.state_dict() if not k.startswith("backbone_list.")) == \
        gold["keys/multi_given"].tolist()
    assert [tuple(m.conv.weight.shape[:2]) for m in multi2.aggregation_layers] == \
        [tuple(r) for r in gold["multi/channels_given"].tolist()]
    bn = multi.aggregation_layers.layer0.bn
    assert bn.eps == 1e-5 and bn.momentum == 0.01 and multi.aggregation_layers.layer0.conv.bias \
        is not None
    # the aggregation part computes what the reference's does
    state = {k[len("multi/state/"):]: torch.from_numpy(gold[k]) for k in gold.files
             if k.startswith("multi/state/")}
    multi.load_state_dict(state, strict=False)
    multi.train()
    out = multi.aggregation_layers(torch.from_numpy(gold["multi/in"]).clone())
    torch.testing.assert_close(out, torch.from_numpy(gold["multi/out"]), rtol=1e-5, atol=1e-6)


def test_constructor_arithmetic_and_assertions():
    from msmdfusion_amd import registry
    cfg = dict(type="PrimitiveHead", **M.head_cfg("z", M.PC.SMALL_CFG))
    head = registry.build_head(copy.deepcopy(cfg))
    assert head.gt_per_seed == 1 and head.num_proposal == M.SEEDS
    assert head.flag_conv.conv.weight.shape[:2] == (M.CHANNELS // 2, M.CHANNELS)
    assert head.flag_pred.weight.shape[:2] == (2, M.CHANNELS // 2)
    assert head.conv_pred.conv_out.weight.shape[0] == 3 + 2 + 18
    assert head.vote_aggregation.mlps[0].layer0.conv.weight.shape[1] == M.CHANNELS + 3
    assert cfg["vote_aggregation_cfg"]["mlp_channels"][0] == M.CHANNELS     # the config is intact
    for breaker in (lambda c: c.update(primitive_mode="yz"),
                    lambda c: c["vote_aggregation_cfg"].update(mlp_channels=[M.CHANNELS + 1, 16]),
                    lambda c: c["vote_module_cfg"].update(in_channels="xyz")):
        bad = copy.deepcopy(cfg)
        breaker(bad)
        with pytest.raises(AssertionError):
            registry.build_head(bad)
    sassg = dict(type="PointNet2SASSG", in_channels=4, num_points=(16, 8), radius=(0.2, 0.4),
                 num_samples=(4, 4), sa_channels=((8, 8), (8, 8)), fp_channels=((8, 8), (8, 8)))
    for bad in (dict(num_streams=3, backbones=[sassg, sassg]),                 # length
                dict(num_streams=2, backbones=sassg, suffixes=("a", "b", "c")),  # suffixes
                dict(num_streams=2, backbones=(sassg, sassg))):                 # neither dict nor list
        with pytest.raises(AssertionError):
            registry.build_backbone(dict(type="MultiBackbone", **copy.deepcopy(bad)))


def test_config_constants_equal_the_fixture_and_build():
    from msmdfusion_amd import configs as C, registry
    from msmdfusion_amd.pointnet2 import MultiBackbone, PointNet2SASSG
    from msmdfusion_amd.primitive_head import PrimitiveHead
    fx = json.load(open(os.path.join(HERE, "golden", "reference_h3dnet_config.json")))
    norm = lambda o: json.loads(json.dumps(o))   # noqa: E731  (tuples -> lists)
    assert norm(C.H3DNET_SCANNET_BACKBONE) == fx["backbone"]
    assert norm(C.H3DNET_PRIMITIVE_Z) == fx["primitive_z"]
    assert norm(C.H3DNET_PRIMITIVE_XY) == fx["primitive_xy"]
    assert norm(C.H3DNET_PRIMITIVE_LINE) == fx["primitive_line"]
    assert set(fx) == {"backbone", "primitive_z", "primitive_xy", "primitive_line", "train_cfg",
                       "test_cfg"}
    before = copy.deepcopy(C.H3DNET_SCANNET_BACKBONE)
    net = registry.build_backbone(C.H3DNET_SCANNET_BACKBONE)
    assert C.H3DNET_SCANNET_BACKBONE == before
    assert isinstance(net, MultiBackbone) and len(net.backbone_list) == 4
    assert all(isinstance(b, PointNet2SASSG) for b in net.backbone_list) and net.share_sampling
    assert net.backbone_list[0].shares_sampling_with(net.backbone_list[3])
    assert [tuple(m.conv.weight.shape[:2]) for m in net.aggregation_layers] == \
        [(512, 1024), (256, 512)]
    for mode, cfg in (("z", C.H3DNET_PRIMITIVE_Z), ("xy", C.H3DNET_PRIMITIVE_XY),
                      ("line", C.H3DNET_PRIMITIVE_LINE)):
        before = copy.deepcopy(cfg)
        head = registry.build_head(cfg)
        assert cfg == before
        assert isinstance(head, PrimitiveHead) and head.primitive_mode == mode
        assert head.conv_pred.conv_out.weight.shape[0] == 3 + head.num_dims + 18


def test_decode_and_primitive_centre_match_the_reference(gold):
    from msmdfusion_amd import registry
    for mode in MODES:
        head = registry.build_head(dict(type="PrimitiveHead", **M.head_cfg(mode, M.PC.SMALL_CFG)))
        predictions = torch.from_numpy(gold["decode/%s/predictions" % mode])
        base = torch.from_numpy(gold["decode/%s/center_%s" % (mode, mode)]) - \
            predictions.transpose(2, 1)[:, :, :3]
        got = head.primitive_decode_scores(predictions, base)
        want = {k.split("/")[-1] for k in gold.files if k.startswith("decode/%s/" % mode)} - \
            {"predictions", "flag", "pred_center", "pred_ind"}
        assert set(got) == want
        for k in ("sem_cls_scores_" + mode,) + (("size_residuals_" + mode,) if mode != "line" else ()):
            assert np.array_equal(got[k].numpy(), gold["decode/%s/%s" % (mode, k)])
        centre = torch.from_numpy(gold["decode/%s/center_%s" % (mode, mode)])
        pred_centre, pred_ind = head.get_primitive_center(
            torch.from_numpy(gold["decode/%s/flag" % mode]), centre)
        assert np.array_equal(pred_centre.numpy(), gold["decode/%s/pred_center" % mode])
        assert np.array_equal(pred_ind.numpy(), gold["decode/%s/pred_ind" % mode])
        assert 0 < float(pred_ind.sum()) < pred_ind.numel()


@pytest.mark.parametrize("mode", MODES)
def test_loss_on_the_reference_targets_matches_losses_and_gradients(gold, mode):
    """The reference's targets of the "yaw" case go through PrimitiveHead.loss_from_targets on
    the CPU (where Chamfer takes the reference's own formulation): every loss and every input
    gradient within 4 x the reference's float32-against-float64 difference."""
    from msmdfusion_amd import registry
    head = registry.build_head(dict(type="PrimitiveHead", **M.head_cfg(mode, M.PC.SMALL_CFG)))
    targets = tuple(torch.from_numpy(gold["yaw/targets/%s/%d" % (mode, k)]) for k in range(6))
    points = torch.from_numpy(gold["yaw/points"])
    seed_indices = torch.from_numpy(gold["yaw/seed_indices"])
    seed_points = torch.gather(points[..., :3], 1, seed_indices[..., None].expand(-1, -1, 3))
    prefix = "loss/%s/f32/" % mode
    leaves = {k[len(prefix + "in/"):]: torch.from_numpy(gold[k]).clone().requires_grad_()
              for k in gold.files if k.startswith(prefix + "in/")}
    preds = dict(leaves, seed_points=seed_points, seed_indices=seed_indices)
    preds["aggregated_points_" + mode] = seed_points
    losses = head.loss_from_targets(preds, targets)
    assert set(losses) == {k + mode for k in ("flag_loss_", "vote_loss_", "center_loss_",
                                              "size_loss_", "sem_loss_")}
    sum(losses.values()).backward()
    assert float(targets[5].sum()) > 0
    for name, value in losses.items():
        g32 = gold["loss/%s/f32/%s" % (mode, name)]
        g64 = gold["loss/%s/f64/%s" % (mode, name)]
        print(name, float(value.detach()), float(g32), float(g64))
        _within(value.detach().numpy(), g32, g64, (mode, name))
    if mode == "line":
        assert float(losses["size_loss_line"]) == 0
    for name, leaf in leaves.items():
        _within(leaf.grad.numpy(), gold["loss/%s/f32/grad/%s" % (mode, name)],
                gold["loss/%s/f64/grad/%s" % (mode, name)], (mode, "grad", name))


def test_c_abi_refuses_bad_arguments():
    from msmdfusion_amd._lib import lib
    p = ctypes.c_void_p(256)
    big = 1 << 30
    assert lib.msmd_primitive_max_labels() == 1024
    assert lib.msmd_primitive_point_chunk() >= 64
    ws = lib.msmd_primitive_index_workspace_bytes
    assert ws(2, 1000, 1024) > 2 * 1000 * 4 + 3 * 2 * 1024 * 4
    assert ws(-1, 10, 64) == 0 and ws(1, -1, 64) == 0 and ws(1, 10, 0) == 0
    assert ws(1, 10, 1025) == 0 and ws(1 << 16, 10, 64) == 0
    index = lib.msmd_primitive_index
    assert index(None, None, None, 1, 8, 8, 18, 64, 4, None, 0, None) == -1            # null
    assert index(p, p, p, -1, 8, 8, 18, 64, 4, p, big, None) == -1                      # negative
    assert index(p, p, p, 1, -8, 8, 18, 64, 4, p, big, None) == -1
    assert index(p, p, p, 1, 8, 8, 18, 0, 4, p, big, None) == -1                        # bound
    assert index(p, p, p, 1, 8, 8, 18, 2048, 4, p, big, None) == -1
    assert index(p, p, p, 1, 8, 8, 18, 64, 4, p, 16, None) == -1                        # workspace
    assert index(p, p, p, 0, 0, 0, 18, 64, 4, p, 0, None) == 0                          # empty: ok
    tgt = lib.msmd_primitive_targets_f32

    def call(points=p, ld=4, samples=1, total=8, boxes=2, mode=0, dims=2, bound=64, idx=p,
             idx_bytes=big, out=p):
        return tgt(points, ld, p, p, p, p, samples, total, boxes, 8, 2, 1, mode, dims, 0.2, 0.01,
                   1e-6, 100, 10, 0.2, bound, idx, idx_bytes, out, out, out, None)
    assert call(points=None) == -1 and call(out=None) == -1 and call(idx=None) == -1
    assert call(samples=-1) == -1 and call(total=-1) == -1 and call(boxes=-1) == -1
    assert call(ld=2) == -1
    assert call(mode=3) == -1 and call(mode=-1) == -1                                   # unknown mode
    assert call(mode=0, dims=1) == -1 and call(mode=1, dims=2) == -1                    # num_dims
    assert call(mode=2, dims=1) == -1
    assert call(bound=0) == -1 and call(bound=4096) == -1
    assert call(idx_bytes=64) == -1                                                     # too small
    assert call(samples=0, total=0) == 0


def test_kernels_refuse_cpu_tensors():
    from msmdfusion_amd import kernels as K
    sem = torch.zeros(8, dtype=torch.long)
    off = torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.primitive_index(sem, sem, off, 18)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.primitive_targets(torch.zeros((8, 3)), sem, off, torch.zeros((1, 8, 3)), off,
                            torch.zeros(8, dtype=torch.uint8), "z", True, M.PC.SMALL_CFG)
    assert K.PRIMITIVE_MAX_LABELS == 1024


def test_sassg_forward_without_sa_indices_is_the_loop_it_was():
    """With stand-in SA / FP modules (the real ones need the GPU): forward() without
    sa_indices passes indices=None to every level and returns exactly what the loop of
    pointnet2_sa_ssg.py:104-136 returns on the same modules; with sa_indices each level
    receives its tensor."""
    from msmdfusion_amd.pointnet2 import PointNet2SASSG
    assert inspect.signature(PointNet2SASSG.forward).parameters["sa_indices"].default is None
    net = PointNet2SASSG(in_channels=4, num_points=(8, 4), radius=(0.2, 0.4), num_samples=(4, 4),
                         sa_channels=((8, 8), (8, 8)), fp_channels=((8, 8), (8, 8)))
    seen = []

    class SA(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, xyz, features, indices=None, target_xyz=None):
            seen.append(indices)
            idx = torch.arange(self.m).flip(0).repeat(xyz.shape[0], 1).int() if indices is None \
                else indices
            picked = torch.gather(xyz, 1, idx.long()[..., None].expand(-1, -1, 3))
            return picked, picked.transpose(1, 2) * 2.0, idx

    class FP(torch.nn.Module):
        def forward(self, target, source, target_feats, source_feats):
            return target.transpose(1, 2) + source_feats.mean()

    net.SA_modules = torch.nn.ModuleList([SA(8), SA(4)])
    net.FP_modules = torch.nn.ModuleList([FP(), FP()])
    torch.manual_seed(0)
    points = torch.rand(2, 16, 4)
    got = net(points)
    assert seen == [None, None] and set(got) == {"fp_xyz", "fp_features", "fp_indices"}
    # the loop as it was, on the same modules
    xyz, features = points[..., :3].contiguous(), points[..., 3:].transpose(1, 2).contiguous()
    sa_xyz, sa_feat = [xyz], [features]
    sa_idx = [torch.arange(16).unsqueeze(0).repeat(2, 1).long()]
    for i in range(2):
        a, b, c = net.SA_modules[i](sa_xyz[i], sa_feat[i])
        sa_xyz.append(a), sa_feat.append(b), sa_idx.append(torch.gather(sa_idx[-1], 1, c.long()))
    fp_xyz, fp_feat, fp_idx = [sa_xyz[-1]], [sa_feat[-1]], [sa_idx[-1]]
    for i in range(2):
        fp_feat.append(net.FP_modules[i](sa_xyz[1 - i], sa_xyz[2 - i], sa_feat[1 - i], fp_feat[-1]))
        fp_xyz.append(sa_xyz[1 - i]), fp_idx.append(sa_idx[1 - i])
    for key, want in (("fp_xyz", fp_xyz), ("fp_features", fp_feat), ("fp_indices", fp_idx)):
        assert len(got[key]) == len(want)
        assert all(torch.equal(a, b) for a, b in zip(got[key], want)), key
    del seen[:]
    given = [torch.arange(8).repeat(2, 1).int(), torch.arange(4).repeat(2, 1).int()]
    other = net(points, sa_indices=given, return_sa_indices=True)
    assert seen[0] is given[0] and seen[1] is given[1]
    assert all(a is b for a, b in zip(other["sa_level_indices"], given))
    assert not torch.equal(other["fp_indices"][0], got["fp_indices"][0])
