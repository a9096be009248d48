"""MultiBackbone on the GPU: the reference test's shapes (tests/test_models/test_backbones.py
test_multi_backbone, list and dict configs), and shared sampling -- stream 0 samples, the other
streams take its indices -- against independent sampling, bit for bit, outputs and gradients."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SASSG = dict(type="PointNet2SASSG", in_channels=4, num_points=(256, 128, 64, 32),
             radius=(0.2, 0.4, 0.8, 1.2), num_samples=(64, 32, 16, 16),
             sa_channels=((64, 64, 128), (128, 128, 256), (128, 128, 256), (128, 128, 256)),
             fp_channels=((256, 256), (256, 256)), norm_cfg=dict(type="BN2d"))


def _points(dev, batch=1, n=1024, seed=0):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand((batch, n, 4), generator=g)
    pts[..., :3] = pts[..., :3] * 4 - 2
    return pts.to(dev)


def test_reference_shapes_list_and_dict_configs(dev):
    from msmdfusion_amd import registry
    from msmdfusion_amd.pointnet2 import MultiBackbone
    cfg_list = dict(type="MultiBackbone", num_streams=4,
                    suffixes=["net0", "net1", "net2", "net3"],
                    backbones=[copy.deepcopy(SASSG) for _ in range(4)])
    net = registry.build_backbone(cfg_list).to(dev)
    assert isinstance(net, MultiBackbone) and len(net.backbone_list) == 4
    ret = net(_points(dev))
    assert ret["hd_feature"].shape == (1, 256, 128)
    assert ret["fp_xyz_net0"][-1].shape == (1, 128, 3)
    assert ret["fp_features_net0"][-1].shape == (1, 256, 128)
    for suffix in ("net0", "net1", "net2", "net3"):
        assert {"fp_xyz_" + suffix, "fp_features_" + suffix, "fp_indices_" + suffix} <= set(ret)
    assert "sa_level_indices" not in ret and "sa_level_indices_net0" not in ret

    cfg_dict = dict(type="MultiBackbone", num_streams=2, suffixes=["net0", "net1"],
                    aggregation_mlp_channels=[512, 128], backbones=copy.deepcopy(SASSG))
    net = registry.build_backbone(cfg_dict).to(dev)
    assert len(net.backbone_list) == 2
    ret = net(_points(dev))
    assert ret["hd_feature"].shape == (1, 128, 128)
    assert ret["fp_xyz_net0"][-1].shape == (1, 128, 3)
    assert ret["fp_features_net0"][-1].shape == (1, 256, 128)


def test_shared_sampling_equals_independent_sampling_bit_for_bit(dev):
    from msmdfusion_amd import registry
    cfg = dict(type="MultiBackbone", num_streams=3, suffixes=["net0", "net1", "net2"],
               backbones=copy.deepcopy(SASSG))
    torch.manual_seed(5)
    shared = registry.build_backbone(copy.deepcopy(cfg)).to(dev)
    alone = registry.build_backbone(dict(copy.deepcopy(cfg), share_sampling=False)).to(dev)
    assert shared.share_sampling and not alone.share_sampling
    alone.load_state_dict(shared.state_dict())
    pts = _points(dev, batch=2, n=700, seed=3)
    calls = []
    from msmdfusion_amd import pointnet_ops
    real = pointnet_ops.Points_Sampler.forward

    def counting(self, *a, **kw):
        calls.append(1)
        return real(self, *a, **kw)
    pointnet_ops.Points_Sampler.forward = counting
    try:
        out_s = shared(pts)
        n_shared = len(calls)
        out_a = alone(pts)
        n_alone = len(calls) - n_shared
    finally:
        pointnet_ops.Points_Sampler.forward = real
    assert n_shared == 4 and n_alone == 12            # one stream's levels against three
    assert set(out_s) == set(out_a)
    for key in out_s:
        a, b = out_s[key], out_a[key]
        if torch.is_tensor(a):
            assert torch.equal(a, b), key
        else:
            assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), key
    out_s["hd_feature"].square().sum().backward()
    out_a["hd_feature"].square().sum().backward()
    grads = 0
    for (name, p), (_, q) in zip(shared.named_parameters(), alone.named_parameters()):
        assert (p.grad is None) == (q.grad is None), name
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), name
            grads += 1
    assert grads > 50


def test_streams_that_do_not_qualify_sample_on_their_own(dev):
    from msmdfusion_amd import registry
    """A stream sampling by feature distance (F-FPS) cannot take D-FPS indices: it falls back
    to its own sampler, silently."""
    other = dict(copy.deepcopy(SASSG),
                 sa_cfg=dict(type="PointSAModule", pool_mod="max", use_xyz=True,
                             normalize_xyz=True, fps_mod=["F-FPS"]))
    net = registry.build_backbone(dict(type="MultiBackbone", num_streams=2,
                                       suffixes=["net0", "net1"],
                                       backbones=[copy.deepcopy(SASSG), other])).to(dev)
    assert not net.backbone_list[0].shares_sampling_with(net.backbone_list[1])
    assert net.backbone_list[0].shares_sampling_with(net.backbone_list[0])
    ret = net(_points(dev))
    assert ret["fp_xyz_net0"][-1].shape == (1, 128, 3) and ret["fp_xyz_net1"][-1].shape == (1, 128, 3)
    assert not torch.equal(ret["fp_indices_net0"][0], ret["fp_indices_net1"][0])


def test_sassg_takes_given_indices_and_is_unchanged_without_them(dev):
    from msmdfusion_amd import registry
    torch.manual_seed(2)
    net = registry.build_backbone(copy.deepcopy(SASSG)).to(dev).eval()
    pts = _points(dev, batch=2, n=600, seed=9)
    base = net(pts)
    again = net(pts, return_sa_indices=True)
    given = net(pts, sa_indices=again["sa_level_indices"])
    assert set(base) == {"fp_xyz", "fp_features", "fp_indices"}
    for key in base:
        assert all(torch.equal(a, b) and torch.equal(a, c)
                   for a, b, c in zip(base[key], again[key], given[key])), key
