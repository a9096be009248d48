"""PointNet++ modules and backbones on the GPU: the shapes the reference's own tests assert
(random clouds of the same sizes in place of its .bin files), and SA / FP modules against
pure-torch restatements with the same weights."""
import copy

import numpy as np
import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu

MARGIN = 4.0          # of torch's own float32 error against float64 (tests/test_gpu_pillar.py)


def cloud(dev, b, n, c, seed=0):
    """Multiples of 1/8 in [-1, 1]: exact distances, ties, a dense neighbourhood."""
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.randint(-8, 9, size=(b, n, c)).astype(np.float32) / 8).to(dev)


def xyz_and_features(dev):
    xyz = cloud(dev, 1, 200, 3)
    return xyz, xyz.repeat([1, 1, 4]).transpose(1, 2).contiguous()


# ---------------------------------------------------------------- the reference tests' shapes
@pytest.mark.parametrize("num_point,fps_mod,ranges,total", [
    (16, ["D-FPS"], [-1], 16), (16, ["F-FPS"], [-1], 16), (8, ["FS"], [-1], 16),
    ([8, 12], ["F-FPS", "D-FPS"], [64, -1], 20)])
@pytest.mark.parametrize("dilated", [False, True])
def test_sa_module_msg_shapes(dev, num_point, fps_mod, ranges, total, dilated):
    from msmdfusion_amd.pointnet_modules import PointSAModuleMSG
    mod = PointSAModuleMSG(num_point=num_point, radii=[0.2, 0.4], sample_nums=[4, 8],
                           mlp_channels=[[12, 16], [12, 32]], norm_cfg=dict(type="BN2d"),
                           use_xyz=False, pool_mod="max", fps_mod=fps_mod,
                           fps_sample_range_list=ranges, dilated_group=dilated).to(dev)
    assert mod.mlps[0].layer0.conv.in_channels == 12 and mod.mlps[0].layer0.conv.out_channels == 16
    assert mod.mlps[1].layer0.conv.in_channels == 12 and mod.mlps[1].layer0.conv.out_channels == 32
    xyz, features = xyz_and_features(dev)
    new_xyz, new_features, inds = mod(xyz, features)
    assert new_xyz.shape == torch.Size([1, total, 3])
    assert new_features.shape == torch.Size([1, 48, total])
    assert inds.shape == torch.Size([1, total])
    assert torch.equal(new_xyz, torch.gather(xyz, 1, inds.long()[..., None].expand(-1, -1, 3)))


def test_sa_module_msg_argument_checks():
    from msmdfusion_amd.pointnet_modules import PointSAModuleMSG
    kw = dict(radii=[0.2, 0.4], sample_nums=[4, 8], mlp_channels=[[12, 16], [12, 32]],
              use_xyz=False)
    with pytest.raises(AssertionError):
        PointSAModuleMSG(num_point=8, fps_mod=["F-FPS", "D-FPS"], fps_sample_range_list=[-1], **kw)
    with pytest.raises(AssertionError):
        PointSAModuleMSG(num_point=[8, 8], fps_mod=["F-FPS"], fps_sample_range_list=[-1], **kw)


def test_sa_module_and_fp_module_shapes(dev):
    from msmdfusion_amd.pointnet_modules import PointFPModule, build_sa_module
    mod = build_sa_module(dict(type="PointSAModule", num_point=16, radius=0.2, num_sample=8,
                               mlp_channels=[12, 32], norm_cfg=dict(type="BN2d"), use_xyz=True,
                               pool_mod="max")).to(dev)
    assert mod.mlps[0].layer0.conv.in_channels == 15 and mod.mlps[0].layer0.conv.out_channels == 32
    xyz, features = xyz_and_features(dev)
    new_xyz, new_features, inds = mod(xyz, features)
    assert new_xyz.shape == torch.Size([1, 16, 3])
    assert new_features.shape == torch.Size([1, 32, 16]) and inds.shape == torch.Size([1, 16])
    fp = PointFPModule(mlp_channels=[24, 16]).to(dev)
    assert fp.mlps.layer0.conv.in_channels == 24 and fp.mlps.layer0.conv.out_channels == 16
    pts = cloud(dev, 1, 100, 3, seed=1)[0]
    xyz1, xyz2 = pts[0::2][None].contiguous(), pts[1::3][None].contiguous()
    f1 = xyz1.repeat([1, 1, 4]).transpose(1, 2).contiguous()
    f2 = xyz2.repeat([1, 1, 4]).transpose(1, 2).contiguous()
    assert fp(xyz1, xyz2, f1, f2).shape == torch.Size([1, 16, 50])


def test_pointnet2_sa_ssg_shapes(dev):
    from msmdfusion_amd.registry import build_backbone
    net = build_backbone(dict(type="PointNet2SASSG", in_channels=6, num_points=(32, 16),
                              radius=(0.8, 1.2), num_samples=(16, 8),
                              sa_channels=((8, 16), (16, 16)),
                              fp_channels=((16, 16), (16, 16)))).to(dev)
    assert net.SA_modules[0].mlps[0].layer0.conv.in_channels == 6
    assert net.SA_modules[0].mlps[0].layer0.conv.out_channels == 8
    assert net.SA_modules[0].mlps[0].layer1.conv.out_channels == 16
    assert net.SA_modules[1].mlps[0].layer1.conv.out_channels == 16
    assert net.FP_modules[0].mlps.layer0.conv.in_channels == 32
    assert net.FP_modules[0].mlps.layer0.conv.out_channels == 16
    assert net.FP_modules[1].mlps.layer0.conv.in_channels == 19
    ret = net(cloud(dev, 1, 100, 6))
    fp_xyz, fp_features, fp_indices = ret["fp_xyz"], ret["fp_features"], ret["fp_indices"]
    assert len(fp_xyz) == len(fp_features) == len(fp_indices) == 3
    assert fp_xyz[0].shape == torch.Size([1, 16, 3]) and fp_xyz[1].shape == torch.Size([1, 32, 3])
    assert fp_xyz[2].shape == torch.Size([1, 100, 3])
    assert fp_features[2].shape == torch.Size([1, 16, 100])
    assert fp_indices[2].shape == torch.Size([1, 100]) and fp_indices[2].dtype == torch.int64


def test_pointnet2_sa_msg_shapes(dev):
    from msmdfusion_amd.registry import build_backbone
    cfg = dict(type="PointNet2SAMSG", in_channels=4, num_points=(256, 64, (32, 32)),
               radii=((0.2, 0.4, 0.8), (0.4, 0.8, 1.6), (1.6, 3.2, 4.8)),
               num_samples=((8, 8, 16), (8, 8, 16), (8, 8, 8)),
               sa_channels=(((8, 8, 16), (8, 8, 16), (8, 8, 16)),
                            ((16, 16, 32), (16, 16, 32), (16, 24, 32)),
                            ((32, 32, 64), (32, 24, 64), (32, 64, 64))),
               aggregation_channels=(16, 32, 64),
               fps_mods=(("D-FPS"), ("FS"), ("F-FPS", "D-FPS")),
               fps_sample_range_lists=((-1), (-1), (64, -1)), norm_cfg=dict(type="BN2d"),
               sa_cfg=dict(type="PointSAModuleMSG", pool_mod="max", use_xyz=True,
                           normalize_xyz=False))
    net = build_backbone(cfg).to(dev)
    assert net.SA_modules[0].mlps[0].layer0.conv.in_channels == 4
    assert net.SA_modules[0].mlps[0].layer0.conv.out_channels == 8
    assert net.SA_modules[0].mlps[1].layer1.conv.out_channels == 8
    assert net.SA_modules[2].mlps[2].layer2.conv.out_channels == 64
    assert net.SA_modules[0].mlps[0].layer0.conv.bias is not None       # bias=True reaches it
    # (the reference's .bin holds 100 points; its first stage asks for 256 samples of them)
    ret = net(cloud(dev, 1, 300, 4))
    assert ret["sa_xyz"][-1].shape == torch.Size([1, 64, 3])
    assert ret["sa_features"][-1].shape == torch.Size([1, 64, 64])
    assert ret["sa_indices"][-1].shape == torch.Size([1, 64])
    with pytest.raises(AssertionError):
        build_backbone(dict(cfg, out_indices=(2, 3)))


# ---------------------------------------------------------------- against pure torch
def _gather_groups(feat, idx):
    b, c, _ = feat.shape
    return torch.gather(feat, 2, idx.long().view(b, 1, -1).expand(b, c, -1)).view(
        b, c, idx.shape[1], idx.shape[2])


def sa_restatement(mod, xyz, features, indices, group_idx):
    """PointSAModuleMSG.forward in torch ops only, on the given sampled and ball-query
    indices (integer outputs of the kernels under test elsewhere)."""
    new_xyz = torch.gather(xyz, 1, indices.long()[..., None].expand(-1, -1, 3))
    outs = []
    for grouper, mlp, idx in zip(mod.groupers, mod.mlps, group_idx):
        gxyz = _gather_groups(xyz.transpose(1, 2).contiguous(), idx)
        gxyz = gxyz - new_xyz.transpose(1, 2).unsqueeze(-1)
        if grouper.normalize_xyz:
            gxyz = gxyz / grouper.max_radius
        gf = _gather_groups(features, idx)
        x = mlp(torch.cat([gxyz, gf], dim=1) if grouper.use_xyz else gf)
        pool = F.max_pool2d if mod.pool_mod == "max" else F.avg_pool2d
        outs.append(pool(x, kernel_size=[1, x.size(3)]).squeeze(-1))
    return new_xyz, torch.cat(outs, dim=1)


def _grad_rule(got, ref32, ref64, what):
    err = float((got.double() - ref64).abs().max())
    err_torch = float((ref32.double() - ref64).abs().max())
    ulp = float(np.spacing(np.float32(ref64.abs().max().item())))
    print("%s: err %.3e, torch float32 err %.3e, ulp %.3e" % (what, err, err_torch, ulp))
    assert err <= MARGIN * err_torch + ulp, what


@pytest.mark.parametrize("fps_mod,num_point,ranges", [
    (["D-FPS"], 24, [-1]), (["F-FPS"], 24, [-1]), (["FS"], 12, [-1]),
    (["F-FPS", "D-FPS"], [8, 16], [64, -1])])
@pytest.mark.parametrize("dilated,pool_mod", [(False, "max"), (True, "avg"), (True, "max")])
def test_sa_module_msg_against_torch(dev, fps_mod, num_point, ranges, dilated, pool_mod):
    from msmdfusion_amd import pointnet_ops as P
    from msmdfusion_amd.pointnet_modules import PointSAModuleMSG
    torch.manual_seed(3)
    mod = PointSAModuleMSG(num_point=num_point, radii=[0.3, 0.6], sample_nums=[6, 12],
                           mlp_channels=[[5, 8, 8], [5, 16]], fps_mod=fps_mod,
                           fps_sample_range_list=ranges, dilated_group=dilated,
                           pool_mod=pool_mod, normalize_xyz=True).to(dev)
    xyz = cloud(dev, 2, 257, 3, seed=5)
    feat = torch.randn((2, 5, 257), device=dev)
    f_a = feat.clone().requires_grad_()
    new_xyz, out, inds = mod(xyz, f_a)
    group_idx = [P.ball_query(gr.min_radius, gr.max_radius, gr.sample_num, xyz, new_xyz)
                 for gr in mod.groupers]
    go = torch.randn_like(out)
    out.backward(go)
    grads = [p.grad.clone() for p in mod.parameters()]
    stats = {k: v.clone() for k, v in mod.state_dict().items() if "running" in k}

    ref = copy.deepcopy(mod)
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d):       # undo the first forward's update
            m.reset_running_stats()
    ref.zero_grad()
    f_b = feat.clone().requires_grad_()
    e_xyz, e_out = sa_restatement(ref, xyz, f_b, inds, group_idx)
    assert torch.equal(new_xyz, e_xyz) and torch.equal(out, e_out)
    e_out.backward(go)
    ref64 = copy.deepcopy(ref).double()
    ref64.zero_grad()
    f_c = feat.double().requires_grad_()
    sa_restatement(ref64, xyz.double(), f_c, inds, group_idx)[1].backward(go.double())
    _grad_rule(f_a.grad, f_b.grad, f_c.grad, "input gradient")
    for (name, _), ga, pb, pc in zip(mod.named_parameters(), grads, ref.parameters(),
                                     ref64.parameters()):
        _grad_rule(ga, pb.grad, pc.grad, name)
    for k, v in stats.items():
        assert torch.equal(v, ref.state_dict()[k]), k


def fp_restatement(mod, target, source, target_feats, source_feats):
    """PointFPModule.forward in torch ops only: cdist-free three nearest by the kernel's
    distance expression, inverse-distance weights, torch.gather."""
    if source is not None:
        d = target[:, :, None, :] - source[:, None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        order = torch.sort(d2, dim=2, stable=True)[1][:, :, :3]
        dist = torch.sqrt(torch.gather(d2, 2, order))
        recip = 1.0 / (dist + 1e-8)
        weight = recip / torch.sum(recip, dim=2, keepdim=True)
        b, c, _ = source_feats.shape
        g = torch.gather(source_feats, 2, order.reshape(b, 1, -1).expand(b, c, -1)).view(
            b, c, -1, 3)
        w = weight[:, None]
        interp = (w[..., 0] * g[..., 0] + w[..., 1] * g[..., 1]) + w[..., 2] * g[..., 2]
    else:
        interp = source_feats.expand(*source_feats.size()[0:2], target.size(1))
    x = torch.cat([interp, target_feats], dim=1) if target_feats is not None else interp
    return mod.mlps(x.unsqueeze(-1)).squeeze(-1)


@pytest.mark.parametrize("with_source,with_target_feats", [(True, True), (True, False),
                                                           (False, True)])
def test_fp_module_against_torch(dev, with_source, with_target_feats):
    from msmdfusion_amd.pointnet_modules import PointFPModule
    torch.manual_seed(4)
    c1, c2 = 6, 10
    target = cloud(dev, 2, 130, 3, seed=7)
    source = cloud(dev, 2, 45, 3, seed=8) if with_source else None
    tf = torch.randn((2, c1, 130), device=dev) if with_target_feats else None
    sf = torch.randn((2, c2, 45 if with_source else 1), device=dev)
    mod = PointFPModule(mlp_channels=[c2 + (c1 if with_target_feats else 0), 16, 8]).to(dev)
    s_a = sf.clone().requires_grad_()
    out = mod(target, source, tf, s_a)
    assert tuple(out.shape) == (2, 8, 130)
    go = torch.randn_like(out)
    out.backward(go)
    grads = [p.grad.clone() for p in mod.parameters()]
    ref = copy.deepcopy(mod)
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.reset_running_stats()
    ref.zero_grad()
    s_b = sf.clone().requires_grad_()
    e_out = fp_restatement(ref, target, source, tf, s_b)
    assert torch.equal(out, e_out)
    e_out.backward(go)
    ref64 = copy.deepcopy(ref).double()
    ref64.zero_grad()
    s_c = sf.double().requires_grad_()
    fp_restatement(ref64, target.double(), None if source is None else source.double(),
                   None if tf is None else tf.double(), s_c).backward(go.double())
    _grad_rule(s_a.grad, s_b.grad, s_c.grad, "source feature gradient")
    for (name, _), ga, pb, pc in zip(mod.named_parameters(), grads, ref.parameters(),
                                     ref64.parameters()):
        _grad_rule(ga, pb.grad, pc.grad, name)


# ---------------------------------------------------------------- a training step
def test_pointnet2_sa_ssg_training_step(dev):
    from msmdfusion_amd.pointnet2 import PointNet2SASSG
    torch.manual_seed(0)
    net = PointNet2SASSG(in_channels=6, num_points=(256, 64, 32), radius=(0.3, 0.6, 1.0),
                         num_samples=(16, 8, 8), sa_channels=((8, 16), (16, 16), (16, 32)),
                         fp_channels=((16, 16), (16, 16))).to(dev).train()
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    pts = cloud(dev, 2, 1024, 6, seed=9)
    ret = net(pts)
    loss = sum((f * f).mean() for f in ret["fp_features"])
    loss.backward()
    for name, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    opt.step()
    idx, xyz = ret["fp_indices"][-1], ret["fp_xyz"][-1]
    assert idx.shape == (2, 256) and idx.dtype == torch.int64      # the last FP stage: SA level 1
    assert torch.equal(torch.gather(pts[..., :3], 1, idx[..., None].expand(-1, -1, 3)), xyz)
    first = ret["fp_indices"][0]
    assert torch.equal(torch.gather(pts[..., :3], 1, first[..., None].expand(-1, -1, 3)),
                       ret["fp_xyz"][0])
