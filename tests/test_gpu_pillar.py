"""The pillar path on the GPU: the fused PillarFeatureNet (csrc/pillar.hip) against the
reference's outputs and against float64, its gradients, bitwise reproducibility, the fall-back
to the composition path, PointPillarsScatter, DynamicPillarFeatureNet and the detector built
from TRANSFUSION_PILLAR_L.

The float64 comparisons use a yardstick measured on the same GPU: the error of the float32
torch restatement of the reference's op sequence against the float64 one.  The fused path may
have at most MARGIN times that error (its statistics are summed in another order and through
the moments), with a floor of FLOOR so that a lucky baseline cannot make the bound
unpassable.  tools/pillar_parity.py writes both errors per case to profiles/pillar_parity.txt."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import pillar_fixture as PF

pytestmark = pytest.mark.gpu

TOL = 1e-4       # the project's feature tolerance, of the expected tensor's largest entry
MARGIN = 4.0
FLOOR = 1e-6

SINGLE_LAYER = sorted(t for t in PF.golden()[1]["cases"] if t != "two_layer")

# (N, M, C, U, training, mode, legacy, with_distance): every N, M, C and U the issue names,
# off the workgroup tile (256 // M pillars) and past one partial block
FORWARD = [
    (1, 20, 5, 64, True, "max", True, False),
    (1, 1, 5, 32, False, "max", True, False),
    (63, 1, 3, 1, True, "avg", True, False),
    (63, 64, 3, 128, True, "max", True, True),
    (257, 32, 4, 32, True, "max", False, False),
    (257, 20, 4, 1, False, "avg", False, True),
    (4099, 20, 5, 64, True, "max", True, False),
    (4099, 20, 5, 64, True, "avg", False, False),
    (4099, 64, 5, 128, False, "max", True, False),
    (4099, 32, 3, 32, True, "avg", True, True),
]
BACKWARD = [
    (257, 20, 5, 64, True, "max", True, False),
    (257, 20, 5, 64, False, "max", True, False),
    (257, 20, 5, 64, True, "avg", True, False),
    (257, 20, 5, 64, False, "avg", False, False),
    (4099, 32, 4, 128, True, "max", False, True),
    (63, 64, 3, 1, True, "avg", True, False),
]


def _encoder(dev, c, u, training, mode, legacy, distance, seed=5):
    from msmdfusion_amd.pillar_encoder import PillarFeatureNet
    mod = PillarFeatureNet(in_channels=c, feat_channels=[u], with_distance=distance, mode=mode,
                           legacy=legacy, voxel_size=PF.VOXEL_SIZE, point_cloud_range=PF.PC_RANGE)
    return PF.seed_encoder(mod, seed).train(training).to(dev)


def _leaves(mod, dtype):
    pfn = mod.pfn_layers[0]
    return [p.detach().to(dtype) for p in (pfn.linear.weight, pfn.norm.weight, pfn.norm.bias)]


@pytest.mark.parametrize("tag", SINGLE_LAYER)
def test_fused_matches_the_reference_outputs(dev, tag):
    mod, (feats, num, coors), exp, after = PF.golden_case(tag, dev)
    assert mod.fused_ok(feats)
    before = feats.clone()
    with torch.no_grad():
        out = mod(feats, num, coors)
    assert tuple(out.shape) == tuple(exp.shape) and out.dtype == torch.float32
    err = PF.scaled_err(out, exp)
    print("%s: scaled err %.3e" % (tag, err))
    assert err <= TOL
    assert torch.equal(feats, before), "the input was written"
    state = mod.state_dict()
    for k, v in after.items():
        if "num_batches" in k:
            assert int(state[k]) == int(v), k
        else:
            assert PF.scaled_err(state[k], v) <= TOL, k


@pytest.mark.parametrize("case", FORWARD, ids=lambda c: "N%d-M%d-C%d-U%d-%s-%s-%s%s" % (
    c[0], c[1], c[2], c[3], "train" if c[4] else "eval", c[5], "legacy" if c[6] else "new",
    "-dist" if c[7] else ""))
def test_forward_against_float64(dev, case):
    n, m, c, u, training, mode, legacy, distance = case
    mod = _encoder(dev, c, u, training, mode, legacy, distance)
    inputs = PF.make_pillars(n, m, c, seed=n + m, device=dev)
    assert mod.fused_ok(inputs[0])
    with torch.no_grad():
        y64 = PF.reference_sequence(mod, *inputs, torch.float64, *_leaves(mod, torch.float64))
        y32 = PF.reference_sequence(mod, *inputs, torch.float32, *_leaves(mod, torch.float32))
        out = mod(*inputs)
    assert tuple(out.shape) == (n, u)
    base, err = PF.scaled_err(y32, y64), PF.scaled_err(out, y64)
    print("fp32 torch %.3e  fused %.3e  ratio %.2f" % (base, err, err / max(base, 1e-30)))
    assert err <= max(MARGIN * base, FLOOR)


@pytest.mark.parametrize("case", BACKWARD, ids=lambda c: "N%d-M%d-C%d-U%d-%s-%s" % (
    c[0], c[1], c[2], c[3], "train" if c[4] else "eval", c[5]))
def test_gradients_against_float64_autograd(dev, case):
    n, m, c, u, training, mode, legacy, distance = case
    mod = _encoder(dev, c, u, training, mode, legacy, distance, seed=9)
    inputs = PF.make_pillars(n, m, c, seed=3 * n + m, device=dev)
    go = torch.randn((n, u), generator=torch.Generator().manual_seed(n)).to(dev)
    # no gradient where float32 rounding alone decides which slot receives it (see the fixture)
    go, dropped = PF.unambiguous_grad_out(mod, inputs, go)
    print("grad_out entries dropped as ambiguous: %.3f %%" % (100 * dropped))
    assert dropped < 0.05
    g64 = PF.reference_grads(mod, inputs, go, torch.float64)
    g32 = PF.reference_grads(mod, inputs, go, torch.float32)
    mod.zero_grad()
    out = mod(*inputs)
    out.backward(go)
    pfn = mod.pfn_layers[0]
    got = (out.detach(), pfn.linear.weight.grad, pfn.norm.weight.grad, pfn.norm.bias.grad)
    for name, a, b32, b64 in zip(("out", "dW", "dgamma", "dbeta"), got, g32, g64):
        base, err = PF.scaled_err(b32, b64), PF.scaled_err(a, b64)
        print("%-6s fp32 autograd %.3e  fused %.3e" % (name, base, err))
        assert err <= max(MARGIN * base, FLOOR), name


def test_two_runs_give_the_same_bytes(dev):
    """Forward + backward at the config's size (2 x 30 000 pillars of 20 slots)."""
    inputs = PF.make_pillars(60000, 20, 5, seed=1, device=dev)
    go = torch.randn((60000, 64), device=dev)
    runs = []
    for _ in range(2):
        mod = _encoder(dev, 5, 64, True, "max", True, False)
        out = mod(*inputs)
        out.backward(go)
        pfn = mod.pfn_layers[0]
        runs.append([out.detach(), pfn.linear.weight.grad, pfn.norm.weight.grad,
                     pfn.norm.bias.grad, pfn.norm.running_mean, pfn.norm.running_var])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.isfinite(runs[0][0]).all() and float(runs[0][1].abs().sum()) > 0


def test_fused_equals_composition_on_the_same_module(dev):
    for training, mode in ((True, "max"), (True, "avg"), (False, "max")):
        a = _encoder(dev, 5, 64, training, mode, True, False)
        b = copy.deepcopy(a)
        inputs = PF.make_pillars(1000, 20, 5, seed=2, device=dev)
        with torch.no_grad():
            fused, comp = a(*inputs), b.forward_composed(*inputs)
        assert PF.scaled_err(fused, comp) <= TOL
        for k, v in b.state_dict().items():
            if "running" in k:
                assert PF.scaled_err(a.state_dict()[k], v) <= TOL, k
            elif "num_batches" in k:
                assert int(a.state_dict()[k]) == int(v) == int(training)


class _OtherNorm(nn.BatchNorm1d):
    """Not a plain nn.BatchNorm1d (what a synchronised or converted norm is to the encoder)."""


def test_fallbacks_take_the_composition_path_and_match_the_reference(dev):
    # two layers
    mod, inputs, exp, _ = PF.golden_case("two_layer", dev)
    assert not mod.fused_ok(inputs[0])
    with torch.no_grad():
        assert PF.scaled_err(mod(*inputs), exp) <= TOL
    # an input that requires grad: it gets one
    mod, (feats, num, coors), exp, _ = PF.golden_case("base_legacy_train_max", dev)
    feats = feats.clone().requires_grad_(True)
    assert not mod.fused_ok(feats)
    out = mod(feats, num, coors)
    assert PF.scaled_err(out, exp) <= TOL
    out.sum().backward()
    assert feats.grad is not None and float(feats.grad.abs().sum()) > 0
    # another norm class with the same state
    mod, inputs, exp, _ = PF.golden_case("base_new_train_avg", dev)
    pfn = mod.pfn_layers[0]
    other = _OtherNorm(64, eps=pfn.norm.eps, momentum=pfn.norm.momentum).to(dev)
    other.load_state_dict(pfn.norm.state_dict())
    pfn.norm = other
    assert not mod.fused_ok(inputs[0])
    with torch.no_grad():
        assert PF.scaled_err(mod(*inputs), exp) <= TOL


def test_autocast_still_computes_in_float32(dev):
    mod, inputs, exp, _ = PF.golden_case("base_legacy_eval_max", dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = mod(*inputs)
    assert out.dtype == torch.float32 and PF.scaled_err(out, exp) <= TOL


def test_fused_encoder_does_not_wait_for_the_device(dev):
    """Forward + backward return while the stream still holds work queued before them."""
    mod = _encoder(dev, 5, 64, True, "max", True, False)
    inputs = PF.make_pillars(60000, 20, 5, seed=4, device=dev)
    go = torch.randn((60000, 64), device=dev)
    big = torch.randn((8192, 8192), device=dev)
    mod(*inputs).backward(go)                       # warm: allocations, module load
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    for _ in range(8):
        big = big @ big * 1e-4                      # tens of milliseconds of queued work
    mod(*inputs).backward(go)
    assert not stream.query(), "the encoder synchronised with the device"
    torch.cuda.synchronize()


def _index_put_scatter(feats, coors, batch_size, ny, nx):
    canvas = torch.zeros((batch_size, feats.shape[1], ny, nx), dtype=feats.dtype,
                         device=feats.device)
    canvas[coors[:, 0].long(), :, coors[:, 2].long(), coors[:, 3].long()] = feats
    return canvas


def test_pillar_scatter_golden_and_index_put(dev):
    from msmdfusion_amd.pillar_encoder import PointPillarsScatter
    g, meta = PF.golden()
    sc = PointPillarsScatter(**{k: v for k, v in meta["scatter"].items() if k != "batch_size"})
    feats = torch.from_numpy(g["scatter.features"]).to(dev)
    coors = torch.from_numpy(g["scatter.coors"]).to(dev)
    out = sc(feats, coors, meta["scatter"]["batch_size"])
    assert torch.equal(out.cpu(), torch.from_numpy(g["scatter.out"]))
    assert out.is_contiguous(memory_format=torch.channels_last)
    single = sc(feats, coors[:, 1:])
    assert isinstance(single, list) and len(single) == 1
    assert torch.equal(single[0].cpu(), torch.from_numpy(g["scatter.single_out"]))
    rng = np.random.RandomState(0)
    for batch_size, empty in ((1, None), (3, 1)):
        ny, nx, c = 37, 23, 64
        rows = []
        for b in range(batch_size):
            if b == empty:
                continue
            cells = rng.choice(ny * nx, 300, replace=False)
            rows.append(np.stack([np.full(300, b), np.zeros(300, np.int64), cells // nx,
                                  cells % nx], 1))
        coors = torch.from_numpy(np.concatenate(rows).astype(np.int32)).to(dev)
        feats = torch.randn((coors.shape[0], c), device=dev, requires_grad=True)
        sc = PointPillarsScatter(c, [ny, nx])
        out = sc(feats, coors, batch_size)
        assert tuple(out.shape) == (batch_size, c, ny, nx)
        assert out.permute(0, 2, 3, 1).is_contiguous()
        assert torch.equal(out, _index_put_scatter(feats.detach(), coors, batch_size, ny, nx))
        gmap = torch.randn_like(out)
        out.backward(gmap)
        want = gmap[coors[:, 0].long(), :, coors[:, 2].long(), coors[:, 3].long()]
        assert torch.equal(feats.grad, want)


DYN_VS, DYN_RANGE, DYN_GRID = (0.2, 0.2, 8), (-6.4, -6.4, -5.0, 6.4, 6.4, 3.0), 64


def _dynamic_reference(net, feats, coors, dtype, weights):
    """DynamicPillarFeatureNet.forward of the reference, canvas lookup included, in `dtype`."""
    feats = feats.to(dtype)
    key = ((coors[:, 0].long() * DYN_GRID + coors[:, 2].long()) * DYN_GRID + coors[:, 3].long())
    uniq, inv = torch.unique(key, return_inverse=True)
    canvas_len = int(coors[-1, 0] + 1) * DYN_GRID * DYN_GRID

    def reduce(x, kind):
        if kind == "mean":
            cnt = torch.bincount(inv, minlength=len(uniq)).to(dtype)
            return torch.zeros((len(uniq), x.shape[1]), dtype=dtype,
                               device=x.device).index_add(0, inv, x) / cnt[:, None]
        return torch.zeros((len(uniq), x.shape[1]), dtype=dtype, device=x.device).scatter_reduce(
            0, inv[:, None].expand(-1, x.shape[1]), x, "amax", include_self=False)

    def to_points(v):
        canvas = v.new_zeros((v.shape[1], canvas_len))
        canvas = canvas.index_copy(1, uniq, v.t())
        return canvas[:, key].t()

    ls = [feats]
    ls.append(feats[:, :3] - to_points(reduce(feats, "mean"))[:, :3])
    f_center = feats.new_zeros((feats.shape[0], 2))
    f_center[:, 0] = feats[:, 0] - (coors[:, 3].to(dtype) * net.vx + net.x_offset)
    f_center[:, 1] = feats[:, 1] - (coors[:, 2].to(dtype) * net.vy + net.y_offset)
    ls.append(f_center)
    x = torch.cat(ls, dim=-1)
    kind = net.pfn_scatter.reduce_type
    for i, (pfn, w) in enumerate(zip(net.pfn_layers, weights)):
        bn = pfn[1]
        p = torch.relu(torch.nn.functional.batch_norm(
            torch.nn.functional.linear(x, w), None, None, bn.weight.to(dtype), bn.bias.to(dtype),
            True, 0.0, bn.eps))
        v = reduce(p, kind)
        if i != len(net.pfn_layers) - 1:
            x = torch.cat([p, to_points(v)], dim=1)
    return v, uniq


@pytest.mark.parametrize("feat_channels", [(64, ), (32, 64)])
def test_dynamic_pillar_feature_net(dev, feat_channels):
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd.pillar_encoder import DynamicPillarFeatureNet
    rng = np.random.RandomState(6)
    clouds = [np.concatenate([rng.uniform(-6.3, 6.3, (1500, 2)), rng.uniform(-4.5, 2.5, (1500, 1)),
                              rng.rand(1500, 2)], 1).astype(np.float32) for _ in range(2)]
    pts = [torch.from_numpy(c).to(dev) for c in clouds]
    coors = torch.cat([nn.functional.pad(K.dynamic_voxelize(p, DYN_VS, DYN_RANGE), (1, 0), value=b)
                       for b, p in enumerate(pts)]).contiguous()
    feats = torch.cat(pts)
    assert int(coors.min()) >= 0
    net = PF.seed_encoder(DynamicPillarFeatureNet(in_channels=5, feat_channels=feat_channels,
                                                  voxel_size=DYN_VS, point_cloud_range=DYN_RANGE),
                          7).to(dev).train()
    out, voxel_coors = net(feats, coors)
    w64 = [l[0].weight.detach().double().requires_grad_(True) for l in net.pfn_layers]
    ref, uniq = _dynamic_reference(net, feats, coors, torch.float64, w64)
    got_key = (voxel_coors[:, 0].long() * DYN_GRID + voxel_coors[:, 2].long()) * DYN_GRID + \
        voxel_coors[:, 3].long()
    assert torch.equal(got_key, uniq) and int(voxel_coors[:, 1].abs().max()) == 0
    assert tuple(out.shape) == (len(uniq), feat_channels[-1])
    assert PF.scaled_err(out, ref) <= TOL
    go = torch.randn_like(out)
    out.backward(go)
    ref.backward(go.double())
    for layer, w in zip(net.pfn_layers, w64):
        assert PF.scaled_err(layer[0].weight.grad, w.grad) <= TOL


def _pillar_detector(dev, rows, dynamic=False):
    """TRANSFUSION_PILLAR_L with the point-cloud range cut to +-12.8 m: a 128 x 128 canvas."""
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.detector import build_detector
    pcr = [-12.8, -12.8, -5.0, 12.8, 12.8, 3.0]
    cfg = copy.deepcopy(C.TRANSFUSION_PILLAR_L["model"])
    cfg["pts_voxel_layer"]["point_cloud_range"] = pcr
    cfg["pts_voxel_encoder"]["point_cloud_range"] = pcr
    cfg["pts_middle_encoder"]["output_shape"] = (128, 128)
    cfg["pts_bbox_head"]["bbox_coder"]["pc_range"] = pcr[:2]
    cfg["pts_bbox_head"]["bbox_coder"]["post_center_range"] = [-15, -15, -10.0, 15, 15, 10.0]
    cfg["train_cfg"]["pts"].update(grid_size=[128, 128, 1], point_cloud_range=pcr)
    cfg["test_cfg"]["pts"].update(grid_size=[128, 128, 1], pc_range=pcr[:2])
    if dynamic:
        cfg["pts_voxel_layer"].update(max_num_points=-1, max_voxels=(-1, -1))
        cfg["pts_voxel_encoder"]["type"] = "DynamicPillarFeatureNet"
    torch.manual_seed(0)
    return build_detector(cfg, rows=rows).to(dev).train()


def _step_inputs(dev):
    from msmdfusion_amd.head_loss import LiDARBoxes
    rs = np.random.RandomState(3)
    clouds = [torch.from_numpy(np.concatenate(
        [rs.uniform(-12.7, 12.7, (5000, 2)), rs.uniform(-4.5, 2.5, (5000, 1)),
         rs.rand(5000, 2)], 1).astype(np.float32)).to(dev) for _ in range(2)]
    gt_boxes, gt_labels = [], []
    for _ in range(2):
        g = 5
        box = np.zeros((g, 9), np.float32)
        box[:, 0:2] = rs.uniform(-10, 10, (g, 2))
        box[:, 2] = rs.uniform(-2, 0, g)
        box[:, 3:6] = rs.uniform((0.5, 0.5, 1.0), (2.0, 4.0, 2.5), (g, 3))
        box[:, 6] = rs.uniform(-3, 3, g)
        gt_boxes.append(LiDARBoxes(torch.from_numpy(box).to(dev)))
        gt_labels.append(torch.from_numpy(rs.randint(0, 10, g).astype(np.int64)).to(dev))
    return clouds, gt_boxes, gt_labels


def _train_step(det, clouds, gt_boxes, gt_labels):
    losses = det(clouds, return_loss=True, prepared=det.prepare(clouds), gt_bboxes_3d=gt_boxes,
                 gt_labels_3d=gt_labels)
    total = sum(v for k, v in losses.items() if "loss" in k)
    assert torch.isfinite(total)
    total.backward()
    missing = [n for n, p in det.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing[:5]
    assert all(torch.isfinite(p.grad).all() for p in det.parameters() if p.grad is not None)


@pytest.mark.parametrize("rows", [True, False])
def test_pillar_detector_trains_and_matches_the_composition(dev, rows):
    det = _pillar_detector(dev, rows)
    assert det.voxel_table_encoder and not det.dynamic_voxelization
    clouds, gt_boxes, gt_labels = _step_inputs(dev)
    _train_step(det, clouds, gt_boxes, gt_labels)
    with torch.no_grad():
        (voxels, num), coors, planned = det.prepare(clouds)
        assert planned is None and voxels.shape[1:] == (20, 5) and coors.shape[1] == 4
        assert det.pts_voxel_encoder.fused_ok(voxels)
        got = det(clouds)
        feats = det.pts_voxel_encoder.forward_composed(voxels, num, coors)
        x = _index_put_scatter(feats, coors, 2, 128, 128)
        want = det.pts_neck(det.pts_backbone(x))
    assert len(got) == len(want) == 1 and tuple(got[0].shape) == (2, 384, 32, 32)
    assert PF.scaled_err(got[0], want[0]) <= TOL


def test_dynamic_pillar_detector_trains(dev):
    det = _pillar_detector(dev, True, dynamic=True)
    assert det.dynamic_voxelization and not det.voxel_table_encoder
    _train_step(det, *_step_inputs(dev))
