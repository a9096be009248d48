"""HardVFE on the GPU: the fused one- and two-layer stack (csrc/hard_vfe.hip) against the
reference's outputs and against float64, its gradients, the backward sums at tile and
grid-stride boundaries, bitwise reproducibility, the fall-backs, and the MVXFasterRCNN detectors
built from POINTPILLARS_FPN_NUS / FREE_ANCHOR_POINTPILLARS_FPN_NUS.

The float64 comparisons use the yardstick of test_gpu_pillar.py: the error of the float32
torch restatement of the reference's op sequence against the float64 one, measured on the same
GPU.  The fused path may have at most MARGIN times that error, with a floor of FLOOR.

Gradients: max and ReLU routing are discrete, and among thousands of decisions some pair lies
within float32 rounding, where any float32 evaluation may route differently from float64.  The
gradient cases therefore leave out, judged on the float64 restatement alone
(hard_vfe_fixture.exclusions): grad_out entries whose last-layer slot or ReLU is decided by less
than TAU, and (two layers) the layer-1 rows of channels with such a decision anywhere.  Both
sets are capped (MAX_CHANNELS_OUT of the layer-1 channels, MAX_ZEROED of the entries) and the
seeds below were chosen so that the restatement, on the CPU and on the GPU, stays inside the caps
and its float32 form stays within TAU / 4 of its float64 form."""
import copy
from unittest import mock

import numpy as np
import pytest
import torch
from torch import nn

import hard_vfe_fixture as HF

pytestmark = pytest.mark.gpu

TOL = 1e-4       # the project's feature tolerance, of the expected tensor's largest entry
MARGIN = 4.0
FLOOR = 1e-6
MAX_CHANNELS_OUT = 8
MAX_ZEROED = 0.01


def _steps_n():
    """More voxels than one pass of the persistent grid covers, and a partial last step."""
    from msmdfusion_amd import kernels as K
    return K.HARD_VFE_VOXELS_PER_STEP * K.HARD_VFE_BLOCKS + 3


# (N, M, C, widths, training, kind)
FORWARD = [
    (1, 20, 4, (64, 64), True, "mixed"),
    (1, 1, 4, (64, 64), False, "mixed"),
    (2, 1, 3, (32, 64), True, "mixed"),
    (2, 5, 5, (16,), True, "mixed"),
    (97, 5, 3, (64, 64), True, "mixed"),
    (97, 20, 4, (32, 64), False, "mixed"),
    (97, 64, 5, (64, 64), True, "mixed"),
    (97, 64, 4, (16,), False, "mixed"),
    (98, 20, 4, (64, 64), True, "one"),
    (98, 20, 4, (64, 64), True, "full"),
    (99, 20, 4, (64, 64), True, "exceed"),
    (99, 5, 4, (64, 64), True, "same"),
    (None, 20, 4, (64, 64), True, "mixed"),
    (None, 64, 5, (32, 64), False, "mixed"),
    (None, 5, 3, (16,), True, "mixed"),
]

GRAD_SHAPES = [(2, 3), (9, 5), (61, 8), (25, 20), (7, 64), (130, 4)]
# seeds of make_voxels per (layers, training), in GRAD_SHAPES order
GRAD_SEEDS = {
    (2, True): (11, 4, 4, 7, 6, 1),
    (2, False): (1, 5, 4, 7, 5, 6),
    (1, True): (1, 2, 1, 3, 6, 1),
    (1, False): (1, 3, 4, 3, 5, 1),
}
GRADS = [(layers, training, n, m, GRAD_SEEDS[(layers, training)][i])
         for layers in (2, 1) for training in (True, False)
         for i, (n, m) in enumerate(GRAD_SHAPES)]


def _layer_tuples(mod, dev):
    """[(W, scale, shift)] float32 with the running statistics folded in (kernel wrapper)."""
    out = []
    for vfe in mod.vfe_layers:
        bn = vfe.norm
        scale = bn.weight.detach().double() * torch.rsqrt(bn.running_var.double() + bn.eps)
        shift = bn.bias.detach().double() - bn.running_mean.double() * scale
        out.append((vfe.linear.weight.detach().float().contiguous(), scale.float(), shift.float()))
    return out


@pytest.mark.parametrize("tag", ["two_train", "two_eval", "one_train", "one_eval"])
def test_fused_matches_the_reference_outputs(dev, tag):
    mod, (feats, num, coors), arr = HF.golden_case(tag, dev)
    assert mod.fused_ok(feats)
    before = feats.clone()
    with torch.no_grad():
        out = mod(feats, num, coors)
    assert tuple(out.shape) == tuple(arr["out"].shape) and out.dtype == torch.float32
    err = HF.scaled_err(out, arr["out"])
    print("%s: scaled err %.3e" % (tag, err))
    assert err <= TOL
    assert torch.equal(feats, before), "the input was written"
    state = mod.state_dict()
    for k, v in arr.items():
        if not k.startswith("after."):
            continue
        if "num_batches" in k:
            assert int(state[k[6:]]) == int(v), k
        else:
            assert HF.scaled_err(state[k[6:]], v) <= TOL, k


@pytest.mark.parametrize("case", FORWARD, ids=lambda c: "N%s-M%d-C%d-%s-%s-%s" % (
    c[0] or "grid", c[1], c[2], "x".join(map(str, c[3])), "train" if c[4] else "eval", c[5]))
def test_forward_against_float64(dev, case):
    n, m, c, widths, training, kind = case
    n = n or _steps_n()
    mod = HF.encoder(dev, c, widths, training)
    inputs = HF.make_voxels(n, m, c, seed=n + m, device=dev, kind=kind)
    assert mod.fused_ok(inputs[0])
    ref = copy.deepcopy(mod)
    with torch.no_grad():
        y64 = HF.reference_sequence(mod, *inputs, torch.float64, HF.leaves(mod, torch.float64))
        y32 = HF.reference_sequence(mod, *inputs, torch.float32, HF.leaves(mod, torch.float32))
        out = mod(*inputs)
        ref.forward_composed(*inputs)
    assert tuple(out.shape) == (n, widths[-1])
    base, err = HF.scaled_err(y32, y64), HF.scaled_err(out, y64)
    print("fp32 torch %.3e  fused %.3e  ratio %.2f" % (base, err, err / max(base, 1e-30)))
    assert err <= max(MARGIN * base, FLOOR)
    for k, v in ref.state_dict().items():          # running statistics as nn.BatchNorm1d's
        if "running" in k:
            assert HF.scaled_err(mod.state_dict()[k], v) <= TOL, k
        elif "num_batches" in k:
            assert int(mod.state_dict()[k]) == int(v) == int(training)


def test_one_slot_training_raises_as_torch_does(dev):
    mod = HF.encoder(dev, 4, (64, 64), True)
    inputs = HF.make_voxels(1, 1, 4, seed=0, device=dev)
    with pytest.raises(ValueError, match="more than 1 value"):
        mod(*inputs)
    with pytest.raises(ValueError, match="more than 1 value"):
        mod.forward_composed(*inputs)


def test_exact_ties_go_to_the_smallest_slot(dev):
    """Identical points in a voxel: every valid slot ties exactly, so the argmax is slot 0 or
    the first padded slot (all padded slots tie as well)."""
    from msmdfusion_amd import kernels as K
    mod = HF.encoder(dev, 4, (64, 64), False)
    feats, num, coors = HF.make_voxels(200, 20, 4, seed=8, device=dev, kind="same")
    for layers in (_layer_tuples(mod, dev), _layer_tuples(mod, dev)[:1]):
        out, arg, _ = K.hard_vfe_forward(feats, num, coors, mod._geom, layers)
        first_padded = num.long().clamp(max=19)[:, None].expand_as(arg)
        assert bool(((arg == 0) | ((arg.long() == first_padded) & (num < 20)[:, None])).all())
        assert int((arg != 0).sum()) > 0 and int((arg == 0).sum()) > 0
        if len(layers) == 2:
            with torch.no_grad():
                assert HF.scaled_err(out, mod.forward_composed(feats, num, coors)) <= TOL


@pytest.mark.parametrize("training", [True, False])
def test_zero_rows_and_negative_gamma(dev, training):
    """A zero row in W1 and in W2 (zero variance: the output is relu(beta)), negative gamma."""
    mod = HF.encoder(dev, 4, (64, 64), training)
    with torch.no_grad():
        mod.vfe_layers[0].linear.weight[3].zero_()
        mod.vfe_layers[1].linear.weight[5].zero_()
        mod.vfe_layers[0].norm.weight[::3].neg_()
        mod.vfe_layers[1].norm.weight[1::4].neg_()
    inputs = HF.make_voxels(97, 20, 4, seed=11, device=dev)
    with torch.no_grad():
        y64 = HF.reference_sequence(mod, *inputs, torch.float64, HF.leaves(mod, torch.float64))
        y32 = HF.reference_sequence(mod, *inputs, torch.float32, HF.leaves(mod, torch.float32))
        out = mod(*inputs)
    assert torch.isfinite(out).all()
    base, err = HF.scaled_err(y32, y64), HF.scaled_err(out, y64)
    print("fp32 torch %.3e  fused %.3e" % (base, err))
    assert err <= max(MARGIN * base, FLOOR)
    if training:
        beta = mod.vfe_layers[1].norm.bias[5]
        assert torch.allclose(out[:, 5], torch.relu(beta).expand(97), atol=1e-6)


@pytest.mark.parametrize("case", GRADS, ids=lambda c: "L%d-%s-N%d-M%d" % (
    c[0], "train" if c[1] else "eval", c[2], c[3]))
def test_gradients_against_float64_autograd(dev, case):
    layers, training, n, m, seed = case
    widths = (64, 64)[:layers]
    mod = HF.encoder(dev, 4, widths, training, seed=9)
    inputs = HF.make_voxels(n, m, 4, seed=seed, device=dev)
    go = torch.randn((n, 64), generator=torch.Generator().manual_seed(n)).to(dev)
    go, zeroed, channels_out = HF.exclusions(mod, inputs, go)
    n_out = 0 if channels_out is None else int(channels_out.sum())
    print("grad_out entries zeroed %.3f %%, layer-1 channels left out %d" % (100 * zeroed, n_out))
    assert zeroed <= MAX_ZEROED and n_out <= MAX_CHANNELS_OUT
    y64, g64 = HF.reference_grads(mod, inputs, go, torch.float64)
    y32, g32 = HF.reference_grads(mod, inputs, go, torch.float32)
    deviation = HF.scaled_err(y32, y64)
    print("float32 composition forward deviation %.3e" % deviation)
    assert deviation < HF.TAU / 4
    mod.zero_grad()
    out = mod(*inputs)
    out.backward(go)
    base, err = deviation, HF.scaled_err(out, y64)
    assert err <= max(MARGIN * base, FLOOR), "out"
    names = ["dW1", "dgamma1", "dbeta1", "dW2", "dgamma2", "dbeta2"][:3 * layers]
    for i, (name, a, b32, b64) in enumerate(zip(names, HF.module_grads(mod), g32, g64)):
        if i < 3 and channels_out is not None:       # layer 1 of two: the kept rows
            keep = ~channels_out
            a, b32, b64 = a[keep], b32[keep], b64[keep]
        base, err = HF.scaled_err(b32, b64), HF.scaled_err(a, b64)
        print("%-8s fp32 autograd %.3e  fused %.3e" % (name, base, err))
        assert err <= max(MARGIN * base, FLOOR), name


def test_backward_sums_at_step_and_grid_boundaries(dev):
    """The raw sums of one call on more voxels than the grid covers in one pass equal the sums
    over calls on its consecutive chunks of at most 64 voxels, to fp64 rounding: per-voxel
    arithmetic is identical in both, so no decision can flip."""
    from msmdfusion_amd import kernels as K
    n, m = 4099, 64
    assert n > _steps_n() and n % K.HARD_VFE_VOXELS_PER_STEP
    mod = HF.encoder(dev, 4, (64, 64), False)
    feats, num, coors = HF.make_voxels(n, m, 4, seed=13, device=dev)
    layers = _layer_tuples(mod, dev)
    gen = torch.Generator().manual_seed(1)
    dp = (torch.randn(64, generator=gen) * 1e-3).to(dev)
    dq = (torch.randn(64, generator=gen) * 1e-3).to(dev)
    for ls, extra in ((layers, (dp, dq)), (layers[:1], ())):
        out, arg, _ = K.hard_vfe_forward(feats, num, coors, mod._geom, ls)
        g2 = (torch.randn((n, 64), generator=gen).to(dev) * (out > 0)).contiguous()
        whole = K.hard_vfe_backward(feats, num, coors, mod._geom, ls, g2, arg, *extra)
        parts = None
        for lo in range(0, n, 64):
            s = slice(lo, min(lo + 64, n))
            got = K.hard_vfe_backward(feats[s].contiguous(), num[s].contiguous(),
                                      coors[s].contiguous(), mod._geom, ls, g2[s].contiguous(),
                                      arg[s].contiguous(), *extra)
            got = [None if t is None else t.clone() for t in got]
            parts = got if parts is None else [None if a is None else a + b
                                               for a, b in zip(parts, got)]
        for name, a, b in zip(("dW2", "A1", "sg1"), whole, parts):
            if a is None:
                continue
            rel = float((a - b).abs().max() / b.abs().max())
            print("%s: whole against chunks, relative %.3e" % (name, rel))
            assert rel <= 1e-12 and float(b.abs().max()) > 0, name


def _run(dev, inputs, go, mod=None):
    mod = mod or HF.encoder(dev, 4, (64, 64), True)
    out = mod(*inputs)
    out.backward(go)
    return mod, [out.detach(), *HF.module_grads(mod),
                 *[b for vfe in mod.vfe_layers for b in (vfe.norm.running_mean,
                                                         vfe.norm.running_var)]]


def test_two_runs_give_the_same_bytes(dev):
    """Forward + backward at one sample of the config's training size."""
    inputs = HF.make_voxels(30000, 64, 4, seed=1, device=dev)
    go = torch.randn((30000, 64), device=dev)
    runs = [_run(dev, inputs, go)[1] for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.isfinite(runs[0][0]).all() and all(float(t.abs().sum()) > 0 for t in runs[0])


def test_fused_equals_composition_on_the_same_module(dev):
    for training, widths in ((True, (64, 64)), (False, (64, 64)), (True, (64,))):
        a = HF.encoder(dev, 4, widths, training)
        b = copy.deepcopy(a)
        inputs = HF.make_voxels(1000, 20, 4, seed=2, device=dev)
        with torch.no_grad():
            y64 = HF.reference_sequence(a, *inputs, torch.float64, HF.leaves(a, torch.float64))
            fused, comp = a(*inputs), b.forward_composed(*inputs)
        base, err = HF.scaled_err(comp, y64), HF.scaled_err(fused, y64)
        assert err <= max(MARGIN * base, FLOOR)
        assert HF.scaled_err(fused, comp) <= TOL
        for k, v in b.state_dict().items():
            if "running" in k:
                assert HF.scaled_err(a.state_dict()[k], v) <= TOL, k
            elif "num_batches" in k:
                assert int(a.state_dict()[k]) == int(v) == int(training)


class _OtherNorm(nn.BatchNorm1d):
    """Not a plain nn.BatchNorm1d (what a converted norm is to the encoder)."""


def test_fallbacks_take_the_composition_path(dev):
    from msmdfusion_amd import kernels as K
    inputs = HF.make_voxels(50, 20, 4, seed=3, device=dev)

    def composed_only(mod, ins):
        assert not mod.fused_ok(ins[0])
        with mock.patch.object(K, "hard_vfe_forward", side_effect=AssertionError("fused")):
            with torch.no_grad():
                y64 = HF.reference_sequence(mod, *ins, torch.float64,
                                            HF.leaves(mod, torch.float64))
                out = mod(*ins)
        assert HF.scaled_err(out, y64) <= TOL

    composed_only(HF.encoder(dev, 4, (32, 32, 64), True), inputs)            # three layers
    composed_only(HF.encoder(dev, 4, (128,), True), inputs)                  # too wide
    composed_only(HF.encoder(dev, 4, (64, 64), True),
                  HF.make_voxels(20, 65, 4, seed=3, device=dev))             # M > 64
    mod = HF.encoder(dev, 4, (64, 64), True)                                 # another norm class
    for vfe in mod.vfe_layers:
        other = _OtherNorm(64, eps=vfe.norm.eps, momentum=vfe.norm.momentum).to(dev)
        other.load_state_dict(vfe.norm.state_dict())
        vfe.norm = other
    composed_only(mod, inputs)
    mod = HF.encoder(dev, 4, (64, 64), True)                                 # cumulative average
    mod.vfe_layers[1].norm.momentum = None
    composed_only(mod, inputs)
    cpu = HF.encoder("cpu", 4, (64, 64), True)                               # CPU tensors
    composed_only(cpu, HF.make_voxels(50, 20, 4, seed=3))
    # an input that requires grad: it gets one
    mod = HF.encoder(dev, 4, (64, 64), True)
    feats = inputs[0].clone().requires_grad_(True)
    assert not mod.fused_ok(feats)
    mod(feats, *inputs[1:]).sum().backward()
    assert feats.grad is not None and float(feats.grad.abs().sum()) > 0
    # naiveSync in a multi-rank group: not its plain branch -> composition, which refuses
    mod = HF.encoder(dev, 4, (64, 64), True)
    with mock.patch("torch.distributed.is_initialized", return_value=True), \
            mock.patch("torch.distributed.get_world_size", return_value=2):
        assert not mod.fused_ok(inputs[0])
        with pytest.raises(NotImplementedError, match="all-reduce"):
            mod(*inputs)
        mod.eval()
        assert mod.fused_ok(inputs[0])
    assert HF.encoder(dev, 4, (64, 64), True, norm="BN1d").fused_ok(inputs[0])


def test_autocast_still_computes_in_float32(dev):
    mod, inputs, arr = HF.golden_case("two_eval", dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = mod(*inputs)
    assert out.dtype == torch.float32 and HF.scaled_err(out, arr["out"]) <= TOL


def test_no_host_synchronisation_and_no_activation_tensor(dev):
    """Forward + backward under the sync debug mode, and a peak below ONE [N, M, U] float
    tensor (the composition keeps several)."""
    n, m = 30000, 64
    inputs = HF.make_voxels(n, m, 4, seed=4, device=dev)
    go = torch.randn((n, 64), device=dev)
    mod = HF.encoder(dev, 4, (64, 64), True)
    _run(dev, inputs, go, mod)                        # warm: workspace, module load
    mod.zero_grad()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _run(dev, inputs, go, mod)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print("peak grew by %.1f MB; one [N, M, U] tensor is %.1f MB" % (grown / 2**20,
                                                                     n * m * 64 * 4 / 2**20))
    assert grown < n * m * 64 * 4


# ---------------------------------------------------------------- detectors
def _detector(dev, name):
    """The config on a 64 x 64 canvas: the range cut to +-8 m, the anchor ranges with it."""
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.registry import build_detector
    cfg = copy.deepcopy(getattr(C, name))
    pcr = [-8, -8, -5, 8, 8, 3]
    cfg["pts_voxel_layer"].update(point_cloud_range=pcr, max_voxels=(4096, 4096))
    cfg["pts_voxel_encoder"]["point_cloud_range"] = pcr
    cfg["pts_middle_encoder"]["output_shape"] = [64, 64]
    cfg["pts_bbox_head"]["anchor_generator"]["ranges"] = [[-8, -8, -1.8, 8, 8, -1.8]]
    torch.manual_seed(3)
    return build_detector(cfg).to(dev)


@pytest.mark.parametrize("name,head", [("POINTPILLARS_FPN_NUS", "Anchor3DHead"),
                                       ("FREE_ANCHOR_POINTPILLARS_FPN_NUS", "FreeAnchor3DHead")])
def test_mvx_faster_rcnn_trains_and_infers(dev, name, head):
    det = _detector(dev, name)
    assert type(det).__name__ == "MVXFasterRCNN" and type(det.pts_bbox_head).__name__ == head
    assert type(det.pts_voxel_encoder).__name__ == "HardVFE" and type(det.pts_neck).__name__ == "FPN"
    assert {k.split(".")[0] for k in det.state_dict()} == {
        "pts_voxel_encoder", "pts_backbone", "pts_neck", "pts_bbox_head"}
    keys = set(det.state_dict())
    assert {"pts_voxel_encoder.vfe_layers.1.linear.weight", "pts_voxel_encoder.vfe_layers.0.norm.bias",
            "pts_neck.lateral_convs.2.conv.weight", "pts_neck.fpn_convs.0.bn.running_mean",
            "pts_backbone.blocks.0.0.weight"} <= keys
    rs = np.random.RandomState(4)
    points = []
    for _ in range(2):
        p = rs.uniform(0, 1, (4000, 4)).astype(np.float32)
        p[:, :2] = -8 + p[:, :2] * 16 * 0.999
        p[:1000, :2] = p[:1000, :2] * 0.02 + 1.0         # a dense patch: pillars of many points
        p[:, 2] = rs.uniform(-2.5, 0.5, 4000)
        points.append(torch.from_numpy(p).to(dev))
    gt = [torch.tensor([[4.0, 1.0, -1.6, 1.9, 4.6, 1.7, 0.3, 0.5, 0.1],
                        [-3.0, -2.0, -1.0, 0.7, 0.7, 1.8, 1.0, 0.0, 0.0]], device=dev),
          torch.zeros((0, 9), device=dev)]
    labels = [torch.tensor([0, 8], device=dev), torch.zeros((0,), dtype=torch.long, device=dev)]
    det.train()
    voxels, _, _ = det.voxelize_table(points)
    assert voxels.shape[1:] == (64, 4) and det.pts_voxel_encoder.fused_ok(voxels)
    losses = det(points, return_loss=True, gt_bboxes_3d=gt, gt_labels_3d=labels)
    total = sum(sum(v) if isinstance(v, (list, tuple)) else v for v in losses.values())
    assert torch.isfinite(total)
    total.backward()
    missing = [k for k, p in det.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing[:5]
    assert all(torch.isfinite(p.grad).all() for p in det.parameters())
    assert float(det.pts_voxel_encoder.vfe_layers[0].linear.weight.grad.abs().sum()) > 0
    det.eval()
    with torch.no_grad():
        out = det.simple_test(points)
    assert len(out) == 2
    for r in out:
        k = r["scores_3d"].shape[0]
        assert r["boxes_3d"].shape == (k, 9) and r["labels_3d"].shape == (k,) and k <= 500
