"""SparseUNet (the Part-A2 middle encoder) on the MI355X: the reference's own structure and
shape test (tests/test_models/test_common_modules/test_sparse_unet.py:7-49), and a small
model in eval mode, forward and backward, against a dense float64 torch restatement in which
every sparse layer is its dense equivalent on a zero-filled grid read at the active cells
(SubM / strided conv: F.conv3d; inverse conv: F.conv_transpose3d)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_updown_ref as R
from msmdfusion_amd import spconv
from msmdfusion_amd.sparse_block import SparseBasicBlock
from msmdfusion_amd.sparse_unet import SparseUNet

pytestmark = pytest.mark.gpu


def test_sparse_unet_reference_structure_and_shapes(dev):
    self = SparseUNet(in_channels=4, sparse_shape=[41, 1600, 1408]).to(dev)
    assert len(self.encoder_layers) == 4
    assert self.encoder_layers.encoder_layer1[0][0].in_channels == 16
    assert self.encoder_layers.encoder_layer1[0][0].out_channels == 16
    assert isinstance(self.encoder_layers.encoder_layer1[0][0], spconv.conv.SubMConv3d)
    assert isinstance(self.encoder_layers.encoder_layer1[0][1], torch.nn.modules.batchnorm.BatchNorm1d)
    assert isinstance(self.encoder_layers.encoder_layer1[0][2], torch.nn.modules.activation.ReLU)
    assert self.encoder_layers.encoder_layer4[0][0].in_channels == 64
    assert self.encoder_layers.encoder_layer4[0][0].out_channels == 64
    assert isinstance(self.encoder_layers.encoder_layer4[0][0], spconv.conv.SparseConv3d)
    assert isinstance(self.encoder_layers.encoder_layer4[2][0], spconv.conv.SubMConv3d)
    assert isinstance(self.lateral_layer1, SparseBasicBlock)
    assert isinstance(self.merge_layer1[0], spconv.conv.SubMConv3d)
    assert isinstance(self.upsample_layer1[0], spconv.conv.SubMConv3d)
    assert isinstance(self.upsample_layer2[0], spconv.conv.SparseInverseConv3d)

    voxel_features = torch.tensor([[6.56126, 0.9648336, -1.7339306, 0.315],
                                   [6.8162713, -2.480431, -1.3616394, 0.36],
                                   [11.643568, -4.744306, -1.3580885, 0.16],
                                   [23.482342, 6.5036807, 0.5806964, 0.35]],
                                  dtype=torch.float32, device=dev)
    coordinates = torch.tensor([[0, 12, 819, 131], [0, 16, 750, 136], [1, 16, 705, 232],
                                [1, 35, 930, 469]], dtype=torch.int32, device=dev)
    unet_ret_dict = self.forward(voxel_features, coordinates, 2)
    assert unet_ret_dict["seg_features"].shape == torch.Size([4, 16])
    assert unet_ret_dict["spatial_features"].shape == torch.Size([2, 256, 200, 176])


# ---------------------------------------------------------------- dense restatement
class _Dense:
    """Dense float64 twin of a SparseUNet: parameters copied as leaves (grads by name)."""

    def __init__(self, model):
        self.p = {n: v.detach().cpu().double().requires_grad_() for n, v in
                  model.named_parameters()}
        self.b = {n: v.detach().cpu().double() for n, v in model.named_buffers()}
        self.names = {id(m): n for n, m in model.named_modules()}
        self.couples = {}

    def conv(self, layer, x, mask):
        w = self.p[self.names[id(layer)] + ".weight"]
        if isinstance(layer, spconv.SparseInverseConv3d):
            mask_out, shape, stride, padding = self.couples[layer.indice_key]
            ks = layer.kernel_size
            extra = [shape[i] - ((x.shape[2 + i] - 1) * stride[i] - 2 * padding[i] + ks[i])
                     for i in range(3)]
            y = F.conv_transpose3d(x, w.permute(4, 0, 1, 2, 3), stride=stride, padding=padding,
                                   output_padding=extra)
        elif layer.subm:
            y, mask_out = F.conv3d(x, w.permute(0, 4, 1, 2, 3),
                                   padding=[k // 2 for k in layer.kernel_size]), mask
        else:
            y = F.conv3d(x, w.permute(0, 4, 1, 2, 3), stride=layer.stride, padding=layer.padding)
            ones = torch.ones((1, 1, *layer.kernel_size), dtype=torch.float64)
            mask_out = F.conv3d(mask, ones, stride=layer.stride, padding=layer.padding) > 0
            mask_out = mask_out.double()
            if layer.indice_key is not None:
                self.couples[layer.indice_key] = (mask, list(x.shape[2:]), layer.stride,
                                                  layer.padding)
        return y * mask_out, mask_out

    def bn(self, layer, x, mask):
        n = self.names[id(layer)]
        shape = (1, -1, 1, 1, 1)
        y = (x - self.b[n + ".running_mean"].view(shape)) / torch.sqrt(
            self.b[n + ".running_var"].view(shape) + layer.eps)
        return (y * self.p[n + ".weight"].view(shape) + self.p[n + ".bias"].view(shape)) * mask

    def seq(self, block, x, mask):
        for child in block:
            if isinstance(child, spconv.SparseConvolution):
                x, mask = self.conv(child, x, mask)
            elif isinstance(child, torch.nn.BatchNorm1d):
                x = self.bn(child, x, mask)
            elif isinstance(child, torch.nn.ReLU):
                x = torch.relu(x)
            elif isinstance(child, spconv.SparseSequential):
                x, mask = self.seq(child, x, mask)
            else:
                raise TypeError(type(child))
        return x, mask

    def basic(self, block, x, mask):
        out, _ = self.conv(block.conv1, x, mask)
        out = torch.relu(self.bn(block.bn1, out, mask))
        out, _ = self.conv(block.conv2, out, mask)
        return torch.relu(self.bn(block.bn2, out, mask) + x), mask

    def forward(self, model, x, mask):
        x, mask = self.seq(model.conv_input, x, mask)
        enc = []
        for layer in model.encoder_layers:
            x, mask = self.seq(layer, x, mask)
            enc.append((x, mask))
        out, _ = self.seq(model.conv_out, *enc[-1])
        n, c, d, h, w = out.shape
        spatial = out.reshape(n, c * d, h, w)
        x, mask = enc[-1]
        for i in range(model.stage_num, 0, -1):
            lat, lmask = enc[i - 1]
            y, _ = self.basic(getattr(model, f"lateral_layer{i}"), lat, lmask)
            y = torch.cat((x, y), 1)
            merged, _ = self.seq(getattr(model, f"merge_layer{i}"), y, lmask)
            y = y.reshape(n, merged.shape[1], -1, *y.shape[2:]).sum(2)
            x, mask = self.seq(getattr(model, f"upsample_layer{i}"), merged + y, lmask)
        return spatial, x, mask


def _scaled_close(got, exp, name):
    got, exp = got.detach().cpu().double(), exp.detach().cpu().double()
    assert got.shape == exp.shape, name
    scale = max(1.0, float(exp.abs().max())) if exp.numel() else 1.0
    err = float((got - exp).abs().max()) if exp.numel() else 0.0
    assert err <= 1e-4 * scale, "%s: max error %.3g at scale %.3g" % (name, err, scale)


def test_sparse_unet_matches_dense_restatement(dev):
    torch.manual_seed(0)
    shape, batch = [25, 32, 32], 2
    model = SparseUNet(4, shape).to(dev)
    with torch.no_grad():       # non-trivial running statistics and affine parameters
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
    model.eval()
    rng = np.random.RandomState(3)
    idx = R.random_voxels(rng, batch, shape, 700)
    feats = rng.randn(idx.shape[0], 4).astype(np.float32)
    coors = torch.from_numpy(idx).to(dev)
    vf = torch.from_numpy(feats).to(dev).requires_grad_()
    ret = model(vf, coors, batch)
    g_spatial = torch.randn(ret["spatial_features"].shape, device=dev)
    g_seg = torch.randn(ret["seg_features"].shape, device=dev)
    ((ret["spatial_features"] * g_spatial).sum() + (ret["seg_features"] * g_seg).sum()).backward()

    dense = _Dense(model)
    x = torch.zeros((batch, 4, *shape), dtype=torch.float64)
    mask = torch.zeros((batch, 1, *shape), dtype=torch.float64)
    b, z, y, xx = (torch.from_numpy(idx[:, i]).long() for i in range(4))
    xin = torch.from_numpy(feats).double().requires_grad_()
    x[b, :, z, y, xx] = xin
    mask[b, 0, z, y, xx] = 1.0
    spatial, out, out_mask = dense.forward(model, x, mask)
    assert bool((out_mask[b, 0, z, y, xx] == 1).all()) and int(out_mask.sum()) == idx.shape[0]
    seg = out[b, :, z, y, xx]
    _scaled_close(ret["spatial_features"], spatial, "spatial_features")
    _scaled_close(ret["seg_features"], seg, "seg_features")
    ((spatial * g_spatial.cpu().double()).sum() + (seg * g_seg.cpu().double()).sum()).backward()
    _scaled_close(vf.grad, xin.grad, "voxel_features.grad")
    for name, p in model.named_parameters():
        _scaled_close(p.grad, dense.p[name].grad, name + ".grad")
