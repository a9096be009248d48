"""Transposed / inverse sparse convs, sparse max-pool and SparseUNet without a GPU: constructor
arithmetic, CONV_LAYERS look-ups, state-dict keys and shapes against the reference's module
names, deconv_output_size, and the numpy transposed-geometry restatement the GPU tests use,
itself checked against the support of F.conv_transpose3d."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_updown_ref as R
from msmdfusion_amd import kernels as K
from msmdfusion_amd import spconv
from msmdfusion_amd.registry import CONV_LAYERS, MIDDLE_ENCODERS, build_conv_layer
from msmdfusion_amd.sparse_block import make_sparse_convmodule


def test_conv_layers_registry_and_constructors():
    t = build_conv_layer(dict(type="SparseConvTranspose3d", indice_key="up"), 16, 32, 3,
                         stride=2, padding=1, bias=False)
    assert isinstance(t, spconv.SparseConvTranspose3d) and CONV_LAYERS.get("SparseConvTranspose3d")
    assert t.transposed and not t.inverse and not t.subm
    assert t.stride == [2, 2, 2] and t.padding == [1, 1, 1] and t.output_padding == [0, 0, 0]
    assert tuple(t.weight.shape) == (32, 3, 3, 3, 16) and t.bias is None
    i = build_conv_layer(dict(type="SparseInverseConv3d", indice_key="d"), 32, 16, (3, 1, 1))
    assert isinstance(i, spconv.SparseInverseConv3d) and i.inverse and not i.transposed
    assert i.kernel_size == [3, 1, 1] and tuple(i.weight.shape) == (16, 3, 1, 1, 32)
    assert i.bias is not None and i.indice_key == "d"
    # an inverse 1x1x1 conv still restores its couple's voxel set
    assert not spconv.SparseInverseConv3d(8, 8, 1, indice_key="d").conv1x1
    m = make_sparse_convmodule(32, 16, 3, indice_key="d", stride=2, padding=1,
                               conv_type="SparseInverseConv3d", norm_cfg=dict(type="BN1d"))
    assert isinstance(m[0], spconv.SparseInverseConv3d) and m[0].stride == [1, 1, 1]
    assert list(m.state_dict()) == ["0.weight", "1.weight", "1.bias", "1.running_mean",
                                    "1.running_var", "1.num_batches_tracked"]
    with pytest.raises(ValueError):
        spconv.SparseConvolution(3, 4, 4, 3, subm=True, transposed=True)
    with pytest.raises(ValueError):
        spconv.SparseConvolution(3, 4, 4, 3, subm=True, inverse=True)
    with pytest.raises(TypeError):      # the reference's signature: indice_key is required
        spconv.SparseInverseConv3d(4, 4, 3)


def test_maxpool_constructor():
    p = spconv.SparseMaxPool3d(3)
    assert p.kernel_size == [3, 3, 3] and p.stride == [1, 1, 1] and p.padding == [0, 0, 0]
    assert p.dilation == [1, 1, 1] and p.indice_key is None and not p.subm
    p = spconv.SparseMaxPool3d((3, 1, 1), (2, 1, 1), 1, indice_key="p", algo=2)
    assert p.kernel_size == [3, 1, 1] and p.stride == [2, 1, 1] and p.padding == [1, 1, 1]
    assert not list(p.state_dict())
    with pytest.raises(NotImplementedError):
        spconv.SparseMaxPool(3, 3, subm=True)
    block = spconv.SparseSequential(spconv.SubMConv3d(4, 4, 3), p,
                                    spconv.SparseInverseConv3d(4, 4, (3, 1, 1), indice_key="p"))
    assert [type(m) for m in spconv.sparse_convs(block)] == [
        spconv.SubMConv3d, spconv.SparseMaxPool3d, spconv.SparseInverseConv3d]


def test_deconv_output_size():
    assert K.deconv_output_size([41, 1600, 1408], 3, 2, 1) == [81, 3199, 2815]
    assert K.deconv_output_size([5, 6, 7], [2, 2, 2], [2, 2, 2], 0, 1) == [11, 13, 15]
    assert K.deconv_output_size([5, 6, 7], [3, 1, 1], [2, 1, 1], 0) == [11, 6, 7]
    for ins, ks, st, pd, op in [([5, 6, 7], [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1]),
                                ([4, 4, 4], [2, 3, 1], [2, 1, 3], [0, 1, 0], [0, 0, 2])]:
        x = torch.zeros((1, 1, *ins))
        w = torch.zeros((1, 1, *ks))
        y = F.conv_transpose3d(x, w, stride=st, padding=pd, output_padding=op)
        assert list(y.shape[2:]) == K.deconv_output_size(ins, ks, st, pd, op)
        assert R.deconv_output_size(ins, ks, st, pd, op) == list(y.shape[2:])


@pytest.mark.parametrize("ks,st,pd,op", [([3, 3, 3], [2, 2, 2], [1, 1, 1], [0, 0, 0]),
                                         ([2, 2, 2], [2, 2, 2], [0, 0, 0], [0, 0, 0]),
                                         ([3, 3, 3], [1, 1, 1], [1, 1, 1], [0, 0, 0]),
                                         ([3, 1, 1], [2, 1, 1], [0, 0, 0], [0, 0, 0]),
                                         ([3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1])])
def test_numpy_transposed_geometry_matches_conv_transpose3d(ks, st, pd, op):
    """Every pair of the restatement is a (input, offset, output) term of F.conv_transpose3d
    over an indicator grid, and nothing else: each offset k gets its own one-hot weight."""
    shape = [5, 7, 6]
    rng = np.random.RandomState(0)
    idx = R.random_voxels(rng, 1, shape, 40)
    out_shape = R.deconv_output_size(shape, ks, st, pd, op)
    oi, pairs, num = R.deconv_pairs(idx, out_shape, ks, st, pd)
    kvol = int(np.prod(ks))
    n = idx.shape[0]
    # channel j of the input = indicator of voxel j; output channel k = offset k
    x = torch.zeros((1, n, *shape), dtype=torch.float64)
    x[0, np.arange(n), idx[:, 1], idx[:, 2], idx[:, 3]] = 1.0
    for k in range(kvol):
        w = torch.zeros((n, n, *ks), dtype=torch.float64)
        kz, rem = divmod(k, ks[1] * ks[2])
        ky, kx = divmod(rem, ks[2])
        w[np.arange(n), np.arange(n), kz, ky, kx] = 1.0
        y = F.conv_transpose3d(x, w, stride=st, padding=pd, output_padding=op)[0]
        j, z, yy, xx = (a.numpy() for a in torch.nonzero(y, as_tuple=True))
        dense_pairs = sorted(zip(j.tolist(), zip(z.tolist(), yy.tolist(), xx.tolist())))
        p = int(num[k])
        mine = sorted((int(i), tuple(int(v) for v in oi[o, 1:]))
                      for i, o in zip(pairs[k, 0, :p], pairs[k, 1, :p]))
        assert mine == dense_pairs
    assert np.unique(oi, axis=0).shape[0] == oi.shape[0]


def _reference_unet_keys(model_cfg):
    """The state-dict names of the reference's SparseUNet, restated from its constructor
    (sparse_unet.py:44-302, make_sparse_convmodule -> '0' conv / '1' BN, SparseBasicBlock ->
    conv1 / bn1 / conv2 / bn2) with the KRSC conv weight shapes."""
    bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    keys = {}

    def module(prefix, cin, cout, ks=(3, 3, 3)):
        keys[prefix + ".0.weight"] = (cout, *ks, cin)
        for b in bn:
            keys[prefix + ".1." + b] = (cout,) if b != "num_batches_tracked" else ()

    module("conv_input", 4, 16)
    cin = 16
    for i, blocks in enumerate(((16,), (32, 32, 32), (64, 64, 64), (64, 64, 64))):
        for j, cout in enumerate(blocks):
            module("encoder_layers.encoder_layer%d.%d" % (i + 1, j), cin, cout)
            cin = cout
    for i, ch in enumerate(((64, 64, 64), (64, 64, 32), (32, 32, 16), (16, 16, 16))):
        lvl = 4 - i
        p = "lateral_layer%d" % lvl
        keys[p + ".conv1.weight"] = (ch[0], 3, 3, 3, cin)
        keys[p + ".conv2.weight"] = (ch[0], 3, 3, 3, ch[0])
        for n in ("bn1", "bn2"):
            for b in bn:
                keys["%s.%s.%s" % (p, n, b)] = (ch[0],) if b != "num_batches_tracked" else ()
        module("merge_layer%d" % lvl, cin * 2, ch[1])
        module("upsample_layer%d" % lvl, cin, ch[2])
        cin = ch[2]
    module("conv_out", 64, 128, (3, 1, 1))
    return keys


def test_sparse_unet_state_dict_matches_the_reference_names():
    from msmdfusion_amd.sparse_unet import SparseUNet
    model = MIDDLE_ENCODERS.build(dict(type="SparseUNet", in_channels=4,
                                       sparse_shape=[41, 1600, 1408]))
    assert isinstance(model, SparseUNet)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert got == _reference_unet_keys(None)
    assert isinstance(model.upsample_layer4[0], spconv.SparseInverseConv3d)
    assert model.upsample_layer4[0].indice_key == "spconv4"
    assert isinstance(model.upsample_layer1[0], spconv.SubMConv3d)
    assert model.conv_out[0].stride == [2, 1, 1] and model.conv_out[0].indice_key == "spconv_down2"
    x = spconv.SparseConvTensor(torch.zeros((3, 16)), torch.zeros((3, 4), dtype=torch.int32),
                                [4, 4, 4], 1)
    x = SparseUNet.reduce_channel(x, 8)
    assert tuple(x.features.shape) == (3, 8)
