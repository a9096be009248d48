"""Transposed and inverse sparse convs and sparse max-pool on the MI355X: the transposed
rulebook (csrc/rulebook.hip, msmd_rulebook_deconv3d_*) against a numpy restatement of the
reference's geometry, the convs against the oracle's indice_conv (inverse included), the
max-pool kernels (csrc/pool.hip) bitwise against the reference's functors, the
sparse_conv_ext shim, and the index pre-pass (SparseConvTensor.plan) over the new layers."""
import numpy as np
import pytest
import torch

import sparse_updown_ref as R
from msmdfusion_amd import kernels as K
from msmdfusion_amd import spconv
from msmdfusion_amd.integration import sparse_conv_ext as ext
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GEOMS = [  # ksize, stride, padding, output_padding
    ([3, 3, 3], [2, 2, 2], [1, 1, 1], [0, 0, 0]),
    ([2, 2, 2], [2, 2, 2], [0, 0, 0], [0, 0, 0]),
    ([3, 3, 3], [1, 1, 1], [1, 1, 1], [0, 0, 0]),
    ([3, 1, 1], [2, 1, 1], [0, 0, 0], [0, 0, 0]),
    ([3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1]),
]
SHAPE = [7, 12, 10]


def _np(x):
    return x.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _tables(can, n_in, n_out):
    fwd = O.nbr_table_from_pairs(can, n_out)
    bwd = np.full((len(can), n_in), -1, np.int32)
    for k, po in enumerate(can):
        bwd[k, po[:, 0]] = po[:, 1]
    return fwd, bwd


def _check_deconv(dev, idx, batch, ks, st, pd, op, shape=SHAPE, need_bwd=True):
    out_shape = R.deconv_output_size(shape, ks, st, pd, op)
    oi, pr, nm = R.deconv_pairs(idx, out_shape, ks, st, pd)
    coi, can, _ = O.canonical_rulebook(oi, pr, nm, out_shape)
    d_idx = torch.from_numpy(np.ascontiguousarray(idx, np.int32).reshape(-1, 4)).to(dev)
    out_idx, nbr_fwd, nbr_bwd, got_shape = K.rulebook_deconv(d_idx, batch, shape, ks, st, pd, op,
                                                             need_bwd=need_bwd)
    assert list(got_shape) == out_shape
    assert np.array_equal(_np(out_idx), coi.reshape(-1, 4))
    fwd, bwd = _tables(can, idx.shape[0], coi.shape[0])
    assert np.array_equal(_np(nbr_fwd), fwd)
    if need_bwd:
        assert np.array_equal(_np(nbr_bwd), bwd)
    else:
        assert nbr_bwd is None
    # reference-format pairs through the shim
    ids, pairs, num = ext.get_indice_pairs_3d(d_idx, batch, out_shape, shape, ks, st, pd,
                                              [1, 1, 1], op, 0, 1)
    assert np.array_equal(_np(ids), coi.reshape(-1, 4))
    got, gnum = _np(pairs), _np(num)
    for k in range(len(can)):
        assert gnum[k] == can[k].shape[0]
        assert np.array_equal(got[k, :, :gnum[k]].T, can[k])
        assert (got[k, :, gnum[k]:] == -1).all()
    return coi


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("ks,st,pd,op", GEOMS)
def test_transposed_rulebook(dev, batch, ks, st, pd, op):
    rng = np.random.RandomState(7 + batch)
    idx = R.random_voxels(rng, batch, SHAPE, 90)
    coi = _check_deconv(dev, idx, batch, ks, st, pd, op)
    assert coi.shape[0] > 0


def test_transposed_rulebook_edges(dev):
    ks, st, pd, op = [3, 3, 3], [2, 2, 2], [1, 1, 1], [0, 0, 0]
    # empty input
    coi = _check_deconv(dev, np.zeros((0, 4), np.int32), 2, ks, st, pd, op)
    assert coi.shape[0] == 0
    # a voxel in the far corner (and one in the near corner), batch 2
    far = np.array([[1, SHAPE[0] - 1, SHAPE[1] - 1, SHAPE[2] - 1], [0, 0, 0, 0]], np.int32)
    _check_deconv(dev, far, 2, ks, st, pd, op)
    _check_deconv(dev, far, 2, [2, 2, 2], [2, 2, 2], [0, 0, 0], [1, 1, 1])
    # every output outside the grid: k1 s1 p2 shrinks the grid by 2 on each side
    out = np.array([[0, 0, 0, 0], [0, 1, 1, 1], [0, 6, 11, 9], [0, 0, 5, 5]], np.int32)
    coi = _check_deconv(dev, out, 1, [1, 1, 1], [1, 1, 1], [2, 2, 2], [0, 0, 0])
    assert coi.shape[0] == 0
    # without the backward table: a filled and an empty input
    small = [4, 6, 6]
    some = R.random_voxels(np.random.RandomState(3), 2, small, 30)
    assert _check_deconv(dev, some, 2, ks, st, pd, op, small, need_bwd=False).shape[0] > 0
    coi = _check_deconv(dev, np.zeros((0, 4), np.int32), 2, ks, st, pd, op, small, need_bwd=False)
    assert coi.shape[0] == 0


def _transposed_case(dev, c, seed=3):
    rng = np.random.RandomState(seed)
    idx = R.random_voxels(rng, 2, SHAPE, 120)
    return rng, idx, torch.from_numpy(idx).to(dev)


@pytest.mark.parametrize("c", [16, 64, 128])
@pytest.mark.parametrize("ks,st,pd", [([3, 3, 3], [2, 2, 2], [1, 1, 1]),
                                      ([2, 2, 2], [2, 2, 2], [0, 0, 0])])
def test_transposed_conv_matches_oracle(dev, c, ks, st, pd):
    rng, idx, d_idx = _transposed_case(dev, c)
    conv = spconv.SparseConvTranspose3d(c, c, ks, st, pd, bias=False).to(dev)
    f = rng.randn(idx.shape[0], c).astype(np.float32)
    fd = torch.from_numpy(f).to(dev).requires_grad_()
    x = spconv.SparseConvTensor(fd, d_idx, SHAPE, 2)
    y = conv(x)
    out_shape = R.deconv_output_size(SHAPE, ks, st, pd)
    assert y.spatial_shape == out_shape
    rb = x.cached_rulebook(ks, st, pd, [1, 1, 1], False, transposed=True)
    pairs, num = (_np(t) for t in rb.pairs())
    kvol = int(np.prod(ks))
    wk = _np(conv.weight).reshape(c, kvol, c).transpose(1, 2, 0).copy()
    exp = O.indice_conv_fwd(f, wk, pairs, num, rb.n_out)
    np.testing.assert_allclose(_np(y.features), exp, rtol=1e-4, atol=1e-4)
    g = rng.randn(rb.n_out, c).astype(np.float32)
    y.features.backward(torch.from_numpy(g).to(dev))
    edin, edw = O.indice_conv_bwd(f, wk, g, pairs, num)
    np.testing.assert_allclose(_np(fd.grad), edin, rtol=1e-4, atol=1e-4)
    dw = _np(conv.weight.grad).reshape(c, kvol, c).transpose(1, 2, 0)
    np.testing.assert_allclose(dw, edw, rtol=1e-4, atol=5e-4)


def _couple(kind, cin, cmid):
    if kind == "conv":
        return spconv.SparseConv3d(cin, cmid, 3, 2, 1, bias=False, indice_key="d")
    return spconv.SparseMaxPool3d(3, 2, 1, indice_key="d")


@pytest.mark.parametrize("kind", ["conv", "pool"])
@pytest.mark.parametrize("c", [16, 64])
def test_inverse_conv_matches_oracle(dev, kind, c):
    rng = np.random.RandomState(11)
    idx = R.random_voxels(rng, 2, SHAPE, 150)
    d_idx = torch.from_numpy(idx).to(dev)
    couple = _couple(kind, c, c).to(dev)
    inv = spconv.SparseInverseConv3d(c, c, 3, indice_key="d", bias=False).to(dev)
    x = spconv.SparseConvTensor(torch.from_numpy(rng.randn(idx.shape[0], c).astype(np.float32))
                                .to(dev), d_idx, SHAPE, 2)
    with torch.no_grad():
        mid = couple(x)
    m = rng.randn(mid.features.shape[0], c).astype(np.float32)
    md = torch.from_numpy(m).to(dev).requires_grad_()
    y = inv(mid.replace_feature(md))
    assert y.indices is d_idx
    assert y.spatial_shape == SHAPE
    rb = mid.indice_dict["d"]
    pairs, num = (_np(t) for t in rb.pairs())
    wk = _np(inv.weight).reshape(c, 27, c).transpose(1, 2, 0).copy()
    exp = O.indice_conv_fwd(m, wk, pairs, num, idx.shape[0], inverse=True)
    np.testing.assert_allclose(_np(y.features), exp, rtol=1e-4, atol=1e-4)
    g = rng.randn(idx.shape[0], c).astype(np.float32)
    y.features.backward(torch.from_numpy(g).to(dev))
    edin, edw = O.indice_conv_bwd(m, wk, g, pairs, num, inverse=True)
    np.testing.assert_allclose(_np(md.grad), edin, rtol=1e-4, atol=1e-4)
    dw = _np(inv.weight.grad).reshape(c, 27, c).transpose(1, 2, 0)
    np.testing.assert_allclose(dw, edw, rtol=1e-4, atol=5e-4)
    assert rb.inverted() is rb.inverted()


def test_inverse_conv_assertions(dev):
    rng = np.random.RandomState(2)
    idx = R.random_voxels(rng, 1, SHAPE, 60)
    x = spconv.SparseConvTensor(torch.randn(idx.shape[0], 16, device=dev),
                                torch.from_numpy(idx).to(dev), SHAPE, 1)
    with torch.no_grad():
        with pytest.raises(AssertionError):
            spconv.SparseInverseConv3d(16, 16, 3, indice_key="none").to(dev)(x)
        s = spconv.SubMConv3d(16, 16, 3, indice_key="s").to(dev)(x)
        with pytest.raises(AssertionError, match="standard conv and pool"):
            spconv.SparseInverseConv3d(16, 16, 3, indice_key="s").to(dev)(s)
        d = spconv.SparseConv3d(16, 16, 3, 2, 1, indice_key="d").to(dev)(x)
        with pytest.raises(AssertionError, match="same kernel size"):
            spconv.SparseInverseConv3d(16, 16, 2, indice_key="d").to(dev)(d)


def _pool_case(rng, idx, c, kind):
    n = idx.shape[0]
    f = (rng.randint(-4, 5, size=(n, c)) / 2.0).astype(np.float32)      # ties
    if kind == "negative":
        f = -np.abs(f) - 0.5
    if kind == "nan":
        f[rng.rand(n, c) < 0.1] = np.nan
    return f


@pytest.mark.parametrize("c", [1, 16, 64, 129])
@pytest.mark.parametrize("kind", ["ties", "negative", "nan", "repeated"])
def test_maxpool_bitwise(dev, c, kind):
    rng = np.random.RandomState(c + len(kind))
    idx = R.random_voxels(rng, 2, SHAPE, 140)
    if kind == "repeated":      # repeated coordinates: every row counts
        idx = np.concatenate([idx, idx[:30], idx[5:15]])
    f = _pool_case(rng, idx, c, kind)
    ks, st, pd = [3, 3, 3], [2, 2, 2], [1, 1, 1]
    oi, pr, nm, osz = O.get_indice_pairs(idx, 2, SHAPE, ks, st, pd, 1, False,
                                         use_ref=O.have_ref())
    coi, _, perm = O.canonical_rulebook(oi, pr, nm, osz)
    exp = R.maxpool_fwd(f, pr, nm, oi.shape[0])
    d_idx = torch.from_numpy(idx).to(dev)
    out_idx, _, nbr_bwd, _ = K.rulebook_conv(d_idx, 2, SHAPE, ks, st, pd)
    assert np.array_equal(_np(out_idx), coi)
    fd = torch.from_numpy(f).to(dev)
    out = K.maxpool_fwd(fd, nbr_bwd, out_idx.shape[0])
    assert np.array_equal(_bits(_np(out)), _bits(exp[perm]))
    if kind == "negative":
        assert not _np(out).any()
    g = rng.randn(out_idx.shape[0], c).astype(np.float32)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    edin = R.maxpool_bwd(f, exp, g[inv], pr, nm)
    din = K.maxpool_bwd(fd, out, torch.from_numpy(g).to(dev), nbr_bwd)
    assert np.array_equal(_bits(_np(din)), _bits(edin))
    # the module: same values, same gradient, through autograd
    fr = fd.clone().requires_grad_()
    y = spconv.SparseMaxPool3d(ks, st, pd)(spconv.SparseConvTensor(fr, d_idx, SHAPE, 2))
    assert y.spatial_shape == osz and torch.equal(y.indices, out_idx)
    assert torch.equal(y.features, out)
    y.features.backward(torch.from_numpy(g).to(dev))
    assert torch.equal(fr.grad, din)


def test_maxpool_reproducible_at_stress_size(dev):
    from msmdfusion_amd import synthetic as S
    pts = torch.from_numpy(np.concatenate([S.lidar_sweep(10 + i, sweeps=10) for i in range(2)]))
    vs = [0.05, 0.05, 0.2]
    coors = K.dynamic_voxelize(pts.to(dev), vs, S.POINT_CLOUD_RANGE)
    coors = torch.unique(coors[(coors >= 0).all(1)], dim=0)
    idx = torch.nn.functional.pad(coors, (1, 0)).int().contiguous()
    shape = [int(coors[:, i].max()) + 1 for i in range(3)]
    out_idx, _, nbr_bwd, _ = K.rulebook_conv(idx, 1, shape, 3, 2, 1)
    n_out = out_idx.shape[0]
    f = torch.randn((idx.shape[0], 64), device=dev)
    a = K.maxpool_fwd(f, nbr_bwd, n_out)
    b = K.maxpool_fwd(f, nbr_bwd, n_out)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    g = torch.randn_like(a)
    da = K.maxpool_bwd(f, a, g, nbr_bwd)
    db = K.maxpool_bwd(f, a, g, nbr_bwd)
    assert torch.equal(da.view(torch.int32), db.view(torch.int32))


def test_shim_transposed_and_inverse(dev):
    rng = np.random.RandomState(5)
    idx = R.random_voxels(rng, 2, SHAPE, 100)
    d_idx = torch.from_numpy(idx).to(dev)
    ks, st, pd = [3, 3, 3], [2, 2, 2], [1, 1, 1]
    osz = O.conv_output_size(SHAPE, ks, st, pd, [1, 1, 1])
    with pytest.raises(RuntimeError):       # the non-transposed outShape
        ext.get_indice_pairs_3d(d_idx, 2, osz, SHAPE, ks, st, pd, [1, 1, 1], [0, 0, 0], 0, 1)
    with pytest.raises(RuntimeError):
        ext.get_indice_pairs_3d(d_idx, 2, SHAPE, SHAPE, ks, [1, 1, 1], [1, 1, 1], [1, 1, 1],
                                [0, 0, 0], 1, 1)
    # inverse conv over a strided rulebook, cached-table and generic-pairs routes
    out_ids, pairs, num = ext.get_indice_pairs_3d(d_idx, 2, osz, SHAPE, ks, st, pd, [1, 1, 1],
                                                  [0, 0, 0], 0, 0)
    n_in, n_out = idx.shape[0], out_ids.shape[0]
    c_in, c_out = 32, 16
    m = rng.randn(n_out, c_in).astype(np.float32)
    w = (rng.randn(*ks, c_in, c_out) / np.sqrt(27 * c_in)).astype(np.float32)
    g = rng.randn(n_in, c_out).astype(np.float32)
    wk = w.reshape(27, c_in, c_out)
    pr, nm = _np(pairs), _np(num)
    exp = O.indice_conv_fwd(m, wk, pr, nm, n_in, inverse=True)
    edin, edw = O.indice_conv_bwd(m, wk, g, pr, nm, inverse=True)
    md, wd, gd = (torch.from_numpy(a).to(dev) for a in (m, w, g))
    for p in (pairs, pairs.clone()):
        out = ext.indice_conv_fp32(md, wd, p, num, n_in, 1, 0)
        np.testing.assert_allclose(_np(out), exp, rtol=1e-4, atol=1e-4)
        d_in, d_w = ext.indice_conv_backward_fp32(md, wd, gd, p, num, 1, 0)
        assert d_w.shape == wd.shape
        np.testing.assert_allclose(_np(d_in), edin, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(_np(d_w).reshape(wk.shape), edw, rtol=1e-4, atol=5e-4)
    with pytest.raises(RuntimeError):
        ext.indice_maxpool_fp32(md, pairs, num, n_out)


def _mixed_block():
    return spconv.SparseSequential(
        spconv.SubMConv3d(16, 16, 3, indice_key="s1"),
        spconv.SparseConv3d(16, 32, 3, 2, 1, indice_key="d1"),
        spconv.SubMConv3d(32, 32, 3),
        spconv.SparseMaxPool3d(3, 2, 1, indice_key="p2"),
        spconv.SparseConv3d(32, 32, 3, 2, 1, indice_key="c3"),
        spconv.SparseInverseConv3d(32, 32, 3, indice_key="c3"),
        spconv.SparseInverseConv3d(32, 32, 3, indice_key="p2"),
        spconv.SubMConv3d(32, 32, 3),
        spconv.SparseInverseConv3d(32, 16, 3, indice_key="d1"),
        spconv.SubMConv3d(16, 16, 3, indice_key="s1"),
        spconv.SparseConvTranspose3d(16, 16, 3, 2, 1),
        spconv.SubMConv3d(16, 16, 3))


def test_plan_follows_the_new_layers(dev):
    torch.manual_seed(0)
    block = _mixed_block().to(dev)
    rng = np.random.RandomState(9)
    shape = [17, 40, 36]
    idx = torch.from_numpy(R.random_voxels(rng, 2, shape, 900)).to(dev)
    feats = torch.randn((idx.shape[0], 16), device=dev)
    ref = block(spconv.SparseConvTensor(feats, idx, shape, 2))
    planned = spconv.SparseConvTensor(feats.new_empty((idx.shape[0], 0)), idx, shape, 2)
    outs = []
    end = planned.plan(spconv.sparse_convs(block), True, outs)
    assert len(outs) == 7
    assert outs[5][0] is idx and outs[5][1] == shape          # back through the inverse convs
    assert end.spatial_shape == R.deconv_output_size(shape, [3] * 3, [2] * 3, [1] * 3)
    got = block(planned.replace_feature(feats))
    assert got.indices is end.indices       # the forward pass found the planned rulebooks
    assert torch.equal(got.indices, ref.indices) and got.spatial_shape == ref.spatial_shape
    torch.testing.assert_close(got.features, ref.features, rtol=1e-5, atol=1e-5)
    # seed_strided_chain: the chain ends at the first pool / transposed / inverse layer
    t = spconv.SparseConvTensor(feats, idx, shape, 2)
    t.seed_strided_chain(spconv.sparse_convs(block))
    assert not t._rb_cache      # (only one plain strided conv in front of the pool)
    chain = [spconv.SparseConv3d(16, 16, 3, 2, 1), spconv.SparseConv3d(16, 16, 3, 2, 1),
             spconv.SparseConvTranspose3d(16, 16, 3, 2, 1), spconv.SparseConv3d(16, 16, 3, 2, 1)]
    t.seed_strided_chain(chain)
    assert len(t._rb_cache) == 2
    assert not any("transposed" in k for k in t._rb_cache)


def test_inverse_conv_refuses_a_foreign_voxel_set(dev):
    rng = np.random.RandomState(4)
    idx = torch.from_numpy(R.random_voxels(rng, 1, SHAPE, 80)).to(dev)
    x = spconv.SparseConvTensor(torch.randn((idx.shape[0], 16), device=dev), idx, SHAPE, 1)
    with torch.no_grad():
        d = spconv.SparseConv3d(16, 16, 3, 2, 1, indice_key="d").to(dev)(x)
        assert d.features.shape[0] != idx.shape[0]
        wrong = x.replace_feature(x.features)   # rows of the couple's INPUT set, not its output
        wrong.indice_dict = d.indice_dict
        with pytest.raises(ValueError):
            spconv.SparseInverseConv3d(16, 16, 3, indice_key="d").to(dev)(wrong)
