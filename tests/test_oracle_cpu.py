"""CPU tests (no GPU): the oracle is pinned against
  (1) the literal vectors of the reference's own tests,
  (2) outputs of the reference's own CPU code, committed as
      tests/golden/reference_vectors.npz (tests/golden/make_golden.py),
  (3) the live reference build oracle/_ref/ when present (build container),
  (4) independent dense-conv / hand-derived cases where no reference exists
      here (spconv 2.x sparse_add, numba modality split).
"""
import os

import numpy as np
import pytest
import torch

from msmdfusion_amd import synthetic as S
from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_vectors.npz")
GEOMS = [("subm3", True, [3, 3, 3], [1, 1, 1], [1, 1, 1]),
         ("down_p1", False, [3, 3, 3], [2, 2, 2], [1, 1, 1]),
         ("down_p011", False, [3, 3, 3], [2, 2, 2], [0, 1, 1]),
         ("out_311", False, [3, 1, 1], [2, 1, 1], [0, 0, 0]),
         ("down_k3s1p0", False, [3, 3, 3], [1, 1, 1], [0, 0, 0]),
         ("down_k2s2", False, [2, 2, 2], [2, 2, 2], [0, 0, 0]),
         ("subm133", True, [1, 3, 3], [1, 1, 1], [0, 1, 1]),
         ("down_s3p2", False, [3, 3, 3], [3, 3, 3], [2, 2, 2])]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ---------------------------------------------------------------- (1) reference test literals
def test_voxel_generator_known_answer():
    """tests/test_models/test_voxel_encoder/test_voxel_generator.py:6-22."""
    np.random.seed(0)
    points = np.random.rand(1000, 4)
    v, c, n = O.hard_voxelize(points.astype(np.float32), [0.5, 0.5, 0.5],
                              [0, -40, -3, 70.4, 40, 1], 1000, 20000)
    expected = np.array([[7, 81, 1], [6, 81, 0], [7, 80, 1], [6, 81, 1], [7, 81, 0], [6, 80, 1],
                         [7, 80, 0], [6, 80, 0]])
    assert np.array_equal(c, expected)
    assert v.shape == (8, 1000, 4)
    assert np.array_equal(n, [120, 121, 127, 134, 115, 127, 125, 131])


def test_fps_known_answer():
    """tests/test_models/test_common_modules/test_pointnet_ops.py:9-23."""
    xyz = np.array([[[-0.2748, 1.0020, -1.1674], [0.1015, 1.3952, -1.2681],
                     [-0.8070, 2.4137, -0.5845], [-1.0001, 2.1982, -0.5859],
                     [0.3841, 1.8983, -0.7431]],
                    [[-1.0696, 3.0758, -0.1899], [-0.2559, 3.5521, -0.1402],
                     [0.8164, 4.0081, -0.1839], [-1.1000, 3.0213, -0.8205],
                     [-0.0518, 3.7251, -0.3950]]], np.float32)
    assert np.array_equal(O.furthest_point_sample(xyz, 3), [[0, 2, 4], [0, 2, 1]])


BQ_NEW = np.array([[[-0.0740, 1.3147, -1.3625], [-2.2769, 2.7817, -0.2334],
                    [-0.4003, 2.4666, -0.5116], [-0.0740, 1.3147, -1.3625],
                    [-0.0740, 1.3147, -1.3625]],
                   [[-2.0289, 2.4952, -0.1708], [-2.0668, 6.0278, -0.4875],
                    [0.4066, 1.4211, -0.2947], [-2.0289, 2.4952, -0.1708],
                    [-2.0289, 2.4952, -0.1708]]], np.float32)
BQ_XYZ = np.array([[[-0.0740, 1.3147, -1.3625], [0.5555, 1.0399, -1.3634],
                    [-0.4003, 2.4666, -0.5116], [-0.5251, 2.4379, -0.8466],
                    [-0.9691, 1.1418, -1.3733], [-0.2232, 0.9561, -1.3626],
                    [-2.2769, 2.7817, -0.2334], [-0.2822, 1.3192, -1.3645],
                    [0.1533, 1.5024, -1.0432], [0.4917, 1.1529, -1.3496]],
                   [[-2.0289, 2.4952, -0.1708], [-0.7188, 0.9956, -0.5096],
                    [-2.0668, 6.0278, -0.4875], [-1.9304, 3.3092, 0.6610],
                    [0.0949, 1.4332, 0.3140], [-1.2879, 2.0008, -0.7791],
                    [-0.7252, 0.9611, -0.6371], [0.4066, 1.4211, -0.2947],
                    [0.3220, 1.4447, 0.3548], [-0.9744, 2.3856, -1.2000]]], np.float32)
BQ_EXP1 = [[[0] * 5, [6] * 5, [2] * 5, [0] * 5, [0] * 5], [[0] * 5, [2] * 5, [7] * 5, [0] * 5, [0] * 5]]
BQ_EXP2 = [[[0, 5, 7, 0, 0], [6] * 5, [2, 3, 2, 2, 2], [0, 5, 7, 0, 0], [0, 5, 7, 0, 0]],
           [[0] * 5, [2] * 5, [7] * 5, [0] * 5, [0] * 5]]


def test_ball_query_known_answer():
    """test_pointnet_ops.py:26-73 (both radius settings)."""
    assert np.array_equal(O.ball_query(0, 0.2, 5, BQ_XYZ, BQ_NEW), BQ_EXP1)
    assert np.array_equal(O.ball_query(0.2, 0.4, 5, BQ_XYZ, BQ_NEW), BQ_EXP2)


# ---------------------------------------------------------------- (2) committed reference outputs
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_voxelize_vs_reference_vectors(gold, tag):
    p = gold[f"vox_{tag}_params"]
    v, c, n = O.hard_voxelize(gold["vox_points"], p[:3], S.POINT_CLOUD_RANGE, int(p[3]), int(p[4]))
    assert np.array_equal(c, gold[f"vox_{tag}_coors"])
    assert np.array_equal(n, gold[f"vox_{tag}_num"])
    assert np.array_equal(v, gold[f"vox_{tag}_voxels"])
    if tag == "c":
        assert c.shape[0] == 1500      # the max_voxels break really fired


@pytest.mark.parametrize("name,subm,ks,st,pd", GEOMS)
def test_rulebook_vs_reference_vectors(gold, name, subm, ks, st, pd):
    shape = gold["rb_shape"].tolist()
    oi, pr, nm, osz = O.get_indice_pairs(gold["rb_indices"], 2, shape, ks, st, pd, 1, subm)
    assert list(osz) == gold[f"rb_{name}_oshape"].tolist()
    assert np.array_equal(oi, gold[f"rb_{name}_out"])
    assert np.array_equal(nm, gold[f"rb_{name}_num"])
    assert np.array_equal(pr, gold[f"rb_{name}_pairs"])


@pytest.mark.parametrize("name,subm", [(g[0], g[1]) for g in GEOMS[:4]])
def test_conv_vs_reference_vectors(gold, name, subm):
    out = O.indice_conv_fwd(gold[f"conv_{name}_feat"], gold[f"conv_{name}_w"],
                            gold[f"rb_{name}_pairs"], gold[f"rb_{name}_num"],
                            gold[f"rb_{name}_out"].shape[0], subm=subm)
    np.testing.assert_allclose(out, gold[f"conv_{name}_out"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name,subm", [(g[0], g[1]) for g in GEOMS[:4]])
def test_conv_backward_vs_reference_vectors(gold, name, subm):
    """The oracle's backward == indiceConvBackward's loop (spconv_ops.h:363-456) run on
    the reference's own gather / scatter-add functors (oracle/ref_shim.cpp)."""
    din, dw = O.indice_conv_bwd(gold[f"conv_{name}_feat"], gold[f"conv_{name}_w"],
                                gold[f"conv_{name}_gout"], gold[f"rb_{name}_pairs"],
                                gold[f"rb_{name}_num"], subm=subm)
    np.testing.assert_allclose(din, gold[f"conv_{name}_din"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(dw, gold[f"conv_{name}_dw"], rtol=1e-5, atol=2e-5)


# ---------------------------------------------------------------- (3) live reference build
needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built (no /root/reference)")


@needs_ref
def test_live_reference_voxelize_and_rulebooks():
    pts = S.lidar_sweep(3, n_az=200)
    for mp, mv in [(10, 120000), (2, 900)]:
        a = O.hard_voxelize(pts, S.VOXEL_SIZE, S.POINT_CLOUD_RANGE, mp, mv)
        b = O.hard_voxelize(pts, S.VOXEL_SIZE, S.POINT_CLOUD_RANGE, mp, mv, use_ref=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    _, c, _ = O.hard_voxelize(pts, S.VOXEL_SIZE, S.POINT_CLOUD_RANGE, 10, 120000)
    idx = np.concatenate([np.zeros((c.shape[0], 1), np.int32), c], 1)
    for _, subm, ks, st, pd in GEOMS:
        a = O.get_indice_pairs(idx, 1, S.SPARSE_SHAPE, ks, st, pd, 1, subm)
        b = O.get_indice_pairs(idx, 1, S.SPARSE_SHAPE, ks, st, pd, 1, subm, use_ref=True)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


@needs_ref
def test_live_reference_conv_backward():
    rng = np.random.RandomState(11)
    idx = S.random_voxel_indices(1200, 2, [9, 40, 40], seed=5)
    for subm, ks, st, pd, cin, cout in [(True, 3, 1, 1, 24, 40), (False, 3, 2, 1, 32, 16)]:
        oi, pr, nm, _ = O.get_indice_pairs(idx, 2, [9, 40, 40], ks, st, pd, 1, subm)
        f = rng.randn(idx.shape[0], cin).astype(np.float32)
        w = (rng.randn(27, cin, cout) * 0.1).astype(np.float32)
        g = rng.randn(oi.shape[0], cout).astype(np.float32)
        a = O.indice_conv_bwd(f, w, g, pr, nm, subm=subm)
        b = O.indice_conv_bwd(f, w, g, pr, nm, subm=subm, use_ref=True)
        np.testing.assert_allclose(a[0], b[0], rtol=1e-5, atol=1e-5)
        # (dW sums ~1000 products per element in a different order: fp32 rounding)
        np.testing.assert_allclose(a[1], b[1], rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------- (4) independent pins
def _dense_conv(feat, idx, shape, batch, w_kio, ks, st, pd):
    """torch.nn.functional.conv3d on the densified input (the cross-check
    mmdet3d/ops/spconv/test_utils.py:145-193 builds)."""
    dense = torch.from_numpy(O.dense(feat, idx, batch, shape))
    kvol, cin, cout = w_kio.shape
    w = torch.from_numpy(w_kio).reshape(*ks, cin, cout).permute(4, 3, 0, 1, 2).contiguous()
    return torch.nn.functional.conv3d(dense.double(), w.double(), stride=st, padding=pd).numpy()


@pytest.mark.parametrize("name,subm,ks,st,pd", GEOMS[:6])
def test_sparse_conv_equals_dense_conv(name, subm, ks, st, pd):
    shape, batch = [7, 12, 12], 2
    idx = S.random_voxel_indices(150, batch, shape, seed=5)
    rng = np.random.RandomState(1)
    f = rng.randn(idx.shape[0], 6).astype(np.float32)
    kvol = int(np.prod(ks))
    w = rng.randn(kvol, 6, 4).astype(np.float32)
    oi, pr, nm, osz = O.get_indice_pairs(idx, batch, shape, ks, st, pd, 1, subm)
    out = O.indice_conv_fwd(f, w, pr, nm, oi.shape[0], subm=subm)
    ref = _dense_conv(f, idx, shape, batch, w, ks, st, [k // 2 for k in ks] if subm else pd)
    got = ref[oi[:, 0], :, oi[:, 1], oi[:, 2], oi[:, 3]]
    np.testing.assert_allclose(out, got, rtol=1e-4, atol=1e-4)
    if not subm:   # every output site the dense conv can reach from an active input is present
        reach = _dense_conv(np.ones((idx.shape[0], 1), np.float32), idx, shape, batch,
                            np.ones((kvol, 1, 1), np.float32), ks, st, pd)[:, 0] > 0
        assert reach.sum() == oi.shape[0]
        assert reach[oi[:, 0], oi[:, 1], oi[:, 2], oi[:, 3]].all()


def test_conv_backward_matches_autograd_of_dense_conv():
    shape, batch, ks = [5, 9, 9], 1, [3, 3, 3]
    idx = S.random_voxel_indices(80, batch, shape, seed=2)
    rng = np.random.RandomState(0)
    f = rng.randn(idx.shape[0], 3).astype(np.float32)
    w = rng.randn(27, 3, 5).astype(np.float32)
    for subm, st, pd in [(True, [1, 1, 1], [1, 1, 1]), (False, [2, 2, 2], [1, 1, 1])]:
        oi, pr, nm, osz = O.get_indice_pairs(idx, batch, shape, ks, st, pd, 1, subm)
        g = rng.randn(oi.shape[0], 5).astype(np.float32)
        din, dw = O.indice_conv_bwd(f, w, g, pr, nm, subm=subm)
        ft = torch.from_numpy(f).double().requires_grad_(True)
        wt = torch.from_numpy(w).double().requires_grad_(True)
        ii = torch.from_numpy(idx).long()
        dense = torch.zeros(batch, *shape, 3, dtype=torch.double)        # channels last
        dense = dense.index_put((ii[:, 0], ii[:, 1], ii[:, 2], ii[:, 3]), ft)
        dense = dense.permute(0, 4, 1, 2, 3)
        y = torch.nn.functional.conv3d(dense, wt.reshape(3, 3, 3, 3, 5).permute(4, 3, 0, 1, 2),
                                       stride=st, padding=pd)
        oo = torch.from_numpy(oi).long()
        loss = (y[oo[:, 0], :, oo[:, 1], oo[:, 2], oo[:, 3]] * torch.from_numpy(g).double()).sum()
        loss.backward()
        np.testing.assert_allclose(din, ft.grad.numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(dw, wt.grad.numpy(), rtol=1e-4, atol=1e-4)


def test_sparse_add_hand_case_and_dense_identity():
    shape = [2, 3, 3]
    ia = np.array([[0, 1, 2, 2], [0, 0, 0, 1], [1, 0, 0, 0]], np.int32)
    ib = np.array([[1, 0, 0, 0], [0, 0, 0, 0], [0, 1, 2, 2]], np.int32)
    fa = np.array([[1, 2], [3, 4], [5, 6]], np.float32)
    fb = np.array([[10, 20], [30, 40], [50, 60]], np.float32)
    oi, of, ma, mb = O.sparse_add(fa, ia, fb, ib, shape)
    assert oi.tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 1, 2, 2], [1, 0, 0, 0]]
    assert of.tolist() == [[30, 40], [3, 4], [51, 62], [15, 26]]
    assert ma.tolist() == [2, 1, 3] and mb.tolist() == [3, 0, 2]
    a = S.random_voxel_indices(200, 2, [5, 20, 20], seed=1)
    b = S.random_voxel_indices(150, 2, [5, 20, 20], seed=2)
    rng = np.random.RandomState(0)
    fa, fb = rng.randn(a.shape[0], 3).astype(np.float32), rng.randn(b.shape[0], 3).astype(np.float32)
    oi, of, _, _ = O.sparse_add(fa, a, fb, b, [5, 20, 20])
    np.testing.assert_allclose(O.dense(of, oi, 2, [5, 20, 20]),
                               O.dense(fa, a, 2, [5, 20, 20]) + O.dense(fb, b, 2, [5, 20, 20]))
    lid = O.linear_ids(oi, [5, 20, 20])
    assert (np.diff(lid) > 0).all()


def test_modality_split_hand_case_and_float_key_aliasing():
    shape = [41, 1440, 1440]
    z3 = np.array([[0, 0, 5], [3, 7, 9], [1, 1, 1], [40, 2, 2]], np.int32)
    z2 = np.array([[1, 1, 1], [0, 0, 6], [40, 2, 2], [9, 9, 9]], np.int32)
    m3, m2, p3, p2 = O.modality_split(z3, z2, shape)
    assert m3.tolist() == [0, 0, 1, 1] and m2.tolist() == [1, 0, 1, 0]
    assert p3.tolist() == [2, 3] and p2.tolist() == [0, 2]
    # the reference's float32 key y*1e3 + x aliases for x >= 1000 ...
    a = np.array([[0, 5, 1000]], np.int32)
    b = np.array([[0, 6, 0]], np.int32)
    assert O.modality_split(a, b, shape, float_keys=True)[0].tolist() == [1]   # false match
    assert O.modality_split(a, b, shape, float_keys=False)[0].tolist() == [0]  # exact keys
    # ... and loses low bits of x once the key passes 2^24 (z >= 17)
    a = np.array([[20, 100, 3]], np.int32)
    b = np.array([[20, 100, 4]], np.int32)
    assert O.modality_split(a, b, shape, float_keys=True)[0].tolist() == [1]
    assert O.modality_split(a, b, shape, float_keys=False)[0].tolist() == [0]


def test_dense_hand_case():
    f = np.array([[1, 2], [3, 4]], np.float32)
    idx = np.array([[1, 0, 1, 2], [0, 1, 0, 0]], np.int32)
    d = O.dense(f, idx, 2, [2, 2, 3])
    assert d.shape == (2, 2, 2, 2, 3) and d.sum() == 10
    assert d[1, :, 0, 1, 2].tolist() == [1, 2] and d[0, :, 1, 0, 0].tolist() == [3, 4]


def test_nn_assign_last_write_wins_and_fps_tie_order():
    grp = np.array([[0, 1, 1], [1, 2, 2], [3, 3, 3]], np.int32)
    assert O.nn_assign(grp, np.array([7, 8, -1], np.int32), 5).tolist() == [7, 8, 8, -1, -1]
    # all points equidistant from point 0: the reference's tree keeps the lower
    # slot of each pair -> among tied thread ids the bit-reversed-smallest wins
    xyz = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0]]], np.float32)
    assert O.fps_block_size(5) == 4
    assert O.furthest_point_sample(xyz, 2).tolist() == [[0, 4]]   # k=4 shares thread 0 with k=0


def test_modality_split_vs_the_references_own_function():
    """tests/golden/modality_split_vectors.npz = what the reference's voxel_modality_split +
    type_assign (MSMDFusion.py:251-325, 27-45, executed by make_modality_split_golden.py)
    returned for voxel sets whose float32 keys alias across the sets: the oracle's float-key
    restatement reproduces the flags and the syn_mix lists -- false matches and the
    non-cumulative batch offsets (:288-289,313-314) included -- and the exact-key mode does not."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             "modality_split_vectors.npz"))
    shape = [41, 1440, 1440]
    for tag, batch in (("b1", 1), ("b2", 2), ("b3", 3)):
        i3, i2 = g[tag + "_idx3"], g[tag + "_idx2"]
        e3, e2, p3, p2 = [], [], [], []
        last3 = last2 = 0
        for b in range(batch):
            r3, r2 = np.flatnonzero(i3[:, 0] == b), np.flatnonzero(i2[:, 0] == b)
            m3, m2, q3, q2 = O.modality_split(i3[r3, 1:], i2[r2, 1:], shape, float_keys=True)
            e3.append(m3); e2.append(m2)
            p3.append(q3.astype(np.int64) + last3); p2.append(q2.astype(np.int64) + last2)
            last3, last2 = len(r3), len(r2)
        assert np.array_equal(np.concatenate(e3), g[tag + "_mix3"]), tag
        assert np.array_equal(np.concatenate(e2), g[tag + "_mix2"]), tag
        assert np.array_equal(np.concatenate(p3), g[tag + "_syn3"]), tag
        assert np.array_equal(np.concatenate(p2), g[tag + "_syn2"]), tag
        x3 = np.concatenate([O.modality_split(i3[i3[:, 0] == b][:, 1:], i2[i2[:, 0] == b][:, 1:],
                                              shape)[0] for b in range(batch)])
        assert not np.array_equal(x3, g[tag + "_mix3"])          # exact keys: fewer "mixed"
        assert x3.sum() < g[tag + "_mix3"].sum()


def test_sparse_add_equals_torch_coo_add_and_coalesce():
    """spconv-2.x is not in the tree; its functional.sparse_add (call site
    sparse_multimodal_encoder_painting.py:455) adds the operands as COO tensors and coalesces
    -- rows in ascending linear index, features summed where coordinates coincide.  The
    oracle's restatement against torch's own `torch.sparse_coo_tensor(...) + ...` followed by
    `.coalesce()` on the same operands (coordinates repeated INSIDE an operand included, which
    the fusion stack's unified sets can produce in reference mode)."""
    import torch
    shape, batch = [5, 24, 24], 2
    a = S.random_voxel_indices(400, batch, shape, seed=3)
    b = np.concatenate([a[::3], S.random_voxel_indices(300, batch, shape, seed=4)])
    b = np.concatenate([b, b[:7]])                         # a few repeated rows inside b
    rng = np.random.RandomState(1)
    fa = rng.randn(a.shape[0], 6).astype(np.float32)
    fb = rng.randn(b.shape[0], 6).astype(np.float32)
    oi, of, ma, mb = O.sparse_add(fa, a, fb, b, shape)
    size = (batch, *shape, 6)
    ta = torch.sparse_coo_tensor(torch.from_numpy(a.T.astype(np.int64)), torch.from_numpy(fa), size)
    tb = torch.sparse_coo_tensor(torch.from_numpy(b.T.astype(np.int64)), torch.from_numpy(fb), size)
    tc = (ta + tb).coalesce()
    assert np.array_equal(tc.indices().numpy().T.astype(np.int32), oi)
    np.testing.assert_allclose(tc.values().numpy(), of, rtol=1e-6, atol=1e-6)
    # the row maps point every operand row at its coordinate's output row
    assert np.array_equal(oi[ma], a) and np.array_equal(oi[mb], b)


def test_subm_numpy_table_equals_the_oracle():
    """tests/subm_table_ref.py, the dense-grid table the SubM rulebook tests compare the
    kernels with, equals get_indice_pairs on the duplicate-free cases; where coordinates
    repeat (the oracle leaves the columns of shadowed rows at -1, the kernels pair every row
    with the last row of its coordinate) the centre entry of both the shadowed rows and their
    winners is the winner."""
    import subm_table_ref as R
    for i, (_, batch, shape, ks, _) in enumerate(R.CASES):
        idx = R.case_indices(i)
        exp = R.subm_table(idx, batch, shape, ks)
        if i == 0:
            n, dup = idx.shape[0], R.N_DUPLICATES
            assert n == R.CASES[0][0] + dup
            winners = np.arange(n - dup, n)
            assert np.array_equal(exp[13, :dup], winners) and np.array_equal(exp[13, n - dup:], winners)
            continue
        _, pr, nm, _ = O.get_indice_pairs(idx, batch, shape, ks, 1, 0, 1, True)
        want = np.full_like(exp, -1)
        for k in range(nm.shape[0]):
            p = int(nm[k])
            want[k, pr[k, 1, :p]] = pr[k, 0, :p]
        assert np.array_equal(exp, want), (i, ks)
