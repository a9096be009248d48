"""Anchor3DHead without a GPU: the generators, the coder and the nearest-BEV overlaps (plain
torch, checked against values worked out by hand from the reference's formulas), state-dict
keys and the registry, the two KITTI config fixtures, the construction-time refusals, and the
C ABI's host-side argument validation."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _assigner(**kw):
    return dict(dict(type="MaxIoUAssigner", iou_calculator=dict(type="BboxOverlapsNearest3D"),
                     pos_iou_thr=0.6, neg_iou_thr=0.45, min_pos_iou=0.45, ignore_iof_thr=-1), **kw)


def _head_cfg(**kw):
    from msmdfusion_amd import configs as C
    m = C.POINTPILLARS_SECFPN_KITTI["model"]
    return dict(dict(m["bbox_head"], train_cfg=m["train_cfg"], test_cfg=m["test_cfg"]), **kw)


def test_range_generator_layout_and_cache():
    """[1, H, W, sizes, rotations, 7]; x runs along W and y along H (linspace over the range,
    ends included); the aligned generator puts centres on the cell centres; custom values are
    zero columns; one tensor per (featmap_sizes, device)."""
    from msmdfusion_amd import anchor_head as A
    g = A.Anchor3DRangeGenerator(ranges=[[0, -4.0, -0.6, 10.0, 4.0, -0.6],
                                         [0, -4.0, -1.78, 10.0, 4.0, -1.78]],
                                 sizes=[[0.6, 0.8, 1.73], [1.6, 3.9, 1.56]], rotations=[0, 1.57],
                                 reshape_out=False)
    assert g.num_base_anchors == 4 and g.num_levels == 1
    (a,) = g.grid_anchors([(8, 6)], "cpu")
    assert tuple(a.shape) == (1, 8, 6, 2, 2, 7)
    np.testing.assert_array_equal(a[0, 0, :, 0, 0, 0].numpy(),
                                  torch.linspace(0, 10.0, 6).numpy())
    np.testing.assert_array_equal(a[0, :, 0, 0, 0, 1].numpy(),
                                  torch.linspace(-4.0, 4.0, 8).numpy())
    assert a[0, 3, 2, 1, 1].tolist() == pytest.approx([4.0, -4.0 + 3 * 8 / 7, -1.78, 1.6, 3.9,
                                                       1.56, 1.57])
    assert g.grid_anchors([(8, 6)], "cpu")[0] is a                  # cached
    al = A.AlignedAnchor3DRangeGenerator(ranges=[[0, -4.0, -1.8, 12.0, 4.0, -1.8]], scales=[1, 2],
                                         sizes=[[1.0, 2.0, 1.5]], custom_values=[0, 0],
                                         rotations=[0, 1.57], reshape_out=True)
    l0, l1 = al.grid_anchors([(8, 6), (4, 3)], "cpu")
    assert tuple(l0.shape) == (8 * 6 * 2, 9) and tuple(l1.shape) == (4 * 3 * 2, 9)
    assert l0[0].tolist() == pytest.approx([1.0, -3.5, -1.8, 1.0, 2.0, 1.5, 0, 0, 0])
    assert l1[0].tolist() == pytest.approx([2.0, -3.0, -1.8, 2.0, 4.0, 3.0, 0, 0, 0])
    with pytest.raises(NotImplementedError):
        A.build_anchor_generator(dict(type="AlignedAnchor3DRangeGeneratorPerCls", ranges=[[0] * 6]))


def test_coder_round_trip_and_formulas():
    from msmdfusion_amd.anchor_head import DeltaXYZWLHRBBoxCoder as Coder
    a = torch.tensor([[1.0, 2.0, -1.0, 1.6, 3.9, 1.56, 0.0, 0.0, 0.0]])
    g = torch.tensor([[2.0, 1.0, -0.5, 2.0, 4.5, 1.2, 0.3, 1.0, -2.0]])
    t = Coder.encode(a, g)
    diag = math.sqrt(3.9 ** 2 + 1.6 ** 2)
    want = [1 / diag, -1 / diag, ((-0.5 + 0.6) - (-1.0 + 0.78)) / 1.56, math.log(2.0 / 1.6),
            math.log(4.5 / 3.9), math.log(1.2 / 1.56), 0.3, 1.0, -2.0]
    assert t[0].tolist() == pytest.approx(want, rel=1e-6)
    np.testing.assert_allclose(Coder.decode(a, t).numpy(), g.numpy(), rtol=1e-6, atol=1e-6)
    assert Coder(code_size=9).code_size == 9


def test_nearest_bev_overlaps():
    """A box turned by more than 45 degrees swaps its footprint; IoU = overlap / max(union,
    1e-6) on the axis-aligned footprints."""
    from msmdfusion_amd import anchor_head as A
    boxes = torch.tensor([[0.0, 0.0, 0.0, 2.0, 4.0, 1.0, 0.0],
                          [0.0, 0.0, 0.0, 2.0, 4.0, 1.0, 1.57],
                          [1.0, 0.0, 0.0, 2.0, 4.0, 1.0, 3.2]])
    bev = A.nearest_bev(boxes)
    assert bev.tolist() == [[-1, -2, 1, 2], [-2, -1, 2, 1], [0, -2, 2, 2]]
    ov = A.bbox_overlaps_nearest_3d(boxes, boxes)
    assert ov.diagonal().tolist() == [1.0, 1.0, 1.0]
    assert float(ov[0, 1]) == pytest.approx(4.0 / 12.0) and float(ov[0, 2]) == pytest.approx(1 / 3)
    assert float(A.BboxOverlapsNearest3D()(boxes[:1], boxes[2:], is_aligned=True)) == \
        pytest.approx(1 / 3)


def test_state_dict_keys_and_registry():
    from msmdfusion_amd.registry import DETECTORS, HEADS, build_detector, build_head
    from msmdfusion_amd import configs as C
    head = build_head(_head_cfg())
    assert "Anchor3DHead" in HEADS and type(head).__name__ == "Anchor3DHead"
    assert sorted(head.state_dict()) == ["conv_cls.bias", "conv_cls.weight", "conv_dir_cls.bias",
                                         "conv_dir_cls.weight", "conv_reg.bias", "conv_reg.weight"]
    assert head.num_anchors == 6 and head.box_code_size == 7 and not head.sampling
    assert tuple(head.conv_cls.weight.shape) == (18, 384, 1, 1)
    assert tuple(head.conv_reg.weight.shape) == (42, 384, 1, 1)
    head.init_weights()
    assert float(head.conv_cls.bias[0].detach()) == pytest.approx(-math.log(99.0))
    assert [type(a).__name__ for a in head.bbox_assigner] == ["MaxIoUAssigner"] * 3
    outs = head([torch.zeros(2, 384, 4, 3)])
    assert [tuple(o[0].shape) for o in outs] == [(2, 18, 4, 3), (2, 42, 4, 3), (2, 12, 4, 3)]
    det = build_detector(C.SECOND_SECFPN_KITTI["model"])
    assert "VoxelNet" in DETECTORS and type(det).__name__ == "VoxelNet"
    assert {k.split(".")[0] for k in det.state_dict()} == {"middle_encoder", "backbone", "neck",
                                                          "bbox_head"}
    assert det.pts_bbox_head is det.bbox_head and det.pts_backbone is det.backbone
    assert type(det.voxel_encoder).__name__ == "HardSimpleVFE"


def test_kitti_configs_equal_the_reference_dicts():
    from msmdfusion_amd import configs as C
    fx = json.load(open(os.path.join(HERE, "golden", "reference_anchor_head_configs.json")))
    norm = lambda o: json.loads(json.dumps(o))   # tuples -> lists
    assert norm(C.POINTPILLARS_SECFPN_KITTI) == fx["hv_pointpillars_secfpn_kitti"]
    assert norm(C.SECOND_SECFPN_KITTI) == fx["hv_second_secfpn_kitti"]


def test_construction_time_refusals():
    from msmdfusion_amd import anchor_head as A
    from msmdfusion_amd.registry import build_head
    for bad in (dict(ignore_iof_thr=0.5), dict(neg_iou_thr=(0.1, 0.4)),
                dict(match_low_quality=False), dict(gt_max_assign_all=False),
                dict(iou_calculator=dict(type="BboxOverlaps3D", coordinate="lidar")),
                dict(iou_calculator=dict(type="BboxOverlapsNearest3D", coordinate="camera"))):
        with pytest.raises(NotImplementedError):
            A.build_assigner(_assigner(**bad))
    A.build_assigner(_assigner())
    with pytest.raises(NotImplementedError, match="sampler"):
        build_head(_head_cfg(loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True,
                                           loss_weight=1.0)))
    with pytest.raises(NotImplementedError, match="softmax"):
        build_head(_head_cfg(loss_cls=dict(type="FocalLoss", use_sigmoid=False)))
    with pytest.raises(NotImplementedError):
        build_head(_head_cfg(train_cfg=dict(assigner=dict(type="HungarianAssigner3D"))))
    head = build_head(_head_cfg())
    with pytest.raises(RuntimeError, match="CUDA"):
        head.bbox_assigner[0].assign(torch.zeros(4, 7), torch.zeros(1, 7))


def test_c_abi_argument_validation():
    """Null pointers, negative counts, offsets that do not ascend (or do not start at 0), too
    many segments, a code size outside 7..16, a missing workspace: refused before anything is
    enqueued."""
    from msmdfusion_amd._lib import float_arr, lib
    p = ctypes.c_void_p(256)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    f = float_arr([0.5, 0.5])
    ws = lib.msmd_anchor_assign_workspace_bytes(4)
    assert ws >= 16 and lib.msmd_anchor_assign_workspace_bytes(-1) == 0
    assert lib.msmd_anchor_max_segments() == 64 and lib.msmd_anchor_gt_chunk() == 128

    def assign(anchor_bev=p, rows=8, offs=ints(0, 5, 8), segs=2, gt=p, num_gt=4, gt_offsets=p,
               entries=4, out=p, work=p, nbytes=ws):
        return lib.msmd_anchor_assign_f32(anchor_bev, rows, offs, segs, gt, num_gt, None,
                                          gt_offsets, entries, f, f, f, out, out, out, work,
                                          nbytes, None)
    assert assign(offs=ints(0, 5, 3)) == -1                  # descending
    assert assign(offs=ints(1, 5, 8)) == -1                  # does not start at 0
    assert assign(offs=None) == -1
    assert assign(anchor_bev=None) == -1 and assign(gt=None) == -1
    assert assign(gt_offsets=None) == -1 and assign(out=None) == -1
    assert assign(rows=-1) == -1 and assign(num_gt=-1) == -1 and assign(entries=-1) == -1
    assert assign(segs=-1) == -1 and assign(segs=65) == -5
    assert assign(entries=5) == -1                           # no gt_index: entries are rows
    assert assign(work=None) == -2 and assign(nbytes=0) == -2
    assert assign(segs=0) == 0                               # nothing to do, nothing launched

    def targets(code=7, offs=ints(0, 5, 8), assigned=p, rows=8, dest=None, labels=p):
        return lib.msmd_anchor_targets_f32(assigned, p, rows, code, offs, 2, p, labels, 4, None, p,
                                           4, dest, 3, -1.0, 0.0, p, p, p, p, p, p, None)
    assert targets(code=6) == -3 and targets(code=17) == -3
    assert targets(offs=ints(0, 5, 3)) == -1 and targets(assigned=None) == -1
    assert targets(labels=None) == -1
    assert targets(rows=3, dest=p) == -1                     # a permutation needs whole samples

    assert lib.msmd_sigmoid_focal_workspace_bytes(4099, 10) >= 8 * 21
    assert lib.msmd_sigmoid_focal_workspace_bytes(-1, 3) == 0
    focal = lambda n=4, c=3, x=p, out=p, work=p, nbytes=256, gamma=2.0: \
        lib.msmd_sigmoid_focal_f32(x, p, p, n, c, gamma, 0.25, None, out, work, nbytes, None)
    assert focal(n=-1) == -1 and focal(c=0) == -1 and focal(x=None) == -1
    assert focal(out=None) == -1 and focal(gamma=-1.0) == -1
    assert focal(work=None) == -2 and focal(nbytes=0) == -2


# ---------------------------------------------------------------- against the reference's outputs
GOLD = os.path.join(HERE, "golden", "anchor_head_vectors.npz")
K_RANGES = [[0, -8.0, -0.6, 20.0, 8.0, -0.6], [0, -8.0, -0.6, 20.0, 8.0, -0.6],
            [0, -8.0, -1.78, 20.0, 8.0, -1.78]]
K_SIZES = [[0.6, 0.8, 1.73], [0.6, 1.76, 1.73], [1.6, 3.9, 1.56]]
N_SIZES = [[0.866, 2.5981, 1.0], [0.5774, 1.7321, 1.0], [1.0, 1.0, 1.0]]


@pytest.fixture(scope="module")
def gold():
    """The reference's own outputs (tests/golden/make_anchor_head_golden.py); read-only."""
    return np.load(GOLD)


def test_generators_equal_the_reference(gold):
    from msmdfusion_amd import anchor_head as A
    (ak,) = A.Anchor3DRangeGenerator(ranges=K_RANGES, sizes=K_SIZES, rotations=[0, 1.57],
                                     reshape_out=False).grid_anchors([(8, 6)], "cpu")
    np.testing.assert_array_equal(ak.numpy(), gold["anchors_k"])
    an = A.AlignedAnchor3DRangeGenerator(
        ranges=[[0, -8.0, -1.8, 20.0, 8.0, -1.8]], scales=[1, 2], sizes=N_SIZES,
        custom_values=[0, 0], rotations=[0, 1.57], reshape_out=True).grid_anchors(
            [(8, 6), (4, 3)], "cpu")
    np.testing.assert_array_equal(an[0].numpy(), gold["anchors_n0"])
    np.testing.assert_array_equal(an[1].numpy(), gold["anchors_n1"])


def test_coder_and_overlaps_equal_the_reference(gold):
    from msmdfusion_amd import anchor_head as A
    an0, n7 = torch.from_numpy(gold["anchors_n0"]), torch.from_numpy(gold["n_gt_boxes_1"])
    enc = A.DeltaXYZWLHRBBoxCoder.encode(an0[:7], n7)
    np.testing.assert_array_equal(enc.numpy(), gold["coder_encode"])
    np.testing.assert_array_equal(A.DeltaXYZWLHRBBoxCoder.decode(an0[7:14], enc * 0.5).numpy(),
                                  gold["coder_decode"])
    seven = torch.from_numpy(gold["k_gt_boxes_1"])
    flat_k = torch.from_numpy(gold["anchors_k"]).reshape(-1, 7)
    np.testing.assert_array_equal(A.bbox_overlaps_nearest_3d(seven, flat_k).numpy(),
                                  gold["overlaps_k7"])
    np.testing.assert_array_equal(
        A.BboxOverlapsNearest3D()(n7, torch.from_numpy(gold["anchors_n1"])).numpy(),
        gold["overlaps_n7"])
    np.testing.assert_array_equal(
        A.bbox_overlaps_nearest_3d(seven, flat_k[40:47], is_aligned=True).numpy(),
        gold["overlaps_aligned"])
    assert (gold["overlaps_k7"] > 0.5).any()
