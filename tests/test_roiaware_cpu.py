"""RoI-aware pooling surface without a GPU.  The test_restatement_* tests check the numpy
restatement (tests/roiaware_ref.py) that the GPU tests compare the kernels against, using the
reference's own test literals (tests/test_models/test_common_modules/test_roiaware_pool3d.py).
The others check the product: points_in_boxes_cpu, the constructor arithmetic, the registry,
and the refusals that happen before anything reaches the device."""
import numpy as np
import pytest
import torch

import roiaware_ref as R

ROIS = [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 0.3], [-10.0, 23.0, 16.0, 10, 20, 20, 0.5]]
PTS = [[1, 2, 3.3], [1.2, 2.5, 3.0], [0.8, 2.1, 3.5], [1.6, 2.6, 3.6], [0.8, 1.2, 3.9],
       [-9.2, 21.0, 18.2], [3.8, 7.9, 6.3], [4.7, 3.5, -12.2], [3.8, 7.6, -2],
       [-10.6, -12.9, -20], [-16, -18, 9], [-21.3, -52, -5], [0, 0, 0], [6, 7, 8], [-2, -3, -4]]
PTS_B = [[[1, 2, 3.3], [1.2, 2.5, 3.0], [0.8, 2.1, 3.5], [1.6, 2.6, 3.6], [0.8, 1.2, 3.9],
          [-9.2, 21.0, 18.2], [3.8, 7.9, 6.3], [4.7, 3.5, -12.2]],
         [[3.8, 7.6, -2], [-10.6, -12.9, -20], [-16, -18, 9], [-21.3, -52, -5], [0, 0, 0],
          [6, 7, 8], [-2, -3, -4], [6, 4, 9]]]
EXPECT_GPU = [[0, 0, 0, 0, 0, -1, -1, -1], [-1, -1, -1, -1, -1, -1, -1, -1]]
EXPECT_CPU = [[1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
              [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
EXPECT_BATCH = [[[1, 0], [1, 0], [1, 0], [1, 0], [1, 0], [0, 1], [0, 0], [0, 0], [0, 0], [0, 0],
                 [0, 0], [0, 0], [0, 0], [0, 0], [0, 0]]]

PARTA2_SEG = dict(type="Single3DRoIAwareExtractor",
                  roi_layer=dict(type="RoIAwarePool3d", out_size=14, max_pts_per_voxel=128,
                                 mode="max"))
PARTA2_PART = dict(type="Single3DRoIAwareExtractor",
                   roi_layer=dict(type="RoIAwarePool3d", out_size=14, max_pts_per_voxel=128,
                                  mode="avg"))


def test_restatement_reproduces_the_reference_index_literals():
    """Checks the numpy restatement (tests/roiaware_ref.py), not the product: the GPU tests
    compare the kernels against this restatement."""
    boxes_b = [[ROIS[0]], [ROIS[1]]]
    np.testing.assert_array_equal(R.points_in_boxes_first(PTS_B, boxes_b), EXPECT_GPU)
    np.testing.assert_array_equal(R.local_coords(PTS, ROIS)[0].astype(np.int32), EXPECT_CPU)
    np.testing.assert_array_equal(R.points_in_boxes_all([PTS], [ROIS]), EXPECT_BATCH)


@pytest.mark.parametrize("mode,expected", [("max", 51.100), ("avg", 49.750)])
def test_restatement_reproduces_the_reference_pooled_sums(mode, expected):
    """Checks the numpy restatement (tests/roiaware_ref.py), not the product: the GPU tests
    compare the kernels against this restatement."""
    kept, _ = R.point_lists(ROIS, PTS, 4, 128)
    pooled, _ = R.pool(np.asarray(PTS, np.float32), kept, 2 * 64, mode)
    assert pooled.shape == (128, 3)
    assert abs(float(pooled.sum()) - expected) <= 1e-3 * expected


def test_restatement_caps_lists_in_point_order():
    """Checks the numpy restatement (tests/roiaware_ref.py), not the product: the GPU tests
    compare the kernels against this restatement."""
    rois = [[0, 0, 0, 4, 4, 4, 0]]
    pts = [[0.1, 0.1, 1.0]] * 5 + [[1.5, 1.5, 3.5]]
    kept, full = R.point_lists(rois, pts, 1, 3)
    assert list(kept) == [0] and full[0] == 6 and list(kept[0]) == [0, 1]
    kept, _ = R.point_lists(rois, pts, 1, 1)
    assert [len(v) for v in kept.values()] == [0]


def test_points_in_boxes_cpu_matches_the_reference_literal():
    from msmdfusion_amd.roiaware_pool3d import points_in_boxes_cpu
    out = points_in_boxes_cpu(points=torch.tensor(PTS), boxes=torch.tensor(ROIS))
    assert out.dtype == torch.int32 and out.shape == (2, 15)
    assert torch.equal(out, torch.tensor(EXPECT_CPU, dtype=torch.int32))
    from msmdfusion_amd.integration import roiaware_pool3d_ext as ext
    buf = torch.full((2, 15), 7, dtype=torch.int32)
    assert ext.points_in_boxes_cpu(torch.tensor(ROIS), torch.tensor(PTS), buf) == 1
    assert torch.equal(buf, out)


def test_roiaware_constructor_arithmetic():
    from msmdfusion_amd.roiaware_pool3d import RoIAwarePool3d
    a = RoIAwarePool3d(out_size=4, max_pts_per_voxel=128, mode="max")
    b = RoIAwarePool3d(out_size=(7, 5, 3), mode="avg")
    assert a.out_xyz == (4, 4, 4) and a.out_size == 4 and a.mode == 0 and a.mode_name == "max"
    assert b.out_xyz == (7, 5, 3) and b.mode == 1 and b.max_pts_per_voxel == 128
    assert RoIAwarePool3d(256).out_xyz == (256,) * 3 and RoIAwarePool3d(1).out_xyz == (1, 1, 1)
    with pytest.raises(ValueError, match="mode"):
        RoIAwarePool3d(4, mode="sum")
    for bad in (257, (14, 300, 2), (4, 4), 0, (4, 4, 4.0)):
        with pytest.raises(ValueError, match="out_size"):
            RoIAwarePool3d(bad)


def test_registry_builds_the_parta2_extractors():
    from msmdfusion_amd.registry import ROI_EXTRACTORS, build_roi_extractor
    from msmdfusion_amd.roiaware_pool3d import RoIAwarePool3d, Single3DRoIAwareExtractor
    seg, part = build_roi_extractor(PARTA2_SEG), build_roi_extractor(PARTA2_PART)
    assert "Single3DRoIAwareExtractor" in ROI_EXTRACTORS
    for ext, mode in ((seg, 0), (part, 1)):
        assert isinstance(ext, Single3DRoIAwareExtractor)
        assert isinstance(ext.roi_layer, RoIAwarePool3d)
        assert ext.roi_layer.out_xyz == (14, 14, 14) and ext.roi_layer.mode == mode
        assert ext.roi_layer.max_pts_per_voxel == 128
        assert list(ext.parameters()) == [] and len(ext.state_dict()) == 0
    with pytest.raises(KeyError):
        build_roi_extractor(dict(type="Single3DRoIAwareExtractor", roi_layer=dict(type="RoIAlign")))


def test_c_abi_refuses_out_sizes_above_256():
    from msmdfusion_amd._lib import lib
    for o in ((257, 4, 4), (4, 0, 4), (4, 4, 1000)):
        st = lib.msmd_roiaware_index(None, None, 0, None, None, 0, *o, 128, None, 0, None, None,
                                     None, None, None, 0, None)
        assert st == -3, o   # MSMD_ERR_UNSUPPORTED, before anything is enqueued


def test_gpu_entry_points_refuse_cpu_tensors():
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd.integration import roiaware_pool3d_ext as ext
    from msmdfusion_amd.roiaware_pool3d import (RoIAwarePool3d, points_in_boxes_batch,
                                                points_in_boxes_gpu)
    rois, pts = torch.tensor(ROIS), torch.tensor(PTS)
    with pytest.raises(RuntimeError):
        RoIAwarePool3d(4)(rois, pts, pts.clone())
    with pytest.raises(RuntimeError):
        K.roiaware_index(rois, pts, 4, 128)
    with pytest.raises(RuntimeError):
        points_in_boxes_gpu(torch.tensor(PTS_B), torch.tensor([[ROIS[0]], [ROIS[1]]]))
    with pytest.raises(RuntimeError):
        points_in_boxes_batch(pts[None], rois[None])
    z = torch.zeros((2, 4, 4, 4, 3))
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.forward(rois, pts, pts.clone(), z.int(), torch.zeros((2, 4, 4, 4, 128), dtype=torch.int32),
                    z, 0)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.backward(torch.zeros((2, 4, 4, 4, 128), dtype=torch.int32), z.int(), z,
                     torch.zeros((15, 3)), 1)
