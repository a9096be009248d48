"""Dynamic voxelization surface without a GPU: DynamicVFE's constructor arithmetic and
state-dict keys against the reference's (voxel_encoder.py:92-176), the registry entries, and
the refusals of the shims and modules (no CPU path)."""
import pytest
import torch

from msmdfusion_amd import synthetic as S

VS, RG = S.VOXEL_SIZE, S.POINT_CLOUD_RANGE


def _ref_keys(n_layers):
    keys = []
    for i in range(n_layers):
        keys += ["vfe_layers.%d.0.weight" % i]
        keys += ["vfe_layers.%d.1.%s" % (i, k) for k in
                 ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    return keys


@pytest.mark.parametrize("cluster,center,dist", [(True, True, False), (False, False, False),
                                                 (True, False, True)])
def test_dynamic_vfe_state_dict_matches_reference(cluster, center, dist):
    from msmdfusion_amd.voxel_encoder import DynamicVFE
    m = DynamicVFE(in_channels=4, feat_channels=[64, 128], with_cluster_center=cluster,
                   with_voxel_center=center, with_distance=dist, voxel_size=VS,
                   point_cloud_range=RG, mode="max")
    sd = m.state_dict()
    assert list(sd) == _ref_keys(2)
    cin = 4 + 3 * cluster + 3 * center + 3 * dist      # (sic) voxel_encoder.py:133-138
    assert m.in_channels == cin
    assert tuple(sd["vfe_layers.0.0.weight"].shape) == (64, cin)
    assert tuple(sd["vfe_layers.1.0.weight"].shape) == (128, 128)
    assert tuple(sd["vfe_layers.1.1.running_var"].shape) == (128,)
    bn = m.vfe_layers[0][1]
    assert isinstance(bn, torch.nn.BatchNorm1d) and bn.eps == 1e-3 and bn.momentum == 0.01
    assert m.x_offset == VS[0] / 2 + RG[0] and m.z_offset == VS[2] / 2 + RG[2]
    assert m.vfe_scatter.average_points is False and m.cluster_scatter.average_points is True


def test_dynamic_vfe_refusals():
    from msmdfusion_amd.voxel_encoder import DynamicVFE
    with pytest.raises(NotImplementedError):
        DynamicVFE(feat_channels=[64], fusion_layer=dict(type="PointFusion"))
    m = DynamicVFE(in_channels=4, feat_channels=[64], with_distance=True)
    with pytest.raises(RuntimeError, match="with_distance"):
        m(torch.zeros((10, 4)), torch.zeros((10, 4), dtype=torch.int32))


def test_registry_builds_dynamic_encoders():
    from msmdfusion_amd.registry import build_voxel_encoder
    from msmdfusion_amd.voxel_encoder import DynamicSimpleVFE, DynamicVFE
    a = build_voxel_encoder(dict(type="DynamicSimpleVFE", voxel_size=VS, point_cloud_range=RG))
    b = build_voxel_encoder(dict(type="DynamicVFE", in_channels=5, feat_channels=[32, 32],
                                 with_cluster_center=True, voxel_size=VS, point_cloud_range=RG,
                                 mode="avg"))
    assert isinstance(a, DynamicSimpleVFE) and isinstance(b, DynamicVFE)
    assert a.scatter.average_points and b.vfe_scatter.average_points


def test_dynamic_scatter_module_surface():
    from msmdfusion_amd.dynamic_scatter import DynamicScatter
    m = DynamicScatter(VS, RG, True)
    assert m.reduce_type == "mean" and DynamicScatter(VS, RG, False).reduce_type == "max"
    assert "average_points=True" in repr(m)


def test_shims_refuse_cpu_tensors_and_unknown_reduce():
    from msmdfusion_amd import kernels as K
    from msmdfusion_amd.integration import voxel_layer
    pts = torch.zeros((8, 5))
    coors = torch.zeros((8, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        voxel_layer.dynamic_voxelize(pts, coors, VS, RG, 3)
    with pytest.raises(RuntimeError):
        voxel_layer.dynamic_point_to_voxel_forward(pts, coors, "mean")
    with pytest.raises(RuntimeError):
        voxel_layer.dynamic_point_to_voxel_backward(pts, pts, pts, pts, coors[:, 0], coors[:, 0],
                                                    "sum")
    with pytest.raises(RuntimeError):
        K.scatter_index(coors)
    with pytest.raises(RuntimeError):
        K.dynamic_voxelize(pts, VS, RG)
    with pytest.raises(RuntimeError, match="reduce type"):
        K._reduce_code("min")


def test_transfusion_detector_accepts_dynamic_voxel_layer():
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.detector import build_detector
    from msmdfusion_amd.voxel_encoder import DynamicSimpleVFE
    cfg = dict(C.TRANSFUSION_L["model"])
    cfg["pts_voxel_layer"] = dict(cfg["pts_voxel_layer"], max_num_points=-1)
    cfg["pts_voxel_encoder"] = dict(type="DynamicSimpleVFE", voxel_size=VS, point_cloud_range=RG)
    det = build_detector(cfg)
    assert det.dynamic_voxelization and isinstance(det.pts_voxel_encoder, DynamicSimpleVFE)
    assert not build_detector(C.TRANSFUSION_L["model"]).dynamic_voxelization
