"""The pillar path without a GPU: the composition path of PillarFeatureNet against the
reference's own outputs (tests/golden/pillar_vectors.npz), the module surface, the config and
the C ABI's refusals."""
import ctypes
import json
import os

import pytest
import torch
from torch import nn

import pillar_fixture as PF

TOL = 1e-4      # the project's feature tolerance, of the expected tensor's largest entry
CASES = sorted(PF.golden()[1]["cases"])


@pytest.mark.parametrize("tag", CASES)
def test_composition_matches_the_reference(tag):
    """Outputs, updated running statistics and batch counter of every golden case; the input
    tensor is left as it was (the reference's legacy path overwrites its x, y)."""
    mod, (feats, num, coors), exp, after = PF.golden_case(tag)
    before = feats.clone()
    with torch.no_grad():
        out = mod(feats, num, coors)
    assert tuple(out.shape) == tuple(exp.shape)
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


def test_golden_covers_what_the_kernel_must_reproduce():
    g, meta = PF.golden()
    assert len(CASES) == 12
    assert (g["exceed.num_points"] > 20).any() and g["exceed.num_points"].min() >= 1
    assert (g["base.num_points"] == 1).any() and (g["base.num_points"] == 20).any()
    assert g["base.features"].shape == (97, 20, 5) and g["c4m32.features"].shape[1:] == (32, 4)
    assert meta["cases"]["distance"]["cfg"]["with_distance"] is True
    assert os.path.getsize(PF.GOLDEN) < 300 * 1024


@pytest.mark.parametrize("tag", ["base_legacy_train_max", "two_layer"])
def test_state_dict_keys_are_the_references(tag):
    mod, _, _, _ = PF.golden_case(tag)
    assert list(mod.state_dict().keys()) == PF.golden()[1]["cases"][tag]["keys"]
    assert "pfn_layers.0.linear.weight" in mod.state_dict()
    assert "pfn_layers.0.norm.num_batches_tracked" in mod.state_dict()


def test_pfn_layer_surface():
    from msmdfusion_amd.pillar_encoder import PFNLayer
    last = PFNLayer(10, 64, last_layer=True)
    mid = PFNLayer(10, 64, last_layer=False, mode="avg")
    assert last.units == 64 and mid.units == 32
    assert isinstance(last.norm, nn.BatchNorm1d) and last.norm.eps == 1e-3
    assert last.linear.bias is None and tuple(mid.linear.weight.shape) == (32, 10)
    x = torch.randn(7, 5, 10)
    num = torch.tensor([1, 2, 3, 4, 5, 5, 5])
    assert tuple(last(x, num).shape) == (7, 1, 64)
    y = mid(x, num)
    assert tuple(y.shape) == (7, 5, 64)          # point features, then the repeated reduction
    assert torch.equal(y[:, 0, 32:], y[:, 4, 32:])
    with pytest.raises(AssertionError):
        PFNLayer(10, 64, mode="min")


def test_single_pillar_keeps_two_dimensions():
    """The reference's bare .squeeze() returns [U] for N = 1; here [1, U]."""
    mod, (feats, num, coors), _, _ = PF.golden_case("base_legacy_eval_max")
    with torch.no_grad():
        out = mod(feats[:1], num[:1], coors[:1])
    assert tuple(out.shape) == (1, 64)


def test_registry_builds_the_pillar_modules_from_the_config():
    from msmdfusion_amd import configs as C
    from msmdfusion_amd.registry import build_middle_encoder, build_voxel_encoder
    m = C.TRANSFUSION_PILLAR_L["model"]
    enc = build_voxel_encoder(m["pts_voxel_encoder"])
    assert type(enc).__name__ == "PillarFeatureNet" and enc.takes_voxel_table
    assert enc.in_channels == 10 and enc.legacy and len(enc.pfn_layers) == 1
    assert enc.pfn_layers[0].units == 64 and enc.pfn_layers[0].mode == "max"
    assert abs(enc.x_offset - (-51.1)) < 1e-12 and enc.vx == 0.2
    mid = build_middle_encoder(m["pts_middle_encoder"])
    assert type(mid).__name__ == "PointPillarsScatter" and (mid.ny, mid.nx) == (512, 512)
    assert mid.in_channels == 64 and not hasattr(mid, "plan")
    dyn = build_voxel_encoder(dict(type="DynamicPillarFeatureNet", in_channels=5,
                                   feat_channels=[64], voxel_size=C.PILLAR_VOXEL_SIZE,
                                   point_cloud_range=C.PILLAR_POINT_CLOUD_RANGE))
    assert type(dyn).__name__ == "DynamicPillarFeatureNet"
    assert not getattr(dyn, "takes_voxel_table", False)


def test_pillar_config_equals_the_reference_dict():
    from msmdfusion_amd import configs as C
    fx = json.load(open(os.path.join(os.path.dirname(PF.GOLDEN), "reference_pillar_config.json")))
    norm = lambda o: json.loads(json.dumps(o))   # tuples -> lists
    assert norm(C.TRANSFUSION_PILLAR_L) == fx["transfusion_nusc_pillar_L"]


def test_build_head_takes_the_pillar_configs_head():
    from msmdfusion_amd import configs as C
    head = C.build_head(C.TRANSFUSION_PILLAR_L)
    lc = C.build_head()
    assert head.test_cfg["grid_size"] == [512, 512, 1] and head.test_cfg["out_size_factor"] == 4
    assert head.train_cfg["out_size_factor"] == 4
    assert lc.test_cfg["grid_size"] == [1440, 1440, 40]
    shape = lambda h: tuple(h.state_dict()["shared_conv.weight"].shape)
    assert shape(head)[1] == 384 and shape(lc)[1] == 512


def test_dynamic_pillar_feature_net_constructor_arithmetic():
    """in_channels grows by 3 + 2 (+ 1), later layers take point + voxel features
    (in_filters *= 2), keys are the reference's Sequential ones."""
    from msmdfusion_amd.pillar_encoder import DynamicPillarFeatureNet
    net = DynamicPillarFeatureNet(in_channels=4, feat_channels=(32, 64, 128), with_distance=True)
    assert net.in_channels == 10 and net.num_pfn == 3
    assert [tuple(l[0].weight.shape) for l in net.pfn_layers] == [(32, 10), (64, 64), (128, 128)]
    assert all(l[0].bias is None and isinstance(l[1], nn.BatchNorm1d) for l in net.pfn_layers)
    keys = list(net.state_dict().keys())
    assert "pfn_layers.0.0.weight" in keys and "pfn_layers.2.1.running_var" in keys
    assert net.pfn_scatter.reduce_type == "max" and net.cluster_scatter.reduce_type == "mean"
    assert DynamicPillarFeatureNet(mode="avg").pfn_scatter.reduce_type == "mean"
    bare = DynamicPillarFeatureNet(in_channels=5, with_cluster_center=False,
                                   with_voxel_center=False)
    assert bare.in_channels == 5


def test_c_abi_refuses_bad_pillar_arguments():
    """Null pointers and shapes outside the built kernels (K > 16, U > 128, M > 64) return a
    non-zero status before anything is launched."""
    from msmdfusion_amd._lib import lib
    p = ctypes.c_void_p(256)
    geo = (0.2, 0.2, -51.1, -51.1)

    def moments(n=4, m=20, c=5, flags=11, vox=p, mom=p, ws=p, nbytes=1 << 20):
        return lib.msmd_pillar_moments_f32(vox, p, p, n, m, c, flags, *geo, mom, ws, nbytes, None)

    def fwd(n=4, m=20, c=5, flags=11, u=64, w=p, out=p, arg=p, mode=1):
        return lib.msmd_pillar_pfn_fwd_f32(p, p, p, n, m, c, flags, *geo, w, p, p, u, mode, out,
                                           arg, None)

    def bwd(n=4, m=20, c=5, flags=11, u=64, go=p, sums=p, ws=p, nbytes=1 << 20):
        return lib.msmd_pillar_pfn_bwd_f32(p, p, p, n, m, c, flags, *geo, p, p, p, u, 1, go, p,
                                           sums, ws, nbytes, None)

    assert moments(vox=None) == -1 and moments(mom=None) == -1 and moments(n=-1) == -1
    assert moments(ws=None) == -2 and moments(nbytes=8) == -2
    assert moments(m=65) == -3 and moments(c=12, flags=7) == -3 and moments(m=0) == -1
    assert moments(c=2) == -1 and moments(flags=16) == -1
    assert fwd(w=None) == -1 and fwd(out=None) == -1 and fwd(arg=None) == -1
    assert fwd(u=129) == -3 and fwd(m=65) == -3 and fwd(c=12, flags=3) == -3 and fwd(u=0) == -1
    assert bwd(go=None) == -1 and bwd(sums=None) == -1 and bwd(ws=None) == -2
    assert bwd(u=129) == -3 and bwd(c=16, flags=1) == -3
    # N == 0: success, nothing launched (no pointer is looked at)
    assert moments(n=0, vox=None, ws=None) == 0 and fwd(n=0, w=None, out=None) == 0
    assert bwd(n=0, go=None, ws=None) == 0
    assert lib.msmd_pillar_workspace_bytes(60000, 20, 64) >= 512 * 64 * 17 * 8
    assert lib.msmd_pillar_workspace_bytes(10, 65, 64) == 0
