"""The PointNet++ op family with the reference's names, argument order and return dtypes
(mmdet3d/ops/{gather_points,group_points,interpolate,knn,furthest_point_sample,ball_query}).

Every op is a call into libmsmd_hip.so (csrc/pointnet.hip, csrc/points.hip); CPU tensors are
refused.  The three differentiable ops -- gather_points, grouping_operation,
three_interpolate -- share one backward: a by-source inverse of the index tensor, built on the
first backward only and kept on the autograd context, walked by a point-stationary kernel in a
fixed order (float32, no atomics: bitwise reproducible).  force_fp32 / auto_fp16 of the
reference are plain float32 here.
"""
import torch
from torch import nn
from torch.autograd import Function

from . import kernels as K


def furthest_point_sample(points_xyz, num_points):
    """(B, N, 3) -> int32 (B, num_points); furthest_point_sample.py:8-38."""
    return K.furthest_point_sample(points_xyz, num_points)


def furthest_point_sample_with_dist(points_dist, num_points):
    """(B, N, N) pairwise distances -> int32 (B, num_points); furthest_point_sample.py:41-74."""
    return K.furthest_point_sample_with_dist(points_dist, num_points)


def ball_query(min_radius, max_radius, sample_num, xyz, center_xyz):
    """-> int32 (B, npoint, sample_num); ball_query.py:14-40."""
    return K.ball_query(min_radius, max_radius, sample_num, xyz, center_xyz)


def calc_square_dist(point_feat_a, point_feat_b, norm=True):
    """furthest_point_sample/utils.py:4-31: (B, N, C), (B, M, C) -> (B, N, M) squared
    distances a^2 + b^2 - 2ab (norm: the root over the channel count)."""
    num_channel = point_feat_a.shape[-1]
    a_square = torch.sum(point_feat_a.unsqueeze(dim=2).pow(2), dim=-1)
    b_square = torch.sum(point_feat_b.unsqueeze(dim=1).pow(2), dim=-1)
    coor = torch.matmul(point_feat_a, point_feat_b.transpose(1, 2))
    dist = a_square + b_square - 2 * coor
    if norm:
        dist = torch.sqrt(dist) / num_channel
    return dist


class _InverseCache:
    """The by-source inverse of one index tensor: built on the first backward, reused by every
    later one (retain_graph, or the same object shared by several ops)."""
    __slots__ = ("indices", "num_src", "inverse")

    def __init__(self, indices, num_src):
        self.indices, self.num_src, self.inverse = indices, num_src, None

    def get(self):
        if self.inverse is None:
            self.inverse = K.point_inverse_index(self.indices, self.num_src)
        return self.inverse


class GatherPoints(Function):
    """features (B, C, N), indices (B, M) -> (B, C, M); gather_points.py:7-52."""

    @staticmethod
    def forward(ctx, features, indices):
        out = K.gather_points(features, indices)
        ctx.inv = _InverseCache(indices, features.shape[2])
        ctx.mark_non_differentiable(indices)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return K.point_scatter_backward(grad_out, ctx.inv.get()), None


class GroupingOperation(Function):
    """features (B, C, N), indices (B, npoint, nsample) -> (B, C, npoint, nsample);
    group_points.py:153-208."""

    @staticmethod
    def forward(ctx, features, indices):
        out = K.group_points(features, indices)
        ctx.inv = _InverseCache(indices, features.shape[2])
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return K.point_scatter_backward(grad_out, ctx.inv.get()), None


class ThreeNN(Function):
    """target (B, N, 3), source (B, M, 3) -> L2 distances (B, N, 3) float32 and indices
    (B, N, 3) int32 of the three nearest source points; three_nn.py:8-45."""

    @staticmethod
    def forward(ctx, target, source):
        dist2, idx = K.three_nn(target, source)
        ctx.mark_non_differentiable(idx)
        return torch.sqrt(dist2), idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None


class ThreeInterpolate(Function):
    """features (B, C, M), indices / weight (B, n, 3) -> (B, C, n);
    three_interpolate.py:8-63.  No gradient for weight or indices, as in the reference."""

    @staticmethod
    def forward(ctx, features, indices, weight):
        out = K.three_interpolate(features, indices, weight)
        ctx.inv = _InverseCache(indices, features.shape[2])
        ctx.weight = weight
        return out

    @staticmethod
    def backward(ctx, grad_out):
        grad = K.point_scatter_backward(grad_out, ctx.inv.get(), weight=ctx.weight,
                                        dest_per_out=3)
        return grad, None, None


class KNN(Function):
    """k, xyz (B, N, 3), center_xyz (B, npoint, 3) [transposed: (B, 3, N), (B, 3, npoint)] ->
    int64 (B, k, npoint), 0-based, nearest first, ties by index; knn.py:7-69.
    1 <= k <= 128 and k <= N."""

    @staticmethod
    def forward(ctx, k, xyz, center_xyz, transposed=False):
        assert k > 0
        if transposed:
            xyz = xyz.transpose(2, 1).contiguous()
            center_xyz = center_xyz.transpose(2, 1).contiguous()
        idx = K.knn(k, xyz, center_xyz)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None, None


gather_points = GatherPoints.apply
grouping_operation = GroupingOperation.apply
three_nn = ThreeNN.apply
three_interpolate = ThreeInterpolate.apply
knn = KNN.apply


class QueryAndGroup(nn.Module):
    """group_points.py:10-109: ball query around every centre, then grouped (xyz - centre)
    [/ max_radius] stacked above the grouped features: (B, 3 + C, npoint, sample_num)."""

    def __init__(self, max_radius, sample_num, min_radius=0, use_xyz=True,
                 return_grouped_xyz=False, normalize_xyz=False, uniform_sample=False,
                 return_unique_cnt=False):
        super().__init__()
        if uniform_sample:
            raise NotImplementedError(
                "QueryAndGroup(uniform_sample=True) is not built: the reference draws from the "
                "global RNG in a per-region Python loop (group_points.py:67-79), and no "
                "reference config sets it")
        assert not return_unique_cnt, "return_unique_cnt needs uniform_sample"
        self.max_radius = max_radius
        self.min_radius = min_radius
        self.sample_num = sample_num
        self.use_xyz = use_xyz
        self.return_grouped_xyz = return_grouped_xyz
        self.normalize_xyz = normalize_xyz
        self.uniform_sample = uniform_sample
        self.return_unique_cnt = return_unique_cnt

    def forward(self, points_xyz, center_xyz, features=None):
        idx = ball_query(self.min_radius, self.max_radius, self.sample_num, points_xyz,
                         center_xyz)
        xyz_trans = points_xyz.transpose(1, 2).contiguous()
        grouped_xyz = grouping_operation(xyz_trans, idx)      # (B, 3, npoint, sample_num)
        grouped_xyz = grouped_xyz - center_xyz.transpose(1, 2).unsqueeze(-1)
        if self.normalize_xyz:
            grouped_xyz = grouped_xyz / self.max_radius
        if features is not None:
            grouped_features = grouping_operation(features.contiguous(), idx)
            if self.use_xyz:
                new_features = torch.cat([grouped_xyz, grouped_features], dim=1)
            else:
                new_features = grouped_features
        else:
            assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
            new_features = grouped_xyz
        if self.return_grouped_xyz:
            return new_features, grouped_xyz
        return new_features


class GroupAll(nn.Module):
    """group_points.py:112-150: the whole cloud as one group, (B, C + 3, 1, N)."""

    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is not None:
            grouped_features = features.unsqueeze(2)
            if self.use_xyz:
                return torch.cat([grouped_xyz, grouped_features], dim=1)
            return grouped_features
        return grouped_xyz


class DFPS_Sampler(nn.Module):
    """FPS on the Euclidean distances of the points."""

    def forward(self, points, features, npoint):
        return furthest_point_sample(points.contiguous(), npoint)


class FFPS_Sampler(nn.Module):
    """FPS on feature distances (xyz stacked on the features)."""

    def forward(self, points, features, npoint):
        features_for_fps = torch.cat([points, features.transpose(1, 2)], dim=2)
        features_dist = calc_square_dist(features_for_fps, features_for_fps, norm=False)
        return furthest_point_sample_with_dist(features_dist, npoint)


class FS_Sampler(nn.Module):
    """F-FPS and D-FPS side by side."""

    def forward(self, points, features, npoint):
        features_for_fps = torch.cat([points, features.transpose(1, 2)], dim=2)
        features_dist = calc_square_dist(features_for_fps, features_for_fps, norm=False)
        fps_idx_ffps = furthest_point_sample_with_dist(features_dist, npoint)
        fps_idx_dfps = furthest_point_sample(points, npoint)
        return torch.cat([fps_idx_ffps, fps_idx_dfps], dim=1)


def get_sampler_type(sampler_type):
    samplers = {"D-FPS": DFPS_Sampler, "F-FPS": FFPS_Sampler, "FS": FS_Sampler}
    if sampler_type not in samplers:
        raise ValueError('Only "sampler_type" of "D-FPS", "F-FPS", or "FS"'
                         f" are supported, got {sampler_type}")
    return samplers[sampler_type]


class Points_Sampler(nn.Module):
    """points_sampler.py:34-99, range arithmetic included: sampler i works on the points
    [last_end, fps_sample_range) (-1: to the end), its indices are shifted by last_end, and
    last_end grows by fps_sample_range (so a -1 range moves it back by one, as there)."""

    def __init__(self, num_point, fps_mod_list=["D-FPS"], fps_sample_range_list=[-1]):
        super().__init__()
        assert len(num_point) == len(fps_mod_list) == len(fps_sample_range_list)
        self.num_point = num_point
        self.fps_sample_range_list = fps_sample_range_list
        self.samplers = nn.ModuleList()
        for fps_mod in fps_mod_list:
            self.samplers.append(get_sampler_type(fps_mod)())
        self.fp16_enabled = False

    def forward(self, points_xyz, features):
        indices = []
        last_fps_end_index = 0
        for fps_sample_range, sampler, npoint in zip(self.fps_sample_range_list, self.samplers,
                                                     self.num_point):
            assert fps_sample_range < points_xyz.shape[1]
            if fps_sample_range == -1:
                sample_points_xyz = points_xyz[:, last_fps_end_index:]
                sample_features = features[:, :, last_fps_end_index:] \
                    if features is not None else None
            else:
                sample_points_xyz = points_xyz[:, last_fps_end_index:fps_sample_range]
                sample_features = features[:, :, last_fps_end_index:fps_sample_range] \
                    if features is not None else None
            fps_idx = sampler(sample_points_xyz.contiguous(), sample_features, npoint)
            indices.append(fps_idx + last_fps_end_index)
            last_fps_end_index += fps_sample_range
        return torch.cat(indices, dim=1)
