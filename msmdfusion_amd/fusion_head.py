"""TransFusionHead with its image-fusion stages (`fuse_img=True`): the head of the reference's
"LC" configs (configs/transfusion_nusc_voxel_LC.py, transfusion_nusc_pillar_LC.py,
transfusion_waymo_voxel_LC.py).

Reference: mmdet3d/models/dense_heads/transfusion_head.py -- the extra modules of
TransFusionHead.__init__ (:712-745) and forward_single (:797-1032):

    image -> BEV      max over the image height, `fc`, then one cross-only decoder layer per
                      view painting the flattened BEV map (:817-834); torch / rocBLAS
    query init        the mean of the LiDAR and the painted heat map (:839-874)
    LiDAR decoder     as in the LiDAR head (:883-898)
    image stage       per (sample, view): project the queries and their box corners, keep the
                      queries on the image, attend into that view's feature map under a
                      Gaussian log-mask around each query (:903-1004)
    prediction        FFN over [query_feat, prev_query_feat] (:1007-1008), queries that no
                      view sees restored from the LiDAR layer's result (:1009-1011)

The image stage has two paths.  `fused=False` is the reference's double loop, op for op, with
its host reads; it runs anywhere and is the oracle of tests/golden/img_fusion_vectors.npz.
`fused=True` (taken on the GPU in float32 for the head widths the kernels are built for) runs
the geometry of all (sample, view, query) triples in one launch (csrc/img_fusion.hip), the
self-attention of all groups as one batched call, the Gaussian-window attention in a native
kernel that never forms the [n, H W] mask, and the row-wise remainder once over [B P] rows,
without reading anything back.

Two quirks of the reference are kept: the reversed 3-D flow is SKIPPED for batch_size == 1
(:946-949, "skip during inference"), and the collapsed position grid is rebuilt on every call
(:827-830 store it under a misspelt attribute).
"""
import copy

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import fusion_layers as FL
from .head import (FFN, PositionEmbeddingLearned, TransformerDecoderLayer, TransFusionHead)
from .registry import HEADS


def box_corners(boxes):
    """LiDARInstance3DBoxes.corners (lidar_box3d.py:46-84) on [N, 7] boxes of any float dtype
    -> [N, 8, 3]."""
    dims = boxes[:, 3:6]
    unit = torch.tensor([[-0.5, -0.5, 0], [-0.5, -0.5, 1], [-0.5, 0.5, 1], [-0.5, 0.5, 0],
                         [0.5, -0.5, 0], [0.5, -0.5, 1], [0.5, 0.5, 1], [0.5, 0.5, 0]],
                        dtype=boxes.dtype).to(boxes.device)
    corners = dims.view([-1, 1, 3]) * unit.reshape([1, 8, 3])
    rot_sin, rot_cos = torch.sin(boxes[:, 6]), torch.cos(boxes[:, 6])
    ones, zeros = torch.ones_like(rot_cos), torch.zeros_like(rot_cos)
    rot_mat_t = torch.stack([torch.stack([rot_cos, -rot_sin, zeros]),
                             torch.stack([rot_sin, rot_cos, zeros]),
                             torch.stack([zeros, zeros, ones])])
    corners = torch.einsum("aij,jka->aik", (corners, rot_mat_t))
    return corners + boxes[:, :3].view(-1, 1, 3)


def geometry_params(img_metas, num_views, skip_flow):
    """float64 [B, V, 20]: msmd_point_sample_params per (sample, view) -- sample_params of the
    sample's meta with lidar2img[view]; skip_flow drops the 3-D flow (the batch-size-1 quirk)."""
    out = np.empty((len(img_metas), num_views, 20), np.float64)
    for b, meta in enumerate(img_metas):
        l2i = [FL._meta_array(m) for m in meta["lidar2img"]]
        base = dict(meta)
        if skip_flow:
            base["transformation_3d_flow"] = []
        for v in range(num_views):
            out[b, v] = FL.sample_params(dict(base, lidar2img=l2i[v]))
    return out


def bn_momentum_chain(bn, means, unbiased_vars, valid):
    """What `k` training-mode calls of a BatchNorm leave in its running statistics, in closed
    form: call j (the j-th group with valid[g], in order) does r <- (1 - m) r + m s_j, so
    r_k = (1 - m)^k r_0 + m sum_j (1 - m)^(k - 1 - j) s_j.  means / unbiased_vars [G, C],
    valid [G] bool, all on the device; k is never read back.  num_batches_tracked += k."""
    with torch.no_grad():
        m = bn.momentum
        vf = valid.to(means.dtype)
        k = vf.sum()
        rank = torch.cumsum(vf, 0) - 1
        w = torch.where(valid, m * (1 - m) ** (k - 1 - rank), torch.zeros_like(vf))   # [G]
        decay = (1 - m) ** k
        zero = torch.zeros_like(means)
        mean_sum = (w[:, None] * torch.where(valid[:, None], means.detach(), zero)).sum(0)
        var_sum = (w[:, None] * torch.where(valid[:, None], unbiased_vars.detach(), zero)).sum(0)
        bn.running_mean.mul_(decay).add_(mean_sum.to(bn.running_mean.dtype))
        bn.running_var.mul_(decay).add_(var_sum.to(bn.running_var.dtype))
        bn.num_batches_tracked.add_(valid.sum())


def posembed_groups(pe, pos, member, valid):
    """PositionEmbeddingLearned over G independent groups at once.  pos [G, N, 2], member
    [G, N] bool (the positions that belong to the group), valid [G] bool (the groups the
    reference calls the module for).  -> [G, N, C]; rows that are no members are zero.  In
    training mode every group is normalised with its own members' statistics and the running
    statistics get one momentum update per valid group, in group order (bn_momentum_chain)."""
    conv1, bn, _, conv2 = pe.position_embedding_head
    sel = member[..., None]
    pos = torch.where(sel, pos, torch.zeros_like(pos))          # selected, never multiplied
    x = F.linear(pos, conv1.weight[:, :, 0], conv1.bias)
    zero = torch.zeros_like(x)
    if bn.training:
        n = member.sum(1).clamp(min=2).to(x.dtype)[:, None]                  # [G, 1]
        mean = torch.where(sel, x, zero).sum(1) / n
        d = torch.where(sel, x - mean[:, None], zero)
        var = (d * d).sum(1) / n
        bn_momentum_chain(bn, mean, var * n / (n - 1), valid)
        y = d * torch.rsqrt(var + bn.eps)[:, None]
    else:
        y = (x - bn.running_mean) * torch.rsqrt(bn.running_var + bn.eps)
    y = F.relu(y * bn.weight + bn.bias)
    y = F.linear(y, conv2.weight[:, :, 0], conv2.bias)
    return torch.where(sel, y, zero)


def posembed_repeated(pe, pos, calls):
    """PositionEmbeddingLearned on the same positions `calls` times (a device tensor): one
    evaluation; in training mode the running statistics move as after `calls` identical
    updates, r <- (1 - m)^k r + (1 - (1 - m)^k) s.  pos [1, N, 2] -> [1, N, C]."""
    conv1, bn, _, conv2 = pe.position_embedding_head
    x = F.linear(pos, conv1.weight[:, :, 0], conv1.bias)
    if bn.training:
        n = x.shape[1]
        mean = x.mean(1)
        d = x - mean[:, None]
        var = (d * d).mean(1)
        with torch.no_grad():
            decay = (1 - bn.momentum) ** calls.to(x.dtype)
            unbiased = var[0] * (n / max(n - 1, 1))
            bn.running_mean.mul_(decay).add_(((1 - decay) * mean[0]).to(bn.running_mean.dtype))
            bn.running_var.mul_(decay).add_(((1 - decay) * unbiased).to(bn.running_var.dtype))
            bn.num_batches_tracked.add_(calls.to(bn.num_batches_tracked.dtype))
        y = d * torch.rsqrt(var + bn.eps)[:, None]
    else:
        y = (x - bn.running_mean) * torch.rsqrt(bn.running_var + bn.eps)
    y = F.relu(y * bn.weight + bn.bias)
    return F.linear(y, conv2.weight[:, :, 0], conv2.bias)


class _NativeBatchNorm:
    """BatchNorm through torch's own kernels instead of MIOpen's.  MIOpen's training-mode
    statistics lose digits where the mean is large beside the spread -- the position grids
    (0 .. 180) behind the position embeddings: the running variance of a cross-only layer's
    `cross_posembed` came out 4.5e-05 off float64 where the same operation on a CPU is 1.3e-06
    off, and the painted heat map inherited it.  Same parameters, buffers and state-dict keys."""

    def forward(self, x):
        with torch.backends.cudnn.flags(enabled=False):
            return super().forward(x)


class NativeBatchNorm1d(_NativeBatchNorm, nn.BatchNorm1d):
    pass


class NativeBatchNorm2d(_NativeBatchNorm, nn.BatchNorm2d):
    pass


def use_native_batchnorm(module):
    """Replace every nn.BatchNorm1d / 2d below `module` by its native-kernel form, in place."""
    for name, child in module.named_children():
        cls = {nn.BatchNorm1d: NativeBatchNorm1d, nn.BatchNorm2d: NativeBatchNorm2d}.get(type(child))
        if cls is None:
            use_native_batchnorm(child)
            continue
        new = cls(child.num_features, eps=child.eps, momentum=child.momentum, affine=child.affine,
                  track_running_stats=child.track_running_stats)
        new.load_state_dict(child.state_dict())
        setattr(module, name, new.to(child.weight.device if child.affine else "cpu"))
    return module


def group_self_attention(attn, x, pad):
    """nn.MultiheadAttention `attn` as self-attention inside G independent groups, written out:
    x [G, N, C], pad [G, N] bool (keys to ignore) -> [G, N, C].  The module's own forward picks
    among attention back ends by mode and mask, some of which read the mask back; these few
    plain operations do not."""
    G, N, C = x.shape
    h = attn.num_heads
    d = C // h
    q, k, v = F.linear(x, attn.in_proj_weight, attn.in_proj_bias).chunk(3, dim=-1)
    q, k, v = (t.reshape(G, N, h, d).transpose(1, 2) for t in (q, k, v))          # [G, h, N, d]
    s = (q * d ** -0.5) @ k.transpose(-1, -2)
    s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    p = F.dropout(torch.softmax(s, dim=-1), attn.dropout, attn.training)
    return attn.out_proj((p @ v).transpose(1, 2).reshape(G, N, C))


@HEADS.register_module()
class TransFusionHeadLC(TransFusionHead):
    """transfusion_head.py:594-1379 with fuse_img=True (see the module docstring).  Parameters
    and state-dict keys are the reference's: `shared_conv_img`, `heatmap_head_img`,
    `decoder.{L}` (the image layer), `decoder.{L+1 .. L+V}` (cross-only, one per view), `fc.0`,
    `prediction_heads.{L}` (2 x hidden input channels)."""

    def __init__(self, fuse_img=True, num_views=0, in_channels_img=64, out_size_factor_img=4,
                 hidden_channel=128, num_heads=8, ffn_channel=256, dropout=0.1, activation="relu",
                 common_heads=None, num_heatmap_convs=2, bias="auto", initialize_by_heatmap=False,
                 learnable_query_pos=False, fused=True, **kw):
        if not fuse_img:
            raise ValueError("TransFusionHeadLC is the fuse_img=True head; build TransFusionHead "
                             "for the LiDAR branch alone")
        if int(num_views) < 1:
            raise ValueError("TransFusionHeadLC needs num_views >= 1, got %r" % (num_views,))
        if not initialize_by_heatmap:
            raise NotImplementedError(
                "TransFusionHeadLC: fuse_img needs initialize_by_heatmap=True (the reference "
                "copies heatmap_head into heatmap_head_img, :724)")
        if learnable_query_pos:
            raise NotImplementedError("TransFusionHeadLC: learnable_query_pos is not built")
        super().__init__(fuse_img=False, hidden_channel=hidden_channel, num_heads=num_heads,
                         ffn_channel=ffn_channel, dropout=dropout, activation=activation,
                         common_heads=common_heads, num_heatmap_convs=num_heatmap_convs, bias=bias,
                         initialize_by_heatmap=True, learnable_query_pos=False, **kw)
        self.fuse_img, self.fused = True, bool(fused)
        self.num_views, self.out_size_factor_img = int(num_views), out_size_factor_img
        self.num_heads = num_heads
        self.shared_conv_img = nn.Conv2d(in_channels_img, hidden_channel, 3, padding=1,
                                         bias=bool(bias))
        self.heatmap_head_img = copy.deepcopy(self.heatmap_head)

        def layer(cross_only=False):
            return TransformerDecoderLayer(
                hidden_channel, num_heads, ffn_channel, dropout, activation,
                self_posembed=PositionEmbeddingLearned(2, hidden_channel),
                cross_posembed=PositionEmbeddingLearned(2, hidden_channel), cross_only=cross_only)
        self.decoder.append(layer())
        for _ in range(self.num_views):
            self.decoder.append(layer(cross_only=True))
        self.fc = nn.Sequential(nn.Conv1d(hidden_channel, hidden_channel, kernel_size=1))
        heads = copy.deepcopy(common_heads or {})
        heads.update(dict(heatmap=(self.num_classes, num_heatmap_convs)))
        self.prediction_heads.append(FFN(hidden_channel * 2, heads, bias=bias))
        use_native_batchnorm(self)
        self.init_weights()                  # (:747: after every module exists)
        self.on_the_image_mask = None
        self._img_pos_cache = {}

    # ------------------------------------------------------------------ helpers
    def _img_feat_pos(self, h, w, device, dtype):
        """create_2D_grid(h, w) on the device (:907-911 cache the first call's grid)."""
        key = (h, w, device, dtype)
        if key not in self._img_pos_cache:
            self._img_pos_cache = {key: self.create_2D_grid(h, w).to(device=device, dtype=dtype)}
        return self._img_pos_cache[key]

    def fused_ok(self, query_feat, img_feat):
        """Whether the image stage takes the native path: float32 on the GPU, a head width the
        window-attention kernels are built for, P and V within the geometry kernel's range."""
        if not (self.fused and query_feat.is_cuda and query_feat.dtype == torch.float32
                and img_feat.dtype == torch.float32):
            return False
        from . import kernels as K
        return K.gauss_attn_supported(query_feat.shape[1], self.num_heads) and \
            self.num_proposals <= K.IMG_GEOMETRY_MAX_QUERIES and \
            self.num_views <= K.IMG_GEOMETRY_MAX_VIEWS

    # ------------------------------------------------------------------ the image stage
    def _image_stage_composed(self, prev_query_feat, query_pos_3d, pred_boxes, img_feat_flatten,
                              img_feat_pos, img_metas):
        """:930-1006, the reference's loop (host reads included)."""
        B, P = prev_query_feat.shape[0], self.num_proposals
        layer = self.decoder[self.num_decoder_layers]
        osf = self.out_size_factor_img
        query_feat = torch.zeros_like(prev_query_feat)
        on_the_image_mask = torch.ones([B, P]).to(query_pos_3d.device) * -1
        for b in range(B):
            meta = img_metas[b]
            lidar2img_rt = query_pos_3d.new_tensor(np.asarray(meta["lidar2img"]))
            scale = query_pos_3d.new_tensor(meta["scale_factor"][:2]
                                            if "scale_factor" in meta else [1.0, 1.0])
            flip = meta["flip"] if "flip" in meta else False
            crop = query_pos_3d.new_tensor(meta["img_crop_offset"]) \
                if "img_crop_offset" in meta else 0
            img_shape, pad_shape = meta["img_shape"][:2], meta["input_shape"][:2]
            corners = box_corners(pred_boxes[b][:, :7])
            pts = torch.cat([query_pos_3d[b], corners.permute(2, 0, 1).reshape(3, -1)], dim=-1)
            if B == 1:                      # QUIRK (:946): no reversed 3-D flow at batch size 1
                points = pts.T
            else:
                points = FL.apply_3d_transformation(pts.T, "LIDAR", meta, reverse=True).detach()
            num_points = points.shape[0]
            for v in range(self.num_views):
                pts_4d = torch.cat([points, points.new_ones(size=(num_points, 1))], dim=-1)
                pts_2d = pts_4d @ lidar2img_rt[v].t()
                depth = torch.clamp(pts_2d[:, 2:3], min=1e-5)
                img_coors = pts_2d[:, 0:2] / depth * scale - crop
                coor_x, coor_y = torch.split(img_coors, 1, dim=1)
                if flip:
                    coor_x = img_shape[1] - coor_x
                coor_x, corner_x = coor_x[:P], coor_x[P:].reshape(P, 8, 1)
                coor_y, corner_y = coor_y[:P], coor_y[P:].reshape(P, 8, 1)
                corner_xy = torch.cat([corner_x, corner_y], dim=-1)
                h, w = pad_shape
                on = ((coor_x > 0) * (coor_x < w) * (coor_y > 0) * (coor_y < h)).reshape(-1)
                if on.sum() <= 1:           # (a host read, as in the reference)
                    continue
                on_the_image_mask[b, on] = v
                center_ys, center_xs = coor_y[on] / osf, coor_x[on] / osf
                centers = torch.cat([center_xs, center_ys], dim=-1).int()
                extent = (corner_xy[on].max(1).values - corner_xy[on].min(1).values) / osf
                radius = torch.ceil(extent.norm(dim=-1, p=2) / 2).int()
                sigma = (radius * 2 + 1) / 6.0
                distance = (centers[:, None, :] - (img_feat_pos - 0.5)).norm(dim=-1) ** 2
                gaussian_mask = (-distance / (2 * sigma[:, None] ** 2)).exp()
                gaussian_mask[gaussian_mask < torch.finfo(torch.float32).eps] = 0
                attn_mask = gaussian_mask.log().to(prev_query_feat.dtype)
                query_pos_view = torch.cat([center_xs, center_ys], dim=-1)
                out = layer(prev_query_feat[b, :, on][None], img_feat_flatten[b:b + 1, v],
                            query_pos_view[None], img_feat_pos, attn_mask=attn_mask)
                query_feat = _put_columns(query_feat, b, on, out[0])      # (:1004)
        return query_feat, on_the_image_mask != -1

    def _image_stage_fused(self, prev_query_feat, query_pos_3d, pred_boxes, img_feat_flatten,
                           img_feat_pos, img_metas, img_hw):
        """The same result without the loop and without host reads (module docstring)."""
        from . import kernels as K
        B, C, P = prev_query_feat.shape
        V, heads = self.num_views, self.num_heads
        H, W = img_hw
        layer = self.decoder[self.num_decoder_layers]
        dev = prev_query_feat.device
        params = torch.from_numpy(geometry_params(img_metas, V, skip_flow=B == 1).astype(
            np.float32)).to(dev, non_blocking=True)
        boxes = torch.stack([b[:, :7] for b in pred_boxes]).float().contiguous()
        geo = K.img_query_geometry(query_pos_3d.float().contiguous(), boxes, params,
                                   float(self.out_size_factor_img))
        member = geo.on & geo.valid[:, :, None]                               # [B, V, P]
        valid = geo.valid.reshape(B * V)
        has = geo.mask                                                        # [B, P]
        win = geo.winner.long().clamp(min=0)                                  # [B, P]

        # position embeddings: every (sample, view) group with its own BatchNorm statistics
        q_pos = posembed_groups(layer.self_posembed, geo.pos.reshape(B * V, P, 2),
                                member.reshape(B * V, P), valid).reshape(B, V, P, C)
        k_pos = posembed_repeated(layer.cross_posembed, img_feat_pos, valid.sum())  # [1, HW, C]

        # self-attention inside every group: members are the keys, winners' rows are kept
        prev = prev_query_feat.permute(0, 2, 1)                               # [B, P, C]
        x = torch.where(member[..., None], prev[:, None] + q_pos, torch.zeros_like(q_pos))
        x = x.reshape(B * V, P, C)
        pad = (~member).reshape(B * V, P) & valid[:, None]      # a skipped group masks nothing
        sa = group_self_attention(layer.self_attn, x, pad).reshape(B, V, P, C)
        pick = win[:, None, :, None].expand(B, 1, P, C)
        sa_w, q_pos_w = sa.gather(1, pick)[:, 0], q_pos.gather(1, pick)[:, 0]  # [B, P, C]
        query = layer.norm1(prev + layer.dropout1(sa_w))

        # Gaussian-window cross-attention: projections in rocBLAS, the rest in the kernel
        attn = layer.multihead_attn
        wq, wk, wv = attn.in_proj_weight.chunk(3)
        bq, bk, bv = attn.in_proj_bias.chunk(3)
        kv = img_feat_flatten.permute(0, 1, 3, 2).reshape(B * V, H * W, C) + k_pos
        q_proj = F.linear(query + q_pos_w, wq, bq).reshape(B * P, C)
        p_drop = float(attn.dropout) if self.training else 0.0
        # (a host-side draw: the seed is a kernel argument, nothing is read from the device)
        seed = int(torch.empty((), dtype=torch.int64).random_()) if p_drop > 0 else 0
        view = torch.where(has, geo.winner, torch.full_like(geo.winner, -1)).reshape(B * P)
        ctx = K.gauss_attn(q_proj, F.linear(kv, wk, bk), F.linear(kv, wv, bv), view.contiguous(),
                           geo.win_centre.reshape(B * P, 2), geo.win_sigma.reshape(B * P), V, H, W,
                           heads, p_drop, seed)
        attended = attn.out_proj(ctx).reshape(B, P, C)
        query = layer.norm2(query + layer.dropout2(attended))
        ffn = layer.linear2(layer.dropout(layer.activation(layer.linear1(query))))
        query = layer.norm3(query + layer.dropout3(ffn))
        query = torch.where(has[..., None], query, torch.zeros_like(query))
        return query.permute(0, 2, 1), has

    # ------------------------------------------------------------------ forward
    def forward_single(self, inputs, img_inputs=None, img_metas=None):
        """:797-1032 with fuse_img.  inputs [B, C, H, W]; img_inputs [B * num_views, C_img, h, w]
        (left untouched); img_metas: per sample lidar2img [V, 4, 4], input_shape, img_shape and
        the optional scale_factor / flip / img_crop_offset / 3-D flow keys."""
        if img_inputs is None or img_metas is None:
            raise ValueError("TransFusionHeadLC.forward_single needs img_inputs and img_metas")
        B, V = inputs.shape[0], self.num_views
        if img_inputs.shape[0] != B * V or len(img_metas) != B:
            raise ValueError("img_inputs must be [B * num_views = %d, C, h, w] with %d metas, got "
                             "%s and %d" % (B * V, B, tuple(img_inputs.shape), len(img_metas)))
        lidar_feat, rows, grid = self._shared_conv(inputs)
        C = lidar_feat.shape[1]
        flat = lidar_feat.reshape(B, C, -1)
        bev_pos = self._bev_pos_on(lidar_feat.device, B).to(lidar_feat.dtype)

        # image -> BEV (:817-834)
        img_feat = self.shared_conv_img(img_inputs)
        img_h, img_w = img_inputs.shape[-2], img_inputs.shape[-1]
        raw_img_feat = img_feat.view(B, V, C, img_h, img_w).permute(0, 2, 3, 1, 4)
        collapsed = raw_img_feat.reshape(B, C, img_h, img_w * V).max(2).values
        collapsed = self.fc(collapsed).view(B, C, img_w * V)
        # QUIRK (:827-830): this grid is rebuilt on every call
        collapsed_pos = self.create_2D_grid(1, collapsed.shape[-1]).to(img_feat.dtype).to(
            img_feat.device, non_blocking=True)                 # (no blocking copy, though)
        bev_feat = flat
        first = self.num_decoder_layers + 1
        for v in range(V):
            cut = slice(img_w * v, img_w * (v + 1))
            bev_feat = self.decoder[first + v](bev_feat, collapsed[..., cut], bev_pos,
                                               collapsed_pos[:, cut])

        # image guided query initialisation (:839-874)
        dense_heatmap = self._heatmap(lidar_feat, rows, grid)
        dense_heatmap_img = self.heatmap_head_img(bev_feat.reshape(lidar_feat.shape))
        heatmap = (dense_heatmap.detach().sigmoid() + dense_heatmap_img.detach().sigmoid()) / 2
        pad = self.nms_kernel_size // 2
        local_max = torch.zeros_like(heatmap)
        inner = F.max_pool2d(heatmap, kernel_size=self.nms_kernel_size, stride=1, padding=0)
        local_max[:, :, pad:heatmap.shape[2] - pad, pad:heatmap.shape[3] - pad] = inner
        for c in {"nuScenes": (8, 9), "Waymo": (1, 2)}.get(self.test_cfg["dataset"], ()):
            local_max[:, c] = heatmap[:, c]
        heatmap = (heatmap * (heatmap == local_max)).reshape(B, heatmap.shape[1], -1)
        top = heatmap.reshape(B, -1).argsort(dim=-1, descending=True)[..., :self.num_proposals]
        top_class, top_index = top // heatmap.shape[-1], top % heatmap.shape[-1]
        query_feat = flat.gather(index=top_index[:, None, :].expand(-1, C, -1), dim=-1)
        self.query_labels = top_class
        one_hot = F.one_hot(top_class, num_classes=self.num_classes).permute(0, 2, 1)
        query_feat = query_feat + self.class_encoding(one_hot.to(query_feat.dtype))
        query_pos = bev_pos.gather(
            index=top_index[:, None, :].permute(0, 2, 1).expand(-1, -1, bev_pos.shape[-1]), dim=1)

        # LiDAR decoder layers (:883-898)
        for i in range(self.num_decoder_layers):
            query_feat = self.decoder[i](query_feat, flat, query_pos, bev_pos)
            res_layer = self.prediction_heads[i](query_feat)
            res_layer["center"] = res_layer["center"] + query_pos.permute(0, 2, 1)
            first_res_layer = res_layer
            query_pos = res_layer["center"].detach().clone().permute(0, 2, 1)

        # image stage (:903-1006)
        img_feat_flatten = raw_img_feat.permute(0, 3, 1, 2, 4).reshape(B, V, C, -1)
        img_feat_pos = self._img_feat_pos(img_h, img_w, img_feat.device, img_feat.dtype)
        prev_query_feat = query_feat.detach().clone()
        cfg = self.test_cfg
        realmetric = query_pos.permute(0, 2, 1) * cfg["out_size_factor"] * cfg["voxel_size"][0] \
            + cfg["pc_range"][0]
        query_pos_3d = torch.cat([realmetric, res_layer["height"]], dim=1).detach().clone()
        vel = res_layer["vel"].detach() if "vel" in res_layer else None
        decoded = self.bbox_coder.decode(
            res_layer["heatmap"].detach(), res_layer["rot"].detach(), res_layer["dim"].detach(),
            res_layer["center"].detach(), res_layer["height"].detach(), vel)
        pred_boxes = [d["bboxes"] for d in decoded]
        if self.fused_ok(prev_query_feat, img_feat):
            query_feat, mask = self._image_stage_fused(
                prev_query_feat, query_pos_3d, pred_boxes, img_feat_flatten, img_feat_pos,
                img_metas, (img_h, img_w))
        else:
            query_feat, mask = self._image_stage_composed(
                prev_query_feat, query_pos_3d, pred_boxes, img_feat_flatten, img_feat_pos,
                img_metas)
        self.on_the_image_mask = mask

        # prediction over [query_feat, prev_query_feat], off-image queries restored (:1007-1011)
        res_layer = self.prediction_heads[self.num_decoder_layers](
            torch.cat([query_feat, prev_query_feat], dim=1))
        res_layer["center"] = res_layer["center"] + query_pos.permute(0, 2, 1)
        for key, value in res_layer.items():
            res_layer[key] = torch.where(mask[:, None, :], value, first_res_layer[key])
        res_layer["query_heatmap_score"] = heatmap.gather(
            index=top_index[:, None, :].expand(-1, self.num_classes, -1), dim=-1)
        res_layer["dense_heatmap"] = dense_heatmap_img
        return [res_layer]

    def forward(self, feats, img_feats=None, img_metas=None):
        """:1034-1049 -- one level of each: `([dict],)`."""
        if isinstance(feats, torch.Tensor):
            feats = [feats]
        if isinstance(img_feats, torch.Tensor):
            img_feats = [img_feats]
        if img_feats is None:
            raise ValueError("TransFusionHeadLC.forward needs img_feats (fuse_img=True)")
        if len(feats) != 1:
            raise AssertionError("only support one level features.")
        return ([self.forward_single(feats[0], img_feats[0], img_metas)[0]],)


def _put_columns(query_feat, b, on, out):
    """query_feat[b, :, on] = out (:1004), out of place so the graph stays differentiable."""
    full = torch.zeros_like(query_feat[b])
    full[:, on] = out
    keep = on[None, :].expand_as(full)
    new_b = torch.where(keep, full, query_feat[b])
    return torch.cat([query_feat[:b], new_b[None], query_feat[b + 1:]], dim=0)
