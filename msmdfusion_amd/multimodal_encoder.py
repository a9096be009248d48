"""SparseMultiModalEncoderPaint: the Gated Modality-Aware (GMA-Conv) fusion
stack (mmdet3d/models/middle_encoders/sparse_multimodal_encoder_painting.py:
99-459; layer table in SURVEY Appendix A.2).

Same constructor, same module tree (including grouped_sp_conv_blocks_2D / _mix,
which the reference builds but never calls, :142-156,413-428 -- kept so
checkpoints load), same forward signature and return value.  The neighbour
search (fps_NN_fast, :276-323) runs entirely on the GPU through the C ABI:
FPS -> nearest LiDAR voxel of each representative -> ball query -> assignment,
no [1,2048,N,3] broadcast temporaries and no host round trip.

Documented deviations from the reference:
  * B.4 batch offsets are cumulative (the reference's are right only for
    batch <= 2; identical results there) unless `reference_quirks` is set;
  * B.5 the per-call random `dummy_embedding` (:372) comes from
    `self.dummy_embedding_fn` so tests can pin it;
  * B.6 a query covered by several balls takes the highest representative
    index (what a sequential index_put_ leaves).
"""
import os

import torch
from torch import nn
from torch.nn import functional as F

from . import kernels as K
from . import spconv
from .registry import MIDDLE_ENCODERS
from .sparse_block import SparseBasicBlock, make_sparse_convmodule
from .spconv import functional as Fsp


def drop_mix_column(idx5):
    """(b, mix, z, y, x) -> (b, z, y, x) rows, contiguous.  As two slices and a cat: `idx5[:,
    [0, 2, 3, 4]]` -- the reference's spelling -- makes torch build the column list on the
    host and copy it to the device with a BLOCKING pageable transfer at every call, i.e. the
    host waits for the whole stream (five such waits per stage of the index pass:
    tools/lc_sampler.py had 2 ms of the prepare thread's 12.6 ms in them)."""
    return torch.cat([idx5[:, :1], idx5[:, 2:]], 1)


def pinned_dummy_embedding(c, device):
    """The reference's per-call random embedding for uncovered 2D voxels
    (sparse_multimodal_encoder_painting.py:372: `torch.rand(1, c).to(device)`): the same
    draw from the CPU generator, sent through a pinned buffer without blocking -- the
    pageable copy made the host wait for the stream four times per step (1.35 ms)."""
    v = torch.rand(1, c)
    if torch.device(device).type != "cuda":
        return v.to(device)
    return v.pin_memory().to(device, non_blocking=True)


def fps_nn_fast(query, key, fps_num, radius, max_cluster_samples, dist_thresh):
    """Nearest key voxel of every query voxel of ONE sample (:276-323).
    query/key are (b,z,y,x) int32 rows; returns long[nq], -1 = none."""
    nq = query.shape[0]
    q_zyx = query[:, 1:].contiguous()
    k_zyx = key[:, 1:].contiguous()
    if nq == 0:
        return torch.zeros((0,), dtype=torch.long, device=query.device)
    if nq <= fps_num:
        return K.nn_search(q_zyx, k_zyx, dist_thresh).long()
    q_f = q_zyx.float().unsqueeze(0)
    rep_idx = K.furthest_point_sample(q_f, fps_num)[0].long()
    rep = q_zyx[rep_idx]
    rep_nn = K.nn_search(rep, k_zyx, dist_thresh)
    group = K.ball_query(0, radius, max_cluster_samples, q_f, rep.float().unsqueeze(0))[0]
    return K.nn_assign(group, rep_nn, nq).long()


@MIDDLE_ENCODERS.register_module()
class SparseMultiModalEncoderPaint(nn.Module):

    def __init__(self, in_channels_3D=(16, 32, 64, 128), in_channels_2D=(259, 259, 259, 259),
                 out_channels=(32, 64, 128, 128), padding=(1, 1, 1, [0, 1, 1]),
                 down_kernel_size=(3, 3, 3, [3, 1, 1]), down_stride=(2, 2, 2, [2, 1, 1]),
                 order=("conv", "norm", "act"),
                 norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01), block_type="conv_module"):
        super().__init__()
        assert block_type in ["conv_module", "basicblock"]
        self.in_channels_3D = in_channels_3D
        self.in_channels_2D = in_channels_2D
        self.out_channels = out_channels
        self.padding = padding
        self.down_kernel_size = down_kernel_size
        self.down_stride = down_stride
        self.order = order
        self.fp16_enabled = False
        # one-launch stage assembly (kernels.gma_assemble); MSMD_FUSED_ASSEMBLY=0: the op chain
        self.fused_assembly = os.environ.get("MSMD_FUSED_ASSEMBLY", "1") != "0"
        # the gate linears inside that launch (kernels.gma_stage); False: rows_linear tables
        self.fused_gates = True
        # True (set by SparseFusionPath / the detector's `reference_quirks`): batch offsets of
        # the nearest-voxel rows as the reference computes them (:355-369: the PREVIOUS
        # sample's count only) instead of cumulative ones; the same rows for batch <= 2
        self.reference_quirks = False
        self.dummy_embedding_fn = pinned_dummy_embedding
        self.make_grouped_sparse_conv_blocks(norm_cfg)
        self.make_aggregation_block(norm_cfg)
        self.make_downscale_block(norm_cfg)

    # ---- construction (:124-206) -------------------------------------------------
    def make_grouped_sparse_conv_blocks(self, norm_cfg, conv_cfg=dict(type="SubMConv3d")):
        self.grouped_sp_conv_blocks_3D = spconv.SparseSequential()
        self.grouped_sp_conv_blocks_2D = spconv.SparseSequential()
        self.grouped_sp_conv_blocks_mix = spconv.SparseSequential()
        gates, cross_gates = [], []
        for i, c3 in enumerate(self.in_channels_3D):
            name = f"stage_{i + 1}"
            self.grouped_sp_conv_blocks_3D.add_module(name, make_sparse_convmodule(
                c3, c3, 3, indice_key=f"subm3D_{i + 1}", norm_cfg=norm_cfg, padding=1,
                conv_type="SubMConv3d"))
            self.grouped_sp_conv_blocks_2D.add_module(name, make_sparse_convmodule(
                64, 64, 3, indice_key=f"block2d_0_{i + 1}", norm_cfg=norm_cfg, padding=1,
                conv_type="SubMConv3d"))
            self.grouped_sp_conv_blocks_mix.add_module(name, SparseBasicBlock(
                c3 + 64, c3 + 64, norm_cfg=norm_cfg, conv_cfg=conv_cfg))
            gates.append(nn.Sequential(nn.Linear(c3, self.in_channels_2D[i]), nn.ReLU()))
            cross_gates.append(nn.Sequential(nn.Linear(c3, self.in_channels_2D[i]), nn.ReLU()))
        self.gate_control = nn.ModuleList(gates)
        self.cross_gate_control = nn.ModuleList(cross_gates)

    def make_aggregation_block(self, norm_cfg, conv_cfg=dict(type="SubMConv3d")):
        self.aggregation_blocks = spconv.SparseSequential()
        for i, c3 in enumerate(self.in_channels_3D):
            self.aggregation_blocks.add_module(f"stage_{i + 1}", SparseBasicBlock(
                c3 + 64, c3 + 64, norm_cfg=norm_cfg, conv_cfg=conv_cfg))

    def make_downscale_block(self, norm_cfg):
        self.downscale_blocks = spconv.SparseSequential()
        for i, c3 in enumerate(self.in_channels_3D):
            self.downscale_blocks.add_module(f"stage_{i + 1}", make_sparse_convmodule(
                c3 + 64, self.out_channels[i] + 64, kernel_size=self.down_kernel_size[i],
                indice_key=f"spconv_ds_{i + 1}", norm_cfg=norm_cfg, stride=self.down_stride[i],
                padding=self.padding[i], conv_type="SparseConv3d"))

    # ---- helpers -----------------------------------------------------------------
    @staticmethod
    def pad_missing_batch_id(indices, features, batch_size, missing=None):
        """:208-225 -- a sample with no row gets one all-zero voxel at the
        origin so every per-sample mask downstream is non-empty.
        missing: the sample ids without a row, when the caller already knows them
        on the host (no device read then)."""
        if missing is None:
            if indices.shape[0]:
                ids = torch.arange(batch_size, device=indices.device, dtype=indices.dtype)
                present = (indices[:, :1] == ids).any(0)     # (bincount would sync for its size)
            else:
                present = torch.zeros(batch_size, dtype=torch.bool, device=indices.device)
            missing = (~present).nonzero().flatten().tolist()
        if len(missing) == 0:
            return indices, features
        pad_idx = indices.new_zeros((len(missing), indices.shape[1]))
        ids = torch.tensor(missing, dtype=indices.dtype)
        if indices.is_cuda:
            ids = ids.pin_memory().to(indices.device, non_blocking=True)
        pad_idx[:, 0] = ids
        pad_feat = features.new_zeros((len(missing), features.shape[1]))
        return torch.cat([indices, pad_idx], 0), torch.cat([features, pad_feat], 0)

    @staticmethod
    def sample_counts(only_2d_bzyx, voxel_3d_bzyx, batch_size):
        """[2, B] device tensor: rows per sample of both voxel sets."""
        ids = torch.arange(batch_size, device=voxel_3d_bzyx.device, dtype=voxel_3d_bzyx.dtype)
        # (two compare-and-sum passes: torch.bincount synchronises to size its output)
        return torch.stack([(only_2d_bzyx[:, :1] == ids).sum(0), (voxel_3d_bzyx[:, :1] == ids).sum(0)])

    def nearest_3d_of_only_2d(self, only_2d_bzyx, voxel_3d_bzyx, batch_size, fps_num, radius,
                              max_cluster_samples, dist_thresh, counts=None, coord_bound=None,
                              n_pad=0):
        """Per sample nearest LiDAR voxel of every only-2D voxel (:349-369);
        returns global row indices into voxel_3D, -1 = unassigned, and `n_pad` more -1 rows
        behind them (the padded only-2D voxels, :208-225).  Rows of both
        tensors are grouped by sample (they always are: voxelize concatenates
        samples in order).  One host read (the per-sample counts; none when the
        caller passes them as nested lists); when every sample needs the FPS
        path, all samples' FPS run in ONE ragged launch, and everything behind FPS is one
        native call for the whole batch (kernels.gma_nn_chain).
        coord_bound: an upper bound of every coordinate (the largest spatial extent the caller
        holds).  The one-call chain orders keys by integer squared distance, which is exact
        for coordinates below 32768 and dist_thresh, radius <= 2048; outside that, or
        without a bound, the per-sample entries run instead."""
        if not K.gma_nn_chain_supported(coord_bound, dist_thresh, radius):
            out = self._nearest_3d_per_sample(only_2d_bzyx, voxel_3d_bzyx, batch_size, fps_num,
                                              radius, max_cluster_samples, dist_thresh, counts)
            return torch.cat([out, out.new_full((n_pad,), -1)]) if n_pad else out
        dev = only_2d_bzyx.device
        if counts is None:
            counts = self.sample_counts(only_2d_bzyx, voxel_3d_bzyx, batch_size).tolist()
        c2, c3 = counts
        o2, o3, modes, bases = [0], [0], [], []
        for b in range(batch_size):
            o2.append(o2[-1] + c2[b])
            o3.append(o3[-1] + c3[b])
            modes.append(K.NN_CHAIN_SKIP if not (c2[b] and c3[b]) else
                         K.NN_CHAIN_DIRECT if c2[b] <= fps_num else K.NN_CHAIN_CLUSTERED)
            # cumulative offsets; the reference adds the previous sample's count only (B.4)
            bases.append((c3[b - 1] if b > 0 else 0) if self.reference_quirks else o3[b])
        # pinned + non_blocking: a pageable copy would block the host until the stream
        # (the previous stage's 6 ms FPS, when this runs on the search stream) drains
        desc = K.gma_nn_chain_desc(o2, o3, modes, bases, dev)
        big = [b for b in range(batch_size) if modes[b] == K.NN_CHAIN_CLUSTERED]
        rep_all = None
        if big:
            q_f = only_2d_bzyx[:, 1:].float()
            if len(big) == batch_size and batch_size > 1:   # the common case at stages 0/1
                rep_all = K.furthest_point_sample_ragged(q_f, desc[:batch_size + 1], max(c2),
                                                         fps_num)
            else:
                rep_all = torch.zeros((batch_size, fps_num), dtype=torch.int32, device=dev)
                for b in big:
                    rep_all[b] = K.furthest_point_sample(q_f[None, o2[b]:o2[b + 1]], fps_num)[0]
        nq_max = max(fps_num if m == K.NN_CHAIN_CLUSTERED else c2[b] if m == K.NN_CHAIN_DIRECT
                     else 0 for b, m in enumerate(modes))
        nk_max = max(c3[b] if m != K.NN_CHAIN_SKIP else 0 for b, m in enumerate(modes))
        return K.gma_nn_chain(only_2d_bzyx, voxel_3d_bzyx, desc, batch_size, rep_all, fps_num,
                              nq_max, nk_max, dist_thresh, radius, max_cluster_samples, n_pad)

    def _nearest_3d_per_sample(self, only_2d_bzyx, voxel_3d_bzyx, batch_size, fps_num, radius,
                               max_cluster_samples, dist_thresh, counts=None):
        """nearest_3d_of_only_2d through the per-sample entries (nn_search / ball_query /
        nn_assign): the path outside the one-call chain's precondition."""
        dev = only_2d_bzyx.device
        out = torch.full((only_2d_bzyx.shape[0],), -1, dtype=torch.long, device=dev)
        if counts is None:
            counts = self.sample_counts(only_2d_bzyx, voxel_3d_bzyx, batch_size).tolist()
        c2, c3 = counts
        o2 = [0]
        o3 = [0]
        for b in range(batch_size):
            o2.append(o2[-1] + c2[b])
            o3.append(o3[-1] + c3[b])
        q_zyx = only_2d_bzyx[:, 1:].contiguous()
        k_zyx = voxel_3d_bzyx[:, 1:].contiguous()
        todo = [b for b in range(batch_size) if c2[b] and c3[b]]
        big = [b for b in todo if c2[b] > fps_num]
        rep_all = None
        if len(big) == batch_size and batch_size > 1:   # the common case at stages 0/1
            # pinned + non_blocking: a pageable copy would block the host until the stream
            # (the previous stage's 6 ms FPS, when this runs on the search stream) drains
            offsets = torch.tensor(o2, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
            rep_all = K.furthest_point_sample_ragged(q_zyx.float(), offsets, max(c2), fps_num)
        for b in todo:
            q = q_zyx[o2[b]:o2[b + 1]]
            k = k_zyx[o3[b]:o3[b + 1]]
            if c2[b] <= fps_num:
                nn_idx = K.nn_search(q, k, dist_thresh).long()
            else:
                q_f = q.float().unsqueeze(0)
                rep_idx = (rep_all[b] if rep_all is not None
                           else K.furthest_point_sample(q_f, fps_num)[0]).long()
                rep = q[rep_idx]
                rep_nn = K.nn_search(rep, k, dist_thresh)
                group = K.ball_query(0, radius, max_cluster_samples, q_f,
                                     rep.float().unsqueeze(0))[0]
                nn_idx = K.nn_assign(group, rep_nn, c2[b]).long()
            # cumulative offsets; the reference adds the previous sample's count only (B.4)
            base = (c3[b - 1] if b > 0 else 0) if self.reference_quirks else o3[b]
            out[o2[b]:o2[b + 1]] = torch.where(nn_idx >= 0, nn_idx + base, nn_idx)
        return out

    # ---- index-only half of a GMA-Conv stage ------------------------------------
    def plan_stage_rows(self, idx3_5, idx2_5, batch_size, stats=None, bzyx3=None, bzyx2=None,
                        mix3=None, mix2=None, plain_rows=None):
        """Everything grouped_sparse_conv derives from the two 5-column index
        tensors alone, up to the neighbour search: row lists of the only-3D /
        only-2D voxels, the padded only-2D indices, the per-sample counts.
        stats: the per-sample row counts kernels.modality_split_many read back
        with the split itself; with them nothing here waits for the device
        (without: three mask.nonzero() calls and a count transfer do).
        bzyx3 / bzyx2: the same voxel sets as 4-column (b,z,y,x) tensors when the caller
        still has them (it made the 5-column ones by inserting the mix flag): selections are
        taken from those instead of dropping the column again after every index_select.
        mix3 / mix2: the flag columns as contiguous int32 vectors, likewise.
        plain_rows: (only-3D rows, only-2D rows) when the caller made them already."""
        if stats is None:
            only_3D_rows = (idx3_5[:, 1] == 0).nonzero().flatten()
            only_2D_rows = (idx2_5[:, 1] == 0).nonzero().flatten()
            missing = None
        else:
            if plain_rows is not None:      # (made for all stages at once: rows_where_eq_many)
                only_3D_rows, only_2D_rows = plain_rows
            else:
                # (the flag vectors themselves when the caller has them: a contiguous read
                # instead of every fifth int of the index tensor)
                only_3D_rows = K.rows_where_eq(mix3 if mix3 is not None else idx3_5[:, 1], 0,
                                               sum(stats["c3_plain"]))
                only_2D_rows = K.rows_where_eq(mix2 if mix2 is not None else idx2_5[:, 1], 0,
                                               sum(stats["c2_plain"]))
            missing = [b for b in range(batch_size) if stats["c2_plain"][b] == 0]
        idx3 = bzyx3 if bzyx3 is not None else drop_mix_column(idx3_5)
        idx2 = bzyx2 if bzyx2 is not None else drop_mix_column(idx2_5)
        # the neighbour search runs on the real only-2D rows, which are grouped by
        # sample; the all-zero pad rows (:208-225) are appended AFTER them whatever
        # their sample id, carry zero features (so their gate is irrelevant) and get
        # "no neighbour" -- slicing the padded tensor by per-sample counts would be
        # wrong whenever a sample other than the last one is the empty one
        o2_bzyx_raw = idx2.index_select(0, only_2D_rows)
        n_raw = o2_bzyx_raw.shape[0]
        # (the pad rows are (b, 0, 0, 0, 0): padding after dropping the mix column is the same)
        o2_bzyx_pad, _ = self.pad_missing_batch_id(
            o2_bzyx_raw, o2_bzyx_raw.new_zeros((n_raw, 0)).float(), batch_size, missing)
        plan = dict(only_3D_rows=only_3D_rows, only_2D_rows=only_2D_rows,
                    o2_bzyx_pad=o2_bzyx_pad, o2_bzyx=o2_bzyx_raw, idx3=idx3, idx2=idx2,
                    n_pad=o2_bzyx_pad.shape[0] - n_raw)
        if stats is None:
            plan["counts"] = self.sample_counts(o2_bzyx_raw, idx3, batch_size)
        else:
            plan["counts_host"] = [list(stats["c2_plain"]),
                                   [a + b for a, b in zip(stats["c3_plain"], stats["c3_mixed"])]]
            plan["mixed_missing"] = [b for b in range(batch_size) if stats["c2_mixed"][b] == 0]
        return plan

    def plan_stage_nn(self, plan, counts, batch_size, fps_num, radius, max_cluster_samples,
                      dist_thresh, coord_bound=None):
        """The neighbour search of a planned stage (no host read: `counts` are the
        nested lists already on the host).  Stream-agnostic: the fusion path
        enqueues it on a side stream under the LiDAR encoder's forward pass.
        coord_bound: see nearest_3d_of_only_2d."""
        nn3 = self.nearest_3d_of_only_2d(plan["o2_bzyx"], plan["idx3"], batch_size, fps_num,
                                         radius, max_cluster_samples, dist_thresh, counts=counts,
                                         coord_bound=coord_bound, n_pad=plan["n_pad"])
        plan["nn3"] = nn3
        # the rows of each nearest voxel, for the assembly's backward (no atomics there)
        n_raw = plan["o2_bzyx"].shape[0]
        plan["nn_segments"] = K.gma_nn_segments(nn3[:n_raw], plan["idx3"].shape[0])
        return plan

    @staticmethod
    def _shell(idx, shape, batch_size):
        return spconv.SparseConvTensor(
            torch.empty((idx.shape[0], 0), dtype=torch.float32, device=idx.device), idx, shape,
            batch_size)

    def plan_stage_sets(self, plan, syn_mix_2D, shape3, shape2, batch_size, stage_id, need_grad):
        """The part of a stage's index-only work that depends on the stage's OWN voxel sets
        alone (no host read, nothing from the previous stage): the per-call dummy embedding,
        the only-3D set and the unified set grouped_sparse_conv builds, and the rulebooks of
        the conv blocks that run on them.  -> the unified (index-only) tensor."""
        stage = f"stage_{stage_id + 1}"
        dev = plan["idx3"].device
        convs = spconv.sparse_convs
        with spconv.plan_batch("stage"):
            plan["dummy"] = self.dummy_embedding_fn(self.in_channels_3D[stage_id], dev)
            o3_idx = plan["idx3"].index_select(0, plan["only_3D_rows"])
            only3d = self._shell(o3_idx, shape3, batch_size)
            only3d.plan(convs(getattr(self.grouped_sp_conv_blocks_3D, stage)), need_grad)
            n_mix = syn_mix_2D.shape[0]
            mixed_idx, _ = self.pad_missing_batch_id(
                plan["idx2"].index_select(0, syn_mix_2D),
                torch.empty((n_mix, 0), dtype=torch.float32, device=dev), batch_size,
                plan.get("mixed_missing"))
            unified = self._shell(torch.cat([o3_idx, plan["o2_bzyx_pad"], mixed_idx], 0), shape2,
                                  batch_size)
            unified.plan(convs(getattr(self.aggregation_blocks, stage)), need_grad)
        plan.update(only3d=only3d, unified=unified, mixed_pad=mixed_idx.shape[0] - n_mix)
        return unified

    def plan_stage_down(self, plan, prev, batch_size, stage_id, need_grad):
        """The rest of ONE stage: the sparse_add union with the previous stage's output
        (`prev`, None for the first stage) and the rulebook of the down-scaling conv on it
        -- two host reads.  -> this stage's (index-only) output tensor."""
        stage = f"stage_{stage_id + 1}"
        unified = plan["unified"]
        total = unified
        with spconv.plan_batch("stage"):
            if prev is not None:
                assert prev.spatial_shape == list(unified.spatial_shape), \
                    "sparse_add needs equal spatial_shape"
                plan["add"] = Fsp.plan_sparse_add(unified.indices, prev.indices, batch_size,
                                                  unified.spatial_shape)
                total = plan["add"]["sum"]
            return total.plan(spconv.sparse_convs(getattr(self.downscale_blocks, stage)), need_grad)

    def plan_stage_chain(self, plans, batch_size, need_grad):
        """plan_stage_down for ALL stages with ONE host read instead of two per stage
        (kernels.add_conv_chain: the unions and the down-scaling convs' output sets counted on
        the device back to back -- the unified sets are known up front).  Falls back to the
        stage-by-stage calls when a down-scaling block is not a single strided conv.
        -> the last stage's output tensor."""
        n = len(plans)
        downs = []
        for i in range(n):
            cs = [c for c in spconv.sparse_convs(getattr(self.downscale_blocks, f"stage_{i + 1}"))
                  if not getattr(c, "conv1x1", False)]
            downs.append(cs)
        chainable = os.environ.get("MSMD_STAGE_CHAIN", "1") == "1" and n > 1 and all(
            len(cs) == 1 and not cs[0].subm and all(d == 1 for d in cs[0].dilation)
            for cs in downs)
        shapes = [list(p["unified"].spatial_shape) for p in plans]
        if chainable:
            sh = shapes[0]
            for i, cs in enumerate(downs):
                chainable = chainable and sh == shapes[i]
                sh = K.conv_output_size(sh, list(cs[0].kernel_size), list(cs[0].stride),
                                        list(cs[0].padding))
        if not chainable:
            prev = None
            for i in range(n):
                prev = self.plan_stage_down(plans[i], prev, batch_size, i, need_grad)
            return prev
        geoms = [(list(cs[0].kernel_size), list(cs[0].stride), list(cs[0].padding)) for cs in downs]
        levels = K.add_conv_chain([p["unified"].indices for p in plans], batch_size, shapes[0],
                                  geoms)
        out = None
        for i, (lv, cs) in enumerate(zip(levels, downs)):
            if i == 0:
                total = plans[0]["unified"]
            else:
                total = self._shell(lv["total_indices"], shapes[i], batch_size)
                plans[i]["add"] = Fsp.add_plan(total, lv["map_a"], lv["map_b"])
            assert total.indices is lv["total_indices"] or i == 0
            total.seed_rulebook(cs[0], lv["out_indices"], lv["nbr_fwd"], lv["nbr_bwd"],
                                lv["out_shape"])
            with spconv.plan_batch("stage"):
                out = total.plan(spconv.sparse_convs(getattr(self.downscale_blocks,
                                                             f"stage_{i + 1}")), need_grad)
        return out

    def plan_stage_tensors(self, plan, idx3_5, idx2_5, syn_mix_2D, shape3, shape2, batch_size,
                           stage_id, prev, need_grad):
        """plan_stage_sets + plan_stage_down of one stage (the stage-by-stage order: two host
        reads per stage; SparseFusionPath.prepare plans the sets of all stages first and then
        the whole chain with one read, plan_stage_chain).  `prev` = the index-only output
        tensor of the previous stage (None for the first); returns this stage's."""
        self.plan_stage_sets(plan, syn_mix_2D, shape3, shape2, batch_size, stage_id, need_grad)
        return self.plan_stage_down(plan, prev, batch_size, stage_id, need_grad)

    # ---- one GMA-Conv stage (:325-430) -----------------------------------------
    @staticmethod
    def _gate_table(seq, rows, tail=None):
        """gate_control / cross_gate_control (Linear + ReLU) over feature rows; `tail`: rows
        appended behind them (the dummy embedding).  On the GPU one row-streaming kernel each
        way (kernels.rows_linear: hipBLASLt's fp32 GEMM took 170-230 us per call on these
        skinny shapes, 16 calls per step); the module itself otherwise."""
        lin = seq[0]
        if (rows.is_cuda and rows.dtype == torch.float32 and len(seq) == 2
                and isinstance(lin, nn.Linear) and isinstance(seq[1], nn.ReLU)
                and K.rows_linear_supported(lin.in_features, lin.out_features)):
            return K.rows_linear(rows, lin.weight, lin.bias, relu=True, x_tail=tail)
        return seq(rows if tail is None else torch.cat([rows, tail], 0))

    @staticmethod
    def _linear_relu(seq):
        return (len(seq) == 2 and isinstance(seq[0], nn.Linear) and isinstance(seq[1], nn.ReLU)
                and seq[0].out_features == 64)

    def grouped_sparse_conv(self, voxel_3D, voxel_2D, syn_mix_3D, syn_mix_2D, stage_id, fps_num,
                            radius, max_cluster_samples, dist_thresh, plan=None):
        B = voxel_3D.batch_size
        c3 = self.in_channels_3D[stage_id]
        zyx = [0, 2, 3, 4]      # indices are (batch, mix_flag, z, y, x)
        # row lists instead of boolean masks: gathers go through index_select,
        # whose backward is index_add_ (torch's advanced-indexing backward sorts
        # the indices -- 2.8 ms per call on the [N3+1,64] gate table here)
        if plan is None:        # index-only work not done ahead of time: do it here
            plan = self.plan_stage_rows(voxel_3D.indices, voxel_2D.indices, B)
            self.plan_stage_nn(plan, plan["counts"].tolist(), B, fps_num, radius,
                               max_cluster_samples, dist_thresh,
                               coord_bound=max(*voxel_3D.spatial_shape, *voxel_2D.spatial_shape))
        elif plan.get("ready") is not None:     # computed on another stream
            torch.cuda.current_stream().wait_event(plan["ready"])
        only_3D_rows, only_2D_rows = plan["only_3D_rows"], plan["only_2D_rows"]
        o2_bzyx_pad, nn3 = plan["o2_bzyx_pad"], plan["nn3"]
        # uncovered 2D voxels are gated by a random embedding (row -1 -> last row)
        dummy = plan["dummy"] if "dummy" in plan else \
            self.dummy_embedding_fn(c3, voxel_3D.features.device)
        n3 = voxel_3D.features.shape[0]
        planned = "unified" in plan     # plan_stage_tensors ran: voxel sets + rulebooks exist
        stage = f"stage_{stage_id + 1}"
        # One launch for everything around the convs (csrc/gma.hip) when the stage was planned
        # ahead and neither input tensor wants a gradient (frozen LiDAR encoder, raw
        # virtual-point voxels: the LC training configuration); the reference's op-by-op chain
        # otherwise -- same values.
        fused = planned and self.fused_assembly and voxel_3D.features.is_cuda and not (
            voxel_3D.features.requires_grad or voxel_2D.features.requires_grad)
        # ... with both gates computed inside that launch, for the rows it reads only (the
        # cross-gate table has n3 + 1 rows, the assembly reads 1-10 % of them) -- same bits
        if (fused and self.fused_gates and plan.get("nn_segments") is not None
                and voxel_3D.features.dtype == torch.float32
                and K.gma_stage_supported(c3, voxel_2D.features.shape[1])
                and self._linear_relu(self.cross_gate_control[stage_id])
                and self._linear_relu(self.gate_control[stage_id])):
            f3_only = voxel_3D.features.index_select(0, only_3D_rows)
            voxel_only_3D = getattr(self.grouped_sp_conv_blocks_3D, stage)(
                plan["only3d"].replace_feature(f3_only))
            lin_c, lin_g = self.cross_gate_control[stage_id][0], self.gate_control[stage_id][0]
            assert syn_mix_3D.shape[0] == syn_mix_2D.shape[0]
            feats = K.gma_stage(
                voxel_only_3D.features, lin_c.weight, lin_c.bias, lin_g.weight, lin_g.bias,
                voxel_3D.features, dummy.to(voxel_3D.features.dtype), voxel_2D.features,
                nn3[:only_2D_rows.shape[0]], only_2D_rows, syn_mix_3D, syn_mix_2D,
                plan["n_pad"], plan["mixed_pad"], plan["nn_segments"])
            return getattr(self.aggregation_blocks, stage)(plan["unified"].replace_feature(feats))
        cross_gating = self._gate_table(self.cross_gate_control[stage_id], voxel_3D.features,
                                        dummy.to(voxel_3D.features.dtype))
        f3_only = voxel_3D.features.index_select(0, only_3D_rows)
        if planned:
            voxel_only_3D = plan["only3d"].replace_feature(f3_only)
        else:
            voxel_only_3D = spconv.SparseConvTensor(
                f3_only, drop_mix_column(voxel_3D.indices.index_select(0, only_3D_rows)),
                voxel_3D.spatial_shape, B)
        mixed_3D = voxel_3D.features.index_select(0, syn_mix_3D)
        assert syn_mix_3D.shape[0] == syn_mix_2D.shape[0]
        gate = self._gate_table(self.gate_control[stage_id], mixed_3D)
        if fused:
            voxel_only_3D = getattr(self.grouped_sp_conv_blocks_3D, stage)(voxel_only_3D)
            n_o2 = only_2D_rows.shape[0]
            feats = K.gma_assemble(
                voxel_only_3D.features, cross_gating, gate, voxel_3D.features, voxel_2D.features,
                nn3[:n_o2], only_2D_rows, syn_mix_3D, syn_mix_2D, plan["n_pad"],
                plan["mixed_pad"], segments=plan.get("nn_segments"))
            unified = plan["unified"].replace_feature(feats)
            return getattr(self.aggregation_blocks, stage)(unified)
        o2_feat = voxel_2D.features.index_select(0, only_2D_rows)
        if plan["n_pad"]:       # :208-225 samples without an only-2D voxel got a zero row
            o2_feat = torch.cat([o2_feat, o2_feat.new_zeros((plan["n_pad"], o2_feat.shape[1]))], 0)
        o2_feat = cross_gating.index_select(
            0, torch.where(nn3 >= 0, nn3, torch.full_like(nn3, n3))) * o2_feat

        mixed_2D = voxel_2D.features.index_select(0, syn_mix_2D)
        mixed_2D = gate * mixed_2D
        mixed_feat = torch.cat([mixed_3D, mixed_2D], -1)
        if planned:
            if plan["mixed_pad"]:
                mixed_feat = torch.cat([mixed_feat, mixed_feat.new_zeros(
                    (plan["mixed_pad"], mixed_feat.shape[1]))], 0)
        else:
            mixed_idx, mixed_feat = self.pad_missing_batch_id(
                voxel_2D.indices.index_select(0, syn_mix_2D), mixed_feat, B)
        voxel_only_3D = getattr(self.grouped_sp_conv_blocks_3D, stage)(voxel_only_3D)
        f2 = F.pad(o2_feat, (c3, 0), mode="constant", value=0)
        f3 = F.pad(voxel_only_3D.features, (0, 64), mode="constant", value=0)
        assert f2.shape[-1] == f3.shape[-1] == mixed_feat.shape[-1]
        feats = torch.cat([f3, f2, mixed_feat], 0)
        if planned:
            unified = plan["unified"].replace_feature(feats)
        else:
            unified = spconv.SparseConvTensor(
                feats, torch.cat([voxel_only_3D.indices, o2_bzyx_pad,
                                  drop_mix_column(mixed_idx)], 0),
                voxel_2D.spatial_shape, voxel_2D.batch_size)
        return getattr(self.aggregation_blocks, stage)(unified)

    def forward(self, voxel_3D_list, voxel_2D_list, syn_mix_3D_list, syn_mix_2D_list,
                fps_num_list, radius_list, max_cluster_samples_list, dist_thresh_list,
                stage_plans=None):
        """stage_plans (optional, not in the reference): per-stage results of
        plan_stage_rows / plan_stage_nn computed ahead of the feature pass."""
        stage_outs = []
        for stage_id in range(len(voxel_2D_list)):
            out = self.grouped_sparse_conv(
                voxel_3D_list[stage_id], voxel_2D_list[stage_id], syn_mix_3D_list[stage_id],
                syn_mix_2D_list[stage_id], stage_id, fps_num_list[stage_id],
                radius_list[stage_id], max_cluster_samples_list[stage_id],
                dist_thresh_list[stage_id],
                plan=None if stage_plans is None else stage_plans[stage_id])
            if stage_id > 0:
                add = None if stage_plans is None else stage_plans[stage_id].get("add")
                out = Fsp.sparse_add(out, stage_outs[stage_id - 1]) if add is None else \
                    Fsp.sparse_add_planned(out, stage_outs[stage_id - 1], add)
            stage_outs.append(getattr(self.downscale_blocks, f"stage_{stage_id + 1}")(out))
        return stage_outs
