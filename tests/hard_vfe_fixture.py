"""Shared by test_hard_vfe_cpu.py, test_gpu_hard_vfe.py, tools/hard_vfe_parity.py and
tools/hard_vfe_bench.py: the committed golden (tests/golden/hard_vfe_vectors.npz), seeded voxel
tables and a torch restatement of the reference's HardVFE op sequence in any dtype."""
import json
import os

import numpy as np
import torch
from torch.nn import functional as F

from pillar_fixture import scaled_err, seed_encoder  # noqa: F401  (re-exported)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "hard_vfe_vectors.npz")
VOXEL_SIZE = (0.25, 0.25, 8)
PC_RANGE = (-50, -50, -5, 50, 50, 3)
GRID = 400
TAU = 1e-5          # of a layer's largest |pre-activation|: closer decisions are left out

_CACHE = {}


def golden():
    if "g" not in _CACHE:
        g = np.load(GOLDEN)
        _CACHE["g"] = ({k: g[k] for k in g.files}, json.loads(bytes(g["meta"]).decode()))
    return _CACHE["g"]


def golden_case(tag, device="cpu"):
    """-> (module with the case's weights and mode, (features, num_points, coors), arrays of
    the case {out, out64, grad_out, grad64.*, after.*} as tensors)."""
    from msmdfusion_amd.hard_vfe import HardVFE
    g, meta = golden()
    info = meta["cases"][tag]
    mod = HardVFE(voxel_size=meta["voxel_size"], point_cloud_range=meta["point_cloud_range"],
                  **info["cfg"])
    mod.load_state_dict({k: torch.from_numpy(g["%s.w.%s" % (info["weights"], k)])
                         for k in info["keys"]})
    mod.train(info["training"]).to(device)
    inputs = tuple(torch.from_numpy(g[k]).to(device) for k in ("features", "num_points", "coors"))
    arrays = {k[len(tag) + 1:]: torch.from_numpy(v) for k, v in g.items()
              if k.startswith(tag + ".") and not k.startswith(tag + ".w.")}
    return mod, inputs, arrays


def make_voxels(n, m, c, seed, device="cpu", kind="mixed"):
    """Voxels as hard voxelization leaves them (points inside their pillar, slots past
    num_points zero).  mixed: the first eighth hold one point (padded slots win maxima), the
    last eighth are full; one: every voxel holds one point; full: every voxel is full;
    exceed: num_points in (M, M + 36], every slot filled; same: a voxel's points are copies of
    its first (exact ties among the valid slots)."""
    rng = np.random.RandomState(seed)
    cells = rng.choice(GRID * GRID, n, replace=False)
    coors = np.stack([rng.randint(0, 2, n), np.zeros(n, np.int64), cells // GRID, cells % GRID], 1)
    feats = np.zeros((n, m, c), np.float32)
    feats[:, :, :2] = (rng.rand(n, m, 2) + coors[:, None, [3, 2]]) * VOXEL_SIZE[0] + PC_RANGE[0]
    feats[:, :, 2] = rng.uniform(-4.5, 2.5, (n, m))
    feats[:, :, 3:] = rng.rand(n, m, c - 3)
    num = rng.randint(1, m + 1, n)
    if kind == "mixed":
        num[: max(1, n // 8)] = 1
        if n > 1:
            num[-max(1, n // 8):] = m
    elif kind == "one":
        num[:] = 1
    elif kind == "full":
        num[:] = m
    elif kind == "same":
        feats[:] = feats[:, :1]
    if kind == "exceed":
        num = rng.randint(m + 1, m + 37, n)
    else:
        feats *= (np.arange(m)[None, :] < num[:, None])[:, :, None]
    return tuple(torch.from_numpy(a).to(device) for a in
                 (feats.astype(np.float32), num.astype(np.int32), coors.astype(np.int32)))


def encoder(device, c, widths, training, seed=5, norm="naiveSyncBN1d"):
    from msmdfusion_amd.hard_vfe import HardVFE
    mod = HardVFE(in_channels=c, feat_channels=list(widths), with_cluster_center=True,
                  with_voxel_center=True, voxel_size=VOXEL_SIZE, point_cloud_range=PC_RANGE,
                  norm_cfg=dict(type=norm, eps=1e-3, momentum=0.01))
    return seed_encoder(mod, seed).train(training).to(device)


def leaves(mod, dtype, grad=False):
    """[(W, gamma, beta)] per layer in `dtype`, detached copies (grad: requiring grad)."""
    return [tuple(p.detach().to(dtype).clone().requires_grad_(grad)
                  for p in (vfe.linear.weight, vfe.norm.weight, vfe.norm.bias))
            for vfe in mod.vfe_layers]


def reference_sequence(mod, features, num_points, coors, dtype, params, detail=False):
    """The reference's HardVFE.forward + VFELayer.forward, op for op, in `dtype`.  params: what
    leaves() returns; the running statistics are read from the layers and never updated.
    -> [N, U_last] (detail: also the list of BatchNorm outputs [N, M, U_i] in front of each
    ReLU)"""
    x = features.detach().to(dtype)
    ls = [x]
    if mod._with_cluster_center:
        ls.append(x[:, :, :3] - x[:, :, :3].sum(dim=1, keepdim=True) /
                  num_points.to(dtype).view(-1, 1, 1))
    if mod._with_voxel_center:
        f_center = torch.zeros_like(x[:, :, :3])
        f_center[:, :, 0] = x[:, :, 0] - (coors[:, 3].to(dtype).unsqueeze(1) * mod.vx + mod.x_offset)
        f_center[:, :, 1] = x[:, :, 1] - (coors[:, 2].to(dtype).unsqueeze(1) * mod.vy + mod.y_offset)
        f_center[:, :, 2] = x[:, :, 2] - (coors[:, 1].to(dtype).unsqueeze(1) * mod.vz + mod.z_offset)
        ls.append(f_center)
    x = torch.cat(ls, dim=-1)
    m = x.shape[1]
    mask = num_points.int().unsqueeze(1) > torch.arange(m, dtype=torch.int, device=x.device)
    x = x * mask.unsqueeze(-1).to(dtype)
    pre = []
    for i, (vfe, (w, gamma, beta)) in enumerate(zip(mod.vfe_layers, params)):
        bn = vfe.norm
        training = bn.training or bn.running_mean is None
        rm = None if training else bn.running_mean.to(dtype)
        rv = None if training else bn.running_var.to(dtype)
        u = F.batch_norm(F.linear(x, w).permute(0, 2, 1).contiguous(), rm, rv, gamma, beta,
                         training, 0.0, bn.eps).permute(0, 2, 1).contiguous()
        pre.append(u)
        h = F.relu(u)
        agg = torch.max(h, dim=1, keepdim=True)[0]
        x = torch.cat([h, agg.repeat(1, m, 1)], dim=2) if i != len(params) - 1 else agg.squeeze(1)
    return (x, pre) if detail else x


def _near_decisions(u, num_points, tau):
    """u[N, M, U] float64, the BatchNorm output in front of a ReLU + max over the slots.
    -> (tie[N, U]: the two best candidates -- the valid slots and ONE padded slot, the padded
    slots being identical rows -- are closer than tau of the largest |u| while the maximum is
    not clipped; zero[N, M, U]: a candidate's |u| is below that threshold)."""
    thr = tau * float(u.abs().max())
    m = u.shape[1]
    keep = torch.arange(m, device=u.device)[None, :] <= num_points.long()[:, None]
    y = torch.relu(u).masked_fill(~keep[:, :, None], -1.0)
    if m > 1:
        top = y.topk(2, dim=1)[0]
        tie = (top[:, 0] - top[:, 1] < thr) & (top[:, 0] > 0)
    else:
        tie = torch.zeros_like(y[:, 0], dtype=torch.bool)
    zero = (u.abs() < thr) & keep[:, :, None]
    return tie, zero


def exclusions(mod, inputs, grad_out, tau=TAU):
    """From the float64 restatement alone: grad_out with zeros where the LAST layer's receiving
    slot, or the ReLU at it, is decided by less than tau; and (two layers) the layer-1 channels
    in which any ReLU or any max is decided by less than tau -- a flip there changes only that
    row of layer 1's gradients, nothing lies upstream of layer 1.
    -> (grad_out, fraction of entries zeroed, bool[U1] channels left out | None)"""
    with torch.no_grad():
        _, pre = reference_sequence(mod, *inputs, torch.float64, leaves(mod, torch.float64),
                                    detail=True)
        num = inputs[1]
        tie, zero = _near_decisions(pre[-1], num, tau)
        u = pre[-1]
        keep = torch.arange(u.shape[1], device=u.device)[None, :] <= num.long()[:, None]
        umax = u.masked_fill(~keep[:, :, None], -float("inf")).max(dim=1)[0]
        bad = tie | (umax.abs() < tau * float(u.abs().max()))
        out_channels = None
        if len(pre) == 2:
            tie1, zero1 = _near_decisions(pre[0], num, tau)
            out_channels = tie1.any(dim=0) | zero1.any(dim=1).any(dim=0)
    return grad_out.masked_fill(bad.to(grad_out.device), 0.0), float(bad.float().mean()), \
        out_channels


def reference_grads(mod, inputs, grad_out, dtype):
    """-> (out, [dW1, dgamma1, dbeta1, (dW2, dgamma2, dbeta2)]) of reference_sequence in `dtype`
    by autograd."""
    params = leaves(mod, dtype, grad=True)
    out = reference_sequence(mod, *inputs, dtype, params)
    out.backward(grad_out.to(dtype))
    return out.detach(), [p.grad for layer in params for p in layer]


def module_grads(mod):
    return [p.grad for vfe in mod.vfe_layers
            for p in (vfe.linear.weight, vfe.norm.weight, vfe.norm.bias)]
