"""Shared by test_pillar_cpu.py, test_gpu_pillar.py, tools/pillar_parity.py and
tools/pillar_bench.py: the committed golden (tests/golden/pillar_vectors.npz), seeded pillar
tables and a torch restatement of the reference's op sequence in any dtype."""
import json
import os

import numpy as np
import torch
from torch.nn import functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pillar_vectors.npz")
VOXEL_SIZE = (0.2, 0.2, 8)
PC_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)
GRID = 512

_CACHE = {}


def golden():
    if "g" not in _CACHE:
        g = np.load(GOLDEN)
        _CACHE["g"] = ({k: g[k] for k in g.files}, json.loads(bytes(g["meta"]).decode()))
    return _CACHE["g"]


def scaled_err(got, exp):
    """max |got - exp| over the largest |exp| (the project's feature tolerance is 1e-4 of it)."""
    got, exp = got.detach().double().cpu(), exp.detach().double().cpu()
    return float((got - exp).abs().max() / exp.abs().max().clamp(min=1e-30))


def golden_case(tag, device="cpu"):
    """-> (module with the case's weights and mode, (features, num_points, coors), expected
    output, {key: state after the forward})."""
    from msmdfusion_amd.pillar_encoder import PillarFeatureNet
    g, meta = golden()
    info = meta["cases"][tag]
    mod = PillarFeatureNet(voxel_size=meta["voxel_size"],
                           point_cloud_range=meta["point_cloud_range"], **info["cfg"])
    mod.load_state_dict({k: torch.from_numpy(g["%s.w.%s" % (info["weights"], k)])
                         for k in info["keys"]})
    mod.train(info["training"]).to(device)
    i = info["input"]
    inputs = tuple(torch.from_numpy(g["%s.%s" % (i, k)]).to(device)
                   for k in ("features", "num_points", "coors"))
    after = {k: torch.from_numpy(g["%s.after.%s" % (tag, k)]) for k in info["keys"]
             if "running" in k or "num_batches" in k}
    return mod, inputs, torch.from_numpy(g["%s.out" % tag]), after


def make_pillars(n, m, c, seed, device="cpu", exceed=False):
    """Pillars as hard voxelization leaves them (points inside their pillar, slots past
    num_points zero); the first eighth hold one point, the last eighth are full, so padded
    slots win the maximum in some channels.  Continuous draws: no exact ties among valid
    slots."""
    rng = np.random.RandomState(seed)
    cells = rng.choice(GRID * GRID, n, replace=False)
    coors = np.stack([rng.randint(0, 2, n), np.zeros(n, np.int64), cells // GRID, cells % GRID], 1)
    feats = np.zeros((n, m, c), np.float32)
    feats[:, :, :2] = (rng.rand(n, m, 2) + coors[:, None, [3, 2]]) * VOXEL_SIZE[0] + PC_RANGE[0]
    feats[:, :, 2] = rng.uniform(-4.5, 2.5, (n, m))
    feats[:, :, 3:] = rng.rand(n, m, c - 3)
    if exceed:
        num = rng.randint(1, 100, n)
    else:
        num = rng.randint(1, m + 1, n)
        num[: max(1, n // 8)] = 1
        if n > 1:
            num[-max(1, n // 8):] = m
        feats *= (np.arange(m)[None, :] < num[:, None])[:, :, None]
    return tuple(torch.from_numpy(a).to(device) for a in
                 (feats.astype(np.float32), num.astype(np.int32), coors.astype(np.int32)))


def seed_encoder(mod, seed):
    """Weights ~ N(0, 0.3), gamma in [0.5, 1.5), beta in [-0.2, 0.5) (relu(shift) > 0 in part
    of the channels), non-trivial running statistics."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if p.dim() == 1 and name.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=g) * 0.7 - 0.2)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
        for name, b in mod.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
            elif name.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) + 0.5)
    return mod


def reference_sequence(mod, features, num_points, coors, dtype, weight, gamma, beta,
                       per_slot=False):
    """The reference's PillarFeatureNet.forward + PFNLayer.forward (one layer), op for op, in
    `dtype`, on a private copy of the input (the reference writes into it).  weight / gamma /
    beta: tensors of `dtype` (leaves, for autograd); the running statistics are read from the
    layer and never updated.  -> [N, U] (per_slot: the BatchNorm output [N, M, U] in front of
    the ReLU instead)"""
    pfn = mod.pfn_layers[0]
    bn = pfn.norm
    features = features.detach().to(dtype).clone()
    ls = [features]
    if mod._with_cluster_center:
        points_mean = features[:, :, :3].sum(dim=1, keepdim=True) / \
            num_points.to(dtype).view(-1, 1, 1)
        ls.append(features[:, :, :3] - points_mean)
    if mod._with_voxel_center:
        cx = coors[:, 3].to(dtype).unsqueeze(1) * mod.vx + mod.x_offset
        cy = coors[:, 2].to(dtype).unsqueeze(1) * mod.vy + mod.y_offset
        if not mod.legacy:
            f_center = torch.zeros_like(features[:, :, :2])
            f_center[:, :, 0] = features[:, :, 0] - cx
            f_center[:, :, 1] = features[:, :, 1] - cy
        else:
            f_center = features[:, :, :2]
            f_center[:, :, 0] = f_center[:, :, 0] - cx
            f_center[:, :, 1] = f_center[:, :, 1] - cy
        ls.append(f_center)
    if mod._with_distance:
        ls.append(torch.norm(features[:, :, :3], 2, 2, keepdim=True))
    x = torch.cat(ls, dim=-1)
    m = x.shape[1]
    mask = num_points.int().unsqueeze(1) > torch.arange(m, dtype=torch.int, device=x.device)
    x = x * mask.unsqueeze(-1).to(dtype)
    x = F.linear(x, weight)
    training = bn.training or bn.running_mean is None
    rm = None if training else bn.running_mean.to(dtype)
    rv = None if training else bn.running_var.to(dtype)
    x = F.batch_norm(x.permute(0, 2, 1).contiguous(), rm, rv, gamma, beta, training, 0.0,
                     bn.eps).permute(0, 2, 1).contiguous()
    if per_slot:
        return x
    x = F.relu(x)
    if pfn.mode == "max":
        return torch.max(x, dim=1)[0]
    return x.sum(dim=1) / num_points.to(dtype).view(-1, 1)


def unambiguous_grad_out(mod, inputs, grad_out, margin=1e-4):
    """grad_out with zeros wherever WHICH slots the gradient reaches is decided by less than
    `margin` of the largest activation -- far above float32 rounding (1e-7), far below the
    spread of the activations.  Max and ReLU are discontinuous there: among 10^5 maxima over M
    slots some pair of candidates always lies within float32 rounding of each other, and then
    any float32 evaluation (torch's included) may route the gradient to another slot than
    float64 does, a discrete event that says nothing about accuracy.  Judged on the float64
    reference: max mode drops (pillar, channel) entries whose two best candidates (the valid
    slots and ONE padded slot: padded slots tie exactly and carry zero rows) are closer than
    the margin, or whose maximum is that close to the ReLU's zero; avg mode drops entries with
    any slot's pre-activation that close to zero."""
    pfn = mod.pfn_layers[0]
    features, num_points, coors = inputs
    with torch.no_grad():
        z = reference_sequence(mod, features, num_points, coors, torch.float64,
                               *[p.detach().double() for p in
                                 (pfn.linear.weight, pfn.norm.weight, pfn.norm.bias)],
                               per_slot=True)
        thr = margin * float(z.abs().max())
        if pfn.mode == "max":
            m = z.shape[1]
            keep = torch.arange(m, device=z.device)[None, :] <= num_points.long()[:, None]
            y = torch.relu(z).masked_fill(~keep[:, :, None], -1.0)
            if m > 1:
                top = y.topk(2, dim=1)[0]
                bad = (top[:, 0] - top[:, 1] < thr) & (top[:, 0] > 0)    # (all clipped: no gradient)
            else:
                bad = torch.zeros_like(y[:, 0], dtype=torch.bool)
            zmax = z.masked_fill(~keep[:, :, None], -float("inf")).max(dim=1)[0]
            bad |= zmax.abs() < thr
        else:
            bad = (z.abs() < thr).any(dim=1)
    return grad_out.masked_fill(bad.to(grad_out.device), 0.0), float(bad.float().mean())


def reference_grads(mod, inputs, grad_out, dtype):
    """-> (out, dW, dgamma, dbeta) of reference_sequence in `dtype` by autograd."""
    pfn = mod.pfn_layers[0]
    leaves = [p.detach().to(dtype).clone().requires_grad_(True)
              for p in (pfn.linear.weight, pfn.norm.weight, pfn.norm.bias)]
    out = reference_sequence(mod, *inputs, dtype, *leaves)
    out.backward(grad_out.to(dtype))
    return (out.detach(),) + tuple(p.grad for p in leaves)
