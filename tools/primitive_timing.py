#!/usr/bin/env python
"""Timings of DESIGN 29 on one GPU: PrimitiveHead.get_targets of the three heads, fused, against
the restated per-sample loop (tests/primitive_ref.py) run on the device with the host reads the
reference has; MultiBackbone forward + backward with shared against independent sampling.

    python tools/primitive_timing.py --out profiles/primitive_timing.txt
"""
import argparse
import copy
import os
import sys
import time

import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import primitive_cases as PC
import primitive_ref as R
from msmdfusion_amd import configs as C, registry
from msmdfusion_amd.head_loss import DepthBoxes
from msmdfusion_amd.primitive_head import prepare_primitive_inputs

dev = torch.device("cuda:0")
parser = argparse.ArgumentParser()
parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "primitive_timing.txt"))
out = open(parser.parse_args().out, "w")
def say(*a):
    line = " ".join(str(x) for x in a); print(line, flush=True); out.write(line + "\n"); out.flush()

B, N, INST = 8, 40000, 30
samples = [PC.make_sample(200 + s, N, [900] * INST) for s in range(B)]
points = torch.stack([s["points"] for s in samples]).to(dev)
boxes = [DepthBoxes(s["boxes"].to(dev)) for s in samples]
labels = [torch.arange(INST, device=dev) for _ in samples]
sems = [s["sem"].to(dev) for s in samples]
insts = [s["inst"].to(dev) for s in samples]
seed_idx = torch.stack([torch.randperm(N)[:1024] for _ in range(B)]).to(dev).int()
seed_pts = torch.gather(points[..., :3], 1, seed_idx.long()[..., None].expand(-1, -1, 3))
heads = {m: registry.build_head(copy.deepcopy(c)).to(dev) for m, c in
         (("z", C.H3DNET_PRIMITIVE_Z), ("xy", C.H3DNET_PRIMITIVE_XY), ("line", C.H3DNET_PRIMITIVE_LINE))}
preds = {m: {"aggregated_points_" + m: seed_pts, "seed_points": seed_pts, "seed_indices": seed_idx} for m in heads}
cfg = C.H3DNET_PRIMITIVE_Z["train_cfg"]

def fused():
    prepared = prepare_primitive_inputs(points, boxes, labels, sems, insts, 18)
    return [heads[m].get_targets(points, boxes, labels, sems, insts, preds[m], prepared=prepared) for m in heads]

for _ in range(5): res = fused()
torch.cuda.synchronize()
times = []
for rep in range(5):
    t0 = time.perf_counter()
    for _ in range(20): fused()
    torch.cuda.synchronize(); times.append((time.perf_counter() - t0) / 20 * 1e3)
say("fused get_targets, three heads, B %d N %d %d instances/sample, config thresholds: ms per step over 5 x 20 runs:" % (B, N, INST), ["%.3f" % t for t in times], "host reads: 0")
say("rows on (z, xy, line):", [int(r[0].sum()) for r in res])

corners = [b.corners for b in boxes]
def loop():
    tr = R.Trace()
    for m in heads:
        for b in range(B):
            R.primitive_targets_ref(points[b], sems[b], insts[b], corners[b], True, m, 18, cfg, torch.float32, None, tr)
    return tr
loop(); torch.cuda.synchronize()
times = []
for rep in range(2):
    t0 = time.perf_counter(); tr = loop(); torch.cuda.synchronize(); times.append((time.perf_counter() - t0) * 1e3)
say("restated per-sample loop on the device (the reference's host reads), same inputs: ms per step:", ["%.1f" % t for t in times], "host reads per step: %d" % tr.reads)

torch.manual_seed(0)
cfgb = copy.deepcopy(C.H3DNET_SCANNET_BACKBONE)
nets = {"shared": registry.build_backbone(copy.deepcopy(cfgb)).to(dev),
        "independent": registry.build_backbone(dict(copy.deepcopy(cfgb), share_sampling=False)).to(dev)}
nets["independent"].load_state_dict(nets["shared"].state_dict())
pts4 = points[..., :4].contiguous()
def step(net):
    net.zero_grad(set_to_none=True)
    net(pts4)["hd_feature"].square().mean().backward()
for name in nets:
    for _ in range(2): step(nets[name])
torch.cuda.synchronize()
rec = {k: [] for k in nets}
for rep in range(4):
    for name in nets:
        t0 = time.perf_counter()
        for _ in range(3): step(nets[name])
        torch.cuda.synchronize(); rec[name].append((time.perf_counter() - t0) / 3 * 1e3)
for name in nets:
    say("MultiBackbone (4 streams, ScanNet config) forward + backward, B %d N %d, %s sampling: ms per step, 4 alternating x 3 runs:" % (B, N, name), ["%.1f" % t for t in rec[name]])
