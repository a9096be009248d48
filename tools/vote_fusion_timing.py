#!/usr/bin/env python
"""VoteFusion and sample_valid_seeds at the ImVoteNet stage-2 shape (batch 8, 1024 seeds, 100
2-D boxes per sample, 10 classes, 3 imvotes per pixel): the fused VoteFusion.forward beside
forward_composed (the reference's op sequence) on the same inputs, and the batched
sample_valid_seeds beside the reference's per-sample loop.  One JSON line per quantity, with
the kernel launches of one call.

    python tools/vote_fusion_timing.py [--repeat 20] [--rounds 5] [--out FILE]

Times are device events around `repeat` back-to-back calls, after warm-up calls of the same
shape; the two versions alternate round by round and the median round is reported.  Needs a
GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imvote_ref as R  # noqa: E402
from msmdfusion_amd.detector import sample_valid_seeds  # noqa: E402
from msmdfusion_amd.fusion_layers import VoteFusion  # noqa: E402

BATCH, SEEDS, BOXES, CLASSES, IMVOTES = 8, 1024, 100, 10, 3


def window(fn, repeat):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(repeat):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / repeat


def launches(fn):
    """Device kernels of one call, counted by the profiler."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def compare(name, ours, theirs, repeat, rounds):
    for fn in (ours, theirs):
        for _ in range(3):
            fn()
    a, b = [], []
    for _ in range(rounds):
        a.append(window(ours, repeat))
        b.append(window(theirs, max(1, repeat // 4)))
    row = dict(quantity=name, repeat=repeat, rounds=rounds, ours_ms_median=statistics.median(a),
               ours_ms_min=min(a), reference_sequence_ms_median=statistics.median(b),
               reference_sequence_ms_min=min(b), ours_launches=launches(ours),
               reference_sequence_launches=launches(theirs))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    case = R.make_case(7, SEEDS, (BOXES,) * BATCH, CLASSES)
    inputs = R.to_torch(case, dev)
    layer = VoteFusion(CLASSES, IMVOTES)
    rows = [compare("VoteFusion.forward", lambda: layer(*inputs),
                    lambda: layer.forward_composed(*inputs), args.repeat, args.rounds)]
    feat, mask = layer(*inputs)
    comp_f, comp_m = layer.forward_composed(*inputs)
    assert torch.equal(mask, comp_m) and float((feat - comp_f).abs().max()) < 1e-4
    gen = torch.Generator(device=dev).manual_seed(0)
    rows.append(compare("sample_valid_seeds", lambda: sample_valid_seeds(mask, SEEDS, gen),
                        lambda: R.sample_valid_seeds_loop(mask, SEEDS, gen), args.repeat,
                        args.rounds))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
