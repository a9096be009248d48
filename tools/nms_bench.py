"""Time the batched device-side NMS against a restatement of the reference's flow.

    python tools/nms_bench.py [--out profiles/nms_bench.txt]

6 tasks x batch 4 = 24 lists of n = 1000 boxes, rotated (thresh 0.2) and circle (thresh 0.5),
post_max_size 83.  Two timings per kind:

  batched    iou3d.nms_batched: sort in torch, one mask launch, one reduce launch, no host read
  reference  what mmdet3d/ops/iou3d/src/iou3d.cpp nms_gpu does, per list: mask on the device
             (here the same mask kernel, one list per call), copy of the mask to the host, the
             greedy reduction on the host (a Python loop over numpy words, slower than the
             reference's C++ loop: read the figure as an upper bound).  For circle the
             reference has no device half at all (a numba loop over host copies of the boxes); the same restated flow
             stands in for it, which flatters it.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msmdfusion_amd import iou3d  # noqa: E402
from msmdfusion_amd import kernels as K  # noqa: E402

TASKS, BATCH, N, POST = 6, 4, 1000, 83


def boxes_and_scores(dev, seed=0):
    rng = np.random.default_rng(seed)
    total = TASKS * BATCH * N
    xy = rng.uniform(0, 40, (total, 2))
    wl = rng.uniform(1.0, 5.0, (total, 2))
    r = rng.uniform(-np.pi, np.pi, (total, 1))
    boxes = np.concatenate([xy - wl / 2, xy + wl / 2, r], 1).astype(np.float32)
    return torch.from_numpy(boxes).to(dev), torch.from_numpy(rng.random(total).astype(np.float32)).to(dev)


def host_reduce(mask, n):
    """iou3d.cpp:128-143 on the copied mask [n, words] (uint64); like it, reads only the words
    on and after the row's own (the words before were never written)."""
    words = mask.shape[1]
    removed = np.zeros(words, np.uint64)
    keep = []
    for i in range(n):
        if not (int(removed[i >> 6]) >> (i & 63)) & 1:
            keep.append(i)
            removed[i >> 6:] |= mask[i, i >> 6:]
    return keep


def reference_flow(kind, boxes, scores, thresh):
    """Per list: sort, mask kernel, device -> host copy, host reduction, indices back."""
    dev, out = boxes.device, []
    words = (N + 63) // 64
    offsets = torch.tensor([0, N], dtype=torch.int32, device=dev)
    th = torch.full((1,), thresh, dtype=torch.float32, device=dev)
    ws = torch.zeros(K.nms_workspace_bytes(N, N), dtype=torch.uint8, device=dev)
    for s in range(TASKS * BATCH):
        b, sc = boxes[s * N:(s + 1) * N], scores[s * N:(s + 1) * N]
        order = sc.sort(0, descending=True)[1]
        K.nms_segments(kind, b[order].contiguous(), offsets, th, N, post_max=0, workspace=ws)
        mask = ws[:N * words * 8].cpu().numpy().view(np.uint64).reshape(N, words)
        keep = torch.tensor(host_reduce(mask, N)[:POST], dtype=torch.long).to(dev)
        out.append(order[keep] + s * N)          # row indices into the whole batch
    return out


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "nms_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    boxes, scores = boxes_and_scores(dev)
    offsets = torch.arange(TASKS * BATCH + 1, dtype=torch.int32, device=dev) * N
    lines = ["nms_bench: %d tasks x batch %d x n = %d, post_max_size %d, ms per call "
             "(median / min)" % (TASKS, BATCH, N, POST)]
    for kind, cols, thresh in (("rotate", boxes, 0.2), ("circle", boxes[:, :2].contiguous(), 0.5)):
        batched = lambda: iou3d.nms_batched(kind, cols, scores, offsets, thresh, N, POST)  # noqa
        keep, num = batched()
        ref = reference_flow(kind, cols, scores, thresh)
        for s, r in enumerate(ref):            # the two flows agree (distinct scores: no ties)
            assert keep[s, :int(num[s])].tolist() == r.tolist(), (kind, s)
        med, low = timed(batched, 20)
        lines.append("%-7s batched   (1 call, no host read)          %9.3f / %9.3f" % (kind, med, low))
        med, low = timed(lambda: reference_flow(kind, cols, scores, thresh), 3)
        lines.append("%-7s reference (24 x mask, copy, host reduce)  %9.3f / %9.3f" % (kind, med, low))
    lines += ["'reference' is NOT the reference's code: the same device mask kernel per list (the call",
              "also runs the device reduce and allocates its outputs), a copy of the mask to the host",
              "and a Python loop over numpy words where the reference has a C++ loop; for circle the",
              "reference has no device half at all.  Read it as an upper bound on that flow here, not",
              "as a measured speed-up over the reference's C++."]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
