#!/usr/bin/env python
"""Writes profiles/hard_vfe_parity.txt: for every forward and gradient case of
tests/test_gpu_hard_vfe.py, the error of the float32 torch restatement of the reference's op
sequence against the float64 one (the yardstick) and the error of the fused HardVFE
(csrc/hard_vfe.hip) against the same float64 result, both scaled by the largest float64 entry;
for the gradient cases also what the float64 restatement left out (hard_vfe_fixture.exclusions).

    python tools/hard_vfe_parity.py [--out profiles/hard_vfe_parity.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hard_vfe_fixture as HF  # noqa: E402
import test_gpu_hard_vfe as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hard_vfe_parity.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["# scaled error against float64 (max |a - b| / max |b|): fp32 torch restatement, fused "
             "kernels, ratio", "# bound of the tests: fused <= max(%g x fp32 torch, %g)"
             % (T.MARGIN, T.FLOOR)]
    worst = 0.0

    def row(tag, what, base, err):
        nonlocal worst
        ratio = err / max(base, 1e-30)
        if err > T.FLOOR:
            worst = max(worst, ratio)
        lines.append("%-40s %-8s fp32 %.3e  fused %.3e  ratio %6.2f" % (tag, what, base, err, ratio))

    for n, m, c, widths, training, kind in T.FORWARD:
        n = n or T._steps_n()
        tag = "fwd N%d M%d C%d %s %s %s" % (n, m, c, "x".join(map(str, widths)),
                                            "train" if training else "eval", kind)
        mod = HF.encoder(dev, c, widths, training)
        inputs = HF.make_voxels(n, m, c, seed=n + m, device=dev, kind=kind)
        with torch.no_grad():
            y64 = HF.reference_sequence(mod, *inputs, torch.float64, HF.leaves(mod, torch.float64))
            y32 = HF.reference_sequence(mod, *inputs, torch.float32, HF.leaves(mod, torch.float32))
            out = mod(*inputs)
        row(tag, "out", HF.scaled_err(y32, y64), HF.scaled_err(out, y64))
    for layers, training, n, m, seed in T.GRADS:
        tag = "bwd L%d %s N%d M%d" % (layers, "train" if training else "eval", n, m)
        mod = HF.encoder(dev, 4, (64, 64)[:layers], training, seed=9)
        inputs = HF.make_voxels(n, m, 4, seed=seed, device=dev)
        go = torch.randn((n, 64), generator=torch.Generator().manual_seed(n)).to(dev)
        go, zeroed, channels_out = HF.exclusions(mod, inputs, go)
        lines.append("%-40s left out: %.3f %% of grad_out, %d layer-1 channels" % (
            tag, 100 * zeroed, 0 if channels_out is None else int(channels_out.sum())))
        y64, g64 = HF.reference_grads(mod, inputs, go, torch.float64)
        y32, g32 = HF.reference_grads(mod, inputs, go, torch.float32)
        out = mod(*inputs)
        out.backward(go)
        row(tag, "out", HF.scaled_err(y32, y64), HF.scaled_err(out, y64))
        names = ["dW1", "dgamma1", "dbeta1", "dW2", "dgamma2", "dbeta2"][:3 * layers]
        for i, (what, a, b32, b64) in enumerate(zip(names, HF.module_grads(mod), g32, g64)):
            if i < 3 and channels_out is not None:
                keep = ~channels_out
                a, b32, b64 = a[keep], b32[keep], b64[keep]
            row(tag, what, HF.scaled_err(b32, b64), HF.scaled_err(a, b64))
    lines.append("# worst ratio among the rows above the floor: %.2f" % worst)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
