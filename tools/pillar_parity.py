#!/usr/bin/env python
"""Writes profiles/pillar_parity.txt: for every forward and backward case of
tests/test_gpu_pillar.py, the error of the float32 torch restatement of the reference's op
sequence against the float64 one (the yardstick) and the error of the fused PillarFeatureNet
(csrc/pillar.hip) against the same float64 result, both scaled by the largest float64 entry.

    python tools/pillar_parity.py [--out profiles/pillar_parity.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pillar_fixture as PF  # noqa: E402
import test_gpu_pillar as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pillar_parity.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["# scaled error against float64 (max |a - b| / max |b|): fp32 torch restatement, fused "
             "kernel, ratio", "# bound of the tests: fused <= max(%g x fp32 torch, %g)"
             % (T.MARGIN, T.FLOOR)]
    worst = 0.0

    def row(tag, what, base, err):
        nonlocal worst
        ratio = err / max(base, 1e-30)
        if err > T.FLOOR:
            worst = max(worst, ratio)
        lines.append("%-44s %-7s fp32 %.3e  fused %.3e  ratio %6.2f" % (tag, what, base, err, ratio))

    for case in T.FORWARD:
        n, m, c, u, training, mode, legacy, distance = case
        tag = "fwd N%d M%d C%d U%d %s %s %s%s" % (n, m, c, u, "train" if training else "eval", mode,
                                                 "legacy" if legacy else "new",
                                                 " dist" if distance else "")
        mod = T._encoder(dev, c, u, training, mode, legacy, distance)
        inputs = PF.make_pillars(n, m, c, seed=n + m, device=dev)
        with torch.no_grad():
            y64 = PF.reference_sequence(mod, *inputs, torch.float64, *T._leaves(mod, torch.float64))
            y32 = PF.reference_sequence(mod, *inputs, torch.float32, *T._leaves(mod, torch.float32))
            out = mod(*inputs)
        row(tag, "out", PF.scaled_err(y32, y64), PF.scaled_err(out, y64))
    for case in T.BACKWARD:
        n, m, c, u, training, mode, legacy, distance = case
        tag = "bwd N%d M%d C%d U%d %s %s" % (n, m, c, u, "train" if training else "eval", mode)
        mod = T._encoder(dev, c, u, training, mode, legacy, distance, seed=9)
        inputs = PF.make_pillars(n, m, c, seed=3 * n + m, device=dev)
        go = torch.randn((n, u), generator=torch.Generator().manual_seed(n)).to(dev)
        go, _ = PF.unambiguous_grad_out(mod, inputs, go)
        g64 = PF.reference_grads(mod, inputs, go, torch.float64)
        g32 = PF.reference_grads(mod, inputs, go, torch.float32)
        out = mod(*inputs)
        out.backward(go)
        pfn = mod.pfn_layers[0]
        got = (out.detach(), pfn.linear.weight.grad, pfn.norm.weight.grad, pfn.norm.bias.grad)
        for what, a, b32, b64 in zip(("out", "dW", "dgamma", "dbeta"), got, g32, g64):
            row(tag, what, PF.scaled_err(b32, b64), PF.scaled_err(a, b64))
    lines.append("# worst ratio among the rows above the floor: %.2f" % worst)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
