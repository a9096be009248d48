#!/usr/bin/env python
"""Dump the `model` dicts of the reference's two VoteNet configs to JSON (values only -- the
dicts are facts): configs/_base_/models/votenet.py with the `model` overrides of
configs/votenet/votenet_16x8_sunrgbd-3d-10class.py and votenet_8x8_scannet-3d-18class.py merged
into it the way mmcv's Config merges a child over its `_base_`.  Runs in the build container,
where /root/reference exists; the result is committed as reference_votenet_configs.json and pins
msmdfusion_amd.configs.VOTENET_SUNRGBD / VOTENET_SCANNET (tests/test_vote_head_cpu.py).

    python tests/golden/make_votenet_config_fixture.py
"""
import copy
import json
import os

REF = "/root/reference/configs"


def load(path):
    ns = {}
    exec(compile(open(os.path.join(REF, path)).read(), path, "exec"), ns)   # plain-Python config
    return ns["model"]


def merge(base, child):
    """mmcv Config._merge_a_into_b for plain dicts: the child's keys win, dicts merge."""
    out = copy.deepcopy(base)
    for k, v in child.items():
        out[k] = merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


def main():
    base = load("_base_/models/votenet.py")
    out = {"votenet_16x8_sunrgbd-3d-10class":
           dict(model=merge(base, load("votenet/votenet_16x8_sunrgbd-3d-10class.py"))),
           "votenet_8x8_scannet-3d-18class":
           dict(model=merge(base, load("votenet/votenet_8x8_scannet-3d-18class.py")))}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "reference_votenet_configs.json")
    json.dump(out, open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst)


if __name__ == "__main__":
    main()
