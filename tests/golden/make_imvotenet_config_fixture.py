#!/usr/bin/env python
"""Dump the `model` dict of the reference's ImVoteNet stage-2 config to JSON (values only -- the
dict is a fact): configs/_base_/models/imvotenet_image.py with the `model` of
configs/imvotenet/imvotenet_stage2_16x8_sunrgbd-3d-10class.py merged into it the way mmcv's
Config merges a child over its `_base_`, without the image branch (`img_backbone`, `img_neck`,
`img_rpn_head`, `img_roi_head` and the `img_*` entries of train_cfg / test_cfg): the 2-D
detector is injected, not built.  Runs in the build container, where /root/reference exists;
the result is committed as reference_imvotenet_config.json and pins
msmdfusion_amd.configs.IMVOTENET_STAGE2_SUNRGBD (tests/test_vote_fusion_cpu.py).

    python tests/golden/make_imvotenet_config_fixture.py
"""
import copy
import json
import os

REF = "/root/reference/configs"
INJECTED = ("img_backbone", "img_neck", "img_rpn_head", "img_roi_head")


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
    model = merge(load("_base_/models/imvotenet_image.py"),
                  load("imvotenet/imvotenet_stage2_16x8_sunrgbd-3d-10class.py"))
    model = {k: v for k, v in model.items() if k not in INJECTED}
    for key in ("train_cfg", "test_cfg"):
        model[key] = {k: v for k, v in model[key].items() if not k.startswith("img_")}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "reference_imvotenet_config.json")
    json.dump(dict(model=model, injected=list(INJECTED)), open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst)


if __name__ == "__main__":
    main()
