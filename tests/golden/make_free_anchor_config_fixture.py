#!/usr/bin/env python
"""Dump what the reference's FreeAnchor config sets -- the `pts_bbox_head` dict (without its
`_delete_` merge directive) and `train_cfg` -- to JSON (values only -- the dicts are facts).
Runs in the build container, where /root/reference exists; the result is committed as
reference_free_anchor_config.json and pins msmdfusion_amd.configs.FREE_ANCHOR_HEAD_NUS /
FREE_ANCHOR_TRAIN_CFG_NUS (tests/test_free_anchor_cpu.py).

    python tests/golden/make_free_anchor_config_fixture.py
"""
import json
import os

REF = "/root/reference/configs/free_anchor"
NAME = "hv_pointpillars_fpn_sbn-all_free-anchor_4x8_2x_nus-3d.py"


def main():
    ns = {}
    exec(compile(open(os.path.join(REF, NAME)).read(), NAME, "exec"), ns)   # plain-Python config
    head = {k: v for k, v in ns["model"]["pts_bbox_head"].items() if k != "_delete_"}
    out = dict(pts_bbox_head=head, train_cfg=ns["model"]["train_cfg"])
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "reference_free_anchor_config.json")
    json.dump(out, open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst)


if __name__ == "__main__":
    main()
