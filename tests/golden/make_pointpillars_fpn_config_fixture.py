#!/usr/bin/env python
"""Dump the `model` dict of the reference's nuScenes PointPillars-FPN base config and the same
dict with the FreeAnchor config merged over it (as mmcv's Config merges: a dict carrying
`_delete_=True` replaces, any other dict updates key by key) to JSON (values only -- the dicts
are facts).  Runs in the build container, where /root/reference exists; the result is committed
as reference_pointpillars_fpn_configs.json and pins msmdfusion_amd.configs.POINTPILLARS_FPN_NUS
/ FREE_ANCHOR_POINTPILLARS_FPN_NUS (tests/test_hard_vfe_cpu.py).

    python tests/golden/make_pointpillars_fpn_config_fixture.py
"""
import copy
import json
import os

REF = "/root/reference/configs"
BASE = "_base_/models/hv_pointpillars_fpn_nus.py"
FREE = "free_anchor/hv_pointpillars_fpn_sbn-all_free-anchor_4x8_2x_nus-3d.py"


def load(name):
    ns = {}
    exec(compile(open(os.path.join(REF, name)).read(), name, "exec"), ns)   # plain-Python config
    return ns["model"]


def merge(base, over):
    out = copy.deepcopy(base)
    for k, v in over.items():
        if isinstance(v, dict) and v.get("_delete_"):
            out[k] = {kk: vv for kk, vv in v.items() if kk != "_delete_"}
        elif isinstance(v, dict) and isinstance(out.get(k), dict):
            out[k] = merge(out[k], v)
        else:
            out[k] = copy.deepcopy(v)
    return out


def main():
    base = load(BASE)
    out = dict(pointpillars_fpn_nus=base, free_anchor_pointpillars_fpn_nus=merge(base, load(FREE)))
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "reference_pointpillars_fpn_configs.json")
    json.dump(out, open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst)


if __name__ == "__main__":
    main()
