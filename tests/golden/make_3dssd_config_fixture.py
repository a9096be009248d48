#!/usr/bin/env python
"""Dump the `model` dict of the reference's 3DSSD config to JSON (values only -- the dict is a
fact): configs/_base_/models/3dssd.py with the `model` override of
configs/3dssd/3dssd_kitti-3d-car.py merged into it the way mmcv's Config merges a child over its
`_base_`.  Runs in the build container, where /root/reference exists; the result is committed as
reference_3dssd_config.json and pins msmdfusion_amd.configs.SSD3D_KITTI_CAR
(tests/test_ssd3d_head_cpu.py).

    python tests/golden/make_3dssd_config_fixture.py
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
    out = {"3dssd_kitti-3d-car":
           dict(model=merge(load("_base_/models/3dssd.py"), load("3dssd/3dssd_kitti-3d-car.py")))}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_3dssd_config.json")
    json.dump(out, open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst)


if __name__ == "__main__":
    main()
