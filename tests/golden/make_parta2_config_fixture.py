#!/usr/bin/env python
"""Dump the `model` dicts (train_cfg and test_cfg inside, as the files have them) of the
reference's two Part-A2 configs to JSON (values only -- the dicts are facts).  Runs in the build
container, where /root/reference exists; the result is committed as
reference_parta2_configs.json and pins msmdfusion_amd.configs.PARTA2_SECFPN_KITTI_3CLASS /
PARTA2_SECFPN_KITTI_CAR (tests/test_parta2_first_stage_cpu.py).

The car file names the 3-class file as its _base_; mmcv is absent, so its merge rule is written
out here from mmcv.Config._merge_a_into_b: a dict value is merged key by key into the base's,
unless it carries _delete_=True, which replaces the base's value; anything else replaces.

    python tests/golden/make_parta2_config_fixture.py
"""
import json
import os

REF = "/root/reference/configs/parta2"


def merge(a, b):
    b = dict(b)
    for k, v in a.items():
        if isinstance(v, dict) and isinstance(b.get(k), dict) and not v.get("_delete_", False):
            b[k] = merge(v, b[k])
        elif isinstance(v, dict):
            b[k] = {kk: vv for kk, vv in v.items() if kk != "_delete_"}
        else:
            b[k] = v
    return b


def load(name):
    ns = {}
    exec(compile(open(os.path.join(REF, name)).read(), name, "exec"), ns)   # plain-Python config
    model = ns["model"]
    base = ns.get("_base_")
    if isinstance(base, str) and "PartA2" in base:
        model = merge(model, load(os.path.basename(base))["model"])
    return dict(model=model)


def main():
    out = {"kitti-3d-3class": load("hv_PartA2_secfpn_2x8_cyclic_80e_kitti-3d-3class.py"),
           "kitti-3d-car": load("hv_PartA2_secfpn_2x8_cyclic_80e_kitti-3d-car.py")}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "reference_parta2_configs.json")
    json.dump(out, open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst)


if __name__ == "__main__":
    main()
