#!/usr/bin/env python
"""Dump the `model` dict of the reference's pillar config to JSON (values only -- the dict is
facts).  Runs in the build container, where /root/reference exists; the result is committed as
reference_pillar_config.json and pins msmdfusion_amd.configs.TRANSFUSION_PILLAR_L
(tests/test_pillar_cpu.py).

    python tests/golden/make_pillar_config_fixture.py
"""
import json
import os

REF = "/root/reference/configs"


def load(name):
    ns = {}
    exec(compile(open(os.path.join(REF, name)).read(), name, "exec"), ns)   # plain-Python config
    return dict(model=ns["model"], samples_per_gpu=ns["data"]["samples_per_gpu"],
                point_cloud_range=ns["point_cloud_range"], voxel_size=ns["voxel_size"],
                optimizer=ns["optimizer"],
                freeze_lidar_components=ns.get("freeze_lidar_components", False))


def main():
    out = {"transfusion_nusc_pillar_L": load("transfusion_nusc_pillar_L.py")}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_pillar_config.json")
    json.dump(out, open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst)


if __name__ == "__main__":
    main()
