#!/usr/bin/env python
"""Dump the reference's two nuScenes TransFusion "LC" configs to JSON (values only -- the dicts
are facts).  Runs in the build container, where /root/reference exists; the result is committed
as reference_transfusion_lc_configs.json and pins msmdfusion_amd.configs.TRANSFUSION_VOXEL_LC and
TRANSFUSION_PILLAR_LC (tests/test_img_fusion_cpu.py).

    python tests/golden/make_transfusion_lc_config_fixture.py
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
    out = {name: load(name + ".py")
           for name in ("transfusion_nusc_voxel_LC", "transfusion_nusc_pillar_LC")}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "reference_transfusion_lc_configs.json")
    json.dump(out, open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst)


if __name__ == "__main__":
    main()
