#!/usr/bin/env python
"""Dump the `model` dict of the reference's MVX-Net KITTI config with dynamic voxelization to
JSON (values only -- the dict is a fact), without its `img_backbone` / `img_neck` entries: the
image branch is injected, not built.  Runs in the build container, where /root/reference exists;
the result is committed as reference_mvxnet_config.json and pins
msmdfusion_amd.configs.MVXNET_DV_SECOND_KITTI (tests/test_point_fusion_cpu.py).

    python tests/golden/make_mvxnet_config_fixture.py
"""
import json
import os

REF = "/root/reference/configs"
NAME = "mvxnet/dv_mvx-fpn_second_secfpn_adamw_2x8_80e_kitti-3d-3class.py"
INJECTED = ("img_backbone", "img_neck")


def main():
    ns = {}
    exec(compile(open(os.path.join(REF, NAME)).read(), NAME, "exec"), ns)   # plain-Python config
    model = {k: v for k, v in ns["model"].items() if k not in INJECTED}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_mvxnet_config.json")
    json.dump(dict(model=model, injected=list(INJECTED)), open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst)


if __name__ == "__main__":
    main()
