#!/usr/bin/env python
"""Dump the `model` dicts of the reference's two KITTI anchor-head base configs to JSON (values
only -- the dicts are facts).  Runs in the build container, where /root/reference exists; the
result is committed as reference_anchor_head_configs.json and pins
msmdfusion_amd.configs.POINTPILLARS_SECFPN_KITTI / SECOND_SECFPN_KITTI
(tests/test_anchor_head_cpu.py).

    python tests/golden/make_anchor_head_config_fixture.py
"""
import json
import os

REF = "/root/reference/configs/_base_/models"


def load(name):
    ns = {}
    exec(compile(open(os.path.join(REF, name)).read(), name, "exec"), ns)   # plain-Python config
    return dict(model=ns["model"])


def main():
    out = {"hv_pointpillars_secfpn_kitti": load("hv_pointpillars_secfpn_kitti.py"),
           "hv_second_secfpn_kitti": load("hv_second_secfpn_kitti.py")}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "reference_anchor_head_configs.json")
    json.dump(out, open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst)


if __name__ == "__main__":
    main()
