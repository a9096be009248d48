#!/usr/bin/env python
"""Dump the `model` dicts of two of the reference's CenterPoint configs to JSON (values only --
the dicts are facts).  The configs inherit through `_base_`; mmcv is absent, so its merge (a
child's dict updates the parent's, key by key) is restated here.  Runs in the build container,
where /root/reference exists; the result is committed as reference_centerpoint_configs.json and
pins msmdfusion_amd.configs.CENTERPOINT_VOXEL_NUS / CENTERPOINT_PILLAR_NUS
(tests/test_iou3d_cpu.py).

    python tests/golden/make_centerpoint_config_fixture.py
"""
import json
import os

REF = "/root/reference/configs"
# child last: `_base_/models/*` <- the 4x8 schedule config <- (its 0.075 m child <- circle NMS)
CHAINS = {
    "centerpoint_0075voxel_second_secfpn_circlenms_nus": [
        "_base_/models/centerpoint_01voxel_second_secfpn_nus.py",
        "centerpoint/centerpoint_01voxel_second_secfpn_4x8_cyclic_20e_nus.py",
        "centerpoint/centerpoint_0075voxel_second_secfpn_4x8_cyclic_20e_nus.py",
        "centerpoint/centerpoint_0075voxel_second_secfpn_circlenms_4x8_cyclic_20e_nus.py"],
    "centerpoint_02pillar_second_secfpn_nus": [
        "_base_/models/centerpoint_02pillar_second_secfpn_nus.py",
        "centerpoint/centerpoint_02pillar_second_secfpn_4x8_cyclic_20e_nus.py"],
}


def merge(parent, child):
    out = dict(parent)
    for k, v in child.items():
        out[k] = merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


def load(chain):
    model = {}
    for name in chain:
        ns = {}
        exec(compile(open(os.path.join(REF, name)).read(), name, "exec"), ns)   # plain Python
        model = merge(model, ns["model"])
    return dict(model=model)


def main():
    out = {k: load(v) for k, v in CHAINS.items()}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "reference_centerpoint_configs.json")
    json.dump(out, open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst)


if __name__ == "__main__":
    main()
