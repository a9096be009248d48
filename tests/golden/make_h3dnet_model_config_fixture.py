#!/usr/bin/env python
"""Dump the whole H3DNet ScanNet model config of the reference to JSON (values only -- the dicts
are facts): configs/_base_/models/h3dnet.py with the `model` dict of
configs/h3dnet/h3dnet_3x8_scannet-3d-18class.py merged into it the way mmcv's Config merges a
child over its `_base_` (dicts recurse, everything else is replaced).  Runs in the build
container, where /root/reference exists; the result is committed as
reference_h3dnet_model_config.json and pins msmdfusion_amd.configs.H3DNET_SCANNET
(tests/test_h3d_head_cpu.py).

    python tests/golden/make_h3dnet_model_config_fixture.py
"""
import json
import os

REF = "/root/reference/configs"


def load(path):
    ns = {}
    exec(compile(open(os.path.join(REF, path)).read(), path, "exec"), ns)   # plain-Python config
    return ns


def merge(base, child):
    for key, value in child.items():
        if isinstance(value, dict) and isinstance(base.get(key), dict):
            merge(base[key], value)
        else:
            base[key] = value
    return base


def main():
    model = load("_base_/models/h3dnet.py")["model"]
    merge(model, load("h3dnet/h3dnet_3x8_scannet-3d-18class.py")["model"])
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "reference_h3dnet_model_config.json")
    json.dump(dict(model=model), open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst)


if __name__ == "__main__":
    main()
