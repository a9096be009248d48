#!/usr/bin/env python
"""Dump the dicts of the reference's configs/_base_/models/h3dnet.py to JSON (values only -- the
dicts are facts): the MultiBackbone config, the three PrimitiveHead configs and, kept as data
for the second stage, the model's train_cfg / test_cfg.  Runs in the build container, where
/root/reference exists; the result is committed as reference_h3dnet_config.json and pins
msmdfusion_amd.configs.H3DNET_SCANNET_BACKBONE / H3DNET_PRIMITIVE_{Z,XY,LINE}
(tests/test_primitive_head_cpu.py).

    python tests/golden/make_h3dnet_config_fixture.py
"""
import json
import os

REF = "/root/reference/configs"


def main():
    path = "_base_/models/h3dnet.py"
    ns = {}
    exec(compile(open(os.path.join(REF, path)).read(), path, "exec"), ns)   # plain-Python config
    model = ns["model"]
    out = dict(backbone=model["backbone"], primitive_z=ns["primitive_z_cfg"],
               primitive_xy=ns["primitive_xy_cfg"], primitive_line=ns["primitive_line_cfg"],
               train_cfg=model["train_cfg"], test_cfg=model["test_cfg"])
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_h3dnet_config.json")
    json.dump(out, open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst)


if __name__ == "__main__":
    main()
