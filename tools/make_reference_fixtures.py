#!/usr/bin/env python3
"""Writes the fixtures of tests/test_reference_fixtures.py from a checkout of the reference tree (its data files only, never its sources):

  tests/golden/reference_tree/data/...     the config, library and scene files, the data/test inputs of the reference's own parse tests and the
                                           curves / meshes / texture those scenes reach before they load or stop, byte for byte
  tests/golden/reference_showcase.npz      what the two showcase tests read of showcase/*_1080p.png: the 8-bit pixels of each Cornell patch
                                           window, and the 5 x 5 block statistics of the linearised moissanite image (float32)

usage: python tools/make_reference_fixtures.py <reference tree>"""
import os
import shutil
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_reference_fixtures as trf  # noqa: E402  (the decoder and the patch table the tests use)

FILES = ["data/test/cornell.csv", "data/test/gold.csv", "data/test/xenon_lamp.spectra", "data/test/test.png", "data/test/test.bmp",
         "data/curves/basis/simple-spectral-srgb-1931.csv", "data/curves/csv/D65.csv", "data/curves/csv/copper-mcpeak.csv",
         "data/curves/csv/cornell.csv", "data/curves/csv/gold.csv", "data/meshes/brilliant_diamond.obj", "data/meshes/brilliant_diamond.mtl",
         "data/meshes/prism.obj", "data/meshes/prism.mtl", "data/textures/single_pixel.png"]


def main(ref):
    out = os.path.join(ROOT, "tests", "golden", "reference_tree")
    shutil.rmtree(out, ignore_errors=True)
    data = os.path.join(ref, "data")
    names = FILES + ["data/" + f for f in os.listdir(data) if f.endswith(".toml")]
    names += ["data/scenes/" + f for f in os.listdir(os.path.join(data, "scenes")) if f.endswith(".toml")]
    for name in sorted(names):
        os.makedirs(os.path.dirname(os.path.join(out, name)), exist_ok=True)
        shutil.copyfile(os.path.join(ref, name), os.path.join(out, name))

    arrays = {}
    show = trf._decode_png(os.path.join(ref, "showcase", "cornell_box_1080p.png"))[..., :3]
    arrays["cornell shape"] = np.array(show.shape)
    for patch, (cx, cy, _) in trf.CORNELL_PATCHES.items():
        arrays["cornell " + patch] = show[trf._patch_window(show.shape, cx, cy)]
    show = trf._decode_png(os.path.join(ref, "showcase", "moissanite_gem_1080p.png"))[..., :3].astype(np.float64) / 255.0
    arrays["moissanite shape"] = np.array(show.shape)
    for k, v in trf._block_statistics(show).items():
        arrays["moissanite " + k] = v.astype(np.float32)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "reference_showcase.npz"), **arrays)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
