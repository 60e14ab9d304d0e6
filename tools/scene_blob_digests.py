#!/usr/bin/env python3
"""Records what tests/test_scene_blob.py compares with: tests/golden/scene_blobs.tsv (per creation case of tests/scene_blob_cases.py: name, blob word
count, SHA-256 of the blob, texel word count, SHA-256 of the texels) and tests/golden/scene_refusals.tsv (per refusal case: name, message).  Run it only when
a change MEANS to move the blob: a refactor of pt_scene_host.cpp leaves both files as they are.

    python tools/scene_blob_digests.py [--out DIR]     (DIR: where to write; default tests/golden)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import scene_blob_cases as cases   # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    out = ap.parse_args().out
    emu, raw = cases.load()
    with open(os.path.join(out, "scene_blobs.tsv"), "w") as f:
        for name, make in cases.creation_cases():
            scene = emu.create_scene(make())
            f.write("\t".join(cases.digest_row(name, cases.scene_words(raw, scene, 0), cases.scene_words(raw, scene, 1))) + "\n")
            scene.close()
    with open(os.path.join(out, "scene_refusals.tsv"), "w") as f:
        for name, make in cases.refusal_cases():
            f.write("%s\t%s\n" % (name, cases.refusal_message(emu, make())))


if __name__ == "__main__":
    main()
