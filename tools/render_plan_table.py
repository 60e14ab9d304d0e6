#!/usr/bin/env python3
"""Records what tests/test_render_plan.py compares with: tests/golden/render_plans.tsv, what pt_plan.cpp's plan_scene and plan_render choose for every scene,
render kind and tuning of tests/render_plan_cases.py on a device of 256 CUs (for a named scene one full line and then the fields each kind and tuning changes, by name; one SHA-256 per fuzz seed).  Run it only when a
change MEANS to move a choice, and read the diff: a refactor of the plan leaves the file as it is.

    python tools/render_plan_table.py [--out DIR]     (DIR: where to write; default tests/golden)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import render_plan_cases as cases   # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    out = ap.parse_args().out
    with open(os.path.join(out, "render_plans.tsv"), "w") as f:
        f.write("\n".join(cases.table(*cases.load())) + "\n")


if __name__ == "__main__":
    main()
