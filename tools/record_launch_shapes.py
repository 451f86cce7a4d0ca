#!/usr/bin/env python3
"""Record the launch shapes of tests/launch_shape_cases.py on the GPU.

    python tools/record_launch_shapes.py [--out tests/golden/launch_shapes.json]

Every case is rendered on a fresh Scene handle through the public API only (so the tool runs against any earlier build of
the library) and the launch-shape fields of its bt_stats are written, with the device's multi_processor_count, to the JSON
file that tests/test_gpu_launch_shapes.py and tests/test_launch_plan.py compare against.  Record on the commit BEFORE a
change to the launch planner, never after it: the file is the yardstick of such a change."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "launch_shapes.json"))
    args = ap.parse_args()
    import torch

    import bendy_tracer_amd as b
    from launch_shape_cases import CASES, render_case

    torch.cuda.set_device(0)
    doc = {"device": torch.cuda.get_device_name(0),
           "multi_processor_count": torch.cuda.get_device_properties(0).multi_processor_count,
           "cases": {}}
    for case in CASES:
        doc["cases"][case["id"]] = render_case(b, case)
        print(case["id"], doc["cases"][case["id"]], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
