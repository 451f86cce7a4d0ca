"""Parameter sweep of the despeckle stage (extension) on the frames of tests/test_gpu_despeckle.py (developer tool):
128x128, scene, cornell2 and volume, 4 x Subpixel(2) samples; relMSE against 1024 samples per pixel from another seed.

Usage: python tools/sweep_despeckle.py [--json PATH]
One parameter is varied at a time around the starting values; per setting and scene the ratios relMSE(despeckled) / relMSE(raw)
and relMSE(denoise(despeckled)) / relMSE(denoise(raw)), the share of the noisy frame's pixels that is flagged, and the cost to
legitimate detail measured on the truth frame itself: the share of its pixels the stage flags and relMSE(despeckle(truth), truth)."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import torch  # noqa: E402

import bendy_tracer_amd as b  # noqa: E402
from test_gpu_despeckle import quality  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "sweep_despeckle.py needs a GPU"

SCENES = ("scene", "cornell2", "volume")
START = dict(radius=1, rank=2, ratio=4.0, floor=0.01)
GRID = dict(rank=[1, 3, 4], ratio=[1.5, 2.0, 3.0, 6.0, 8.0, 16.0], radius=[2], floor=[0.0, 0.1])
settings = [dict(START)] + [{**START, k: v} for k, vs in GRID.items() for v in vs] + [{**START, "radius": 2, "rank": r} for r in (4, 6)]
rows = []
for p in settings:
    row = dict(params=p)
    for name in SCENES:
        row[name] = {k: float("%.5g" % v) for k, v in quality(b, name, p).items()}
    row["worst_plain"] = max(row[n]["plain"] for n in SCENES)
    row["worst_denoised"] = max(row[n]["denoised"] for n in SCENES)
    rows.append(row)
    print(json.dumps(row), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), start=START, rows=rows), f, indent=1)
