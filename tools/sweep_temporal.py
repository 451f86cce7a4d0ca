"""Parameter sweep of temporal accumulation (extension) on the moving-camera sequence of
tests/test_gpu_temporal.py (developer tool): 128x128, scene and cornell2, eight frames of 1 x Subpixel(2) samples, the camera
translating by about a pixel per frame; relMSE against 1024 samples per pixel at the last pose from another seed.

Usage: python tools/sweep_temporal.py [--json PATH]
One parameter is varied at a time around the starting values; per setting the ratios relMSE(temporal) / relMSE(last frame alone)
and relMSE(denoise(temporal)) / relMSE(denoise(last frame)) of both scenes, and the ratio of a buffer that naively kept adding
samples while the camera moved."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import torch  # noqa: E402

import bendy_tracer_amd as b  # noqa: E402
from test_gpu_temporal import moving_camera_ratios  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "sweep_temporal.py needs a GPU"

START = dict(alpha_min=0.05, max_history=256.0, depth_tolerance=0.05, normal_min=0.9)
GRID = dict(alpha_min=[0.0, 0.1, 0.2, 0.4], max_history=[8.0, 16.0, 64.0], depth_tolerance=[0.01, 0.02, 0.1, 0.2],
            normal_min=[0.0, 0.5, 0.7, 0.98])
settings = [dict(START)] + [{**START, k: v} for k, vs in GRID.items() for v in vs] + [{**START, "normal_min": 0.5, "depth_tolerance": 0.1}]
rows = []
for p in settings:
    row = dict(params=p)
    for name in ("scene", "cornell2"):
        r = moving_camera_ratios(b, name, p)
        row[name] = {k: round(v, 5) for k, v in r.items()}
    row["worst_temporal"] = max(row[n]["temporal"] for n in ("scene", "cornell2"))
    row["worst_denoised"] = max(row[n]["denoised"] for n in ("scene", "cornell2"))
    rows.append(row)
    print(json.dumps(row), flush=True)
shipped = dict(defaults=True)
for name in ("scene", "cornell2"):
    shipped[name] = {k: round(v, 5) for k, v in moving_camera_ratios(b, name).items()}
print(json.dumps(shipped), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), start=START, rows=rows, shipped_defaults=shipped), f, indent=1)
