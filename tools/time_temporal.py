"""HIP-event times of temporal accumulation with reprojection (extension) at 768x512 and 1920x1080 (developer tool).

Usage: python tools/time_temporal.py [--reps 50] [--json PATH]
Renders scene.json's colour, normal and depth (1 x Subpixel(2)) on the GPU, warms the handle up, then times `reps` back-to-back
bt_temporal_accumulate_device calls between two events, once with a view that alternates between two poses (every call
reprojects) and once with the same view (every call takes the pixel's own history), and reports the mean per call with the
bytes one call moves: 48 B of sums read and 48 B written per pixel (out, history, guides) through HBM / the Infinity Cache,
plus the gathered history and guide taps (eight 16-B taps per pixel when the camera moves, one when it does not), which
neighbouring pixels share and the caches serve."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bendy_tracer_amd as b  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--json", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_temporal.py needs a GPU"

rows = []
for w, h in ((768, 512), (1920, 1080)):
    sc = b.Scene.load(os.path.join(HERE, "..", "scenes", "scene.json.gz"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    rc = b.RenderConfig(samples=1, subsample=b.Subsample(2))
    color, normal, depth = b.Buffer.new(w, h), b.Buffer.new(w, h), b.Buffer.new(w, h)
    b.Tracer.new().render_guided(sc, cam, rc, color, None, normal, depth, seed=1)
    views = [sc.camera_view(cam, b.Config(), rc, w, h)]
    m = views[0].matrix()
    m[9:] += np.float32(0.03) * m[:3]                      # about a pixel at 768 wide, along the camera's own x axis
    sc.set_camera_pose(cam, m)
    views.append(sc.camera_view(cam, b.Config(), rc, w, h))
    t = b.Temporal(w, h)
    out = b.Buffer.new(w, h)
    for mode, seq in (("moving", views), ("static", views[:1])):
        t.reset()
        for i in range(6):
            t.accumulate(seq[i % len(seq)], color, normal, depth, out=out)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(args.reps):
            t.accumulate(seq[i % len(seq)], color, normal, depth, out=out)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.reps
        px = w * h
        stream_bytes, tap_bytes = px * 96, px * 16 * (8 if mode == "moving" else 1)
        row = dict(width=w, height=h, view=mode, reps=args.reps, us_per_call=round(ms * 1e3, 2), stream_bytes=stream_bytes,
                   tap_bytes=tap_bytes, stream_tb_s=round(stream_bytes / (ms * 1e-3) / 1e12, 3),
                   mean_history=round(float(t.history()[..., 3].mean()), 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    t.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
