"""HIP-event times of the AOV-guided a-trous denoiser (extension) at 768x512 and 1920x1080 (developer tool).

Usage: python tools/time_denoise.py [--levels 5] [--reps 50] [--json PATH]
Renders scene.json's colour (4 spp) and its three guides (4 spp) on the GPU, warms the denoiser up, then times `reps`
back-to-back bt_denoise_device calls between two events and reports the mean per call, with the bytes one call must
move through HBM at least (each level reads e + guide and writes e: 48 B per pixel; prepare reads the four sums and
writes e + guide: 96 B; the last level also reads the albedo sums: 16 B) and the rate that implies."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import bendy_tracer_amd as b  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--levels", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--json", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_denoise.py needs a GPU"

rows = []
for w, h in ((768, 512), (1920, 1080)):
    sc = b.Scene.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scenes", "scene.json.gz"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    bufs = []
    for o in (b.Output.Full, b.Output.Albedo, b.Output.Normal, b.Output.Depth):
        buf = b.Buffer.new(w, h)
        b.Tracer.with_config(b.Config(output=o)).render(sc, cam, b.RenderConfig.with_samples(4), buf, seed=1)
        bufs.append(buf)
    dn = b.Denoiser()
    out = b.Buffer.new(w, h)
    for _ in range(5):
        dn.denoise(*bufs, out=out, levels=args.levels)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.reps):
        dn.denoise(*bufs, out=out, levels=args.levels)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / args.reps
    px = w * h
    min_bytes = px * (96 + 48 * args.levels + 16)
    row = dict(width=w, height=h, levels=args.levels, reps=args.reps, ms_per_call=round(ms, 4),
               min_hbm_bytes=min_bytes, implied_gb_s=round(min_bytes / (ms * 1e-3) / 1e9, 1))
    rows.append(row)
    print(json.dumps(row), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
