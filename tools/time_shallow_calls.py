#!/usr/bin/env python3
"""Host overhead of a shallow render call: calls per second of back-to-back bt_render_device calls in the interactive
pattern (scene.json 768 x 512, 1 sample x Subpixel(2) per call, main.rs:234-254), where the 0.1 ms kernel leaves the host
side of the call -- fill_launch, the launch planner, the counter ring, the mask key -- in plain sight.

    python tools/time_shallow_calls.py [--calls 3000] [--rounds 3] [--label NAME] [--json out.json]

Public API only, so it runs against any build of the library; A/B two builds by running it alternately with each."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch

    import bendy_tracer_amd as b

    torch.cuda.set_device(0)
    w, h = 768, 512
    sc = b.Scene.load(os.path.join(ROOT, "scenes", "scene.json.gz"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    buf, tr = b.Buffer.new(w, h), b.Tracer.new()
    rc = b.RenderConfig.with_samples_subsample(1, b.Subsample.subpixel(2))
    for _ in range(200):
        tr.render(sc, cam, rc, buf)
    torch.cuda.synchronize()
    rates = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            tr.render(sc, cam, rc, buf)
        torch.cuda.synchronize()
        rates.append(args.calls / (time.perf_counter() - t0))
    out = {"label": args.label, "workload": f"scene {w}x{h}, 1 sample x Subpixel(2) per call", "calls": args.calls,
           "calls_per_s": [round(r, 1) for r in rates]}
    print(json.dumps(out), flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
