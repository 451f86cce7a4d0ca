"""What the upscale stage (extension) does to the error of a small render shown large, and a parameter sweep around
the starting values (developer tool).

Usage: python tools/sweep_upscale.py [--json PATH] [--no-sweep]
Six rows -- cornell2 64x64 -> 128x128 and 48x48 -> 144x144, cornell 32x32 -> 128x128, scene 64x36 -> 128x72, volume and cloud
60x40 -> 120x80 -- each rendered once: colour and lo guides 4 x Subpixel(2) at the small size (seed 0x5EED), hi guides
1 x Subpixel(2) at the shown size (seed 0xABC), truth 256 x Subpixel(2) at the shown size (seed 777).  Per row: relMSE
(mean((x - y)^2 / (y^2 + 0.01))) of the resample stage's tent, mitchell and lanczos3 on the same colour frame, of
this stage, and of a render at the shown size with the same ray budget (1 x Subpixel(2), seed 0x5EED); the shares of output
pixels that took tier 2 and tier 3; and the share of each total error that the worst 1 % of the pixels carry, so that a reader
sees when a ratio is a few edge pixels.  Then one parameter at a time around the defaults, relMSE per row."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bendy_tracer_amd as b  # noqa: E402
from helpers import gpu_scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default="")
ap.add_argument("--no-sweep", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "sweep_upscale.py needs a GPU"

ROWS = [("cornell2", 64, 64, 128, 128), ("cornell2", 48, 48, 144, 144), ("cornell", 32, 32, 128, 128), ("scene", 64, 36, 128, 72),
        ("volume", 60, 40, 120, 80), ("cloud", 60, 40, 120, 80)]
GRID = dict(sigma_depth=[0.03, 0.3], sigma_albedo=[0.03, 0.3], normal_squarings=[1, 5], min_weight=[0.001, 0.1])
CFG = dict(chunks_x=8, chunks_y=4)


def errors(x, y):
    """-> (relMSE, the share of it that the worst 1 % of the pixels carry)."""
    x, y = x[..., :3].astype(np.float64), y[..., :3].astype(np.float64)
    e = ((x - y) ** 2 / (y ** 2 + 0.01)).mean(axis=-1).ravel()
    worst = np.sort(e)[-max(1, e.size // 100):]
    return float(e.mean()), float(worst.sum() / e.sum()) if e.sum() > 0 else 0.0


def render_row(name, w, h, W, H):
    sc, cam = gpu_scene(b, name, W, H)
    sub = b.Subsample(2)
    lo = [b.Buffer.new(w, h) for _ in range(4)]
    b.Tracer.with_config(b.Config(**CFG)).render_guided(sc, cam, b.RenderConfig(samples=4, subsample=sub), *lo, seed=0x5EED)
    hi = []
    for output in (b.Output.Albedo, b.Output.Normal, b.Output.Depth):
        g = b.Buffer.new(W, H)
        b.Tracer.with_config(b.Config(output=output, **CFG)).render(sc, cam, b.RenderConfig(samples=1, subsample=sub), g, seed=0xABC)
        hi.append(g)
    truth, equal = b.Buffer.new(W, H), b.Buffer.new(W, H)
    b.Tracer.with_config(b.Config(**CFG)).render(sc, cam, b.RenderConfig(samples=256, subsample=sub), truth, seed=777)
    b.Tracer.with_config(b.Config(**CFG)).render(sc, cam, b.RenderConfig(samples=1, subsample=sub), equal, seed=0x5EED)
    torch.cuda.synchronize()
    return lo, tuple(hi), truth.mean(), equal.mean()


frames = {row: render_row(*row) for row in ROWS}
table = []
for row in ROWS:
    name, w, h, W, H = row
    lo, hi, y, equal = frames[row]
    out = dict(scene=name, lo=[w, h], hi=[W, H])
    for filt in ("tent", "mitchell", "lanczos3"):
        out[filt], out[filt + "_worst1"] = errors(b.Resample(filter=filt).apply(lo[0], W, H).numpy(), y)
    handle = b.Upscale()
    out["guided"], out["guided_worst1"] = errors(handle.apply(lo[0], W, H, lo=tuple(lo[1:]), hi=hi).numpy(), y)
    st = handle.poll()
    out["guided_over_tent"] = out["guided"] / out["tent"]
    out["tier2"], out["tier3"] = st.tier2 / st.pixels, st.tier3 / st.pixels
    out["equal_budget"], out["equal_budget_worst1"] = errors(equal, y)
    out = {k: (float("%.5g" % v) if isinstance(v, float) else v) for k, v in out.items()}
    table.append(out)
    print(json.dumps(out), flush=True)

sweep = []
if not args.no_sweep:
    for p in [dict()] + [{k: v} for k, vs in GRID.items() for v in vs]:
        entry = dict(params=p)
        for row in ROWS:
            name, w, h, W, H = row
            lo, hi, y, _ = frames[row]
            entry[f"{name} {w}x{h}"] = float("%.5g" % errors(b.Upscale(**p).apply(lo[0], W, H, lo=tuple(lo[1:]), hi=hi).numpy(), y)[0])
        sweep.append(entry)
        print(json.dumps(entry), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rows=table, sweep=sweep), f, indent=1)
