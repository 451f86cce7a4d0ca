"""HIP-event times of the glare stage (extension) at 768x512 and 1920x1080 (developer tool).

Usage: python tools/time_glare.py [--reps 50] [--json PATH] [--preview-lib PATH/libbendy_hip.so] [--levels 2,6]
Renders scene.json (1 x Subpixel(2)) on the GPU for a noisy frame, then times `reps` back-to-back calls between two events:
bt_preview_device (the yardstick; with --preview-lib the one of another build of the library, e.g. the parent commit's), a
1x1 bt_preview_device (what a launch costs when the kernel has nothing to do) and bt_glare_device with each level count.

The model a call is held against.  down0 reads the frame's 16 B per pixel and writes a quarter-size float4 plane (4 B per
pixel); the composite reads 16 and writes 16 B per pixel (its four A_1 taps are cached); the levels between touch a third of
that again between them.  The preview moves 20 B per pixel, so
    model = (bytes per pixel / 20) * preview + (2 L - 2) * an empty launch,    bytes per pixel = 16 + 4 + 16 + 16 = 52."""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import torch  # noqa: E402

import bendy_tracer_amd as b  # noqa: E402
from bendy_tracer_amd import api  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--json", default="")
ap.add_argument("--preview-lib", default="")
ap.add_argument("--levels", default="2,6")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_glare.py needs a GPU"

preview_lib = api.lib
if args.preview_lib:
    preview_lib = C.CDLL(args.preview_lib)
    preview_lib.bt_preview_device.argtypes = api.lib.bt_preview_device.argtypes
stream = torch.cuda.current_stream().cuda_stream
BYTES_PER_PIXEL = 16 + 4 + 16 + 16


def timed(call):
    for _ in range(6):
        call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.reps):
        call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / args.reps * 1e3           # microseconds per call


rows = []
for w, h in ((768, 512), (1920, 1080)):
    sc = b.Scene.load(os.path.join(HERE, "..", "scenes", "scene.json.gz"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    noisy = b.Buffer.new(w, h)
    b.Tracer.new().render(sc, cam, b.RenderConfig(samples=1, subsample=b.Subsample(2)), noisy, seed=1)
    rgba8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    tiny_in, tiny_out = torch.ones(4, dtype=torch.float32, device="cuda"), torch.empty(4, dtype=torch.uint8, device="cuda")
    g = b.Glare()

    def preview():
        assert preview_lib.bt_preview_device(noisy.data.data_ptr(), rgba8.data_ptr(), w, h, noisy.samples, 3, stream) == 0

    def launch():
        api._check(api.lib.bt_preview_device(tiny_in.data_ptr(), tiny_out.data_ptr(), 1, 1, 1, 3, stream))

    for rep in range(3):                                   # the spread of the runs: everything three times over
        us_preview, us_launch = timed(preview), timed(launch)
        for levels in (int(v) for v in args.levels.split(",")):
            p = b.GlareParams(levels=levels)._c()

            def glare():
                api._check(api.lib.bt_glare_device(g._h, noisy.data.data_ptr(), noisy.samples, out.data_ptr(), w, h, C.byref(p), stream))
            us = timed(glare)
            model = BYTES_PER_PIXEL / 20.0 * us_preview + (2 * levels - 2) * us_launch
            row = dict(width=w, height=h, run=rep, reps=args.reps, levels=levels, launches=2 * levels, us_preview=round(us_preview, 2),
                       us_launch_1x1=round(us_launch, 2), us_per_call=round(us, 2), model_us=round(model, 2),
                       over_model_us=round(us - model, 2), ratio_to_preview=round(us / us_preview, 3), bytes=w * h * BYTES_PER_PIXEL)
            rows.append(row)
            print(json.dumps(row), flush=True)
    g.close()
    sc = None                                              # freed here, not at interpreter shutdown
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), preview_lib=os.path.basename(os.path.dirname(args.preview_lib)) or "this build",
                       rows=rows), f, indent=1)
