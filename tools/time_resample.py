"""HIP-event times of the resample stage (extension): supersampled still, equal size, interactive upscale (developer tool).

Usage: python tools/time_resample.py [--reps 50] [--json PATH] [--preview-lib PATH/libbendy_hip.so] [--lib PATH/libbendy_hip.so]
                                     [--filters tent,lanczos3]
Renders scene.json (1 x Subpixel(2)) on the GPU for a noisy source frame of each case, then times `reps` back-to-back calls
between two events: bt_preview_device on the SOURCE frame (the yardstick; with --preview-lib the one of another build of the
library, e.g. the parent commit's), a 1x1 bt_preview_device (what a launch costs when the kernel has nothing to do) and
bt_resample_device with each filter (with --lib the one of another build, e.g. `make variant SRC=bt_resample
KFLAGS=-DBT_RESAMPLE_LDS=0`).

The model a call is held against.  The sums are read once (16 B per source pixel), the intermediate plane W x h is written and
read once (32 B per texel), the output is written once (16 B per pixel); taps come from cache or LDS.  The preview moves 20 B
per source pixel, so
    model = (bytes / (20 B * w * h)) * preview + one empty launch,    bytes = 16 w h + 32 W h + 16 W H."""
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

CASES = (((3840, 2160), (1920, 1080)), ((1920, 1080), (1920, 1080)), ((768, 512), (1920, 1080)))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--json", default="")
ap.add_argument("--preview-lib", default="")
ap.add_argument("--lib", default="")
ap.add_argument("--filters", default="tent,lanczos3")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_resample.py needs a GPU"

preview_lib, lib = api.lib, api.lib
if args.preview_lib:
    preview_lib = C.CDLL(args.preview_lib)
    preview_lib.bt_preview_device.argtypes = api.lib.bt_preview_device.argtypes
if args.lib:
    lib = C.CDLL(args.lib)
    for name in ("bt_resample_new", "bt_resample_free", "bt_resample_device", "bt_debug_resample_weights"):
        getattr(lib, name).argtypes = getattr(api.lib, name).argtypes
    lib.bt_resample_new.restype = C.c_void_p
stream = torch.cuda.current_stream().cuda_stream


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
for (w, h), (W, H) in CASES:
    sc = b.Scene.load(os.path.join(HERE, "..", "scenes", "scene.json.gz"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    noisy = b.Buffer.new(w, h)
    b.Tracer.new().render(sc, cam, b.RenderConfig(samples=1, subsample=b.Subsample(2)), noisy, seed=1)
    rgba8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    tiny_in, tiny_out = torch.ones(4, dtype=torch.float32, device="cuda"), torch.empty(4, dtype=torch.uint8, device="cuda")
    handle = C.c_void_p(lib.bt_resample_new())
    model_bytes = 16 * w * h + 32 * W * h + 16 * W * H

    def preview():
        assert preview_lib.bt_preview_device(noisy.data.data_ptr(), rgba8.data_ptr(), w, h, noisy.samples, 3, stream) == 0

    def launch():
        api._check(api.lib.bt_preview_device(tiny_in.data_ptr(), tiny_out.data_ptr(), 1, 1, 1, 3, stream))

    for rep in range(3):                                   # the spread of the runs: everything three times over
        us_preview, us_launch = timed(preview), timed(launch)
        for name in args.filters.split(","):
            p = b.ResampleParams(filter=name)._c()

            def resample():
                assert lib.bt_resample_device(handle, noisy.data.data_ptr(), noisy.samples, w, h, out.data_ptr(), W, H, C.byref(p), stream) == 0
            us = timed(resample)
            taps = [lib.bt_debug_resample_weights(handle, a, None, None, None, None) for a in (0, 1)]
            model = model_bytes / (20.0 * w * h) * us_preview + us_launch
            row = dict(source=[w, h], shown=[W, H], filter=name, taps=taps, run=rep, reps=args.reps, us_preview_of_source=round(us_preview, 2),
                       us_launch_1x1=round(us_launch, 2), us_per_call=round(us, 2), model_us=round(model, 2), over_model_us=round(us - model, 2),
                       ratio_to_model=round(us / model, 3), bytes=model_bytes)
            rows.append(row)
            print(json.dumps(row), flush=True)
    lib.bt_resample_free(handle)
    sc = None                                              # freed here, not at interpreter shutdown
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), preview_lib=os.path.basename(os.path.dirname(args.preview_lib)) or "this build",
                       lib=os.path.basename(args.lib) or "this build", rows=rows), f, indent=1)
