"""HIP-event times of the despeckle stage (extension) at 768x512 and 1920x1080 (developer tool).

Usage: python tools/time_despeckle.py [--reps 50] [--json PATH] [--preview-lib PATH/libbendy_hip.so] [--despeckle-lib PATH/lib.so]
Renders scene.json (1 x Subpixel(2)) on the GPU for a noisy frame, then times `reps` back-to-back calls between two events:
bt_preview_device (the yardstick; with --preview-lib the one of another build of the library, e.g. the parent commit's) and
bt_despeckle_device at both radii, with rank 2 (the two-largest selection), rank 4 (the four-largest) and the radius's largest rank (the counting selection).
With --despeckle-lib the stage is another build's, e.g. `make variant SRC=bt_despeckle KFLAGS=-DBT_DESPECKLE_LDS=0`.

The model a call is held against.  The stage streams 16 B in and 16 B out per pixel (the halo re-reads are cached); the preview
moves 20 B per pixel, so    model = (32 / 20) * preview."""
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
ap.add_argument("--despeckle-lib", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_despeckle.py needs a GPU"

preview_lib = stage_lib = api.lib
if args.preview_lib:
    preview_lib = C.CDLL(args.preview_lib)
    preview_lib.bt_preview_device.argtypes = api.lib.bt_preview_device.argtypes
if args.despeckle_lib:
    stage_lib = C.CDLL(args.despeckle_lib)
    stage_lib.bt_despeckle_new.restype = C.c_void_p
    for name in ("bt_despeckle_new", "bt_despeckle_free", "bt_despeckle_device"):
        getattr(stage_lib, name).argtypes = getattr(api.lib, name).argtypes
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
for w, h in ((768, 512), (1920, 1080)):
    sc = b.Scene.load(os.path.join(HERE, "..", "scenes", "scene.json.gz"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    noisy = b.Buffer.new(w, h)
    b.Tracer.new().render(sc, cam, b.RenderConfig(samples=1, subsample=b.Subsample(2)), noisy, seed=1)
    rgba8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    handle = C.c_void_p(stage_lib.bt_despeckle_new())

    def preview():
        assert preview_lib.bt_preview_device(noisy.data.data_ptr(), rgba8.data_ptr(), w, h, noisy.samples, 3, stream) == 0

    for rep in range(3):                                   # the spread of the runs: everything three times over
        us_preview = timed(preview)
        for radius, rank in ((1, 2), (1, 4), (1, 8), (2, 2), (2, 4), (2, 24)):
            p = b.DespeckleParams(radius=radius, rank=rank)._c()

            def despeckle():
                assert stage_lib.bt_despeckle_device(handle, noisy.data.data_ptr(), noisy.samples, out.data_ptr(), w, h, C.byref(p), stream) == 0
            us = timed(despeckle)
            model = 32.0 / 20.0 * us_preview
            row = dict(width=w, height=h, run=rep, reps=args.reps, radius=radius, rank=rank, us_preview=round(us_preview, 2),
                       us_per_call=round(us, 2), model_us=round(model, 2), over_model_us=round(us - model, 2),
                       ratio_to_preview=round(us / us_preview, 3), bytes=w * h * 32)
            rows.append(row)
            print(json.dumps(row), flush=True)
    stage_lib.bt_despeckle_free(handle)
    sc = None                                              # freed here, not at interpreter shutdown
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), preview_lib=os.path.basename(os.path.dirname(args.preview_lib)) or "this build",
                       despeckle_lib=os.path.basename(args.despeckle_lib) or "this build", rows=rows), f, indent=1)
