"""HIP-event times of the upscale stage (extension) at 768x512 -> 1536x1024 and 960x540 -> 1920x1080 (developer tool).

Usage: python tools/time_upscale.py [--reps 50] [--json PATH] [--preview-lib PATH/libbendy_hip.so] [--upscale-lib PATH/lib.so]
Renders scene.json with its guides at the small size (1 x Subpixel(2)) and the three guides at the shown size, then times `reps`
back-to-back calls between two events: bt_preview_device on the shown frame (the yardstick; with --preview-lib the one of
another build of the library, e.g. the parent commit's), bt_resample_device with the tent (what the parent can show) and
bt_upscale_device with all three guide pairs and with none.  With --upscale-lib the stage is another build's, e.g.
`make variant SRC=bt_upscale KFLAGS=-DBT_UPSCALE_LDS=0`.

The model a call is held against.  Per output pixel the main kernel reads three hi guides (48 B) and writes 16 B; per lo texel
the prepare kernel reads 64 B and writes 48 B, which the main kernel reads again once (the footprints overlap in cache or LDS).
The preview moves 20 B per pixel, so    model = (64 + 160 * (w h) / (W H)) / 20 * preview."""
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
ap.add_argument("--upscale-lib", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_upscale.py needs a GPU"

preview_lib = stage_lib = api.lib
if args.preview_lib:
    preview_lib = C.CDLL(args.preview_lib)
    preview_lib.bt_preview_device.argtypes = api.lib.bt_preview_device.argtypes
if args.upscale_lib:
    stage_lib = C.CDLL(args.upscale_lib)
    stage_lib.bt_upscale_new.restype = C.c_void_p
    for name in ("bt_upscale_new", "bt_upscale_free", "bt_upscale_device"):
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
for w, h, W, H in ((768, 512, 1536, 1024), (960, 540, 1920, 1080)):
    sc = b.Scene.load(os.path.join(HERE, "..", "scenes", "scene.json.gz"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, W / H)
    rc = b.RenderConfig(samples=1, subsample=b.Subsample(2))
    lo = [b.Buffer.new(w, h) for _ in range(4)]
    b.Tracer.new().render_guided(sc, cam, rc, *lo, seed=1)
    hi = []
    for output in (b.Output.Albedo, b.Output.Normal, b.Output.Depth):
        g = b.Buffer.new(W, H)
        b.Tracer.with_config(b.Config(chunks_x=8, chunks_y=4, output=output)).render(sc, cam, rc, g, seed=2)
        hi.append(g)
    rgba8 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    out = b.Buffer.new(W, H)
    handle = C.c_void_p(stage_lib.bt_upscale_new())
    resample = b.Resample(filter="tent")
    gl, gh, none = api._device_guides(lo[1:]), api._device_guides(hi), api._CUpscaleGuides()

    def preview():
        assert preview_lib.bt_preview_device(hi[0].data.data_ptr(), rgba8.data_ptr(), W, H, 1, 3, stream) == 0

    def tent():
        resample.apply(lo[0], W, H, out=out)

    def guided():
        assert stage_lib.bt_upscale_device(handle, lo[0].data.data_ptr(), lo[0].samples, w, h, C.byref(gl), C.byref(gh), out.data.data_ptr(), W, H,
                                           None, stream) == 0

    def unguided():
        assert stage_lib.bt_upscale_device(handle, lo[0].data.data_ptr(), lo[0].samples, w, h, C.byref(none), C.byref(none), out.data.data_ptr(),
                                           W, H, None, stream) == 0

    for rep in range(3):                                   # the spread of the runs: everything three times over
        us_preview = timed(preview)
        model = (64.0 + 160.0 * (w * h) / (W * H)) / 20.0 * us_preview
        for name, call in (("tent", tent), ("guided", guided), ("no_guides", unguided)):
            us = timed(call)
            row = dict(lo=[w, h], hi=[W, H], run=rep, reps=args.reps, call=name, us_preview=round(us_preview, 2), us_per_call=round(us, 2),
                       model_us=round(model, 2), ratio_to_preview=round(us / us_preview, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    stage_lib.bt_upscale_free(handle)
    sc = None                                              # freed here, not at interpreter shutdown
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), preview_lib=os.path.basename(os.path.dirname(args.preview_lib)) or "this build",
                       upscale_lib=os.path.basename(args.upscale_lib) or "this build", rows=rows), f, indent=1)
