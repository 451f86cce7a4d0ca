"""HIP-event times of the display stage (extension) at 768x512 and 1920x1080 (developer tool).

Usage: python tools/time_display.py [--reps 50] [--json PATH] [--preview-lib PATH/libbendy_hip.so]
Renders scene.json (1 x Subpixel(2)) on the GPU for a noisy frame and fills a second frame with one value (every pixel in
one luminance bin: the worst case for the meter's LDS adds), then times `reps` back-to-back calls between two events:
bt_preview_device (the yardstick; with --preview-lib the one of another build of the library, e.g. the parent commit's),
a 1x1 bt_preview_device (what a launch costs when the kernel has nothing to do) and bt_display_device for the three operators,
metered and manual.  Bytes a call moves: the preview and a manual display call read 16 and write 4 B per pixel; a metered call
reads the 16 B per pixel once more (the meter; the second read is served by the Infinity Cache) and adds two launches.

The meter's A/B build (lanes of a wave that hit the same bin elect one to add their count):
    make -C bendy_tracer_amd/csrc B=build_merge LIB=../libbendy_hip_merge.so FLAGS="<the Makefile's FLAGS> -DBT_METER_MERGE=1" ../libbendy_hip_merge.so
    tools/run_with_lib.sh libbendy_hip_merge.so python tools/time_display.py"""
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
args = ap.parse_args()
assert torch.cuda.is_available(), "time_display.py needs a GPU"

preview_lib = api.lib
if args.preview_lib:
    preview_lib = C.CDLL(args.preview_lib)
    preview_lib.bt_preview_device.argtypes = api.lib.bt_preview_device.argtypes
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
    const = b.Buffer.new(w, h)
    const.data[..., :3] = 0.5
    const.samples = 1
    out = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    tiny_in, tiny_out = torch.ones(4, dtype=torch.float32, device="cuda"), torch.empty(4, dtype=torch.uint8, device="cuda")
    d = b.Display()
    for frame_name, buf in (("rendered", noisy), ("constant", const)):
        def preview():
            assert preview_lib.bt_preview_device(buf.data.data_ptr(), out.data_ptr(), w, h, buf.samples, 3, stream) == 0
        us_preview = timed(preview)
        us_launch = timed(lambda: api._check(api.lib.bt_preview_device(tiny_in.data_ptr(), tiny_out.data_ptr(), 1, 1, 1, 3, stream)))
        base = dict(width=w, height=h, frame=frame_name, reps=args.reps, us_preview=round(us_preview, 2), us_launch_1x1=round(us_launch, 2))
        for op in ("clip", "reinhard", "aces"):
            for mode in ("auto", "manual"):
                p = b.DisplayParams(tonemap=op, auto_exposure=int(mode == "auto"), ev=0.5)._c()

                def display():
                    api._check(api.lib.bt_display_device(d._h, buf.data.data_ptr(), buf.samples, out.data_ptr(), w, h, 3, C.byref(p), stream))
                us = timed(display)
                row = dict(base, operator=op, exposure=mode, us_per_call=round(us, 2), ratio_to_preview=round(us / us_preview, 3),
                           bound_us=round(1.8 * us_preview + 2 * us_launch, 2) if mode == "auto" else None,
                           bytes=w * h * (36 if mode == "auto" else 20), ev=round(d.exposure()[0], 5))
                rows.append(row)
                print(json.dumps(row), flush=True)
    d.close()
    sc = None                                              # freed here, not at interpreter shutdown
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), preview_lib=os.path.basename(os.path.dirname(args.preview_lib)) or "this build",
                       rows=rows), f, indent=1)
