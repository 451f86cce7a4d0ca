"""HIP-event times of the compare stage (extension) at 768x512 and 1920x1080 (developer tool).

Usage: python tools/time_compare.py [--reps 50] [--json PATH] [--preview-lib PATH/libbendy_hip.so]
Uploads two frames (a log-normal reference and the same with 10 % noise), then times `reps` back-to-back calls between two events,
three times over: bt_preview_device on the same frame (the yardstick; with --preview-lib the one of another build of the library,
e.g. the parent commit's, loaded next to this one), bt_compare_device (the point and the SSIM kernel), and, each with its host
round trips, Compare.tail and Compare.map.

The streaming model a call is held against, in bytes per pixel: the point kernel reads 32 and writes 20; the SSIM kernel reads
16 * (26 / 16)^2 = 42 through the cache and writes 8.  Together 102 B against the preview's 20 B:  model = 5.1 * preview.  The
other bound is arithmetic: four float64 divisions per pixel and 2 * 55 float64 multiply-adds of the two blurs."""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bendy_tracer_amd as b  # noqa: E402
from bendy_tracer_amd import api  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--json", default="")
ap.add_argument("--preview-lib", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_compare.py needs a GPU"

preview_lib = api.lib
if args.preview_lib:
    preview_lib = C.CDLL(args.preview_lib)
    preview_lib.bt_preview_device.argtypes = api.lib.bt_preview_device.argtypes
stream = torch.cuda.current_stream().cuda_stream


def timed(call, reps):
    for _ in range(6):
        call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3           # microseconds per call


def upload(frame):
    buf = b.Buffer.new(frame.shape[1], frame.shape[0])
    buf.data.copy_(torch.from_numpy(frame))
    buf.samples = 1
    return buf


rows = []
for w, h in ((768, 512), (1920, 1080)):
    rng = np.random.default_rng(w)
    y = np.ones((h, w, 4), dtype=np.float32)
    y[..., :3] = np.exp2(rng.uniform(-6.0, 6.0, size=(h, w, 3))).astype(np.float32)
    x = y.copy()
    x[..., :3] *= (1.0 + 0.1 * rng.standard_normal((h, w, 3))).astype(np.float32)
    test, ref = upload(x), upload(y)
    rgba8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    handle = b.Compare()
    cp = handle.params._c()

    def preview():
        assert preview_lib.bt_preview_device(ref.data.data_ptr(), rgba8.data_ptr(), w, h, 1, 3, stream) == 0

    def compare():
        assert api.lib.bt_compare_device(handle._h, test.data.data_ptr(), 1, ref.data.data_ptr(), 1, w, h, C.byref(cp), stream) == 0

    st = handle.measure(test, ref)
    for rep in range(3):                                   # the spread of the runs: everything three times over
        us_preview = timed(preview, args.reps)
        for name, call, reps in (("compare", compare, args.reps), ("tail", lambda: handle.tail(0.01), 10), ("map", lambda: handle.map(1.0, out=rgba8), args.reps)):
            us = timed(call, reps)
            row = dict(size=[w, h], run=rep, reps=reps, call=name, us_preview=round(us_preview, 2), us_per_call=round(us, 2),
                       model_us=round(5.1 * us_preview, 2) if name == "compare" else None, ratio_to_preview=round(us / us_preview, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps(dict(size=[w, h], rel_mse=st.rel_mse, ssim=st.ssim, tail_share=handle.tail(0.01)[0])), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), preview_lib=os.path.basename(os.path.dirname(args.preview_lib)) or "this build", rows=rows), f,
                  indent=1)
