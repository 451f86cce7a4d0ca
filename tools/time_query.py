"""HIP-event times of the ray query API (extension) (developer tool).

Usage: python tools/time_query.py [--reps 50] [--json PATH] [--other-lib PATH/libbendy_hip_NAME.so]
Times, each with a warm-up and `reps` back-to-back launches between two events, three windows over:
  - bt_query_rays_device at 2^21 recipe rays (the mix of tests/query_ref.py, restated here: half aimed at the scene's objects, a
    tenth along the axes, the rest isotropic, a fifth with a short clip) on scene.json.gz and cornell2.json.gz;
  - bt_view_rays_device at 1920 x 1080, and the 1080p pick-map pair (view rays, then the query of those rays).
With --other-lib the query windows alternate between this build and another build of the library (`make variant`), which is how
two forms of the kernel are compared in one call.

What a time is held against: a query moves 96 B per ray (32 B in, 64 B out; the scalar loads of the rows are shared by a wave),
the view-ray kernel 32 B.  The least time is the larger of bytes / (8.0 TB/s, the HBM peak of the MI355X) and VALU issue: the
SIMD cycles a wave64 spends issuing the VALU instructions on its path through bt_query.hip's ISA, each instruction at the price
profiles/valu_issue_costs.json measured for its class (2.25 cycles plain, 4.15 with an SGPR operand, 4.57 for a compare or
v_div_scale, 8.13 for v_rcp / v_sqrt), over 1 024 SIMDs at 2.4 GHz.  Per row: sphere 166 cycles (51 instructions), rect 274 (83),
axis-aligned rect 159 (47), axis-aligned with an axis normal 123 (36), local-axes rect 176 (53); 485 around the loop (208, the hit
record's 81 included).  The view-ray kernel: 473 cycles, the 210 instructions of its path with the small-argument reduction in all
four sinf / cosf at the plain price -- a lower estimate.  The report names the larger floor as the bound."""
import argparse
import ctypes as C
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bendy_tracer_amd as b  # noqa: E402
from bendy_tracer_amd import api  # noqa: E402

HBM_PEAK = 8.0e12                       # bytes / s
SIMD_CYCLES = 1024 * 2.4e9              # SIMD cycles / s of the whole chip
ROW_CYCLES = (166, 274, 159, 123, 176)  # by BT_PRIM_* shape: sphere, rect, rect AA, rect AAN, rect LA
AROUND_CYCLES, VIEW_CYCLES = 485, 473

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rays", type=int, default=1 << 21)
ap.add_argument("--json", default="")
ap.add_argument("--other-lib", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_query.py needs a GPU"
assert args.reps >= 50, "at least 50 launches per window"
stream = torch.cuda.current_stream().cuda_stream


def recipe_rays(seed, aims, n):
    rng = np.random.default_rng(seed)
    o = rng.uniform([-6.0, -1.9, -8.0], [6.0, 6.0, 10.0], (n, 3)).astype(np.float32)
    n_aim, n_axis = n // 2, n // 10
    d = np.zeros((n, 3), np.float32)
    d[:n_aim] = (aims[rng.integers(len(aims), size=n_aim)] + rng.normal(0.0, 0.3, (n_aim, 3)) - o[:n_aim]).astype(np.float32)
    d[np.arange(n_aim, n_aim + n_axis), rng.integers(3, size=n_axis)] = rng.choice([-1.0, 1.0], n_axis)
    d[n_aim + n_axis:] = rng.normal(0.0, 1.0, (n - n_aim - n_axis, 3)).astype(np.float32)
    d = (d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]).astype(np.float32)
    rays = np.empty((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7] = o, d, 0.01, 1000.0
    k = n - n // 5
    rays[k:, 3] = rng.uniform(0.0, 6.0, n - k).astype(np.float32)
    rays[k:, 7] = rays[k:, 3] + rng.uniform(0.0, 6.0, n - k).astype(np.float32)
    return rays


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
    return t0.elapsed_time(t1) / reps                    # milliseconds per call


def other_library(path):
    L = C.CDLL(path)
    L.bt_scene_load.restype = C.c_void_p
    L.bt_scene_load.argtypes = [C.c_char_p]
    L.bt_query_rays_device.argtypes = api.lib.bt_query_rays_device.argtypes
    return L


def report(case, build, run, n, ms, bytes_per_ray, wave_cycles):
    t_bytes, t_valu = n * bytes_per_ray / HBM_PEAK * 1e3, (n + 63) // 64 * wave_cycles / SIMD_CYCLES * 1e3
    row = dict(case=case, build=build, run=run, rays=n, ms=round(ms, 4), rays_per_s=round(n / ms * 1e3), bytes_per_s=round(n * bytes_per_ray / ms * 1e3),
               share_of_hbm_peak=round(n * bytes_per_ray / ms * 1e3 / HBM_PEAK, 4), floor_ms_bytes=round(t_bytes, 4), floor_ms_valu=round(t_valu, 4),
               bound="bytes" if t_bytes >= t_valu else "VALU issue", share_of_floor=round(max(t_bytes, t_valu) / ms, 4))
    print(json.dumps(row), flush=True)
    return row


rows = []
other = other_library(args.other_lib) if args.other_lib else None
other_name = os.path.basename(args.other_lib)
for name in ("scene", "cornell2"):
    path = os.path.join(ROOT, "scenes", name + ".json.gz")
    doc = json.load(gzip.open(path, "rt"))
    aims = np.asarray([o["transform"]["transform_world"][9:12] for o in doc["objects"]["collection"].values()
                       if o["inner"] != "Empty" and "Camera" not in o["inner"]], np.float64)
    sc = b.Scene.load(path)
    kinds = sc.export_prims().view(np.int32)[:, 0] & 7
    valu = sum(ROW_CYCLES[k] for k in kinds) + AROUND_CYCLES
    rays = torch.from_numpy(recipe_rays(1, aims, args.rays)).cuda()
    hits = torch.empty((args.rays, 64), dtype=torch.uint8, device="cuda")
    builds = [("this build", lambda: sc.query(rays, out=hits))]
    if other:
        h_other = C.c_void_p(other.bt_scene_load(path.encode()))
        hits_other = torch.empty_like(hits)

        def query_other():
            assert other.bt_query_rays_device(h_other, rays.data_ptr(), args.rays, hits_other.data_ptr(), stream) == args.rays
        builds.append((other_name, query_other))
    for run in range(3):                                  # alternating: the spread of the runs is in the rows
        for build, call in builds:
            rows.append(report(f"query {name} ({len(kinds)} rows)", build, run, args.rays, timed(call, args.reps), 96, valu))
    if other:
        torch.cuda.synchronize()
        assert torch.equal(hits, hits_other), "the two builds disagree"
    print(json.dumps(dict(scene=name, hit_share=round(float((b.hits_numpy(hits)["face"] >= 0).mean()), 4))), flush=True)

w, h = 1920, 1080
sc = b.Scene.load(os.path.join(ROOT, "scenes", "scene.json.gz"))
cam = sc.find_by_tag("camera")
sc.set_camera_aspect(cam, w / h)
view = sc.camera_view(cam, b.Config(), b.RenderConfig(samples=1), w, h)
rays = torch.empty((w * h, 8), dtype=torch.float32, device="cuda")
hits = torch.empty((w * h, 64), dtype=torch.uint8, device="cuda")
n_rows = sc.export_prims().shape[0]
for run in range(3):
    rows.append(report("view rays 1920x1080", "this build", run, w * h, timed(lambda: b.view_rays(view, 0, 0, w, h, out=rays), args.reps), 32, VIEW_CYCLES))

    def pair():
        b.view_rays(view, 0, 0, w, h, out=rays)
        sc.query(rays, out=hits)
    rows.append(report("pick map 1920x1080 (view rays + query, scene)", "this build", run, w * h, timed(pair, args.reps), 128,
                       VIEW_CYCLES + n_rows * ROW_CYCLES[0] + AROUND_CYCLES))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), other_lib=other_name or None, rows=rows), f, indent=1)
sc = None                                                 # the handle goes before the interpreter takes the library away
