"""The headless CLI's --temporal flags (EXTENSION): what is refused before anything is rendered (no GPU), and on
the GPU a three-frame run under a moving camera whose screenshot is the Python sequence's `out.preview()`."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_cli_io import read_png

CLI = os.path.join(ROOT, "bendy_tracer_amd", "bendy-tracer-hip")


def _cli(*extra):
    return subprocess.run([CLI, "--width", "16", "--height", "16", "--samples", "1", *extra], capture_output=True, text=True,
                          timeout=60)


def test_cli_refuses_temporal_combinations():
    r = _cli("--output", "albedo", "--temporal")
    assert r.returncode != 0 and "--temporal needs --output full" in r.stderr
    r = _cli("--output", "full", "--temporal", "--lens", "0,0,0,0.1,0.1,2")
    assert r.returncode != 0 and "--temporal" in r.stderr and "--lens" in r.stderr
    r = _cli("--output", "full", "--temporal", "--shard", "0,2")
    assert r.returncode != 0 and "--temporal" in r.stderr and "--shard" in r.stderr
    r = _cli("--output", "full", "--temporal", "--adaptive", "0.05")
    assert r.returncode != 0 and "--temporal" in r.stderr and "--adaptive" in r.stderr
    r = _cli("--output", "full", "--temporal", "--denoise-inline")
    assert r.returncode != 0 and "--temporal" in r.stderr and "--denoise-inline" in r.stderr
    for flag in (("--frames", "3"), ("--camera-step", "0.1,0,0")):
        r = _cli("--output", "full", *flag)
        assert r.returncode != 0 and "need --temporal" in r.stderr
    for bad in ("0", "-2", "x", "", "3x"):
        r = _cli("--output", "full", "--temporal", "--frames=" + bad)
        assert r.returncode != 0 and "--frames expects a count >= 1" in r.stderr, bad
    for bad in ("1,2", "1,2,3,4", "a,b,c", "nan,0,0", "inf,0,0", ""):
        r = _cli("--output", "full", "--temporal", "--camera-step=" + bad)
        assert r.returncode != 0 and "--camera-step expects X,Y,Z" in r.stderr, bad
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--temporal" in r.stderr and "--camera-step X,Y,Z" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("denoise", [False, True])
def test_cli_temporal_run(bendy, tmp_path, denoise):
    """N frames of --samples x subsample^2 rays into cleared buffers, sample indices continuing from frame to frame, the camera
    moved by --camera-step before every frame after the first; the screenshot is the last accumulate's out (or its denoised mean,
    filtered with the last frame's guides)."""
    import torch
    w, h, spp, n, frames, step = 64, 36, 2, 2, 3, (0.04, 0.015, -0.02)
    shot, stats_p = tmp_path / "t.png", tmp_path / "s.json"
    cmd = [CLI, "--width", str(w), "--height", str(h), "--output", "full", "--scene", scene_path("scene"), "--samples", str(spp),
           "--subsample", str(n), "--temporal", "--frames", str(frames), "--camera-step", ",".join(str(v) for v in step),
           "--stats-json", str(stats_p), "--screenshot", str(shot), "--quiet"]
    r = subprocess.run(cmd + (["--denoise"] if denoise else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    cfg = bendy.Config(chunks_x=8, chunks_y=4)
    tr, rc = bendy.Tracer.with_config(cfg), bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n))
    t = bendy.Temporal(w, h)
    view = sc.camera_view(cam, cfg, rc, w, h)
    for f in range(frames):
        if f > 0:
            for k in range(3):
                view.to_world[9 + k] = float(np.float32(view.to_world[9 + k]) + np.float32(step[k]))
            sc.set_camera_pose(cam, view.matrix())
        bufs = [bendy.Buffer.new(w, h) for _ in range(4)]
        tr.render_guided(sc, cam, rc, *bufs, seed=0x5EED, sample_base=f * spp)
        out = t.accumulate(view, bufs[0], bufs[2], bufs[3])
    if denoise:
        out = bendy.denoise(out, *bufs[1:])
    torch.cuda.synchronize()
    assert np.array_equal(read_png(shot), out.preview())
    doc, hist = json.load(open(stats_p)), t.history()[..., 3]
    assert doc["temporal"]["frames"] == frames and len(doc["calls"]) == frames
    assert doc["temporal"]["history_mean"] == pytest.approx(float(hist.astype(np.float64).mean()), abs=1e-3)
    assert doc["temporal"]["history_min"] == pytest.approx(float(hist.min()), abs=1e-3)
    assert spp * n * n <= hist.min() and hist.max() <= frames * spp * n * n + 1e-3 and hist.mean() > 2 * spp * n * n
    if not denoise:                                                            # without the flag the file has no such object
        plain = [c for c in cmd if c not in ("--temporal", "--frames", str(frames), "--camera-step", ",".join(str(v) for v in step))]
        assert subprocess.run(plain, capture_output=True, text=True, timeout=300).returncode == 0
        assert "temporal" not in json.load(open(stats_p))
