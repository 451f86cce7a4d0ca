"""The headless CLI's resample flags (EXTENSION): what is refused before anything is rendered (no GPU), and on the
GPU the screenshot against `Display().present(Resample().apply(Glare().apply(...)))` of the same render, --hdr holding the
resampled mean, the `resample` object of --stats-json, the same under --temporal, and the outputs without the flag."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_cli_io import read_png
from test_pfm import read_pfm

CLI = os.path.join(ROOT, "bendy_tracer_amd", "bendy-tracer-hip")


def _cli(*extra):
    return subprocess.run([CLI, "--width", "16", "--height", "16", "--samples", "1", *extra], capture_output=True, text=True,
                          timeout=60)


def test_cli_refuses_resample_combinations():
    r = _cli("--output", "albedo", "--resample", "8x8")
    assert r.returncode != 0 and "--resample needs --output full" in r.stderr
    r = _cli("--output", "normal", "--resample", "8x8", "--resample-filter", "box")
    assert r.returncode != 0 and "--resample needs --output full" in r.stderr
    r = _cli("--output", "full", "--shard", "0,2", "--resample", "8x8")
    assert r.returncode != 0 and "--resample" in r.stderr and "--shard" in r.stderr
    r = _cli("--output", "full", "--resample-filter", "tent")
    assert r.returncode != 0 and "--resample-filter needs --resample" in r.stderr
    for bad in ("", "x", "8", "8x", "x8", "0x8", "8x0", "-8x8", "8x-8", "8x8x8", "8.5x8", "8 x 8", "nanxinf"):
        r = _cli("--output", "full", "--resample=" + bad)
        assert r.returncode != 0 and "--resample expects WxH" in r.stderr, bad
    for bad in ("", "cubic", "Lanczos3", "lanczos", "3"):
        r = _cli("--output", "full", "--resample", "8x8", "--resample-filter=" + bad)
        assert r.returncode != 0 and "--resample-filter expects box, tent, mitchell or lanczos3" in r.stderr, bad
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--resample WxH" in r.stderr and "--resample-filter box|tent|mitchell|lanczos3" in r.stderr


@pytest.mark.gpu
def test_cli_resample_screenshot_hdr_and_stats(bendy, tmp_path):
    import torch
    w, h, spp, n = 64, 36, 2, 2
    shot, stats_p, hdr = tmp_path / "g.png", tmp_path / "s.json", tmp_path / "g.pfm"
    cmd = [CLI, "--width", str(w), "--height", str(h), "--output", "full", "--scene", scene_path("scene"), "--samples", str(spp * n * n),
           "--subsample", str(n), "--samples-per-call", str(spp), "--stats-json", str(stats_p), "--screenshot", str(shot), "--quiet"]
    r = subprocess.run(cmd + ["--resample", "90x70", "--glare", "0.1", "--tonemap", "aces", "--exposure", "auto", "--hdr", str(hdr)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    buf = bendy.Buffer.new(w, h)
    bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4)).render(
        sc, cam, bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n)), buf, seed=0x5EED)
    torch.cuda.synchronize()
    gl, rs, d = bendy.Glare(), bendy.Resample(), bendy.Display()
    resampled = rs.apply(gl.apply(buf, strength=0.1), 90, 70)
    png = read_png(shot)
    assert png.shape == (70, 90, 4) and np.array_equal(png, d.present(resampled, tonemap="aces"))       # pixel for pixel
    doc = json.load(open(stats_p))
    assert doc["resample"] == {"width": 90, "height": 70, "filter": "mitchell", "taps_x": rs.weights(0)[1], "taps_y": rs.weights(1)[1]}
    assert "display" in doc and "glare" in doc and (doc["width"], doc["height"]) == (w, h)
    magic, scale, rows = read_pfm(hdr)                                             # --hdr holds the 90 x 70 mean
    assert (magic, scale) == (b"PF", b"-1.0") and rows.shape == (70, 90, 3)
    assert np.array_equal(rows[::-1], resampled.numpy()[..., :3])
    # a thumbnail without the other stages: the plain preview of the resampled frame
    r = subprocess.run(cmd + ["--resample", "16x9", "--resample-filter", "lanczos3", "--hdr", str(hdr)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    small = rs.apply(buf, 16, 9, filter="lanczos3")
    assert np.array_equal(read_png(shot), small.preview())
    assert np.array_equal(read_pfm(hdr)[2][::-1], small.numpy()[..., :3])
    doc = json.load(open(stats_p))
    assert doc["resample"] == {"width": 16, "height": 9, "filter": "lanczos3", "taps_x": 24, "taps_y": 24} and "display" not in doc
    # a ratio beyond 128 taps fails with the library's message
    r = subprocess.run(cmd + ["--resample", "2x36", "--resample-filter", "lanczos3"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "the x axis" in r.stderr and "taps" in r.stderr
    # without the flag: the plain preview, the mean in --hdr, and no such object
    assert subprocess.run(cmd + ["--hdr", str(hdr)], capture_output=True, text=True, timeout=300).returncode == 0
    assert np.array_equal(read_png(shot), buf.preview()) and "resample" not in json.load(open(stats_p))
    assert np.array_equal(read_pfm(hdr)[2][::-1], buf.numpy()[..., :3] * (np.float32(1.0) / np.float32(buf.samples)))


@pytest.mark.gpu
def test_cli_resample_under_temporal(bendy, tmp_path):
    """Under --temporal every displayed frame's accumulated mean is glared, resampled, then shown: the exposure adapts on the
    resampled frames."""
    import torch
    w, h, spp, n, frames, step = 64, 36, 2, 2, 2, (0.04, 0.015, -0.02)
    shot, hdr = tmp_path / "t.png", tmp_path / "t.pfm"
    cmd = [CLI, "--width", str(w), "--height", str(h), "--output", "full", "--scene", scene_path("scene"), "--samples", str(spp),
           "--subsample", str(n), "--temporal", "--frames", str(frames), "--camera-step", ",".join(str(v) for v in step),
           "--screenshot", str(shot), "--quiet", "--glare", "0.2", "--glare-levels", "3", "--tonemap", "aces", "--exposure-adapt", "0.5",
           "--resample", "90x70", "--hdr", str(hdr)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    cfg = bendy.Config(chunks_x=8, chunks_y=4)
    tr, rc = bendy.Tracer.with_config(cfg), bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n))
    t, gl, rs, d = bendy.Temporal(w, h), bendy.Glare(strength=0.2, levels=3), bendy.Resample(), bendy.Display(adapt=0.5)
    view = sc.camera_view(cam, cfg, rc, w, h)
    for f in range(frames):
        if f > 0:
            for k in range(3):
                view.to_world[9 + k] = float(np.float32(view.to_world[9 + k]) + np.float32(step[k]))
            sc.set_camera_pose(cam, view.matrix())
        bufs = [bendy.Buffer.new(w, h) for _ in range(4)]
        tr.render_guided(sc, cam, rc, *bufs, seed=0x5EED, sample_base=f * spp)
        resampled = rs.apply(gl.apply(t.accumulate(view, bufs[0], bufs[2], bufs[3])), 90, 70)
        shown = d.present(resampled)
    torch.cuda.synchronize()
    assert np.array_equal(read_png(shot), shown)
    assert np.array_equal(read_pfm(hdr)[2][::-1], resampled.numpy()[..., :3])
