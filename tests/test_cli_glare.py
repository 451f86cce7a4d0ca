"""The headless CLI's glare flags (EXTENSION): what is refused before anything is rendered (no GPU), and on the
GPU the screenshot against `Display().present(Glare().apply(...))` of the same render, --hdr holding the glared mean, the
`glare` object of --stats-json, and the outputs without the flag."""
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


def test_cli_refuses_glare_combinations():
    r = _cli("--output", "albedo", "--glare", "0.1")
    assert r.returncode != 0 and "--glare needs --output full" in r.stderr
    r = _cli("--output", "normal", "--glare", "0.1", "--glare-levels", "3")
    assert r.returncode != 0 and "--glare needs --output full" in r.stderr
    r = _cli("--output", "full", "--shard", "0,2", "--glare", "0.1")
    assert r.returncode != 0 and "--glare" in r.stderr and "--shard" in r.stderr
    for flags in (("--glare-levels", "3"), ("--glare-spread", "2")):
        r = _cli("--output", "full", *flags)
        assert r.returncode != 0 and "need --glare" in r.stderr, flags
    for bad in ("", "x", "nan", "inf", "-0.1", "1.5", "0.1x"):
        r = _cli("--output", "full", "--glare=" + bad)
        assert r.returncode != 0 and "--glare expects a strength in [0, 1]" in r.stderr, bad
    for bad in ("", "x", "-1", "17", "2.5"):
        r = _cli("--output", "full", "--glare", "0.1", "--glare-levels=" + bad)
        assert r.returncode != 0 and "--glare-levels expects a count in 0 .. 16" in r.stderr, bad
    for bad in ("", "x", "0", "-1", "nan", "inf", "16.5"):
        r = _cli("--output", "full", "--glare", "0.1", "--glare-spread=" + bad)
        assert r.returncode != 0 and "--glare-spread expects a value in (0, 16]" in r.stderr, bad
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--glare STRENGTH" in r.stderr and "--glare-levels" in r.stderr and "--glare-spread" in r.stderr


@pytest.mark.gpu
def test_cli_glare_screenshot_hdr_and_stats(bendy, tmp_path):
    import torch
    w, h, spp, n = 64, 36, 2, 2
    shot, stats_p, hdr = tmp_path / "g.png", tmp_path / "s.json", tmp_path / "g.pfm"
    cmd = [CLI, "--width", str(w), "--height", str(h), "--output", "full", "--scene", scene_path("scene"), "--samples", str(spp * n * n),
           "--subsample", str(n), "--samples-per-call", str(spp), "--stats-json", str(stats_p), "--screenshot", str(shot), "--quiet"]
    r = subprocess.run(cmd + ["--glare", "0.1", "--tonemap", "aces", "--exposure", "auto", "--hdr", str(hdr)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    buf = bendy.Buffer.new(w, h)
    bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4)).render(
        sc, cam, bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n)), buf, seed=0x5EED)
    torch.cuda.synchronize()
    gl, d = bendy.Glare(), bendy.Display()
    glared = gl.apply(buf, strength=0.1)
    assert np.array_equal(read_png(shot), d.present(glared, tonemap="aces"))       # pixel for pixel
    doc = json.load(open(stats_p))
    assert np.float32(doc["glare"].pop("strength")) == np.float32(0.1)
    assert doc["glare"] == {"levels": 6, "spread": 1.0} and "display" in doc
    magic, scale, rows = read_pfm(hdr)                                             # --hdr holds the glared mean
    assert (magic, scale) == (b"PF", b"-1.0")
    assert np.array_equal(rows[::-1], glared.numpy()[..., :3])
    # the other two flags, without the display stage: the plain preview of the glared mean; levels are the effective ones
    r = subprocess.run(cmd + ["--glare", "0.5", "--glare-levels", "16", "--glare-spread", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_png(shot), gl.apply(buf, strength=0.5, levels=16, spread=2.0).preview())
    doc = json.load(open(stats_p))
    assert doc["glare"] == {"strength": 0.5, "levels": 6, "spread": 2.0} and "display" not in doc
    # without the flag: the plain preview, the mean in --hdr, and no such object
    assert subprocess.run(cmd + ["--hdr", str(hdr)], capture_output=True, text=True, timeout=300).returncode == 0
    assert np.array_equal(read_png(shot), buf.preview()) and "glare" not in json.load(open(stats_p))
    assert np.array_equal(read_pfm(hdr)[2][::-1], buf.numpy()[..., :3] * (np.float32(1.0) / np.float32(buf.samples)))


@pytest.mark.gpu
def test_cli_glare_under_temporal(bendy, tmp_path):
    """Under --temporal the last displayed frame's accumulated mean is glared, then shown."""
    import torch
    w, h, spp, n, frames, step = 64, 36, 2, 2, 2, (0.04, 0.015, -0.02)
    shot = tmp_path / "t.png"
    cmd = [CLI, "--width", str(w), "--height", str(h), "--output", "full", "--scene", scene_path("scene"), "--samples", str(spp),
           "--subsample", str(n), "--temporal", "--frames", str(frames), "--camera-step", ",".join(str(v) for v in step),
           "--screenshot", str(shot), "--quiet", "--glare", "0.2", "--glare-levels", "3", "--tonemap", "aces", "--exposure-adapt", "0.5"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    cfg = bendy.Config(chunks_x=8, chunks_y=4)
    tr, rc = bendy.Tracer.with_config(cfg), bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n))
    t, gl, d = bendy.Temporal(w, h), bendy.Glare(strength=0.2, levels=3), bendy.Display(adapt=0.5)
    view = sc.camera_view(cam, cfg, rc, w, h)
    for f in range(frames):
        if f > 0:
            for k in range(3):
                view.to_world[9 + k] = float(np.float32(view.to_world[9 + k]) + np.float32(step[k]))
            sc.set_camera_pose(cam, view.matrix())
        bufs = [bendy.Buffer.new(w, h) for _ in range(4)]
        tr.render_guided(sc, cam, rc, *bufs, seed=0x5EED, sample_base=f * spp)
        shown = d.present(gl.apply(t.accumulate(view, bufs[0], bufs[2], bufs[3])))
    torch.cuda.synchronize()
    assert np.array_equal(read_png(shot), shown)
