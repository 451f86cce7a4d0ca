"""The headless CLI's display flags (EXTENSION): what is refused before anything is rendered (no GPU), and on the
GPU the screenshot against `Display().present(...)` of the same render, the exposure adapting across --temporal frames, and
--hdr."""
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


def test_cli_refuses_display_combinations():
    for flags in (("--tonemap", "aces"), ("--exposure", "auto"), ("--exposure", "1.5"), ("--white", "2"), ("--exposure-key", "0.2"),
                  ("--exposure-adapt", "0.5")):
        r = _cli("--output", "albedo", *flags)
        assert r.returncode != 0 and "need --output full" in r.stderr, flags
        r = _cli("--output", "full", "--shard", "0,2", *flags)
        assert r.returncode != 0 and "--shard" in r.stderr, flags
    r = _cli("--output", "normal", "--hdr", "x.pfm")
    assert r.returncode != 0 and "--hdr needs --output full" in r.stderr
    r = _cli("--output", "full", "--shard", "0,2", "--hdr", "x.pfm")
    assert r.returncode != 0 and "--hdr" in r.stderr and "--shard" in r.stderr
    for bad in ("filmic", "", "ACES"):
        r = _cli("--output", "full", "--tonemap=" + bad)
        assert r.returncode != 0 and "--tonemap expects clip, reinhard or aces" in r.stderr, bad
    for bad in ("", "x", "nan", "inf", "1.5x", "Auto"):
        r = _cli("--output", "full", "--exposure=" + bad)
        assert r.returncode != 0 and "--exposure expects auto or a finite EV" in r.stderr, bad
    for flag, word in (("--exposure-key", "> 0"), ("--white", "> 0"), ("--exposure-adapt", "(0, 1]")):
        for bad in ("0", "-1", "x", "", "nan", "inf"):
            r = _cli("--output", "full", flag + "=" + bad)
            assert r.returncode != 0 and flag + " expects" in r.stderr and word in r.stderr, (flag, bad)
    r = _cli("--output", "full", "--exposure-adapt=1.5")
    assert r.returncode != 0 and "--exposure-adapt expects a value in (0, 1]" in r.stderr
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--tonemap clip|reinhard|aces" in r.stderr and "--exposure auto|EV" in r.stderr and "--hdr PATH.pfm" in r.stderr


def _render(bendy, w, h, spp, n):
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    cfg = bendy.Config(chunks_x=8, chunks_y=4)
    return sc, cam, cfg, bendy.Tracer.with_config(cfg), bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n))


@pytest.mark.gpu
def test_cli_display_screenshot_hdr_and_stats(bendy, tmp_path):
    import torch
    w, h, spp, n = 64, 36, 2, 2
    shot, stats_p, hdr = tmp_path / "d.png", tmp_path / "s.json", tmp_path / "d.pfm"
    cmd = [CLI, "--width", str(w), "--height", str(h), "--output", "full", "--scene", scene_path("scene"), "--samples", str(spp * n * n),
           "--subsample", str(n), "--samples-per-call", str(spp), "--stats-json", str(stats_p), "--screenshot", str(shot), "--quiet"]
    r = subprocess.run(cmd + ["--tonemap", "aces", "--exposure", "auto", "--hdr", str(hdr)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sc, cam, cfg, tr, rc = _render(bendy, w, h, spp, n)
    buf = bendy.Buffer.new(w, h)
    tr.render(sc, cam, rc, buf, seed=0x5EED)
    torch.cuda.synchronize()
    d = bendy.Display()
    assert np.array_equal(read_png(shot), d.present(buf, tonemap="aces"))          # pixel for pixel
    doc = json.load(open(stats_p))["display"]
    ev, mult = d.exposure()
    assert (np.float32(doc["ev"]), np.float32(doc["mult"])) == (np.float32(ev), np.float32(mult))
    assert (doc["under"], doc["over"], doc["operator"]) == (d.histogram()[1], d.histogram()[2], "aces")
    magic, scale, rows = read_pfm(hdr)                                             # --hdr writes the mean
    assert (magic, scale) == (b"PF", b"-1.0")
    assert np.array_equal(rows[::-1], buf.numpy()[..., :3] * (np.float32(1.0) / np.float32(buf.samples)))
    # a manual exposure and another operator
    r = subprocess.run(cmd + ["--tonemap", "reinhard", "--exposure", "-0.5", "--white", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_png(shot), d.present(buf, tonemap="reinhard", auto_exposure=0, ev=-0.5, white=2.0))
    doc = json.load(open(stats_p))["display"]
    assert (doc["ev"], doc["operator"], doc["under"], doc["over"]) == (-0.5, "reinhard", 0, 0)
    # without the flags: the plain preview, and no such object
    assert subprocess.run(cmd, capture_output=True, text=True, timeout=300).returncode == 0
    assert np.array_equal(read_png(shot), buf.preview()) and "display" not in json.load(open(stats_p))


@pytest.mark.gpu
def test_cli_display_adapts_across_temporal_frames(bendy, tmp_path):
    import torch
    w, h, spp, n, frames, step = 64, 36, 2, 2, 3, (0.04, 0.015, -0.02)
    shot, stats_p = tmp_path / "t.png", tmp_path / "s.json"
    cmd = [CLI, "--width", str(w), "--height", str(h), "--output", "full", "--scene", scene_path("scene"), "--samples", str(spp),
           "--subsample", str(n), "--temporal", "--frames", str(frames), "--camera-step", ",".join(str(v) for v in step),
           "--stats-json", str(stats_p), "--screenshot", str(shot), "--quiet", "--tonemap", "aces", "--exposure", "auto",
           "--exposure-adapt", "0.5"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sc, cam, cfg, tr, rc = _render(bendy, w, h, spp, n)
    t, d = bendy.Temporal(w, h), bendy.Display(adapt=0.5)
    view = sc.camera_view(cam, cfg, rc, w, h)
    evs = []
    for f in range(frames):
        if f > 0:
            for k in range(3):
                view.to_world[9 + k] = float(np.float32(view.to_world[9 + k]) + np.float32(step[k]))
            sc.set_camera_pose(cam, view.matrix())
        bufs = [bendy.Buffer.new(w, h) for _ in range(4)]
        tr.render_guided(sc, cam, rc, *bufs, seed=0x5EED, sample_base=f * spp)
        out = t.accumulate(view, bufs[0], bufs[2], bufs[3])
        shown = d.present(out)
        evs.append(d.exposure()[0])
    torch.cuda.synchronize()
    doc = json.load(open(stats_p))
    assert np.float32(doc["display"]["ev"]) == np.float32(evs[-1]) and doc["temporal"]["frames"] == frames
    assert len(set(evs)) == frames                                                 # the exposure did move from frame to frame
    assert np.array_equal(read_png(shot), shown)
