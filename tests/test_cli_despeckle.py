"""The headless CLI's despeckle flags (EXTENSION): what is refused before anything is rendered (no GPU), and on the
GPU the screenshot against the Python sequence render -> Despeckle -> Glare -> Display of the same frame, the same under
--temporal (each frame's sums before the accumulate), the `despeckle` object of --stats-json, and the outputs without the flag."""
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


def test_cli_refuses_despeckle_combinations():
    r = _cli("--output", "albedo", "--despeckle", "4")
    assert r.returncode != 0 and "--despeckle needs --output full" in r.stderr
    r = _cli("--output", "normal", "--despeckle", "4", "--despeckle-rank", "3")
    assert r.returncode != 0 and "--despeckle needs --output full" in r.stderr
    r = _cli("--output", "full", "--shard", "0,2", "--despeckle", "4")
    assert r.returncode != 0 and "--despeckle" in r.stderr and "--shard" in r.stderr
    for flags in (("--despeckle-rank", "3"), ("--despeckle-radius", "2")):
        r = _cli("--output", "full", *flags)
        assert r.returncode != 0 and "need --despeckle" in r.stderr, flags
    for bad in ("", "x", "nan", "inf", "0.5", "-4", "4x"):
        r = _cli("--output", "full", "--despeckle=" + bad)
        assert r.returncode != 0 and "--despeckle expects a finite ratio >= 1" in r.stderr, bad
    for bad in ("", "x", "0", "-1", "25", "2.5"):
        r = _cli("--output", "full", "--despeckle", "4", "--despeckle-rank=" + bad)
        assert r.returncode != 0 and "--despeckle-rank expects a count in 1 .. 24" in r.stderr, bad
    for bad in ("", "x", "0", "3", "1.5"):
        r = _cli("--output", "full", "--despeckle", "4", "--despeckle-radius=" + bad)
        assert r.returncode != 0 and "--despeckle-radius expects 1 or 2" in r.stderr, bad
    r = _cli("--output", "full", "--despeckle", "4", "--despeckle-rank", "9")
    assert r.returncode != 0 and "--despeckle-rank must not exceed" in r.stderr
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--despeckle RATIO" in r.stderr and "--despeckle-rank" in r.stderr and "--despeckle-radius" in r.stderr


def _render(bendy, w, h, spp, n):
    import torch
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    buf = bendy.Buffer.new(w, h)
    bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4)).render(
        sc, cam, bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n)), buf, seed=0x5EED)
    torch.cuda.synchronize()
    return buf


@pytest.mark.gpu
def test_cli_despeckle_screenshot_hdr_and_stats(bendy, tmp_path):
    w, h, spp, n = 64, 36, 2, 2
    shot, stats_p, hdr = tmp_path / "d.png", tmp_path / "s.json", tmp_path / "d.pfm"
    cmd = [CLI, "--width", str(w), "--height", str(h), "--output", "full", "--scene", scene_path("scene"), "--samples", str(spp * n * n),
           "--subsample", str(n), "--samples-per-call", str(spp), "--stats-json", str(stats_p), "--screenshot", str(shot), "--quiet"]
    r = subprocess.run(cmd + ["--despeckle", "4", "--glare", "0.1", "--tonemap", "aces", "--exposure", "auto", "--hdr", str(hdr)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    buf = _render(bendy, w, h, spp, n)
    ds, gl, d = bendy.Despeckle(), bendy.Glare(), bendy.Display()
    clean = ds.apply(buf, ratio=4.0)
    st = ds.poll()
    glared = gl.apply(clean, strength=0.1)
    assert np.array_equal(read_png(shot), d.present(glared, tonemap="aces"))       # pixel for pixel
    doc = json.load(open(stats_p))
    assert doc["despeckle"] == {"ratio": 4.0, "rank": 2, "radius": 1, "flagged": st.flagged, "sanitised": st.sanitised}
    assert "glare" in doc and "display" in doc
    magic, scale, rows = read_pfm(hdr)                                             # --hdr holds what is shown
    assert (magic, scale) == (b"PF", b"-1.0")
    assert np.array_equal(rows[::-1], glared.numpy()[..., :3])
    # the other two flags, without any other stage: the plain preview of the despeckled sums, and their mean in --hdr
    r = subprocess.run(cmd + ["--despeckle", "1.5", "--despeckle-rank", "5", "--despeckle-radius", "2", "--hdr", str(hdr)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    clean = ds.apply(buf, ratio=1.5, rank=5, radius=2)
    st = ds.poll()
    assert st.flagged > 0 and clean.samples == buf.samples
    assert np.array_equal(read_png(shot), clean.preview())
    assert np.array_equal(read_pfm(hdr)[2][::-1], clean.numpy()[..., :3] * (np.float32(1.0) / np.float32(clean.samples)))
    doc = json.load(open(stats_p))
    assert doc["despeckle"] == {"ratio": 1.5, "rank": 5, "radius": 2, "flagged": st.flagged, "sanitised": st.sanitised}
    assert "glare" not in doc and "display" not in doc
    # without the flag: the plain preview, the mean in --hdr, and no such object
    assert subprocess.run(cmd + ["--hdr", str(hdr)], capture_output=True, text=True, timeout=300).returncode == 0
    assert np.array_equal(read_png(shot), buf.preview()) and "despeckle" not in json.load(open(stats_p))
    assert np.array_equal(read_pfm(hdr)[2][::-1], buf.numpy()[..., :3] * (np.float32(1.0) / np.float32(buf.samples)))
    # and with the other stages alone, what they showed before: glare and display of the raw sums
    r = subprocess.run(cmd + ["--glare", "0.1", "--tonemap", "aces", "--exposure", "auto"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_png(shot), bendy.Display().present(gl.apply(buf, strength=0.1), tonemap="aces"))
    assert "despeckle" not in json.load(open(stats_p))


@pytest.mark.gpu
def test_cli_despeckle_under_temporal(bendy, tmp_path):
    """Under --temporal each frame's sums are despeckled before they enter the history."""
    import torch
    w, h, spp, n, frames, step = 64, 36, 2, 2, 2, (0.04, 0.015, -0.02)
    shot, stats_p = tmp_path / "t.png", tmp_path / "s.json"
    cmd = [CLI, "--width", str(w), "--height", str(h), "--output", "full", "--scene", scene_path("scene"), "--samples", str(spp),
           "--subsample", str(n), "--temporal", "--frames", str(frames), "--camera-step", ",".join(str(v) for v in step),
           "--screenshot", str(shot), "--quiet", "--stats-json", str(stats_p), "--despeckle", "4", "--glare", "0.1", "--tonemap", "aces",
           "--exposure", "auto"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    cfg = bendy.Config(chunks_x=8, chunks_y=4)
    tr, rc = bendy.Tracer.with_config(cfg), bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n))
    t, ds, gl, d = bendy.Temporal(w, h), bendy.Despeckle(ratio=4.0), bendy.Glare(strength=0.1), bendy.Display()
    view = sc.camera_view(cam, cfg, rc, w, h)
    for f in range(frames):
        if f > 0:
            for k in range(3):
                view.to_world[9 + k] = float(np.float32(view.to_world[9 + k]) + np.float32(step[k]))
            sc.set_camera_pose(cam, view.matrix())
        bufs = [bendy.Buffer.new(w, h) for _ in range(4)]
        tr.render_guided(sc, cam, rc, *bufs, seed=0x5EED, sample_base=f * spp)
        clean = ds.apply(bufs[0])
        assert clean.samples == bufs[0].samples == spp * n * n
        shown = d.present(gl.apply(t.accumulate(view, clean, bufs[2], bufs[3])), tonemap="aces")
    torch.cuda.synchronize()
    assert np.array_equal(read_png(shot), shown)
    st = ds.poll()                                                                 # the last frame's counts
    assert json.load(open(stats_p))["despeckle"] == {"ratio": 4.0, "rank": 2, "radius": 1, "flagged": st.flagged, "sanitised": st.sanitised}
