"""The headless CLI's --adaptive flags (EXTENSION): what is refused before anything is rendered (no GPU), and on
the GPU a run to BT_DONE whose screenshot is the resolved mean."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_cli_io import read_png

CLI = os.path.join(ROOT, "bendy_tracer_amd", "bendy-tracer-hip")


def _cli(*extra):
    return subprocess.run([CLI, "--width", "16", "--height", "16", "--samples", "8", *extra], capture_output=True, text=True,
                          timeout=60)


def test_cli_refuses_adaptive_combinations():
    r = _cli("--output", "albedo", "--adaptive", "0.05")
    assert r.returncode != 0 and "--adaptive needs --output full" in r.stderr
    r = _cli("--output", "full", "--adaptive", "0.05", "--lens", "0,0,0,0.1,0.1,2")
    assert r.returncode != 0 and "--adaptive" in r.stderr and "--lens" in r.stderr
    r = _cli("--output", "full", "--adaptive", "0.05", "--shard", "0,2")
    assert r.returncode != 0 and "--adaptive" in r.stderr and "--shard" in r.stderr
    r = _cli("--output", "full", "--adaptive", "0.05", "--denoise-inline")
    assert r.returncode != 0 and "--adaptive" in r.stderr and "--denoise-inline" in r.stderr
    for bad in ("-0.5", "nan", "inf", "x", ""):
        r = _cli("--output", "full", "--adaptive=" + bad)
        assert r.returncode != 0 and "--adaptive expects a finite threshold >= 0" in r.stderr, bad
    r = _cli("--output", "full", "--adaptive", "0.05", "--adaptive-min", "9")
    assert r.returncode != 0 and "--adaptive-min must not exceed --samples" in r.stderr
    for flag in (("--adaptive-min", "4"), ("--adaptive-map", "m.png")):
        r = _cli("--output", "full", *flag)
        assert r.returncode != 0 and "need --adaptive" in r.stderr
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--adaptive THRESHOLD" in r.stderr and "--adaptive-map" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("denoise", [False, True])
def test_cli_adaptive_run(bendy, tmp_path, denoise):
    """--samples is the cap, --samples-per-call the pass; the loop ends at BT_DONE; the screenshot is resolve().preview() of the
    same passes through the Python API (or its denoised mean), the count map one grey pixel per tile."""
    import torch
    w, h, cap, mn, spp, n, thr = 77, 45, 24, 8, 1, 2, 0.05
    shot, stats_p, map_p = tmp_path / "a.png", tmp_path / "s.json", tmp_path / "m.png"
    cmd = [CLI, "--width", str(w), "--height", str(h), "--output", "full", "--scene", scene_path("scene"), "--samples", str(cap),
           "--subsample", str(n), "--samples-per-call", str(spp), "--adaptive", str(thr), "--adaptive-min", str(mn),
           "--adaptive-map", str(map_p), "--stats-json", str(stats_p), "--screenshot", str(shot), "--quiet"]
    r = subprocess.run(cmd + (["--denoise"] if denoise else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    tr = bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4))
    buf, ad = bendy.Buffer.new(w, h), bendy.Adaptive(w, h, threshold=thr, min_samples=mn, max_samples=cap)
    rc = bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n))
    passes = 1
    while tr.render_adaptive(sc, cam, rc, buf, ad, seed=0x5EED) != bendy.Status.Done:
        passes += 1
        assert passes <= cap
    counts, st = ad.counts(), ad.poll()
    doc, shown = json.load(open(stats_p)), read_png(shot)
    assert doc["adaptive"] == {"active_tiles": 0, "tiles": st.tiles, "min_count": st.min_count, "max_count": st.max_count,
                               "pixel_samples": st.pixel_samples, "passes": passes}
    assert len(doc["calls"]) == passes and doc["calls"][-1]["active_tiles"] == 0
    if not denoise:                                                           # without the flag the file has no such object
        plain = [c for c in cmd if c not in ("--adaptive", str(thr), "--adaptive-min", "--adaptive-map", str(map_p))]
        plain.remove(str(mn))                                                 # (the run below overwrites screenshot and stats)
        assert subprocess.run(plain, capture_output=True, text=True, timeout=300).returncode == 0
        assert "adaptive" not in json.load(open(stats_p)) and "active_tiles" not in json.load(open(stats_p))["calls"][0]
    assert st.min_count >= mn and st.max_count <= cap and st.min_count < st.max_count
    mean = ad.resolve(buf)
    if denoise:
        guides = []
        for out in (bendy.Output.Albedo, bendy.Output.Normal, bendy.Output.Depth):
            g = bendy.Buffer.new(w, h)
            bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4, output=out)).render(
                sc, cam, bendy.RenderConfig(samples=4, subsample=bendy.Subsample(n)), g, seed=0x5EED, sample_base=0)
            guides.append(g)
        mean = bendy.denoise(mean, *guides)
        torch.cuda.synchronize()
    assert np.array_equal(shown, mean.preview())
    grey = read_png(map_p)
    assert grey.shape == (counts.shape[0], counts.shape[1], 4)
    assert np.array_equal(grey[..., 0], (counts.astype(np.int64) * 255 // cap).astype(np.uint8)) and (grey[..., 3] == 255).all()
