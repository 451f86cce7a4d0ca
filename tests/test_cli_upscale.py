"""The headless CLI's upscale flags (EXTENSION): what is refused before anything is rendered (no GPU), and on the
GPU the screenshot against `Display().present(Glare().apply(Upscale().apply(...)))` of the same renders, --hdr holding the
upscaled mean, the `upscale` object of --stats-json, the stage after --despeckle and --denoise-inline, and the outputs without
the flag."""
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


def test_cli_refuses_upscale_combinations():
    for output in ("albedo", "normal"):
        r = _cli("--output", output, "--upscale", "32x32")
        assert r.returncode != 0 and "--upscale needs --output full" in r.stderr
    for other, word in ((("--shard", "0,2"), "--shard"), (("--lens", "0,0,0,1,0.1,5"), "--lens"), (("--resample", "8x8"), "--resample"),
                        (("--denoise",), "--denoise-inline"), (("--adaptive", "0.05"), "--adaptive"), (("--temporal",), "--temporal")):
        r = _cli("--output", "full", "--upscale", "32x32", *other)
        assert r.returncode != 0 and "--upscale" in r.stderr and word in r.stderr, (other, r.stderr)
    for small in ("15x32", "32x15", "8x8"):
        r = _cli("--output", "full", "--upscale", small)
        assert r.returncode != 0 and "--upscale must not be smaller" in r.stderr and "--resample" in r.stderr, small
    r = _cli("--output", "full", "--upscale-guide-samples", "2")
    assert r.returncode != 0 and "--upscale-guide-samples needs --upscale" in r.stderr
    for bad in ("", "x", "32", "32x", "x32", "0x32", "32x0", "-32x32", "32x-32", "32x32x32", "32.5x32", "32 x 32", "nanxinf"):
        r = _cli("--output", "full", "--upscale=" + bad)
        assert r.returncode != 0 and "--upscale expects WxH" in r.stderr, bad
    for bad in ("", "0", "-1", "1.5", "many", "65536"):
        r = _cli("--output", "full", "--upscale", "32x32", "--upscale-guide-samples=" + bad)
        assert r.returncode != 0 and "--upscale-guide-samples expects a count" in r.stderr, bad
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--upscale WxH" in r.stderr and "--upscale-guide-samples 1" in r.stderr


@pytest.mark.gpu
def test_cli_upscale_screenshot_hdr_and_stats(bendy, tmp_path):
    import torch
    w, h, W, H, spp, n = 48, 36, 96, 72, 2, 2
    shot, stats_p, hdr = tmp_path / "g.png", tmp_path / "s.json", tmp_path / "g.pfm"
    cmd = [CLI, "--width", str(w), "--height", str(h), "--output", "full", "--scene", scene_path("scene"), "--samples", str(spp * n * n),
           "--subsample", str(n), "--samples-per-call", str(spp), "--stats-json", str(stats_p), "--screenshot", str(shot), "--quiet"]
    r = subprocess.run(cmd + ["--upscale", f"{W}x{H}", "--glare", "0.1", "--tonemap", "aces", "--exposure", "auto", "--hdr", str(hdr)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cfg = dict(chunks_x=8, chunks_y=4)
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, W / H)
    rc = bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n))
    lo = [bendy.Buffer.new(w, h) for _ in range(4)]
    bendy.Tracer.with_config(bendy.Config(**cfg)).render_guided(sc, cam, rc, *lo, seed=0x5EED)

    def hi_guides(samples):
        out = []
        for output in (bendy.Output.Albedo, bendy.Output.Normal, bendy.Output.Depth):
            b = bendy.Buffer.new(W, H)
            bendy.Tracer.with_config(bendy.Config(output=output, **cfg)).render(
                sc, cam, bendy.RenderConfig(samples=samples, subsample=bendy.Subsample(n)), b, seed=0x5EED)
            out.append(b)
        return tuple(out)

    hi = hi_guides(1)
    torch.cuda.synchronize()
    up, gl, d = bendy.Upscale(), bendy.Glare(), bendy.Display()
    big = up.apply(lo[0], W, H, lo=tuple(lo[1:]), hi=hi)
    st = up.poll()
    glared = gl.apply(big, strength=0.1)
    png = read_png(shot)
    assert png.shape == (H, W, 4) and np.array_equal(png, d.present(glared, tonemap="aces"))           # pixel for pixel
    doc = json.load(open(stats_p))
    assert doc["upscale"] == {"width": W, "height": H, "tier2": st.tier2, "tier3": st.tier3}
    assert "display" in doc and "glare" in doc and "resample" not in doc and (doc["width"], doc["height"]) == (w, h)
    magic, scale, rows = read_pfm(hdr)                                             # --hdr holds the 96 x 72 mean, glared
    assert (magic, scale) == (b"PF", b"-1.0") and rows.shape == (H, W, 3)
    assert np.array_equal(rows[::-1], glared.numpy()[..., :3])
    # after --despeckle and --denoise-inline, with guides of two samples, and the plain preview
    r = subprocess.run(cmd + ["--upscale", f"{W}x{H}", "--upscale-guide-samples", "2", "--despeckle", "4", "--denoise-inline", "--hdr", str(hdr)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    clean = bendy.Despeckle(ratio=4.0).apply(lo[0])
    den = bendy.Denoiser().denoise(clean, *lo[1:])
    big = up.apply(den, W, H, lo=tuple(lo[1:]), hi=hi_guides(2))
    st = up.poll()
    assert np.array_equal(read_png(shot), big.preview())
    assert np.array_equal(read_pfm(hdr)[2][::-1], big.numpy()[..., :3])
    doc = json.load(open(stats_p))
    assert doc["upscale"] == {"width": W, "height": H, "tier2": st.tier2, "tier3": st.tier3} and "display" not in doc and "despeckle" in doc
    # the same size is allowed
    r = subprocess.run(cmd + ["--upscale", f"{w}x{h}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and read_png(shot).shape == (h, w, 4), r.stderr
    # without the flag: the plain preview, the mean in --hdr, and no such object
    assert subprocess.run(cmd + ["--hdr", str(hdr)], capture_output=True, text=True, timeout=300).returncode == 0
    sc.set_camera_aspect(cam, w / h)
    buf = bendy.Buffer.new(w, h)
    bendy.Tracer.with_config(bendy.Config(**cfg)).render(sc, cam, rc, buf, seed=0x5EED)
    torch.cuda.synchronize()
    assert np.array_equal(read_png(shot), buf.preview()) and "upscale" not in json.load(open(stats_p))
    assert np.array_equal(read_pfm(hdr)[2][::-1], buf.numpy()[..., :3] * (np.float32(1.0) / np.float32(buf.samples)))
