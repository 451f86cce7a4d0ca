"""The headless CLI's compare flags (EXTENSION): what is refused before anything is rendered (no GPU), and on the
GPU the `compare` object of --stats-json against `Compare().measure` on the same sequence of stages in Python, the error map
against `.map()`, and the outputs with and without the flag."""
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


def _pfm(path, w, h, magic="PF"):
    with open(path, "wb") as f:
        f.write(f"{magic}\n{w} {h}\n-1.0\n".encode())
        f.write(np.zeros((h, w, 3 if magic == "PF" else 1), dtype="<f4").tobytes())
    return str(path)


def test_cli_refuses_compare_combinations(tmp_path):
    good = _pfm(tmp_path / "t.pfm", 16, 16)
    for output in ("albedo", "normal"):
        r = _cli("--output", output, "--compare", good)
        assert r.returncode != 0 and "--compare needs --output full" in r.stderr
    r = _cli("--output", "full", "--compare", good, "--shard", "0,2")
    assert r.returncode != 0 and "--compare does not apply to a --shard run" in r.stderr
    # a file of another size: the message names both sizes; the shown frame is the resampled or upscaled one
    for w, h, extra, shown in ((17, 16, (), "16x16"), (16, 15, (), "16x16"), (16, 16, ("--resample", "8x8"), "8x8"),
                               (16, 16, ("--upscale", "32x32"), "32x32")):
        r = _cli("--output", "full", "--compare", _pfm(tmp_path / "o.pfm", w, h), *extra)
        assert r.returncode != 0 and f"{w}x{h} pixels" in r.stderr and "shown frame " + shown in r.stderr, r.stderr
    r = _cli("--output", "full", "--compare", str(tmp_path / "missing.pfm"))
    assert r.returncode != 0 and "--compare" in r.stderr and "cannot open" in r.stderr
    (tmp_path / "bad.pfm").write_bytes(b"P6\n16 16\n255\n")
    r = _cli("--output", "full", "--compare", str(tmp_path / "bad.pfm"))
    assert r.returncode != 0 and "not a PFM" in r.stderr
    for extra in (("--compare-tail", "0.5"), ("--compare-map", str(tmp_path / "m.png")), ("--compare-map-scale", "2")):
        r = _cli("--output", "full", *extra)
        assert r.returncode != 0 and "need --compare" in r.stderr, extra
    r = _cli("--output", "full", "--compare", good, "--compare-map-scale", "2")
    assert r.returncode != 0 and "--compare-map-scale needs --compare-map" in r.stderr
    for bad in ("", "0", "-0.1", "1.5", "nan", "half"):
        r = _cli("--output", "full", "--compare", good, "--compare-tail=" + bad)
        assert r.returncode != 0 and "--compare-tail expects a fraction" in r.stderr, bad
    for bad in ("", "0", "-1", "inf", "nan", "big"):
        r = _cli("--output", "full", "--compare", good, "--compare-map", str(tmp_path / "m.png"), "--compare-map-scale=" + bad)
        assert r.returncode != 0 and "--compare-map-scale expects" in r.stderr, bad
    assert not (tmp_path / "m.png").exists()
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--compare TRUTH.pfm" in r.stderr and "--compare-tail 0.01" in r.stderr


@pytest.mark.gpu
def test_cli_compare_stats_map_and_untouched_outputs(bendy, tmp_path):
    import torch
    w, h, n = 48, 36, 2
    truth, shot, stats_p, hdr, emap = tmp_path / "truth.pfm", tmp_path / "g.png", tmp_path / "s.json", tmp_path / "g.pfm", tmp_path / "m.png"
    base = [CLI, "--width", str(w), "--height", str(h), "--output", "full", "--scene", scene_path("scene"), "--subsample", str(n), "--quiet"]
    r = subprocess.run(base + ["--samples", "64", "--samples-per-call", "16", "--no-screenshot", "--hdr", str(truth)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    run = base + ["--samples", "4", "--samples-per-call", "1", "--despeckle", "4", "--glare", "0.1", "--screenshot", str(shot), "--stats-json",
                  str(stats_p), "--hdr", str(hdr)]
    r = subprocess.run(run + ["--compare", str(truth), "--compare-map", str(emap)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "compare:" not in r.stderr, r.stderr                  # --quiet
    doc, png, pfm = json.load(open(stats_p)), open(shot, "rb").read(), open(hdr, "rb").read()
    # the same sequence in Python
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    buf = bendy.Buffer.new(w, h)
    bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4)).render(sc, cam, bendy.RenderConfig(samples=1, subsample=bendy.Subsample(n)),
                                                                           buf, seed=0x5EED)
    torch.cuda.synchronize()
    shown = bendy.Glare().apply(bendy.Despeckle(ratio=4.0).apply(buf), strength=0.1)
    y, tw, th = bendy.read_pfm(truth)
    assert (tw, th) == (w, h)
    ref = bendy.Buffer.new(w, h)
    ref.data.copy_(torch.from_numpy(y))
    ref.samples = 1
    handle = bendy.Compare()
    st = handle.measure(shown, ref)
    share, _ = handle.tail(0.01)
    assert doc["compare"] == {"mse": st.mse, "rel_mse": st.rel_mse, "psnr": st.psnr, "ssim": st.ssim, "max_abs": st.max_abs,
                              "max_x": st.max_index % w, "max_y": st.max_index // w, "valid": st.valid, "nonfinite": st.nonfinite,
                              "tail_fraction": 0.01, "tail_share": share}
    assert st.rel_mse > 0 and st.nonfinite == 0
    assert np.array_equal(read_png(emap), handle.map(1.0).cpu().numpy())
    # another fraction and scale, printed unless --quiet
    quiet = run.index("--quiet")
    r = subprocess.run(run[:quiet] + run[quiet + 1:] + ["--compare", str(truth), "--compare-tail", "0.25", "--compare-map", str(emap),
                                                        "--compare-map-scale", "0.05"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "compare: against" in r.stderr and "saved error map" in r.stderr, r.stderr
    d2 = json.load(open(stats_p))["compare"]
    assert d2["tail_fraction"] == 0.25 and d2["tail_share"] == handle.tail(0.25)[0] and d2["rel_mse"] == st.rel_mse
    assert np.array_equal(read_png(emap), handle.map(0.05).cpu().numpy())
    # a frame against itself: psnr is null
    r = subprocess.run(base + ["--samples", "64", "--samples-per-call", "16", "--no-screenshot", "--stats-json", str(stats_p), "--compare", str(truth)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    same = json.load(open(stats_p))["compare"]
    assert same["psnr"] is None and same["mse"] == 0.0 and same["ssim"] == 1.0 and same["tail_share"] == 0.0
    # without the flag: the same screenshot and --hdr, byte for byte, and no such object
    r = subprocess.run(run, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain = json.load(open(stats_p))
    assert open(shot, "rb").read() == png and open(hdr, "rb").read() == pfm
    assert "compare" not in plain and set(plain) == set(doc) - {"compare"}
    assert {k: v for k, v in plain.items() if k != "calls"} == {k: v for k, v in doc.items() if k not in ("calls", "compare")}
