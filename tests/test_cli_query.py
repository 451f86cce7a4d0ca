"""The headless CLI's --pick and --autofocus (EXTENSION): what is refused before anything is rendered (no GPU), and
on the GPU --pick's JSON against `Scene.pick` and --autofocus's screenshot against Python's render after `set_camera_focus`."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_cli_io import read_png

CLI = os.path.join(ROOT, "bendy_tracer_amd", "bendy-tracer-hip")


def _cli(*extra):
    return subprocess.run([CLI, "--width", "16", "--height", "12", "--samples", "1", "--output", "full", *extra], capture_output=True,
                          text=True, timeout=60)


def test_cli_refuses_pick_and_autofocus_combinations():
    for flag in ("--pick", "--autofocus"):
        for spec in ("16,0", "0,12", "99,99"):
            r = _cli(flag, spec)
            assert r.returncode != 0 and flag in r.stderr and "outside the 16x12 frame" in r.stderr, r.stderr
        r = _cli(flag, "3,3", "--lens", "0,0,0,0.1,0.05,2")
        assert r.returncode != 0 and flag + " sends a straight ray: not with --lens" in r.stderr, r.stderr
        r = _cli(flag, "3,3", "--shard", "0,2")
        assert r.returncode != 0 and flag + " does not apply to a --shard run" in r.stderr, r.stderr
        for bad in ("", "3", "3,", "a,b", "-1,2", "3,4,5", "3,4x"):
            r = _cli(flag + "=" + bad)
            assert r.returncode != 0 and flag + " expects X,Y" in r.stderr, (bad, r.stderr)
        assert r.stdout == ""
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--pick X,Y" in r.stderr and "--autofocus X,Y" in r.stderr


def _f32(v):
    return np.asarray(v, np.float32).tolist()


@pytest.mark.gpu
def test_cli_pick_and_autofocus_match_python(bendy, tmp_path):
    import torch
    w, h, spp = 48, 32, 4
    base = [CLI, "--width", str(w), "--height", str(h), "--output", "full", "--scene", scene_path("scene"), "--subsample", "2", "--quiet",
            "--samples", str(spp), "--seed", "99"]
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    cfg, rc = bendy.Config(chunks_x=8, chunks_y=4), bendy.RenderConfig.with_samples_subsample(1, bendy.Subsample(2))   # the CLI's: one sample per call
    hit_px = next((x, y) for y in range(h // 2, h) for x in range(w // 2, w) if sc.pick(cam, cfg, rc, w, h, x, y) is not None)
    miss_px = next(((x, y) for y in range(h) for x in range(w) if sc.pick(cam, cfg, rc, w, h, x, y) is None), None)
    stats = tmp_path / "s.json"
    for px in filter(None, (hit_px, miss_px)):
        r = subprocess.run(base + ["--no-screenshot", "--pick", f"{px[0]},{px[1]}", "--stats-json", str(stats)], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        line = json.loads(r.stdout.strip().splitlines()[0])
        want = sc.pick(cam, cfg, rc, w, h, *px)
        assert json.loads(stats.read_text())["pick"] == line["pick"]
        if want is None:
            assert line == {"pick": None}
            continue
        got = line["pick"]
        assert set(got) == set(want)
        for k in want:                                        # the CLI prints float32 values with nine digits: the same float32
            assert (_f32(got[k]) == _f32(want[k])) if isinstance(want[k], (float, list)) else got[k] == want[k], k

    shot = tmp_path / "af.png"
    r = subprocess.run(base + ["--screenshot", str(shot), "--autofocus", f"{hit_px[0]},{hit_px[1]}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sc.set_camera_focus(cam, sc.pick(cam, cfg, rc, w, h, *hit_px)["focus"])
    buf = bendy.Buffer.new(w, h)
    while buf.samples < spp:
        bendy.Tracer.with_config(cfg).render(sc, cam, rc, buf, seed=99)
    torch.cuda.synchronize()
    assert np.array_equal(read_png(str(shot)), buf.preview())
    if miss_px is not None:
        r = subprocess.run(base + ["--no-screenshot", "--autofocus", f"{miss_px[0]},{miss_px[1]}"], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and f"({miss_px[0]}, {miss_px[1]}) hits nothing" in r.stderr
