"""Guided render (EXTENSION): Tracer.render_guided / bt_render_guided_device add the colour samples and, from the
same paths, the Albedo / Normal / Depth values to four frames in one pass.  The yardstick is the CPU oracle, which renders
each Output mode on its own: every frame must equal the oracle's bit for bit, and the segment count must be the oracle's."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from helpers import flat_scene_json, gpu_scene, oracle_scene

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "bendy_tracer_amd", "bendy-tracer-hip")
SEED = 0x5EED
NAMES = ("color", "albedo", "normal", "depth")


def _oracle4(o, osc, ocam, w, h, spp, n=0, seed=SEED, sample_base=0, pre=None, **kw):
    """The oracle's four renders (Output 0 .. 3) and the segment count of the Full one."""
    frames, segs = [], []
    for out in range(4):
        cfg = o.default_config(samples=spp, subsample_n=n, output=out, recursive=0, sample_base=sample_base, **kw)
        img, _, seg = o.render(osc, ocam, cfg, w, h, seed, nthreads=16, rgba=None if pre is None else pre[out].copy())
        frames.append(img)
        segs.append(seg)
    assert len(set(segs)) == 1          # the four modes walk the same paths
    return frames, segs[0]


def _frames(b, w, h, fill=None):
    """Four Buffers that are views of ONE tensor [4, h, w, 4]: a write past the end of a frame lands in its neighbour."""
    import torch
    block = torch.zeros((4, h, w, 4), dtype=torch.float32, device="cuda")
    block[..., 3] = 1.0
    if fill is not None:
        block.copy_(torch.from_numpy(np.stack(fill)))
    bufs = []
    for i in range(4):
        buf = b.Buffer.new(1, 1)
        buf.width, buf.height, buf.data = w, h, block[i]
        bufs.append(buf)
    return bufs


def _guided(b, sc, cam, bufs, spp, n=0, seed=SEED, use=(True, True, True), config=None, sample_base=None, **rc_kw):
    import torch
    tr = b.Tracer.with_config(config or b.Config(chunks_x=8, chunks_y=4))
    guides = [bufs[i + 1] if use[i] else None for i in range(3)]
    st = tr.render_guided(sc, cam, b.RenderConfig(samples=spp, subsample=b.Subsample(n), **rc_kw), bufs[0], *guides, seed=seed,
                          sample_base=sample_base)
    torch.cuda.synchronize()
    return st, sc.last_stats()


def _same(bufs, want, nan=False):
    for name, buf, img in zip(NAMES, bufs, want):
        assert np.array_equal(buf.numpy(), img, equal_nan=nan), name


def _json_scenes(b, o, txt, w, h):
    gs = b.Scene.from_json(txt)
    cam = gs.find_by_tag("camera")
    gs.set_camera_aspect(cam, w / h)
    osc = o.Scene(json.loads(txt))
    ocam = osc.find_by_tag("camera")
    osc.set_camera_aspect(ocam, w / h)
    return gs, cam, osc, ocam


@pytest.mark.parametrize("n", [0, 2])
@pytest.mark.parametrize("name,w,h", [("scene", 61, 37), ("cornell", 96, 54), ("cornell2", 45, 77), ("volume", 61, 37),
                                      ("cloud", 50, 30)])
def test_bundled_scenes(bendy, oracle, name, w, h, n):
    spp = 2 if n else 5
    sc, cam = gpu_scene(bendy, name, w, h)
    bufs = _frames(bendy, w, h)
    st, stats = _guided(bendy, sc, cam, bufs, spp, n=n)
    osc, ocam = oracle_scene(oracle, name, w, h)
    want, seg = _oracle4(oracle, osc, ocam, w, h, spp, n=n)
    assert st == bendy.Status.InProgress and all(buf.samples == spp * max(1, n * n) for buf in bufs)
    assert stats.segments == seg and stats.samples == w * h * spp * max(1, n * n) and stats.pixels == w * h
    tiles = -(-w // 16) * -(-h // 16)
    assert stats.parked_bytes == tiles * 256 * spp * max(1, n * n) * 40
    _same(bufs, want)


@pytest.mark.parametrize("seed", range(12))
def test_random_scenes(bendy, oracle, seed):
    """scene_gen.random_scene: every primitive, material and light kind, volumes, scaled transforms, three kinds of root."""
    from scene_gen import random_scene
    w, h, spp = 72, 48, 4
    gs, cam, osc, ocam = _json_scenes(bendy, oracle, random_scene(seed, n_objects=4 + seed % 9), w, h)
    bufs = _frames(bendy, w, h)
    _, stats = _guided(bendy, gs, cam, bufs, spp, seed=seed)
    want, seg = _oracle4(oracle, osc, ocam, w, h, spp, seed=seed)
    assert stats.segments == seg
    _same(bufs, want, nan=True)


_shape_cache = {}


@pytest.mark.parametrize("packed", [0, 1, 2])
@pytest.mark.parametrize("slices", [1, 2, 4, 8, 16, 32])
@pytest.mark.parametrize("name", ["scene", "cornell2"])
def test_every_pinned_launch_shape(bendy, oracle, name, slices, packed):
    """bt_tuning.slices x bt_tuning.packed.  The frame is 330 x 200 (larger than the other cases') because a packed launch
    exists only where the launch has more blocks than the GPU has workgroup slots (7 per CU): 273 tiles x 8 slices and up.
    The guided builds have no compacting drain: packed = 2 runs as 1."""
    import torch
    w, h, spp = 330, 200, 2
    if name not in _shape_cache:
        osc, ocam = oracle_scene(oracle, name, w, h)
        _shape_cache[name] = _oracle4(oracle, osc, ocam, w, h, spp)
    want, seg = _shape_cache[name]
    sc, cam = gpu_scene(bendy, name, w, h, tuning={"slices": slices, "packed": packed})
    bufs = _frames(bendy, w, h)
    _, stats = _guided(bendy, sc, cam, bufs, spp)
    slots = torch.cuda.get_device_properties(0).multi_processor_count * 7
    blocks = -(-w // 16) * -(-h // 16) * slices
    assert stats.slices == slices and stats.segments == seg
    assert stats.packed == (1 if packed and blocks > slots else 0)
    if name == "cornell2" and packed == 2 and slices >= 16:
        assert blocks > slots and stats.packed == 1            # (needs a GPU with at most 624 CUs to be a packed launch)
    _same(bufs, want)


def test_small_scratch_cap_splits_the_guided_render_into_more_launches(bendy, oracle):
    """40 bytes per guided sample against 12: under the cap that makes 40 plain samples four launches (12 + 12 + 12 + 4,
    as tests/test_gpu_parity.py pins it) the guided render takes 14 launches of 3 samples (the last of 1)."""
    from helpers import gpu_render
    w, h, spp = 64, 48, 40
    cap = 64 * 48 * 12 * 12
    sc, cam = gpu_scene(bendy, "volume", w, h, tuning={"scratch_cap_bytes": cap})
    bufs = _frames(bendy, w, h)
    _, stats = _guided(bendy, sc, cam, bufs, spp)
    osc, ocam = oracle_scene(oracle, "volume", w, h)
    want, seg = _oracle4(oracle, osc, ocam, w, h, spp)
    assert stats.launches == 14 and stats.launches >= 3 and 0 < stats.scratch_bytes <= cap
    assert stats.segments == seg and stats.parked_bytes == w * h * spp * 40
    _same(bufs, want)
    # two guides: 28 bytes per sample, 5 samples per launch
    bufs2 = _frames(bendy, w, h)
    _, stats2 = _guided(bendy, sc, cam, bufs2, spp, use=(True, False, True))
    assert stats2.launches == 8 and stats2.parked_bytes == w * h * spp * 28
    _same([bufs2[0], bufs2[1], bufs2[3]], [want[0], want[1], want[3]])
    # the plain render under the same cap: what it is today
    plain, pstats, _ = gpu_render(bendy, "volume", w, h, spp, tuning={"scratch_cap_bytes": cap})
    assert pstats.launches == 4 and pstats.parked_bytes == w * h * spp * 12 and np.array_equal(plain.numpy(), want[0])


def test_progressive_calls_and_prefilled_frames(bendy, oracle):
    """k guided calls of 1 sample x Subpixel(2) == one guided call of k samples == the oracle; frames that hold sums already are
    added to (alpha untouched)."""
    w, h, k = 80, 50, 3
    sc, cam = gpu_scene(bendy, "cornell", w, h)
    osc, ocam = oracle_scene(oracle, "cornell", w, h)
    want, seg = _oracle4(oracle, osc, ocam, w, h, k, n=2)
    one = _frames(bendy, w, h)
    _guided(bendy, sc, cam, one, k, n=2)
    many = _frames(bendy, w, h)
    for i in range(k):
        _guided(bendy, sc, cam, many, 1, n=2)                 # sample_base = what the colour buffer holds
    assert all(buf.samples == 4 * k for buf in one + many)
    _same(one, want)
    _same(many, want)
    rng = np.random.default_rng(5)
    pre = [rng.uniform(0.1, 3.0, (h, w, 4)).astype(np.float32) for _ in range(4)]
    filled = _frames(bendy, w, h, fill=pre)
    _, stats = _guided(bendy, sc, cam, filled, k, n=2, sample_base=0)
    want_pre, _ = _oracle4(oracle, osc, ocam, w, h, k, n=2, pre=pre)
    assert stats.segments == seg
    _same(filled, want_pre)
    for buf, p in zip(filled, pre):
        assert np.array_equal(buf.numpy()[..., 3], p[..., 3])


@pytest.mark.parametrize("mask", range(8))
@pytest.mark.parametrize("name", ["scene", "cloud"])
def test_every_subset_of_guides(bendy, oracle, name, mask):
    """A guide that is not passed is neither parked nor summed: its (sentinel-filled) frame, which lies between the others in
    one allocation, keeps every bit; the frames that are passed equal the oracle's."""
    import torch
    from helpers import gpu_render
    w, h, spp = 56, 34, 3
    use = tuple(bool(mask >> i & 1) for i in range(3))
    sentinel = [np.full((h, w, 4), -7.5 - i, np.float32) for i in range(4)]
    sc, cam = gpu_scene(bendy, name, w, h)
    bufs = _frames(bendy, w, h)
    for i in range(3):
        if not use[i]:
            bufs[i + 1].data.copy_(torch.from_numpy(sentinel[i + 1]))
    _, stats = _guided(bendy, sc, cam, bufs, spp, use=use)
    key = (name, "subsets")
    if key not in _shape_cache:
        osc, ocam = oracle_scene(oracle, name, w, h)
        _shape_cache[key] = _oracle4(oracle, osc, ocam, w, h, spp)
    want, seg = _shape_cache[key]
    assert stats.segments == seg
    assert stats.parked_bytes == -(-w // 16) * -(-h // 16) * 256 * spp * (12 + 12 * use[0] + 12 * use[1] + 4 * use[2])
    assert np.array_equal(bufs[0].numpy(), want[0]) and bufs[0].samples == spp
    for i in range(3):
        if use[i]:
            assert np.array_equal(bufs[i + 1].numpy(), want[i + 1]) and bufs[i + 1].samples == spp
        else:
            assert np.array_equal(bufs[i + 1].numpy(), sentinel[i + 1]) and bufs[i + 1].samples == 0
    if mask == 0:       # no guide at all: the plain Full render, launch shape and all
        _, pstats, _ = gpu_render(bendy, name, w, h, spp)
        assert (stats.slices, stats.launches, stats.workgroups, stats.packed) == (pstats.slices, pstats.launches, pstats.workgroups, pstats.packed)


@pytest.mark.parametrize("name", ["cornell2", "cloud", "scene"])
def test_paths_that_end_before_or_at_their_first_event(bendy, oracle, name):
    w, h, spp = 60, 40, 3
    sc, cam = gpu_scene(bendy, name, w, h)
    osc, ocam = oracle_scene(oracle, name, w, h)
    # Config.max_bounces = 0: the first scatter is the last event
    bufs = _frames(bendy, w, h)
    _, stats = _guided(bendy, sc, cam, bufs, spp, config=bendy.Config(chunks_x=8, chunks_y=4, max_bounces=0))
    want, seg = _oracle4(oracle, osc, ocam, w, h, spp, max_bounces=0)
    assert stats.segments == seg
    _same(bufs, want)
    # RenderConfig.max_bounces overrides both limits (quirk Q1, mod.rs:223-224)
    for mb in (0, 1):
        bufs = _frames(bendy, w, h)
        _, stats = _guided(bendy, sc, cam, bufs, spp, max_bounces=mb)
        want, seg = _oracle4(oracle, osc, ocam, w, h, spp, max_bounces=mb, max_volume_bounces=mb)
        assert stats.segments == seg
        _same(bufs, want)


def test_flat_scene_and_scene_without_primitives(bendy, oracle):
    """Flat / Emissive materials only: every path ends at its first hit (ColorData::from_emitted) or at the root."""
    w, h, spp = 33, 33, 4
    color = (0.25, 0.5, 0.75)
    txt = flat_scene_json(sphere_color=color, root_intensity=0.5)
    gs, cam, osc, ocam = _json_scenes(bendy, oracle, txt, w, h)
    gs.set_camera_aspect(cam, 1.0)
    osc.set_camera_aspect(ocam, 1.0)
    bufs = _frames(bendy, w, h)
    _, stats = _guided(bendy, gs, cam, bufs, spp)
    want, seg = _oracle4(oracle, osc, ocam, w, h, spp)
    assert stats.segments == seg == w * h * spp
    _same(bufs, want)
    assert np.array_equal(bufs[0].numpy()[16, 16, :3], np.float32(4) * np.array(color, np.float32))     # closed form
    assert np.array_equal(bufs[1].numpy()[16, 16, :3], np.float32(4) * np.array(color, np.float32))     # albedo = emitted
    assert np.array_equal(bufs[2].numpy()[16, 16, :3], np.zeros(3, np.float32))                         # no scatter, no normal
    assert np.array_equal(bufs[3].numpy()[16, 16, :3], np.full(3, 4, np.float32))                       # depth stays +inf -> 1
    doc = json.loads(txt)
    del doc["objects"]["collection"]["1"]
    gs, cam, osc, ocam = _json_scenes(bendy, oracle, json.dumps(doc), 40, 24)
    bufs = _frames(bendy, 40, 24)
    _, stats = _guided(bendy, gs, cam, bufs, 3)
    want, seg = _oracle4(oracle, osc, ocam, 40, 24, 3)
    assert gs.export_prims().shape[0] == 0 and stats.segments == seg
    _same(bufs, want)


def test_interleaved_with_plain_renders_on_one_handle(bendy):
    """The scratch is shared with the plain renders and carries nothing over: plain Full, guided, plain Albedo, plain Full again
    on ONE handle each give what a fresh handle gives."""
    import torch
    w, h, spp = 150, 90, 6

    def plain(sc, cam, output):
        buf = bendy.Buffer.new(w, h)
        bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4, output=output)).render(
            sc, cam, bendy.RenderConfig.with_samples(spp), buf)
        torch.cuda.synchronize()
        return buf.numpy().copy(), sc.last_stats()

    def guided(sc, cam):
        bufs = _frames(bendy, w, h)
        _, st = _guided(bendy, sc, cam, bufs, spp)
        return [b_.numpy().copy() for b_ in bufs], st

    for name in ("volume", "cornell2"):
        fresh_full, fs = plain(*gpu_scene(bendy, name, w, h), bendy.Output.Full)
        fresh_albedo, _ = plain(*gpu_scene(bendy, name, w, h), bendy.Output.Albedo)
        fresh_guided, gs = guided(*gpu_scene(bendy, name, w, h))
        assert np.array_equal(fresh_guided[0], fresh_full) and np.array_equal(fresh_guided[1], fresh_albedo)
        assert (gs.segments, gs.samples, gs.pixels, gs.slices, gs.launches, gs.workgroups) == \
               (fs.segments, fs.samples, fs.pixels, fs.slices, fs.launches, fs.workgroups)
        sc, cam = gpu_scene(bendy, name, w, h)
        a, _ = plain(sc, cam, bendy.Output.Full)
        g, _ = guided(sc, cam)
        c, _ = plain(sc, cam, bendy.Output.Albedo)
        d, _ = plain(sc, cam, bendy.Output.Full)
        assert np.array_equal(a, fresh_full) and np.array_equal(c, fresh_albedo) and np.array_equal(d, fresh_full)
        for x, y in zip(g, fresh_guided):
            assert np.array_equal(x, y)


def test_lens_is_unsupported_and_touches_nothing(bendy):
    import torch
    w, h = 48, 32
    sc, cam = gpu_scene(bendy, "scene", w, h)
    sc.set_lens((0.6, 0.4, 4.0), 0.15, 0.1, 6.0, 800)
    rng = np.random.default_rng(9)
    pre = [rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32) for _ in range(4)]
    bufs = _frames(bendy, w, h, fill=pre)
    with pytest.raises(bendy.BendyError) as e:
        _guided(bendy, sc, cam, bufs, 2)
    assert e.value.code == -9
    torch.cuda.synchronize()
    for buf, p in zip(bufs, pre):
        assert np.array_equal(buf.numpy(), p) and buf.samples == 0
    sc.clear_lens()                                            # ... and the handle renders guided frames once the lens is gone
    _, stats = _guided(bendy, sc, cam, bufs, 2)
    assert stats.segments > 0 and all(buf.samples == 2 for buf in bufs)


def test_full_size_equals_the_four_separate_passes(bendy):
    """BASELINE configs[2]'s frame (scene.json 1920 x 1080 x 64): too large for the oracle four times over, so the yardstick
    here is the library's own separate passes -- the unchanged builds that test_c3_scene_1080p_64spp pins to the oracle.  At
    40 B per sample the guided render does not fit the default 2 GiB scratch cap in one launch."""
    import torch
    w, h, spp = 1920, 1080, 64
    sc, cam = gpu_scene(bendy, "scene", w, h)
    bufs = _frames(bendy, w, h)
    _, gstats = _guided(bendy, sc, cam, bufs, spp)
    assert gstats.launches == 3 and gstats.samples == w * h * spp
    for i, output in enumerate((bendy.Output.Full, bendy.Output.Albedo, bendy.Output.Normal, bendy.Output.Depth)):
        ref = bendy.Buffer.new(w, h)
        bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4, output=output)).render(
            sc, cam, bendy.RenderConfig.with_samples(spp), ref)
        torch.cuda.synchronize()
        st = sc.last_stats()
        assert st.segments == gstats.segments and st.launches == 1
        assert torch.equal(ref.data, bufs[i].data), NAMES[i]
        del ref


def test_cli_denoise_inline_equals_library(bendy, tmp_path):
    """--denoise-inline: every call of the progressive loop is a guided call; the screenshot is the denoised mean of the four
    frames, each with the buffer's sample count."""
    import torch
    from test_cli_io import read_png
    w, h, samples, sub, seed = 96, 64, 8, 2, 31
    shot = tmp_path / "inline.png"
    r = subprocess.run([CLI, "--output", "full", "--width", str(w), "--height", str(h), "--samples", str(samples),
                        "--subsample", str(sub), "--screenshot", str(shot), "--scene", scene_path("scene"), "--seed",
                        str(seed), "--denoise-inline", "--quiet"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "denoised with in-pass guides of 8 samples" in r.stderr
    sc, cam = gpu_scene(bendy, "scene", w, h)
    bufs = [bendy.Buffer.new(w, h, bendy.ColorSpace.SRgb) for _ in range(4)]
    tr = bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4))
    while bufs[0].samples < samples:
        tr.render_guided(sc, cam, bendy.RenderConfig.with_samples_subsample(1, bendy.Subsample(sub)), *bufs, seed=seed)
    assert all(buf.samples == samples for buf in bufs)
    den = bendy.denoise(*bufs)
    torch.cuda.synchronize()
    assert np.array_equal(read_png(shot), den.preview())
