"""Pixel blocks whose camera rays provably reach no sphere are not traced: frames and segment counts
must stay bit-identical to the oracle's wherever such blocks occur -- random sphere scenes with many empty and many
partial blocks, every output, Subsample(2), progressive calls, shards, ragged frames and pinned block sizes."""
import json

import numpy as np
import pytest

from sphere_scenes import sphere_scene

pytestmark = pytest.mark.gpu


def _gpu(bendy, txt, w, h, spp, n=0, output=0, seed=3, slices=None, sample_base=None, buf=None):
    import torch
    gs = bendy.Scene.from_json(txt)
    cam = gs.find_by_tag("camera")
    gs.set_camera_aspect(cam, w / h)
    if slices:
        gs.set_tuning(slices=slices)
    buf = buf if buf is not None else bendy.Buffer.new(w, h)
    tr = bendy.Tracer.with_config(bendy.Config(output=bendy.Output(output)))
    tr.render(gs, cam, bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n)), buf, seed=seed, sample_base=sample_base)
    torch.cuda.synchronize()
    return buf, gs.last_stats().segments


def _oracle(oracle, txt, w, h, spp, n=0, output=0, seed=3, sample_base=0):
    osc = oracle.Scene(json.loads(txt))
    ocam = osc.find_by_tag("camera")
    osc.set_camera_aspect(ocam, w / h)
    cfg = oracle.default_config(samples=spp, subsample_n=n, output=output, recursive=0, sample_base=sample_base)
    img, _, seg = oracle.render(osc, ocam, cfg, w, h, seed, nthreads=8)
    return img, seg


def _empty_fraction(bendy, txt, w, h, slices):
    gs = bendy.Scene.from_json(txt)
    cam = gs.find_by_tag("camera")
    gs.set_camera_aspect(cam, w / h)
    m = bendy.Tracer().primary_masks(gs, cam, bendy.RenderConfig.with_samples(1), w, h, slices)
    return float((m == 0).mean())


@pytest.mark.parametrize("seed", range(12))
def test_random_sphere_scenes_bit_exact(bendy, oracle, seed):
    txt = sphere_scene(100 + seed)
    w, h = [(72, 48), (61, 37), (96, 40)][seed % 3]
    spp, n = (4, 0) if seed % 4 else (2, 2)
    output = [0, 0, 1, 3, 2, 0][seed % 6]
    slices = [None, 1, 4, 16, 32, None][seed % 6]
    buf, seg = _gpu(bendy, txt, w, h, spp, n=n, output=output, seed=seed, slices=slices)
    it, oseg = _oracle(oracle, txt, w, h, spp, n=n, output=output, seed=seed)
    assert seg == oseg
    assert np.array_equal(buf.numpy(), it, equal_nan=True)


def test_the_random_scenes_have_empty_and_partial_blocks(bendy):
    fr = [_empty_fraction(bendy, sphere_scene(100 + s), 72, 48, 4) for s in range(12)]
    assert sum(0.1 < f < 0.9 for f in fr) >= 6, fr


@pytest.mark.parametrize("output", [0, 1, 2, 3])
def test_outputs_on_scene_json(bendy, oracle, output):
    from helpers import gpu_render, oracle_render
    buf, st, _ = gpu_render(bendy, "scene", 160, 90, 4, output=output)
    it, seg = oracle_render(oracle, "scene", 160, 90, 4, output=output)
    assert st.segments == seg and np.array_equal(buf.numpy(), it)


def test_progressive_calls(bendy, oracle):
    txt = sphere_scene(205, focus=True)
    w, h = 64, 40
    buf = None
    for k in range(3):
        buf, _ = _gpu(bendy, txt, w, h, 2, seed=9, sample_base=2 * k, buf=buf)
    it, _ = _oracle(oracle, txt, w, h, 6, seed=9)
    assert np.array_equal(buf.numpy(), it)


@pytest.mark.parametrize("world", [2])
def test_shards_equal_full_frame(bendy, oracle, world):
    import torch
    txt = sphere_scene(301, focus=False)
    w, h, spp = 70, 45, 4
    gs = bendy.Scene.from_json(txt)
    cam = gs.find_by_tag("camera")
    gs.set_camera_aspect(cam, w / h)
    tr = bendy.Tracer()
    shards = []
    for r in range(world):
        s = bendy.new_shard(w, h, world)
        tr.render_shard(gs, cam, bendy.RenderConfig.with_samples(spp), s, w, h, r, world, seed=5)
        shards.append(s)
    out = bendy.Buffer.new(w, h)
    bendy.unshard(torch.cat(shards), out, world)
    torch.cuda.synchronize()
    it, _ = _oracle(oracle, txt, w, h, spp, seed=5)
    assert np.array_equal(out.numpy(), it)
