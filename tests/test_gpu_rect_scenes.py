"""The sorted rect path (bt_device.hpp intersect_sorted) and its neighbours on the scenes of rect_scenes.py:
axis-aligned rooms (every orientation of a BtRectAAN row, empty / single / odd / even axis groups, identity cuboids, shared
normals among the BtRectLA rows, general rects) and constructed exact ties.  tests/test_rect_rows.py proves on the CPU that the
scenes hold those rows.  The yardstick is the CPU oracle's iterative form: segment count and every bit of the frame (numerics
contract N1-N8 makes equality the requirement, so no tolerance appears)."""
import json

import numpy as np
import pytest

from rect_scenes import ROOM_SEEDS, TIE_CASES, VOLUME_SEEDS, limit_scene, room_scene, tie_scene

pytestmark = pytest.mark.gpu

SHAPE_SEEDS = (6, 15)          # identity cuboids and six walls; 41 and 56 rows
_oracle_frames = {}


def _scenes(b, o, txt, w, h, tuning=None):
    gs = b.Scene.from_json(txt)
    cam = gs.find_by_tag("camera")
    gs.set_camera_aspect(cam, w / h)
    if tuning:
        gs.set_tuning(**tuning)
    osc = o.Scene(json.loads(txt))
    ocam = osc.find_by_tag("camera")
    osc.set_camera_aspect(ocam, w / h)
    return gs, cam, osc, ocam


def _want(o, osc, ocam, key, w, h, spp, n=0, output=0, seed=0, lens=None, clips=None, threads=8):
    """The oracle's frame and segment count, rendered once per `key` and shared by the tests that need it."""
    key = (key, w, h, spp, n, output, seed)
    if key not in _oracle_frames:
        cfg = o.default_config(samples=spp, subsample_n=n, recursive=0, output=output, lens=lens)
        for k, v in (clips or {}).items():
            setattr(cfg, k, v)
        img, _, seg = o.render(osc, ocam, cfg, w, h, seed, nthreads=threads)
        img.setflags(write=False)
        _oracle_frames[key] = (img, seg)
    return _oracle_frames[key]


def _render(b, gs, cam, w, h, spp, n=0, output=0, seed=0, **cfg):
    import torch
    buf = b.Buffer.new(w, h)
    tr = b.Tracer.with_config(b.Config(chunks_x=8, chunks_y=4, output=b.Output(output), **cfg))
    tr.render(gs, cam, b.RenderConfig(samples=spp, subsample=b.Subsample(n)), buf, seed=seed)
    torch.cuda.synchronize()
    return buf.numpy(), gs.last_stats()


def _same(got, stats, want, seg):
    assert stats.segments == seg
    assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("seed", ROOM_SEEDS)
def test_room_fuzz(bendy, oracle, seed):
    w, h = 72, 48
    output = seed % 4 if seed >= 16 else 0
    spp, n = (1, 2) if 8 <= seed < 16 else (4, 0)          # the reference's interactive pattern on a third of the seeds
    gs, cam, osc, ocam = _scenes(bendy, oracle, room_scene(seed), w, h)
    got, stats = _render(bendy, gs, cam, w, h, spp, n=n, output=output, seed=seed)
    _same(got, stats, *_want(oracle, osc, ocam, ("room", seed), w, h, spp, n=n, output=output, seed=seed))


NAMED = {"tie-%s-%d-%s" % c: (lambda c=c: tie_scene(*c)) for c in TIE_CASES}
NAMED.update({"limit-inf": lambda: limit_scene("inf"), "limit-zero": lambda: limit_scene("zero")})


@pytest.mark.parametrize("case", sorted(NAMED))
def test_named_ties_and_limits(bendy, oracle, case):
    """Exact ties between two plain rects, two cuboids, a cuboid face and a rect, as BtRectAAN rows, as BtRectLA rows of one
    normal, and across the tables (the oracle's frames flip with the order of the two objects: test_rect_rows.py); half
    extents whose squares are +inf and 0."""
    w, h, spp = 72, 48, 4
    gs, cam, osc, ocam = _scenes(bendy, oracle, NAMED[case](), w, h)
    for output in (0, 1, 2):                                # Full, Albedo, Normal
        got, stats = _render(bendy, gs, cam, w, h, spp, output=output, seed=5)
        _same(got, stats, *_want(oracle, osc, ocam, case, w, h, spp, output=output, seed=5))


@pytest.mark.parametrize("seed", VOLUME_SEEDS)
def test_volume_in_a_room(bendy, oracle, seed):
    """A volumetric sphere in the room: the scene leaves the sorted tables for the build with the march, whose generic loop
    then takes the axis-aligned rows (intersect_row) between the marches and, from inside the sphere, during them."""
    w, h, spp = 72, 48, 4
    gs, cam, osc, ocam = _scenes(bendy, oracle, room_scene(seed, volume=True), w, h)
    got, stats = _render(bendy, gs, cam, w, h, spp, seed=seed)
    _same(got, stats, *_want(oracle, osc, ocam, ("volroom", seed), w, h, spp, seed=seed))


LENS = dict(centre=(0.3, 0.6, 0.0), rs=0.1, step=0.1, radius=3.0, max_steps=2000)


@pytest.mark.parametrize("seed", [3, 9, 18])
def test_lens_in_a_room(bendy, oracle, seed):
    w, h, spp = 64, 40, 4
    gs, cam, osc, ocam = _scenes(bendy, oracle, room_scene(seed), w, h)
    gs.set_lens(**LENS)
    got, stats = _render(bendy, gs, cam, w, h, spp, seed=11)
    want, seg = _want(oracle, osc, ocam, ("room-lens", seed), w, h, spp, seed=11, lens=LENS)
    assert stats.lens_steps > 0
    _same(got, stats, want, seg)


@pytest.mark.parametrize("clips", [dict(clip_min=0.0), dict(clip_max=2e18)], ids=["clip_min-0", "clip_max-2e18"])
@pytest.mark.parametrize("seed", [2, 23])
def test_rooms_outside_the_rect_builds_clip_range(bendy, oracle, seed, clips):
    """clip_min < 2^-30 or clip_max > 2^60 (bt_api.cpp fill_launch): the generic loop instead of the sorted tables."""
    w, h, spp = 72, 48, 4
    gs, cam, osc, ocam = _scenes(bendy, oracle, room_scene(seed), w, h)
    got, stats = _render(bendy, gs, cam, w, h, spp, seed=seed, **clips)
    _same(got, stats, *_want(oracle, osc, ocam, ("room-clips", seed, tuple(clips.items())), w, h, spp, seed=seed, clips=clips))


@pytest.mark.parametrize("slices", [1, 4, 32])
@pytest.mark.parametrize("seed", SHAPE_SEEDS)
def test_room_launch_shapes(bendy, oracle, seed, slices):
    w, h, spp = 96, 64, 4
    gs, cam, osc, ocam = _scenes(bendy, oracle, room_scene(seed), w, h, tuning={"slices": slices, "packed": 0})
    got, stats = _render(bendy, gs, cam, w, h, spp, seed=seed)
    assert stats.slices == slices and stats.packed == 0
    _same(got, stats, *_want(oracle, osc, ocam, ("room", seed), w, h, spp, seed=seed))


def _workgroup_slots():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 7      # bt_api.cpp: 7 workgroups per CU for small scene tables


@pytest.mark.parametrize("packed", [1, 2])
@pytest.mark.parametrize("seed", SHAPE_SEEDS)
def test_room_packed_launches(bendy, oracle, seed, packed):
    """The frame of test_gpu_parity.test_packed_launches (3 rays per pixel: rows padded to 4).  packed = 2, the drain that moves
    paths between lanes, is compiled into the rect build only."""
    w, h, spp = 330, 200, 3
    gs, cam, osc, ocam = _scenes(bendy, oracle, room_scene(seed), w, h, tuning={"packed": packed})
    got, stats = _render(bendy, gs, cam, w, h, spp, seed=seed)
    _same(got, stats, *_want(oracle, osc, ocam, ("room", seed), w, h, spp, seed=seed, threads=16))
    blocks = -(-w // 16) * -(-h // 16) * stats.slices
    assert stats.packed == (packed if blocks > _workgroup_slots() else 0)
    if stats.packed:
        assert stats.workgroups == _workgroup_slots()


@pytest.mark.parametrize("seed", [0, 7, 13, 22])
def test_room_guided_equals_four_renders(bendy, oracle, seed):
    """Tracer.render_guided against the four separate renders of the same handle, and the colour against the
    oracle."""
    import torch
    w, h, spp = 72, 48, 4
    gs, cam, osc, ocam = _scenes(bendy, oracle, room_scene(seed), w, h)
    bufs = [bendy.Buffer.new(w, h) for _ in range(4)]
    tr = bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4))
    tr.render_guided(gs, cam, bendy.RenderConfig.with_samples(spp), *bufs, seed=seed)
    torch.cuda.synchronize()
    seg = gs.last_stats().segments
    for output, buf in enumerate(bufs):
        got, stats = _render(bendy, gs, cam, w, h, spp, output=output, seed=seed)
        assert stats.segments == seg and np.array_equal(buf.numpy(), got, equal_nan=True), output
    _same(bufs[0].numpy(), gs.last_stats(), *_want(oracle, osc, ocam, ("room", seed), w, h, spp, seed=seed))
