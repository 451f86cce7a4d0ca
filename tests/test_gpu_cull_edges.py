"""The fallback and limit branches of the block cull (bt_cull.hpp, fill_empty_block) on the GPU: the
documents of tests/test_cull_edges.py -- scaled, mirrored, nearly and not at all orthogonal camera matrices, very wide
frusta, huge apertures, other clip ranges, 63 - 130 spheres -- through the mask kernel (bit for bit the host's masks)
and through the render kernel (frame AND segment count bit for bit the oracle's, every output, Subsample 0 and 2, a
ragged and a tile-aligned frame).  Then what the shortcut writes for every kind of root material and clip range, bounce
limits 0 and 1, cameras and clip ranges changing in one process, and the rect build's clip-range fallback."""
import json

import numpy as np
import pytest

from sphere_scenes import block_rects, sphere_scene
from test_cull_edges import INSIDE, _aperture_doc, _shear, beside_focus, many_spheres, near_camera

pytestmark = pytest.mark.gpu

FRAMES = [(61, 37), (96, 64)]
WIDE_ASPECT = 16 / 9


def _case(name, make, cfg=None, aspect=None):
    return pytest.param(make, cfg or {}, aspect, id=name)


# one or two documents of every family of test_cull_edges.py (the same builders, seeds from the same ranges, picked on the
# host so that the frame shows spheres and, where the bound holds, a good share of the blocks is empty)
CASES = [
    _case("scale-0.25", lambda: sphere_scene(20000, focus=False, cam_post=np.eye(3) * 0.25)),
    _case("scale-3-f0.1-near", lambda: near_camera(sphere_scene(20105, n_spheres=4, focus=True, fstop=0.1,
                                                                 cam_post=np.eye(3) * 3.0), 20105)),
    _case("scale-3-f0.1-focus-plane", lambda: beside_focus(sphere_scene(20101, n_spheres=4, focus=True, fstop=0.1,
                                                                        cam_post=np.eye(3) * 3.0), 20101, 96, 64)),
    _case("mirror-x", lambda: sphere_scene(21007, n_spheres=4, focus=True, fstop=0.1, cam_post=np.diag([-1.0, 1.0, 1.0]))),
    _case("mirror-y-scale-3", lambda: sphere_scene(21106, focus=False, cam_post=np.diag([3.0, -3.0, 3.0]))),
    _case("gram-inside", lambda: sphere_scene(22009, n_spheres=4, focus=True, fstop=0.1, cam_post=INSIDE)),
    _case("gram-outside", lambda: sphere_scene(23012, focus=False, cam_post=np.diag([1.0, 1.0 + 1e-5, 1.0]))),
    _case("non-uniform", lambda: sphere_scene(24008, focus=True, cam_post=np.diag([1.0, 1.3, 0.8]))),
    _case("shear-0.2", lambda: sphere_scene(24106, focus=False, cam_post=_shear(0.2))),
    _case("wide-0.012", lambda: sphere_scene(25004, focus=True, focal_length=0.012), aspect=WIDE_ASPECT),
    _case("wide-0.006", lambda: sphere_scene(25206, focus=True, focal_length=0.006), aspect=WIDE_ASPECT),
    _case("wide-0.003", lambda: sphere_scene(25506, focus=False, focal_length=0.003), aspect=WIDE_ASPECT),
    _case("wide-0.003-square", lambda: sphere_scene(25608, focus=True, focal_length=0.003), aspect=1.0),
    _case("aperture-0.3", lambda: _aperture_doc(26003, 0.3, n_spheres=4)),
    _case("aperture-0.49", lambda: beside_focus(_aperture_doc(26000, 0.49, n_spheres=4), 26000, 96, 64)),
    _case("aperture-0.51", lambda: _aperture_doc(26008, 0.51, n_spheres=4)),
    _case("aperture-2", lambda: _aperture_doc(26008, 2.0, n_spheres=4)),
    _case("clip_min-0", lambda: sphere_scene(27003, focus=True), cfg=dict(clip_min=0.0)),
    _case("clip_min-negative", lambda: sphere_scene(27506, focus=False), cfg=dict(clip_min=-1.0)),
    _case("clip_max-5", lambda: sphere_scene(27109, focus=False), cfg=dict(clip_max=5.0)),
    _case("clip_min-eq-clip_max", lambda: sphere_scene(27207, focus=True), cfg=dict(clip_min=6.0, clip_max=6.0)),
    _case("63-spheres", lambda: json.dumps(many_spheres(28001, 63, focus=True))),
    _case("64-spheres", lambda: json.dumps(many_spheres(28002, 64, focus=False))),
    _case("65-spheres", lambda: json.dumps(many_spheres(28003, 65, focus=True))),
    _case("130-spheres", lambda: json.dumps(many_spheres(28004, 130, focus=False))),
]


def _gpu(b, txt, w, h, spp=4, n=0, output=0, seed=3, cfg=None, aspect=None, rc_kw=None, handle=None):
    """-> (frame, segments, the handle)"""
    import torch
    gs, cam = handle if handle is not None else (None, None)
    if gs is None:
        gs = b.Scene.from_json(txt)
        cam = gs.find_by_tag("camera")
    gs.set_camera_aspect(cam, aspect if aspect is not None else w / h)
    buf = b.Buffer.new(w, h)
    tr = b.Tracer.with_config(b.Config(output=b.Output(output), **(cfg or {})))
    tr.render(gs, cam, b.RenderConfig(samples=spp, subsample=b.Subsample(n), **(rc_kw or {})), buf, seed=seed, sample_base=0)
    torch.cuda.synchronize()
    return buf.numpy(), gs.last_stats().segments, (gs, cam)


def _oracle(o, txt, w, h, spp=4, n=0, output=0, seed=3, cfg=None, aspect=None, max_bounces=None):
    osc = o.Scene(json.loads(txt))
    ocam = osc.find_by_tag("camera")
    osc.set_camera_aspect(ocam, aspect if aspect is not None else w / h)
    c = o.default_config(samples=spp, subsample_n=n, output=output, recursive=0, sample_base=0)
    for k, v in (cfg or {}).items():
        setattr(c, k, v)
    if max_bounces is not None:
        c.max_bounces = max_bounces
    img, _, seg = o.render(osc, ocam, c, w, h, seed, nthreads=8)
    return img, seg


def _same(b, o, txt, w, h, what, **kw):
    okw = {k: v for k, v in kw.items() if k not in ("rc_kw", "handle")}
    img, seg, handle = _gpu(b, txt, w, h, **kw)
    want, oseg = _oracle(o, txt, w, h, **okw)
    assert seg == oseg, (what, seg, oseg)
    assert np.array_equal(img, want, equal_nan=True), what
    return handle


@pytest.mark.parametrize("make,cfg,aspect", CASES)
def test_device_masks_equal_host_masks(bendy, make, cfg, aspect):
    b = bendy
    txt = make()
    tr = b.Tracer.with_config(b.Config(**cfg))
    for w, h in FRAMES:
        sc = b.Scene.from_json(txt)
        cam = sc.find_by_tag("camera")
        sc.set_camera_aspect(cam, aspect if aspect is not None else w / h)
        for n in (0, 2):
            rc = b.RenderConfig(samples=1, subsample=b.Subsample(n))
            for slices in (1, 4, 32):
                for rank, world in ((0, 1), (0, 3), (1, 3), (2, 3)):
                    host = tr.primary_masks(sc, cam, rc, w, h, slices, rank, world)
                    dev = tr.block_masks_device(sc, cam, rc, w, h, slices, rank, world)
                    assert host.shape == dev.shape and np.array_equal(host, dev), (w, h, n, slices, rank, world)


@pytest.mark.parametrize("make,cfg,aspect", CASES)
def test_frames_bit_exact(bendy, oracle, make, cfg, aspect):
    """Full, Albedo, Normal and Depth of every document, Subsample 0 and 2, a ragged and a tile-aligned frame, 4 spp."""
    txt = make()
    for output in range(4):
        for w, h in FRAMES:
            for n in (0, 2):
                _same(bendy, oracle, txt, w, h, (output, w, h, n), n=n, output=output, cfg=cfg, aspect=aspect)


# ---- what an empty block is filled with ---------------------------------------------------------------------------------
def _one_sphere_doc(root, **kw):
    """A camera at the origin looking down -z and one small sphere far to the left of the view (the document of
    test_gpu_block_masks.py), with a root material of the given kind."""
    doc = json.loads(sphere_scene(4242, n_spheres=1, focus=False, root=root, **kw))
    col = doc["objects"]["collection"]
    for o in col.values():
        t = o["transform"]
        if o["tag"] == "camera":
            m = np.asarray(kw.get("cam_post", np.eye(3)), np.float32)
            for name in ("transform_world", "transform_local"):
                t[name][:9] = [float(v) for v in m.T.reshape(-1)]
                t[name][9:12] = [0.0, 0.0, 0.0]
        else:
            o["inner"]["Sphere"]["radius"] = 0.5
            for name in ("transform_world", "transform_local"):
                t[name][9:12] = [-1.2, 0.0, -6.0]
    return json.dumps(doc)


def _empty_share(b, txt, w, h, cfg=None):
    sc = b.Scene.from_json(txt)
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    m = b.Tracer.with_config(b.Config(**(cfg or {}))).primary_masks(sc, cam, b.RenderConfig.with_samples(1), w, h, 4)
    inside = np.array([bool(r[2] and r[3]) for r in block_rects(w, h, 4)])
    return float((m[inside] == 0).mean())


@pytest.mark.parametrize("root", ["Flat", "Diffuse", "Metallic", "Glass", "Emissive"])
@pytest.mark.parametrize("clips", [{}, dict(clip_min=0.5, clip_max=20.0)], ids=["default-clips", "clips-0.5-20"])
def test_root_materials(bendy, oracle, root, clips):
    """Mostly sky: fill_empty_block writes the larger part of the frame -- root_color, root_albedo and the depth of a
    miss (clip_max with an albedo, infinity for an Emissive root), under both clip ranges."""
    txt = _one_sphere_doc(root)
    w, h = 80, 48
    assert _empty_share(bendy, txt, w, h, clips) > 0.3
    for output in (0, 1, 3):
        _same(bendy, oracle, txt, w, h, (root, output), spp=3, output=output, cfg=clips)
    _same(bendy, oracle, txt, 61, 37, (root, "Subsample(2)"), spp=1, n=2, output=3, cfg=clips)


# ---- bounce limits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [0, 1])
@pytest.mark.parametrize("through", ["Config", "RenderConfig"])
def test_bounce_limits(bendy, oracle, bounces, through):
    """`CULL && max_bounces >= 0`: with 0 and 1 bounces the empty blocks' segment counts and values must still be the
    trace's.  (The ABI field is unsigned: there is no negative limit to pass.)"""
    kw = dict(cfg=dict(max_bounces=bounces)) if through == "Config" else dict(rc_kw=dict(max_bounces=bounces))
    for txt in (sphere_scene(103), _one_sphere_doc("Diffuse")):
        assert 0.1 < _empty_share(bendy, txt, 72, 48) < 1.0
        for output in (0, 3, 1):
            img, seg, _ = _gpu(bendy, txt, 72, 48, output=output, **kw)
            want, oseg = _oracle(oracle, txt, 72, 48, output=output, max_bounces=bounces)
            assert seg == oseg, (through, bounces, output, seg, oseg)
            assert np.array_equal(img, want, equal_nan=True), (through, bounces, output)


# ---- nothing stays behind from the camera or clip range before ----------------------------------------------------------
def test_cameras_in_turn(bendy, oracle):
    """normal -> scaled -> sheared -> normal cameras of one scene in one process (fresh handles: a handle's camera matrix
    cannot change), Full and Depth."""
    w, h = 80, 48
    posts = [("normal", None), ("scaled", np.eye(3) * 3.0), ("sheared", _shear(0.2)), ("normal again", None)]
    shares = []
    for name, post in posts:
        txt = _one_sphere_doc("Emissive", **({} if post is None else dict(cam_post=post)))
        shares.append(_empty_share(bendy, txt, w, h))
        for output in (0, 3):
            _same(bendy, oracle, txt, w, h, (name, output), spp=3, output=output)
    assert shares[0] > 0.3 and shares[1] > 0.3 and shares[2] == 0.0 and shares[3] == shares[0]


def test_clip_ranges_in_turn_on_one_handle(bendy, oracle):
    """default clips -> clip_min = 0 -> a short clip_max -> default, on ONE handle: the masks' key holds clip_min, the
    shortcut's depth value both limits."""
    txt = _one_sphere_doc("Flat")
    w, h = 80, 48
    handle = None
    for cfg in ({}, dict(clip_min=0.0), dict(clip_max=5.0), dict(clip_min=-1.0), {}):
        for output in (0, 3):
            handle = _same(bendy, oracle, txt, w, h, (cfg, output), spp=3, output=output, cfg=cfg, handle=handle)


# ---- the rect build's clip-range fallback (bt_api.cpp fill_launch) ------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(clip_min=0.0), dict(clip_max=2e18)], ids=["clip_min-0", "clip_max-2e18"])
def test_cornell2_outside_the_rect_builds_clip_range(bendy, oracle, cfg):
    """clip_min < 2^-30 or clip_max > 2^60 sends a rect scene to the generic loop: same frame as the oracle's."""
    import torch
    from helpers import gpu_scene, oracle_scene
    w, h, spp = 64, 64, 4
    sc, cam = gpu_scene(bendy, "cornell2", w, h)
    buf = bendy.Buffer.new(w, h)
    bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4, **cfg)).render(sc, cam, bendy.RenderConfig(samples=spp), buf,
                                                                             seed=0x5EED)
    torch.cuda.synchronize()
    osc, ocam = oracle_scene(oracle, "cornell2", w, h)
    c = oracle.default_config(samples=spp, recursive=0)
    for k, v in cfg.items():
        setattr(c, k, v)
    want, _, oseg = oracle.render(osc, ocam, c, w, h, 0x5EED, nthreads=8)
    assert sc.last_stats().segments == oseg
    assert np.array_equal(buf.numpy(), want, equal_nan=True)
