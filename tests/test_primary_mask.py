"""The per-block sphere masks of the sphere-only build, on the host: bt_debug_primary_mask runs the
kernel's own mask code (bt_cull.hpp).  A cleared bit is a promise that no camera ray of the block makes that sphere row
pass the kernel's intersection test; dense float32 camera rays, brute-forced against every sphere, must never break it."""
import json
import os

import numpy as np
import pytest

from sphere_scenes import block_rects, camera_of, primary_rays, sphere_hits, sphere_scene, spheres_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JIT = [(0.0, 0.0), (0.9999999, 0.9999999), (0.0, 0.9999999), (0.9999999, 0.0), (0.5, 0.5)]
DISK = [(0.0, 0.0)] + [(a, 1.0) for a in np.linspace(0, 2 * np.pi, 8, endpoint=False)]


def _masks(b, doc_txt, w, h, slices, n=0, rank=0, world=1):
    sc = b.Scene.from_json(doc_txt)
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    rc = b.RenderConfig(samples=1, subsample=b.Subsample(n))
    return b.Tracer().primary_masks(sc, cam, rc, w, h, slices, rank, world)


def _check_scene(b, seed, w, h, slices, n, rank=0, world=1, focus=None):
    txt = sphere_scene(seed, focus=focus)
    doc = json.loads(txt)
    masks = _masks(b, txt, w, h, slices, n, rank, world)
    cam, rows = camera_of(doc, w / h), spheres_of(doc)
    rects = block_rects(w, h, slices, rank, world)
    assert len(masks) == len(rects)
    empty = 0
    for m, (x0, y0, nx, ny) in zip(masks, rects):
        if nx == 0 or ny == 0:
            assert m == 0
            continue
        m = int(m)
        empty += m == 0
        culled = [i for i in range(len(rows)) if not (m >> i) & 1]
        if not culled:
            continue
        ys, xs = np.mgrid[y0:y0 + ny, x0:x0 + nx]
        O, D = primary_rays(cam, w, h, xs.ravel(), ys.ravel(), n, JIT, DISK)
        hit = sphere_hits(O, D, rows[culled])
        assert not hit.any(), (seed, (x0, y0, nx, ny), [culled[i] for i in np.nonzero(hit.any(axis=0))[0]])
    return empty, sum(1 for r in rects if r[2] and r[3])


@pytest.mark.parametrize("chunk", range(8))
def test_no_culled_sphere_is_ever_hit(bendy, chunk):
    """Random sphere scenes and cameras, focus on and off, Subsample 1 / 2 / 3, every block size, ragged frames."""
    sizes = [(40, 24), (37, 29), (48, 33), (23, 17)]
    empty = total = 0
    for k in range(40):
        seed = chunk * 1000 + k
        w, h = sizes[k % len(sizes)]
        slices = [1, 2, 4, 8, 16, 32][(k + chunk) % 6]
        n = [0, 2, 3][k % 3]
        e, t = _check_scene(bendy, seed, w, h, slices, n, focus=bool(k & 1))
        empty += e
        total += t
    assert 0 < empty < total            # the check is not vacuous: some blocks are culled whole, others are not


@pytest.mark.parametrize("world", [2, 3])
def test_shard_blocks(bendy, world):
    for k in range(12):
        for rank in range(world):
            _check_scene(bendy, 7000 + k, 56, 40, [4, 8, 16][k % 3], 0, rank=rank, world=world, focus=bool(k & 1))


def test_spheres_on_block_silhouettes(bendy):
    """A sphere whose silhouette runs through the frame, moved in tiny steps: every position must hold."""
    base = json.loads(sphere_scene(11, n_spheres=1, focus=False))
    cam = camera_of(base, 1.5)
    fwd = -cam["m"][:, 2]
    for k, off in enumerate(np.linspace(-1.0, 1.0, 41)):
        doc = json.loads(json.dumps(base))
        s = doc["objects"]["collection"]["1"]
        c = cam["t"] + fwd * 6 + cam["m"][:, 0] * (1.3 + off * 0.05) + cam["m"][:, 1] * off * 0.02
        s["transform"]["transform_world"][9:12] = [float(v) for v in c]
        s["inner"]["Sphere"]["radius"] = 0.5
        txt = json.dumps(doc)
        masks = _masks(bendy, txt, 48, 32, 4)
        rows, rects = spheres_of(doc), block_rects(48, 32, 4)
        for m, (x0, y0, nx, ny) in zip(masks, rects):
            if nx and ny and not int(m) & 1:
                ys, xs = np.mgrid[y0:y0 + ny, x0:x0 + nx]
                O, D = primary_rays(cam, 48, 32, xs.ravel(), ys.ravel(), 0, JIT, DISK)
                assert not sphere_hits(O, D, rows).any(), (k, x0, y0)


def test_sphere_around_the_camera_is_never_culled(bendy):
    for focus in (False, True):
        doc = json.loads(sphere_scene(5, n_spheres=1, focus=focus))
        cam = camera_of(doc, 1.5)
        s = doc["objects"]["collection"]["1"]
        s["transform"]["transform_world"][9:12] = [float(v) for v in cam["t"] + np.float32(0.01)]
        s["inner"]["Sphere"]["radius"] = 0.05
        masks = _masks(bendy, json.dumps(doc), 32, 32, 4)
        assert (masks == 1).all()


def test_c3_mask_statistics(bendy):
    """scene.json at 1920x1080 (C3, 64-pixel blocks): the light sphere is never in view; print what is culled."""
    sc = bendy.Scene.load(os.path.join(ROOT, "scenes", "scene.json.gz"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, 1920 / 1080)
    masks = bendy.Tracer().primary_masks(sc, cam, bendy.RenderConfig.with_samples(64), 1920, 1080, 4)
    rects = block_rects(1920, 1080, 4)
    inside = np.array([bool(r[2] and r[3]) for r in rects])
    m = masks[inside]
    pop = np.array([bin(int(v)).count("1") for v in m])
    frac = float((m == 0).mean())
    print(f"C3: {inside.sum()} blocks, {frac:.3f} empty, mean popcount of the others {pop[m != 0].mean():.2f}")
    assert 0.45 < frac < 0.65
    assert not (np.bitwise_or.reduce(m) >> 2) & 1              # row 2: the light at (6, 10, 0)


def test_mask_of_non_sphere_scenes_is_all_ones(bendy):
    sc = bendy.Scene.load(os.path.join(ROOT, "scenes", "cornell.json.gz"))
    cam = sc.find_by_tag("camera")
    masks = bendy.Tracer().primary_masks(sc, cam, bendy.RenderConfig.with_samples(1), 64, 64, 4)
    assert (masks == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
