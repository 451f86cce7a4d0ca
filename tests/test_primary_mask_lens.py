"""The per-block sphere masks with the lens radius the camera event really has.  The masks must only
shrink against the earlier bound (recorded in tests/golden/primary_masks_cone.npz), and dense float32 camera rays --
from the rim of the aperture above all, next to spheres placed just off a block's patch of the focus plane -- must never
hit a culled row."""
import json
import math
import os

import numpy as np
import pytest

from sphere_scenes import block_rects, camera_of, primary_rays, sphere_hits, sphere_scene, spheres_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "primary_masks_cone.npz")
JIT = [(0.0, 0.0), (0.9999999, 0.9999999), (0.0, 0.9999999), (0.9999999, 0.0), (0.5, 0.5), (0.5, 0.0), (0.0, 0.5)]
# the aperture's rim (radius 1 >= every r2 the kernel draws) at 16 angles, and its centre
RIM = [(0.0, 0.0)] + [(a, 1.0) for a in np.linspace(0, 2 * np.pi, 16, endpoint=False)]
SIZES = [(40, 24), (37, 29), (48, 33), (23, 17)]


def _masks(b, txt, w, h, slices, n=0, rank=0, world=1):
    sc = b.Scene.from_json(txt)
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    rc = b.RenderConfig(samples=1, subsample=b.Subsample(n))
    return b.Tracer().primary_masks(sc, cam, rc, w, h, slices, rank, world)


def _c3_masks(b):
    sc = b.Scene.load(os.path.join(ROOT, "scenes", "scene.json.gz"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, 1920 / 1080)
    return b.Tracer().primary_masks(sc, cam, b.RenderConfig.with_samples(64), 1920, 1080, 4)


def _brute(doc, masks, w, h, slices, n):
    """No culled row of any block is hit by the block's camera rays; returns the number of culled (block, row) pairs."""
    cam, rows = camera_of(doc, w / h), spheres_of(doc)
    culled_pairs = 0
    for m, (x0, y0, nx, ny) in zip(masks, block_rects(w, h, slices)):
        if nx == 0 or ny == 0:
            continue
        culled = [i for i in range(len(rows)) if not (int(m) >> i) & 1]
        if not culled:
            continue
        culled_pairs += len(culled)
        ys, xs = np.mgrid[y0:y0 + ny, x0:x0 + nx]
        O, D = primary_rays(cam, w, h, xs.ravel(), ys.ravel(), n, JIT, RIM)
        hit = sphere_hits(O, D, rows[culled])
        assert not hit.any(), ((x0, y0, nx, ny), [culled[i] for i in np.nonzero(hit.any(axis=0))[0]])
    return culled_pairs


def test_masks_only_shrink(bendy):
    """Every bit the new bound sets, the earlier one set too: C3 and 48 random scenes (focus on and off, Subsample 1 /
    2 / 3, every block size)."""
    b = bendy
    g = np.load(GOLDEN)
    new = _c3_masks(b)
    assert new.shape == g["c3_s4"].shape
    assert not (new & ~g["c3_s4"]).any()
    fewer = 0
    for k in range(48):
        w, h = SIZES[k % 4]
        slices, n = [1, 2, 4, 8, 16, 32][k % 6], [0, 2, 3][k % 3]
        m = _masks(b, sphere_scene(9000 + k, focus=bool(k & 1)), w, h, slices, n)
        old = g[f"rand_{k}"]
        assert m.shape == old.shape
        assert not (m & ~old).any(), k
        fewer += int((m != old).sum())
    assert fewer > 0                     # the lens bound is tighter somewhere


def test_c3_empty_blocks(bendy):
    """The cone with the true lens radius empties 54.45 % of C3's blocks (50.4 % with twice the radius).  The depth-slice
    bound that would reach 57 % is not part of this bound ("Not kept")."""
    b = bendy
    masks = _c3_masks(b)
    inside = np.array([bool(r[2] and r[3]) for r in block_rects(1920, 1080, 4)])
    frac = float((masks[inside] == 0).mean())
    print(f"C3: {frac:.4f} of the blocks empty")
    assert frac >= 0.544


def _near_focus_doc(seed, side, gap, radius):
    """A camera with focus and one sphere whose centre sits beside the focus point of pixel (x, y) = (13, 9) of a 32x24
    frame: `gap` (a fraction of the radius) off the sphere's surface in the image-plane direction `side`."""
    doc = json.loads(sphere_scene(seed, n_spheres=1, focus=True))
    cam = camera_of(doc, 32 / 24)
    m, t = cam["m"].astype(np.float64), cam["t"].astype(np.float64)
    uu, vv = 13 * 2.0 / 32 - 1.0, 9 * 2.0 / 24 - 1.0
    y, x = float(cam["xfov"]) * 0.5 * -uu, float(cam["yfov"]) * 0.5 * -vv
    d_cam = np.array([-math.cos(x) * math.sin(y), math.sin(x), -math.cos(x) * math.cos(y)])
    p = d_cam * float(cam["focus"]) / abs(d_cam[2])                        # the pixel's point in the focus plane
    off = np.array([math.cos(side), math.sin(side), 0.0]) * radius * (1.0 + gap)
    c = t + m @ (p + off)
    s = doc["objects"]["collection"]["1"]
    s["transform"]["transform_world"][9:12] = [float(v) for v in c.astype(np.float32)]
    s["inner"]["Sphere"]["radius"] = radius
    return doc


@pytest.mark.parametrize("slices", [1, 2, 4, 8, 16, 32])
def test_spheres_beside_the_focus_plane(bendy, slices):
    """Small spheres just off a block's patch of the focus plane, where the rays of the block are narrowest: rays from
    the aperture's rim, every jitter corner, Subsample 1 / 2 / 3."""
    b = bendy
    culled = 0
    for k in range(12):
        side = 2 * math.pi * k / 12
        for gap in (0.02, 0.2, 1.0):
            doc = _near_focus_doc(300 + k, side, gap, [0.05, 0.2, 0.6][k % 3])
            n = [0, 2, 3][k % 3]
            masks = _masks(b, json.dumps(doc), 32, 24, slices, n)
            culled += _brute(doc, masks, 32, 24, slices, n)
    assert culled > 0


@pytest.mark.parametrize("focus", [False, True])
def test_random_scenes_rim_rays(bendy, focus):
    """Random scenes with rays from the aperture's rim, focus on and off, every block size, Subsample 1 / 2 / 3."""
    b = bendy
    culled = 0
    for k in range(18):
        w, h = SIZES[k % 4]
        slices, n = [1, 2, 4, 8, 16, 32][k % 6], [0, 2, 3][(k // 6) % 3]
        txt = sphere_scene(12000 + k, focus=focus)
        culled += _brute(json.loads(txt), _masks(b, txt, w, h, slices, n), w, h, slices, n)
    assert culled > 0


def _wide_aperture_doc(seed, n_spheres):
    """f/0.1 (aperture 0.1 - 0.3: the lens radius dominates every other margin of the bound) and small spheres close to
    the camera, where the block's rays still fan out over the whole lens disc: in front of the lens, beside it and just
    outside the fan of a pixel's rays."""
    rng = np.random.default_rng(seed)
    doc = json.loads(sphere_scene(seed, n_spheres=n_spheres, focus=True))
    cam_o = next(o for o in doc["objects"]["collection"].values() if o["tag"] == "camera")
    cam_o["inner"]["Camera"]["fstop"] = 0.1
    cam = camera_of(doc, 1.5)
    m, t = cam["m"].astype(np.float64), cam["t"].astype(np.float64)
    for k in range(1, n_spheres + 1):
        s = doc["objects"]["collection"][str(k)]
        depth = rng.uniform(0.15, 3.0)
        lateral = rng.uniform(-0.8, 0.8, 2) * depth * 0.6 + rng.uniform(-0.35, 0.35, 2)
        c = t + m @ np.array([lateral[0], lateral[1], -depth])
        s["transform"]["transform_world"][9:12] = [float(v) for v in c.astype(np.float32)]
        s["inner"]["Sphere"]["radius"] = float(rng.uniform(0.02, 0.25))
    return doc


@pytest.mark.parametrize("slices", [1, 4, 16, 32])
def test_wide_aperture_near_spheres(bendy, slices):
    """A lens radius bound that is too small culls rows that rays from the rim of a wide aperture do hit: these scenes
    catch that (a lens radius of 0, or half the true one, fails here), and every culled row must stay unhit."""
    b = bendy
    culled = 0
    for k in range(24):
        w, h = SIZES[k % 4]
        n = [0, 2, 3][k % 3]
        doc = _wide_aperture_doc(500 + 40 * slices + k, 4)
        masks = _masks(b, json.dumps(doc), w, h, slices, n)
        culled += _brute(doc, masks, w, h, slices, n)
    assert culled > 0
