"""The per-block sphere masks once they are computed outside the render kernel: the depth-slice
("hourglass") bound that is ANDed with the cone, and the key under which a scene handle keeps a launch's masks.

Runs without a GPU: the masks come from bt_debug_primary_mask (the mask kernel's own function on the host), the key from
bt_debug_mask_key."""
import json
import math
import os

import numpy as np
import pytest

from sphere_scenes import block_rects, camera_of, primary_rays, sphere_hits, sphere_scene, spheres_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "primary_masks_depth_slices.npz")
JIT = [(0.0, 0.0), (0.9999999, 0.9999999), (0.0, 0.9999999), (0.9999999, 0.0), (0.5, 0.5), (0.5, 0.0), (0.0, 0.5)]
RIM = [(0.0, 0.0)] + [(a, 1.0) for a in np.linspace(0, 2 * np.pi, 16, endpoint=False)]
W, H, SLICES = 64, 48, 32          # blocks of 4 x 2 pixels
BLOCK_PX = (28, 20)                # the block under test: pixels [28, 32) x [20, 22)
FOCUS, RADIUS = 6.0, 0.05


def _masks(b, doc, n=0):
    sc = b.Scene.from_json(json.dumps(doc))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, W / H)
    return b.Tracer().primary_masks(sc, cam, b.RenderConfig(samples=1, subsample=b.Subsample(n)), W, H, SLICES)


def _beta(cam, px, py):
    """Where the ray of the frame position (px, py) (pixels, fractional) meets the plane of depth 1, camera space."""
    uu, vv = px * 2.0 / W - 1.0, py * 2.0 / H - 1.0
    y, x = float(cam["xfov"]) * 0.5 * -uu, float(cam["yfov"]) * 0.5 * -vv
    d = np.array([-math.cos(x) * math.sin(y), math.sin(x), -math.cos(x) * math.cos(y)])
    return d[:2] / abs(d[2])


def wide_aperture_doc(depth, lateral_gap, seed=77):
    """f/0.1 (lens radius 0.25) and one sphere of radius 0.05 at the camera-space depth `depth`, beside the rays of the block
    BLOCK_PX: its surface `lateral_gap` away (in +x of the camera) from the circle around the block's patch at that depth
    (the patch of the focus plane, scaled: exact at depth = FOCUS, where the block's rays are narrowest).  Returns the
    document and the lens radius."""
    doc = json.loads(sphere_scene(seed, n_spheres=1, focus=True))
    cam_o = next(o for o in doc["objects"]["collection"].values() if o["tag"] == "camera")
    cam_o["inner"]["Camera"].update({"sensor_size": 0.024, "focal_length": 0.05, "fstop": 0.1, "focus": FOCUS})
    cam = camera_of(doc, W / H)
    m, t = cam["m"].astype(np.float64), cam["t"].astype(np.float64)
    x0, y0 = BLOCK_PX
    # the block's directions: pixel corners plus the half pixel of jitter on either side
    corners = [_beta(cam, x, y) for x in (x0 - 0.5, x0 + 3.5) for y in (y0 - 0.5, y0 + 1.5)]
    centre = _beta(cam, x0 + 1.5, y0 + 0.5)
    circle = max(float(np.linalg.norm(c - centre)) for c in corners)
    lat = centre * depth + np.array([1.0, 0.0]) * (circle * depth + RADIUS + lateral_gap)
    c = t + m @ np.array([lat[0], lat[1], -depth])
    s = next(o for o in doc["objects"]["collection"].values() if "Sphere" in o["inner"])
    s["transform"]["transform_world"][9:12] = [float(v) for v in c.astype(np.float32)]
    s["transform"]["transform_local"][9:12] = s["transform"]["transform_world"][9:12]
    s["inner"]["Sphere"]["radius"] = RADIUS
    return doc, float(cam["aperture"])


def _block_index():
    rects = block_rects(W, H, SLICES)
    return next(i for i, r in enumerate(rects) if (r[0], r[1]) == BLOCK_PX)


def _brute(doc, masks, n=0):
    """Dense float32 camera rays (aperture rim, jitter corners): (a culled row is never hit, the blocks that are hit)."""
    cam, rows = camera_of(doc, W / H), spheres_of(doc)
    hit_blocks = set()
    for bi, (m, (x0, y0, nx, ny)) in enumerate(zip(masks, block_rects(W, H, SLICES))):
        if nx == 0 or ny == 0:
            continue
        ys, xs = np.mgrid[y0:y0 + ny, x0:x0 + nx]
        O, D = primary_rays(cam, W, H, xs.ravel(), ys.ravel(), n, JIT, RIM)
        hit = sphere_hits(O, D, rows).any(axis=0)
        for i in np.nonzero(hit)[0]:
            assert (int(m) >> int(i)) & 1, ("a culled row is hit", (x0, y0), int(i))
            hit_blocks.add(bi)
    return hit_blocks


# The same documents' masks under the cone alone (the bound before the depth slices), recorded with the library built
# with -DBT_NO_DEPTH_SLICES: wide_aperture_doc(FOCUS, 0.3 * lens radius) and wide_aperture_doc(FOCUS, -0.02).
def test_depth_slice_sharpness(bendy):
    """Near the focus distance the block's rays pass through a patch no wider than the block itself, the lens radius
    notwithstanding.  A sphere 0.3 lens radii beside that patch lies inside the block's cone (the golden masks of the
    cone keep it) and outside its hourglass: culled now.  Moved to overlap the patch it is kept, and is in fact hit."""
    b = bendy
    g = np.load(GOLDEN)
    bi = _block_index()
    doc, lens = wide_aperture_doc(FOCUS, 0.0)
    assert abs(lens - 0.25) < 1e-6
    beside, _ = wide_aperture_doc(FOCUS, 0.3 * lens)
    m = _masks(b, beside)
    assert m.shape == g["beside"].shape
    assert not (m & ~g["beside"]).any()                 # only shrinks
    assert int(g["beside"][bi]) & 1                     # the cone kept the sphere for this block ...
    assert not int(m[bi]) & 1                           # ... the depth slices cull it
    assert (m == 0).sum() > (g["beside"] == 0).sum()
    _brute(beside, m)
    touching, _ = wide_aperture_doc(FOCUS, -0.02)
    m = _masks(b, touching)
    assert not (m & ~g["touching"]).any()
    assert int(m[bi]) & 1
    assert bi in _brute(touching, m)                    # and rays of the block do hit it


@pytest.mark.parametrize("depth,n", [(0.4, 0), (2.0, 0), (4.5, 0), (5.7, 0), (6.0, 0), (6.3, 0), (8.0, 0), (14.0, 0),
                                     (2.0, 2), (5.7, 2), (6.3, 2), (14.0, 2), (6.0, 3)])
def test_depth_slices_rim_rays(bendy, depth, n):
    """Spheres beside the block's rays at depths in front of, at and behind the focus distance, gaps from overlapping to
    a lens radius away: rays from the rim of the wide aperture never hit a culled row."""
    b = bendy
    culled = 0
    for gap in (-0.04, 0.01, 0.05, 0.3):
        doc, _ = wide_aperture_doc(depth, gap, seed=77 + n)
        m = _masks(b, doc, n)
        _brute(doc, m, n)
        culled += int((m == 0).sum())
    assert culled > 0


def test_c3_empty_block_share(bendy):
    """0.5749 was recorded for the first build of this bound (profiles/r09b/attempts.json); the cone alone: 0.5445."""
    b = bendy
    sc = b.Scene.load(os.path.join(ROOT, "scenes", "scene.json.gz"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, 1920 / 1080)
    masks = b.Tracer().primary_masks(sc, cam, b.RenderConfig.with_samples(64), 1920, 1080, 4)
    inside = np.array([bool(r[2] and r[3]) for r in block_rects(1920, 1080, 4)])
    frac = float((masks[inside] == 0).mean())
    print(f"C3: {frac:.4f} of the blocks empty")
    assert frac >= 0.57


# ---- the key under which a handle keeps a launch's masks ------------------------------------------------------------------
def _key(b, doc, w=W, h=H, slices=4, n=0, rank=0, world=1, samples=4, config=None, aspect=None):
    sc = b.Scene.from_json(json.dumps(doc))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, aspect if aspect is not None else w / h)
    tr = b.Tracer.with_config(config) if config is not None else b.Tracer()
    return tr.mask_key(sc, cam, b.RenderConfig(samples=samples, subsample=b.Subsample(n)), w, h, slices, rank, world)


def _base_doc():
    return json.loads(sphere_scene(4711, n_spheres=3, focus=True))


def _cam(doc):
    return next(o for o in doc["objects"]["collection"].values() if o["tag"] == "camera")


def test_key_ignores_what_the_masks_do_not_depend_on(bendy):
    b = bendy
    doc = _base_doc()
    k = _key(b, doc)
    assert k == _key(b, doc)
    assert k == _key(b, doc, samples=64)                 # the launches of one deep render share their masks
    assert k == _key(b, doc, config=b.Config(max_bounces=3, clip_max=50.0))


def test_key_completeness(bendy):
    """Changing any one input of the masks changes the key."""
    b = bendy
    base = _base_doc()
    k = _key(b, base)
    variants = {}

    def doc_with(change):
        d = json.loads(json.dumps(base))
        change(d)
        return d

    def cam_world(i, v):
        def f(d):
            for name in ("transform_world", "transform_local"):
                _cam(d)["transform"][name][i] = v
        return f

    tw = _cam(base)["transform"]["transform_world"]
    variants["camera moved"] = _key(b, doc_with(cam_world(9, tw[9] + 0.5)))
    variants["camera moved in y"] = _key(b, doc_with(cam_world(10, tw[10] + 0.5)))
    variants["camera moved in z"] = _key(b, doc_with(cam_world(11, tw[11] + 0.5)))
    for i in range(9):
        variants[f"camera matrix [{i}]"] = _key(b, doc_with(cam_world(i, tw[i] + 1e-3)))
    variants["fov"] = _key(b, doc_with(lambda d: _cam(d)["inner"]["Camera"].update(focal_length=0.031)))
    variants["aspect"] = _key(b, base, aspect=1.0)
    variants["focus"] = _key(b, doc_with(lambda d: _cam(d)["inner"]["Camera"].update(focus=4.25)))
    variants["no focus"] = _key(b, doc_with(lambda d: _cam(d)["inner"]["Camera"].update(focus=None)))
    variants["aperture"] = _key(b, doc_with(lambda d: _cam(d)["inner"]["Camera"].update(fstop=0.7)))
    variants["Subsample(2)"] = _key(b, base, n=2)
    variants["Subsample(3)"] = _key(b, base, n=3)
    variants["width"] = _key(b, base, w=W + 16, aspect=W / H)
    variants["width, same tiles"] = _key(b, base, w=W - 3, aspect=W / H)
    variants["height"] = _key(b, base, h=H + 16, aspect=W / H)
    variants["height, same tiles"] = _key(b, base, h=H - 3, aspect=W / H)
    variants["slices"] = _key(b, base, slices=8)
    variants["world 2"] = _key(b, base, rank=0, world=2)
    variants["rank 1 of 2"] = _key(b, base, rank=1, world=2)
    variants["world 3"] = _key(b, base, rank=1, world=3)
    variants["clip_min"] = _key(b, base, config=b.Config(clip_min=0.02))
    variants["sphere added"] = _key(b, json.loads(sphere_scene(4711, n_spheres=4, focus=True)))
    assert variants["rank 1 of 2"] != variants["world 2"] and variants["world 3"] != variants["rank 1 of 2"]
    assert variants["Subsample(2)"] != variants["Subsample(3)"]
    for what, kk in variants.items():
        assert len(kk) == len(k) and kk != k, what

    # the rows themselves: one handle, a sphere moved / resized in place
    sc = b.Scene.from_json(json.dumps(base))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, W / H)
    tr, rc = b.Tracer(), b.RenderConfig(samples=4)
    k0 = tr.mask_key(sc, cam, rc, W, H, 4)
    assert k0 == tr.mask_key(sc, cam, rc, W, H, 4)
    sphere = next(int(key) for key, o in base["objects"]["collection"].items() if "Sphere" in o["inner"])
    sc.debug_set_object(sphere, [0.25, -1.0, 2.0])
    k1 = tr.mask_key(sc, cam, rc, W, H, 4)
    assert k1 != k0
    sc.debug_set_object(sphere, None, 0.77)
    k2 = tr.mask_key(sc, cam, rc, W, H, 4)
    assert k2 != k1 and k2 != k0
    # ... and the masks follow
    m1 = tr.primary_masks(sc, cam, rc, W, H, 4)
    sc.debug_set_object(sphere, [40.0, 40.0, 40.0])
    assert tr.mask_key(sc, cam, rc, W, H, 4) != k2
    assert (tr.primary_masks(sc, cam, rc, W, H, 4) != m1).any() or not m1.any()
