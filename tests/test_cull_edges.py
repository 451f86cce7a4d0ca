"""The fallback and limit branches of the per-block sphere masks (bt_cull.hpp), on the host: cameras
whose matrix is a scaled, mirrored, nearly or not at all orthogonal one, very wide frusta, huge apertures, other clip
ranges and sphere counts around the 64 bits of a mask.

The masks come from Tracer.primary_masks (the mask kernel's own function).  The check is the brute force of
test_primary_mask.py / test_block_mask_cache.py: float32 camera rays at 7 jitter points x 17 aperture points x every
sub-pixel cell of every pixel, through sphere_hits; NO RAY OF A BLOCK HITS A SPHERE ROW WHOSE BIT IS CLEAR IN THAT BLOCK'S
MASK.  Where the bound is expected to hold a family must show empty and partial masks, where a fallback is expected every
in-frame block keeps every row while the same document with the offending parameter put back has empty masks: so that
neither a bound that silently became wrong nor one that silently gave up passes."""
import hashlib
import itertools
import json
import math
import os

import numpy as np
import pytest

from sphere_scenes import block_rects, camera_of, primary_rays, sphere_hits, sphere_scene, spheres_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGESTS = os.path.join(ROOT, "tests", "golden", "sphere_scene_digests.json")
JIT = [(0.0, 0.0), (0.9999999, 0.9999999), (0.0, 0.9999999), (0.9999999, 0.0), (0.5, 0.5), (0.5, 0.0), (0.0, 0.5)]
RIM = [(0.0, 0.0)] + [(a, 1.0) for a in np.linspace(0, 2 * np.pi, 16, endpoint=False)]
SIZES = [(40, 24), (37, 29), (48, 33), (23, 17)]
# slices x Subsample x focus: every family runs the whole product, each combination with a seed of its own
COMBOS = list(itertools.product([1, 4, 16, 32], [0, 2], [False, True]))
ALL64 = (1 << 64) - 1


# ---- the scene helper's old calls give the old text ---------------------------------------------------------------------
def existing_calls():
    """(seed, n_spheres, focus) of every sphere_scene() call the suite made before the helper grew its optional
    arguments (search tests/ for `sphere_scene(`)."""
    calls = []
    for c in range(8):                                   # test_primary_mask.py
        calls += [(1000 * c + k, None, bool(k & 1)) for k in range(40)]
    calls += [(7000 + k, None, bool(k & 1)) for k in range(12)]
    calls += [(11, 1, False), (5, 1, False), (5, 1, True)]
    calls += [(77, 1, True), (79, 1, True), (80, 1, True), (4711, 3, True), (4711, 4, True)]     # test_block_mask_cache.py
    calls += [(9000 + k, None, bool(k & 1)) for k in range(48)]                                  # test_primary_mask_lens.py
    calls += [(300 + k, 1, True) for k in range(12)]
    calls += [(12000 + k, None, f) for k in range(18) for f in (False, True)]
    calls += [(500 + 40 * s + k, 4, True) for s in (1, 4, 16, 32) for k in range(24)]
    calls += [(4242, 1, False)]                                                                  # test_gpu_block_masks.py
    calls += [(100 + s, None, None) for s in range(12)] + [(205, None, True), (301, None, False)]  # test_gpu_empty_blocks.py
    return calls


def call_name(seed, n, focus):
    return f"{seed}|{n}|{focus}"


def test_sphere_scene_is_unchanged_for_existing_calls():
    with open(DIGESTS) as f:
        want = json.load(f)
    calls = existing_calls()
    assert len(set(calls)) == len(want) == 535
    for seed, n, focus in calls:
        got = hashlib.sha256(sphere_scene(seed, n_spheres=n, focus=focus).encode()).hexdigest()
        assert got == want[call_name(seed, n, focus)], (seed, n, focus)
    # the optional arguments move no sphere: the draws keep their number and order
    for seed in (3, 4711):
        base = spheres_of(json.loads(sphere_scene(seed, n_spheres=5, focus=True)))
        edge = sphere_scene(seed, n_spheres=5, focus=True, cam_post=np.diag([1.0, 1.3, 0.8]), focal_length=0.006, fstop=0.1,
                            focus_dist=2.0, root="Glass")
        assert np.array_equal(spheres_of(json.loads(edge)), base)
        assert json.loads(edge)["root_material"] == 10 and json.loads(sphere_scene(seed))["root_material"] == 1


def test_placement_of_many_spheres():
    """130 spheres: in front of the camera inside and beside the view, behind it and around it."""
    doc = json.loads(sphere_scene(31, n_spheres=130, focus=False))
    cam, rows = camera_of(doc, 1.5), spheres_of(doc)
    assert len(rows) == 130
    v = (rows[:, :3] - cam["t"]).astype(np.float64) @ cam["m"].astype(np.float64)          # camera space
    depth, lat = -v[:, 2], np.abs(v[:, 0]) / np.maximum(-v[:, 2], 1e-9)
    tan_x = math.tan(float(cam["xfov"]) / 2)
    r = np.sqrt(rows[:, 3])
    assert ((depth > 1) & (lat < tan_x)).sum() >= 10          # in front, inside the view
    assert ((depth > 1) & (lat > tan_x)).sum() >= 10          # in front, beside it
    assert (depth < -r).sum() >= 10                           # wholly behind the camera
    assert (np.linalg.norm(v, axis=1) < r).sum() >= 3         # around it


# ---- masks, rays, the check ---------------------------------------------------------------------------------------------
def _masks(b, txt, w, h, slices, n=0, config=None, aspect=None):
    sc = b.Scene.from_json(txt)
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, aspect if aspect is not None else w / h)
    tr = b.Tracer.with_config(config) if config is not None else b.Tracer()
    return tr.primary_masks(sc, cam, b.RenderConfig(samples=1, subsample=b.Subsample(n)), w, h, slices)


def _key(b, txt, w, h, slices, n=0, config=None, aspect=None):
    sc = b.Scene.from_json(txt)
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, aspect if aspect is not None else w / h)
    tr = b.Tracer.with_config(config) if config is not None else b.Tracer()
    return tr.mask_key(sc, cam, b.RenderConfig(samples=1, subsample=b.Subsample(n)), w, h, slices)


class Tally:
    """What a family's masks looked like (in-frame blocks only)."""

    def __init__(self):
        self.blocks = self.empty = self.partial = 0

    def add(self, masks, rects, n_rows):
        for m, (_, _, nx, ny) in zip(masks, rects):
            if nx == 0 or ny == 0:
                continue
            m = int(m)
            self.blocks += 1
            self.empty += m == 0
            self.partial += 0 < bin(m).count("1") < min(n_rows, 64)


def brute(txt, masks, w, h, slices, n, aspect=None, tmin=np.float32(0.01), tmax=np.float32(1000.0), what=None):
    """No ray of a block hits a row whose bit is clear in the block's mask.  The frame's rays are made once, in pixel
    chunks; `hit[p, i]`: some ray of pixel p hits row i."""
    doc = json.loads(txt)
    cam, rows = camera_of(doc, aspect if aspect is not None else w / h), spheres_of(doc)
    rects = block_rects(w, h, slices)
    assert len(masks) == len(rects)
    n_bits = min(len(rows), 64)
    full = ALL64 if len(rows) > 64 else (1 << n_bits) - 1
    if all(int(m) == full for m, r in zip(masks, rects) if r[2] and r[3]):
        for m, r in zip(masks, rects):
            assert r[2] and r[3] or int(m) == 0
        return rects                                       # nothing is culled anywhere: nothing to break
    hit = np.zeros((h * w, n_bits), bool)
    step = max(1, 400000 // (len(JIT) * len(RIM) * max(n, 1) ** 2))
    for p0 in range(0, h * w, step):
        p = np.arange(p0, min(h * w, p0 + step))
        O, D = primary_rays(cam, w, h, p % w, p // w, n, JIT, RIM)
        hits = sphere_hits(O, D, rows[:n_bits], tmin=tmin, tmax=tmax)
        hit[p] = hits.reshape(-1, len(p), n_bits).any(axis=0)
    hit = hit.reshape(h, w, n_bits)
    for m, (x0, y0, nx, ny) in zip(masks, rects):
        if nx == 0 or ny == 0:
            assert int(m) == 0
            continue
        rows_hit = np.nonzero(hit[y0:y0 + ny, x0:x0 + nx].any(axis=(0, 1)))[0]
        bad = [int(i) for i in rows_hit if not (int(m) >> int(i)) & 1]
        assert not bad, ("a culled row is hit", what, (x0, y0, nx, ny), bad)
    return rects


def _cam_obj(doc):
    return next(o for o in doc["objects"]["collection"].values() if o["tag"] == "camera")


def near_camera(txt, seed, aspect=1.5):
    """The document's spheres made small and moved close to the camera, where a block's rays still fan out over the whole
    lens disc: in front of the lens, beside it and just outside the fan (as test_primary_mask_lens._wide_aperture_doc,
    with the lateral spread in units of the lens radius the scaled camera matrix really gives)."""
    rng = np.random.default_rng([seed, 1])
    doc = json.loads(txt)
    cam = camera_of(doc, aspect)
    m, t = cam["m"].astype(np.float64), cam["t"].astype(np.float64)
    scale = np.linalg.norm(m, axis=0).mean()
    axes = m / np.linalg.norm(m, axis=0)
    lens = float(cam["aperture"]) * scale
    for o in doc["objects"]["collection"].values():
        if "Sphere" not in o["inner"]:
            continue
        depth = rng.uniform(0.15, 3.0)
        lateral = rng.uniform(-0.8, 0.8, 2) * depth * 0.6 + rng.uniform(-1.4, 1.4, 2) * lens
        c = t + axes @ np.array([lateral[0], lateral[1], -depth])
        for name in ("transform_world", "transform_local"):
            o["transform"][name][9:12] = [float(v) for v in c.astype(np.float32)]
        o["inner"]["Sphere"]["radius"] = float(rng.uniform(0.02, 0.25))
    return json.dumps(doc)


def beside_focus(txt, seed, w, h):
    """One small sphere per document sphere next to the focus point of a random pixel, a fraction of the lens radius
    beside the patch of the focus plane its block's rays pass through: where the depth slices decide."""
    rng = np.random.default_rng([seed, 2])
    doc = json.loads(txt)
    cam = camera_of(doc, w / h)
    m, t = cam["m"].astype(np.float64), cam["t"].astype(np.float64)
    scale = np.linalg.norm(m, axis=0).mean()
    axes = m / np.linalg.norm(m, axis=0)
    lens = float(cam["aperture"]) * scale
    for o in doc["objects"]["collection"].values():
        if "Sphere" not in o["inner"]:
            continue
        uu, vv = rng.uniform(-0.8, 0.8, 2)
        y, x = float(cam["xfov"]) * 0.5 * -uu, float(cam["yfov"]) * 0.5 * -vv
        d = np.array([-math.cos(x) * math.sin(y), math.sin(x), -math.cos(x) * math.cos(y)])
        depth = float(cam["focus"]) * rng.choice([0.5, 0.9, 1.0, 1.1, 2.0])
        radius = float(rng.uniform(0.03, 0.15))
        side = rng.uniform(0, 2 * math.pi)
        p = d / abs(d[2]) * depth + np.array([math.cos(side), math.sin(side), 0.0]) * (radius + rng.uniform(0.05, 1.0) * lens)
        c = t + axes @ p
        for name in ("transform_world", "transform_local"):
            o["transform"][name][9:12] = [float(v) for v in c.astype(np.float32)]
        o["inner"]["Sphere"]["radius"] = radius
    return json.dumps(doc)


def _run(b, txt, w, h, slices, n, tally=None, config=None, aspect=None, what=None, **clip):
    masks = _masks(b, txt, w, h, slices, n, config=config, aspect=aspect)
    rects = brute(txt, masks, w, h, slices, n, aspect=aspect, what=what, **clip)
    if tally is not None:
        tally.add(masks, rects, len(spheres_of(json.loads(txt))))
    return masks, rects


def _holds(tally, what):
    assert tally.empty > 0 and tally.partial > 0, (what, vars(tally))


def _all_kept(masks, rects, n_rows, what):
    full = ALL64 if n_rows > 64 else (1 << n_rows) - 1
    for m, (x0, y0, nx, ny) in zip(masks, rects):
        assert int(m) == (full if nx and ny else 0), ("a fallback block lost a row", what, (x0, y0), hex(int(m)))


# ---- scaled and mirrored cameras ----------------------------------------------------------------------------------------
def _scaled_family(b, posts, seed0):
    """Random scenes under each camera matrix; with focus also f/0.1 (the lens radius is aperture x the matrix's scale),
    every other time with the spheres close to the lens or beside the focus plane."""
    for vi, (name, post) in enumerate(posts):
        t = Tally()
        for i, (slices, n, focus) in enumerate(COMBOS):
            seed = seed0 + 100 * vi + i
            w, h = SIZES[i % 4]
            kw = dict(cam_post=post, focus=focus)
            if focus:
                kw.update(fstop=0.1)
            txt = sphere_scene(seed, n_spheres=4 if focus else None, **kw)
            if focus and i % 4 == 1:
                txt = near_camera(txt, seed, w / h)
            elif focus and i % 4 == 3:
                txt = beside_focus(txt, seed, w, h)
            _run(b, txt, w, h, slices, n, t, what=(name, seed, slices, n, focus))
        _holds(t, name)


def test_uniform_scale(bendy):
    _scaled_family(bendy, [("s=0.25", np.eye(3) * 0.25), ("s=3", np.eye(3) * 3.0)], 20000)


def test_mirror(bendy):
    _scaled_family(bendy, [("mirror x, s=1", np.diag([-1.0, 1.0, 1.0])), ("mirror y, s=3", np.diag([3.0, -3.0, 3.0])),
                           ("mirror z, s=1", np.diag([1.0, 1.0, -1.0]))], 21000)


def test_scale_and_mirror_change_the_key(bendy):
    b = bendy
    for focus in (False, True):
        normal = sphere_scene(4711, n_spheres=3, focus=focus)
        k = _key(b, normal, 48, 32, 4)
        assert k == _key(b, sphere_scene(4711, n_spheres=3, focus=focus, cam_post=np.eye(3)), 48, 32, 4)
        for post in (np.eye(3) * 0.25, np.eye(3) * 3.0, np.diag([-1.0, 1.0, 1.0]), np.diag([1.0, -1.0, 1.0]),
                     np.diag([1.0, 1.0, -1.0])):
            assert _key(b, sphere_scene(4711, n_spheres=3, focus=focus, cam_post=post), 48, 32, 4) != k
        assert _key(b, normal, 48, 32, 4, config=b.Config(clip_min=0.0)) != k


# ---- the Gram test: at its tolerance, and failing -----------------------------------------------------------------------
def _shear(e):
    m = np.eye(3)
    m[0, 1] = e
    return m


INSIDE = np.diag([1.0, 1.0 + 3e-6, 1.0 - 3e-6]) @ _shear(3e-6)


def test_gram_tolerance_inside(bendy):
    """Column lengths 1, 1 + 3e-6, 1 - 3e-6 and a shear of 3e-6: the Gram test (1e-5) passes, and the bound must hold
    for the rays of this not quite orthogonal matrix under its 2e-4 rad margin."""
    _scaled_family(bendy, [("inside the tolerance", INSIDE)], 22000)


def _fallback_family(b, variants, seed0):
    """Every in-frame block keeps every row; the same scenes under the plain rotation have empty masks."""
    for vi, (name, post) in enumerate(variants):
        normal = Tally()
        for i, (slices, n, focus) in enumerate(COMBOS):
            seed = seed0 + 100 * vi + i
            w, h = SIZES[i % 4]
            txt = sphere_scene(seed, focus=focus, cam_post=post)
            masks, rects = _run(b, txt, w, h, slices, n, what=(name, seed, slices, n, focus))
            _all_kept(masks, rects, len(spheres_of(json.loads(txt))), (name, seed, slices, n, focus))
            _run(b, sphere_scene(seed, focus=focus), w, h, slices, n, normal, what=("normal", seed))
        assert normal.empty > 0, name


def test_gram_tolerance_outside(bendy):
    _fallback_family(bendy, [("column length 1 + 1e-5", np.diag([1.0, 1.0 + 1e-5, 1.0]))], 23000)


def test_non_uniform_scale_and_shear(bendy):
    _fallback_family(bendy, [("diag(1, 1.3, 0.8)", np.diag([1.0, 1.3, 0.8])), ("shear 0.2", _shear(0.2))], 24000)


# ---- very wide frusta ---------------------------------------------------------------------------------------------------
def _uniform_scale_f32(lo, hi):
    return float(np.float32(hi) - np.float32(lo))


def block_angles(cam, w, h, n, rect):
    """(|ym|, |xm|, alpha, cth) of a block as DESIGN.md 5.15 steps 1 - 3 and 5 define them, in float64: the centre of the
    block's yrot / xrot intervals, the cone's half-angle and the cosine of the centre direction's angle from the axis."""
    x0, y0, nx, ny = rect
    pw, ph = float(np.float32(2.0) * (np.float32(1.0) / np.float32(w))), float(np.float32(2.0) * (np.float32(1.0) / np.float32(h)))
    nn = float(max(n, 1))
    sub_hi = (nn - 1.0) / nn
    sub = np.float32(1.0) / np.float32(n) if n > 1 else np.float32(1.0)
    ju0, jv0 = float(np.float32(-0.5) * np.float32(pw) * sub), float(np.float32(-0.5) * np.float32(ph) * sub)
    ju1, jv1 = ju0 + _uniform_scale_f32(ju0, -ju0), jv0 + _uniform_scale_f32(jv0, -jv0)
    uu_lo, uu_hi = x0 * pw - 1.0 + ju0, (x0 + nx - 1) * pw - 1.0 + sub_hi * pw + ju1
    vv_lo, vv_hi = y0 * ph - 1.0 + jv0, (y0 + ny - 1) * ph - 1.0 + sub_hi * ph + jv1
    hxf, hyf = 0.5 * float(cam["xfov"]), 0.5 * float(cam["yfov"])
    wid = 1e-5 * (1.0 + hxf + hyf)
    y_lo, y_hi = min(-hxf * uu_lo, -hxf * uu_hi) - wid, max(-hxf * uu_lo, -hxf * uu_hi) + wid
    x_lo, x_hi = min(-hyf * vv_lo, -hyf * vv_hi) - wid, max(-hyf * vv_lo, -hyf * vv_hi) + wid
    ym, xm = 0.5 * (y_lo + y_hi), 0.5 * (x_lo + x_hi)
    err = lambda x: abs(x) ** 11 / math.factorial(11) + abs(x) ** 12 / math.factorial(12) + 1e-15
    alpha = math.hypot(0.5 * (y_hi - y_lo), 0.5 * (x_hi - x_lo)) + 8.0 * (err(ym) + err(xm)) + 2e-4
    if cam["focus"] is not None:
        r = float(cam["aperture"]) * (1.0 + 1e-4) / (float(cam["focus"]) * (1.0 - 1e-5))
        alpha += r + r ** 3
    return abs(ym), abs(xm), alpha, abs(math.cos(xm) * math.cos(ym))


WIDE = [(0.012, 16 / 9, 64, 36), (0.012, 1.0, 32, 32), (0.006, 16 / 9, 64, 36), (0.006, 1.0, 32, 32),
        (0.006, 16 / 9, 32, 32), (0.003, 16 / 9, 64, 36), (0.003, 1.0, 32, 32), (0.006, 16 / 9, 160, 90),
        (0.003, 16 / 9, 160, 90)]


def test_wide_frusta(bendy):
    """Half-angles up to 2.36 rad (rays that point behind the camera): a block whose centre angle exceeds 1.6 rad or
    whose cone exceeds 0.9 rad keeps every row, the others are bounded as ever, with the depth slices off where the
    centre direction is within 0.1 of perpendicular to the axis."""
    b = bendy
    EPS = 1e-6                                  # a block this close to a limit may fall on either side of it
    seen = dict(ym=0, alpha16=0, cth=0)
    near, normal = Tally(), Tally()
    for ci, (fl, aspect, w, h) in enumerate(WIDE):
        combos = COMBOS if w < 160 else COMBOS[ci % 4::4]
        for i, (slices, n, focus) in enumerate(combos):
            seed = 25000 + 100 * ci + i
            what = (fl, aspect, w, h, seed, slices, n, focus)
            txt = sphere_scene(seed, focus=focus, focal_length=fl)
            masks, rects = _run(b, txt, w, h, slices, n, aspect=aspect, what=what)
            doc = json.loads(txt)
            cam, n_rows = camera_of(doc, aspect), len(spheres_of(doc))
            full = (1 << n_rows) - 1
            unaffected = []
            for m, rect in zip(masks, rects):
                if rect[2] == 0 or rect[3] == 0:
                    continue
                ym, xm, alpha, cth = block_angles(cam, w, h, n, rect)
                if max(ym, xm) > 1.6 + EPS or alpha > 0.9 + EPS:
                    assert int(m) == full, ("a block beyond the limits lost a row", what, rect, ym, xm, alpha)
                    seen["ym"] += max(ym, xm) > 1.6 + EPS
                    seen["alpha16"] += alpha > 0.9 + EPS and slices == 1 and max(ym, xm) <= 1.6 - EPS
                elif max(ym, xm) < 1.6 - EPS and alpha < 0.9 - EPS:
                    unaffected.append((m, rect))
                    seen["cth"] += focus and cth < 0.1
            near.add([m for m, _ in unaffected], [r for _, r in unaffected], n_rows)
            _run(b, sphere_scene(seed, focus=focus), w, h, slices, n, normal, aspect=aspect, what=("normal",) + what)
    assert seen["ym"] > 0 and seen["alpha16"] > 0 and seen["cth"] > 0, seen
    _holds(near, "blocks inside the limits")
    assert normal.empty > 0


# ---- huge apertures -----------------------------------------------------------------------------------------------------
def _aperture_doc(seed, ratio, focus_dist=2.0, fl=0.05, **kw):
    """lens radius / focus distance = ratio (aperture = focal_length / 2 / fstop)"""
    return sphere_scene(seed, focus=True, focal_length=fl, fstop=0.5 * fl / (ratio * focus_dist), focus_dist=focus_dist, **kw)


def test_huge_aperture(bendy):
    """rho / focus = 0.3 and 0.49: bounded (asin(r) <= r + r^3 up to 1/2); 0.51 and 2: every row kept."""
    b = bendy
    slices_n = list(itertools.product([1, 4, 16, 32], [0, 2]))
    for ratio in (0.3, 0.49):
        t = Tally()
        for i, (slices, n) in enumerate(slices_n):
            seed = 26000 + i
            w, h = SIZES[i % 4]
            txt = _aperture_doc(seed, ratio, n_spheres=4)
            if i % 2:
                txt = near_camera(txt, seed, w / h) if i % 4 == 1 else beside_focus(txt, seed, w, h)
            _run(b, txt, w, h, slices, n, t, what=(ratio, seed, slices, n))
        _holds(t, ratio)
    for ratio in (0.51, 2.0):
        normal = Tally()
        for i, (slices, n) in enumerate(slices_n):
            seed = 26000 + i
            w, h = SIZES[i % 4]
            txt = _aperture_doc(seed, ratio, n_spheres=4)
            masks, rects = _run(b, txt, w, h, slices, n, what=(ratio, seed, slices, n))
            _all_kept(masks, rects, 4, (ratio, seed, slices, n))
            _run(b, sphere_scene(seed, n_spheres=4, focus=True), w, h, slices, n, normal)
        assert normal.empty > 0


# ---- clip ranges --------------------------------------------------------------------------------------------------------
CLIPS_HOLD = [("clip_min 0", dict(clip_min=0.0), 0.0, 1000.0), ("clip_max 5", dict(clip_max=5.0), 0.01, 5.0),
              ("clip_min == clip_max", dict(clip_min=6.0, clip_max=6.0), 6.0, 6.0)]


def test_clip_ranges(bendy):
    """clip_min = 0 (roots at the origin count), a short clip_max and an empty range: the masks never depend on
    clip_max and stay valid; the rays are tested with the same range."""
    b = bendy
    for ci, (name, kw, tmin, tmax) in enumerate(CLIPS_HOLD):
        t = Tally()
        for i, (slices, n, focus) in enumerate(COMBOS):
            seed = 27000 + 100 * ci + i
            w, h = SIZES[i % 4]
            txt = sphere_scene(seed, focus=focus)
            if focus and i % 4 == 1:
                txt = near_camera(txt, seed, w / h)
            _run(b, txt, w, h, slices, n, t, config=b.Config(**kw), what=(name, seed, slices, n, focus),
                 tmin=np.float32(tmin), tmax=np.float32(tmax))
        _holds(t, name)


def test_negative_clip_min_keeps_every_row(bendy):
    b = bendy
    normal = Tally()
    for i, (slices, n, focus) in enumerate(COMBOS):
        seed = 27500 + i
        w, h = SIZES[i % 4]
        txt = sphere_scene(seed, focus=focus)
        for cm in (-1.0, -1e-6):
            masks, rects = _run(b, txt, w, h, slices, n, config=b.Config(clip_min=cm), what=(cm, seed),
                                tmin=np.float32(cm))
            _all_kept(masks, rects, len(spheres_of(json.loads(txt))), (cm, seed, slices, n, focus))
        _run(b, txt, w, h, slices, n, normal)
    assert normal.empty > 0


# ---- 63, 64, 65 and 130 spheres -----------------------------------------------------------------------------------------
def many_spheres(seed, n, focus):
    """`n` spheres, thinned so that blocks without any remain: a sphere around the camera moves behind it, radii shrink
    to a quarter (the ground spheres to 1), and row 63 (when there is one) sits small in the middle of the view."""
    doc = json.loads(sphere_scene(seed, n_spheres=n, focus=focus, focal_length=0.05))
    cam = camera_of(doc, 1.5)
    m, t = cam["m"].astype(np.float64), cam["t"].astype(np.float64)
    k = 0
    for key in sorted(doc["objects"]["collection"], key=int):
        o = doc["objects"]["collection"][key]
        if "Sphere" not in o["inner"]:
            continue
        c = np.asarray(o["transform"]["transform_world"][9:12], np.float64)
        r = o["inner"]["Sphere"]["radius"]
        r = 1.0 if r >= 50 else 0.25 * r
        if np.linalg.norm(c - t) < 4 * r + 1.0:
            c = t + m @ np.array([0.3 * (k % 7 - 3), 0.0, 3.0 + 0.1 * k])
        if k == 63:
            c, r = t + m @ np.array([0.0, 0.0, -8.0]), 0.3
        for name in ("transform_world", "transform_local"):
            o["transform"][name][9:12] = [float(v) for v in c.astype(np.float32)]
        o["inner"]["Sphere"]["radius"] = float(r)
        k += 1
    return doc


def first_rows(doc, n):
    """The document with its first n spheres only."""
    doc = json.loads(json.dumps(doc))
    col, k = doc["objects"]["collection"], 0
    for key in sorted(col, key=int):
        if "Sphere" in col[key]["inner"]:
            if k >= n:
                del col[key]
            k += 1
    return doc


SLICES_N = list(itertools.product([1, 4, 16, 32], [0, 2]))


@pytest.mark.parametrize("count", [63, 64])
def test_sphere_counts_that_fit_a_mask(bendy, count):
    b = bendy
    t = Tally()
    bit63_clear = bit63_set = 0
    for i, (slices, n) in enumerate(SLICES_N):
        w, h = SIZES[i % 4]
        txt = json.dumps(many_spheres(28000 + i, count, focus=bool(i & 1)))
        masks, rects = _run(b, txt, w, h, slices, n, t, what=(count, i))
        inside = [int(m) for m, r in zip(masks, rects) if r[2] and r[3]]
        assert all(m >> count == 0 for m in inside)
        bit63_clear += sum(not m >> 63 for m in inside)
        bit63_set += sum(m >> 63 for m in inside)
    _holds(t, count)
    if count == 64:
        assert bit63_clear > 0 and bit63_set > 0


@pytest.mark.parametrize("count", [65, 130])
def test_sphere_counts_beyond_a_mask(bendy, count):
    b = bendy
    normal = Tally()
    for i, (slices, n) in enumerate(SLICES_N):
        w, h = SIZES[i % 4]
        doc = many_spheres(28000 + i, count, focus=bool(i & 1))
        masks, rects = _run(b, json.dumps(doc), w, h, slices, n, what=(count, i))
        _all_kept(masks, rects, count, (count, i))
        _run(b, json.dumps(first_rows(doc, 64)), w, h, slices, n, normal, what=("first 64 of", count, i))
    assert normal.empty > 0
