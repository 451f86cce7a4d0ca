"""Axis-aligned rooms and exact ties for the sorted rect path (test infrastructure; pure data, as scene_gen.py).

scene_gen.random_scene gives every rect and cuboid a random rotation, so it never produces the rows that bt_scene.cpp sorts
into BtRectAAN (identity matrix, unit-axis normal), never two objects with one matrix (the `first_of_normal == 0` rows of
BtRectLA), never a rect whose local axes are not unit axes, and a tie in t only by accident.  room_scene() constructs all of
them; tie_scene() puts two objects exactly into one plane; limit_scene() squares a half extent to +inf and to 0.
tests/test_rect_rows.py proves on the CPU that each ingredient is present in what the library uploads.
"""
import json
import math

import numpy as np

from scene_gen import _affine, _cuboid, _rect, _rot

# the 24 ordered pairs (x, y) of distinct signed unit axes as ((axis of x, sign), (axis of y, sign)), by the axis of x cross y
PAIRS = [((iu, su), (iv, sv)) for iu in range(3) for su in (1, -1) for iv in range(3) if iv != iu for sv in (1, -1)]
PAIRS_BY_NORMAL_AXIS = [[p for p in PAIRS if 3 - p[0][0] - p[1][0] == w] for w in range(3)]

ROOM_LO = np.array([-4.0, -2.0, -6.0])
ROOM_HI = np.array([4.0, 3.0, 5.0])
ROOM_SEEDS = range(24)
VOLUME_SEEDS = (0, 1, 2, 3, 5, 8)      # room_scene(seed, volume=True): one seed of every axis_plan mode and more


def _unit(i, s):
    v = np.zeros(3)
    v[i] = s
    return v


def aligned_rect(material, pair, extents):
    """Rect::new with x, y along the signed unit axes of `pair`; extents = half extents along the WORLD axes."""
    (iu, su), (iv, sv) = pair
    assert abs(extents[iu] - extents[iv]) > 1e-3, "walls are never square: a swapped limit has to show"
    return _rect(material, _unit(iu, su) * extents[iu], _unit(iv, sv) * extents[iv])


class _Doc:
    """The bookkeeping of scene_gen.random_scene: data and objects keyed by ascending refs."""

    def __init__(self):
        self.data = {"0": {"inner": {"Material": {"Flat": {"albedo": {"r": 0.0, "g": 0.0, "b": 0.0}}}}}}
        self.objects = {}
        self.root = 0

    def add_data(self, inner):
        k = str(len(self.data))
        self.data[k] = {"inner": inner}
        return int(k)

    def add_obj(self, inner, m, t, tag=None, flags=0):
        k = len(self.objects)
        a = _affine(m, t)
        self.objects[str(k)] = {"object_ref": k, "tag": tag, "flags": {"bits": flags},
                                "transform": {"transform_world": a, "transform_local": a, "transform_parent": None},
                                "inner": inner, "children": None}
        return k

    def dumps(self):
        return json.dumps({"roots": [], "root_material": self.root,
                           "objects": {"collection": self.objects, "next_key": len(self.objects)},
                           "data": {"collection": self.data, "next_key": len(self.data)}})


def axis_plan(seed):
    """(plain axis-aligned rects per normal axis, identity cuboids) of room_scene(seed): seed % 4 = 0 leaves one axis without
    a row, gives one axis exactly one and one axis 3 or 4; 1 leaves two axes empty; 2 and 3 add identity cuboids (two strict
    rows per axis each) to 1 / 2 / 3 rects and to the six walls plus panels."""
    mode, rot = seed % 4, (seed // 4) % 3
    counts = [0, 0, 0]
    if mode == 0:
        counts[(rot + 1) % 3] = 1
        counts[(rot + 2) % 3] = 3 + (seed // 12) % 2
        return counts, 0
    if mode == 1:
        counts[rot] = 3 + (seed // 4) % 4
        return counts, 0
    if mode == 2:
        for k in range(3):
            counts[(rot + k) % 3] = 1 + k
        return counts, 1
    counts = [2, 2, 2]
    counts[rot] += 1 + (seed // 12) % 2
    return counts, 2 + (seed // 4) % 2


def room_scene(seed, volume=False, counts=None, ident_cuboids=None, n_spheres=None, floor_half_width=None,
               la_half_height=None):
    """A room of axis-aligned rects around the camera.  `counts` / `ident_cuboids` override axis_plan(seed), `n_spheres` the
    drawn 1 or 2; floor_half_width / la_half_height replace one half extent of the low y wall / of the rect that shares
    its matrix with two cuboids (limit_scene)."""
    rng = np.random.default_rng(1000 + seed)
    col = lambda lo=0.1, hi=0.95: dict(zip("rgb", [float(v) for v in rng.uniform(lo, hi, 3)]))
    d = _Doc()
    root_kind = seed % 3 if seed < 3 else int(rng.integers(3))
    if root_kind == 0:
        d.root = d.add_data({"Material": {"Emissive": {"albedo": col(), "intensity": float(rng.uniform(0.05, 0.5))}}})
    elif root_kind == 1:
        d.root = d.add_data({"Material": {"Flat": {"albedo": col(0.0, 0.3)}}})
    diffuse = d.add_data({"Material": {"Diffuse": {"albedo": col(), "roughness": 0.5}}})
    diffuse2 = d.add_data({"Material": {"Diffuse": {"albedo": col(), "roughness": 1.0}}})
    metallic = d.add_data({"Material": {"Metallic": {"albedo": col(), "roughness": float(rng.uniform(0.0, 0.4))}}})
    glass = d.add_data({"Material": {"Glass": {"albedo": col(0.8, 1.0), "roughness": float(rng.uniform(0.0, 0.1)),
                                               "ior": float(rng.uniform(1.1, 1.8))}}})
    flat = d.add_data({"Material": {"Flat": {"albedo": col()}}})
    light_mat = d.add_data({"Material": {"Emissive": {"albedo": col(0.7, 1.0), "intensity": float(rng.uniform(5, 20))}}})
    mats = [diffuse, diffuse2, metallic, glass, flat]
    eye = np.eye(3)

    # the camera inside the room, looking down -z with a small tilt
    a = rng.uniform(-0.15, 0.15)
    tilt = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    focus = float(rng.uniform(4, 9)) if seed % 2 else None
    d.add_obj({"Camera": {"sensor_size": 0.024, "focal_length": float(rng.uniform(0.025, 0.04)), "aspect_ratio": 1.5,
                          "fstop": float(rng.uniform(0.7, 4.0)), "focus": focus}}, tilt,
              (rng.uniform(-0.5, 0.5), rng.uniform(0.2, 0.8), 3.5), tag="camera")

    plan_counts, plan_cuboids = axis_plan(seed)
    counts = list(plan_counts if counts is None else counts)
    ident_cuboids = plan_cuboids if ident_cuboids is None else ident_cuboids
    # lights: 1 - 3 of {axis-aligned lamp, identity cuboid, rotated rect}; a scene that keeps an axis free of rows cannot
    # hold an identity cuboid (its faces have all six normals)
    mask = 1 + int(rng.integers(7))
    lamp, cuboid_light, rotated_light = bool(mask & 1), bool(mask & 2) and ident_cuboids > 0, bool(mask & 4)
    lamp = lamp and max(counts) >= 4
    if not (lamp or cuboid_light):
        rotated_light = True

    centre, half = (ROOM_LO + ROOM_HI) / 2, (ROOM_HI - ROOM_LO) / 2
    n_aligned = 0
    for w in range(3):
        inplane = [i for i in range(3) if i != w]
        for j in range(counts[w]):
            pair = PAIRS_BY_NORMAL_AXIS[w][(seed * 3 + n_aligned * 5 + j) % 8]
            n_aligned += 1
            t, ext, tag, mat, flags = centre.copy(), half.copy(), None, int(rng.choice([diffuse, diffuse2, metallic, flat])), 0
            if j < 2:                                     # the two walls of the axis
                t[w] = (ROOM_LO, ROOM_HI)[j][w]
                tag = "floor" if (w, j) == (1, 0) else None
            else:                                        # panels inside the room: a glass pane, the lamp, anything
                for i in inplane:
                    t[i] = rng.uniform(-1.5, 1.5) + (0.5 if i == 1 else -1.0 if i == 2 else 0.0)
                    ext[i] = rng.uniform(1.1, 1.5) if i == inplane[0] else rng.uniform(0.4, 0.9)
                if j == 2:
                    mat = glass                           # free-standing, in the middle of the room: met from both sides
                    t[w] = centre[w] + rng.uniform(-0.5, 0.5) + (-1.5 if w == 2 else 0.0)
                elif j == 3 and lamp:
                    mat, flags = light_mat, 1
                    t[w] = ROOM_HI[w] - 0.25
                else:
                    t[w] = rng.uniform(ROOM_LO[w] + 1.0, min(ROOM_HI[w], 2.5) - 0.5)
            r = aligned_rect(mat, pair, ext)
            if tag == "floor" and floor_half_width is not None:
                r["half_width"] = floor_half_width        # not through Rect::new: the norm of such an x leaves float32 itself
            d.add_obj({"Rect": r}, eye, t, tag=tag, flags=flags)

    for k in range(ident_cuboids):                        # strict axis-aligned rows: Diffuse, Metallic, Glass in turn
        h = rng.uniform(0.3, 0.8, 3)
        pos = np.array([rng.uniform(-3, 3), ROOM_LO[1] + h[1] + (0.0 if k % 2 else 0.5), rng.uniform(-4.5, 0.5)])
        d.add_obj({"Cuboid": _cuboid([diffuse, metallic, glass][(seed // 4 + k) % 3], *h)}, eye, pos)
    if cuboid_light:
        d.add_obj({"Cuboid": _cuboid(light_mat, 0.5, 0.1, 0.3)}, eye, (rng.uniform(-2, 2), 2.5, rng.uniform(-3, 0)), flags=1)

    place = lambda: rng.uniform([-3.0, -1.2, -5.0], [3.0, 2.0, 0.5])
    # one matrix, bit for bit, under two cuboids and a plain rect: the rect's world normal is a cuboid face's
    shared = _rot(rng).astype(np.float32)
    assert np.all(shared != 0.0)                          # then a +-0 in a local normal cannot reach the world normal
    d.add_obj({"Cuboid": _cuboid(int(rng.choice(mats)), *rng.uniform(0.25, 0.7, 3))}, shared, place())
    r = _rect(int(rng.choice(mats)), np.array([rng.uniform(0.4, 1.2), 0, 0]), np.array([0, rng.uniform(0.4, 1.2), 0]))
    if la_half_height is not None:
        r["half_height"] = la_half_height
    d.add_obj({"Rect": r}, shared, place(), tag="shared_rect")
    d.add_obj({"Cuboid": _cuboid(int(rng.choice(mats)), *rng.uniform(0.25, 0.7, 3))}, shared, place())
    # rotations of their own; one of the two objects under a non-uniform scale
    m1, m2 = _rot(rng), _rot(rng)
    scale = np.diag(rng.uniform(0.7, 1.4, 3))
    if seed % 2:
        m1 = m1 @ scale
    else:
        m2 = m2 @ scale
    d.add_obj({"Cuboid": _cuboid(int(rng.choice(mats)), *rng.uniform(0.25, 0.7, 3))}, m1, place())
    d.add_obj({"Rect": _rect(int(rng.choice(mats)), np.array([rng.uniform(0.4, 1.2), 0, 0]),
                             np.array([0, rng.uniform(0.4, 1.2), 0]))}, m2, place())
    if rotated_light:
        tip = _rot(rng) if seed % 3 else np.array([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]])   # or a quarter turn: still no identity
        d.add_obj({"Rect": _rect(light_mat, np.array([0.8, 0, 0]), np.array([0, 0.5, 0]))}, tip,
                  (rng.uniform(-2, 2), 2.6, rng.uniform(-3, 0)), flags=1)
    # general rects: local axes that are no unit axes, one pair orthogonal, one not
    u, v = rng.uniform(0.5, 1.0, 2)
    d.add_obj({"Rect": _rect(int(rng.choice(mats)), np.array([u, u, 0.0]), np.array([-v, v, 0.0]))}, eye, place())
    d.add_obj({"Rect": _rect(int(rng.choice(mats)), np.array([u, 0.3 * u, 0.1 * u]), np.array([0.2 * v, v, -0.2 * v]))},
              _rot(rng), place())
    for k in range(int(rng.integers(1, 3)) if n_spheres is None else n_spheres):
        d.add_obj({"Sphere": {"material": glass if k == 0 else int(rng.choice(mats)), "volume": None,
                              "radius": float(rng.uniform(0.3, 0.8))}}, eye, place())
    if volume:
        n = int(rng.choice([3, 5]))
        buf = rng.uniform(0, 1, n * n * n).astype(np.float32)
        buf[rng.uniform(size=buf.size) < 0.5] = 0.0
        buf *= np.float32(rng.choice([0.5, 3.0, 12.0]))
        vol = d.add_data({"Volume": {"DensityMap": {"width": n, "height": n, "depth": n, "size": [n - 1.0] * 3,
                                                    "buffer": [float(x) for x in buf]}}})
        d.add_obj({"Sphere": {"material": int(rng.choice(mats)), "volume": vol, "radius": float(rng.uniform(0.7, 1.2))}},
                  _rot(rng), (rng.uniform(-1, 1), rng.uniform(0, 1), rng.uniform(-2.5, 0.5)))
    return d.dumps()


def limit_scene(kind):
    """The room of seed 3 (six walls) with a half extent whose square leaves float32: "inf" -- the floor's half_width and the
    shared-matrix rect's half_height are 2e19 (squares overflow to +inf: a plane and a strip without ends); "zero" -- both
    are 1e-23 (squares underflow to 0: only a local coordinate whose own square underflows passes)."""
    v = {"inf": 2e19, "zero": 1e-23}[kind]
    return room_scene(3, floor_half_width=v, la_half_height=v)


# ---- exact ties ---------------------------------------------------------------------------------------------------------
TIE_KINDS = ("plain_plain", "strict_strict", "strict_plain")
TIE_FRAMES = ("identity", "rotated", "generic")
# a Y "rotation" whose entries, and every sum formed from them below, are exact in float32 (cos, sin ~ 0.8, 0.6)
_C, _S = 3277.0 / 4096.0, 2457.0 / 4096.0
TIE_MATRIX = {"identity": np.eye(3), "generic": np.eye(3),
              "rotated": np.array([[_C, 0, _S], [0, 1, 0], [-_S, 0, _C]])}
TIE_CASES = [(kind, order, frame) for kind in TIE_KINDS for frame in TIE_FRAMES[:2] for order in (0, 1)] + \
            [("plain_plain", order, "generic") for order in (0, 1)]
TIE_PLAIN_TAG = "tie_plain"


def tie_scene(kind, order, frame="identity"):
    """Two Flat objects A (red) and B (blue) that meet every ray at bit-identical t where they overlap; order 0: A has the
    lower ObjectRef, 1: B.  Same matrix and, for the first two kinds, the same translation, so p and q of rect.rs:120-124
    are the same numbers for both.
    plain_plain: two rects (try_hit's later one wins, mod.rs:389-402); frame "identity" -> two BtRectAAN rows, "rotated" ->
    two BtRectLA rows, "generic" -> a BtRectAAN row against a rect whose local axes are diagonal (a BtPrim row).
    strict_strict: a cuboid and its exact duplicate (`manifold.t < t`, cuboid.rs:96: the earlier one wins).
    strict_plain: a rect in the plane of a cuboid's face towards the camera; the face's translation t + M * offset is exact
    in float32 and is the rect's.  The rect wins in both orders."""
    assert kind in TIE_KINDS and frame in TIE_FRAMES and (frame != "generic" or kind == "plain_plain")
    d = _Doc()
    d.root = d.add_data({"Material": {"Flat": {"albedo": {"r": 0.2, "g": 0.25, "b": 0.2}}}})
    red = d.add_data({"Material": {"Flat": {"albedo": {"r": 0.9, "g": 0.1, "b": 0.1}}}})
    blue = d.add_data({"Material": {"Flat": {"albedo": {"r": 0.1, "g": 0.2, "b": 0.9}}}})
    d.add_obj({"Camera": {"sensor_size": 0.024, "focal_length": 0.05, "aspect_ratio": 1.5, "fstop": 2.0, "focus": None}},
              np.eye(3), (0.0, 0.0, 3.0), tag="camera")
    m = TIE_MATRIX[frame]
    t0 = np.array([0.25, 0.125, -2.0])
    ex, ey = np.array([1.0, 0, 0]), np.array([0, 1.0, 0])
    ta = tb = t0
    tag_b = None
    if kind == "plain_plain":
        a = {"Rect": _rect(red, 1.5 * ex, 1.0 * ey)}
        if frame == "generic":
            b = {"Rect": _rect(blue, np.array([0.9, 0.9, 0]), np.array([-0.6, 0.6, 0]))}
            assert b["Rect"]["z"] == [0.0, 0.0, 1.0]      # the same normal as A's, or the two t would differ by a rounding
        else:
            b = {"Rect": _rect(blue, 1.0 * ex, 1.5 * ey)}
    elif kind == "strict_strict":
        a, b = {"Cuboid": _cuboid(red, 0.75, 0.625, 0.5)}, {"Cuboid": _cuboid(blue, 0.75, 0.625, 0.5)}
    else:
        a, b = {"Cuboid": _cuboid(red, 0.75, 0.625, 0.5)}, {"Rect": _rect(blue, 0.5 * ex, 0.25 * ey)}
        tb = t0 + m @ np.array([0, 0, 0.5])               # Cuboid::new's offset of the +z face (cuboid.rs:19-30)
        assert np.array_equal(tb.astype(np.float32).astype(np.float64), tb)
        tag_b = TIE_PLAIN_TAG
    if order == 0:
        d.add_obj(a, m, ta)
        d.add_obj(b, m, tb, tag=tag_b)
    else:
        d.add_obj(b, m, tb, tag=tag_b)
        d.add_obj(a, m, ta)
    return d.dumps()


def without_tagged(txt, tag):
    """The scene without the object that carries `tag`."""
    doc = json.loads(txt)
    col = doc["objects"]["collection"]
    for k in [k for k, o in col.items() if o["tag"] == tag]:
        del col[k]
    return json.dumps(doc)
