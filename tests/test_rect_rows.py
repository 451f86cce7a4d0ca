"""The sorted rect tables (bt_scene.cpp flatten_scene -> bt_device.hpp intersect_sorted) on the host alone.

Scene.export_sorted_rows() returns what would be uploaded; the tests restate every field in numpy from export_prims() and the
scene documents, check abs_limit() against its definition rather than against a second bisection, and prove that
rect_scenes.py really constructs what tests/test_gpu_rect_scenes.py relies on -- so that those tests cannot pass vacuously.
No GPU: the host library and the CPU oracle."""
import json

import numpy as np
import pytest

from conftest import scene_path
from rect_scenes import (PAIRS, ROOM_SEEDS, TIE_CASES, TIE_PLAIN_TAG, VOLUME_SEEDS, axis_plan, limit_scene, room_scene, tie_scene,
                         without_tagged)

# words of a BtPrim row (bt_types.h) in export_prims()
KIND, OBJECT, MATERIAL, VOLUME, C, T, W_SQR, ICX, H_SQR, ICY, AA_U, ICZ, AA_V, IT, AA_W, AX, AX_W, AY, AY_W = \
    0, 1, 2, 3, 4, 8, 11, 12, 15, 16, 19, 20, 23, 24, 27, 28, 31, 32, 35
SPHERE, RECT, RECT_AA, RECT_AAN, RECT_LA, SHAPE_MASK, STRICT = 0, 1, 2, 3, 4, 7, 8
BUNDLED = ("scene", "cornell", "cornell2", "volume", "cloud")

CASES = [f"bundled-{n}" for n in BUNDLED] + ["default"] + [f"room-{s}" for s in ROOM_SEEDS] + \
        [f"volroom-{s}" for s in VOLUME_SEEDS] + ["tie-%s-%d-%s" % c for c in TIE_CASES] + ["limit-inf", "limit-zero"]
_tables = {}


def _text(case):
    kind, _, rest = case.partition("-")
    if kind == "room":
        return room_scene(int(rest))
    if kind == "volroom":
        return room_scene(int(rest), volume=True)
    if kind == "tie":
        k, order, frame = rest.rsplit("-", 2)
        return tie_scene(k, int(order), frame)
    if kind == "limit":
        return limit_scene(rest)
    return None


def tables(bendy, case):
    """(prims [n, 36] float32, export_sorted_rows()) of a case, flattened once."""
    if case not in _tables:
        txt = _text(case)
        if txt is not None:
            sc = bendy.Scene.from_json(txt)
        elif case == "default":
            sc = bendy.Scene.default()
        else:
            sc = bendy.Scene.load(scene_path(case.partition("-")[2]))
        _tables[case] = (sc.export_prims(), sc.export_sorted_rows())
    return _tables[case]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_limit(s, L):
    """abs_limit by its definition, in float32: s is the largest float whose square, as the kernel would round it, is <= L."""
    s, L = np.float32(s), np.float32(L)
    if not L >= 0:
        assert s == np.float32(-1.0), (s, L)
        return
    if np.isinf(L):
        assert np.isposinf(s), (s, L)
        return
    with np.errstate(over="ignore", under="ignore"):
        up = np.nextafter(s, np.float32(np.inf))
        assert s >= 0 and np.isfinite(s) and s * s <= L and up * up > L, (s, L)
        assert (s * s).dtype == np.float32


def restated(p):
    """The three tables from the primitive table, field by field, as flatten_scene documents them (bt_types.h)."""
    pi = p.view(np.int32)
    n = p.shape[0]
    shape, strict = pi[:, KIND] & SHAPE_MASK, (pi[:, KIND] & STRICT) != 0
    prio = [0xfffe - i if strict[i] else 0x10000 + i for i in range(n)]
    n_aan, aan = [0, 0, 0], []
    for w in range(3):
        a, b = (1 if w == 0 else 0), (1 if w == 2 else 2)        # the in-plane axes, ascending
        for i in range(n):
            if shape[i] != RECT_AAN or pi[i, AA_W] != w:
                continue
            u, v = pi[i, AA_U], pi[i, AA_V]
            assert {u, v} == {a, b}
            src_a, src_b = (p[i, W_SQR], p[i, H_SQR]) if u == a else (p[i, H_SQR], p[i, W_SQR])
            assert abs(p[i, C + w]) == 1.0
            aan.append(dict(it_a=p[i, IT + a], it_b=p[i, IT + b], src_a=src_a, src_b=src_b, t_w=p[i, T + w],
                            sgn_mask=0x80000000 if np.signbit(p[i, C + w]) else 0, prio=prio[i], prim=i))
            n_aan[w] += 1
    la, seen = [], {}
    for i in range(n):
        if shape[i] == RECT_LA:
            seen.setdefault(bits(p[i, C:C + 3]).tobytes(), []).append(i)
    for run in sorted(seen.values(), key=lambda r: r[0]):      # a run sits where its first row would
        for k, i in enumerate(run):
            u, v = pi[i, AA_U], pi[i, AA_V]
            la.append(dict(n=p[i, C:C + 3], first_of_normal=int(k == 0), t=p[i, T:T + 3], prio=prio[i],
                           a_x=(p[i, ICX + u], p[i, ICX + v]), a_y=(p[i, ICY + u], p[i, ICY + v]),
                           a_z=(p[i, ICZ + u], p[i, ICZ + v]), a_w=(p[i, IT + u], p[i, IT + v]),
                           src=(p[i, W_SQR], p[i, H_SQR]), prim=i))
    other = [i for i in range(n) if shape[i] not in (RECT_AAN, RECT_LA)]
    return n_aan, aan, la, other


@pytest.mark.parametrize("case", CASES)
def test_sorted_tables_restated(bendy, case):
    p, s = tables(bendy, case)
    n_aan, aan, la, other = restated(p)
    assert list(s["n_aan"]) == n_aan and len(s["aan"]) == len(aan) and len(s["la"]) == len(la)
    assert np.array_equal(s["other"], np.array(other, dtype=np.int32))
    for got, want in zip(s["aan"], aan):
        for f in ("it_a", "it_b", "t_w"):
            assert bits(got[f]) == bits(np.float32(want[f])), (f, want["prim"])
        assert got["sgn_mask"] == want["sgn_mask"] and got["prio"] == want["prio"] and got["pad"] == 0, want["prim"]
        check_limit(got["lim_a"], want["src_a"])
        check_limit(got["lim_b"], want["src_b"])
        # the same six constants as the generic loop reads them from the primitive row itself (bt_types.h BtPrim.ax / ay)
        i = want["prim"]
        packed = [want["t_w"], want["it_a"], want["it_b"], want["src_a"], want["src_b"], p[i, C + p.view(np.int32)[i, AA_W]],
                  np.float32(0), np.float32(0)]
        assert np.array_equal(bits(p[i, AX:AX + 8]), bits(np.array(packed, dtype=np.float32)))
    for got, want in zip(s["la"], la):
        for f in ("n", "t", "a_x", "a_y", "a_z", "a_w"):
            assert np.array_equal(bits(got[f]), bits(np.array(want[f], dtype=np.float32))), (f, want["prim"])
        assert got["first_of_normal"] == want["first_of_normal"] and got["prio"] == want["prio"], want["prim"]
        assert not got["pad"].any()
        check_limit(got["lim"][0], want["src"][0])
        check_limit(got["lim"][1], want["src"][1])
    # every row of the primitive table in exactly one of the three tables
    prims_of = lambda rows: [int(r["prio"]) - 0x10000 if r["prio"] >= 0x10000 else 0xfffe - int(r["prio"]) for r in rows]
    everywhere = prims_of(s["aan"]) + prims_of(s["la"]) + [int(i) for i in s["other"]]
    assert sorted(everywhere) == list(range(p.shape[0]))
    # group order x, y, z with ascending rows inside a group
    at = 0
    for w in range(3):
        group = prims_of(s["aan"][at:at + n_aan[w]])
        assert group == sorted(group) and all(p.view(np.int32)[i, AA_W] == w for i in group)
        at += n_aan[w]


def test_abs_limit_planted_values(bendy):
    f = bendy.api.lib.bt_debug_abs_limit
    one = np.float32(1.0)
    tiny, flt_min, flt_max = np.float32(1.401298464e-45), np.float32(1.17549435e-38), np.float32(3.4028234664e38)
    planted = [0.0, tiny, np.nextafter(tiny, one), flt_min, np.nextafter(flt_min, np.float32(0)), np.nextafter(one, np.float32(0)),
               one, np.nextafter(one, np.float32(2)), flt_max, np.float32(np.inf), np.float32(-0.0), np.float32(-1.0),
               -tiny, np.float32(-np.inf), np.float32(np.nan), np.float32(2.0)]
    # either side of rounding boundaries of x * x: for x with a full mantissa the exact square lies strictly between two
    # floats; L = the float below, fl(x * x) itself and the float above it
    rng = np.random.default_rng(7)
    with np.errstate(over="ignore", under="ignore"):
        for x in np.concatenate([rng.uniform(0.5, 2.0, 40), rng.uniform(1e-20, 1e-18, 10), rng.uniform(1e18, 1.8e19, 10),
                                 rng.uniform(1e-23, 4e-23, 10)]).astype(np.float32):
            sq = x * x
            planted += [np.nextafter(sq, np.float32(0)), sq, np.nextafter(sq, np.float32(np.inf))]
    for L in planted:
        check_limit(f(float(L)), L)
    assert f(0.0) > 0 and f(0.0) ** 2 < 1.5e-45            # squares that underflow to zero do pass `x * x <= 0`
    assert f(float("inf")) == float("inf") and f(float("nan")) == -1.0 and f(-1.0) == -1.0 and f(-0.0) == f(0.0)


# ---- what the generator has to contain ---------------------------------------------------------------------------------------
def _docs():
    return {seed: json.loads(room_scene(seed)) for seed in ROOM_SEEDS}


def _is_identity(obj):
    return obj["transform"]["transform_world"][:9] == [1, 0, 0, 0, 1, 0, 0, 0, 1]


def _kind_of(doc, ref):
    (name, _), = doc["data"]["collection"][str(ref)]["inner"]["Material"].items()
    return name


def _objects(doc, kind):
    return [(o, o["inner"][kind]) for o in doc["objects"]["collection"].values() if isinstance(o["inner"], dict) and kind in o["inner"]]


def test_room_walls_cover_every_orientation(bendy):
    pairs, combos, glass_panes = set(), set(), 0
    for seed, doc in _docs().items():
        panes = 0
        for o, r in _objects(doc, "Rect"):
            if not _is_identity(o):
                continue
            x, y = np.array(r["x"]), np.array(r["y"])
            if not (np.abs(x).sum() == 1 and np.abs(y).sum() == 1 and np.abs(x).max() == 1 and np.abs(y).max() == 1):
                continue                                   # a general rect under the identity
            assert r["half_width"] != r["half_height"]
            iu, iv = int(np.abs(x).argmax()), int(np.abs(y).argmax())
            pairs.add(((iu, int(x[iu])), (iv, int(y[iv]))))
            panes += _kind_of(doc, r["material"]) == "Glass"
        assert panes >= 1, seed                            # a free-standing Glass rect on an axis-aligned row, every seed
        glass_panes += panes
        p, s = tables(bendy, f"room-{seed}")
        pi = p.view(np.int32)
        for i in range(p.shape[0]):
            if pi[i, KIND] == RECT_AAN:                    # plain: not strict
                w = pi[i, AA_W]
                combos.add((int(w), bool(np.signbit(p[i, C + w])), bool(pi[i, AA_U] == (1 if w == 0 else 0))))
    assert pairs == set(PAIRS) and len(pairs) == 24
    assert combos == {(w, neg, first) for w in range(3) for neg in (False, True) for first in (False, True)}


def test_room_axis_groups_come_in_every_size(bendy):
    n = {seed: [int(v) for v in tables(bendy, f"room-{seed}")[1]["n_aan"]] for seed in ROOM_SEEDS}
    for axis in range(3):
        sizes = {v[axis] for v in n.values()}
        assert 0 in sizes and 1 in sizes, (axis, sizes)
        assert any(v >= 3 and v % 2 for v in sizes) and any(v >= 3 and v % 2 == 0 for v in sizes), (axis, sizes)
    empties = {sum(1 for c in v if c == 0) for v in n.values()}
    assert {0, 1, 2} <= empties                           # seeds with one and with two axes without a row
    for seed in ROOM_SEEDS:                               # without identity cuboids the library counts what the plan says
        counts, cuboids = axis_plan(seed)
        assert cuboids or n[seed] == counts, seed


def test_room_identity_cuboids_are_strict_aligned_rows_of_three_materials(bendy):
    mats = set()
    for seed, doc in _docs().items():
        ident = [c for o, c in _objects(doc, "Cuboid") if _is_identity(o)]
        mats |= {_kind_of(doc, c["faces"][0][1]["material"]) for c in ident}
        kinds = tables(bendy, f"room-{seed}")[0].view(np.int32)[:, KIND]
        assert int((kinds == (RECT_AAN | STRICT)).sum()) == 6 * len(ident), seed
    assert {"Diffuse", "Metallic", "Glass"} <= mats


def test_room_shared_normals_general_rects_and_spheres_in_every_seed(bendy):
    for seed, doc in _docs().items():
        p, s = tables(bendy, f"room-{seed}")
        pi = p.view(np.int32)
        la = s["la"]
        assert int((la["first_of_normal"] == 0).sum()) >= 1, seed
        # a run that holds a cuboid face AND the plain rect under the same matrix
        runs, mixed = np.cumsum(la["first_of_normal"]), False
        for r in set(runs.tolist()):
            strict = {bool(x < 0x10000) for x in la["prio"][runs == r]}
            mixed |= strict == {True, False}
        assert mixed, seed
        shapes = {int(pi[i, KIND] & SHAPE_MASK) for i in s["other"]}
        assert RECT in shapes and SPHERE in shapes, seed
        general = [r for o, r in _objects(doc, "Rect") if np.abs(np.array(r["x"])).max() < 0.999]
        dots = sorted(abs(float(np.dot(r["x"], r["y"]))) for r in general)
        assert len(general) == 2 and dots[0] < 1e-6 and dots[1] > 0.05, (seed, dots)      # one pair orthogonal, one not
        # one object under a non-uniform scale, others under rotations of their own
        mats = [np.array(o["transform"]["transform_world"][:9]).reshape(3, 3) for o, _ in _objects(doc, "Rect") + _objects(doc, "Cuboid")
                if not _is_identity(o)]
        spread = [np.ptp(np.linalg.norm(m, axis=1)) for m in mats]
        assert sum(1 for v in spread if v > 0.01) == 1 and len({m.tobytes() for m in mats}) >= 4, seed
        assert 1 <= len(_objects(doc, "Sphere")) <= 2
        assert _kind_of(doc, _objects(doc, "Sphere")[0][1]["material"]) == "Glass"


def test_room_lights_roots_and_cameras():
    light_kinds, roots, focus = set(), set(), set()
    for seed, doc in _docs().items():
        lights = [(o, k) for k in ("Rect", "Cuboid", "Sphere") for o, _ in _objects(doc, k) if o["flags"]["bits"] & 1]
        assert 1 <= len(lights) <= 3, seed
        light_kinds |= {(k, _is_identity(o)) for o, k in lights}
        roots.add("black" if doc["root_material"] == 0 else _kind_of(doc, doc["root_material"]))
        (_, cam), = _objects(doc, "Camera")
        focus.add(cam["focus"] is None)
    assert light_kinds == {("Rect", True), ("Cuboid", True), ("Rect", False)}      # aligned lamp, identity cuboid, rotated rect
    assert roots == {"black", "Flat", "Emissive"} and focus == {True, False}


def test_volume_rooms_hold_aligned_rows_and_a_volume(bendy):
    for seed in VOLUME_SEEDS:
        p, s = tables(bendy, f"volroom-{seed}")
        pi = p.view(np.int32)
        assert int(s["n_aan"].sum()) >= 3 and (pi[:, VOLUME] >= 0).sum() == 1, seed
        assert (pi[pi[:, VOLUME] >= 0, KIND] == SPHERE).all()


def test_limit_scenes_square_to_inf_and_to_zero(bendy):
    for kind, L in (("inf", np.float32(np.inf)), ("zero", np.float32(0.0))):
        p, s = tables(bendy, f"limit-{kind}")
        pi = p.view(np.int32)
        plain_aan, la = pi[:, KIND] == RECT_AAN, (pi[:, KIND] & SHAPE_MASK) == RECT_LA
        assert (p[plain_aan, W_SQR] == L).sum() == 1 and (p[la, H_SQR] == L).sum() == 1
        want = np.float32(np.inf) if kind == "inf" else np.float32(bendy.api.lib.bt_debug_abs_limit(0.0))
        assert ((s["aan"]["lim_a"] == want) | (s["aan"]["lim_b"] == want)).sum() == 1 and (s["la"]["lim"][:, 1] == want).sum() == 1
        assert 0 < bendy.api.lib.bt_debug_abs_limit(0.0) < 1e-22


def test_tie_scenes_put_two_rows_into_one_plane(bendy):
    for kind, order, frame in TIE_CASES:
        p, s = tables(bendy, "tie-%s-%d-%s" % (kind, order, frame))
        pi = p.view(np.int32)
        shape, obj = pi[:, KIND] & SHAPE_MASK, pi[:, OBJECT]
        first, second = sorted(set(obj.tolist()))
        want = {"identity": {RECT_AAN}, "rotated": {RECT_LA}, "generic": {RECT_AAN, RECT}}[frame]
        assert set(shape.tolist()) == want
        assert (frame == "generic") == (len(s["other"]) == 1)
        if frame == "rotated":
            assert (s["la"]["first_of_normal"] == 0).sum() >= 1
        # some row of the first object and some row of the second lie in one plane: same translation, same normal up to sign
        pairs = [(i, j) for i in np.flatnonzero(obj == first) for j in np.flatnonzero(obj == second)
                 if np.array_equal(bits(p[i, T:T + 3]), bits(p[j, T:T + 3])) and
                 (np.array_equal(p[i, C:C + 3], p[j, C:C + 3]) or np.array_equal(p[i, C:C + 3], -p[j, C:C + 3]))]
        assert pairs, (kind, order, frame)
        strictness = {(bool(pi[i, KIND] & STRICT), bool(pi[j, KIND] & STRICT)) for i, j in pairs}
        assert strictness == {"plain_plain": {(False, False)}, "strict_strict": {(True, True)},
                              "strict_plain": {(True, False)} if order == 0 else {(False, True)}}[kind]


# ---- the bundled scenes, as documented in DESIGN.md 5.6 ----------------------------------------------------------------
def test_bundled_rect_scenes_have_no_shared_normal(bendy, capsys):
    """`first_of_normal == 0` needs two BtRectLA rows with bit-identical world normals.  Cuboid::new (cuboid.rs:19-30) gives
    opposite faces opposite normals, so one rotated box has six runs of one row: the Cornell scenes never take that branch."""
    for case in ("bundled-cornell", "bundled-cornell2", "default"):
        _, s = tables(bendy, case)
        shared = int((s["la"]["first_of_normal"] == 0).sum())
        with capsys.disabled():
            print(f"\n{case}: n_aan {s['n_aan'].tolist()}, {len(s['la'])} LA rows, {shared} with first_of_normal == 0", end="")
        assert list(s["n_aan"]) == [4, 5, 3] and len(s["la"]) == 6 and shared == 0 and len(s["other"]) == 0


# ---- a wrong winner of a tie shows: the oracle alone ------------------------------------------------------------------------
def _albedo(oracle, txt, w=72, h=48, spp=4):
    osc = oracle.Scene(json.loads(txt))
    cam = osc.find_by_tag("camera")
    osc.set_camera_aspect(cam, w / h)
    img, _, _ = oracle.render(osc, cam, oracle.default_config(samples=spp, recursive=0, output=oracle.OUT_ALBEDO), w, h, 5, nthreads=8)
    return img


@pytest.mark.parametrize("kind,frame", sorted({(k, f) for k, _, f in TIE_CASES}))
def test_tie_order_decides_pixels(oracle, kind, frame):
    a, b = _albedo(oracle, tie_scene(kind, 0, frame)), _albedo(oracle, tie_scene(kind, 1, frame))
    flipped = int((a != b).any(axis=-1).sum())
    if kind == "strict_plain":                            # the plain rect wins in both orders, and it is seen
        removed = _albedo(oracle, without_tagged(tie_scene(kind, 0, frame), TIE_PLAIN_TAG))
        assert flipped == 0 and (a != removed).any(axis=-1).sum() >= 0.01 * a.shape[0] * a.shape[1]
        removed1 = _albedo(oracle, without_tagged(tie_scene(kind, 1, frame), TIE_PLAIN_TAG))
        assert (b != removed1).any(axis=-1).sum() >= 0.01 * a.shape[0] * a.shape[1]
    else:
        assert flipped >= 0.01 * a.shape[0] * a.shape[1], flipped
