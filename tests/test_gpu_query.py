"""The ray query API on the GPU (EXTENSION): bt_query_rays_device against the oracle's try_hit (tests/query_ref.py),
bit for bit; tails, degenerate rays, staleness; bt_view_rays_device against the camera rays of tests/sphere_scenes.py;
bt_scene_pick's known answer; bt_scene_set_camera_focus against the same document loaded with that focus."""
import json

import numpy as np
import pytest

import query_ref as q
import rect_scenes
import scene_gen
import sphere_scenes
from conftest import scene_path
from helpers import flat_scene_json

pytestmark = pytest.mark.gpu

NO_REF = q.NO_REF


def _query(b, sc, rays):
    import torch
    return b.hits_numpy(sc.query(torch.from_numpy(np.array(rays, np.float32)).cuda()))


def _assert_misses(hits):
    assert np.all(np.isposinf(hits["t"])) and np.all(hits["face"] == -1) and np.all(hits["prim"] == -1)
    for f in ("object_ref", "material_ref", "volume_ref"):
        assert np.all(hits[f] == NO_REF), f
    assert not hits["position"].any() and not hits["normal"].any()


def _assert_equal(hits, ref, doc):
    """Numerics contract N1 - N8: equality as float32 values (the sign of a zero is not compared)."""
    for f in ("t", "position", "normal", "face", "object_ref"):
        assert np.array_equal(hits[f], ref[f]), (f, int((hits[f] != ref[f]).sum()))
    miss = ref["face"] < 0
    _assert_misses(hits[miss])
    mats, vols = q.materials_of(doc), q.volumes_of(doc)
    for h in hits[~miss]:
        obj = int(h["object_ref"])
        assert int(h["material_ref"]) in mats[obj] and h["prim"] >= 0
        assert h["volume_ref"] == (NO_REF if vols.get(obj) is None else vols[obj])
        assert (h["face"] >= 3) == (vols.get(obj) is not None)


def _batch_conditions(ref, ties=False):
    share = float((ref["face"] >= 0).mean())
    assert 0.3 <= share <= 0.8, share
    if ties:
        assert int(ref["tie"].sum()) >= 100, int(ref["tie"].sum())


GENERATED = [(f"random{s}", lambda s=s: scene_gen.random_scene(s), s, False) for s in (0, 1, 3)] + \
            [(f"room{s}", lambda s=s: rect_scenes.room_scene(s), s, False) for s in list(rect_scenes.ROOM_SEEDS)[:3]] + \
            [("tie-" + "-".join(map(str, c)), lambda c=c: rect_scenes.tie_scene(*c), i, True) for i, c in enumerate(rect_scenes.TIE_CASES)]


@pytest.mark.parametrize("key,make,seed,ties", GENERATED, ids=[g[0] for g in GENERATED])
def test_query_equals_oracle_on_generated_scenes(bendy, oracle, key, make, seed, ties):
    text = make()
    rays, ref, doc = q.reference(oracle, key, text, seed, ties=ties)
    _batch_conditions(ref, ties)
    _assert_equal(_query(bendy, bendy.Scene.from_json(text), rays), ref, doc)


@pytest.mark.parametrize("name", ["scene", "cornell2", "volume"])
def test_query_equals_oracle_on_bundled_scenes(bendy, oracle, name):
    text = json.dumps(oracle.load_scene_json(scene_path(name)))
    rays, ref, doc = q.reference(oracle, name, text, 7)      # the scene's own object positions are the aim points
    _batch_conditions(ref)
    _assert_equal(_query(bendy, bendy.Scene.load(scene_path(name)), rays), ref, doc)


def test_query_tails_write_their_records_and_nothing_else(bendy, oracle):
    import torch
    text = rect_scenes.room_scene(0)
    rays, ref, doc = q.reference(oracle, "room0", text, 0)
    sc = bendy.Scene.from_json(text)
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    full = sc.query(d_rays).cpu().numpy()
    _assert_equal(full.reshape(-1).view(bendy.HIT_DTYPE), ref, doc)
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        out = torch.full((1024 + 8, 64), 0xAB, dtype=torch.uint8, device="cuda")
        sc.query(d_rays[:n], out=out[:n])
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], full[:n]), n
        assert np.all(got[n:] == 0xAB), n


def test_degenerate_rays_miss(bendy):
    sc = bendy.Scene.from_json(flat_scene_json())
    good = np.array([0, 0, 5, 0.01, 0, 0, -1, 1000.0], np.float32)
    assert _query(bendy, sc, good[None])["t"][0] == 4.0
    bad = []
    for col in (0, 1, 2, 3, 4, 5, 6):                        # origin, tmin, dir: NaN and both infinities
        for v in (np.nan, np.inf, -np.inf):
            r = good.copy()
            r[col] = v
            bad.append(r)
    r = good.copy(); r[7] = np.nan; bad.append(r)            # NaN tmax
    r = good.copy(); r[3], r[7] = 6.0, 5.0; bad.append(r)    # tmin > tmax
    bad = np.stack(bad)
    mixed = np.concatenate([bad, good[None]])                # a good ray in the same wave is not disturbed
    hits = _query(bendy, sc, mixed)
    _assert_misses(hits[:-1])
    assert hits["t"][-1] == 4.0 and hits["object_ref"][-1] == 1
    # tmax = +inf is allowed and hits what 1e30 hits
    a, c = good.copy(), good.copy()
    a[7], c[7] = np.inf, 1e30
    ha, hc = _query(bendy, sc, a[None]), _query(bendy, sc, c[None])
    assert ha.tobytes() == hc.tobytes() and ha["t"][0] == 4.0
    # a scene with only a camera misses everywhere
    doc = json.loads(flat_scene_json())
    del doc["objects"]["collection"]["1"]
    rays = q.recipe_rays(5, np.zeros((1, 3)), 300)
    _assert_misses(_query(bendy, bendy.Scene.from_json(json.dumps(doc)), rays))


def test_query_follows_a_moved_object_and_leaves_renders_alone(bendy, oracle):
    import torch
    text = sphere_scenes.sphere_scene(3, n_spheres=5, focus=False)
    doc = json.loads(text)
    sc = bendy.Scene.from_json(text)
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, 64 / 48)
    aims = q.aim_points(doc)
    rays = q.recipe_rays(11, aims, 600)
    before = _query(bendy, sc, rays)
    sphere = next(int(k) for k, o in sorted(doc["objects"]["collection"].items(), key=lambda kv: int(kv[0])) if "Sphere" in o["inner"])
    target = [0.5, 1.0, -0.5]
    sc.debug_set_object(sphere, target)
    for key in ("transform_world", "transform_local"):
        doc["objects"]["collection"][str(sphere)]["transform"][key][9:12] = target
    ref = q.try_hit(oracle, oracle.Scene(doc), rays)
    after = _query(bendy, sc, rays)
    _assert_equal(after, ref, doc)
    assert after.tobytes() != before.tobytes()               # the move is seen by these rays

    def render():
        buf = bendy.Buffer.new(64, 48)
        bendy.Tracer().render(sc, cam, bendy.RenderConfig(samples=4), buf, seed=77)
        torch.cuda.synchronize()
        return buf.numpy().copy(), sc.last_stats().segments

    f0, s0 = render()
    _assert_equal(_query(bendy, sc, rays), ref, doc)
    f1, s1 = render()
    assert f0.tobytes() == f1.tobytes() and s0 == s1


def test_view_rays(bendy):
    w, h = 40, 24
    text = sphere_scenes.sphere_scene(4, focus=True)
    doc = json.loads(text)
    sc = bendy.Scene.from_json(text)
    cam = sc.find_by_tag("camera")
    cam_ref = dict(sphere_scenes.camera_of(doc, 1.5), focus=None)
    py, px = [a.reshape(-1) for a in np.mgrid[0:h, 0:w]]
    for n, shift in ((0, 0.0), (2, 0.25)):                   # Subpixel(n) shifts the centre by (n - 1) / (2 n) of a pixel
        view = sc.camera_view(cam, bendy.Config(), bendy.RenderConfig(samples=1, subsample=bendy.Subsample(n)), w, h)
        rays = bendy.view_rays(view, 0, 0, w, h).cpu().numpy()
        assert np.array_equal(rays[:, 0:3], np.broadcast_to(view.matrix()[9:12], (w * h, 3)))
        assert np.all(rays[:, 3] == np.float32(0.01)) and np.all(rays[:, 7] == np.float32(1000.0))
        _, D = sphere_scenes.primary_rays(cam_ref, w, h, px.astype(np.float32) + np.float32(shift), py.astype(np.float32) + np.float32(shift),
                                          0, [(0.5, 0.5)], [])
        err = float(np.abs(rays[:, 4:7] - D).max())
        print(f"subsample {n}: largest direction difference {err:.3g}")
        # both sides are float32 trigonometry on unit-length quantities, each within a few ulp of 6e-8: 1e-6 is sixteen of them
        assert err <= 1e-6
        # a sub-rectangle's rays are the same pixels of the full frame, bit for bit
        x0, y0, rw, rh = 7, 5, 21, 13
        sub = bendy.view_rays(view, x0, y0, rw, rh).cpu().numpy().reshape(rh, rw, 8)
        assert sub.tobytes() == np.ascontiguousarray(rays.reshape(h, w, 8)[y0:y0 + rh, x0:x0 + rw]).tobytes()
    for rect in ((0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (0, 1, 1, h)):
        with pytest.raises(bendy.BendyError):
            bendy.view_rays(view, *rect)


def test_pick_known_answer(bendy):
    sc = bendy.Scene.from_json(flat_scene_json())
    cam = sc.find_by_tag("camera")
    cfg, rc = bendy.Config(), bendy.RenderConfig(samples=1)
    hit = sc.pick(cam, cfg, rc, 64, 64, 32, 32)
    # u = v = 0 gives the direction (0, 0, -1) and the quadratic is 25 - 24 = 1: all exact
    assert hit["t"] == 4.0 and hit["position"] == [0.0, 0.0, 1.0] and hit["normal"] == [0.0, 0.0, 1.0]
    assert hit["face"] == 0 and hit["object_ref"] == 1 and hit["material_ref"] == 2 and hit["volume_ref"] is None and hit["prim"] == 0
    assert hit["focus"] == 4.0
    off = sc.pick(cam, cfg, rc, 64, 64, 37, 29)              # off-centre, still on the sphere
    assert off is not None and off["object_ref"] == 1
    print("off-centre pick: focus", off["focus"], "against", 5.0 - off["position"][2])
    assert abs(off["focus"] - (5.0 - off["position"][2])) <= 1e-5 * (5.0 - off["position"][2])
    assert sc.pick(cam, cfg, rc, 64, 64, 0, 0) is None
    assert sc.pick(cam, cfg, rc, 64, 64, 63, 63) is None
    with pytest.raises(bendy.BendyError):
        sc.pick(cam, cfg, rc, 64, 64, 64, 0)


def test_set_camera_focus_renders_as_the_document_with_that_focus(bendy):
    import torch
    w, h, f = 64, 48, 3.5
    text = sphere_scenes.sphere_scene(6, n_spheres=6, focus=False)
    doc = json.loads(text)
    cam_key = next(k for k, o in doc["objects"]["collection"].items() if o["tag"] == "camera")
    assert doc["objects"]["collection"][cam_key]["inner"]["Camera"]["focus"] is None
    doc["objects"]["collection"][cam_key]["inner"]["Camera"]["focus"] = f

    def render(sc):
        cam = sc.find_by_tag("camera")
        sc.set_camera_aspect(cam, w / h)
        buf = bendy.Buffer.new(w, h)
        bendy.Tracer().render(sc, cam, bendy.RenderConfig(samples=4), buf, seed=0xF0C5)
        torch.cuda.synchronize()
        return buf.numpy().copy(), sc.last_stats().segments

    sc = bendy.Scene.from_json(text)
    plain = render(sc)                                        # the mask cache is warm
    sc.set_camera_focus(sc.find_by_tag("camera"), f)
    focused = render(sc)
    loaded = render(bendy.Scene.from_json(json.dumps(doc)))
    assert focused[0].tobytes() == loaded[0].tobytes() and focused[1] == loaded[1]
    assert focused[0].tobytes() != plain[0].tobytes()
    sc.set_camera_focus(sc.find_by_tag("camera"), None)
    again = render(sc)
    assert again[0].tobytes() == plain[0].tobytes() and again[1] == plain[1]
