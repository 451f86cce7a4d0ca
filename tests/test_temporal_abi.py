"""Temporal accumulation (EXTENSION) on a machine without a GPU: what bt_temporal_accumulate_device refuses before
it touches the device and in which order, the defaults, the handle's life cycle, bt_scene_camera_view against the scene files
and bt_scene_set_camera_pose."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import scene_path
from helpers import flat_scene_json

ALL_SCENES = ["scene", "cornell", "cornell2", "volume", "cloud"]
FAKE = [0x10000, 0x20000, 0x30000, 0x40000]        # never dereferenced: every call below fails before the device is touched


def _view(bendy, w=8, h=8):
    s = bendy.Scene.load(scene_path("scene"))
    return s.camera_view(s.find_by_tag("camera"), bendy.Config(), bendy.RenderConfig(), w, h)


def _call(bendy, t, view, color=FAKE[0], nc=1, normal=FAKE[1], nn=1, depth=FAKE[2], nd=1, out=FAKE[3], params=None):
    lib = bendy.api.lib
    p = None if params is None else C.byref(bendy.api._CTemporalParams(*params))
    rc = lib.bt_temporal_accumulate_device(t, None if view is None else C.byref(view), color, nc, normal, nn, depth, nd, out, p, None)
    return rc, lib.bt_last_error().decode()


def test_defaults_and_python_mirror(bendy):
    p = bendy.api._CTemporalParams()
    bendy.api.lib.bt_temporal_params_default(C.byref(p))
    assert (p.alpha_min, p.max_history, p.depth_tolerance, p.normal_min) == (np.float32(0.05), 256.0, np.float32(0.05), 0.5)
    bendy.api.lib.bt_temporal_params_default(None)
    q = bendy.TemporalParams(max_history=8)
    assert (q.alpha_min, q.max_history, q.normal_min) == (p.alpha_min, 8, p.normal_min)
    assert C.sizeof(bendy.View) == 76 and C.sizeof(bendy.api._CTemporalParams) == 16


def test_new_reset_free_without_a_device(bendy):
    lib = bendy.api.lib
    assert not lib.bt_temporal_new(0, 4) and lib.bt_last_error_code() == -1
    assert not lib.bt_temporal_new(4, 0)
    assert not lib.bt_temporal_new(1 << 16, 1 << 16)
    t = lib.bt_temporal_new(5, 3)
    assert t
    assert lib.bt_temporal_reset(t) == 0
    assert lib.bt_debug_temporal_history(t, None, 0) == 5 * 3 * 4
    host = np.ones(60, dtype=np.float32)
    assert lib.bt_debug_temporal_history(t, host.ctypes.data_as(C.POINTER(C.c_float)), 60) == 60 and (host == 0).all()
    lib.bt_temporal_free(t)
    lib.bt_temporal_free(None)
    assert lib.bt_temporal_reset(None) == -1
    h = bendy.Temporal(5, 3, alpha_min=0.25)
    assert h.history().shape == (3, 5, 4) and not h.history().any()
    h.reset()
    h.close()
    h.close()
    with pytest.raises(bendy.BendyError) as e:
        bendy.Temporal(0, 3)
    assert e.value.code == -1


def test_validation_order(bendy):
    """Each rule alone, and each rule together with a violation of every later one: the earlier rule's message wins."""
    lib = bendy.api.lib
    t = C.c_void_p(lib.bt_temporal_new(8, 8))
    good = _view(bendy)

    def view_with(**kw):
        v = good.copy()
        for k, val in kw.items():
            if k == "m":
                v.to_world[val[0]] = val[1]
            else:
                setattr(v, k, val)
        return v

    singular = good.copy()
    for i in range(3):
        singular.to_world[6 + i] = singular.to_world[i]            # column z = column x
    # (arguments that break the rule, a word of its message), in the header's order
    rules = [
        [dict(t=None), dict(view=None), dict(color=None), dict(depth=None), dict(out=None)],
        [dict(nc=0), dict(nn=0), dict(nd=0)],
        [dict(view=view_with(width=9)), dict(view=view_with(height=7))],
        [dict(view=view_with(m=(3, float("nan")))), dict(view=view_with(m=(10, float("inf")))), dict(view=view_with(yfov=0.0)),
         dict(view=view_with(xfov=-0.5)), dict(view=view_with(xfov=float("nan"))), dict(view=view_with(clip_max=good.clip_min)),
         dict(view=view_with(clip_min=float("inf"))), dict(view=singular)],
        [dict(params=(-0.1, 256, 0.05, 0.9)), dict(params=(1.5, 256, 0.05, 0.9)), dict(params=(float("nan"), 256, 0.05, 0.9)),
         dict(params=(0.05, 0.5, 0.05, 0.9)), dict(params=(0.05, float("inf"), 0.05, 0.9)), dict(params=(0.05, 256, -1e-3, 0.9)),
         dict(params=(0.05, 256, float("nan"), 0.9)), dict(params=(0.05, 256, 0.05, 1.5)), dict(params=(0.05, 256, 0.05, -1.5)),
         dict(params=(0.05, 256, 0.05, float("nan")))],
        [dict(out=FAKE[0]), dict(out=FAKE[1]), dict(out=FAKE[2])],
    ]
    words = ["null", "0 samples", "temporal handle of 8x8", "bt_view needs", "bt_temporal_params", "alias"]
    for k, cases in enumerate(rules):
        for case in cases:
            kw = dict(case)
            rc, msg = _call(bendy, kw.pop("t", t), kw.pop("view", good), **kw)
            assert rc == -1 and words[k] in msg, (case, msg)
            for later in range(k + 1, len(rules)):
                merged = {**rules[later][0], **case}
                if "view" in rules[later][0] and "view" in case:
                    continue
                rc, msg = _call(bendy, merged.pop("t", t), merged.pop("view", good), **merged)
                assert rc == -1 and words[k] in msg, (case, rules[later][0], msg)
    # a missing normal buffer is no error, whatever its count
    import torch
    if not torch.cuda.is_available():
        rc, msg = _call(bendy, t, good, normal=None, nn=0)
        assert rc == -8, msg
    lib.bt_temporal_free(t)


def test_valid_call_fails_loudly_without_gpu(bendy):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    t = C.c_void_p(bendy.api.lib.bt_temporal_new(8, 8))
    rc, msg = _call(bendy, t, _view(bendy))
    assert rc == -8, msg                                            # BT_ERR_DEVICE, as bt_denoise_device
    rc, msg = _call(bendy, t, _view(bendy), params=(0.0, 1.0, 0.0, -1.0))     # the ends of every range are inside it
    assert rc == -8, msg
    bendy.api.lib.bt_temporal_free(t)


@pytest.mark.parametrize("name", ALL_SCENES)
def test_camera_view_matches_scene_file(bendy, oracle, name):
    s, o = bendy.Scene.load(scene_path(name)), oracle.Scene.load(scene_path(name))
    cam, oc = s.find_by_tag("camera"), o._objects[o.find_by_tag("camera")]
    s.set_camera_aspect(cam, 1.5)
    cfg = bendy.Config(clip_min=0.25, clip_max=77.0)
    for n in (0, 1, 2, 3):
        v = s.camera_view(cam, cfg, bendy.RenderConfig(subsample=bendy.Subsample(n)), 48, 32)
        want = [getattr(getattr(oc.world, c), a) for c in ("cx", "cy", "cz", "t") for a in "xyz"]
        assert list(v.to_world) == want
        yfov = np.float32(2.0) * np.float32(math.atan2(oc.sensor_size, np.float32(2.0) * np.float32(oc.focal_length)))
        assert abs(v.yfov - yfov) <= 2 * np.spacing(np.float32(yfov)) and v.xfov == np.float32(v.yfov) * np.float32(1.5)
        assert (v.clip_min, v.clip_max, v.width, v.height, v.subsample_n) == (0.25, 77.0, 48, 32, n)


def test_camera_view_and_pose_errors(bendy):
    s = bendy.Scene.from_json(flat_scene_json())
    E = bendy.BendyError
    for call in (lambda ref: s.camera_view(ref, bendy.Config(), bendy.RenderConfig(), 8, 8),
                 lambda ref: s.set_camera_pose(ref, np.arange(12.0))):
        with pytest.raises(E) as e:
            call(1)                                                  # object 1 is a sphere
        assert e.value.code == -5
        with pytest.raises(E) as e:
            call(99)
        assert e.value.code == -4
    cam = s.find_by_tag("camera")
    with pytest.raises(E) as e:
        s.camera_view(cam, bendy.Config(), bendy.RenderConfig(), 0, 8)
    assert e.value.code == -1
    before = list(s.camera_view(cam, bendy.Config(), bendy.RenderConfig(), 8, 8).to_world)
    for bad in (float("nan"), float("inf")):
        m = np.array(before)
        m[7] = bad
        with pytest.raises(E) as e:
            s.set_camera_pose(cam, m)
        assert e.value.code == -1
    assert list(s.camera_view(cam, bendy.Config(), bendy.RenderConfig(), 8, 8).to_world) == before     # a refused pose changes nothing


def test_set_camera_pose_round_trips_and_keeps_planning(bendy):
    s = bendy.Scene.load(scene_path("scene"))
    cam = s.find_by_tag("camera")
    tr, rc = bendy.Tracer.new(), bendy.RenderConfig.with_samples_subsample(2, bendy.Subsample(2))
    plan0 = tr.plan_launch(s, cam, rc, 64, 48, 256)
    json0 = s.to_json()
    rng = np.random.default_rng(5)
    m = rng.standard_normal(12).astype(np.float32)
    m[5] = np.float32(-0.0)
    s.set_camera_pose(cam, m)
    v = s.camera_view(cam, bendy.Config(), rc, 64, 48)
    assert np.array_equal(v.matrix().view(np.uint32), m.view(np.uint32))          # bit for bit, -0.0 included
    plan1 = tr.plan_launch(s, cam, rc, 64, 48, 256)
    assert (plan1.pixels, plan1.samples, plan1.launches) == (plan0.pixels, plan0.samples, plan0.launches)
    assert s.to_json() == json0                                       # the pose is not written back into the document
    key0 = tr.mask_key(s, cam, rc, 64, 48, 4)
    s.set_camera_pose(cam, m + np.float32(0.5))
    assert tr.mask_key(s, cam, rc, 64, 48, 4) != key0                 # the block masks' key depends on the camera
