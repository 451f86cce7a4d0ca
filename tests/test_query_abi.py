"""The ray query API without a GPU (EXTENSION): struct sizes, every refusal of bt_query_rays_device,
bt_view_rays_device, bt_scene_pick and bt_scene_set_camera_focus in the header's order, the focus setter seen through the
block-mask key and the host's masks, and the compiler's resource remarks of bt_query.hip."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import sphere_scenes
from conftest import ROOT
from helpers import flat_scene_json

INVALID_ARG, INVALID_REF, NOT_CAMERA, DEVICE, UNSUPPORTED = -1, -4, -5, -8, -9


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


def test_struct_sizes(bendy):
    api = bendy.api
    assert C.sizeof(api._CRay) == 32 and C.sizeof(api._CHit) == 64
    assert bendy.RAY_DTYPE.itemsize == 32 and bendy.HIT_DTYPE.itemsize == 64
    for name, (_, offset) in ((n, bendy.HIT_DTYPE.fields[n][:2]) for n in bendy.HIT_DTYPE.names):
        assert getattr(api._CHit, name).offset == offset, name
    for name in bendy.RAY_DTYPE.names:
        assert getattr(api._CRay, name).offset == bendy.RAY_DTYPE.fields[name][1], name


def test_query_refusals_in_order(bendy):
    L = bendy.api.lib
    sc = bendy.Scene.from_json(flat_scene_json())
    h, A, B = sc._h, 0x1000, 0x2000                           # addresses that are never dereferenced: every call is refused first
    q = L.bt_query_rays_device
    # NULL first: also with everything else wrong
    assert q(None, 8, 1 << 30, 8, None) == INVALID_ARG and b"null" in L.bt_last_error()
    assert q(h, None, 1, B, None) == INVALID_ARG and q(h, A, 1, None, None) == INVALID_ARG
    # alignment and aliasing before the count and the lens
    sc.set_lens((0, 0, 0), 0.1, 0.05, 2.0)
    assert q(h, A + 8, 1 << 30, B, None) == INVALID_ARG and b"aligned" in L.bt_last_error()
    assert q(h, A, 1 << 30, B + 4, None) == INVALID_ARG and b"aligned" in L.bt_last_error()
    assert q(h, A, 1 << 30, A, None) == INVALID_ARG and b"two buffers" in L.bt_last_error()
    # the count before the lens
    assert q(h, A, 1 << 30, B, None) == INVALID_ARG and b"2^30" in L.bt_last_error()
    assert q(h, A, 0xFFFFFFFF, B, None) == INVALID_ARG
    # the lens before n == 0
    assert q(h, A, 0, B, None) == UNSUPPORTED and q(h, A, 5, B, None) == UNSUPPORTED
    sc.clear_lens()
    assert q(h, A, 0, B, None) == 0                           # nothing is launched, no device is touched


@pytest.mark.skipif(not _no_gpu(), reason="needs a machine without a GPU")
def test_valid_calls_without_a_device(bendy):
    L = bendy.api.lib
    sc = bendy.Scene.from_json(flat_scene_json())
    cam = sc.find_by_tag("camera")
    assert L.bt_query_rays_device(sc._h, 0x1000, 1, 0x2000, None) == DEVICE
    view = sc.camera_view(cam, bendy.Config(), bendy.RenderConfig(samples=1), 8, 8)
    assert L.bt_view_rays_device(C.byref(view), 0, 0, 8, 8, 0x1000, None) == DEVICE
    with pytest.raises(bendy.BendyError) as e:
        sc.pick(cam, bendy.Config(), bendy.RenderConfig(samples=1), 8, 8, 4, 4)
    assert e.value.code == DEVICE


def test_view_rays_refusals(bendy):
    L = bendy.api.lib
    sc = bendy.Scene.from_json(flat_scene_json())
    view = sc.camera_view(sc.find_by_tag("camera"), bendy.Config(), bendy.RenderConfig(samples=1), 32, 16)
    v = L.bt_view_rays_device
    assert v(None, 0, 0, 1, 1, 0x1000, None) == INVALID_ARG and v(C.byref(view), 0, 0, 1, 1, None, None) == INVALID_ARG
    assert v(C.byref(view), 0, 0, 1, 1, 0x1008, None) == INVALID_ARG
    for field, value in (("yfov", 0.0), ("xfov", float("nan")), ("clip_max", 0.01), ("width", 0)):      # what btview::prepare refuses
        bad = view.copy()
        setattr(bad, field, value)
        assert v(C.byref(bad), 0, 0, 1, 1, 0x1000, None) == INVALID_ARG, field
    bad = view.copy()
    for k in range(9):
        bad.to_world[k] = 0.0
    assert v(C.byref(bad), 0, 0, 1, 1, 0x1000, None) == INVALID_ARG
    for rect in ((0, 0, 0, 1), (0, 0, 1, 0)):
        assert v(C.byref(view), *rect, 0x1000, None) == INVALID_ARG and b"empty" in L.bt_last_error()
    for rect in ((32, 0, 1, 1), (0, 16, 1, 1), (1, 0, 32, 1), (0, 1, 1, 16), (31, 15, 2, 1), (0xFFFFFFFF, 0, 2, 1)):
        assert v(C.byref(view), *rect, 0x1000, None) == INVALID_ARG and b"32 x 16 frame" in L.bt_last_error(), rect


def test_pick_and_focus_refusals(bendy):
    L = bendy.api.lib
    sc = bendy.Scene.from_json(flat_scene_json())
    cam = sc.find_by_tag("camera")
    cfg, rc = bendy.Config(), bendy.RenderConfig(samples=1)
    c, r = bendy.api._c_configs(cfg, rc, 0)
    hit = bendy.api._CHit()
    assert L.bt_scene_pick(sc._h, cam, C.byref(c), C.byref(r), 8, 8, 1, 1, None, None) == INVALID_ARG
    assert L.bt_scene_pick(None, cam, C.byref(c), C.byref(r), 8, 8, 1, 1, C.byref(hit), None) == INVALID_ARG
    assert L.bt_scene_pick(sc._h, 99, C.byref(c), C.byref(r), 8, 8, 1, 1, C.byref(hit), None) == INVALID_REF
    assert L.bt_scene_pick(sc._h, 1, C.byref(c), C.byref(r), 8, 8, 1, 1, C.byref(hit), None) == NOT_CAMERA
    for x, y in ((8, 0), (0, 8)):
        assert L.bt_scene_pick(sc._h, cam, C.byref(c), C.byref(r), 8, 8, x, y, C.byref(hit), None) == INVALID_ARG
        assert b"8 x 8 frame" in L.bt_last_error()
    sc.set_lens((0, 0, 0), 0.1, 0.05, 2.0)
    assert L.bt_scene_pick(sc._h, cam, C.byref(c), C.byref(r), 8, 8, 1, 1, C.byref(hit), None) == UNSUPPORTED
    sc.clear_lens()

    f = L.bt_scene_set_camera_focus
    assert f(None, cam, 1, 2.0) == INVALID_ARG
    assert f(sc._h, 99, 1, 2.0) == INVALID_REF and f(sc._h, 1, 1, 2.0) == NOT_CAMERA
    assert f(sc._h, 99, 1, -1.0) == INVALID_REF and f(sc._h, 1, 1, float("nan")) == NOT_CAMERA     # the ref before the value
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert f(sc._h, cam, 1, bad) == INVALID_ARG, bad
    assert f(sc._h, cam, 0, float("nan")) == 0                # without has_focus the value is not looked at
    assert f(sc._h, cam, 1, 2.5) == 0
    # the saved JSON is not updated
    doc = json.loads(sc.to_json())
    assert doc["objects"]["collection"][str(cam)]["inner"]["Camera"]["focus"] is None


def test_focus_setter_changes_the_mask_key_and_the_masks(bendy):
    w, h, slices, f = 96, 64, 4, 2.25
    text = sphere_scenes.sphere_scene(2, n_spheres=6, focus=False, fstop=0.5)     # sphere-only: the build that culls
    doc = json.loads(text)
    cam_key = next(k for k, o in doc["objects"]["collection"].items() if o["tag"] == "camera")
    tr, rc = bendy.Tracer(), bendy.RenderConfig(samples=4)

    def load(t):
        sc = bendy.Scene.from_json(t)
        cam = sc.find_by_tag("camera")
        sc.set_camera_aspect(cam, w / h)
        return sc, cam

    sc, cam = load(text)
    k0, m0 = tr.mask_key(sc, cam, rc, w, h, slices), tr.primary_masks(sc, cam, rc, w, h, slices)
    sc.set_camera_focus(cam, f)
    k1, m1 = tr.mask_key(sc, cam, rc, w, h, slices), tr.primary_masks(sc, cam, rc, w, h, slices)
    assert k1 != k0                                           # masks cached under the old focus are not taken again
    doc["objects"]["collection"][cam_key]["inner"]["Camera"]["focus"] = f
    ref, ref_cam = load(json.dumps(doc))
    assert k1 == tr.mask_key(ref, ref_cam, rc, w, h, slices)
    assert np.array_equal(m1, tr.primary_masks(ref, ref_cam, rc, w, h, slices))
    sc.set_camera_focus(cam, None)
    assert tr.mask_key(sc, cam, rc, w, h, slices) == k0 and np.array_equal(tr.primary_masks(sc, cam, rc, w, h, slices), m0)


def test_query_kernels_use_no_scratch_and_spill_nothing():
    path = os.path.join(ROOT, "bendy_tracer_amd", "csrc", "build", "bt_query.resources.txt")
    assert os.path.exists(path), "the Makefile leaves bt_query.hip's resource remarks there"
    text = open(path).read()
    blocks = re.split(r"remark: Function Name: ", text)[1:]
    seen = {}
    for blk in blocks:
        name = blk.split()[0]
        field = lambda key: int(re.search(re.escape(key) + r"[^:]*: (\d+)", blk).group(1))
        seen[name] = (field("ScratchSize"), field("VGPRs Spill"), field("SGPRs Spill"))
    for kernel in ("bt_query_kernel", "bt_view_rays_kernel"):
        rows = [v for n, v in seen.items() if kernel in n]
        assert rows, (kernel, sorted(seen))
        assert all(scratch == 0 and vspill == 0 for scratch, vspill, _ in rows), (kernel, rows)
