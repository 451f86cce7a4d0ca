"""The per-block sphere masks are written by a kernel of their own (bt_block_mask_kernel) and kept on the scene handle
between renders.  The device masks must equal the host masks bit for bit -- both sides run
btcull::block_mask, the same IEEE f64 operations without contraction -- and a handle must never render with masks that
belong to another camera, scene, frame, Subsample, shard or launch shape: frames AND segment counts are compared with
the oracle after every such change on ONE handle."""
import json
import os

import numpy as np
import pytest

from sphere_scenes import sphere_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(40, 24), (37, 29), (48, 33), (23, 17)]


def _both(b, sc, cam, rc, w, h, slices, rank=0, world=1):
    tr = b.Tracer()
    return tr.primary_masks(sc, cam, rc, w, h, slices, rank, world), tr.block_masks_device(sc, cam, rc, w, h, slices, rank, world)


@pytest.mark.parametrize("w,h,spp", [(1920, 1080, 64), (3840, 2160, 256)])
def test_device_masks_equal_host_masks_c3_c5(bendy, w, h, spp):
    b = bendy
    sc = b.Scene.load(os.path.join(ROOT, "scenes", "scene.json.gz"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    for slices in (1, 2, 4, 8, 16, 32):
        host, dev = _both(b, sc, cam, b.RenderConfig.with_samples(spp), w, h, slices)
        assert host.shape == dev.shape
        assert np.array_equal(host, dev), (slices, int((host != dev).sum()))
    for world in (2, 3):
        for rank in range(world):
            host, dev = _both(b, sc, cam, b.RenderConfig.with_samples(spp), w, h, 8, rank, world)
            assert np.array_equal(host, dev), (world, rank)


def test_device_masks_equal_host_masks_random_scenes(bendy):
    """The 48 random scenes of the golden masks: focus on and off, every slice count, Subsample 1 / 2 / 3, and every
    scene once more as the shards of 2 and 3 ranks."""
    b = bendy
    some_empty = some_partial = 0
    for k in range(48):
        w, h = SIZES[k % 4]
        slices, n = [1, 2, 4, 8, 16, 32][k % 6], [0, 2, 3][k % 3]
        sc = b.Scene.from_json(sphere_scene(9000 + k, focus=bool(k & 1)))
        cam = sc.find_by_tag("camera")
        sc.set_camera_aspect(cam, w / h)
        rc = b.RenderConfig(samples=1, subsample=b.Subsample(n))
        host, dev = _both(b, sc, cam, rc, w, h, slices)
        assert np.array_equal(host, dev), k
        some_empty += int((host == 0).sum())
        some_partial += int(((host != 0) & (host != host.max())).sum())
        for world in (2, 3):
            for rank in range(world):
                host, dev = _both(b, sc, cam, rc, w, h, slices, rank, world)
                assert np.array_equal(host, dev), (k, world, rank)
    assert some_empty > 0 and some_partial > 0


# ---- a stale cache would show -------------------------------------------------------------------------------------------
def _oracle(oracle, doc, w, h, spp, n=0, output=0, seed=3):
    osc = oracle.Scene(doc)
    ocam = osc.find_by_tag("camera")
    osc.set_camera_aspect(ocam, w / h)
    cfg = oracle.default_config(samples=spp, subsample_n=n, output=output, recursive=0, sample_base=0)
    img, _, seg = oracle.render(osc, ocam, cfg, w, h, seed, nthreads=8)
    return img, seg


def _set_t(doc, key, t):
    tw = doc["objects"]["collection"][key]["transform"]
    for name in ("transform_world", "transform_local"):
        tw[name][9:12] = [float(v) for v in np.asarray(t, np.float32)]


class _Handle:
    """One GPU scene handle and the JSON document it stands for, changed together."""

    def __init__(self, b, oracle, doc):
        self.b, self.o, self.doc = b, oracle, doc
        self.sc = b.Scene.from_json(json.dumps(doc))
        self.cam = self.sc.find_by_tag("camera")
        self.cam_key = next(k for k, o in doc["objects"]["collection"].items() if o["tag"] == "camera")

    def move(self, key, t, radius=0.0):
        _set_t(self.doc, key, t)
        if radius:
            self.doc["objects"]["collection"][key]["inner"]["Sphere"]["radius"] = radius
        self.sc.debug_set_object(int(key), t, radius)

    def check(self, w, h, spp=3, n=0, output=0, what=""):
        import torch
        self.sc.set_camera_aspect(self.cam, w / h)
        buf = self.b.Buffer.new(w, h)
        tr = self.b.Tracer.with_config(self.b.Config(output=self.b.Output(output)))
        tr.render(self.sc, self.cam, self.b.RenderConfig(samples=spp, subsample=self.b.Subsample(n)), buf, seed=3, sample_base=0)
        torch.cuda.synchronize()
        seg = self.sc.last_stats().segments
        it, oseg = _oracle(self.o, self.doc, w, h, spp, n=n, output=output)
        assert seg == oseg, (what, seg, oseg)
        assert np.array_equal(buf.numpy(), it, equal_nan=True), what
        m = tr.primary_masks(self.sc, self.cam, self.b.RenderConfig(samples=spp, subsample=self.b.Subsample(n)), w, h, 4)
        return float((m == 0).mean())


def _one_sphere_doc():
    """A camera at the origin looking down -z and one small sphere far to the left of the view: most blocks are empty."""
    doc = json.loads(sphere_scene(4242, n_spheres=1, focus=False))
    col = doc["objects"]["collection"]
    cam_key = next(k for k, o in col.items() if o["tag"] == "camera")
    ident = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    for name in ("transform_world", "transform_local"):
        col[cam_key]["transform"][name][:9] = ident
    _set_t(doc, cam_key, [0, 0, 0])
    sph = next(k for k, o in col.items() if "Sphere" in o["inner"])
    col[sph]["inner"]["Sphere"]["radius"] = 0.5
    _set_t(doc, sph, [-1.2, 0.0, -6.0])
    return doc, sph


def test_a_stale_cache_would_show(bendy, oracle):
    b = bendy
    doc, sph = _one_sphere_doc()
    H = _Handle(b, oracle, doc)
    w, h = 80, 48
    e0 = H.check(w, h, what="first render")
    assert 0.3 < e0 < 1.0
    assert H.check(w, h, what="same again (cached masks)") == e0
    # the camera moves so that the sphere crosses to the other side of the frame: empty blocks become non-empty and
    # the other way round
    H.move(H.cam_key, [-2.4, 0.0, 0.0])
    H.check(w, h, what="camera moved")
    H.move(H.cam_key, [0.0, 0.0, 0.0])
    H.check(w, h, what="camera moved back")
    # a sphere moves into the former sky, then grows
    H.move(sph, [1.5, 0.6, -5.0])
    H.check(w, h, what="sphere moved")
    H.move(sph, [1.5, 0.6, -5.0], radius=1.25)
    H.check(w, h, what="sphere resized")
    # frame size, Subsample
    H.check(61, 37, what="frame size")
    H.check(w, h, what="frame size back")
    H.check(w, h, spp=1, n=2, what="Subsample(2)")
    H.check(w, h, spp=1, n=3, what="Subsample(3)")
    H.check(w, h, what="Subsample off")
    # Normal output (no masks) between two Full renders
    H.check(w, h, output=2, what="Normal")
    H.check(w, h, what="Full after Normal")
    H.check(w, h, output=1, what="Albedo")
    H.check(w, h, output=3, what="Depth")
    # pinned launch shapes
    for slices in (1, 16, 4):
        H.sc.set_tuning(slices=slices)
        H.check(w, h, what=f"slices {slices}")


def test_shard_then_full_frame_on_one_handle(bendy, oracle):
    import torch
    b = bendy
    doc, _ = _one_sphere_doc()
    H = _Handle(b, oracle, doc)
    w, h, spp = 70, 45, 3
    H.sc.set_camera_aspect(H.cam, w / h)
    it, _ = _oracle(oracle, doc, w, h, spp)
    tr = b.Tracer()
    for world in (2, 3):
        shards = []
        for r in range(world):
            s = b.new_shard(w, h, world)
            tr.render_shard(H.sc, H.cam, b.RenderConfig.with_samples(spp), s, w, h, r, world, seed=3)
            shards.append(s)
        out = b.Buffer.new(w, h)
        b.unshard(torch.cat(shards), out, world)
        torch.cuda.synchronize()
        assert np.array_equal(out.numpy(), it), world
        H.check(w, h, spp=spp, what=f"full frame after the shards of {world} ranks")


def test_second_stream_on_one_handle(bendy, oracle):
    import torch
    b = bendy
    doc, _ = _one_sphere_doc()
    H = _Handle(b, oracle, doc)
    w, h = 80, 48
    H.check(w, h, what="default stream")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        H.check(w, h, what="second stream, same key otherwise")
        H.move(H.cam_key, [-2.4, 0.0, 0.0])
        H.check(w, h, what="second stream, camera moved")
    torch.cuda.synchronize()
    H.check(w, h, what="back on the default stream")


def test_multi_launch_renders(bendy, oracle):
    """A scratch cap small enough to split a render into several launches: they share one mask computation."""
    import torch
    b = bendy
    doc, _ = _one_sphere_doc()
    H = _Handle(b, oracle, doc)
    w, h, spp = 80, 48, 12
    H.sc.set_camera_aspect(H.cam, w / h)
    per_sample = ((w + 15) // 16) * ((h + 15) // 16) * 256 * 12
    H.sc.set_tuning(scratch_cap_bytes=2 * per_sample)
    buf = b.Buffer.new(w, h)
    b.Tracer().render(H.sc, H.cam, b.RenderConfig.with_samples(spp), buf, seed=3, sample_base=0)
    torch.cuda.synchronize()
    st = H.sc.last_stats()
    assert st.launches == 6
    it, oseg = _oracle(oracle, doc, w, h, spp)
    assert st.segments == oseg
    assert np.array_equal(buf.numpy(), it)
