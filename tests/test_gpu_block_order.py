"""The cull builds take a launch's blocks in bt_block_order_kernel's order: traced blocks first, then the empty ones `slices`
at a time in fill workgroups, then workgroups that return at once.  The kernel's order must equal the
host's word for word, and frames AND segment counts must stay the oracle's bit for bit whatever the mix of the three kinds
of workgroup -- none traced, none filled, a partial last fill workgroup -- at every block size, on one handle through
every change that makes the order stale, and in shards with padded tile slots."""
import json

import numpy as np
import pytest

from block_order_cases import FILLS, LENGTHS, check_order, mask_array
from sphere_scenes import block_rects, sphere_scene

pytestmark = pytest.mark.gpu

FRAMES = [(61, 37), (96, 64)]          # ragged edge tiles | whole tiles
SLICES = [1, 4, 32]                    # blocks per fill workgroup: 1, 4, 32
SCENES = {"empty": ([0.0, 0.0, 6.0], 0.5),         # one small sphere behind the camera: every block empty
          "full": ([0.0, 0.0, -30.0], 29.0),       # a sphere that fills the view: no block of the frame empty
          "mixed": ([-1.2, 0.0, -6.0], 0.5)}       # a small sphere left of the centre: mostly sky


# ---- the kernel's order is the host's -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", FILLS)
def test_device_order_equals_host_order(bendy, fill):
    for n in LENGTHS:
        masks = mask_array(n, fill)
        host, host_header = bendy.Tracer.block_order(masks)
        dev, dev_header = bendy.Tracer.block_order(masks, device=True)
        assert dev_header == host_header, (n, dev_header, host_header)
        assert np.array_equal(dev, host), (n, int((dev != host).sum()))
        check_order(masks, dev, dev_header)


def test_device_order_of_a_c5_sized_launch(bendy):
    """518 400 masks (3840 x 2160 at 64-pixel blocks), the sky on top as in scene.json: 127 chunks of the scan."""
    n = 518400
    masks = mask_array(n, "random-0.5")
    masks[: n // 3] = 0
    host, host_header = bendy.Tracer.block_order(masks)
    dev, dev_header = bendy.Tracer.block_order(masks, device=True)
    assert dev_header == host_header and np.array_equal(dev, host)


# ---- frames and segment counts ------------------------------------------------------------------------------------------
def _doc(kind):
    """A camera at the origin looking down -z (the document of test_gpu_block_masks.py) and one sphere, see SCENES."""
    doc = json.loads(sphere_scene(4242, n_spheres=1, focus=False))
    centre, radius = SCENES[kind]
    for o in doc["objects"]["collection"].values():
        t = o["transform"]
        for name in ("transform_world", "transform_local"):
            if o["tag"] == "camera":
                t[name][:9] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
                t[name][9:12] = [0.0, 0.0, 0.0]
            else:
                t[name][9:12] = [float(v) for v in centre]
        if o["tag"] != "camera":
            o["inner"]["Sphere"]["radius"] = radius
    return doc


def _keys(doc):
    col = doc["objects"]["collection"]
    return (next(k for k, o in col.items() if o["tag"] == "camera"), next(k for k, o in col.items() if "Sphere" in o["inner"]))


_ORACLE = {}


def _oracle(oracle, doc, w, h, spp, n=0, output=0, bounces=None, sample_base=0):
    """(frame, segments) of the oracle's iterative form; computed once per distinct render and never written to."""
    key = (json.dumps(doc, sort_keys=True), w, h, spp, n, output, bounces, sample_base)
    if key not in _ORACLE:
        osc = oracle.Scene(doc)
        ocam = osc.find_by_tag("camera")
        osc.set_camera_aspect(ocam, w / h)
        cfg = oracle.default_config(samples=spp, subsample_n=n, output=output, recursive=0, sample_base=sample_base)
        if bounces is not None:
            cfg.max_bounces = cfg.max_volume_bounces = bounces        # (mod.rs:223-224: the override sets both)
        img, _, seg = oracle.render(osc, ocam, cfg, w, h, 3, nthreads=8)
        img.setflags(write=False)
        _ORACLE[key] = (img, seg)
    return _ORACLE[key]


def _handle(b, doc, slices):
    sc = b.Scene.from_json(json.dumps(doc))
    sc.set_tuning(slices=slices, packed=0)                 # small launches are otherwise packed and read no order
    return sc, sc.find_by_tag("camera")


def _render(b, sc, cam, w, h, spp, n=0, output=0, bounces=None, sample_base=0, buf=None):
    import torch
    sc.set_camera_aspect(cam, w / h)
    buf = buf if buf is not None else b.Buffer.new(w, h)
    tr = b.Tracer.with_config(b.Config(output=b.Output(output)))
    rc = b.RenderConfig(samples=spp, subsample=b.Subsample(n), **({} if bounces is None else dict(max_bounces=bounces)))
    tr.render(sc, cam, rc, buf, seed=3, sample_base=sample_base)
    torch.cuda.synchronize()
    return buf, sc.last_stats()


def _host_counts(b, sc, cam, w, h, slices, n=0, rank=0, world=1):
    """(masks, n_live, n_empty) of the launch, from the host's masks and the host's order."""
    sc.set_camera_aspect(cam, w / h)
    masks = b.Tracer().primary_masks(sc, cam, b.RenderConfig(samples=1, subsample=b.Subsample(n)), w, h, slices, rank, world)
    _, (n_live, n_empty) = b.Tracer.block_order(masks)
    return masks, n_live, n_empty


def _in_frame(w, h, slices, rank=0, world=1):
    return np.array([bool(r[2] and r[3]) for r in block_rects(w, h, slices, rank, world)])


@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("kind", list(SCENES))
def test_the_scenes_are_what_they_claim(bendy, kind, slices):
    """every block empty | no block with a pixel in the frame empty (none at all in the frame of whole tiles) | a mix whose
    empty blocks do not fill the last fill workgroup"""
    sc, cam = _handle(bendy, _doc(kind), slices)
    for w, h in FRAMES:
        for n in (0, 2):
            masks, n_live, n_empty = _host_counts(bendy, sc, cam, w, h, slices, n)
            inside = _in_frame(w, h, slices)
            assert not masks[~inside].any()
            if kind == "empty":
                assert n_live == 0 and n_empty == masks.size
            elif kind == "full":
                assert masks[inside].all() and n_live == int(inside.sum())
                assert n_empty == (0 if (w, h) == (96, 64) else int((~inside).sum()))
            else:
                assert n_live > 0 and n_empty > n_live
                if slices > 1:
                    assert n_empty % slices != 0, (w, h, n, n_empty)


@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("kind", list(SCENES))
def test_frames_and_segments_bit_exact(bendy, oracle, kind, slices):
    """Full, Albedo and Depth; both frames; Subsample 0 and 2; the default bounce limit and 0: every combination."""
    doc = _doc(kind)
    sc, cam = _handle(bendy, doc, slices)
    for output in (0, 1, 3):
        for w, h in FRAMES:
            for n, spp in ((0, 3), (2, 1)):
                for bounces in (None, 0):
                    buf, st = _render(bendy, sc, cam, w, h, spp, n=n, output=output, bounces=bounces)
                    assert st.slices == slices and not st.packed
                    want, seg = _oracle(oracle, doc, w, h, spp, n=n, output=output, bounces=bounces)
                    what = (kind, slices, output, w, h, n, bounces)
                    assert st.segments == seg, (what, st.segments, seg)
                    assert np.array_equal(buf.numpy(), want, equal_nan=True), what


@pytest.mark.parametrize("kind", list(SCENES))
def test_negative_bounce_limit_takes_no_shortcut(bendy, oracle, kind):
    """RenderConfig.max_bounces = -1 (the ABI's 0xffffffff): no block is filled, every block traces in launch order."""
    doc = _doc(kind)
    for slices in SLICES:
        sc, cam = _handle(bendy, doc, slices)
        for output in (0, 3):
            w, h = FRAMES[(slices + output) % 2]
            buf, st = _render(bendy, sc, cam, w, h, 2, output=output, bounces=-1)
            want, seg = _oracle(oracle, doc, w, h, 2, output=output, bounces=-1)
            assert st.segments == seg, (kind, slices, output, st.segments, seg)
            assert np.array_equal(buf.numpy(), want, equal_nan=True), (kind, slices, output)
            buf, st = _render(bendy, sc, cam, w, h, 2, output=output)              # ... and the shortcut again on that handle
            want, seg = _oracle(oracle, doc, w, h, 2, output=output)
            assert st.segments == seg and np.array_equal(buf.numpy(), want, equal_nan=True), (kind, slices, output)


def test_normal_output_is_as_it_was(bendy, oracle):
    """The Normal output's build reads neither masks nor order."""
    doc = _doc("mixed")
    sc, cam = _handle(bendy, doc, 4)
    for w, h in FRAMES:
        buf, st = _render(bendy, sc, cam, w, h, 3, output=2)
        want, seg = _oracle(oracle, doc, w, h, 3, output=2)
        assert st.segments == seg and np.array_equal(buf.numpy(), want, equal_nan=True), (w, h)


# ---- a stale order would show -------------------------------------------------------------------------------------------
def _set_t(doc, key, t):
    for name in ("transform_world", "transform_local"):
        doc["objects"]["collection"][key]["transform"][name][9:12] = [float(v) for v in np.asarray(t, np.float32)]


def test_one_handle_through_every_change(bendy, oracle):
    b = bendy
    doc = _doc("mixed")
    cam_key, sph_key = _keys(doc)
    sc, cam = _handle(b, doc, 4)
    w, h, spp = 96, 64, 2

    def check(what, w=w, h=h, spp=spp):
        buf, st = _render(b, sc, cam, w, h, spp)
        want, seg = _oracle(oracle, doc, w, h, spp)
        assert st.segments == seg, (what, st.segments, seg)
        assert np.array_equal(buf.numpy(), want, equal_nan=True), what
        return st

    # two progressive calls: the second reuses masks and order
    buf, st = _render(b, sc, cam, w, h, spp)
    assert st.segments == _oracle(oracle, doc, w, h, spp)[1]
    buf, st = _render(b, sc, cam, w, h, spp, sample_base=spp, buf=buf)
    assert st.segments == _oracle(oracle, doc, w, h, spp, sample_base=spp)[1]
    assert np.array_equal(buf.numpy(), _oracle(oracle, doc, w, h, 2 * spp)[0], equal_nan=True), "progressive"
    live0 = _host_counts(b, sc, cam, w, h, 4)[1]
    # the camera moves so that the sphere crosses to the other side of the frame: other blocks are live now
    _set_t(doc, cam_key, [-2.4, 0.0, 0.0])
    sc.debug_set_object(int(cam_key), [-2.4, 0.0, 0.0], 0.0)
    check("camera moved")
    # the sphere moves into the former sky and grows: more live blocks
    _set_t(doc, sph_key, [-0.9, 0.6, -5.0])
    doc["objects"]["collection"][sph_key]["inner"]["Sphere"]["radius"] = 1.25
    sc.debug_set_object(int(sph_key), [-0.9, 0.6, -5.0], 1.25)
    check("sphere moved")
    assert _host_counts(b, sc, cam, w, h, 4)[1] > live0
    # another frame size (fewer blocks: the buffers are kept, the order is not), and back
    check("frame size", w=61, h=37)
    check("frame size back")
    # several launches per render share one order
    per_sample = ((w + 15) // 16) * ((h + 15) // 16) * 256 * 12
    sc.set_tuning(scratch_cap_bytes=2 * per_sample)
    st = check("several launches", spp=6)
    assert st.launches == 3


# ---- shards -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_shards(bendy, oracle, world):
    """70 x 50 is 5 x 4 tiles: with 3 ranks the last rank's seventh tile slot has no tile.  Its blocks have no pixel in the
    frame: they are listed among the empty blocks, are filled with nothing and count nothing."""
    b = bendy
    import torch
    doc = _doc("mixed")
    w, h, spp, slices = 70, 50, 3, 4
    sc, cam = _handle(b, doc, slices)
    sc.set_camera_aspect(cam, w / h)
    want, seg = _oracle(oracle, doc, w, h, spp)
    tiles_x, n_tiles = (w + 15) // 16, ((w + 15) // 16) * ((h + 15) // 16)
    slots = (n_tiles + world - 1) // world
    total = 0
    for rank in range(world):
        masks, n_live, n_empty = _host_counts(b, sc, cam, w, h, slices, rank=rank, world=world)
        assert masks.size == slots * slices
        order, _ = b.Tracer.block_order(masks)
        padded = [s for s in range(slots) if s * world + rank >= n_tiles]
        assert bool(padded) == (world == 3 and rank == 2)
        for s in padded:
            assert not masks[s * slices:(s + 1) * slices].any()
            assert set(range(s * slices, (s + 1) * slices)) <= set(order[n_live:].tolist())
        shard = b.new_shard(w, h, world)
        b.Tracer().render_shard(sc, cam, b.RenderConfig.with_samples(spp), shard, w, h, rank, world, seed=3)
        torch.cuda.synchronize()
        total += sc.last_stats().segments
        got = shard.cpu().numpy().reshape(slots, 16, 16, 4)
        for s in range(slots):
            tile = s * world + rank
            if tile >= n_tiles:
                assert np.array_equal(got[s, :, :, :3], np.zeros((16, 16, 3), np.float32)), (rank, s)
                continue
            x0, y0 = (tile % tiles_x) * 16, (tile // tiles_x) * 16
            ref = want[y0:y0 + 16, x0:x0 + 16]
            assert np.array_equal(got[s, :ref.shape[0], :ref.shape[1]], ref, equal_nan=True), (rank, s)
    assert total == seg
