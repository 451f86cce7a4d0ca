"""The sphere-only render builds without volumes, lens or packing keep their Philox keys and a few launch constants out of
the SGPR file: the same operations on every (lane, sample), only their uniform operands live elsewhere.
Frame, running sums and the device's segment count must therefore equal the oracle's iterative form bit for bit -- on
tables of 1, 2, 3, 5 and 6 spheres (odd and even, the peeled last row), every material kind, focus on and off, two ragged
frame sizes, Subsample 0 and 2, outputs 0 - 3, seeds 0, 2^64 - 1 and 0x5EED, progressive calls, a two-rank shard, and a scene
whose tables take more than 20 KB of LDS (at most seven workgroups fit a CU).  Every launch here is an unpacked one."""
import json

import numpy as np
import pytest

from sphere_scenes import sphere_scene

pytestmark = pytest.mark.gpu

SPP = 5
SEEDS = [0, (1 << 64) - 1, 0x5EED]
SIZES = [(61, 37), (96, 64)]
# (scene seed, spheres, focus, size, Subsample, output, render seed): every value of every axis occurs, not their product
CASES = [(400 + i, n, bool(i & 1), SIZES[(i // 2) % 2], (0, 2)[(i // 3) % 2], i % 4, SEEDS[i % 3])
         for i, n in enumerate([1, 2, 3, 5, 6, 1, 2, 3, 5, 6, 5, 6])]


def _gpu(bendy, txt, w, h, spp, n=0, output=0, seed=3, sample_base=None, buf=None):
    import torch
    gs = bendy.Scene.from_json(txt)
    cam = gs.find_by_tag("camera")
    gs.set_camera_aspect(cam, w / h)
    buf = buf if buf is not None else bendy.Buffer.new(w, h)
    tr = bendy.Tracer.with_config(bendy.Config(output=bendy.Output(output)))
    tr.render(gs, cam, bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n)), buf, seed=seed, sample_base=sample_base)
    torch.cuda.synchronize()
    st = gs.last_stats()
    assert st.packed == 0                      # the builds this file is about
    return buf, st.segments


def _oracle(oracle, txt, w, h, spp, n=0, output=0, seed=3, sample_base=0):
    osc = oracle.Scene(json.loads(txt))
    ocam = osc.find_by_tag("camera")
    osc.set_camera_aspect(ocam, w / h)
    cfg = oracle.default_config(samples=spp, subsample_n=n, output=output, recursive=0, sample_base=sample_base)
    img, _, seg = oracle.render(osc, ocam, cfg, w, h, seed, nthreads=8)
    return img, seg


def _material_kinds(txt):
    doc = json.loads(txt)
    data = doc["data"]["collection"]
    used = {o["inner"]["Sphere"]["material"] for o in doc["objects"]["collection"].values() if "Sphere" in o["inner"]}
    used.add(doc["root_material"])
    return {next(iter(data[str(m)]["inner"]["Material"])) for m in used}


def test_the_cases_cover_every_axis():
    kinds = set().union(*[_material_kinds(sphere_scene(s, n_spheres=n, focus=f)) for s, n, f, *_ in CASES])
    assert kinds == {"Emissive", "Diffuse", "Metallic", "Glass", "Flat"}
    assert {c[1] for c in CASES} == {1, 2, 3, 5, 6} and {c[2] for c in CASES} == {False, True}
    assert {c[3] for c in CASES} == set(SIZES) and {c[4] for c in CASES} == {0, 2}
    assert {c[5] for c in CASES} == {0, 1, 2, 3} and {c[6] for c in CASES} == set(SEEDS)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "s%d-n%d-f%d-%dx%d-sub%d-out%d-seed%x" % (c[0], c[1], c[2], *c[3], c[4], c[5], c[6]))
def test_bit_exact_against_the_oracle(bendy, oracle, case):
    scene_seed, n_spheres, focus, (w, h), sub, output, seed = case
    txt = sphere_scene(scene_seed, n_spheres=n_spheres, focus=focus)
    buf, seg = _gpu(bendy, txt, w, h, SPP, n=sub, output=output, seed=seed)
    it, oseg = _oracle(oracle, txt, w, h, SPP, n=sub, output=output, seed=seed)
    assert seg == oseg
    assert np.array_equal(buf.numpy(), it, equal_nan=True)


@pytest.mark.parametrize("seed", SEEDS)
def test_two_progressive_calls(bendy, oracle, seed):
    txt = sphere_scene(431, n_spheres=5, focus=True)
    w, h = 61, 37
    buf, seg0 = _gpu(bendy, txt, w, h, 3, seed=seed)
    buf, seg1 = _gpu(bendy, txt, w, h, 2, seed=seed, sample_base=3, buf=buf)
    it, oseg = _oracle(oracle, txt, w, h, SPP, seed=seed)
    assert seg0 + seg1 == oseg
    assert np.array_equal(buf.numpy(), it)


def test_two_rank_shard(bendy, oracle):
    import torch
    txt = sphere_scene(432, n_spheres=6, focus=False)
    w, h, world = 61, 37, 2
    gs = bendy.Scene.from_json(txt)
    cam = gs.find_by_tag("camera")
    gs.set_camera_aspect(cam, w / h)
    tr = bendy.Tracer()
    shards, seg = [], 0
    for r in range(world):
        s = bendy.new_shard(w, h, world)
        tr.render_shard(gs, cam, bendy.RenderConfig.with_samples(SPP), s, w, h, r, world, seed=(1 << 64) - 1)
        torch.cuda.synchronize()
        seg += gs.last_stats().segments
        shards.append(s)
    out = bendy.Buffer.new(w, h)
    bendy.unshard(torch.cat(shards), out, world)
    torch.cuda.synchronize()
    it, oseg = _oracle(oracle, txt, w, h, SPP, seed=(1 << 64) - 1)
    assert seg == oseg
    assert np.array_equal(out.numpy(), it)


def test_tables_beyond_20_kb_of_lds(bendy, oracle):
    # 704 spheres: their LDS rows alone (32 bytes each) are 22 528 bytes, so seven workgroups are all a CU's 160 KB hold
    txt = sphere_scene(433, n_spheres=704, focus=True)
    w, h = 61, 37
    buf, seg = _gpu(bendy, txt, w, h, SPP, seed=0x5EED)
    it, oseg = _oracle(oracle, txt, w, h, SPP, seed=0x5EED)
    assert seg == oseg
    assert np.array_equal(buf.numpy(), it, equal_nan=True)
