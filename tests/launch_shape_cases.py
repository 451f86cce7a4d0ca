"""The launch-shape cases: renders whose bt_stats were recorded once on the MI355X into
tests/golden/launch_shapes.json (tools/record_launch_shapes.py).  tests/test_gpu_launch_shapes.py renders them again and
tests/test_launch_plan.py plans them without a GPU (bt_debug_plan_launch); both must give the recorded fields.

A case: a bundled scene, a frame, samples x Subpixel(subsample), and optionally `output` (Output value), `tuning` (bt_tuning
fields), `kind` ("plain", "guided" with `guides` = bit 0 albedo | bit 1 normal | bit 2 depth, or "adaptive"), `rank` / `world`
(a sharded render) and `lens` (Scene.set_lens arguments).  Every shape is the smallest that still reaches its branch of the
planner on the 256 CUs of the MI355X."""

FIELDS = ("slices", "launches", "packed", "workgroups", "scratch_bytes", "parked_bytes", "pixels", "samples")
KINDS = {"plain": 0, "guided": 1, "adaptive": 2}
LENS = dict(centre=(0.6, 0.4, 4.0), rs=0.15, step=0.1, radius=6.0, max_steps=800)


def _case(id, scene, width, height, samples, subsample=0, **more):
    return dict(id=id, scene=scene, width=width, height=height, samples=samples, subsample=subsample, **more)


CASES = [
    _case("scene_64x48_s1", "scene", 64, 48, 1),
    _case("scene_64x48_s64", "scene", 64, 48, 64),
    _case("scene_400x260_s1_n2", "scene", 400, 260, 1, 2),
    _case("cornell2_512x300_s4_full", "cornell2", 512, 300, 4),
    _case("cornell2_512x300_s4_albedo", "cornell2", 512, 300, 4, output=1),
    _case("cornell2_512x300_s128", "cornell2", 512, 300, 128),
    _case("volume_330x200_s5", "volume", 330, 200, 5),
    _case("volume_330x200_s5_packed1", "volume", 330, 200, 5, tuning={"packed": 1}),
    _case("cornell_330x200_s2_n3", "cornell", 330, 200, 2, 3),
    _case("cornell_330x200_s2_n3_rank1of3", "cornell", 330, 200, 2, 3, rank=1, world=3),
    # three samples' worth of scratch: 12 tiles x 256 pixels x 12 bytes per sample
    _case("scene_64x48_s12_cap3", "scene", 64, 48, 12, tuning={"scratch_cap_bytes": 3 * 12 * 256 * 12}),
    _case("cornell2_512x300_s4_guided_all", "cornell2", 512, 300, 4, kind="guided", guides=7),
    _case("cornell2_512x300_s4_guided_depth", "cornell2", 512, 300, 4, kind="guided", guides=4),
    _case("scene_330x200_s4_adaptive", "scene", 330, 200, 4, kind="adaptive"),
    _case("scene_128x96_s8_lens", "scene", 128, 96, 8, lens=LENS),
    _case("cornell2_330x200_s2_slices1", "cornell2", 330, 200, 2, tuning={"slices": 1}),
    _case("cornell2_330x200_s2_slices32", "cornell2", 330, 200, 2, tuning={"slices": 32}),
]


def case_scene(b, case):
    """A fresh Scene handle set up for `case`, and its camera."""
    from conftest import scene_path
    sc = b.Scene.load(scene_path(case["scene"]))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, case["width"] / case["height"])
    if case.get("tuning"):
        sc.set_tuning(**case["tuning"])
    if case.get("lens"):
        sc.set_lens(**case["lens"])
    return sc, cam


def case_configs(b, case):
    config = b.Config(chunks_x=8, chunks_y=4, output=b.Output(case.get("output", 0)))
    return config, b.RenderConfig(samples=case["samples"], subsample=b.Subsample(case["subsample"]))


def render_case(b, case):
    """Renders `case` on a fresh handle through the public API; the FIELDS of its bt_stats."""
    import torch
    sc, cam = case_scene(b, case)
    config, rc = case_configs(b, case)
    tr = b.Tracer.with_config(config)
    w, h, kind = case["width"], case["height"], case.get("kind", "plain")
    if case.get("world", 1) > 1:
        shard = b.new_shard(w, h, case["world"])
        tr.render_shard(sc, cam, rc, shard, w, h, case["rank"], case["world"])
    elif kind == "guided":
        guides = [b.Buffer.new(w, h) if case["guides"] >> g & 1 else None for g in range(3)]
        tr.render_guided(sc, cam, rc, b.Buffer.new(w, h), *guides)
    elif kind == "adaptive":
        tr.render_adaptive(sc, cam, rc, b.Buffer.new(w, h), b.Adaptive(w, h))
    else:
        tr.render(sc, cam, rc, b.Buffer.new(w, h))
    torch.cuda.synchronize()
    st = sc.last_stats()
    return {f: int(getattr(st, f)) for f in FIELDS}
