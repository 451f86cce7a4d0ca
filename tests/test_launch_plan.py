"""The launch planner (bendy_tracer_amd/csrc/bt_plan.hpp) without a GPU: bt_debug_plan_launch runs fill_launch
and the planner for a device of a given CU count and returns the launch-shape fields of bt_stats.

Every case of launch_shape_cases.py must plan to what the MI355X recorded for it (tests/golden/launch_shapes.json, written by
the commit before the planner was split out of render_common).  The branches no render on a shared GPU can reach -- a failed
allocation, the 32-bit segment-counter clamp, the LDS refusal, the scratch's shrink policy -- are checked against what the
code states."""
import json
import os

import pytest

from conftest import GOLDEN
from helpers import flat_scene_json
from launch_shape_cases import CASES, FIELDS, KINDS, case_configs, case_scene

with open(os.path.join(GOLDEN, "launch_shapes.json")) as _f:
    GOLD = json.load(_f)
N_CU = GOLD["multi_processor_count"]
BY_ID = {c["id"]: c for c in CASES}
BT_ERR_INVALID_ARG, BT_ERR_DEVICE = -1, -8


def plan_case(b, case, alloc_limit=0, handle=None, n_cu=N_CU):
    sc, cam = handle or case_scene(b, case)
    config, rc = case_configs(b, case)
    world = case.get("world", 1)
    st = b.Tracer.with_config(config).plan_launch(sc, cam, rc, case["width"], case["height"], n_cu, rank=case.get("rank", 0),
                                                  world=world, sharded=world > 1, kind=KINDS[case.get("kind", "plain")],
                                                  guides=case.get("guides", 0), alloc_limit=alloc_limit)
    return {f: int(getattr(st, f)) for f in FIELDS}


def _tiles(case):
    return -(-case["width"] // 16) * -(-case["height"] // 16)


def test_recorded_file_covers_every_branch():
    rec = GOLD["cases"]
    assert set(rec) == set(BY_ID)
    assert {r["packed"] for r in rec.values()} == {0, 1, 2}
    assert any(r["launches"] > 1 for r in rec.values())
    assert len({r["slices"] for r in rec.values()}) >= 4
    for what in ("guided", "adaptive"):
        assert any(c.get("kind") == what for c in CASES)
    assert any(c.get("world", 1) > 1 for c in CASES) and any(c.get("lens") for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_plan_equals_recorded_shape(bendy, case):
    assert plan_case(bendy, case) == GOLD["cases"][case["id"]]


@pytest.mark.parametrize("samples,fits", [(64, 20), (12, 2.5), (7, 1)])
def test_failed_allocation_halves_the_samples_per_launch(bendy, samples, fits):
    """`fits` samples' worth of memory can be had: the samples per launch go c -> (c + 1) / 2 until they fit."""
    case = dict(BY_ID["scene_64x48_s64"], samples=samples)
    per_sample = _tiles(case) * 256 * 12
    chunk = samples
    while chunk * per_sample > fits * per_sample:
        chunk = (chunk + 1) // 2
    got = plan_case(bendy, case, alloc_limit=int(fits * per_sample))
    whole = plan_case(bendy, case)
    assert whole["launches"] == 1 and whole["scratch_bytes"] == samples * per_sample
    assert got["scratch_bytes"] == chunk * per_sample
    assert got["launches"] == -(-samples // chunk) > 1
    assert got["launches"] * chunk >= samples                     # every sample is covered
    assert (got["samples"], got["pixels"], got["parked_bytes"]) == (whole["samples"], whole["pixels"], whole["parked_bytes"])


def test_no_memory_for_one_sample_is_a_device_error(bendy):
    case = BY_ID["scene_64x48_s64"]
    with pytest.raises(bendy.BendyError) as e:
        plan_case(bendy, case, alloc_limit=_tiles(case) * 256 * 12 - 1)
    assert e.value.code == BT_ERR_DEVICE


def test_failed_packed_reservation_falls_back_to_the_unpacked_shape(bendy):
    """The unpacked size is reserved first and fits; the packed size (rows padded to a power of two, whole blocks per
    workgroup) is larger and does not: the plan is the one bt_tuning.packed = 0 gives."""
    case = BY_ID["cornell2_512x300_s4_full"]
    unpacked_bytes = _tiles(case) * 256 * case["samples"] * 12
    packed = plan_case(bendy, case)
    assert packed["packed"] == 2 and packed["scratch_bytes"] > unpacked_bytes
    got = plan_case(bendy, case, alloc_limit=unpacked_bytes)
    pinned = plan_case(bendy, dict(case, tuning={"packed": 0}))
    assert got["packed"] == 0 and got["scratch_bytes"] == unpacked_bytes and got["launches"] == 1
    assert got["workgroups"] == _tiles(case) * got["slices"]
    assert got == pinned


def test_pinned_shape_keeps_a_workgroups_segments_in_32_bits(bendy):
    """bt_tuning.slices = 1 (256 pixels per block) with an enormous scratch cap and sample count: pixels per block x samples
    per launch x the longest path ((max_bounces + 2) x (max_volume_bounces + 3) segments) stays below 2^32."""
    samples = 0x7fffffff
    case = dict(BY_ID["scene_64x48_s64"], samples=samples, tuning={"slices": 1, "scratch_cap_bytes": 1 << 62})
    got = plan_case(bendy, case)
    config, _ = case_configs(bendy, case)
    longest = (config.max_bounces + 2) * (config.max_volume_bounces + 3)
    assert got["slices"] == 1 and got["launches"] > 1
    # launches = ceil(samples / chunk)  =>  chunk <= (samples - 1) // (launches - 1)
    chunk_max = (samples - 1) // (got["launches"] - 1)
    assert 256 * chunk_max * longest < 1 << 32
    assert 256 * (chunk_max + 1) * longest * 2 > 1 << 32          # ... and not by a wide margin: the clamp, nothing coarser


def _many_spheres(n):
    ident = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    objs = {}
    for i in range(n):
        t = [float(i % 100) * 3.0, float(i // 100) * 3.0, -50.0]
        objs[str(2 + i)] = {"object_ref": 2 + i, "tag": None, "flags": {"bits": 0},
                            "transform": {"transform_world": ident + t, "transform_local": ident + t, "transform_parent": None},
                            "inner": {"Sphere": {"material": 2, "volume": None, "radius": 1.0}}, "children": None}
    return flat_scene_json(extra_objects=objs)


def test_scene_tables_beyond_158_kb_of_lds_are_refused(bendy):
    """32 bytes of LDS per primitive (BtPrimLite) + the materials: 4000 spheres fit, 5200 exceed 158 KB."""
    rc = bendy.RenderConfig(samples=1)
    for n, fits in ((4000, True), (5200, False)):
        sc = bendy.Scene.from_json(_many_spheres(n))
        cam = sc.find_by_tag("camera")
        if fits:
            assert bendy.Tracer.new().plan_launch(sc, cam, rc, 64, 48, N_CU).launches == 1
            continue
        with pytest.raises(bendy.BendyError) as e:
            bendy.Tracer.new().plan_launch(sc, cam, rc, 64, 48, N_CU)
        assert e.value.code == BT_ERR_INVALID_ARG and "LDS" in str(e.value)


def test_scratch_shrinks_at_the_eighth_small_request_in_a_row(bendy):
    """A handle keeps its scratch while a render needs at least a quarter of it; the eighth consecutive render that needs
    less gives it back (bt_plan.hpp scratch_serves).  Plans on one handle carry the scratch as renders do."""
    deep, quarter, small = (dict(BY_ID["scene_64x48_s64"], samples=s) for s in (64, 16, 1))
    per_sample = _tiles(deep) * 256 * 12
    handle = case_scene(bendy, deep)
    held = lambda case: plan_case(bendy, case, handle=handle)["scratch_bytes"]
    assert held(deep) == 64 * per_sample
    assert [held(small) for _ in range(7)] == [64 * per_sample] * 7
    assert held(quarter) == 64 * per_sample                       # a quarter of what is held: the streak starts again
    assert [held(small) for _ in range(7)] == [64 * per_sample] * 7
    assert held(small) == per_sample                              # the eighth
    assert held(deep) == 64 * per_sample                          # grows at once
    handle[0].trim()
    assert held(small) == per_sample                              # bt_scene_trim: from an empty scratch again
