"""Launch shapes on the GPU: every case of launch_shape_cases.py, rendered on a fresh handle, must leave the bt_stats that
tests/golden/launch_shapes.json holds for it -- recorded on the MI355X by the commit before the launch planner was split out
of render_common (tools/record_launch_shapes.py).  No shape can change a pixel, so the parity suite cannot see a slip here."""
import json
import os

import pytest

from conftest import GOLDEN
from launch_shape_cases import CASES, render_case

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "launch_shapes.json")) as _f:
    GOLD = json.load(_f)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_render_leaves_the_recorded_shape(bendy, case):
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    if n_cu != GOLD["multi_processor_count"]:
        pytest.skip(f"the shapes were recorded on {GOLD['multi_processor_count']} CUs, this device has {n_cu}")
    assert render_case(bendy, case) == GOLD["cases"][case["id"]]
