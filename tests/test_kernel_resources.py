"""The register budgets of the sphere-only render builds without volumes, lens or packing, outputs 0 - 3,
read from the resource remarks the Makefile keeps next to the library's objects (build/bt_kernels.resources.txt, written by
the compiler when it builds bt_kernels.hip):

    .sgpr_count <= 80                  the granule up to which a CU admits EIGHT 256-thread workgroups (82 - 96: seven,
                                       whatever the occupancy line says; tools/residency_census.hip, profiles/r15/census.txt)
    .vgpr_count <= 64                  eight waves per SIMD
    private_segment_fixed_size == 0    no scratch
    sgpr_spill_count <= the parent's   27 / 27 / 33 / 32 for outputs 0 - 3 at 94 SGPRs (profiles/r15/kernel_resources.txt)

The other parent-relative figure, v_readlane inside the loop span, needs the assembly (tools/loop_spill_reloads.py) and
is logged in profiles/r15/kernel_resources.txt.  A missing artefact fails the test: the build has to leave it."""
import os
import re

import pytest

from conftest import ROOT

ARTEFACT = os.path.join(ROOT, "bendy_tracer_amd", "csrc", "build", "bt_kernels.resources.txt")
PARENT_SGPR_SPILLS = {0: 27, 1: 27, 2: 33, 3: 32}
FIELDS = {"TotalSGPRs": "sgpr_count", "VGPRs": "vgpr_count", "AGPRs": "agpr_count", "ScratchSize [bytes/lane]": "scratch",
          "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills", "Occupancy [waves/SIMD]": "occupancy"}


def _resources():
    assert os.path.exists(ARTEFACT), f"{ARTEFACT} is missing: `make -C bendy_tracer_amd/csrc` (build()) writes it"
    out, cur = {}, None
    for line in open(ARTEFACT):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


@pytest.fixture(scope="module")
def resources():
    return _resources()


def _name(output):
    return "_Z16bt_render_kernelILi%dELb0ELb0ELb0ELb0EEv8BtLaunch" % output


def test_the_artefact_lists_every_render_build(resources):
    names = [n for n in resources if "bt_render_kernel" in n]
    assert len(names) >= 60 and all(_name(o) in resources for o in range(4)), len(names)
    assert all(set(FIELDS.values()) <= set(resources[n]) for n in names)


@pytest.mark.parametrize("output", [0, 1, 2, 3])
def test_sphere_builds_fit_the_eight_workgroup_granules(resources, output):
    r = resources[_name(output)]
    print(output, r)
    assert r["sgpr_count"] <= 80
    assert r["vgpr_count"] + r["agpr_count"] <= 64
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0
    assert r["sgpr_spills"] <= PARENT_SGPR_SPILLS[output]
