"""Code-generation guard for fpldpc_harvest.hip (the scan kernel and the two kernels of the ordered compaction of
a harvesting simulation), as tests/test_codegen_sim_source.py: a device-only hipcc compile for gfx950
(tools/resource_usage.py), CPU only.  The unit is outside the kernel build id; no kernel uses scratch or spills
a VGPR or an SGPR."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
UNIT = "fpldpc_harvest.hip"
KERNELS = ("harvest_scan_kernel", "harvest_index_kernel", "harvest_gather_kernel")


@pytest.fixture(scope="module")
def usage():
    import resource_usage
    rows = resource_usage.usage(os.path.join(ROOT, "fixedpointldpc_amd", "csrc", UNIT))
    assert len(rows) == len(KERNELS), [r["name"] for r in rows]  # and no other kernel
    return {k: [r for r in rows if k in r["name"]] for k in KERNELS}


def test_three_kernels_without_scratch_or_spills(usage):
    for k, rows in usage.items():
        assert len(rows) == 1, (k, rows)
        r = rows[0]
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    # the scan stages a frame's hard words in dynamic LDS; the gather uses none
    assert int(usage["harvest_gather_kernel"][0]["LDS Size [bytes/block]"]) == 0


def test_unit_is_built_outside_the_build_id():
    from fixedpointldpc_amd import _build
    assert UNIT in _build.SOURCES and UNIT not in _build.DEVICE_TUS and UNIT not in _build.HASHED_TUS
    assert UNIT not in _build.SOURCE_FLAGS
