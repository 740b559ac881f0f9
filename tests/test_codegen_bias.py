"""Code-generation guard for fpldpc_bias.hip (the patch kernel of mean-shift importance sampling), as
tests/test_codegen_harvest.py: a device-only hipcc compile for gfx950 (tools/resource_usage.py), CPU only.  The
unit is outside the kernel build id; the kernel uses no scratch, spills no VGPR or SGPR, needs no LDS and ships
with 64 VGPRs ("Importance sampling")."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
UNIT = "fpldpc_bias.hip"
KERNEL = "bias_patch_kernel"
VGPRS = 64  # as shipped; eight waves of a workgroup fit a SIMD pair at up to 128


@pytest.fixture(scope="module")
def usage():
    import resource_usage
    rows = resource_usage.usage(os.path.join(ROOT, "fixedpointldpc_amd", "csrc", UNIT))
    assert len(rows) == 1 and KERNEL in rows[0]["name"], [r["name"] for r in rows]  # and no other kernel
    return rows[0]


def test_patch_kernel_without_scratch_spills_or_lds(usage):
    r = usage
    assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    assert r["Dynamic Stack"] == "False" and int(r["LDS Size [bytes/block]"]) == 0, r
    assert int(r["VGPRs"]) <= VGPRS and int(r["AGPRs"]) == 0, r


def test_unit_is_built_outside_the_build_id():
    from fixedpointldpc_amd import _build
    assert UNIT in _build.SOURCES and UNIT not in _build.DEVICE_TUS and UNIT not in _build.HASHED_TUS
    assert UNIT not in _build.SOURCE_FLAGS
    # the channel unit keeps its own copy of the variate code: the patch kernel's unit includes no other unit's source
    text = open(os.path.join(_build.CSRC, UNIT)).read()
    assert '.hip"' not in text
