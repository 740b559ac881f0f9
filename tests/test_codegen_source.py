"""Code-generation guard for fpldpc_source.hip (the Philox channel kernel and its patch kernel for a bias), as
tests/test_codegen_bias.py: a device-only hipcc compile for gfx950 (tools/resource_usage.py), CPU only.  The unit
holds exactly these two kernels and is outside the kernel build id; neither kernel uses scratch, spills a VGPR or
an SGPR or needs LDS, and both fit 64 VGPRs, eight waves per SIMD ("A counter-based noise
source")."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
UNIT = "fpldpc_source.hip"
KERNELS = ("philox_channel_kernel", "philox_patch_kernel")
VGPRS = 64


@pytest.fixture(scope="module")
def usage():
    import resource_usage
    rows = resource_usage.usage(os.path.join(ROOT, "fixedpointldpc_amd", "csrc", UNIT))
    assert len(rows) == 2 and all(k in r["name"] for k, r in zip(KERNELS, rows)), [r["name"] for r in rows]
    return rows


@pytest.mark.parametrize("which", [0, 1], ids=KERNELS)
def test_kernels_without_scratch_spills_or_lds(usage, which):
    r = usage[which]
    assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    assert r["Dynamic Stack"] == "False" and int(r["LDS Size [bytes/block]"]) == 0, r
    assert int(r["VGPRs"]) <= VGPRS and int(r["AGPRs"]) == 0, r


def test_unit_is_built_outside_the_build_id():
    from fixedpointldpc_amd import _build
    assert UNIT in _build.SOURCES and UNIT not in _build.DEVICE_TUS and UNIT not in _build.HASHED_TUS
    assert UNIT not in _build.SOURCE_FLAGS
    # the Lehmer channel and its patch kernel stay in their own units: this one includes no other unit's source
    text = open(os.path.join(_build.CSRC, UNIT)).read()
    assert '.hip"' not in text
    assert text.count("__global__") == 2
