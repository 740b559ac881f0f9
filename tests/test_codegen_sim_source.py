"""Code-generation guard for fpldpc_sim_source.hip (the information-bit kernel and the count kernel of a
random_info simulation), as tests/test_codegen_minsum.py for the min-sum units: a device-only hipcc compile for
gfx950 (tools/resource_usage.py), CPU only.  The unit is outside the kernel build id; neither kernel uses
scratch, spills a VGPR or allocates LDS."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
UNIT = "fpldpc_sim_source.hip"


@pytest.fixture(scope="module")
def usage():
    import resource_usage
    rows = resource_usage.usage(os.path.join(ROOT, "fixedpointldpc_amd", "csrc", UNIT))
    return {k: [r for r in rows if k in r["name"]] for k in ("info_bits_kernel", "count_info_kernel")}


def test_two_kernels_without_scratch_or_spills(usage):
    for k, rows in usage.items():
        assert len(rows) == 1, (k, rows)
        r = rows[0]
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
        assert int(r["LDS Size [bytes/block]"]) == 0, r


def test_unit_is_built_outside_the_build_id():
    from fixedpointldpc_amd import _build
    assert UNIT in _build.SOURCES and UNIT not in _build.DEVICE_TUS and UNIT not in _build.HASHED_TUS
