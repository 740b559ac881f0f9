"""Code-generation guard for the wide form of the two min-sum decoders (fpldpc_minsum_wide.hip), as
tests/test_codegen_minsum_long.py for their global form: a device-only hipcc compile for gfx950
(tools/resource_usage.py), CPU only.  The unit is outside the kernel build id, so this is what notices a
change to its register allocation.
  * Exactly the 4 kernels: each schedule with its state in LDS and in global memory.
  * None uses scratch or spills a VGPR: a chunk's 32 gathered values and the check's 8 sign words stay in
    registers (the sign words are selected by compare chains, never indexed at run time).
  * Each keeps the VGPR count and the waves per SIMD of the build that ships (DESIGN.md "Min-sum decoders:
    check degrees above 64")."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

UNIT = "fpldpc_minsum_wide.hip"
# kernel<GLOBAL>: mangled-name fragment -> (max VGPRs, min waves / SIMD), as shipped
SHIPPED = {
    "flood_minsum_wideILb0EE": (178, 2),
    "flood_minsum_wideILb1EE": (181, 2),
    "layered_minsum_wideILb0EE": (174, 2),
    "layered_minsum_wideILb1EE": (171, 2),
}


@pytest.fixture(scope="module")
def usage():
    import resource_usage
    return resource_usage.usage(os.path.join(ROOT, "fixedpointldpc_amd", "csrc", UNIT))


def test_exactly_the_four_kernels(usage):
    names = [r["name"] for r in usage]
    assert len(names) == 4, names
    for frag in SHIPPED:
        assert sum(frag in n for n in names) == 1, (frag, names)


def test_no_scratch_and_no_vgpr_spills(usage):
    for r in usage:
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r


def test_shipped_register_budget(usage):
    for frag, (vmax, occ) in SHIPPED.items():
        rows = [r for r in usage if frag in r["name"]]
        assert len(rows) == 1, frag
        vg, oc = int(rows[0]["VGPRs"]), int(rows[0]["Occupancy [waves/SIMD]"])
        assert vg <= vmax and oc >= occ, (frag, vg, oc)
