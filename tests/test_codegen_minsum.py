"""Code-generation guard for the flooding min-sum kernels (fpldpc_minsum.hip), as tests/test_codegen.py for
the default kernels: a device-only hipcc compile for gfx950 (tools/resource_usage.py), CPU only.  The unit
is outside the kernel build id, so this is what notices a change to its register allocation.
  * No instantiation uses scratch or spills a VGPR: the unrolled slot arrays (pk[DC]) stay in registers.
  * The instantiations A / R (DC = 47, computed addresses) and W (DC = 8) keep the VGPR count and the waves
    per SIMD of the build that ships (DESIGN.md "Flooding min-sum decoder")."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
UNIT = os.path.join(ROOT, "fixedpointldpc_amd", "csrc", "fpldpc_minsum.hip")

# flood_minsum<DC, EXACT, COMPUTED>: mangled-name fragment -> (max VGPRs, min waves / SIMD), as shipped
SHIPPED = {
    "flood_minsumILi47ELb1ELb1EE": (142, 3),  # A, R
    "flood_minsumILi8ELb0ELb1EE": (60, 7),    # short array codes
    "flood_minsumILi8ELb0ELb0EE": (60, 7),    # W
}


@pytest.fixture(scope="module")
def usage():
    import resource_usage
    rows = [r for r in resource_usage.usage(UNIT) if "flood_minsum" in r["name"]]
    assert len(rows) == 12, [r["name"] for r in rows]  # {47 exact, 8, 16, 32, 48, 64} x {computed, table}
    return rows


def test_no_scratch_and_no_vgpr_spills(usage):
    for r in usage:
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r


def test_shipped_register_budget(usage):
    for frag, (vmax, occ) in SHIPPED.items():
        rows = [r for r in usage if frag in r["name"]]
        assert len(rows) == 1, frag
        vg, oc = int(rows[0]["VGPRs"]), int(rows[0]["Occupancy [waves/SIMD]"])
        assert vg <= vmax and oc >= occ, (frag, vg, oc)
