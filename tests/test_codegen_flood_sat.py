"""Code-generation guard for the saturated flooding decoder's unit (fpldpc_flood_sat.hip), as
tests/test_codegen_minsum.py for the min-sum units: a device-only hipcc compile for gfx950
(tools/resource_usage.py), CPU only.  The unit is outside the kernel build id, so this is what notices a change
to its register allocation.
  * 12 kernels: {47 exact, 8, 16, 32, 48, 64} x {computed addresses, index table}.
  * No instantiation uses scratch or spills a VGPR: the unrolled slot arrays (pk[DC], B[DC]) stay in registers.
  * The instantiations A / R (DC = 47, computed addresses), W (DC = 8, table) and the short array codes (DC = 8,
    computed) keep the VGPR count and the waves per SIMD of the build that ships (DESIGN.md "Saturated flooding
    decoder")."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

UNIT = "fpldpc_flood_sat.hip"
# flood_sat<DC, EXACT, COMPUTED>: mangled-name fragment -> (max VGPRs, min waves / SIMD), as shipped
SHIPPED = {
    "flood_satILi47ELb1ELb1EE": (197, 2),  # A, R
    "flood_satILi8ELb0ELb1EE": (79, 6),    # short array codes
    "flood_satILi8ELb0ELb0EE": (63, 7),    # W
}


@pytest.fixture(scope="module")
def usage():
    """the resource rows of the unit's 12 kernels"""
    import resource_usage
    rows = [r for r in resource_usage.usage(os.path.join(ROOT, "fixedpointldpc_amd", "csrc", UNIT)) if "flood_sat" in r["name"]]
    assert len(rows) == 12, [r["name"] for r in rows]
    return rows


def test_twelve_instantiations(usage):
    want = {f"flood_satILi{dc}ELb{int(dc == 47)}ELb{c}EE" for dc in (47, 8, 16, 32, 48, 64) for c in (0, 1)}
    for frag in want:
        assert sum(frag in r["name"] for r in usage) == 1, frag


def test_no_scratch_and_no_vgpr_spills(usage):
    for r in usage:
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r


def test_shipped_register_budget(usage):
    for frag, (vmax, occ) in SHIPPED.items():
        rows = [r for r in usage if frag in r["name"]]
        assert len(rows) == 1, frag
        vg, oc = int(rows[0]["VGPRs"]), int(rows[0]["Occupancy [waves/SIMD]"])
        assert vg <= vmax and oc >= occ, (frag, vg, oc)
