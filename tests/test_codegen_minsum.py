"""Code-generation guard for the two min-sum units (fpldpc_minsum.hip: flooding; fpldpc_layered_minsum.hip:
layered), as tests/test_codegen.py for the default kernels: a device-only hipcc compile for gfx950
(tools/resource_usage.py), CPU only.  Both units are outside the kernel build id, so this is what notices a
change to their register allocation (they share the check rule of fpldpc_minsum_device.hpp).
  * No instantiation uses scratch or spills a VGPR: the unrolled slot arrays (pk[DC]) stay in registers.
  * The instantiations A / R (DC = 47, computed addresses) and W (DC = 8) keep the VGPR count and the waves
    per SIMD of the build that ships (DESIGN.md "Flooding min-sum decoder", "Layered min-sum decoder")."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

# unit -> kernel<DC, EXACT, COMPUTED>: mangled-name fragment -> (max VGPRs, min waves / SIMD), as shipped
SHIPPED = {
    "fpldpc_minsum.hip": {
        "flood_minsumILi47ELb1ELb1EE": (142, 3),  # A, R
        "flood_minsumILi8ELb0ELb1EE": (60, 7),    # short array codes
        "flood_minsumILi8ELb0ELb0EE": (60, 7),    # W
    },
    "fpldpc_layered_minsum.hip": {
        "layered_minsumILi47ELb1ELb1EE": (141, 3),  # A, R
        "layered_minsumILi8ELb0ELb1EE": (73, 6),    # short array codes
        "layered_minsumILi8ELb0ELb0EE": (72, 7),    # W
    },
}


@pytest.fixture(scope="module")
def usage():
    """unit -> the resource rows of its 12 kernels"""
    import resource_usage
    out = {}
    for unit, shipped in SHIPPED.items():
        kernel = next(iter(shipped)).split("IL")[0]
        rows = [r for r in resource_usage.usage(os.path.join(ROOT, "fixedpointldpc_amd", "csrc", unit)) if kernel in r["name"]]
        assert len(rows) == 12, (unit, [r["name"] for r in rows])  # {47 exact, 8, 16, 32, 48, 64} x {computed, table}
        out[unit] = rows
    return out


def test_no_scratch_and_no_vgpr_spills(usage):
    for rows in usage.values():
        for r in rows:
            assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r


def test_shipped_register_budget(usage):
    for unit, shipped in SHIPPED.items():
        for frag, (vmax, occ) in shipped.items():
            rows = [r for r in usage[unit] if frag in r["name"]]
            assert len(rows) == 1, frag
            vg, oc = int(rows[0]["VGPRs"]), int(rows[0]["Occupancy [waves/SIMD]"])
            assert vg <= vmax and oc >= occ, (frag, vg, oc)
