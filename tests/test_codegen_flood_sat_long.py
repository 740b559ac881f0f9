"""Code-generation guard for the global form of the saturated flooding decoder (fpldpc_flood_sat_global.hip), as
tests/test_codegen_flood_sat.py for its LDS form: a device-only hipcc compile for gfx950
(tools/resource_usage.py), CPU only.  The unit is outside the kernel build id, so this is what notices a change
to its register allocation.
  * Exactly the six kernels: {exact 47, 8, 16, 32, 48, 64}, table addressing only.
  * No instantiation uses scratch or spills a VGPR: the unrolled slot arrays (pk[DC], B[DC]) stay in registers
    (AGPRs may hold part of them, as in the LDS unit).
  * The DC = 47 and DC = 8 instantiations keep the VGPR count and the waves per SIMD of the build that ships
    (DESIGN.md "Saturated flooding decoder: state off chip").
  * The unit is built into the library and stays outside the kernel build id."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

UNIT = "fpldpc_flood_sat_global.hip"
WIDTHS = ["ILi47ELb1EE", "ILi8ELb0EE", "ILi16ELb0EE", "ILi32ELb0EE", "ILi48ELb0EE", "ILi64ELb0EE"]  # <DC, EXACT>
# flood_sat_global<DC, EXACT>: mangled-name fragment -> (max VGPRs, min waves / SIMD), as shipped
SHIPPED = {
    "flood_sat_globalILi47ELb1EE": (207, 2),
    "flood_sat_globalILi8ELb0EE": (64, 7),
}


@pytest.fixture(scope="module")
def usage():
    import resource_usage
    return resource_usage.usage(os.path.join(ROOT, "fixedpointldpc_amd", "csrc", UNIT))


def test_exactly_the_six_kernels(usage):
    names = [r["name"] for r in usage]
    assert len(names) == 6, names
    for w in WIDTHS:
        assert sum("flood_sat_global" + w in n for n in names) == 1, (w, names)


def test_no_scratch_and_no_vgpr_spills(usage):
    for r in usage:
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r


def test_shipped_register_budget(usage):
    for frag, (vmax, occ) in SHIPPED.items():
        rows = [r for r in usage if frag in r["name"]]
        assert len(rows) == 1, frag
        vg, oc = int(rows[0]["VGPRs"]), int(rows[0]["Occupancy [waves/SIMD]"])
        assert vg <= vmax and oc >= occ, (frag, vg, oc)


def test_the_unit_is_built_outside_the_build_id():
    from fixedpointldpc_amd import _build
    assert UNIT in _build.SOURCES and UNIT not in _build.HASHED_TUS and UNIT not in _build.SOURCE_FLAGS
