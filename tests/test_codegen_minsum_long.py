"""Code-generation guard for the global form of the two min-sum decoders (fpldpc_minsum_global.hip), as
tests/test_codegen_minsum.py for their LDS forms: a device-only hipcc compile for gfx950
(tools/resource_usage.py), CPU only.  The unit is outside the kernel build id, so this is what notices a
change to its register allocation.
  * Exactly the 12 kernels: {exact 47, 8, 16, 32, 48, 64} for each decoder, table addressing only.
  * No instantiation uses scratch or spills a VGPR: the unrolled slot arrays (pk[DC]) stay in registers.
  * The DC = 47 and DC = 8 instantiations keep the VGPR count and the waves per SIMD of the build that ships
    (DESIGN.md "Min-sum decoders: state off chip")."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

UNIT = "fpldpc_minsum_global.hip"
WIDTHS = ["ILi47ELb1EE", "ILi8ELb0EE", "ILi16ELb0EE", "ILi32ELb0EE", "ILi48ELb0EE", "ILi64ELb0EE"]  # <DC, EXACT>
# kernel<DC, EXACT>: mangled-name fragment -> (max VGPRs, min waves / SIMD), as shipped
SHIPPED = {
    "flood_minsum_globalILi47ELb1EE": (137, 3),
    "flood_minsum_globalILi8ELb0EE": (72, 7),
    "layered_minsum_globalILi47ELb1EE": (158, 3),
    "layered_minsum_globalILi8ELb0EE": (74, 6),
}


@pytest.fixture(scope="module")
def usage():
    import resource_usage
    return resource_usage.usage(os.path.join(ROOT, "fixedpointldpc_amd", "csrc", UNIT))


def test_exactly_the_twelve_kernels(usage):
    names = [r["name"] for r in usage]
    assert len(names) == 12, names
    for kernel in ("flood_minsum_global", "layered_minsum_global"):
        for w in WIDTHS:
            assert sum(kernel + w in n for n in names) == 1, (kernel + w, names)


def test_no_scratch_and_no_vgpr_spills(usage):
    for r in usage:
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r


def test_shipped_register_budget(usage):
    for frag, (vmax, occ) in SHIPPED.items():
        rows = [r for r in usage if frag in r["name"]]
        assert len(rows) == 1, frag
        vg, oc = int(rows[0]["VGPRs"]), int(rows[0]["Occupancy [waves/SIMD]"])
        assert vg <= vmax and oc >= occ, (frag, vg, oc)
