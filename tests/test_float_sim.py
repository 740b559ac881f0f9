"""The simulation around the float decoder (fpldpc_float_ber_sim, fpldpc_float_ber_sim_source), what needs no GPU:
the shared-noise property of the two channels, the two symbols and their argument types, and the code-generation
guard of the kernel that writes the float run's forced positions (a device-only hipcc compile for gfx950,
tools/resource_usage.py, as tests/test_codegen_sim_source.py).  CPU only."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
SEED = 123456789
UNIT = "fpldpc_sim_source.hip"


@pytest.mark.parametrize("frac_bits", [0, 4, 8])
@pytest.mark.parametrize("source", ["lehmer", "philox"])
def test_float_and_fixed_channels_share_their_noise(F, source, frac_bits):
    """LLR_fp = (int)(LLR * 2^frac_bits) of the same double: frame f of a float run is frame f of a fixed run.
    A's n at 4.5 dB (the scaling by a power of two is exact, numpy's trunc is the cast's)."""
    n, frames, first = 2209, 5, 37
    snr, sigma = F.snr_sigma(4.5, 1978 / 2209)
    llr = F.channel_llr(SEED, first, frames, n, snr, sigma, frac_bits, dtype=np.float64, source=source)
    fixed = F.channel_llr(SEED, first, frames, n, snr, sigma, frac_bits, dtype=np.int16, source=source)
    scaled = np.trunc(llr * 2.0 ** frac_bits)
    assert np.abs(scaled).max() < 32768 and len(np.unique(fixed)) > 8
    assert (scaled.astype(np.int16) == fixed).all()
    # the double does not depend on frac_bits: one float run stands beside the fixed runs of every frac_bits
    assert (llr == F.channel_llr(SEED, first, frames, n, snr, sigma, 4, dtype=np.float64, source=source)).all()


def test_symbols_and_argument_types(F):
    from fixedpointldpc_amd import _lib
    L = F.lib()
    P, I32 = ctypes.c_void_p, ctypes.c_int32
    sp, res = ctypes.POINTER(_lib.SimParams), ctypes.POINTER(_lib.SimResult)
    assert L.fpldpc_float_ber_sim.restype is ctypes.c_int
    assert list(L.fpldpc_float_ber_sim.argtypes) == [P, sp, res] == list(L.fpldpc_ber_sim.argtypes)
    assert L.fpldpc_float_ber_sim_source.restype is ctypes.c_int
    assert list(L.fpldpc_float_ber_sim_source.argtypes) == [P, I32, sp, I32, I32, P, P, res, P]
    assert list(L.fpldpc_float_ber_sim_source.argtypes) == list(L.fpldpc_ber_sim_source.argtypes)
    header = open(os.path.join(ROOT, "include", "fpldpc.h")).read()
    assert "int fpldpc_float_ber_sim(fpldpc_decoder_t dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out);" in header
    assert "int fpldpc_float_ber_sim_source(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp," in header
    # null arguments are refused without a GPU
    assert L.fpldpc_float_ber_sim(None, None, None) == -1
    assert L.fpldpc_float_ber_sim_source(None, 0, None, F.FPLDPC_COLL_HOST, 0, None, None, None, None) == -1


def test_float_bp_belongs_to_the_flooding_decoder(F):
    """The keyword is refused by class, before any handle is touched."""
    from fixedpointldpc_amd import _lib
    for cls in (F.LayeredDecoder, F.MinSumDecoder, F.FloodSatDecoder):
        dec = cls.__new__(cls)  # no handle: the refusal is the class's
        with pytest.raises(TypeError, match="float_bp=True needs Decoder objects") as e:
            _lib._DecoderBase.ber_sim(dec, 1.0, 1.0, float_bp=True, max_frames=1)
        assert cls.__name__ in str(e.value)
        with pytest.raises(TypeError, match="float_bp=True needs Decoder objects"):
            F.ber_sim_multi([dec, dec], 1.0, 1.0, float_bp=True, max_frames=1)


@pytest.fixture(scope="module")
def usage():
    import resource_usage
    rows = resource_usage.usage(os.path.join(ROOT, "fixedpointldpc_amd", "csrc", UNIT))
    return [r for r in rows if "force_llr_f64_kernel" in r["name"]]


def test_force_kernel_codegen(usage):
    """One kernel, no scratch, no spills, no LDS, and the VGPR count as shipped."""
    assert len(usage) == 1, usage
    r = usage[0]
    assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    assert int(r["LDS Size [bytes/block]"]) == 0 and int(r["AGPRs"]) == 0, r
    assert int(r["VGPRs"]) == 13, r


def test_force_kernel_is_outside_the_build_id():
    from fixedpointldpc_amd import _build
    assert UNIT in _build.SOURCES and UNIT not in _build.DEVICE_TUS and UNIT not in _build.HASHED_TUS
    for hashed in ("fpldpc_gen.hip", "fpldpc_float.hip"):
        assert "force_llr_f64" not in open(os.path.join(_build.CSRC, hashed)).read()
