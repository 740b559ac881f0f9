"""fpldpc_flood_create_sat_placed (FloodSatDecoder(state=)): the entry point's signature and the validation of its
`state` argument, which comes with the width rules before a HIP device is looked for.  CPU only."""
import ctypes

import pytest


def test_signature(F):
    from fixedpointldpc_amd import _lib
    P, I32 = ctypes.c_void_p, ctypes.c_int32
    want = (ctypes.c_int, [P, ctypes.POINTER(_lib.Params), I32, I32, I32, ctypes.POINTER(P)])
    assert "fpldpc_flood_create_sat_placed" in _lib.EXPORTED and _lib.SIGNATURES["fpldpc_flood_create_sat_placed"] == want
    fn = F.lib().fpldpc_flood_create_sat_placed
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[1]
    assert F.FloodSatDecoder.STATES == {"lds": 0, "global": 1, "auto": 2}


@pytest.mark.parametrize("state", [3, -1])
def test_state_outside_the_three_values(F, state):
    """FPLDPC_ERR_ARG with the decoder's name, on a machine with or without a HIP device."""
    from fixedpointldpc_amd import _lib
    code = F.Code.array(13, 2)
    p = _lib.Params()
    F.lib().fpldpc_params_default(ctypes.byref(p))
    h = ctypes.c_void_p()
    st = F.lib().fpldpc_flood_create_sat_placed(code._h, ctypes.byref(p), 12, 10, state, ctypes.byref(h))
    assert st == -1 and not h.value
    with pytest.raises(F.FpldpcError) as e:
        _lib._check(st)
    assert e.value.code == -1 and str(e.value).count("saturated flooding decoder:") and f"state {state}" in str(e.value), e.value


def test_widths_are_still_validated_with_a_valid_state(F):
    with pytest.raises(F.FpldpcError) as e:
        F.FloodSatDecoder(F.Code.array(13, 2), post_bits=10, msg_bits=10, state="global")
    assert e.value.code == -1 and "saturated flooding decoder: need 2 <= msg_bits < post_bits <= 16" in str(e.value), e.value


@pytest.mark.parametrize("state", ["x", "LDS", "", None, 1])
def test_python_state_keyword(F, state):
    with pytest.raises(ValueError) as e:
        F.FloodSatDecoder(F.Code.array(13, 2), state=state)
    assert "state" in str(e.value)
