"""The harvest object of include/fpldpc.h without a device: the creation rules, what a fresh object reports, its
dimensions for two codes, and the ctypes signatures the binding declares.  CPU only."""
import ctypes

import numpy as np
import pytest


def create(F, code_handle, max_records):
    h = ctypes.c_void_p()
    st = F.lib().fpldpc_harvest_create(code_handle, max_records, ctypes.byref(h))
    return st, h


def test_creation_rules(F):
    lib = F.lib()
    code = F.Code.array(13, 2)
    for handle, cap in [(None, 10), (code._h, -1), (code._h, (1 << 20) + 1)]:
        st, h = create(F, handle, cap)
        assert st == -1 and not h.value and b"harvest" in lib.fpldpc_last_error(), (cap, lib.fpldpc_last_error())
    for cap in (0, 1, 1 << 20):
        st, h = create(F, code._h, cap)
        assert st == 0 and h.value
        lib.fpldpc_harvest_free(h)
    lib.fpldpc_harvest_free(None)  # as free(NULL)
    with pytest.raises(F.FpldpcError) as e:
        F.Harvest(code, -1)
    assert e.value.code == -1


def test_a_fresh_object_is_empty(F):
    lib = F.lib()
    hv = F.Harvest(F.Code.array(13, 2), 100)
    assert hv.counts == dict(frames=0, codeword_errors=0, detected=0, undetected=0, recorded=0, dropped=0)
    assert hv.classes == {}
    n = ctypes.c_int32(-1)
    assert lib.fpldpc_harvest_classes(hv._h, None, None, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.fpldpc_harvest_records(hv._h, 0, 0, *[None] * 7) == 0
    frame = np.zeros(1, np.int64)
    assert lib.fpldpc_harvest_records(hv._h, 0, 1, frame.ctypes.data_as(ctypes.c_void_p), *[None] * 6) == -1
    assert b"harvest" in lib.fpldpc_last_error()
    for first, count in [(-1, 0), (1, 0), (0, -1)]:
        assert lib.fpldpc_harvest_records(hv._h, first, count, *[None] * 7) == -1
    assert hv.frame.shape == (0,) and hv.err.shape == (0, 6) and hv.syn.shape == (0, 1)
    assert hv.err.dtype == np.uint32 and hv.frame.dtype == np.int64 and hv.weight.dtype == np.int32


def test_null_arguments(F):
    lib = F.lib()
    hv = F.Harvest(F.Code.array(13, 2), 1)
    dims, counts, n = np.zeros(4, np.int32), np.zeros(6, np.int64), ctypes.c_int32(0)
    assert lib.fpldpc_harvest_dims(None, dims.ctypes.data_as(ctypes.c_void_p)) == -1
    assert lib.fpldpc_harvest_dims(hv._h, None) == -1
    assert lib.fpldpc_harvest_counts(None, counts.ctypes.data_as(ctypes.c_void_p)) == -1
    assert lib.fpldpc_harvest_counts(hv._h, None) == -1
    assert lib.fpldpc_harvest_records(None, 0, 0, *[None] * 7) == -1
    assert lib.fpldpc_harvest_classes(None, None, None, None, 0, ctypes.byref(n)) == -1
    assert lib.fpldpc_harvest_classes(hv._h, None, None, None, 0, None) == -1
    # the scan's argument rules come before it looks for a device
    assert lib.fpldpc_harvest_scan(None, None, None, 0, 0, None, None, None, None, None) == -1
    assert lib.fpldpc_harvest_scan(hv._h, None, None, 0, 1, None, None, None, None, None) == -1
    assert lib.fpldpc_harvest_scan(hv._h, None, None, 0, -1, None, None, None, None, None) == -1
    assert lib.fpldpc_harvest_scan(hv._h, None, None, 0, 0, None, None, None, None, None) == 0  # nothing to do


@pytest.mark.parametrize("p,r,dims", [(13, 2, (169, 26, 6, 1)), (47, 5, (2209, 235, 70, 8))])
def test_dims(F, p, r, dims):
    hv = F.Harvest(F.Code.array(p, r), 0)
    assert (hv.n, hv.m, hv.hard_words, hv.syn_words) == dims
    d = np.zeros(4, np.int32)
    assert F.lib().fpldpc_harvest_dims(hv._h, d.ctypes.data_as(ctypes.c_void_p)) == 0 and tuple(d) == dims


def test_a_simulation_without_a_harvest_object_is_refused_before_a_device_is_needed(F):
    """h = NULL: -1 with "harvest" in the message, on all three entry points (no decoder: "null argument" comes
    first only when there is no decoder list at all)."""
    lib = F.lib()
    p, r = F._lib.SimParams(), F._lib.SimResult()
    lib.fpldpc_sim_params_default(ctypes.byref(p))
    fake = (ctypes.c_void_p * 1)(None)
    for name in ("fpldpc_ber_sim_harvest", "fpldpc_layered_ber_sim_harvest", "fpldpc_minsum_ber_sim_harvest"):
        assert getattr(lib, name)(fake, 1, ctypes.byref(p), 2, None, ctypes.byref(r), None) == -1
        assert b"harvest" in lib.fpldpc_last_error()


def test_ctypes_signatures(F):
    lib = F.lib()
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    SP, SR = ctypes.POINTER(F._lib.SimParams), ctypes.POINTER(F._lib.SimResult)
    sim = (ctypes.c_int, [P, I32, SP, I32, P, SR, P])
    want = {
        "fpldpc_harvest_create": (ctypes.c_int, [P, I32, ctypes.POINTER(P)]),
        "fpldpc_harvest_free": (None, [P]),
        "fpldpc_harvest_scan": (ctypes.c_int, [P, P, P, I32, I32, P, P, P, P, P]),
        "fpldpc_ber_sim_harvest": sim,
        "fpldpc_layered_ber_sim_harvest": sim,
        "fpldpc_minsum_ber_sim_harvest": sim,
        "fpldpc_harvest_dims": (ctypes.c_int, [P, P]),
        "fpldpc_harvest_counts": (ctypes.c_int, [P, P]),
        "fpldpc_harvest_records": (ctypes.c_int, [P, I64, I64, P, P, P, P, P, P, P]),
        "fpldpc_harvest_classes": (ctypes.c_int, [P, P, P, P, I32, ctypes.POINTER(I32)]),
    }
    for name, (res, args) in want.items():
        f = getattr(lib, name)
        assert f.restype == res and list(f.argtypes) == args, name
        assert name in F._lib.EXPORTED


def test_python_keywords(F):
    """harvest= is a keyword of every ber_sim and of ber_sim_multi, None by default."""
    import inspect
    for fn in (F.Decoder.ber_sim, F.LayeredDecoder.ber_sim, F.MinSumDecoder.ber_sim, F.ber_sim_multi):
        assert inspect.signature(fn).parameters["harvest"].default is None
