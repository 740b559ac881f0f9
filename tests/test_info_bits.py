"""The information-bit stream of a random_info simulation (fpldpc_info_bits_host) against the Lehmer recurrence
it is defined by, its argument rules, and the layout of fpldpc_sim_params against its ctypes mirror.  CPU only."""
import ctypes

import numpy as np
import pytest

M31 = 2**31 - 1


def recurrence(seed, first_frame, frames, k):
    """Bit i of frame f: the top bit of the state after draw f*k + i (s = s * 48271 mod 2^31 - 1)."""
    s = seed
    out = []
    for _ in range((first_frame + frames) * k):
        s = s * 48271 % M31
        out.append(s >> 30)
    return np.array(out[first_frame * k:], np.uint8).reshape(frames, k)


@pytest.mark.parametrize("seed,first,frames,k", [(987654321, 0, 5, 144), (987654321, 37, 3, 144), (1, 0, 70, 1),
                                                 (M31 - 1, 11, 2, 1978), (123456789, 3, 1, 1978), (42, 1000, 4, 7)])
def test_stream_is_the_recurrence(F, seed, first, frames, k):
    got = F.info_bits(seed, first, frames, k)
    assert got.dtype == np.uint8 and got.shape == (frames, k)
    assert (got == recurrence(seed, first, frames, k)).all()
    # the documented closed form
    for f, i in [(0, 0), (frames - 1, k - 1)]:
        assert got[f, i] == (F.rng_skip(seed, (first + f) * k + i + 1) >> 30) & 1


@pytest.mark.parametrize("seed,f0,frames,k", [(987654321, 37, 64, 144), (5, 1, 3, 1978), (77, 200, 9, 1)])
def test_a_block_is_rows_of_the_longer_block(F, seed, f0, frames, k):
    assert (F.info_bits(seed, f0, frames, k) == F.info_bits(seed, 0, f0 + frames, k)[f0:]).all()


def test_zero_frames(F):
    assert F.info_bits(1, 5, 0, 9).shape == (0, 9)


def test_bias(F):
    """Half the states are >= 2^30: the "uniform >= 1/2" rule (a ">> 31" or "& 1" slip shows here)."""
    share = F.info_bits(987654321, 0, 100, 2000).mean()
    assert abs(share - 0.5) <= 0.005, share


@pytest.mark.parametrize("args,ok", [((0, 0, 1, 8), False), ((M31, 0, 1, 8), False), ((1, 0, 1, 0), False),
                                     ((1, 0, -1, 8), False), ((1, -1, 1, 8), False),
                                     ((1, 2**48 - 1, 1, 1), False),       # the state after draw index 2^48 - 1: 2^48 draws
                                     ((1, 2**47, 1, 2), False), ((1, 2**62, 1, 4), False),
                                     ((1, 2**48 - 2, 1, 1), True), ((M31 - 1, 0, 1, 8), True)])
def test_argument_rules(F, args, ok):
    out = np.zeros((1, 8), np.uint8)
    st = F.lib().fpldpc_info_bits_host(*args, out.ctypes.data_as(ctypes.c_void_p))
    assert (st == 0) == ok and st in (0, -1), st
    if not ok:
        assert F.lib().fpldpc_last_error()
    else:
        assert out[0, 0] == (F.rng_skip(args[0], args[1] * args[3] + 1) >> 30) & 1
    # the device entry point refuses the same arguments before it touches HIP
    if not ok:
        assert F.lib().fpldpc_info_bits(*args, ctypes.c_void_p(8), None) == -1


def test_sim_params_layout_and_defaults(F):
    """fpldpc_sim_params_default on a SimParams inside a 0xAA-filled buffer: the C struct ends where the ctypes
    mirror ends, and every field holds its default."""
    from fixedpointldpc_amd._lib import SimParams
    size, pad = ctypes.sizeof(SimParams), 64
    buf = (ctypes.c_ubyte * (size + 2 * pad))(*([0xAA] * (size + 2 * pad)))
    p = SimParams.from_buffer(buf, pad)
    F.lib().fpldpc_sim_params_default(ctypes.byref(p))
    raw = bytes(buf)
    assert raw[:pad] == b"\xaa" * pad and raw[pad + size:] == b"\xaa" * pad
    assert p.random_info == 0 and p.info_seed == 987654321
    assert (p.seed, p.first_frame, p.snr, p.sigma, p.frac_bits) == (123456789, 0, 0.0, 0.0, 4)
    assert (p.codeword, p.info_index, p.info_bits, p.k, p.forced_index, p.n_forced, p.forced_llr) == (None, None, None, 0,
                                                                                                      None, 0, 0)
    assert (p.max_frame_errors, p.max_frames, p.count_mode, p.chunk, p.host_threads) == (100, 0, 0, 0, 0)
    assert (p.on_frame, p.on_frame_ctx, p.device_channel) == (None, None, 0)
    # the mirror's last fields sit where the header puts them: int32 after device_channel, then an aligned int64
    assert SimParams.random_info.offset == SimParams.device_channel.offset + 4
    assert SimParams.info_seed.offset == SimParams.random_info.offset + 4 + (-(SimParams.random_info.offset + 4)) % 8
    assert size == SimParams.info_seed.offset + 8


def test_python_defaults(F):
    p, _ = F._lib.sim_params(1.0, 1.0)
    assert p.random_info == 0 and p.info_seed == 987654321
    p, _ = F._lib.sim_params(1.0, 1.0, random_info=True, info_seed=5)
    assert p.random_info == 1 and p.info_seed == 5


def test_ber_sim_multi_refuses_a_mix_of_classes(F):
    class Fake:
        _h = None
    with pytest.raises(ValueError):
        F.ber_sim_multi([Fake(), Fake()], 1.0, 1.0)
    with pytest.raises(ValueError):
        F.ber_sim_multi([], 1.0, 1.0)
