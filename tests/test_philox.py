"""The counter-based noise source on the host (include/fpldpc.h, FPLDPC_NOISE_PHILOX), CPU only: the Philox
primitive against known answers, the host twins of the channel and of the shifted channel against
tests/philox_model.py by its comparison rule, independence of the thread count and of how a frame range is split,
the statistics of the variates, the Lehmer source through the *_src host functions, and the argument rules."""
import ctypes

import numpy as np
import pytest

import bias_model as BM
import philox_model as PM

SNR, SIGMA = 2.3, 0.66
SEEDS = (123456789, 0, 2**40 + 7)
BUDGET = PM.Budget(2)  # boundary positions over everything this module compares

KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
# (seed, frame): the words of pairs 0 and 1, z[0..3]
RULE = [(123456789, 0, ("23bdfdf2 526f577f d3f04ad4 21a5ec5d", "7f4c1eda 011fd626 50ed66c5 2eb295cc"),
         (1.020584009206694, 1.106681836604068, 1.357521948786167, 3.002175634790103)),
        (2**40 + 7, 2**33 + 5, ("01689da7 57080f7d c70104b0 2bd89840", "3f7cd55b 66197544 ac60ba3e e221d03f"),
         (0.697347726090395, 1.292873198644735, 1.007601009333817, -0.907303975882482))]


def hexwords(w):
    return " ".join(f"{int(x):08x}" for x in w)


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(F, ctr, key, want):
    assert hexwords(F.philox4x32(ctr, key)) == want
    assert hexwords(PM.philox4x32(np.array(ctr), key)) == want


@pytest.mark.parametrize("seed,frame,want_words,want_z", RULE)
def test_rule_words_and_variates(F, seed, frame, want_words, want_z):
    for pair, want in enumerate(want_words):
        ctr = (pair, 0, frame & 0xFFFFFFFF, frame >> 32)
        assert hexwords(F.philox4x32(ctr, (seed & 0xFFFFFFFF, seed >> 32))) == want
        assert hexwords(PM.words(seed, frame, [pair])[0]) == want
    # snr = 0.5, sigma = 1, no codeword: LLR = 1 + z
    llr = F.channel_llr(seed, frame, 1, 4, 0.5, 1.0, dtype=np.float64, source="philox")[0]
    assert np.abs(llr - (1 + np.array(want_z))).max() <= 1e-12
    assert np.abs(PM.variates(seed, frame, 1, 4)[0] - np.array(want_z)).max() <= 1e-12


def codeword(n, with_cw):
    return np.random.default_rng(n).integers(0, 2, n).astype(np.uint8) if with_cw else None


@pytest.mark.parametrize("n", [1, 2, 25, 169, 2209])
@pytest.mark.parametrize("first", [0, 37, 2**33 + 5, 2**62])
def test_host_twin_against_the_model(F, n, first):
    frames = 5
    for k, seed in enumerate(SEEDS):
        cw = codeword(n, (k + n) % 2 == 0)
        model = PM.channel(seed, first, frames, n, SNR, SIGMA, 4, cw)
        assert np.abs(model["fp"]).max() <= 32767
        f64 = F.channel_llr(seed, first, frames, n, SNR, SIGMA, 4, cw, np.float64, source="philox")
        assert np.abs(f64 - model["llr"]).max() <= PM.f64_bound(SNR, SIGMA)
        i32 = F.channel_llr(seed, first, frames, n, SNR, SIGMA, 4, cw, np.int32, source="philox")
        PM.assert_fixed_equal(BUDGET, model, i32, SNR, SIGMA, 4, (n, first, seed))
        i16 = F.channel_llr(seed, first, frames, n, SNR, SIGMA, 4, cw, np.int16, source="philox")
        assert (i16 == i32).all()


@pytest.mark.parametrize("n", [1, 25, 2209])
@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.float64])
def test_split_and_threads_change_nothing(F, n, dtype):
    seed, a, b, c = 2**40 + 7, 2**33 + 5, 2**33 + 12, 2**33 + 38
    cw = codeword(n, True)
    whole = F.channel_llr(seed, a, c - a, n, SNR, SIGMA, 4, cw, dtype, nthreads=1, source="philox")
    parts = np.concatenate([F.channel_llr(seed, a, b - a, n, SNR, SIGMA, 4, cw, dtype, nthreads=1, source="philox"),
                            F.channel_llr(seed, b, c - b, n, SNR, SIGMA, 4, cw, dtype, nthreads=3, source="philox")])
    many = F.channel_llr(seed, a, c - a, n, SNR, SIGMA, 4, cw, dtype, nthreads=16, source="philox")
    assert whole.tobytes() == parts.tobytes() == many.tobytes()


def test_int16_overflow_is_an_error(F):
    with pytest.raises(F.FpldpcError, match="does not fit int16"):
        F.channel_llr(123456789, 0, 50, 25, 3.0, 0.5, 12, dtype=np.int16, source="philox")
    assert np.abs(F.channel_llr(123456789, 0, 50, 25, 3.0, 0.5, 12, dtype=np.int32, source="philox")).max() > 32767


def test_statistics(F):
    """2000 frames of 2209 values from the host channel (snr 0.5, sigma 1, no codeword: LLR = 1 + z): each figure
    within five of its own standard errors."""
    llr = F.channel_llr(123456789, 0, 2000, 2209, 0.5, 1.0, dtype=np.float64, source="philox")
    assert np.abs(llr[:40] - (1.0 + PM.variates(123456789, 0, 40, 2209))).max() <= PM.f64_bound(0.5, 1.0)  # the model's z
    z = llr - 1.0
    N = z.size
    assert abs(z.mean()) <= 5 / np.sqrt(N)
    assert abs(z.var() - 1) <= 5 * np.sqrt(2.0 / N)
    even, odd = z[:, 0:2208:2].ravel(), z[:, 1:2208:2].ravel()
    assert abs(np.corrcoef(even, odd)[0, 1]) <= 5 / np.sqrt(even.size)
    assert abs(np.corrcoef(z[:-1].ravel(), z[1:].ravel())[0, 1]) <= 5 / np.sqrt(z[1:].size)
    p = 6.334e-5  # P(|z| > 4)
    assert abs((np.abs(z) > 4).sum() - N * p) <= 5 * np.sqrt(N * p)


def test_lehmer_through_the_src_host_functions(F):
    L = F.lib()
    n, frames, first = 169, 7, 37
    cw = codeword(n, True)
    for dtype, t in ((np.int16, F.FPLDPC_LLR_I16), (np.int32, F.FPLDPC_LLR_I32), (np.float64, F.FPLDPC_LLR_F64)):
        want = F.channel_llr(123456789, first, frames, n, SNR, SIGMA, 4, cw, dtype)
        got = np.empty((frames, n), dtype)
        assert L.fpldpc_channel_llr_src_host(F.FPLDPC_NOISE_LEHMER, 123456789, first, frames, n, SNR, SIGMA, 4,
                                             cw.ctypes.data_as(ctypes.c_void_p), got.ctypes.data_as(ctypes.c_void_p), t,
                                             2) == 0
        assert got.tobytes() == want.tobytes()
        bias = F.Bias(n, [0, 15, 16, 168], [0.5, -0.25, 1.0, 0.3])
        want, want_logw = F.channel_llr_biased(bias, 123456789, first, frames, SNR, SIGMA, 4, cw, dtype)
        got, logw = np.empty((frames, n), dtype), np.empty(frames)
        assert L.fpldpc_bias_channel_llr_src_host(bias._h, F.FPLDPC_NOISE_LEHMER, 123456789, first, frames, SNR, SIGMA, 4,
                                                  cw.ctypes.data_as(ctypes.c_void_p), 0,
                                                  got.ctypes.data_as(ctypes.c_void_p), t,
                                                  logw.ctypes.data_as(ctypes.c_void_p), 2) == 0
        assert got.tobytes() == want.tobytes() and logw.tobytes() == want_logw.tobytes()


def test_python_default_is_lehmer(F):
    want = F.channel_llr(123456789, 3, 2, 25, SNR, SIGMA)
    assert (F.channel_llr(123456789, 3, 2, 25, SNR, SIGMA, source="lehmer") == want).all()
    assert (F.channel_llr(123456789, 3, 2, 25, SNR, SIGMA, source="philox") != want).any()
    assert (F.FPLDPC_NOISE_LEHMER, F.FPLDPC_NOISE_PHILOX) == (0, 1)


def test_argument_rules(F):
    L = F.lib()
    out = np.empty((1, 25), np.int32)
    p = out.ctypes.data_as(ctypes.c_void_p)

    def call(source, seed, first, frames=1):
        return L.fpldpc_channel_llr_src_host(source, seed, first, frames, 25, SNR, SIGMA, 4, None, p, F.FPLDPC_LLR_I32, 1)
    assert call(2, 1, 0) != 0 and b"source" in L.fpldpc_last_error()
    assert call(-1, 1, 0) != 0
    assert call(F.FPLDPC_NOISE_PHILOX, -1, 0) != 0  # a negative seed
    assert call(F.FPLDPC_NOISE_PHILOX, 0, 0) == 0 and call(F.FPLDPC_NOISE_PHILOX, 2**63 - 1, 0) == 0
    assert call(F.FPLDPC_NOISE_PHILOX, 1, 2**48) == 0  # f * n far beyond 2^48
    assert call(F.FPLDPC_NOISE_PHILOX, 1, 2**63 - 2, 1) == 0 and call(F.FPLDPC_NOISE_PHILOX, 1, 2**63 - 1, 1) != 0
    assert call(F.FPLDPC_NOISE_PHILOX, 1, -1) != 0
    # Lehmer's rules are unchanged
    assert call(F.FPLDPC_NOISE_LEHMER, 0, 0) != 0 and call(F.FPLDPC_NOISE_LEHMER, 2**31 - 1, 0) != 0
    assert call(F.FPLDPC_NOISE_LEHMER, 1, 0) == 0
    bias = F.Bias(25, [3], [0.5])
    logw = np.empty(1)

    def bcall(b, source, seed):
        return L.fpldpc_bias_channel_llr_src_host(b, source, seed, 0, 1, SNR, SIGMA, 4, None, 0, p, F.FPLDPC_LLR_I32,
                                                  logw.ctypes.data_as(ctypes.c_void_p), 1)
    assert bcall(bias._h, 7, 1) != 0 and b"source" in L.fpldpc_last_error()
    assert bcall(None, F.FPLDPC_NOISE_PHILOX, 1) != 0 and b"bias" in L.fpldpc_last_error()
    assert bcall(bias._h, F.FPLDPC_NOISE_PHILOX, -5) != 0 and bcall(bias._h, F.FPLDPC_NOISE_PHILOX, 0) == 0
    assert bcall(bias._h, F.FPLDPC_NOISE_LEHMER, 0) != 0
    for fn in (F.channel_llr, lambda *a, **k: F.channel_llr_biased(bias, *a[:3], *a[4:], **k)):
        with pytest.raises(ValueError):
            fn(1, 0, 1, 25, SNR, SIGMA, source="mt19937")
    with pytest.raises(ValueError):
        F.channel_llr(1, 0, 1, 25, SNR, SIGMA, source=1)


PHILOX_RANGE = b"bad channel arguments (philox: 0 <= seed, first_frame + frames < 2^63)"
# rule -> (the argument it breaks, the message): the rules are written once (philox_rules, fpldpc_source.hpp) for the
# host twins and the device entry points; the host entry points report each with the status and message they always had
PHILOX_RULES = {"null out": (dict(out=None), PHILOX_RANGE),
                "n <= 0": (dict(n=0), PHILOX_RANGE),
                "frac_bits 25": (dict(frac_bits=25), PHILOX_RANGE),
                "negative seed": (dict(seed=-1), PHILOX_RANGE),
                "frame range overflow": (dict(first=2**63 - 2, frames=2), PHILOX_RANGE),
                "negative frames": (dict(frames=-1), PHILOX_RANGE),
                "bad out_type": (dict(out_type=77), b"bad out_type"),
                "bad cw_per_frame": (dict(cw_per_frame=2), b"cw_per_frame must be 0 or 1")}


@pytest.mark.parametrize("rule", list(PHILOX_RULES))
def test_philox_rule_status_and_message(F, rule):
    L = F.lib()
    buf, logw = np.empty((2, 25), np.int32), np.empty(2)
    change, message = PHILOX_RULES[rule]
    a = dict(seed=5, first=0, frames=1, n=25, frac_bits=4, out=buf.ctypes.data_as(ctypes.c_void_p), out_type=F.FPLDPC_LLR_I32,
             cw_per_frame=0)
    a.update(change)
    bias = F.Bias(25, [3], [0.5])
    if "cw_per_frame" not in change:  # the plain channel has no such argument
        assert L.fpldpc_channel_llr_src_host(F.FPLDPC_NOISE_PHILOX, a["seed"], a["first"], a["frames"], a["n"], SNR, SIGMA,
                                             a["frac_bits"], None, a["out"], a["out_type"], 1) == -1  # FPLDPC_ERR_ARG
        assert L.fpldpc_last_error() == message
    if "n" not in change:  # the shifted channel's n is its bias's
        assert L.fpldpc_bias_channel_llr_src_host(bias._h, F.FPLDPC_NOISE_PHILOX, a["seed"], a["first"], a["frames"], SNR, SIGMA,
                                                  a["frac_bits"], None, a["cw_per_frame"], a["out"], a["out_type"],
                                                  logw.ctypes.data_as(ctypes.c_void_p), 1) == -1
        assert L.fpldpc_last_error() == message
    # the rules come after the source and, for the shifted channel, after the bias
    assert L.fpldpc_bias_channel_llr_src_host(None, F.FPLDPC_NOISE_PHILOX, a["seed"], a["first"], a["frames"], SNR, SIGMA,
                                              a["frac_bits"], None, a["cw_per_frame"], a["out"], a["out_type"], None, 1) == -1
    assert L.fpldpc_last_error() == b"bias: null bias"


@pytest.mark.parametrize("n,first", [(25, 0), (169, 2**33 + 5), (2209, 37)])
def test_shifted_host_channel(F, n, first):
    frames, seed = 6, 2**40 + 7
    cw = np.random.default_rng(n).integers(0, 2, (frames, n)).astype(np.uint8)
    # all shifts 0.0: the plain channel's values, logw = +0.0
    for dtype in (np.int16, np.int32, np.float64):
        plain = F.channel_llr(seed, first, frames, n, SNR, SIGMA, 4, cw[0], dtype, source="philox")
        got, logw = F.channel_llr_biased(F.Bias(n, np.arange(n), 0.0), seed, first, frames, SNR, SIGMA, 4, cw[0], dtype,
                                         source="philox")
        assert got.tobytes() == plain.tobytes()
        assert (logw == 0.0).all() and not np.signbit(logw).any()
    pos = np.unique(np.concatenate([[0, n - 1], np.random.default_rng(n + 1).choice(n, min(n, 70), replace=False)]))
    shift = np.linspace(-0.7, 1.2, len(pos))
    model = PM.channel(seed, first, frames, n, SNR, SIGMA, 4, cw, pos, shift)
    bias = F.Bias(n, pos, shift)
    f64, logw = F.channel_llr_biased(bias, seed, first, frames, SNR, SIGMA, 4, cw, np.float64, source="philox")
    assert np.abs(f64 - model["llr"]).max() <= PM.f64_bound(SNR, SIGMA)
    assert (np.abs(logw - model["logw"]) <= BM.logw_bound(model["abs_terms"])).all()
    i32, logw32 = F.channel_llr_biased(bias, seed, first, frames, SNR, SIGMA, 4, cw, np.int32, nthreads=3, source="philox")
    PM.assert_fixed_equal(BUDGET, model, i32, SNR, SIGMA, 4, (n, first))
    assert logw32.tobytes() == logw.tobytes()
