"""The host side of mean-shift importance sampling (include/fpldpc.h: fpldpc_bias_create,
fpldpc_bias_channel_llr_host) against the unbiased host channel and tests/bias_model.py, the weight's sign and
normalisation against a closed form, and every FPLDPC_ERR_ARG rule of the create and channel calls.  CPU only."""
import ctypes
import math

import numpy as np
import pytest

import bias_model as BM

SEED = 123456789
SNR, SIGMA = 2.3, 0.66
DTYPES = (np.int16, np.int32, np.float64)


def position_sets(n):
    return {"first": [0], "last": [n - 1], "15_16": [15, 16], "all": list(range(n))}


def codewords(n, frames, mode):
    rng = np.random.default_rng(n * 7 + frames)
    if mode == "none":
        return None
    return rng.integers(0, 2, n if mode == "shared" else (frames, n)).astype(np.uint8)


def plain(F, first, frames, n, cw, dtype, frac_bits=4):
    """The unbiased host channel; a codeword per frame goes through it a frame at a time."""
    if cw is None or cw.ndim == 1:
        return F.channel_llr(SEED, first, frames, n, SNR, SIGMA, frac_bits, cw=cw, dtype=dtype)
    return np.concatenate([F.channel_llr(SEED, first + f, 1, n, SNR, SIGMA, frac_bits, cw=cw[f], dtype=dtype)
                           for f in range(frames)])


@pytest.mark.parametrize("mode", ["none", "shared", "per_frame"])
@pytest.mark.parametrize("first", [0, 37, 2**33])
@pytest.mark.parametrize("n", [25, 169])
def test_identity(F, n, first, mode):
    """No position, or every shift 0.0: the unbiased channel bit for bit in all three output types."""
    frames = 5
    cw = codewords(n, frames, mode)
    for dtype in DTYPES:
        want = plain(F, first, frames, n, cw, dtype)
        for nthreads in (1, 3):
            got, logw = F.channel_llr_biased(F.Bias(n, [], []), SEED, first, frames, SNR, SIGMA, cw=cw, dtype=dtype,
                                             nthreads=nthreads)
            assert got.dtype == want.dtype and (got == want).all()
            assert (logw == 0.0).all() and not np.signbit(logw).any()  # 0.0 exactly
            for name, pos in position_sets(n).items():
                got, logw = F.channel_llr_biased(F.Bias(n, pos, 0.0), SEED, first, frames, SNR, SIGMA, cw=cw, dtype=dtype,
                                                 nthreads=nthreads)
                assert (got == want).all(), (name, dtype)
                assert (logw == 0.0).all(), name


@pytest.mark.parametrize("mode", ["none", "shared", "per_frame"])
@pytest.mark.parametrize("first", [0, 37, 2**33])
@pytest.mark.parametrize("n", [25, 169])
def test_locality_and_biased_positions(F, n, first, mode):
    """Outside the bias the unbiased channel exactly; on it the model's values (I32 and F64) and log-weight."""
    frames = 7
    cw = codewords(n, frames, mode)
    for name, pos in position_sets(n).items():
        shift = np.linspace(-0.4, 1.3, len(pos))  # mixed signs where there are several
        if len(pos) == 1:
            shift = np.array([0.5])
        model = BM.channel(SEED, first, frames, n, SNR, SIGMA, 4, cw, pos, shift)
        outside = np.setdiff1d(np.arange(n), pos)
        for nthreads in (1, 3):
            bias = F.Bias(n, pos, shift)
            for dtype in DTYPES:
                got, logw = F.channel_llr_biased(bias, SEED, first, frames, SNR, SIGMA, cw=cw, dtype=dtype,
                                                 nthreads=nthreads)
                assert (got[:, outside] == plain(F, first, frames, n, cw, dtype)[:, outside]).all(), (name, dtype)
                if dtype is np.float64:
                    assert (got[:, pos] == model["llr"][:, pos]).all(), name
                else:
                    assert (got[:, pos] == model["fp"][:, pos]).all(), (name, dtype)
                err = np.abs(logw - model["logw"])
                assert (err <= BM.logw_bound(model["abs_terms"])).all(), (name, err.max())
        assert (model["logw"] != 0).all()  # there is a weight to compare


def test_the_model_is_the_unbiased_channel_without_a_bias(F):
    """The numpy restatement of the stream and the variate against the library's channel, exactly."""
    for first in (0, 37, 2**33):
        m = BM.channel(SEED, first, 6, 25, SNR, SIGMA, 4)
        assert (m["llr"] == F.channel_llr(SEED, first, 6, 25, SNR, SIGMA, dtype=np.float64)).all()
        assert (m["fp"] == F.channel_llr(SEED, first, 6, 25, SNR, SIGMA, dtype=np.int32)).all()
    assert int(BM.states(1, 9999, 1)[0]) == 399268537  # rngs.cpp:154-180 CHECK


CLOSED = dict(n=25, pos=[0, 7, 15, 16, 24], sigma=0.5, frames=20000)


def closed_form_run(F, shift):
    n, sigma = CLOSED["n"], CLOSED["sigma"]
    snr = 1 / sigma**2
    llr, logw = F.channel_llr_biased(F.Bias(n, CLOSED["pos"], shift), SEED, 0, CLOSED["frames"], snr, sigma,
                                     dtype=np.float64)
    return llr / (2 * snr), np.exp(logw)


def test_weight_sign_and_normalisation_against_a_closed_form(F):
    """All-zero codeword, sigma = 0.5, shift 1.0 on five positions: the weighted frequency of sum_{i in B} y_i < 0
    estimates Q(sqrt(5) / sigma) = 3.872e-6, within 5 standard errors taken from the run's own sum (w * 1)^2.
    (A numpy restatement of the stream gives 3.902e-6, se 6.2e-8, 10,068 hits; the plain channel has none.)"""
    y, w = closed_form_run(F, 1.0)
    frames = CLOSED["frames"]
    hit = y[:, CLOSED["pos"]].sum(axis=1) < 0
    est = (w * hit).sum() / frames
    se = math.sqrt(max(((w * hit) ** 2).sum() / frames - est**2, 0) / frames)
    exact = 0.5 * math.erfc(math.sqrt(5) / CLOSED["sigma"] / math.sqrt(2))
    print(f"est {est:.4e} se {se:.2e} exact {exact:.4e} hits {int(hit.sum())}")
    assert abs(exact - 3.872e-6) < 1e-9
    assert abs(est - exact) <= 5 * se
    assert hit.sum() > 5000
    y0, w0 = closed_form_run(F, 0.0)
    assert not (y0[:, CLOSED["pos"]].sum(axis=1) < 0).any() and (w0 == 1.0).all()


def test_mean_weight(F):
    """Shift 0.1: E w = 1 and Var w = exp(5 * 0.01 / 0.25) - 1, so |mean(w) - 1| <= 5 sqrt(Var / 20000) = 0.0166."""
    _, w = closed_form_run(F, 0.1)
    bound = 5 * math.sqrt((math.exp(5 * 0.01 / 0.25) - 1) / CLOSED["frames"])
    print(f"mean weight {w.mean():.4f} bound {bound:.4f}")
    assert abs(bound - 0.0166) < 1e-4
    assert abs(w.mean() - 1) <= bound


def _create(F, n, pos, shift, count=None):
    pos = np.ascontiguousarray(pos, np.int32)
    shift = np.ascontiguousarray(shift, np.float64)
    h = ctypes.c_void_p()
    st = F.lib().fpldpc_bias_create(n, F._lib._ptr(pos), F._lib._ptr(shift), len(pos) if count is None else count,
                                    ctypes.byref(h))
    if st == 0:
        F.lib().fpldpc_bias_free(h)
    return st, F.lib().fpldpc_last_error().decode()


@pytest.mark.parametrize("pos,shift,count,rule", [
    ([3, 2], [0.5, 0.5], None, "ascending"), ([2, 2], [0.5, 0.5], None, "duplicate"),
    ([-1, 2], [0.5, 0.5], None, "out of range"), ([2, 25], [0.5, 0.5], None, "out of range"),
    ([2, 3], [0.5, float("nan")], None, "finite"), ([2, 3], [float("inf"), 0.5], None, "finite"),
    ([2, 3], [0.5, -float("inf")], None, "finite"),
    ([2, 3], [0.5, 0.5], -1, "count"), (list(range(26)), [0.5] * 26, None, "count"),
])
def test_create_rules(F, pos, shift, count, rule):
    st, msg = _create(F, 25, pos, shift, count)
    assert st == -1 and rule in msg and "bias" in msg, msg
    with pytest.raises(F.FpldpcError, match="n must be positive"):
        F.Bias(0, [], [])


def test_create_accepts_the_edges(F):
    assert _create(F, 25, [], [])[0] == 0
    assert _create(F, 25, list(range(25)), [-2.0] * 25)[0] == 0
    b = F.Bias(25, [0, 24], [0.0, -1.5])
    assert (b.n, b.count) == (25, 2) and b.sums["frames"] == 0 and b.sums["sum_w"] == 0.0
    assert (F.Bias(25, [3, 4], 0.5).shifts == 0.5).all()  # a scalar shift


CHANNEL_RULES = [(dict(frames=-1), "channel arguments"), (dict(first_frame=-1), "channel arguments"),
                 (dict(frac_bits=-1), "channel arguments"), (dict(frac_bits=25), "channel arguments"),
                 (dict(seed=0), "channel arguments"), (dict(seed=2**31 - 1), "channel arguments"),
                 (dict(out=None), "channel arguments"), (dict(out_type=3), "out_type"),
                 (dict(cw_per_frame=2), "cw_per_frame"), (dict(bias=None), "null bias")]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("change,rule", CHANNEL_RULES + [(dict(first_frame=2**48 // 25, device_only=True), "channel arguments")])
def test_channel_rules(F, change, rule, device):
    """Both channel calls refuse before they touch anything: the device call's rules need no device."""
    change = dict(change)
    if change.pop("device_only", False) and not device:
        return
    bias = F.Bias(25, [1], 0.5)
    buf = np.zeros((2, 25), np.int32)
    a = dict(bias=bias._h, seed=SEED, first_frame=0, frames=2, frac_bits=4, out=F._lib._ptr(buf), out_type=F.FPLDPC_LLR_I32,
             cw_per_frame=0)
    a.update(change)
    if device:
        st = F.lib().fpldpc_bias_channel_llr(a["bias"], a["seed"], a["first_frame"], a["frames"], SNR, SIGMA, a["frac_bits"], None,
                                             a["cw_per_frame"], a["out"], a["out_type"], None, None, None)
    else:
        st = F.lib().fpldpc_bias_channel_llr_host(a["bias"], a["seed"], a["first_frame"], a["frames"], SNR, SIGMA,
                                                  a["frac_bits"], None, a["cw_per_frame"], a["out"], a["out_type"], None, 1)
    msg = F.lib().fpldpc_last_error().decode()
    assert st == -1 and rule in msg and "bias" in msg, msg
    assert not buf.any()


def test_int16_rule_follows_the_stored_value(F):
    """frac_bits = 12: the unshifted values fit int16, a shift of -9 puts the biased one outside -- an error, as the
    host channel's; and a value the plain channel cannot store is fine once the shift brings it back."""
    n, snr, sigma = 25, 1.0, 0.5
    assert np.abs(F.channel_llr(SEED, 0, 4, n, snr, sigma, 12, dtype=np.int32)).max() <= 32767
    F.channel_llr_biased(F.Bias(n, [3], 0.5), SEED, 0, 4, snr, sigma, 12, dtype=np.int16)
    with pytest.raises(F.FpldpcError, match="int16"):
        F.channel_llr_biased(F.Bias(n, [3], -9.0), SEED, 0, 4, snr, sigma, 12, dtype=np.int16)
    got, _ = F.channel_llr_biased(F.Bias(n, [3], -9.0), SEED, 0, 4, snr, sigma, 12, dtype=np.int32)
    assert (np.abs(got[:, 3]) > 32767).all()
    big = F.channel_llr(SEED, 0, 1, n, 3.0, sigma, 12, dtype=np.int32)[0]
    over = np.nonzero(np.abs(big) > 32767)[0]
    assert len(over) > 0
    with pytest.raises(F.FpldpcError, match="int16"):
        F.channel_llr(SEED, 0, 1, n, 3.0, sigma, 12, dtype=np.int16)
    back, _ = F.channel_llr_biased(F.Bias(n, over, 1.0), SEED, 0, 1, 3.0, sigma, 12, dtype=np.int16)
    assert (back[0, over] == F.channel_llr_biased(F.Bias(n, over, 1.0), SEED, 0, 1, 3.0, sigma, 12, dtype=np.int32)[0][0, over]).all()
