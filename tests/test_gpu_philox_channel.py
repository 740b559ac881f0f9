"""The counter-based noise source on the device (fpldpc_channel_llr_src, fpldpc_bias_channel_llr_src with
FPLDPC_NOISE_PHILOX: the Philox channel kernel and its patch kernel) against the host twins and
tests/philox_model.py, by that file's comparison rule: F64 within f64_bound, I32 / I16 equal except within one at
the model's boundary positions, of which the whole module may meet two.  The channel kernel takes a thread per pair:
n = 1 and odd n (a half pair ends each frame and odd frames are misaligned), 300 * ceil(n / 2) no multiple of 256,
a frame index that uses counter word 3, a seed that uses key word 1.  Guard words behind every output, an overflow
count equal to the count on the stored values, a second call with the same bits, and the Lehmer source through the
same entry points equal to the entry points without a source."""
import ctypes
import itertools

import numpy as np
import pytest

import bias_model as BM
import philox_model as PM
from test_gpu_bias_channel import CASES as BIAS_CASES, codeword, positions

pytestmark = pytest.mark.gpu
SNR, SIGMA = 2.3, 0.66
SEEDS = (123456789, 2**40 + 7)
MODES = ("none", "shared", "per_frame")
GUARD, GUARD_LOGW, PAD = 0x5A, -77.25, 64
BUDGET = PM.Budget(2)  # boundary positions over everything this module compares

NS, FRAMES, FIRSTS = (1, 2, 25, 169, 2209), (1, 3, 300), (0, 37, 2**33 + 5)
# every n with every number of frames and every first frame; seeds and codeword modes rotate so that every n, every
# number of frames and every first frame meets each of them
CHANNEL = [(n, fr, fi, SEEDS[(a + b + c) % 2], MODES[(a + 2 * b + c) % 3])
           for (a, n), (b, fr), (c, fi) in itertools.product(enumerate(NS), enumerate(FRAMES), enumerate(FIRSTS))]


def device_call(F, dev, source, seed, first, frames, n, snr, sigma, frac_bits, cw, dtype, bias=None):
    """fpldpc_channel_llr_src (bias None) or fpldpc_bias_channel_llr_src into buffers with PAD guard words behind
    them: (llr [frames][n], logw [frames] or None, overflow, guards ok)."""
    import torch
    fill = {torch.int16: GUARD * 257, torch.int32: GUARD * 0x01010101, torch.float64: GUARD_LOGW}[dtype]
    out = torch.full((frames * n + PAD,), fill, dtype=dtype, device=dev)
    logw = torch.full((frames + PAD,), GUARD_LOGW, dtype=torch.float64, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    cw_t = None if cw is None else torch.from_numpy(cw).to(dev)
    t = {torch.int16: F.FPLDPC_LLR_I16, torch.int32: F.FPLDPC_LLR_I32, torch.float64: F.FPLDPC_LLR_F64}[dtype]
    c = ctypes.c_void_p
    cw_p, per = c(cw_t.data_ptr()) if cw is not None else None, 1 if cw is not None and cw.ndim == 2 else 0
    stream = c(torch.cuda.current_stream(dev).cuda_stream or None)
    if bias is None:
        st = F.lib().fpldpc_channel_llr_src(source, seed, first, frames, n, snr, sigma, frac_bits, cw_p, per,
                                            c(out.data_ptr()), t, c(ovf.data_ptr()), stream)
    else:
        st = F.lib().fpldpc_bias_channel_llr_src(bias._h, source, seed, first, frames, snr, sigma, frac_bits, cw_p, per,
                                                 c(out.data_ptr()), t, c(ovf.data_ptr()), c(logw.data_ptr()), stream)
    assert st == 0, F.lib().fpldpc_last_error()
    torch.cuda.synchronize()
    out, logw = out.cpu().numpy(), logw.cpu().numpy()
    ok = bool((out[frames * n:] == fill).all()) and bool((logw[frames:] == GUARD_LOGW).all())
    assert bias is not None or (logw == GUARD_LOGW).all()
    return out[:frames * n].reshape(frames, n), logw[:frames] if bias is not None else None, int(ovf.cpu()[0]), ok


def host_twin(F, seed, first, frames, n, cw, dtype, bias=None):
    """The host twin; a codeword per frame goes through the shifted host channel with an empty bias."""
    if bias is None and (cw is None or cw.ndim == 1):
        return F.channel_llr(seed, first, frames, n, SNR, SIGMA, 4, cw, dtype, source="philox"), None
    return F.channel_llr_biased(bias or F.Bias(n, [], []), seed, first, frames, SNR, SIGMA, 4, cw, dtype, source="philox")


@pytest.mark.parametrize("n,frames,first,seed,mode", CHANNEL)
def test_channel_against_host_twin_and_model(F, torch_dev, n, frames, first, seed, mode):
    import torch
    P = F.FPLDPC_NOISE_PHILOX
    cw = codeword(n, frames, mode)
    model = PM.channel(seed, first, frames, n, SNR, SIGMA, 4, cw)
    BUDGET.take(PM.boundary(model["x"], SNR, SIGMA, 4))  # before the other sides are looked at
    assert np.abs(model["fp"]).max() < 32767  # so the int16 output is the same numbers
    host32 = host_twin(F, seed, first, frames, n, cw, np.int32)[0]
    host64 = host_twin(F, seed, first, frames, n, cw, np.float64)[0]
    PM.assert_fixed_pair(None, model, host32, model["fp"], SNR, SIGMA, 4, "host / model")
    assert np.abs(host64 - model["llr"]).max() <= PM.f64_bound(SNR, SIGMA)
    got = {}
    for dtype in (torch.int32, torch.int16, torch.float64):
        got[dtype], _, ovf, ok = device_call(F, torch_dev, P, seed, first, frames, n, SNR, SIGMA, 4, cw, dtype)
        assert ok and ovf == 0, dtype
    PM.assert_fixed_pair(None, model, got[torch.int32], model["fp"], SNR, SIGMA, 4, "device / model")
    PM.assert_fixed_pair(None, model, got[torch.int32], host32, SNR, SIGMA, 4, "device / host")
    assert (got[torch.int16] == got[torch.int32]).all()
    assert np.abs(got[torch.float64] - model["llr"]).max() <= PM.f64_bound(SNR, SIGMA)
    assert np.abs(got[torch.float64] - host64).max() <= PM.f64_bound(SNR, SIGMA)
    for dtype in (torch.int16, torch.float64):  # the same call, the same bits
        again = device_call(F, torch_dev, P, seed, first, frames, n, SNR, SIGMA, 4, cw, dtype)[0]
        assert again.tobytes() == got[dtype].tobytes()


@pytest.mark.parametrize("n,frames", [(25, 300), (2209, 3), (1, 300)])
def test_overflow_count_is_the_stored_values(F, torch_dev, n, frames):
    """frac_bits = 12 at 2 snr = 6: some values leave int16.  The count is that of the int32 output's values outside
    int16, the stored values are those truncated to 16 bits, and the int32 output counts nothing."""
    import torch
    P, seed, first, snr, sigma = F.FPLDPC_NOISE_PHILOX, 2**40 + 7, 2**33 + 5, 3.0, 0.5
    cw = codeword(n, frames, "per_frame")
    got32, _, ovf32, ok32 = device_call(F, torch_dev, P, seed, first, frames, n, snr, sigma, 12, cw, torch.int32)
    got16, _, ovf16, ok16 = device_call(F, torch_dev, P, seed, first, frames, n, snr, sigma, 12, cw, torch.int16)
    want = int(((got32 < -32768) | (got32 > 32767)).sum())
    assert ok32 and ok16 and ovf32 == 0 and ovf16 == want and want > 0
    assert (got16 == got32.astype(np.int16)).all()
    model = PM.channel(seed, first, frames, n, snr, sigma, 12, cw)
    BUDGET.take(PM.boundary(model["x"], snr, sigma, 12))
    PM.assert_fixed_pair(None, model, got32, model["fp"], snr, sigma, 12)


@pytest.mark.parametrize("n,frames,first,mode", [(25, 300, 37, "per_frame"), (2209, 3, 2**33 + 5, "shared"), (1, 3, 0, "none")])
def test_lehmer_through_the_src_entry_point(F, torch_dev, n, frames, first, mode):
    import torch
    cw = codeword(n, frames, mode)
    cw_t = None if cw is None else torch.from_numpy(cw).to(torch_dev)
    for dtype in (torch.int16, torch.int32, torch.float64):
        want, want_ovf = F.channel_llr_torch(123456789, first, frames, n, SNR, SIGMA, cw=cw_t, dtype=dtype, device=torch_dev)
        torch.cuda.synchronize()
        got, _, ovf, ok = device_call(F, torch_dev, F.FPLDPC_NOISE_LEHMER, 123456789, first, frames, n, SNR, SIGMA, 4, cw, dtype)
        assert ok and got.tobytes() == want.cpu().numpy().tobytes() and ovf == int(want_ovf.cpu()[0])
    bias = F.Bias(n, [0], [0.5])
    want, want_logw, _ = F.channel_llr_biased_torch(bias, 123456789, first, frames, SNR, SIGMA, cw=cw_t, device=torch_dev)
    torch.cuda.synchronize()
    got, logw, _, ok = device_call(F, torch_dev, F.FPLDPC_NOISE_LEHMER, 123456789, first, frames, n, SNR, SIGMA, 4, cw,
                                   torch.int16, bias)
    assert ok and got.tobytes() == want.cpu().numpy().tobytes() and logw.tobytes() == want_logw.cpu().numpy().tobytes()


def test_python_sources_and_argument_rules(F, torch_dev):
    import torch
    a, _ = F.channel_llr_torch(5, 0, 3, 25, SNR, SIGMA, device=torch_dev, source="philox")
    b = F.channel_llr(5, 0, 3, 25, SNR, SIGMA, source="philox")
    torch.cuda.synchronize()
    assert np.abs(a.cpu().numpy().astype(np.int64) - b).max() <= 1
    with pytest.raises(ValueError):
        F.channel_llr_torch(5, 0, 3, 25, SNR, SIGMA, device=torch_dev, source="xorshift")
    out = torch.zeros(25, dtype=torch.int32, device=torch_dev)
    c = ctypes.c_void_p

    def call(source, seed, first):
        return F.lib().fpldpc_channel_llr_src(source, seed, first, 1, 25, SNR, SIGMA, 4, None, 0, c(out.data_ptr()),
                                              F.FPLDPC_LLR_I32, None, None)
    assert call(3, 1, 0) != 0 and b"source" in F.lib().fpldpc_last_error()
    assert call(F.FPLDPC_NOISE_PHILOX, -1, 0) != 0 and call(F.FPLDPC_NOISE_PHILOX, 1, 2**63 - 1) != 0
    assert call(F.FPLDPC_NOISE_LEHMER, 0, 0) != 0 and call(F.FPLDPC_NOISE_LEHMER, 1, 2**48) != 0  # unchanged
    assert call(F.FPLDPC_NOISE_PHILOX, 0, 2**48) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,kind,frames,first,mode", BIAS_CASES)
def test_shifted_channel_device_equals_host(F, torch_dev, n, kind, frames, first, mode):
    import torch
    P, seed = F.FPLDPC_NOISE_PHILOX, SEEDS[(n + frames) % 2]
    pos = positions(n, kind)
    shift = np.linspace(-0.7, 1.2, len(pos)) if kind == "n" else 0.5  # every position: shifts of both signs
    cw = codeword(n, frames, mode)
    bias = F.Bias(n, pos, shift)
    model = PM.channel(seed, first, frames, n, SNR, SIGMA, 4, cw, pos, shift)
    BUDGET.take(PM.boundary(model["x"], SNR, SIGMA, 4))
    assert np.abs(model["fp"]).max() < 32767
    bound = BM.logw_bound(model["abs_terms"])
    want, want_logw = host_twin(F, seed, first, frames, n, cw, np.int32, bias)
    PM.assert_fixed_pair(None, model, want, model["fp"], SNR, SIGMA, 4, "host / model")
    assert (np.abs(want_logw - model["logw"]) <= bound).all()
    seen = {}
    for dtype in (torch.int32, torch.int16):
        got, logw, ovf, ok = device_call(F, torch_dev, P, seed, first, frames, n, SNR, SIGMA, 4, cw, dtype, bias)
        assert ok and ovf == 0
        PM.assert_fixed_pair(None, model, got, want, SNR, SIGMA, 4, "device / host")
        assert (np.abs(logw - want_logw) <= bound).all() and (np.abs(logw - model["logw"]) <= bound).all(), \
            (np.abs(logw - want_logw).max(), bound.min())
        seen[dtype] = (got, logw)
    assert (seen[torch.int32][0] == seen[torch.int16][0]).all()
    assert seen[torch.int32][1].tobytes() == seen[torch.int16][1].tobytes()
    again = device_call(F, torch_dev, P, seed, first, frames, n, SNR, SIGMA, 4, cw, torch.int16, bias)
    assert again[1].tobytes() == seen[torch.int16][1].tobytes() and again[0].tobytes() == seen[torch.int16][0].tobytes()


@pytest.mark.parametrize("n,frames", [(25, 300), (169, 3), (2209, 3)])
def test_zero_shift_is_the_philox_channel(F, torch_dev, n, frames):
    """The patch kernel forms its variate by the channel kernel's code behind a call: with every shift 0.0, and with
    an empty bias, it must write back what the channel kernel wrote, in every output type, and logw = +0.0."""
    import torch
    seed, first = 2**40 + 7, 2**33 + 5
    cw = torch.from_numpy(codeword(n, frames, "per_frame")).to(torch_dev)
    for dtype in (torch.int16, torch.int32, torch.float64):
        plain, _ = F.channel_llr_torch(seed, first, frames, n, SNR, SIGMA, cw=cw, dtype=dtype, source="philox")
        got, logw, ovf = F.channel_llr_biased_torch(F.Bias(n, np.arange(n), 0.0), seed, first, frames, SNR, SIGMA, cw=cw,
                                                    dtype=dtype, source="philox")
        none, logw0, _ = F.channel_llr_biased_torch(F.Bias(n, [], []), seed, first, frames, SNR, SIGMA, cw=cw, dtype=dtype,
                                                    source="philox")
        torch.cuda.synchronize()
        assert torch.equal(got, plain) and torch.equal(none, plain) and int(ovf.cpu()[0]) == 0
        for lw in (logw.cpu().numpy(), logw0.cpu().numpy()):
            assert (lw == 0.0).all() and not np.signbit(lw).any()


def test_shifted_overflow_follows_the_stored_value(F, torch_dev):
    """frac_bits = 12: a shift of -9 puts biased values outside int16 where the unshifted ones are inside, and the
    count follows the stored values, against the host's int32 values."""
    import torch
    P, n, frames, snr, sigma, seed = F.FPLDPC_NOISE_PHILOX, 25, 300, 1.0, 0.5, 123456789
    bias = F.Bias(n, [3, 16], -9.0)
    plain = device_call(F, torch_dev, P, seed, 0, frames, n, snr, sigma, 12, None, torch.int16)
    want, _ = F.channel_llr_biased(bias, seed, 0, frames, snr, sigma, 12, dtype=np.int32, source="philox")
    want_over = int(((want < -32768) | (want > 32767)).sum())
    assert want_over > plain[2]
    got, _, ovf, ok = device_call(F, torch_dev, P, seed, 0, frames, n, snr, sigma, 12, None, torch.int16, bias)
    model = PM.channel(seed, 0, frames, n, snr, sigma, 12, None, [3, 16], -9.0)
    BUDGET.take(PM.boundary(model["x"], snr, sigma, 12))
    assert ok and ovf == want_over
    PM.assert_fixed_pair(None, model, got, want.astype(np.int16), snr, sigma, 12)
