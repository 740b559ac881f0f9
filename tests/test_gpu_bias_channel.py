"""The device side of mean-shift importance sampling (fpldpc_bias_channel_llr: the channel kernel followed by
the patch kernel) against its host twin: equal LLRs (I16, I32) and overflow counts, logw within
tests/bias_model.py's bound of the host's and of the model's, bit-identical logw from a second call, a guard
word behind both outputs.  The patch kernel takes a wave per frame, eight frames per workgroup, lanes striding
the biased positions by 64: one frame, three, and 300 (not a multiple of eight; 300 * ceil(n / 16) is not a
multiple of the channel kernel's 256 either), counts below, at and above 64 and 128, and every position."""
import ctypes

import numpy as np
import pytest

import bias_model as BM

pytestmark = pytest.mark.gpu
SEED = 123456789
SNR, SIGMA = 2.3, 0.66
GUARD_LLR, GUARD_LOGW, PAD = 0x5A, -77.25, 64


def positions(n, kind):
    if kind == "1":
        return np.array([n // 2])
    if kind == "2":
        return np.array([15, 16])
    if kind == "n":
        return np.arange(n)
    rng = np.random.default_rng(n + int(kind))
    inner = rng.choice(np.arange(1, n - 1), int(kind) - 2, replace=False)
    return np.sort(np.concatenate([[0, n - 1], inner]))  # both ends among them


def codeword(n, frames, mode):
    rng = np.random.default_rng(n * 7 + frames)
    return None if mode == "none" else rng.integers(0, 2, n if mode == "shared" else (frames, n)).astype(np.uint8)


def device_call(F, dev, bias, first, frames, snr, sigma, frac_bits, cw, dtype):
    """fpldpc_bias_channel_llr into buffers with PAD guard words behind them: (llr, logw, overflow, llr guard ok,
    logw guard ok)."""
    import torch
    n = bias.n
    fill = {torch.int16: GUARD_LLR * 257, torch.int32: GUARD_LLR * 0x01010101, torch.float64: GUARD_LOGW}[dtype]
    out = torch.full((frames * n + PAD,), fill, dtype=dtype, device=dev)
    logw = torch.full((frames + PAD,), GUARD_LOGW, dtype=torch.float64, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    cw_t = None if cw is None else torch.from_numpy(cw).to(dev)
    t = {torch.int16: F.FPLDPC_LLR_I16, torch.int32: F.FPLDPC_LLR_I32, torch.float64: F.FPLDPC_LLR_F64}[dtype]
    c = ctypes.c_void_p
    st = F.lib().fpldpc_bias_channel_llr(bias._h, SEED, first, frames, snr, sigma, frac_bits,
                                         c(cw_t.data_ptr()) if cw is not None else None,
                                         1 if cw is not None and cw.ndim == 2 else 0, c(out.data_ptr()), t, c(ovf.data_ptr()),
                                         c(logw.data_ptr()), c(torch.cuda.current_stream(dev).cuda_stream or None))
    assert st == 0, F.lib().fpldpc_last_error()
    torch.cuda.synchronize()
    out, logw = out.cpu().numpy(), logw.cpu().numpy()
    return (out[:frames * n].reshape(frames, n), logw[:frames], int(ovf.cpu()[0]), bool((out[frames * n:] == fill).all()),
            bool((logw[frames:] == GUARD_LOGW).all()))


# every n with every number of frames, every first frame and every kind of codeword; every count each n allows
CASES = [(25, "1", 1, 0, "none"), (25, "2", 3, 37, "shared"), (25, "n", 300, 2**33, "per_frame"),
         (169, "1", 300, 37, "per_frame"), (169, "2", 1, 2**33, "none"), (169, "64", 3, 0, "shared"),
         (169, "65", 300, 0, "none"), (169, "130", 3, 2**33, "per_frame"), (169, "n", 1, 37, "shared"),
         (2209, "1", 3, 2**33, "shared"), (2209, "2", 300, 0, "per_frame"), (2209, "64", 1, 37, "none"),
         (2209, "65", 300, 2**33, "shared"), (2209, "130", 300, 37, "none"), (2209, "n", 3, 0, "per_frame")]


@pytest.mark.parametrize("n,kind,frames,first,mode", CASES)
def test_device_equals_host(F, torch_dev, n, kind, frames, first, mode):
    import torch
    pos = positions(n, kind)
    # every position: shifts of both signs; else 0.5
    shift = np.linspace(-0.7, 1.2, len(pos)) if kind == "n" else 0.5
    cw = codeword(n, frames, mode)
    bias = F.Bias(n, pos, shift)
    want, want_logw = F.channel_llr_biased(bias, SEED, first, frames, SNR, SIGMA, cw=cw, dtype=np.int32)
    model_logw, abs_terms = BM.weights(SEED, first, frames, n, SIGMA, cw, pos, shift)
    bound = BM.logw_bound(abs_terms)
    assert (np.abs(want_logw - model_logw) <= bound).all()
    assert np.abs(want).max() <= 32767  # so the int16 output is the same numbers
    seen = {}
    for dtype in (torch.int32, torch.int16):
        got, logw, ovf, guard_llr, guard_logw = device_call(F, torch_dev, bias, first, frames, SNR, SIGMA, 4, cw, dtype)
        assert guard_llr and guard_logw
        assert (got == want).all(), np.argwhere(got != want)[:4]
        assert ovf == 0
        assert (np.abs(logw - want_logw) <= bound).all() and (np.abs(logw - model_logw) <= bound).all(), \
            (np.abs(logw - want_logw).max(), bound.min())
        seen[dtype] = logw
    assert (seen[torch.int32] == seen[torch.int16]).all()
    again = device_call(F, torch_dev, bias, first, frames, SNR, SIGMA, 4, cw, torch.int16)[1]
    assert (again.view(np.uint64) == seen[torch.int16].view(np.uint64)).all()  # the same bits


def test_mixed_sign_shifts_on_a_few_positions(F, torch_dev):
    import torch
    n, frames, pos, shift = 169, 300, [0, 15, 16, 63, 64, 168], [-1.5, 0.25, -0.0, 1.0, 2.5, -0.3]
    cw = codeword(n, frames, "per_frame")
    bias = F.Bias(n, pos, shift)
    for dtype, np_dtype in ((torch.int32, np.int32), (torch.float64, np.float64)):
        want, want_logw = F.channel_llr_biased(bias, SEED, 37, frames, SNR, SIGMA, cw=cw, dtype=np_dtype)
        got, logw, _, g0, g1 = device_call(F, torch_dev, bias, 37, frames, SNR, SIGMA, 4, cw, dtype)
        assert g0 and g1
        if dtype is torch.int32:
            assert (got == want).all()
        else:  # the double output differs by the device's log: the same few ulps of z, scaled
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        _, abs_terms = BM.weights(SEED, 37, frames, n, SIGMA, cw, pos, shift)
        assert (np.abs(logw - want_logw) <= BM.logw_bound(abs_terms)).all()


@pytest.mark.parametrize("n,frames", [(25, 300), (2209, 3)])
def test_zero_shift_is_the_device_channel(F, torch_dev, n, frames):
    """The patch kernel holds its own copy of the channel kernel's variate code: with every shift 0.0 it must
    write back what the channel kernel wrote, in every output type, and logw = 0."""
    import torch
    cw = torch.from_numpy(codeword(n, frames, "per_frame")).to(torch_dev)
    for dtype in (torch.int16, torch.int32, torch.float64):
        plain, _ = F.channel_llr_torch(SEED, 37, frames, n, SNR, SIGMA, cw=cw, dtype=dtype)
        got, logw, ovf = F.channel_llr_biased_torch(F.Bias(n, np.arange(n), 0.0), SEED, 37, frames, SNR, SIGMA, cw=cw,
                                                    dtype=dtype)
        none, logw0, _ = F.channel_llr_biased_torch(F.Bias(n, [], []), SEED, 37, frames, SNR, SIGMA, cw=cw, dtype=dtype)
        torch.cuda.synchronize()
        assert torch.equal(got, plain) and torch.equal(none, plain) and int(ovf.cpu()[0]) == 0
        assert (logw.cpu().numpy() == 0.0).all() and (logw0.cpu().numpy() == 0.0).all()
        assert not np.signbit(logw0.cpu().numpy()).any()


def test_overflow_follows_the_stored_value(F, torch_dev):
    """frac_bits = 12.  A shift of -9 puts a biased value outside int16 where the unshifted one is inside: the
    count rises.  At 2 snr = 6 the plain channel overflows on some positions; a shift of 1.0 on exactly those
    brings most back inside: the count falls.  Both against the host's int32 values."""
    import torch
    n, frames, sigma = 25, 300, 0.5
    for snr, pos, shift in ((1.0, [3, 16], -9.0), (3.0, None, 1.0)):
        plain32 = F.channel_llr(SEED, 0, frames, n, snr, sigma, 12, dtype=np.int32)
        plain_over = int((np.abs(plain32 + 0.5) > 32767.5).sum())
        if pos is None:  # the positions where frame 0 overflows unshifted
            pos = np.nonzero(np.abs(plain32[0] + 0.5) > 32767.5)[0]
            assert len(pos) > 0
        bias = F.Bias(n, pos, shift)
        want, _ = F.channel_llr_biased(bias, SEED, 0, frames, snr, sigma, 12, dtype=np.int32)
        want_over = int(((want < -32768) | (want > 32767)).sum())
        assert want_over != plain_over  # the correction has something to correct
        _, _, plain_dev = F.channel_llr_biased_torch(F.Bias(n, [], []), SEED, 0, frames, snr, sigma, 12)
        assert int(plain_dev.cpu()[0]) == plain_over
        got, _, ovf, g0, g1 = device_call(F, torch_dev, bias, 0, frames, snr, sigma, 12, None, torch.int16)
        assert g0 and g1 and ovf == want_over, (ovf, want_over, plain_over)
        assert (got == want.astype(np.int16)).all()  # stored truncated to 16 bits
        got32, _, ovf32, _, _ = device_call(F, torch_dev, bias, 0, frames, snr, sigma, 12, None, torch.int32)
        assert (got32 == want).all() and ovf32 == 0  # the count is the int16 output's


def test_logw_may_be_null(F, torch_dev):
    import torch
    bias = F.Bias(25, [15, 16], 0.5)
    out = torch.zeros((3, 25), dtype=torch.int32, device=torch_dev)
    c = ctypes.c_void_p
    assert F.lib().fpldpc_bias_channel_llr(bias._h, SEED, 0, 3, SNR, SIGMA, 4, None, 0, c(out.data_ptr()), F.FPLDPC_LLR_I32,
                                           None, None, c(torch.cuda.current_stream(torch_dev).cuda_stream or None)) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == F.channel_llr_biased(bias, SEED, 0, 3, SNR, SIGMA, dtype=np.int32)[0]).all()
