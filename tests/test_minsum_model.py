"""The numpy model of the flooding min-sum decoder (tests/minsum_model.py) anchored to the reference: at
widths 16/15, scale_16 = 16, offset = 0 no clamp acts, and the model equals the oracle's flooding decoder
at frac_bits = 0 (Constant = 0: sxor is sign * min) in every output; clamped inputs on A; and the argument
rules of fpldpc_minsum_create, which are tested before a HIP device is looked for.  The model asserts the
definition's bounds, and that the compressed check state rebuilds every message, on every run.  CPU only."""
import numpy as np
import pytest

import minsum_model as FM

SEED = 123456789
KEYS = ("iters", "hard", "post", "syndrome_ok")


def _llr(F, O, code, eb, frames):
    snr, sigma = F.snr_sigma(eb, code.rate)
    return O.gen_llr(SEED, 0, frames, code.n, snr, sigma, 4)


def _rand(seed, frames, n, lim):
    return np.random.default_rng(seed).integers(-lim, lim, (frames, n)).astype(np.int32)


def _pair(F, O, codes, name):
    if name in codes:
        return codes[name]
    code = F.Code.array(13, 2)
    return code, O.OracleCode.from_alist_text(code.write_alist())


# (code, Eb/N0, AWGN frames, random frames of +-300, max_iter, width mask handed to the oracle)
ANCHOR = [("A", 4.5, 24, 8, 30, 0xFF), ("R", 6.5, 8, 8, 50, 0x3F), ("p13r2", 3.0, 24, 8, 8, 0xFF), ("W", 2.0, 16, 0, 30, 0xFF)]


@pytest.mark.parametrize("name,eb,frames,random,max_iter,mask", ANCHOR)
def test_plain_minsum_at_16_15_equals_the_oracle_at_frac_bits_0(F, O, codes, name, eb, frames, random, max_iter, mask):
    """clipped == 0 is a condition on the inputs: where no clamp acts the definition is the reference's
    flooding decoder with Constant = 0."""
    code, ocode = _pair(F, O, codes, name)
    llr = _llr(F, O, code, eb, frames)
    if random:
        llr = np.concatenate([llr, _rand(5, random, code.n, 300)])
    ref = O.decode_batch(ocode, llr, max_iter, 0, mask)
    got = FM.minsum_decode(FM.ModelCode.from_code(code), llr, 16, 15, max_iter=max_iter)
    assert got["clipped"] == 0
    for k in KEYS:
        assert (np.asarray(got[k]) == np.asarray(ref[k])).all(), (name, k)
    assert (got["iters"] > 1).any()


def test_clamped_inputs_on_a(F, codes):
    """Full-range random LLRs at 12/10: clamps act, the bounds (asserted by the model) hold."""
    code = codes["A"][0]
    got = FM.minsum_decode(FM.ModelCode.from_code(code), _rand(1, 6, code.n, 32768), 12, 10, max_iter=4)
    assert got["clipped"] > 0
    assert np.abs(got["post"]).max() <= 2047


def test_precheck_and_fixed_iterations(F, O, codes):
    code = codes["A"][0]
    mc = FM.ModelCode.from_code(code)
    llr = _llr(F, O, code, 8.0, 8)
    a = FM.minsum_decode(mc, llr, 12, 10, scale_16=12, precheck=True)
    assert a["prechecked"].any() and not a["prechecked"].all()
    assert (a["iters"][a["prechecked"]] == 0).all() and (a["iters"][~a["prechecked"]] >= 1).all()
    b = FM.minsum_decode(mc, llr, 12, 10, scale_16=12, max_iter=3, early_term=False)
    assert (b["iters"] == 3).all()


def _create_error(F, code, **kw):
    with pytest.raises(F.FpldpcError) as e:
        F.MinSumDecoder(code, **kw)
    return e.value


@pytest.mark.parametrize("kw,rule", [(dict(post_bits=10, msg_bits=10), "msg_bits < post_bits"),
                                     (dict(post_bits=8, msg_bits=10), "msg_bits < post_bits"),
                                     (dict(post_bits=17, msg_bits=10), "post_bits <= 16"),
                                     (dict(post_bits=12, msg_bits=1), "2 <= msg_bits"),
                                     (dict(scale_16=0), "1 <= scale_16 <= 16"), (dict(scale_16=17), "1 <= scale_16 <= 16"),
                                     (dict(offset=-1), "0 <= offset <= S_m (511)"),
                                     (dict(offset=512), "0 <= offset <= S_m (511)")])
def test_argument_rules_need_no_gpu(F, codes, kw, rule):
    """2 <= msg_bits < post_bits <= 16, 1 <= scale_16 <= 16, 0 <= offset <= S_m (511 at msg_bits = 10):
    FPLDPC_ERR_ARG with a message naming the rule, with or without a device."""
    err = _create_error(F, codes["A"][0], **kw)
    assert err.code == -1, err
    assert "flooding min-sum decoder" in str(err) and rule in str(err), err


def test_unused_parameters_are_validated(F, codes):
    """frac_bits and width_mask are not used, and validated as elsewhere (through the C ABI: the Python
    class leaves them at their defaults)."""
    import ctypes
    from fixedpointldpc_amd._lib import Params
    for field, bad in (("frac_bits", 17), ("width_mask", 0), ("max_iter", 0)):
        p = Params()
        F.lib().fpldpc_params_default(ctypes.byref(p))
        setattr(p, field, bad)
        h = ctypes.c_void_p()
        st = F.lib().fpldpc_minsum_create(codes["A"][0]._h, ctypes.byref(p), 12, 10, 16, 0, ctypes.byref(h))
        assert st == -1 and not h.value, field


def test_valid_arguments_without_gpu_fail_loudly(F, codes):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for kw in ({}, dict(post_bits=16, msg_bits=15, scale_16=12, offset=16383), dict(post_bits=10, msg_bits=8, scale_16=1)):
        err = _create_error(F, codes["A"][0], **kw)
        assert err.code == -5, err
