"""The numpy model of the saturated flooding decoder (tests/flood_sat_model.py) anchored to the reference: at
widths 16/15 no clamp acts, and the model equals the oracle's flooding decoder at the same frac_bits and
width_mask in every output; clamped inputs on A; precheck and fixed iterations; and the argument rules of
fpldpc_flood_create_sat, which are tested before a HIP device is looked for.  The model asserts the
definition's four bounds on every run.  CPU only."""
import numpy as np
import pytest

import flood_sat_model as FS

SEED = 123456789
KEYS = ("iters", "hard", "post", "syndrome_ok")


def _llr(F, O, code, eb, frames, frac=4):
    snr, sigma = F.snr_sigma(eb, code.rate)
    return O.gen_llr(SEED, 0, frames, code.n, snr, sigma, frac)


def _rand(seed, frames, n, lim):
    return np.random.default_rng(seed).integers(-lim, lim, (frames, n)).astype(np.int32)


def _pair(F, O, codes, name):
    if name in codes:
        return codes[name]
    code = F.Code.array(13, 2)
    return code, O.OracleCode.from_alist_text(code.write_alist())


# (code, Eb/N0, AWGN frames, random frames of +-300, max_iter, frac_bits, width mask): the anchor list of
# test_minsum_model.py at frac_bits 4, and A at frac_bits 6 / mask 0x1ff
ANCHOR = [("A", 4.5, 24, 8, 30, 4, 0xFF), ("R", 6.5, 8, 8, 50, 4, 0x3F), ("p13r2", 3.0, 24, 8, 8, 4, 0xFF),
          ("W", 2.0, 16, 0, 30, 4, 0xFF), ("A", 4.5, 24, 8, 30, 6, 0x1FF)]


@pytest.mark.parametrize("name,eb,frames,random,max_iter,frac,mask", ANCHOR)
def test_at_16_15_equals_the_oracle(F, O, codes, name, eb, frames, random, max_iter, frac, mask):
    """clipped == 0 is a condition on the inputs: where no clamp acts the definition is the reference's
    flooding decoder at the same frac_bits and width_mask."""
    code, ocode = _pair(F, O, codes, name)
    llr = _llr(F, O, code, eb, frames, frac)
    if random:
        llr = np.concatenate([llr, _rand(5, random, code.n, 300)])
    ref = O.decode_batch(ocode, llr, max_iter, frac, mask)
    got = FS.flood_sat_decode(FS.ModelCode.from_code(code), llr, 16, 15, max_iter=max_iter, frac_bits=frac, mask=mask)
    assert got["clipped"] == 0
    for k in KEYS:
        assert (np.asarray(got[k]) == np.asarray(ref[k])).all(), (name, k)
    assert (got["iters"] > 1).any()


def test_clamped_inputs_on_a(F, codes):
    """Full-range random LLRs at 12/10: clamps act, the bounds (asserted by the model) hold."""
    code = codes["A"][0]
    got = FS.flood_sat_decode(FS.ModelCode.from_code(code), _rand(1, 6, code.n, 32768), 12, 10, max_iter=4)
    assert got["clipped"] > 0
    assert np.abs(got["post"]).max() <= 2047


def test_precheck_and_fixed_iterations(F, O, codes):
    code = codes["A"][0]
    mc = FS.ModelCode.from_code(code)
    llr = _llr(F, O, code, 8.0, 8)
    a = FS.flood_sat_decode(mc, llr, 12, 10, precheck=True)
    assert a["prechecked"].any() and not a["prechecked"].all()
    assert (a["iters"][a["prechecked"]] == 0).all() and (a["iters"][~a["prechecked"]] >= 1).all()
    assert (a["post"][a["prechecked"]] == np.clip(llr, -2047, 2047)[a["prechecked"]]).all()
    b = FS.flood_sat_decode(mc, llr, 12, 10, max_iter=3, early_term=False)
    assert (b["iters"] == 3).all()


def _create_error(F, code, **kw):
    with pytest.raises(F.FpldpcError) as e:
        F.FloodSatDecoder(code, **kw)
    return e.value


@pytest.mark.parametrize("kw,rule", [(dict(post_bits=10, msg_bits=10), "msg_bits < post_bits"),
                                     (dict(post_bits=8, msg_bits=10), "msg_bits < post_bits"),
                                     (dict(post_bits=17, msg_bits=10), "post_bits <= 16"),
                                     (dict(post_bits=12, msg_bits=1), "2 <= msg_bits"),
                                     (dict(post_bits=5, msg_bits=4), "S_p > S_m + C"),
                                     (dict(post_bits=12, msg_bits=11, frac_bits=16), "S_p > S_m + C")])
def test_argument_rules_need_no_gpu(F, codes, kw, rule):
    """2 <= msg_bits < post_bits <= 16 and S_p > S_m + C (5/4 at frac_bits 4: 15 <= 7 + 10; 12/11 at
    frac_bits 16: 2047 <= 1023 + 40960): FPLDPC_ERR_ARG with a message naming the rule, with or without a
    device."""
    err = _create_error(F, codes["A"][0], **kw)
    assert err.code == -1, err
    assert "saturated flooding decoder:" in str(err) and rule in str(err), err


def test_parameters_are_validated(F, codes):
    """frac_bits, width_mask and max_iter are validated as elsewhere, through the C entry point."""
    import ctypes
    from fixedpointldpc_amd._lib import Params
    for field, bad in (("frac_bits", 17), ("width_mask", 0), ("max_iter", 0)):
        p = Params()
        F.lib().fpldpc_params_default(ctypes.byref(p))
        setattr(p, field, bad)
        h = ctypes.c_void_p()
        st = F.lib().fpldpc_flood_create_sat(codes["A"][0]._h, ctypes.byref(p), 12, 10, ctypes.byref(h))
        assert st == -1 and not h.value, field


def test_valid_arguments_without_gpu_fail_loudly(F, codes):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for kw in ({}, dict(post_bits=16, msg_bits=15), dict(post_bits=10, msg_bits=8), dict(post_bits=6, msg_bits=4)):
        err = _create_error(F, codes["A"][0], **kw)
        assert err.code == -5, err
