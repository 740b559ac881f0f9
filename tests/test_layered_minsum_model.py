"""The numpy model of the layered min-sum decoder (tests/layered_minsum_model.py): plain min-sum
(scale_16 = 16, offset = 0) pinned to the saturated sxor model at frac_bits = 0, where the reference's
Constant is 0 and sxor is sign * min; layer size still not semantics; decoding behaviour on A; and the
argument rules of fpldpc_layered_create_minsum, which are tested before a HIP device is looked for.
The model asserts the definition's bounds, and that the compressed check state rebuilds every message,
on every run.  CPU only."""
import numpy as np
import pytest

import layered_minsum_model as MS
import layered_model as M
import layered_sat_model as S
from test_gpu_layered_sat import irregular_alist

SEED = 123456789
KEYS = ("iters", "hard", "post", "syndrome_ok")


def _llr(F, O, code, eb, frames, first=0):
    snr, sigma = F.snr_sigma(eb, code.rate)
    return O.gen_llr(SEED, first, frames, code.n, snr, sigma, 4)


def _rand(seed, frames, n, lim):
    return np.random.default_rng(seed).integers(-lim, lim, (frames, n)).astype(np.int32)


def _same(got, ref, where):
    for k in KEYS:
        assert (np.asarray(got[k]) == np.asarray(ref[k])).all(), (where, k)


@pytest.fixture(scope="module")
def a_frames(F, O, codes):
    code = codes["A"][0]
    llr = np.concatenate([_llr(F, O, code, 4.5, 24), _llr(F, O, code, 8.0, 4), _rand(1, 6, code.n, 32768),
                          _rand(3, 4, code.n, 3)])
    assert (llr[-4:] == 0).any() and np.abs(llr[28:34]).max() > 32000
    return M.ModelCode.from_code(code), llr


@pytest.mark.parametrize("widths", [(12, 10), (16, 15), (10, 8)])
def test_plain_minsum_equals_the_sxor_model_at_frac_bits_0_on_a(a_frames, widths):
    mc, llr = a_frames
    ref = S.layered_sat_decode(mc, llr, 47, *widths, max_iter=6, frac_bits=0)
    got = MS.layered_minsum_decode(mc, llr, 47, *widths, max_iter=6)
    _same(got, ref, f"A {widths}")
    assert got["clipped"] == ref["clipped"]
    assert (ref["iters"] > 1).any()


def test_plain_minsum_equals_the_sxor_model_at_frac_bits_0_on_other_codes(F, O, codes):
    w = codes["W"][0]
    cases = [("W", w, _llr(F, O, w, 2.0, 8), w.layering()[0]),
             ("array13x2", F.Code.array(13, 2), None, 13),
             ("irregular", F.Code.parse(irregular_alist()), None, 1)]
    for name, code, llr, L in cases:
        if llr is None:
            llr = _rand(30, 16, code.n, 3000)
        mc = M.ModelCode.from_code(code)
        ref = S.layered_sat_decode(mc, llr, L, 12, 10, max_iter=6, frac_bits=0)
        _same(MS.layered_minsum_decode(mc, llr, L, 12, 10, max_iter=6), ref, name)


@pytest.mark.parametrize("name,eb,frames,La,Lb", [("A", 4.5, 4, 1, 47), ("W", 2.0, 4, 27, 81)])
def test_layer_size_is_not_semantics(F, O, codes, name, eb, frames, La, Lb):
    code = codes[name][0]
    mc = M.ModelCode.from_code(code)
    llr = _llr(F, O, code, eb, frames)
    a = MS.layered_minsum_decode(mc, llr, La, 12, 10, scale_16=12, offset=1, max_iter=5)
    b = MS.layered_minsum_decode(mc, llr, Lb, 12, 10, scale_16=12, offset=1, max_iter=5)
    _same(a, b, f"{name} L={La} / L={Lb}")
    assert a["clipped"] == b["clipped"]


def test_a_at_4_5_db_decodes_every_frame(F, O, codes):
    """24 frames of the oracle's channel at widths 12/10, scale 12/16: a condition on the inputs."""
    code = codes["A"][0]
    got = MS.layered_minsum_decode(M.ModelCode.from_code(code), _llr(F, O, code, 4.5, 24), 47, 12, 10, scale_16=12)
    print(f"A @ 4.5 dB, scale 12/16: iterations {got['iters'].tolist()}")
    assert got["syndrome_ok"].all()
    assert 1 < got["iters"].mean() < 30


def test_corrected_magnitudes():
    x = np.arange(0, 16384, dtype=np.int64)
    assert (MS.correct(x, 16, 0) == x).all()
    assert (MS.correct(x, 12, 0) == (x * 3) >> 2).all()
    assert (MS.correct(x, 16, 8) == np.maximum(x - 8, 0)).all()


def _create_error(F, code, **kw):
    with pytest.raises(F.FpldpcError) as e:
        F.LayeredDecoder(code, check="minsum", **kw)
    return e.value


@pytest.mark.parametrize("kw", [dict(post_bits=10, msg_bits=10), dict(post_bits=8, msg_bits=10),
                                dict(post_bits=17, msg_bits=10), dict(post_bits=12, msg_bits=1),
                                dict(post_bits=12, msg_bits=10, scale_16=0), dict(post_bits=12, msg_bits=10, scale_16=17),
                                dict(post_bits=12, msg_bits=10, offset=-1), dict(post_bits=12, msg_bits=10, offset=512)])
def test_argument_rules_need_no_gpu(F, codes, kw):
    """2 <= msg_bits < post_bits <= 16, 1 <= scale_16 <= 16, 0 <= offset <= S_m (511 at msg_bits = 10):
    FPLDPC_ERR_ARG with a message, with or without a device."""
    err = _create_error(F, codes["A"][0], **kw)
    assert err.code == -1, err
    assert "layered min-sum decoder" in str(err), err


def test_python_keyword(F, codes):
    code = codes["A"][0]
    with pytest.raises(ValueError):
        F.LayeredDecoder(code, check="minsum")
    with pytest.raises(ValueError):
        F.LayeredDecoder(code, check="minsum", post_bits=12)
    with pytest.raises(ValueError):
        F.LayeredDecoder(code, check="spa", post_bits=12, msg_bits=10)
    with pytest.raises(ValueError):
        F.LayeredDecoder(code, post_bits=12, msg_bits=10, scale_16=12)


def test_valid_arguments_without_gpu_fail_loudly(F, codes):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for kw in (dict(post_bits=12, msg_bits=10), dict(post_bits=16, msg_bits=15, scale_16=12, offset=16383),
               dict(post_bits=10, msg_bits=8, scale_16=1)):
        err = _create_error(F, codes["A"][0], **kw)
        assert err.code == -5, err
