"""The numpy model of the saturated layered decoder (tests/layered_sat_model.py): pinned to the
unsaturated model where no clamp acts, layer size still not semantics, the high-SNR cases the
unsaturated decoder cannot run (its intermediates leave int32 there), and the argument rules of
fpldpc_layered_create_sat, which are tested before a HIP device is looked for.  CPU only."""
import numpy as np
import pytest

import layered_model as M
import layered_sat_model as S

SEED = 123456789
KEYS = ("iters", "hard", "post", "syndrome_ok")


def _llr(F, O, code, eb, frames):
    snr, sigma = F.snr_sigma(eb, code.rate)
    return O.gen_llr(SEED, 0, frames, code.n, snr, sigma, 4)


@pytest.fixture(scope="module")
def mcodes(codes):
    return {k: M.ModelCode.from_code(c) for k, (c, _) in codes.items()}


@pytest.mark.parametrize("name,eb,frames,max_iter", [("A", 4.5, 6, 3), ("W", 2.0, 4, 4)])
def test_wide_widths_equal_the_unsaturated_model(F, O, codes, mcodes, name, eb, frames, max_iter):
    """(24, 23) on inputs whose unsaturated peak stays below S_m: no clamp acts and the two models agree."""
    code = codes[name][0]
    llr = _llr(F, O, code, eb, frames)
    L = code.layering()[0]
    ref = M.layered_decode(mcodes[name], llr, L, max_iter=max_iter)
    assert ref["peak"] < S.limits(24, 23)[1], ref["peak"]
    got = S.layered_sat_decode(mcodes[name], llr, L, 24, 23, max_iter=max_iter)
    assert got["clipped"] == 0
    for k in KEYS:
        assert (got[k] == ref[k]).all(), k
    assert (ref["iters"] > 1).any()


def test_layer_size_is_not_semantics(F, O, codes, mcodes):
    llr = _llr(F, O, codes["A"][0], 4.5, 4)
    a = S.layered_sat_decode(mcodes["A"], llr, 47, 12, 10, max_iter=5)
    b = S.layered_sat_decode(mcodes["A"], llr, 1, 12, 10, max_iter=5)
    for k in KEYS + ("clipped", "c2v_peak"):
        assert (np.asarray(a[k]) == np.asarray(b[k])).all(), k


def test_a_at_8db_without_early_termination(F, O, codes, mcodes):
    """(12, 10) decodes every frame; the same frames reach beyond S_m unsaturated, so the clamps act."""
    llr = _llr(F, O, codes["A"][0], 8.0, 8)
    got = S.layered_sat_decode(mcodes["A"], llr, 47, 12, 10, max_iter=4, early_term=False)
    assert (got["iters"] == 4).all() and got["syndrome_ok"].all()
    assert got["clipped"] > 0
    unsat = M.layered_decode(mcodes["A"], llr, 47, max_iter=4, early_term=False)
    assert unsat["peak"] > S.limits(12, 10)[1]
    print(f"A @ 8 dB: unsaturated peak {unsat['peak']}, clipped {got['clipped']}, c2v peak {got['c2v_peak']}")


def test_r_at_8db_two_iterations(F, O, codes, mcodes):
    """What the feature exists for: the unsaturated definition leaves int32 here (the int64 model
    shows how far), the saturated one decodes every frame."""
    llr = _llr(F, O, codes["R"][0], 8.0, 2)
    unsat = M.layered_decode(mcodes["R"], llr, 47, max_iter=2, early_term=False)
    assert unsat["peak"] >= 2 ** 31, unsat["peak"]
    got = S.layered_sat_decode(mcodes["R"], llr, 47, 12, 10, max_iter=2, early_term=False)
    assert (got["iters"] == 2).all() and got["syndrome_ok"].all()
    print(f"R @ 8 dB: unsaturated peak {unsat['peak']:.3g}, clipped {got['clipped']}")


def _create_code(F, code, **kw):
    with pytest.raises(F.FpldpcError) as e:
        F.LayeredDecoder(code, **kw)
    return e.value


@pytest.mark.parametrize("post_bits,msg_bits,frac", [(10, 10, 4), (8, 10, 4), (25, 10, 4), (12, 1, 4), (8, 7, 8)])
def test_width_rules_need_no_gpu(F, codes, post_bits, msg_bits, frac):
    """2 <= msg_bits < post_bits <= 24 and S_p > S_m + C (frac_bits = 8: C = 160, and 127 <= 63 + 160):
    FPLDPC_ERR_ARG with a message, with or without a device."""
    err = _create_code(F, codes["A"][0], post_bits=post_bits, msg_bits=msg_bits, frac_bits=frac)
    assert err.code == -1, err
    assert "saturated layered decoder" in str(err), err


def test_valid_widths_without_gpu_fail_loudly(F, codes):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for widths in ((12, 10), (16, 15), (20, 12)):
        err = _create_code(F, codes["A"][0], post_bits=widths[0], msg_bits=widths[1])
        assert err.code == -5, err
