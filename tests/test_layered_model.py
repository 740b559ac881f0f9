"""The numpy model of the layered schedule (tests/layered_model.py) pinned to the oracle, the layer
validation of the library (fpldpc_code_layering, host only) and the point of the schedule: fewer
iterations than flooding on the waterfall workloads.  CPU only."""
import numpy as np
import pytest

import layered_model as M

SEED = 123456789


def _llr(F, O, code, eb, frames):
    snr, sigma = F.snr_sigma(eb, code.rate)
    return O.gen_llr(SEED, 0, frames, code.n, snr, sigma, 4)


@pytest.fixture(scope="module")
def mcodes(codes):
    return {k: M.ModelCode.from_code(c) for k, (c, _) in codes.items()}


@pytest.mark.parametrize("mask", [0xFF, 0x3F])
def test_model_sxor_is_the_oracles(O, mask):
    v = np.arange(-300, 301)
    got = M.sxor(v[:, None], v[None, :], M.constant(4), mask)
    assert (got == O.sxor_table(-300, 300, 4, mask)).all()


@pytest.mark.parametrize("name,eb,frames", [("A", 4.5, 6), ("W", 2.0, 4)])
def test_flooding_from_model_fold_equals_oracle(F, O, codes, mcodes, name, eb, frames):
    """A flooding decoder built from the model's check_update equals the oracle in iterations and
    posteriors: the fold order and sxor of the model are the reference's."""
    code, ocode = codes[name]
    llr = _llr(F, O, code, eb, frames)
    ref = O.decode_batch(ocode, llr, max_iter=30)
    got = M.flooding_decode(mcodes[name], llr, max_iter=30)
    assert got["peak"] < 2 ** 31
    assert (got["iters"] == ref["iters"]).all()
    assert (got["post"] == ref["post"]).all()
    assert (got["hard"] == ref["hard"]).all() and (got["syndrome_ok"] == ref["syndrome_ok"]).all()


@pytest.mark.parametrize("name,eb,frames,big,small", [("A", 4.5, 4, 47, 1), ("W", 2.0, 4, 81, 27)])
def test_layer_size_is_not_semantics(F, O, codes, mcodes, name, eb, frames, big, small):
    code, _ = codes[name]
    llr = _llr(F, O, code, eb, frames)
    a = M.layered_decode(mcodes[name], llr, big, max_iter=5)
    b = M.layered_decode(mcodes[name], llr, small, max_iter=5)
    assert max(a["peak"], b["peak"]) < 2 ** 31
    for k in ("iters", "hard", "post", "syndrome_ok"):
        assert (a[k] == b[k]).all(), k


# three checks, checks 0 and 1 share variable 1: no layer of more than one check starts at check 0
HAND_ALIST = "4 3\n2 2\n1 2 2 1\n2 2 2\n0\n0 1\n1 2\n2\n0 1\n1 2\n2 3\n"


def test_code_layering(F, codes):
    """Auto picks p / Z; FPLDPC_ERR_ARG when L does not divide m, FPLDPC_ERR_UNSUPPORTED when a
    variable repeats inside a layer (include/fpldpc.h).  A has m = 235 = 5 * 47 checks: 94 and 10 do
    not divide it (ERR_ARG by the header's rule -- two block rows in one layer is the UNSUPPORTED
    case, tested where 94 divides m, on R, and on A with its divisors 5 and 235)."""
    A, W, R = (codes[k][0] for k in "AWR")
    assert A.layering() == (47, 5) and A.layering(0) == (47, 5)
    assert W.layering() == (81, 12)
    assert R.layering() == (47, 24)
    for c in (A, W, R):
        assert c.layering(1) == (1, c.m)
    assert W.layering(27) == (27, 36)
    for code, L, err in ((A, 94, -1), (A, 10, -1), (A, -1, -1), (R, 94, -4), (A, 5, -4), (A, 235, -4), (W, 162, -4)):
        with pytest.raises(F.FpldpcError) as e:
            code.layering(L)
        assert e.value.code == err, (L, e.value)
    hand = F.Code.parse(HAND_ALIST)
    assert hand.layering() == (1, 3)
    with pytest.raises(F.FpldpcError) as e:
        hand.layering(3)
    assert e.value.code == -4


def test_layered_create_without_gpu_fails_loudly(F, codes):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(F.FpldpcError) as e:
        F.LayeredDecoder(codes["A"][0])
    assert e.value.code == -5


@pytest.mark.parametrize("name,eb,frames", [("A", 4.5, 64), ("W", 2.0, 48)])
def test_layered_needs_fewer_iterations_than_flooding(F, O, codes, mcodes, name, eb, frames):
    code, ocode = codes[name]
    llr = _llr(F, O, code, eb, frames)
    flood = O.decode_batch(ocode, llr, max_iter=30, want_post=False)
    lay = M.layered_decode(mcodes[name], llr, code.layering()[0], max_iter=30)
    assert lay["peak"] < 2 ** 31
    print(f"{name} @ {eb} dB, {frames} frames: flooding {flood['iters'].mean():.2f}, layered {lay['iters'].mean():.2f} "
          f"mean iterations; {(lay['iters'] > flood['iters']).sum()} frames need more; peak {lay['peak']}")
    assert lay["iters"].mean() < flood["iters"].mean()
