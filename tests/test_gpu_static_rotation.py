"""The packed A kernel (flood_pk<ArrayChecks<47>, 3>) against the oracle where its step loop's
bookkeeping can go wrong: the three rotating posterior buffers (a frame may start, end and be
refilled at any step mod 3, in either half, and hand over to the split tail from any of them), the
final-update syndrome pass, and the int16 range guard -- from two chain values (the default
parameters) or per output (large FRAC_WIDTH), two instantiations of the same kernel.
"""
import math

import numpy as np
import pytest

from conftest import assert_same

pytestmark = pytest.mark.gpu

SEED = 123456789
A_KERNEL = "flood_array2<P=47,W=3>"


@pytest.fixture(scope="module")
def acodes(F, O):
    out = {}
    for r in (5, 2):
        c = F.Code.array(47, r)
        out[r] = (c, O.OracleCode.from_alist_text(c.write_alist()))
    return out


def _mixed(O, code, frames, salt, ebs=(3.0, 4.0, 5.0, 6.0), never=0.1, clean=0.07):
    """AWGN frames at mixed Eb/N0, some that never converge, some noiseless, shuffled."""
    rng = np.random.default_rng(salt)
    per = -(-frames // len(ebs))
    parts = []
    for i, eb in enumerate(ebs):
        snr = 2 * math.pow(10.0, eb / 10) * code.rate
        parts.append(O.gen_llr(SEED, 1000 * salt + per * i, per, code.n, snr, math.sqrt(1 / snr), 4))
    llr = np.concatenate(parts)[:frames]
    nn, nc = int(round(never * frames)), int(round(clean * frames))
    pick = rng.permutation(frames)
    llr[pick[:nn]] = rng.integers(-60, 61, (nn, code.n))
    llr[pick[nn:nn + nc]] = 40
    return llr[rng.permutation(frames)]


def _decode(dec, llr, torch_dev):
    import torch
    out = dec.decode_torch(torch.from_numpy(llr.astype(np.int16)).to(torch_dev), post=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(F, code, gpu, ref, kw, where):
    """Against the oracle.  The oracle always stops at a passing syndrome; with early_term off the
    frames it ran to the cap are compared in full, the others must report the cap and the syndrome of
    their own final hard decisions."""
    pre = kw.get("precheck", False)
    if kw.get("early_term", True):
        assert_same(gpu, ref, code.n, check_post=not pre, where=where)
        if pre:
            ran = ref["iters"] > 0
            assert (gpu["post"][ran] == ref["post"][ran]).all(), where
        return
    cap = kw["max_iter"]
    full = ref["iters"] == cap
    stopped0 = (ref["iters"] == 0) if pre else np.zeros(len(ref["iters"]), bool)
    assert (gpu["iters"][~stopped0] == cap).all(), where
    assert (gpu["iters"][stopped0] == 0).all(), where
    sub = {k: np.asarray(v)[full] for k, v in gpu.items()}
    rsub = {k: np.asarray(v)[full] for k, v in ref.items() if v is not None}
    if full.any():
        assert_same(sub, rsub, code.n, where=where + " (frames at the cap)")
    hard = F.unpack_hard(gpu["hard"], code.n)
    assert [code.syndrome_ok(h) for h in hard] == [bool(o) for o in gpu["syndrome_ok"]], where


@pytest.fixture(scope="module")
def pools(O, acodes):
    """Per code: 600 mixed frames and their oracle decode at the defaults (computed once, read only)."""
    out = {}
    for r, (code, ocode) in acodes.items():
        llr = _mixed(O, code, 600, 23 + r)
        llr.setflags(write=False)
        out[r] = (llr, O.decode_batch(ocode, llr))
    return out


@pytest.mark.parametrize("r", [5, 2])
def test_small_batches_every_step_copy(F, O, acodes, pools, torch_dev, r):
    """Batches 1, 2, 3, 5 at max_iter 1..5 and 7, early_term and precheck on and off, over frames that
    converge after 3, 2 and 4 updates, one that never does and a noiseless one: frames end after
    0..7 steps, so at every step mod 3, on the step's own syndrome and on the final-update pass."""
    code, ocode = acodes[r]
    pool, pref = pools[r]
    it = pref["iters"]
    noiseless = np.nonzero((pool == 40).all(axis=1))[0][0]
    llr = pool[[np.nonzero(it == 3)[0][0], np.nonzero(it == 30)[0][0], np.nonzero(it == 2)[0][0], noiseless,
                np.nonzero(it == 4)[0][0]]]
    ends = set()
    for mi in (1, 2, 3, 4, 5, 7):
        for pre in (False, True):
            full = O.decode_batch(ocode, llr, max_iter=mi, precheck=pre)
            ends |= {(int(x), pre) for x in full["iters"]}
            for et in (True, False):
                kw = dict(max_iter=mi, precheck=pre, early_term=et)
                dec = F.Decoder(code, **kw)
                assert dec.describe().startswith(A_KERNEL), dec.describe()
                for B in (1, 2, 3, 5):
                    ref = {k: (v[:B] if v is not None else None) for k, v in full.items()}
                    gpu = _decode(dec, llr[:B], torch_dev)
                    _check(F, code, gpu, ref, kw, f"p47r{r} {kw} B={B}")
    assert {e for e, _ in ends} == {0, 1, 2, 3, 4, 5, 7}, ends


@pytest.mark.parametrize("split", ["1", "0"])
@pytest.mark.parametrize("r", [5, 2])
def test_refills_in_every_copy(F, O, acodes, pools, torch_dev, monkeypatch, r, split):
    """600 frames on 256 workgroups (one per CU): every half is refilled, the two halves of a lane
    start at different steps mod 3, and lone frames hand over to the split tail (or not) from each."""
    monkeypatch.setenv("FPLDPC_GRID_PER_CU", "1")
    monkeypatch.setenv("FPLDPC_SPLIT_TAIL", split)
    code, ocode = acodes[r]
    llr, ref = pools[r]
    it = ref["iters"]
    assert {int(x) % 3 for x in it} == {0, 1, 2} and (it == 30).sum() >= 20 and (it <= 6).sum() >= 100, np.bincount(it)
    dec = F.Decoder(code)
    assert dec.describe().startswith(A_KERNEL) and "grid=256" in dec.describe(), dec.describe()
    gpu = _decode(dec, llr, torch_dev)
    assert_same(gpu, ref, code.n, where=f"p47r{r} split={split} [{dec.describe()}]")
    refp = O.decode_batch(ocode, llr, precheck=True)
    gpu = _decode(F.Decoder(code, precheck=True), llr, torch_dev)
    assert_same(gpu, refp, code.n, check_post=False, where=f"p47r{r} split={split} precheck")


def test_range_guard_chain_form(F, O, acodes, torch_dev):
    """64 frames at 0 dB, 12 of them with every |LLR| in 5000..8000 (c2v above cmax = 4095 in their
    first iteration): outputs equal the oracle, the 12 go down the fallback (with at most one partner
    each), and a plain 0 dB batch leaves the fallback untouched."""
    code, ocode = acodes[5]
    dec = F.Decoder(code)
    assert dec.describe().startswith(A_KERNEL), dec.describe()
    snr = 2 * math.pow(10.0, 0.0) * code.rate
    sigma = math.sqrt(1 / snr)
    rng = np.random.default_rng(11)
    B, nbig = 64, 12
    llr = O.gen_llr(SEED, 0, B, code.n, snr, sigma, 4)
    assert np.abs(llr).max() <= 8000
    big = np.sort(rng.choice(B, nbig, replace=False))
    llr[big] = rng.integers(5000, 8001, (nbig, code.n)) * rng.choice([-1, 1], (nbig, code.n))
    ref = O.decode_batch(ocode, llr)
    gpu = _decode(dec, llr, torch_dev)
    fb = dec.fallback_counts()
    assert_same(gpu, ref, code.n, where=f"range guard [{dec.describe()}] fallbacks={fb}")
    assert nbig <= fb[0] <= 2 * nbig and fb[1] == 0, fb
    plain = O.gen_llr(SEED, 4096, 256, code.n, snr, sigma, 4)
    gpu = _decode(dec, plain, torch_dev)
    assert dec.fallback_counts() == (0, 0)
    assert_same(gpu, O.decode_batch(ocode, plain), code.n, where="plain 0 dB")


def test_range_guard_per_output_form(F, O, acodes, torch_dev):
    """FRAC_WIDTH 8 (C = 160: G = 24 C = 3840 > 512): the same kernel with the per-output guard."""
    code, ocode = acodes[5]
    cg = __import__("ctypes").c_int32(-1)
    assert F.lib().fpldpc_testing_range_guard(code.dv_max, 160, 24, cg) == 4095 and cg.value == 0
    dec = F.Decoder(code, frac_bits=8, width_mask=0xFF)
    assert dec.describe().startswith(A_KERNEL), dec.describe()
    rng = np.random.default_rng(5)
    parts = []
    for i, eb in enumerate((0.0, 3.0, 5.0)):
        snr = 2 * math.pow(10.0, eb / 10) * code.rate
        parts.append(O.gen_llr(SEED, 300 * i, 24, code.n, snr, math.sqrt(1 / snr), 8))
    parts.append(rng.integers(5000, 8001, (6, code.n)) * rng.choice([-1, 1], (6, code.n)))
    parts.append(rng.integers(-2000, 2001, (6, code.n)))
    llr = np.concatenate(parts).astype(np.int32)
    ref = O.decode_batch(ocode, llr, frac_bits=8, mask=0xFF)
    import torch
    out = dec.decode_torch(torch.from_numpy(llr).to(torch_dev), post=True)
    torch.cuda.synchronize()
    fb = dec.fallback_counts()
    assert_same({k: v.cpu().numpy() for k, v in out.items()}, ref, code.n, where=f"frac 8 [{dec.describe()}] fallbacks={fb}")
    assert fb[0] >= 6, fb
