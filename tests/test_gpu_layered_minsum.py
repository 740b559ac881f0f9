"""The layered min-sum decoder on the GPU (fpldpc_layered_create_minsum, LayeredDecoder(check="minsum"))
against the numpy model of its definition (tests/layered_minsum_model.py): iterations, hard decisions,
syndrome flags and posteriors exactly, on every path of the kernel -- A (exact degree, computed
addresses), W (table in global memory and in LDS, layers wider than a wave, degrees 7 and 8 in DC = 8),
R (its check state in LDS: there is no global scratch), every predicated width, small and irregular
codes, every mode.  The model asserts the definition's bounds and the rebuild of every message from the
compressed state on every run."""
import re

import numpy as np
import pytest

import layered_minsum_model as MS
import layered_model as M
from conftest import assert_same
from test_gpu_layered_sat import awgn, rand, run, small_code

pytestmark = pytest.mark.gpu


def model(code, llr, widths, L=0, **kw):
    return MS.layered_minsum_decode(M.ModelCode.from_code(code), llr, L or code.layering()[0], *widths, **kw)


def lds_of(d):
    return int(re.search(r" lds=(\d+) ", d).group(1))


@pytest.fixture(scope="module")
def case_a(F, O, codes):
    """The A frames most tests share, with their model results per (widths, scale_16, offset), each computed once."""
    code = codes["A"][0]
    llr = np.concatenate([awgn(F, O, code, 4.5, 24), awgn(F, O, code, 8.0, 8), rand(1, 8, code.n, 32768),
                          rand(3, 4, code.n, 3)])
    assert (llr[-4:] == 0).any() and np.abs(llr[32:40]).max() > 32000 and np.abs(llr).max() < 32768
    refs = {}

    def ref(widths=(12, 10), scale_16=16, offset=0):
        key = (widths, scale_16, offset)
        if key not in refs:
            refs[key] = model(code, llr, widths, scale_16=scale_16, offset=offset)
        return refs[key]
    return code, llr, ref


@pytest.mark.parametrize("widths,scale_16,offset", [((12, 10), 16, 0), ((12, 10), 12, 0), ((12, 10), 16, 8), ((12, 10), 13, 3),
                                                    ((16, 15), 16, 0), ((10, 8), 16, 0)])
def test_a(F, case_a, torch_dev, widths, scale_16, offset):
    """2209 int16 posteriors (4420 B with the pad), the control words and 16 B for each of the 235 checks."""
    code, llr, ref = case_a
    r = ref(widths, scale_16, offset)
    dec = F.LayeredDecoder(code, check="minsum", post_bits=widths[0], msg_bits=widths[1], scale_16=scale_16, offset=offset)
    assert_same(run(dec, llr, torch_dev), r, code.n, where=f"A {widths} {scale_16}/16-{offset}")
    d = dec.describe()
    assert d.startswith("layered_minsum<DC=47,addr=computed,deg=exact> L=47 layers=5 "), d
    assert d.endswith(f" sat={widths[0]}/{widths[1]} ms={scale_16}/16-{offset} state=compressed"), d
    assert " threads=64 " in d and lds_of(d) <= 4420 + 64 + 16 * 235, d
    assert r["iters"][:24].mean() > 1
    if widths == (12, 10):  # (at (10, 8) plain min-sum decodes none of these frames: all 30 iterations are compared)
        assert r["iters"][:24].mean() < 30 and r["clipped"] > 0


@pytest.mark.parametrize("table", ["global", "lds"])
def test_w(F, O, codes, torch_dev, monkeypatch, table):
    code = codes["W"][0]
    llr = awgn(F, O, code, 2.0, 16)
    monkeypatch.setenv("FPLDPC_LAYERED_TABLE", table)
    dec = F.LayeredDecoder(code, check="minsum", post_bits=12, msg_bits=10, scale_16=12)
    monkeypatch.delenv("FPLDPC_LAYERED_TABLE")
    d = dec.describe()
    assert d.startswith(f"layered_minsum<DC=8,addr={'table' if table == 'lds' else 'gtable'},deg=table> L=81 layers=12 "), d
    assert "threads=128" in d and d.endswith(" sat=12/10 ms=12/16-0 state=compressed"), d
    # posteriors and control words, 17 B per check, and the table [8][972] uint16 when it is staged
    assert lds_of(d) <= 3888 + 64 + 17 * 972 + (2 * 8 * 972 if table == "lds" else 0), d
    assert_same(run(dec, llr, torch_dev), model(code, llr, (12, 10), scale_16=12), code.n, where=f"W table={table}")


def test_w_table_placement_rule(F, codes):
    """Without the switch the table is staged in LDS only where that costs no resident workgroup."""
    d = F.LayeredDecoder(codes["W"][0], check="minsum", post_bits=12, msg_bits=10).describe()
    assert re.match(r"layered_minsum<DC=8,addr=g?table,deg=table> L=81 layers=12 ", d), d


def test_r(F, O, codes, torch_dev):
    """R at 8 dB, 3 iterations without early termination.  The state of its 1128 checks is 18 KB of LDS,
    where the per-edge int16 c2v of the sxor decoder takes 106 KB and goes to a global scratch."""
    code = codes["R"][0]
    llr = awgn(F, O, code, 8.0, 4)
    ref = model(code, llr, (12, 10), max_iter=3, early_term=False)
    assert ref["syndrome_ok"].all() and ref["clipped"] > 0
    dec = F.LayeredDecoder(code, max_iter=3, early_term=False, check="minsum", post_bits=12, msg_bits=10)
    d = dec.describe()
    assert d.startswith("layered_minsum<DC=47,addr=computed,deg=exact> L=47 layers=24 "), d
    assert "c2v=global" not in d and lds_of(d) <= 4436 + 64 + 16 * 1128, d
    assert_same(run(dec, llr, torch_dev), ref, code.n, where="R")


@pytest.mark.parametrize("which", ["irregular", "array13x2", "array31x2", "array37x2", "array59x2"])
def test_small_codes(F, torch_dev, which):
    """An irregular code (L = 1, table addressing, degrees 2..6: DC = 8) and one array code per other
    predicated width: degrees 13, 31, 37 and 59 take DC = 16, 32, 48 and 64 (the sign word's upper half
    from slot 32 on); p odd makes n odd, so the int16 posteriors end on half a word.  Random +-300 LLRs
    with zeros among them, offset min-sum with a scale."""
    code, L = small_code(F, which)
    llr = rand(30, 64, code.n, 300)
    assert (llr == 0).any()
    ref = model(code, llr, (12, 10), L, scale_16=14, offset=2, max_iter=8)
    dec = F.LayeredDecoder(code, max_iter=8, layer_checks=L, check="minsum", post_bits=12, msg_bits=10, scale_16=14,
                           offset=2)
    d = dec.describe()
    dc = next(x for x in (8, 16, 32, 48, 64) if code.dc_max <= x)
    assert d.startswith(f"layered_minsum<DC={dc},addr={'computed' if which != 'irregular' else 'table'},deg=table> "), d
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=which)
    if which == "irregular":
        _, cdeg, _, _ = code.lists()
        assert min(cdeg) == 2


def test_plain_minsum_equals_the_sxor_decoder_at_frac_bits_0(F, case_a, torch_dev):
    """On the device: C = 0 makes the sxor fold sign * min, so the two kernels agree output for output."""
    code, llr, _ = case_a
    a = run(F.LayeredDecoder(code, check="minsum", post_bits=12, msg_bits=10), llr, torch_dev)
    b = run(F.LayeredDecoder(code, frac_bits=0, post_bits=12, msg_bits=10), llr, torch_dev)
    for k in b:
        assert (a[k] == b[k]).all(), k


@pytest.mark.parametrize("precheck", [False, True])
def test_precheck(F, O, codes, precheck):
    """A passing channel syndrome returns 0 iterations with the channel decision and leaves the posteriors untouched."""
    code = codes["A"][0]
    llr = awgn(F, O, code, 8.0, 16)
    ref = model(code, llr, (12, 10), scale_16=12, precheck=precheck)
    pre = ref["prechecked"]
    assert pre.any() == precheck and not pre.all()
    sentinel = np.full(llr.shape, -123456, np.int32)
    dec = F.LayeredDecoder(code, precheck=precheck, check="minsum", post_bits=12, msg_bits=10, scale_16=12)
    out = dec.decode_host(llr, post=sentinel.copy())
    assert_same(out, ref, code.n, check_post=False, where=f"precheck={precheck}")
    assert (out["iters"][pre] == 0).all() and (out["iters"][~pre] >= 1).all()
    assert (out["post"][pre] == -123456).all()
    assert (out["post"][~pre] == ref["post"][~pre]).all()


def test_max_iter_1(F, case_a, torch_dev):
    code, llr, _ = case_a
    ref = model(code, llr[:16], (12, 10), max_iter=1)
    dec = F.LayeredDecoder(code, max_iter=1, check="minsum", post_bits=12, msg_bits=10)
    assert_same(run(dec, llr[:16], torch_dev), ref, code.n, where="max_iter=1")
    assert (ref["iters"] == 1).all()


def test_int16_and_int32_llr(F, case_a, torch_dev):
    """The same frames as int16 and as int32 LLRs; then int32 LLRs beyond int16: the input clamp runs first."""
    code, llr, ref = case_a
    dec = F.LayeredDecoder(code, check="minsum", post_bits=12, msg_bits=10)
    a, b = run(dec, llr, torch_dev, np.int16), run(dec, llr, torch_dev, np.int32)
    assert_same(a, ref(), code.n, where="int16")
    for k in a:
        assert (a[k] == b[k]).all(), k
    big = llr[28:36].astype(np.int64) * 4097 + np.sign(llr[28:36]) * 65536
    assert np.abs(big).max() > 2 ** 23 and np.abs(big).max() < 2 ** 31
    big = big.astype(np.int32)
    assert_same(run(dec, big, torch_dev), model(code, big, (12, 10)), code.n, where="int32 beyond S_p")


def test_more_frames_than_the_grid(F, torch_dev):
    """The resident grid plus 3 frames on a small code: workgroups pull a second frame, whose state starts at zero."""
    code = F.Code.array(7, 3)
    dec = F.LayeredDecoder(code, max_iter=4, check="minsum", post_bits=12, msg_bits=10, scale_16=12)
    grid = int(dec.describe().split("grid=")[1].split()[0])
    assert 0 < grid < 100000
    llr = rand(31, 64, code.n, 3000)
    ref = model(code, llr, (12, 10), scale_16=12, max_iter=4)
    sel = np.tile(np.arange(64), -(-(grid + 3) // 64))[:grid + 3]
    big = {k: ref[k][sel] for k in ("iters", "hard", "syndrome_ok", "post")}
    assert_same(run(dec, llr[sel], torch_dev), big, code.n, where=f"batch {grid + 3}")


def test_two_calls_on_a_stream(F, case_a, torch_dev):
    import torch
    code, llr, ref = case_a
    dec = F.LayeredDecoder(code, check="minsum", post_bits=12, msg_bits=10)
    t = torch.from_numpy(llr).to(torch_dev)
    s = torch.cuda.Stream(torch_dev)
    torch.cuda.synchronize()
    a = dec.decode_torch(t, post=True, stream=s)
    b = dec.decode_torch(t, post=True, stream=s)
    s.synchronize()
    for out in (a, b):
        assert_same({k: v.cpu().numpy() for k, v in out.items()}, ref(), code.n, where="stream")


def test_counters(F, case_a, torch_dev):
    """bit_errors per frame and totals {bit errors, frames in error, frames, iteration sum} from the
    model's hard decisions; totals are added to across calls."""
    import torch
    code, llr, ref = case_a
    r = ref()
    idx = np.arange(0, code.n, 3, dtype=np.int32)
    bits = (np.arange(len(idx)) % 5 == 0).astype(np.uint8)
    want = (r["hard"][:, idx] != bits).sum(axis=1)
    dec = F.LayeredDecoder(code, check="minsum", post_bits=12, msg_bits=10)
    dec.set_reference(idx, bits)
    tot = torch.zeros(4, dtype=torch.int64, device=torch_dev)
    out = None
    for _ in range(2):
        out = run(dec, llr, torch_dev, bit_errors=True, totals=tot)
    assert (out["bit_errors"] == want).all()
    one = np.array([want.sum(), (want > 0).sum(), len(llr), r["iters"].sum()])
    assert (tot.cpu().numpy() == 2 * one).all(), (tot, one)
    host = dec.decode_host(llr, bit_errors=True, totals=np.array([1, 2, 3, 4]))
    assert (host["bit_errors"] == want).all() and (host["totals"] == one + [1, 2, 3, 4]).all()
