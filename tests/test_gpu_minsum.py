"""The flooding min-sum decoder on the GPU (fpldpc_minsum_create, MinSumDecoder) against the numpy model of
its definition (tests/minsum_model.py): iterations, hard decisions, syndrome flags and posteriors exactly,
on every path of the kernel -- A (exact degree, computed addresses, one lane per check), W (table in global
memory and in LDS, degrees 7 and 8 in DC = 8), R (several checks per lane, a partial last pass), every
predicated width, small and irregular codes, every mode -- and, where no clamp acts, against the shipped
flooding decoder and the oracle at frac_bits = 0.  The model asserts the definition's bounds and the
rebuild of every message from the compressed state on every run."""
import re

import numpy as np
import pytest

import minsum_model as FM
from conftest import assert_same
from test_gpu_layered_sat import awgn, rand, run, small_code

pytestmark = pytest.mark.gpu


def model(code, llr, widths, **kw):
    return FM.minsum_decode(FM.ModelCode.from_code(code), llr, *widths, **kw)


def lds_of(d):
    return int(re.search(r" lds=(\d+) ", d).group(1))


def lds_cap(code, table=False):
    """14 n + 17 m + 256 bytes, plus the index table [dc_max][m] uint16 when it is staged."""
    return 14 * code.n + 17 * code.m + 256 + (2 * code.dc_max * code.m if table else 0)


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
    code, llr, ref = case_a
    r = ref(widths, scale_16, offset)
    dec = F.MinSumDecoder(code, post_bits=widths[0], msg_bits=widths[1], scale_16=scale_16, offset=offset)
    assert_same(run(dec, llr, torch_dev), r, code.n, where=f"A {widths} {scale_16}/16-{offset}")
    d = dec.describe()
    assert d.startswith("flood_minsum<DC=47,addr=computed,deg=exact> grid="), d
    assert d.endswith(f" sat={widths[0]}/{widths[1]} ms={scale_16}/16-{offset} state=compressed"), d
    assert " threads=256 " in d and " grid=" in d and lds_of(d) <= lds_cap(code), d
    assert r["iters"][:24].mean() > 1
    if widths == (12, 10):
        assert r["clipped"] > 0


@pytest.mark.parametrize("table", ["global", "lds"])
def test_w(F, O, codes, torch_dev, monkeypatch, table):
    code = codes["W"][0]
    llr = awgn(F, O, code, 2.0, 16)
    monkeypatch.setenv("FPLDPC_MINSUM_TABLE", table)
    dec = F.MinSumDecoder(code, scale_16=12)
    monkeypatch.delenv("FPLDPC_MINSUM_TABLE")
    d = dec.describe()
    assert d.startswith(f"flood_minsum<DC=8,addr={'table' if table == 'lds' else 'gtable'},deg=table> grid="), d
    assert " threads=256 " in d and d.endswith(" sat=12/10 ms=12/16-0 state=compressed"), d
    assert lds_of(d) <= lds_cap(code, table == "lds"), d
    _, cdeg, _, _ = code.lists()
    assert set(cdeg) == {7, 8}
    assert_same(run(dec, llr, torch_dev), model(code, llr, (12, 10), scale_16=12), code.n, where=f"W table={table}")


def test_w_table_placement_rule(F, codes):
    """Without the switch the table is staged in LDS only where that costs no resident workgroup."""
    d = F.MinSumDecoder(codes["W"][0]).describe()
    assert re.match(r"flood_minsum<DC=8,addr=g?table,deg=table> grid=\d+ threads=256 lds=\d+ ", d), d


def test_r(F, O, codes, torch_dev):
    """R at 8 dB, 3 iterations without early termination: 1128 checks on 256 lanes, four full passes and a
    partial one per step; the state of every check in LDS, no scratch of any kind."""
    code = codes["R"][0]
    llr = awgn(F, O, code, 8.0, 4)
    ref = model(code, llr, (12, 10), max_iter=3, early_term=False)
    assert (ref["iters"] == 3).all() and ref["clipped"] > 0
    dec = F.MinSumDecoder(code, max_iter=3, early_term=False)
    d = dec.describe()
    assert d.startswith("flood_minsum<DC=47,addr=computed,deg=exact> grid="), d
    assert "global" not in d and "scratch" not in d and " threads=256 " in d and lds_of(d) <= lds_cap(code), d
    assert_same(run(dec, llr, torch_dev), ref, code.n, where="R")


@pytest.mark.parametrize("which", ["irregular", "array13x2", "array31x2", "array37x2", "array59x2"])
def test_small_codes(F, torch_dev, which):
    """An irregular code (table addressing, degrees 2..6: DC = 8) and one array code per other predicated
    width: degrees 13, 31, 37 and 59 take DC = 16, 32, 48 and 64 (the sign word's upper half from slot 32
    on); p odd makes n odd, so the int16 LLRs end on half a word.  Random +-300 LLRs with zeros among
    them, offset min-sum with a scale."""
    code, _ = small_code(F, which)
    llr = rand(30, 64, code.n, 300)
    assert (llr == 0).any()
    ref = model(code, llr, (12, 10), scale_16=14, offset=2, max_iter=8)
    dec = F.MinSumDecoder(code, max_iter=8, scale_16=14, offset=2)
    d = dec.describe()
    dc = next(x for x in (8, 16, 32, 48, 64) if code.dc_max <= x)
    assert d.startswith(f"flood_minsum<DC={dc},addr={'computed' if which != 'irregular' else 'table'},deg=table> "), d
    assert lds_of(d) <= lds_cap(code, which == "irregular"), d
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=which)
    if which == "irregular":
        _, cdeg, _, _ = code.lists()
        assert min(cdeg) == 2


def test_equals_the_shipped_flooding_decoder_at_frac_bits_0(F, O, codes, torch_dev):
    """On the device, where no clamp acts (16/15, plain min-sum; the model confirms clipped == 0): the
    flooding sxor decoder at frac_bits = 0 (C = 0: sxor is sign * min) and the oracle, output for output."""
    code, ocode = codes["A"]
    llr = awgn(F, O, code, 4.5, 24)
    ref = model(code, llr, (16, 15))
    assert ref["clipped"] == 0
    a = run(F.MinSumDecoder(code, post_bits=16, msg_bits=15), llr, torch_dev)
    b = run(F.Decoder(code, frac_bits=0), llr, torch_dev)
    for k in b:
        assert (a[k] == b[k]).all(), k
    assert_same(a, O.decode_batch(ocode, llr, 30, 0, 0xFF), code.n, where="oracle at frac_bits=0")
    assert_same(a, ref, code.n, where="model")


@pytest.mark.parametrize("precheck", [False, True])
def test_precheck(F, O, codes, precheck):
    """A passing channel syndrome returns 0 iterations with the channel decision and leaves the posteriors untouched."""
    code = codes["A"][0]
    llr = awgn(F, O, code, 8.0, 16)
    ref = model(code, llr, (12, 10), scale_16=12, precheck=precheck)
    pre = ref["prechecked"]
    assert pre.any() == precheck and not pre.all()
    sentinel = np.full(llr.shape, -123456, np.int32)
    dec = F.MinSumDecoder(code, precheck=precheck, scale_16=12)
    out = dec.decode_host(llr, post=sentinel.copy())
    assert_same(out, ref, code.n, check_post=False, where=f"precheck={precheck}")
    assert (out["iters"][pre] == 0).all() and (out["iters"][~pre] >= 1).all()
    assert (out["post"][pre] == -123456).all()
    assert (out["post"][~pre] == ref["post"][~pre]).all()


def test_max_iter_1(F, case_a, torch_dev):
    code, llr, _ = case_a
    ref = model(code, llr[:16], (12, 10), max_iter=1)
    assert_same(run(F.MinSumDecoder(code, max_iter=1), llr[:16], torch_dev), ref, code.n, where="max_iter=1")
    assert (ref["iters"] == 1).all()


def test_without_early_termination(F, case_a, torch_dev):
    code, llr, _ = case_a
    ref = model(code, llr[20:36], (12, 10), scale_16=12, max_iter=5, early_term=False)
    dec = F.MinSumDecoder(code, max_iter=5, early_term=False, scale_16=12)
    assert_same(run(dec, llr[20:36], torch_dev), ref, code.n, where="early_term=False")
    assert (ref["iters"] == 5).all() and ref["syndrome_ok"].any() and not ref["syndrome_ok"].all()


def test_int16_and_int32_llr(F, case_a, torch_dev):
    """The same frames as int16 and as int32 LLRs; then int32 LLRs beyond int16: the input clamp runs first."""
    code, llr, ref = case_a
    dec = F.MinSumDecoder(code)
    a, b = run(dec, llr, torch_dev, np.int16), run(dec, llr, torch_dev, np.int32)
    assert_same(a, ref(), code.n, where="int16")
    for k in a:
        assert (a[k] == b[k]).all(), k
    big = llr[28:36].astype(np.int64) * 4097 + np.sign(llr[28:36]) * 65536
    assert np.abs(big).max() > 2 ** 23 and np.abs(big).max() < 2 ** 31
    big = big.astype(np.int32)
    assert_same(run(dec, big, torch_dev), model(code, big, (12, 10)), code.n, where="int32 beyond S_p")


def test_more_frames_than_the_grid(F, torch_dev):
    """The resident grid plus 3 frames on a small code: workgroups pull a second frame, which starts from
    zero check state and fresh accumulators."""
    code = F.Code.array(7, 3)
    dec = F.MinSumDecoder(code, max_iter=4, scale_16=12)
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
    dec = F.MinSumDecoder(code)
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
    dec = F.MinSumDecoder(code)
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
