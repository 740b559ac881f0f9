"""The saturated flooding decoder on the GPU (fpldpc_flood_create_sat, FloodSatDecoder) against the numpy model
of its definition (tests/flood_sat_model.py): iterations, hard decisions, syndrome flags and posteriors
exactly, on every path of the kernel -- A (exact degree, computed addresses, one lane per check), W (table in
global memory and in LDS, degrees 7 and 8 in DC = 8), R (several checks per lane, a partial last pass), every
predicated width, small and irregular codes, every mode -- and, where no clamp acts, against the shipped
flooding decoder and the oracle at the same frac_bits and width_mask.  The model asserts the definition's
bounds on every run."""
import re

import numpy as np
import pytest

import flood_sat_model as FS
from conftest import assert_same
from test_gpu_layered_sat import awgn, rand, run, small_code

pytestmark = pytest.mark.gpu


def model(code, llr, widths, **kw):
    return FS.flood_sat_decode(FS.ModelCode.from_code(code), llr, *widths, **kw)


def lds_of(d):
    return int(re.search(r" lds=(\d+) ", d).group(1))


def lds_bytes(code, table=False, exact=False):
    """c2v [dc_max][m] int16 and the int16 LLRs, each up to a whole word, three int32 accumulators, 16 bytes of
    control words, the index table when it is staged and one byte per check unless every degree is the kernel's."""
    def up(x):
        return (x + 3) // 4 * 4
    edges = code.dc_max * code.m
    return up(2 * edges) + 12 * code.n + up(2 * code.n) + 16 + (2 * edges if table else 0) + (0 if exact else code.m)


@pytest.fixture(scope="module")
def case_a(F, O, codes):
    """The A frames most tests share, 24 AWGN frames at 4.5 dB and 8 frames in +-300, with their model results per
    widths, each computed once."""
    code = codes["A"][0]
    llr = np.concatenate([awgn(F, O, code, 4.5, 24), rand(5, 8, code.n, 300)])
    refs = {}

    def ref(widths=(12, 10)):
        if widths not in refs:
            refs[widths] = model(code, llr, widths)
            for v in refs[widths].values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        return refs[widths]
    return code, llr, ref


@pytest.mark.parametrize("widths", [(12, 10), (10, 8)])
def test_a(F, case_a, torch_dev, widths):
    code, llr, ref = case_a
    r = ref(widths)
    assert r["clipped"] > 0 and r["iters"][:24].mean() > 1
    dec = F.FloodSatDecoder(code, post_bits=widths[0], msg_bits=widths[1])
    assert_same(run(dec, llr, torch_dev), r, code.n, where=f"A {widths}")
    d = dec.describe()
    assert d.startswith("flood_sat<DC=47,addr=computed,deg=exact> grid="), d
    assert d.endswith(f" sat={widths[0]}/{widths[1]} state=i16"), d
    assert " threads=256 " in d and lds_of(d) == lds_bytes(code, exact=True) == 53036, d


@pytest.mark.parametrize("table", ["global", "lds"])
def test_w(F, O, codes, torch_dev, monkeypatch, table):
    code = codes["W"][0]
    llr = awgn(F, O, code, 2.0, 16)
    monkeypatch.setenv("FPLDPC_FLOOD_SAT_TABLE", table)
    dec = F.FloodSatDecoder(code)
    monkeypatch.delenv("FPLDPC_FLOOD_SAT_TABLE")
    d = dec.describe()
    assert d.startswith(f"flood_sat<DC=8,addr={'table' if table == 'lds' else 'gtable'},deg=table> grid="), d
    assert " threads=256 " in d and d.endswith(" sat=12/10 state=i16"), d
    assert lds_of(d) == lds_bytes(code, table == "lds") == (59308 if table == "lds" else 43756), d
    _, cdeg, _, _ = code.lists()
    assert set(cdeg) == {7, 8}
    ref = model(code, llr, (12, 10))
    assert ref["clipped"] > 0
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"W table={table}")


def test_w_table_placement_rule(F, codes):
    """Without the switch the table is staged in LDS only where that costs no resident workgroup."""
    d = F.FloodSatDecoder(codes["W"][0]).describe()
    assert re.match(r"flood_sat<DC=8,addr=g?table,deg=table> grid=\d+ threads=256 lds=\d+ device=\d+ sat=12/10 state=i16$", d), d
    assert lds_of(d) == lds_bytes(codes["W"][0], "addr=table" in d), d


def test_r(F, O, codes, torch_dev):
    """R at 6.5 dB, mask 0x3f, 10 iterations: 1128 checks on 256 lanes, four full passes and a partial one per step."""
    code = codes["R"][0]
    llr = awgn(F, O, code, 6.5, 8)
    ref = model(code, llr, (12, 10), max_iter=10, mask=0x3F)
    assert ref["clipped"] > 0 and (ref["iters"] > 1).any()
    dec = F.FloodSatDecoder(code, max_iter=10, width_mask=0x3F)
    d = dec.describe()
    assert d.startswith("flood_sat<DC=47,addr=computed,deg=exact> grid="), d
    assert " threads=256 " in d and lds_of(d) == lds_bytes(code, exact=True) == 136976 and d.endswith(" sat=12/10 state=i16"), d
    assert_same(run(dec, llr, torch_dev), ref, code.n, where="R")


@pytest.mark.parametrize("which", ["irregular", "array13x2", "array31x2", "array37x2", "array59x2"])
def test_small_codes(F, torch_dev, which):
    """An irregular code (table addressing, degrees 2..6: DC = 8) and one array code per other predicated
    width: degrees 13, 31, 37 and 59 take DC = 16, 32, 48 and 64; p odd makes n and the edge count odd, so c2v
    and the int16 LLRs end on half a word.  Random +-300 LLRs with zeros among them."""
    code, _ = small_code(F, which)
    llr = rand(30, 64, code.n, 300)
    assert (llr == 0).any()
    ref = model(code, llr, (12, 10), max_iter=8)
    dec = F.FloodSatDecoder(code, max_iter=8)
    d = dec.describe()
    dc = next(x for x in (8, 16, 32, 48, 64) if code.dc_max <= x)
    assert d.startswith(f"flood_sat<DC={dc},addr={'computed' if which != 'irregular' else 'table'},deg=table> "), d
    assert lds_of(d) == lds_bytes(code, which == "irregular"), d
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=which)
    if which == "irregular":
        _, cdeg, _, _ = code.lists()
        assert min(cdeg) == 2


@pytest.mark.parametrize("name,eb,frac,mask", [("A", 4.5, 4, 0xFF), ("W", 2.0, 4, 0xFF), ("A", 4.5, 2, 0x3F)])
def test_identity_at_16_15(F, O, codes, torch_dev, name, eb, frac, mask):
    """On the device, where no clamp acts (16/15; the model confirms clipped == 0): the shipped flooding decoder and
    the oracle at the same frac_bits and width_mask, output for output."""
    code, ocode = codes[name]
    llr = awgn(F, O, code, eb, 24 if name == "A" else 16, frac=frac)
    ref = model(code, llr, (16, 15), frac_bits=frac, mask=mask)
    assert ref["clipped"] == 0 and (ref["iters"] > 1).any()
    a = run(F.FloodSatDecoder(code, frac_bits=frac, width_mask=mask, post_bits=16, msg_bits=15), llr, torch_dev)
    b = run(F.Decoder(code, frac_bits=frac, width_mask=mask), llr, torch_dev)
    for k in b:
        assert (a[k] == b[k]).all(), k
    assert_same(a, O.decode_batch(ocode, llr, 30, frac, mask), code.n, where="oracle")
    assert_same(a, ref, code.n, where="model")


@pytest.mark.parametrize("precheck", [False, True])
def test_precheck(F, O, codes, precheck):
    """A passing channel syndrome returns 0 iterations with the channel decision and leaves the posteriors untouched."""
    code = codes["A"][0]
    llr = awgn(F, O, code, 8.0, 16)
    ref = model(code, llr, (12, 10), precheck=precheck)
    pre = ref["prechecked"]
    assert pre.any() == precheck and not pre.all()
    sentinel = np.full(llr.shape, -123456, np.int32)
    dec = F.FloodSatDecoder(code, precheck=precheck)
    out = dec.decode_host(llr, post=sentinel.copy())
    assert_same(out, ref, code.n, check_post=False, where=f"precheck={precheck}")
    assert (out["iters"][pre] == 0).all() and (out["iters"][~pre] >= 1).all()
    assert (out["post"][pre] == -123456).all()
    assert (out["post"][~pre] == ref["post"][~pre]).all()


def test_max_iter_1(F, case_a, torch_dev):
    code, llr, _ = case_a
    ref = model(code, llr[:16], (12, 10), max_iter=1)
    assert_same(run(F.FloodSatDecoder(code, max_iter=1), llr[:16], torch_dev), ref, code.n, where="max_iter=1")
    assert (ref["iters"] == 1).all()


def test_without_early_termination(F, case_a, torch_dev):
    code, llr, _ = case_a
    ref = model(code, llr[16:32], (12, 10), max_iter=5, early_term=False)
    dec = F.FloodSatDecoder(code, max_iter=5, early_term=False)
    assert_same(run(dec, llr[16:32], torch_dev), ref, code.n, where="early_term=False")
    assert (ref["iters"] == 5).all() and ref["syndrome_ok"].any() and not ref["syndrome_ok"].all()


def test_int16_and_int32_llr(F, case_a, torch_dev):
    """The same frames as int16 and as int32 LLRs; then int32 LLRs beyond int16: the input clamp runs first."""
    code, llr, ref = case_a
    dec = F.FloodSatDecoder(code)
    a, b = run(dec, llr, torch_dev, np.int16), run(dec, llr, torch_dev, np.int32)
    assert_same(a, ref(), code.n, where="int16")
    for k in a:
        assert (a[k] == b[k]).all(), k
    big = llr[20:28].astype(np.int64) * 40961 + np.sign(llr[20:28]) * 65536
    assert np.abs(big).max() > 2 ** 23 and np.abs(big).max() < 2 ** 31
    big = big.astype(np.int32)
    assert_same(run(dec, big, torch_dev), model(code, big, (12, 10)), code.n, where="int32 beyond S_p")


def test_more_frames_than_the_grid(F, torch_dev):
    """The resident grid plus 3 frames on a small code: workgroups pull a second frame, whose first step must read
    every c2v as 0 over the previous frame's column, from fresh accumulators."""
    code = F.Code.array(7, 3)
    dec = F.FloodSatDecoder(code, max_iter=4)
    grid = int(dec.describe().split("grid=")[1].split()[0])
    assert 0 < grid < 100000
    llr = rand(31, 64, code.n, 3000)
    ref = model(code, llr, (12, 10), max_iter=4)
    sel = np.tile(np.arange(64), -(-(grid + 3) // 64))[:grid + 3]
    big = {k: ref[k][sel] for k in ("iters", "hard", "syndrome_ok", "post")}
    assert_same(run(dec, llr[sel], torch_dev), big, code.n, where=f"batch {grid + 3}")


def test_two_calls_on_a_stream(F, case_a, torch_dev):
    import torch
    code, llr, ref = case_a
    dec = F.FloodSatDecoder(code)
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
    dec = F.FloodSatDecoder(code)
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


@pytest.mark.parametrize("p,r,text", [(67, 2, "check degree above 64"), (61, 30, "do not fit 160 KiB")])
def test_envelope(F, p, r, text):
    """Degree 67, and degree 61 on 1830 checks, whose c2v alone is 223 KB: FPLDPC_ERR_UNSUPPORTED, the message
    naming the decoder and the reason."""
    with pytest.raises(F.FpldpcError) as e:
        F.FloodSatDecoder(F.Code.array(p, r))
    assert e.value.code == -4, e.value
    assert "saturated flooding decoder:" in str(e.value) and text in str(e.value), e.value
