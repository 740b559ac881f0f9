"""The global form of the saturated flooding decoder (fpldpc_flood_sat_global.hip, FloodSatDecoder(state="global" |
"auto"): the int16 c2v of every edge and the three int32 accumulators in a per-workgroup slice of global memory)
against the numpy model of the definition (tests/flood_sat_model.py): iterations, hard decisions, syndrome flags
and posteriors exactly, and against the LDS form wherever the code has one.
  * Codes whose state does not fit 160 KiB of LDS: long_alist(1123) (146 q + 16 B in the LDS form: the first prime
    outside), Code.array(61, 30) (degree 61 in DC = 64, c2v alone 223 KB) and long_alist(8191), the longest the
    loader takes; long_alist(1117), the last inside, keeps the LDS form under "auto".  Several iterations per
    frame: every accumulator is read again one step after atomics changed it.  The properties the docstrings
    state (iteration counts, failures, whether a clamp acts) are asserted on the model's result.
  * state="global" on codes that fit: every instantiation (exact 47 and the predicated 8 / 16 / 32 / 48 / 64),
    equal to the model and to the LDS form.
  * The frame framework of the global form, forced on small codes: a slice's second frame (the scratch is never
    cleared: step 1 masks the column it reads), precheck, modes, LLR types, counters, streams.
Not covered here, as in tests/test_gpu_minsum_long.py: the degree table read from global memory, which needs
2 n + 16 + m > 160 KiB."""
import re

import numpy as np
import pytest

from conftest import assert_same
from test_gpu_flood_sat import case_a, model  # noqa: F401  (case_a: the A frames of the LDS form's tests)
from test_gpu_layered_sat import awgn, long_alist, rand, run, small_code

pytestmark = pytest.mark.gpu

KEYS = ("iters", "hard", "syndrome_ok", "post")


def noisy(n, frames, sigma):
    """As tests/test_gpu_minsum_long.py's."""
    return np.rint(np.random.default_rng(5).normal(60, sigma, (frames, n))).astype(np.int32)


def up(x, to=4):
    return -(-x // to) * to


def slice_bytes(code):
    """A workgroup's slice of the scratch: c2v [dc_max][m] int16 up to a whole word | acc [3][n] int32, to 256 B."""
    return up(up(2 * code.dc_max * code.m) + 12 * code.n, 256)


def lds_bytes(code, exact=False):
    """The int16 LLRs up to a whole word, 16 bytes of control words, one byte per check unless every degree is DC."""
    return up(2 * code.n) + 16 + (0 if exact else code.m)


def fields(d):
    return {k: int(v) for k, v in re.findall(r" (grid|threads|lds|scratch)=(\d+)", d)}


def check_global_describe(d, code, dc=8, deg="table", widths=(12, 10)):
    assert d.startswith(f"flood_sat<DC={dc},addr=gtable,deg={deg},mem=global> grid="), d
    f = fields(d)
    assert 0 < f["grid"] < 100000, d
    assert d.endswith(f" sat={widths[0]}/{widths[1]} state=i16 scratch={f['grid'] * slice_bytes(code)}"), d
    assert f["lds"] == lds_bytes(code, deg == "exact"), d
    assert re.fullmatch(r"\S+ grid=\d+ threads=\d+ lds=\d+ device=\d+ sat=\d+/\d+ state=i16 scratch=\d+", d), d
    return f


def is_lds_form(d):
    return "mem=global" not in d and "scratch=" not in d


def same_outputs(a, b):
    for k in KEYS:
        assert (a[k] == b[k]).all(), k


def parts(code, blocks, widths, **kw):
    """The model on each block of frames (its `clipped` is per run), and the results joined."""
    rs = [model(code, b, widths, **kw) for b in blocks]
    return rs, {k: np.concatenate([r[k] for r in rs]) for k in KEYS}


@pytest.fixture(scope="module")
def long_code(F):
    made = {}

    def get(q):
        if q not in made:
            assert all(q % d for d in range(2, int(q ** 0.5) + 1))
            made[q] = F.Code.parse(long_alist(q))
            assert (made[q].n, made[q].m, made[q].dc_max) == (8 * q, 2 * q, 8)
        return made[q]
    return get


def test_just_outside_lds(F, long_code, torch_dev):
    """q = 1123: 146 q + 16 = 163,974 B > 163,840, state="auto".  12 noisy frames (the model: 5 to 12 iterations, one
    fails, no clamp acts at 12/10) and 4 random ones far beyond S_p (12 iterations, none passes); the same at 10/8,
    where the clamps act on the noisy frames too."""
    q = 1123
    code = long_code(q)
    assert 146 * q + 16 > 160 * 1024 >= 146 * 1117 + 16
    blocks = [noisy(code.n, 12, 30), rand(32, 4, code.n, 3000)]
    llr = np.concatenate(blocks)
    (rn, rr), ref = parts(code, blocks, (12, 10), max_iter=12)
    assert list(rn["iters"]) == [12, 9, 5, 6, 9, 6, 6, 9, 7, 5, 8, 7]
    assert (rn["syndrome_ok"] == 0).sum() == 1 and rn["clipped"] == 0
    assert (rr["iters"] == 12).all() and not rr["syndrome_ok"].any() and rr["clipped"] > 4 * code.n
    with pytest.raises(F.FpldpcError) as e:
        F.FloodSatDecoder(code, max_iter=12)
    assert e.value.code == -4 and "163974 bytes" in str(e.value) and "do not fit 160 KiB" in str(e.value), e.value
    dec = F.FloodSatDecoder(code, max_iter=12, state="auto")
    d = dec.describe()
    f = check_global_describe(d, code)
    assert f["threads"] == 256 and f["lds"] == 20230 and slice_bytes(code) == 143872, d
    assert d == F.FloodSatDecoder(code, max_iter=12, state="global").describe()
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"q={q}")

    (rn8, _), ref8 = parts(code, blocks, (10, 8), max_iter=12)
    assert (rn8["iters"] == rn["iters"]).all() and rn8["clipped"] > 0
    dec = F.FloodSatDecoder(code, max_iter=12, post_bits=10, msg_bits=8, state="auto")
    check_global_describe(dec.describe(), code, widths=(10, 8))
    assert_same(run(dec, llr, torch_dev), ref8, code.n, where=f"q={q} at 10/8")


def test_last_code_inside_lds_keeps_the_lds_form(F, long_code, torch_dev):
    q = 1117
    code = long_code(q)
    llr = noisy(code.n, 4, 28)
    ref = model(code, llr, (12, 10), max_iter=8)
    assert list(ref["iters"]) == [6, 5, 4, 5] and ref["syndrome_ok"].all()
    dec = F.FloodSatDecoder(code, max_iter=8, state="auto")
    d = dec.describe()
    assert is_lds_form(d) and d.startswith("flood_sat<DC=8,addr=gtable,deg=table> grid="), d
    assert d == F.FloodSatDecoder(code, max_iter=8, state="lds").describe() == F.FloodSatDecoder(code, max_iter=8).describe()
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"q={q}")


@pytest.mark.parametrize("widths", [(12, 10), (10, 8)])
def test_high_degree_outside_lds(F, torch_dev, widths):
    """Code.array(61, 30): DC = 64 predicated at degree 61, 1,830 checks on 256 lanes with a partial last pass,
    c2v alone 223 KB.  8 frames at sigma 24 (the model: 4 to 9 iterations, all pass), 8 at sigma 25 (seven reach 10,
    six fail), 3 random ones beyond S_p.  No clamp acts on the noisy frames at 12/10; at 10/8 the clamps do."""
    code = F.Code.array(61, 30)
    assert (code.n, code.m, code.dc_max) == (3721, 1830, 61)
    blocks = [noisy(code.n, 8, 24), noisy(code.n, 8, 25), rand(32, 3, code.n, 3000)]
    llr = np.concatenate(blocks)
    (r24, r25, rr), ref = parts(code, blocks, widths, max_iter=10)
    assert list(r24["iters"]) == [5, 6, 5, 9, 7, 5, 9, 4] and r24["syndrome_ok"].all()
    assert (r25["iters"] == 10).sum() == 7 and (r25["syndrome_ok"] == 0).sum() == 6
    assert (r24["clipped"] > 0) == (r25["clipped"] > 0) == (widths == (10, 8)) and rr["clipped"] > 0
    for state in ("lds", None):
        with pytest.raises(F.FpldpcError) as e:
            F.FloodSatDecoder(code, max_iter=10, **({"state": state} if state else {}))
        assert e.value.code == -4 and "saturated flooding decoder:" in str(e.value) and "do not fit 160 KiB" in str(e.value), e.value
    for state in ("global", "auto"):
        dec = F.FloodSatDecoder(code, max_iter=10, post_bits=widths[0], msg_bits=widths[1], state=state)
        f = check_global_describe(dec.describe(), code, dc=64, widths=widths)
        assert f["threads"] == 256 and f["lds"] == 9290 and slice_bytes(code) == 268032, dec.describe()
        assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"array(61, 30) {state} {widths}")


def test_longest_code(F, long_code, torch_dev):
    """q = 8191: n = 65528, the longest code of this shape the loader takes; 131,056 B of int16 LLRs in LDS, the
    degree table beside them, a slice of 1 MiB."""
    q = 8191
    code = long_code(q)
    llr = noisy(code.n, 3, 28)
    ref = model(code, llr, (12, 10), max_iter=6)
    assert list(ref["iters"]) == [6, 6, 5] and (ref["syndrome_ok"] == 0).sum() == 1
    dec = F.FloodSatDecoder(code, max_iter=6, state="auto")
    f = check_global_describe(dec.describe(), code)
    assert f["threads"] == 256 and f["lds"] == 147454 and slice_bytes(code) == 1048576, dec.describe()
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"q={q}")


def forced_and_not(F, code, **kw):
    forced, plain = F.FloodSatDecoder(code, state="global", **kw), F.FloodSatDecoder(code, **kw)
    assert is_lds_form(plain.describe()), plain.describe()
    assert plain.describe() == F.FloodSatDecoder(code, state="auto", **kw).describe()
    return forced, plain


@pytest.mark.parametrize("widths", [(12, 10), (10, 8)])
def test_forced_on_a(F, case_a, torch_dev, widths):  # noqa: F811
    """A forced: the exact degree 47, now through the index table."""
    code, llr, ref = case_a
    r = ref(widths)
    assert r["clipped"] > 0 and r["iters"][:24].mean() > 1
    forced, plain = forced_and_not(F, code, post_bits=widths[0], msg_bits=widths[1])
    f = check_global_describe(forced.describe(), code, dc=47, deg="exact", widths=widths)
    assert f["threads"] == 256 and f["lds"] == 4436 and slice_bytes(code) == 48640, forced.describe()
    assert plain.describe().startswith("flood_sat<DC=47,addr=computed,deg=exact> ")
    out = run(forced, llr, torch_dev)
    assert_same(out, r, code.n, where=f"A forced {widths}")
    same_outputs(out, run(plain, llr, torch_dev))


def test_forced_on_w(F, O, codes, torch_dev):
    code = codes["W"][0]
    llr = awgn(F, O, code, 2.0, 16)
    ref = model(code, llr, (12, 10))
    assert ref["clipped"] > 0
    forced, plain = forced_and_not(F, code)
    f = check_global_describe(forced.describe(), code)
    assert f["threads"] == 256 and f["lds"] == 4876 and slice_bytes(code) == 38912, forced.describe()
    _, cdeg, _, _ = code.lists()
    assert set(cdeg) == {7, 8}
    out = run(forced, llr, torch_dev)
    assert_same(out, ref, code.n, where="W forced")
    same_outputs(out, run(plain, llr, torch_dev))


def test_forced_on_r(F, O, codes, torch_dev):
    """R at 6.5 dB, mask 0x3f, 10 iterations: 1128 checks on 256 lanes, four full passes and a partial one per step."""
    code = codes["R"][0]
    llr = awgn(F, O, code, 6.5, 8)
    ref = model(code, llr, (12, 10), max_iter=10, mask=0x3F)
    assert ref["clipped"] > 0 and (ref["iters"] > 1).any()
    forced, plain = forced_and_not(F, code, max_iter=10, width_mask=0x3F)
    check_global_describe(forced.describe(), code, dc=47, deg="exact")
    out = run(forced, llr, torch_dev)
    assert_same(out, ref, code.n, where="R forced")
    same_outputs(out, run(plain, llr, torch_dev))


@pytest.mark.parametrize("which", ["irregular", "array13x2", "array31x2", "array37x2", "array59x2"])
def test_forced_on_small_codes(F, torch_dev, which):
    """DC = 8 / 16 / 32 / 48 / 64 and odd edge counts (c2v ends on half a word); the array codes' computed addressing
    is turned off and the table built.  Random +-300 LLRs with zeros among them."""
    code, _ = small_code(F, which)
    llr = rand(30, 64, code.n, 300)
    assert (llr == 0).any()
    ref = model(code, llr, (12, 10), max_iter=8)
    forced, plain = forced_and_not(F, code, max_iter=8)
    dc = next(x for x in (8, 16, 32, 48, 64) if code.dc_max <= x)
    check_global_describe(forced.describe(), code, dc=dc)
    out = run(forced, llr, torch_dev)
    assert_same(out, ref, code.n, where=f"{which} forced")
    same_outputs(out, run(plain, llr, torch_dev))


def test_more_frames_than_the_grid(F, torch_dev):
    """The resident grid plus 3 frames: a slice's second frame starts from a column full of the previous frame's
    messages (LLRs +-3000: every message is large), which step 1 must read as 0, and from fresh accumulators."""
    code = F.Code.array(7, 3)
    dec = F.FloodSatDecoder(code, max_iter=4, state="global")
    grid = check_global_describe(dec.describe(), code)["grid"]
    llr = rand(31, 64, code.n, 3000)
    ref = model(code, llr, (12, 10), max_iter=4)
    assert ref["clipped"] > 0
    sel = np.tile(np.arange(64), -(-(grid + 3) // 64))[:grid + 3]
    big = {k: ref[k][sel] for k in KEYS}
    assert_same(run(dec, llr[sel], torch_dev), big, code.n, where=f"batch {grid + 3}")


@pytest.mark.parametrize("precheck", [False, True])
def test_precheck(F, O, codes, precheck):
    code = codes["A"][0]
    llr = awgn(F, O, code, 8.0, 16)
    ref = model(code, llr, (12, 10), precheck=precheck)
    pre = ref["prechecked"]
    assert pre.any() == precheck and not pre.all()
    sentinel = np.full(llr.shape, -123456, np.int32)
    dec = F.FloodSatDecoder(code, precheck=precheck, state="global")
    assert "mem=global" in dec.describe()
    out = dec.decode_host(llr, post=sentinel.copy())
    assert_same(out, ref, code.n, check_post=False, where=f"precheck={precheck}")
    assert (out["iters"][pre] == 0).all() and (out["iters"][~pre] >= 1).all()
    assert (out["post"][pre] == -123456).all()
    assert (out["post"][~pre] == ref["post"][~pre]).all()


def test_without_early_termination_and_max_iter_1(F, case_a, torch_dev):  # noqa: F811
    code, llr, _ = case_a
    ref = model(code, llr[16:32], (12, 10), max_iter=5, early_term=False)
    assert (ref["iters"] == 5).all() and ref["syndrome_ok"].any() and not ref["syndrome_ok"].all()
    dec = F.FloodSatDecoder(code, max_iter=5, early_term=False, state="global")
    assert_same(run(dec, llr[16:32], torch_dev), ref, code.n, where="early_term=False")
    ref = model(code, llr[:16], (12, 10), max_iter=1)
    assert (ref["iters"] == 1).all()
    dec = F.FloodSatDecoder(code, max_iter=1, state="global")
    assert_same(run(dec, llr[:16], torch_dev), ref, code.n, where="max_iter=1")


def test_int16_and_int32_llr_and_a_batch_of_1(F, case_a, torch_dev):  # noqa: F811
    """The same frames as int16 and as int32 LLRs; int32 LLRs beyond int16: the input clamp runs first; one frame."""
    code, llr, ref = case_a
    dec = F.FloodSatDecoder(code, state="global")
    a, b = run(dec, llr, torch_dev, np.int16), run(dec, llr, torch_dev, np.int32)
    assert_same(a, ref(), code.n, where="int16")
    same_outputs(a, b)
    big = llr[20:28].astype(np.int64) * 40961 + np.sign(llr[20:28]) * 65536
    assert np.abs(big).max() > 2 ** 23 and np.abs(big).max() < 2 ** 31
    big = big.astype(np.int32)
    assert_same(run(dec, big, torch_dev), model(code, big, (12, 10)), code.n, where="int32 beyond S_p")
    one = {k: ref()[k][5:6] for k in KEYS}
    assert one["iters"][0] > 1
    assert_same(run(dec, llr[5:6], torch_dev), one, code.n, where="batch 1")


def test_counters_streams_and_two_decoders(F, case_a, torch_dev):  # noqa: F811
    """bit_errors and totals over two calls, two calls on one stream, and a global and an LDS decoder of the same
    code alive at once, decoding in turn."""
    import torch
    code, llr, ref = case_a
    r = ref()
    idx = np.arange(0, code.n, 3, dtype=np.int32)
    bits = (np.arange(len(idx)) % 5 == 0).astype(np.uint8)
    want = (r["hard"][:, idx] != bits).sum(axis=1)
    dec, plain = forced_and_not(F, code)
    assert "mem=global" in dec.describe()
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

    t = torch.from_numpy(llr).to(torch_dev)
    s = torch.cuda.Stream(torch_dev)
    torch.cuda.synchronize()
    outs = [dec.decode_torch(t, post=True, stream=s), plain.decode_torch(t, post=True, stream=s),
            dec.decode_torch(t, post=True, stream=s)]
    s.synchronize()
    for o in outs:
        assert_same({k: v.cpu().numpy() for k, v in o.items()}, r, code.n, where="stream")


def test_identity_at_16_15(F, O, codes, torch_dev):
    """Where no clamp acts (16/15; the model confirms clipped == 0) the global form is the shipped flooding decoder
    and the oracle at the same frac_bits and width_mask, output for output."""
    code, ocode = codes["A"]
    llr = awgn(F, O, code, 4.5, 24, frac=4)
    ref = model(code, llr, (16, 15), frac_bits=4, mask=0xFF)
    assert ref["clipped"] == 0 and (ref["iters"] > 1).any()
    dec = F.FloodSatDecoder(code, frac_bits=4, width_mask=0xFF, post_bits=16, msg_bits=15, state="global")
    check_global_describe(dec.describe(), code, dc=47, deg="exact", widths=(16, 15))
    a = run(dec, llr, torch_dev)
    b = run(F.Decoder(code, frac_bits=4, width_mask=0xFF), llr, torch_dev)
    for k in b:
        assert (a[k] == b[k]).all(), k
    assert_same(a, O.decode_batch(ocode, llr, 30, 4, 0xFF), code.n, where="oracle")
    assert_same(a, ref, code.n, where="model")


@pytest.mark.parametrize("state", ["global", "auto"])
def test_envelope(F, state):
    """Degree 67 is outside every placement."""
    with pytest.raises(F.FpldpcError) as e:
        F.FloodSatDecoder(F.Code.array(67, 2), state=state)
    assert e.value.code == -4, e.value
    assert "saturated flooding decoder:" in str(e.value) and "check degree above 64" in str(e.value), e.value
