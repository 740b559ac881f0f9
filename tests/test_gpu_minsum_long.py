"""The global form of the two min-sum decoders (fpldpc_minsum_global.hip: the 16-byte check state, and the
flooding decoder's accumulators, in a per-workgroup slice of global memory) against the numpy models of
their definitions (tests/minsum_model.py, tests/layered_minsum_model.py): iterations, hard decisions,
syndrome flags and posteriors exactly.
  * Codes whose state does not fit 160 KiB of LDS -- long_alist(q): n = 8q, m = 2q, every check of degree 8,
    146 q + 16 B of LDS in the flooding LDS form and 50 q + 16 B in the layered one -- at the first prime
    outside each envelope (q = 1123, q = 3299), at the last inside (q = 1117, q = 3271: still the LDS form)
    and at the longest the loader takes (q = 8191, n = 65528).  Several iterations per frame: every
    accumulator is read again one step after atomics changed it.
  * The switches FPLDPC_MINSUM_STATE / FPLDPC_LAYERED_MINSUM_STATE = global on codes that fit: every
    instantiation (exact 47 and the predicated 8 / 16 / 32 / 48 / 64), equal to the model and to the LDS form.
  * The frame framework of the global form, forced on small codes.
Not covered here: the degree table read from global memory, which needs 2 n + 16 + m > 160 KiB (the
smallest code of this family is n = 59,588, m = 44,691, which takes the loader minutes to parse); every
code below stages its degrees in LDS.  tests/test_gpu_degree_edges.py, which runs every check degree at the
edges of the kernels' DC buckets in every other form, leaves that one form out for the same reason: it
exists only for codes of that length."""
import re

import numpy as np
import pytest

import layered_minsum_model as MS
import layered_model as M
import minsum_model as FM
from conftest import assert_same
from test_gpu_layered_sat import awgn, long_alist, rand, run, small_code

pytestmark = pytest.mark.gpu

KINDS = ("flood", "layered")
SWITCH = {"flood": "FPLDPC_MINSUM_STATE", "layered": "FPLDPC_LAYERED_MINSUM_STATE"}
KERNEL = {"flood": "flood_minsum", "layered": "layered_minsum"}
KEYS = ("iters", "hard", "syndrome_ok", "post")


def roundup(x, to=256):
    return -(-x // to) * to


def slice_bytes(kind, code):
    """A workgroup's slice of the scratch: state [m] uint4 (| acc [3][n] int32: flooding), to 256 B."""
    return roundup(16 * code.m + (12 * code.n if kind == "flood" else 0))


def model(kind, code, llr, L=0, widths=(12, 10), **kw):
    if kind == "flood":
        return FM.minsum_decode(FM.ModelCode.from_code(code), llr, *widths, **kw)
    return MS.layered_minsum_decode(M.ModelCode.from_code(code), llr, L or code.layering()[0], *widths, **kw)


def create(F, kind, code, L=0, monkeypatch=None, **kw):
    """The decoder of `kind`; with monkeypatch, under its switch (set around creation only)."""
    if monkeypatch:
        monkeypatch.setenv(SWITCH[kind], "global")
    try:
        if kind == "flood":
            return F.MinSumDecoder(code, **kw)
        return F.LayeredDecoder(code, check="minsum", layer_checks=L, **{"post_bits": 12, "msg_bits": 10, **kw})
    finally:
        if monkeypatch:
            monkeypatch.delenv(SWITCH[kind])


def fields(d):
    return {k: int(v) for k, v in re.findall(r" (grid|threads|lds|scratch)=(\d+)", d)}


def check_global_describe(d, kind, code, dc=8, deg="table"):
    """The kernel's name, scratch = grid * slice at the end, and LDS: the int16 vector, control words, degrees."""
    assert d.startswith(f"{KERNEL[kind]}<DC={dc},addr=gtable,deg={deg},mem=global> " + ("grid=" if kind == "flood" else "L=")), d
    f = fields(d)
    assert 0 < f["grid"] < 100000, d
    assert d.endswith(f" state=compressed scratch={f['grid'] * slice_bytes(kind, code)}"), d
    assert f["lds"] <= 2 * code.n + code.m + 64, d
    return f


def is_lds_form(d):
    return "mem=global" not in d and "scratch=" not in d


def same_outputs(a, b):
    for k in KEYS:
        assert (a[k] == b[k]).all(), k


def noisy(n, frames, sigma):
    return np.rint(np.random.default_rng(5).normal(60, sigma, (frames, n))).astype(np.int32)


@pytest.fixture(scope="module")
def long_code(F):
    made = {}

    def get(q):
        if q not in made:
            assert all(q % d for d in range(2, int(q ** 0.5) + 1))
            made[q] = F.Code.parse(long_alist(q))
            assert (made[q].n, made[q].m, made[q].dc_max) == (8 * q, 2 * q, 8) and made[q].layering(q) == (q, 2)
        return made[q]
    return get


def test_flooding_just_outside_lds(F, long_code, torch_dev):
    """q = 1123: 146 q + 16 = 163,974 B > 163,840.  12 noisy frames (the model: 5 to 12 iterations, some
    fail) and 4 random ones far beyond S_p."""
    q = 1123
    code = long_code(q)
    assert 146 * q + 16 > 160 * 1024 >= 146 * 1117 + 16
    llr = np.concatenate([noisy(code.n, 12, 30), rand(32, 4, code.n, 3000)])
    ref = model("flood", code, llr, scale_16=12, max_iter=12)
    it, ok = ref["iters"][:12], ref["syndrome_ok"][:12]
    assert 1 < it.min() < it.max() == 12 and ok.any() and not ok.all() and ref["clipped"] > 0
    dec = create(F, "flood", code, scale_16=12, max_iter=12)
    d = dec.describe()
    f = check_global_describe(d, "flood", code)
    assert f["threads"] == 256 and " sat=12/10 ms=12/16-0 state=compressed scratch=" in d, d
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"flooding q={q}")
    ref = model("flood", code, llr, widths=(10, 8), scale_16=13, offset=3, max_iter=12)
    dec = create(F, "flood", code, post_bits=10, msg_bits=8, scale_16=13, offset=3, max_iter=12)
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"flooding q={q} at 10/8, 13/16-3")


def test_layered_just_outside_lds(F, long_code, torch_dev):
    """q = 3299, layers of q checks: 50 q + 16 = 164,966 B > 163,840.  8 noisy frames (the model: 2 to 4
    iterations, all pass) and 3 random ones far beyond S_p (12 iterations, none passes)."""
    q = 3299
    code = long_code(q)
    assert 50 * q + 16 > 160 * 1024 >= 50 * 3271 + 16
    llr = np.concatenate([noisy(code.n, 8, 28), rand(32, 3, code.n, 3000)])
    ref = model("layered", code, llr, q, max_iter=12)
    it, ok = ref["iters"], ref["syndrome_ok"]
    assert 1 < it[:8].min() < it[:8].max() < it.max() == 12 and ok[:8].all() and not ok[8:].any() and ref["clipped"] > 0
    dec = create(F, "layered", code, q, max_iter=12)
    d = dec.describe()
    f = check_global_describe(d, "layered", code)
    assert f["threads"] == 256 and f" L={q} layers=2 " in d and " sat=12/10 ms=16/16-0 state=compressed scratch=" in d, d
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"layered q={q}")


@pytest.mark.parametrize("kind", KINDS)
def test_longest_code(F, long_code, torch_dev, kind):
    """q = 8191: n = 65528, the longest code of this shape the loader takes; 131,056 B of int16 in LDS, the
    degree table beside them, a slice of 1 MiB (flooding) / 256 KiB (layered)."""
    q = 8191
    code = long_code(q)
    llr = noisy(code.n, 3, 25)
    ref = model(kind, code, llr, q, max_iter=6)
    assert ref["iters"].min() > 1 and ref["syndrome_ok"].all()
    dec = create(F, kind, code, q, max_iter=6)
    f = check_global_describe(dec.describe(), kind, code)
    assert f["threads"] == 256 and f["lds"] >= 2 * code.n
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"{kind} q={q}")


@pytest.mark.parametrize("kind,q", [("flood", 1117), ("layered", 3271)])
def test_last_code_inside_lds_keeps_the_lds_form(F, long_code, torch_dev, kind, q):
    code = long_code(q)
    llr = noisy(code.n, 4, 28)
    ref = model(kind, code, llr, q, max_iter=8)
    dec = create(F, kind, code, q, max_iter=8)
    d = dec.describe()
    assert is_lds_form(d) and d.startswith(f"{KERNEL[kind]}<DC=8,addr=gtable,deg=table> "), d
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"{kind} q={q}")


@pytest.fixture(scope="module")
def case_a(F, O, codes):
    """The A frames of the existing min-sum tests."""
    code = codes["A"][0]
    llr = np.concatenate([awgn(F, O, code, 4.5, 24), awgn(F, O, code, 8.0, 8), rand(1, 8, code.n, 32768),
                          rand(3, 4, code.n, 3)])
    assert (llr[-4:] == 0).any() and np.abs(llr[32:40]).max() > 32000 and np.abs(llr).max() < 32768
    return code, llr


def forced_and_not(F, kind, code, L, monkeypatch, **kw):
    forced, plain = create(F, kind, code, L, monkeypatch, **kw), create(F, kind, code, L, **kw)
    assert is_lds_form(plain.describe()), plain.describe()
    return forced, plain


@pytest.mark.parametrize("kind", KINDS)
def test_switch_on_a(F, case_a, torch_dev, monkeypatch, kind):
    """A forced: the exact degree 47, now through the index table."""
    code, llr = case_a
    ref = model(kind, code, llr, scale_16=13, offset=3)
    forced, plain = forced_and_not(F, kind, code, 0, monkeypatch, scale_16=13, offset=3)
    f = check_global_describe(forced.describe(), kind, code, dc=47, deg="exact")
    assert f["threads"] == (256 if kind == "flood" else 64), forced.describe()
    assert plain.describe().startswith(f"{KERNEL[kind]}<DC=47,addr=computed,deg=exact> ")
    out = run(forced, llr, torch_dev)
    assert_same(out, ref, code.n, where=f"{kind} A forced")
    same_outputs(out, run(plain, llr, torch_dev))
    assert ref["iters"][:24].mean() > 1 and ref["clipped"] > 0


@pytest.mark.parametrize("kind", KINDS)
def test_switch_on_w(F, O, codes, torch_dev, monkeypatch, kind):
    code = codes["W"][0]
    llr = awgn(F, O, code, 2.0, 16)
    ref = model(kind, code, llr, scale_16=12)
    forced, plain = forced_and_not(F, kind, code, 0, monkeypatch, scale_16=12)
    f = check_global_describe(forced.describe(), kind, code)
    assert f["threads"] == (256 if kind == "flood" else 128), forced.describe()
    _, cdeg, _, _ = code.lists()
    assert set(cdeg) == {7, 8}
    out = run(forced, llr, torch_dev)
    assert_same(out, ref, code.n, where=f"{kind} W forced")
    same_outputs(out, run(plain, llr, torch_dev))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["irregular", "array13x2", "array31x2", "array37x2", "array59x2"])
def test_switch_on_small_codes(F, torch_dev, monkeypatch, which, kind):
    """DC = 8 / 16 / 32 / 48 / 64; the array codes' computed addressing is turned off and the table built."""
    code, L = small_code(F, which)
    llr = rand(30, 64, code.n, 300)
    assert (llr == 0).any()
    ref = model(kind, code, llr, L, scale_16=14, offset=2, max_iter=8)
    forced, plain = forced_and_not(F, kind, code, L, monkeypatch, max_iter=8, scale_16=14, offset=2)
    dc = next(x for x in (8, 16, 32, 48, 64) if code.dc_max <= x)
    check_global_describe(forced.describe(), kind, code, dc=dc)
    out = run(forced, llr, torch_dev)
    assert_same(out, ref, code.n, where=f"{kind} {which} forced")
    same_outputs(out, run(plain, llr, torch_dev))


@pytest.mark.parametrize("kind", KINDS)
def test_more_frames_than_the_grid(F, torch_dev, monkeypatch, kind):
    """The resident grid plus 3 frames: a slice's second frame starts from zero state and fresh accumulators."""
    code = F.Code.array(7, 3)
    dec = create(F, kind, code, 0, monkeypatch, max_iter=4, scale_16=12)
    f = check_global_describe(dec.describe(), kind, code)
    grid = f["grid"]
    llr = rand(31, 64, code.n, 3000)
    ref = model(kind, code, llr, scale_16=12, max_iter=4)
    sel = np.tile(np.arange(64), -(-(grid + 3) // 64))[:grid + 3]
    big = {k: ref[k][sel] for k in KEYS}
    assert_same(run(dec, llr[sel], torch_dev), big, code.n, where=f"{kind} batch {grid + 3}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("precheck", [False, True])
def test_precheck(F, O, codes, monkeypatch, precheck, kind):
    code = codes["A"][0]
    llr = awgn(F, O, code, 8.0, 16)
    ref = model(kind, code, llr, scale_16=12, precheck=precheck)
    pre = ref["prechecked"]
    assert pre.any() == precheck and not pre.all()
    sentinel = np.full(llr.shape, -123456, np.int32)
    dec = create(F, kind, code, 0, monkeypatch, precheck=precheck, scale_16=12)
    assert "mem=global" in dec.describe()
    out = dec.decode_host(llr, post=sentinel.copy())
    assert_same(out, ref, code.n, check_post=False, where=f"{kind} precheck={precheck}")
    assert (out["iters"][pre] == 0).all() and (out["iters"][~pre] >= 1).all()
    assert (out["post"][pre] == -123456).all()
    assert (out["post"][~pre] == ref["post"][~pre]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_without_early_termination_and_max_iter_1(F, case_a, torch_dev, monkeypatch, kind):
    code, llr = case_a
    ref = model(kind, code, llr[20:36], scale_16=12, max_iter=5, early_term=False)
    assert (ref["iters"] == 5).all() and ref["syndrome_ok"].any() and not ref["syndrome_ok"].all()
    dec = create(F, kind, code, 0, monkeypatch, max_iter=5, early_term=False, scale_16=12)
    assert_same(run(dec, llr[20:36], torch_dev), ref, code.n, where=f"{kind} early_term=False")
    ref = model(kind, code, llr[:16], max_iter=1)
    assert (ref["iters"] == 1).all()
    dec = create(F, kind, code, 0, monkeypatch, max_iter=1)
    assert_same(run(dec, llr[:16], torch_dev), ref, code.n, where=f"{kind} max_iter=1")


@pytest.mark.parametrize("kind", KINDS)
def test_int16_and_int32_llr(F, case_a, torch_dev, monkeypatch, kind):
    """The same frames as int16 and as int32 LLRs; then int32 LLRs beyond int16: the input clamp runs first."""
    code, llr = case_a
    dec = create(F, kind, code, 0, monkeypatch)
    a, b = run(dec, llr, torch_dev, np.int16), run(dec, llr, torch_dev, np.int32)
    assert_same(a, model(kind, code, llr), code.n, where=f"{kind} int16")
    same_outputs(a, b)
    big = llr[28:36].astype(np.int64) * 4097 + np.sign(llr[28:36]) * 65536
    assert np.abs(big).max() > 2 ** 23 and np.abs(big).max() < 2 ** 31
    big = big.astype(np.int32)
    assert_same(run(dec, big, torch_dev), model(kind, code, big), code.n, where=f"{kind} int32 beyond S_p")


@pytest.mark.parametrize("kind", KINDS)
def test_counters_streams_and_two_decoders(F, case_a, torch_dev, monkeypatch, kind):
    """bit_errors and totals over two calls, two calls on one stream, and a forced and an unforced decoder
    of the same code alive at once, decoding in turn."""
    import torch
    code, llr = case_a
    r = model(kind, code, llr)
    idx = np.arange(0, code.n, 3, dtype=np.int32)
    bits = (np.arange(len(idx)) % 5 == 0).astype(np.uint8)
    want = (r["hard"][:, idx] != bits).sum(axis=1)
    dec, plain = forced_and_not(F, kind, code, 0, monkeypatch)
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
        assert_same({k: v.cpu().numpy() for k, v in o.items()}, r, code.n, where=f"{kind} stream")
