"""The layered decoder on the GPU (fpldpc_layered_*, fixedpointldpc_amd.LayeredDecoder) against the numpy
model of its definition (tests/layered_model.py): iterations, hard decisions, syndrome flags and
posteriors exactly, on every path of the kernel -- c2v in LDS with computed addressing (A, the
exact-degree form) and with the index table in global memory or in LDS (W, whose layers of 81 are
wider than a wave and mix degrees 7 and 8), c2v in global scratch (R, and forced on W and small
codes), every predicated kernel width, small and irregular codes, every layer size, every parameter.
Every model run asserts
that its largest |value| stayed below 2^31: the definition holds inside int32 only, and that is a
condition on the inputs, not a tolerance."""
import numpy as np
import pytest

import layered_model as M
from conftest import assert_same

pytestmark = pytest.mark.gpu
SEED = 123456789


def awgn(F, O, code, eb, frames, first=0, frac=4):
    snr, sigma = F.snr_sigma(eb, code.rate)
    return O.gen_llr(SEED, first, frames, code.n, snr, sigma, frac)


def rand(seed, frames, n, lim):
    return np.random.default_rng(seed).integers(-lim, lim, (frames, n)).astype(np.int32)


def model(code, llr, L=0, **kw):
    ref = M.layered_decode(M.ModelCode.from_code(code), llr, L or code.layering()[0], **kw)
    assert ref["peak"] < 2 ** 31, f"inputs leave the int32 envelope (peak {ref['peak']})"
    return ref


def run(dec, llr, dev, dtype=np.int32, **kw):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(llr.astype(dtype))).to(dev)
    out = dec.decode_torch(t, post=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def case_a(F, O, codes):
    """The A frames most tests share, and their model result (computed once, never modified)."""
    code = codes["A"][0]
    llr = np.concatenate([awgn(F, O, code, 4.5, 24), awgn(F, O, code, 4.0, 24), rand(1, 8, code.n, 32768),
                          rand(2, 8, code.n, 2000), rand(3, 4, code.n, 3)])
    return code, llr, model(code, llr)


def test_a(F, case_a, torch_dev):
    code, llr, ref = case_a
    assert (llr[-4:] == 0).any() and np.abs(llr[48:56]).max() > 32000  # exact zeros (sgn(0) = -1); beyond int16 c2v
    dec = F.LayeredDecoder(code)
    assert_same(run(dec, llr, torch_dev), ref, code.n, where="A")
    d = dec.describe()
    assert d.startswith("layered_generic<DC=47,c2v=lds,addr=computed,deg=exact> L=47 layers=5 "), d
    assert 1 < ref["iters"][:24].mean() < 30 and (ref["iters"][24:48] == 30).any()


def test_w(F, O, codes, torch_dev):
    code = codes["W"][0]
    llr = np.concatenate([awgn(F, O, code, 2.0, 16), awgn(F, O, code, 1.5, 16), rand(4, 4, code.n, 32768),
                          rand(5, 4, code.n, 2000), rand(6, 4, code.n, 3)])
    dec = F.LayeredDecoder(code)
    assert_same(run(dec, llr, torch_dev), model(code, llr), code.n, where="W")
    d = dec.describe()
    # (the index table stays in global memory where LDS would cost resident workgroups: "gtable")
    assert d.startswith("layered_generic<DC=8,c2v=lds,addr=gtable,deg=table> L=81 layers=12 ") and "threads=128" in d, d


def test_w_with_the_table_in_lds(F, O, codes, torch_dev, monkeypatch):
    code = codes["W"][0]
    llr = np.concatenate([awgn(F, O, code, 2.0, 6), rand(9, 2, code.n, 2000)])
    monkeypatch.setenv("FPLDPC_LAYERED_TABLE", "lds")
    dec = F.LayeredDecoder(code)
    monkeypatch.delenv("FPLDPC_LAYERED_TABLE")
    assert "c2v=lds,addr=table," in dec.describe(), dec.describe()
    assert_same(run(dec, llr, torch_dev), model(code, llr), code.n, where="W, table in LDS")


def test_r(F, O, codes, torch_dev):
    """R: 1128 x 47 int32 c2v do not fit LDS (global scratch), 50 iterations with the 6-bit wrap.  No
    frame above 6 dB runs with early_term = 0 (its posteriors would leave int32)."""
    code = codes["R"][0]
    llr = np.concatenate([awgn(F, O, code, 6.5, 12), awgn(F, O, code, 7.0, 8), rand(7, 4, code.n, 2000)])
    ref = model(code, llr, max_iter=50, mask=0x3F)
    dec = F.LayeredDecoder(code, max_iter=50, width_mask=0x3F)
    assert_same(run(dec, llr, torch_dev), ref, code.n, where="R")
    d = dec.describe()
    assert d.startswith("layered_generic<DC=47,c2v=global,addr=computed,deg=exact> L=47 layers=24 "), d
    assert (ref["iters"][:12] == 1).any() and (ref["iters"][:12] == 50).any()


def test_lds_state_above_64k(F, O, codes, torch_dev):
    """p = 47, r = 10: 88 KB of c2v with the posteriors in LDS, above the 64 KB a kernel gets unasked."""
    code = F.Code.array(47, 10)
    llr = np.concatenate([awgn(F, O, code, 5.0, 6), rand(8, 2, code.n, 2000)])
    dec = F.LayeredDecoder(code, max_iter=10)
    assert_same(run(dec, llr, torch_dev), model(code, llr, max_iter=10), code.n, where="array 47 x 10")
    d = dec.describe()
    assert "c2v=lds" in d and int(d.split("lds=")[1].split()[0]) > 64 * 1024, d


def irregular_alist(seed=11, n=24, m=12):
    """A seeded irregular non-quasi-cyclic code: check degrees 2..6, rows ascending."""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(n, int(rng.integers(2, 7)), replace=False)) for _ in range(m)]
    cols = [[c for c in range(m) if v in rows[c]] for v in range(n)]
    lines = [f"{n} {m}", f"{max(len(c) for c in cols)} {max(len(r) for r in rows)}",
             " ".join(str(len(c)) for c in cols), " ".join(str(len(r)) for r in rows)]
    lines += [" ".join(map(str, c)) for c in cols] + [" ".join(map(str, r)) for r in rows]
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("which", ["array5x2", "array7x3", "irregular", "array11x2", "array23x2", "array37x2", "array53x2"])
def test_small_codes(F, torch_dev, which):
    """Small and irregular codes, and one code per predicated kernel width: degrees 11, 23, 37 and 53
    take DC = 16, 32, 48 and 64 (A and R take the exact-degree form)."""
    code = {"irregular": lambda: F.Code.parse(irregular_alist())}.get(
        which, lambda: F.Code.array(*map(int, which[5:].split("x"))))()
    L = 1 if which == "irregular" else 0
    llr = np.concatenate([rand(20, 16, code.n, 200), rand(21, 12, code.n, 2000), rand(22, 4, code.n, 3)])
    ref = model(code, llr, L, max_iter=8)
    dec = F.LayeredDecoder(code, max_iter=8, layer_checks=L)
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=which)
    if which.startswith("array"):
        dc = next(d for d in (8, 16, 32, 48, 64) if code.dc_max <= d)
        assert f"<DC={dc},c2v=lds,addr=computed,deg=table>" in dec.describe(), dec.describe()
    if which == "irregular":
        assert code.layering(1) == (1, 12) and "addr=table,deg=table> L=1 layers=12 " in dec.describe(), dec.describe()
        assert sorted(set(code.lists()[1])) != [code.dc_max]  # mixed degrees


@pytest.mark.parametrize("which", ["W", "irregular", "array7x3"])
def test_global_state_on_codes_that_fit_lds(F, O, codes, torch_dev, monkeypatch, which):
    """FPLDPC_LAYERED_C2V=global (read at creation) keeps c2v and the index table in global memory:
    the table form of the path R takes, on mixed degrees and on small codes."""
    code = {"W": lambda: codes["W"][0], "irregular": lambda: F.Code.parse(irregular_alist()),
            "array7x3": lambda: F.Code.array(7, 3)}[which]()
    L = 1 if which == "irregular" else 0
    llr = np.concatenate([awgn(F, O, code, 2.0, 6), rand(23, 6, code.n, 2000), rand(24, 2, code.n, 3)])
    monkeypatch.setenv("FPLDPC_LAYERED_C2V", "global")
    dec = F.LayeredDecoder(code, max_iter=8, layer_checks=L)
    monkeypatch.delenv("FPLDPC_LAYERED_C2V")
    assert "c2v=global" in dec.describe(), dec.describe()
    assert_same(run(dec, llr, torch_dev), model(code, llr, L, max_iter=8), code.n, where=f"{which} global")


@pytest.mark.parametrize("name,eb,frames,Ls,max_iter", [("A", 4.5, 4, (1, 47), 5), ("W", 2.0, 8, (27, 81), 30)])
def test_layer_size_is_not_semantics(F, O, codes, torch_dev, name, eb, frames, Ls, max_iter):
    code = codes[name][0]
    llr = awgn(F, O, code, eb, frames)
    ref = model(code, llr, Ls[1], max_iter=max_iter)
    outs = []
    for L in Ls:
        dec = F.LayeredDecoder(code, max_iter=max_iter, layer_checks=L)
        assert f" L={L} layers={code.m // L} " in dec.describe()
        outs.append(run(dec, llr, torch_dev))
        assert_same(outs[-1], ref, code.n, where=f"{name} L={L}")
    for k in ("iters", "hard", "syndrome_ok", "post"):
        assert (outs[0][k] == outs[1][k]).all(), k


@pytest.mark.parametrize("max_iter", [1, 2])
def test_max_iter(F, case_a, torch_dev, max_iter):
    code, llr, _ = case_a
    llr = llr[:16]
    ref = model(code, llr, max_iter=max_iter)
    assert_same(run(F.LayeredDecoder(code, max_iter=max_iter), llr, torch_dev), ref, code.n, where=f"max_iter={max_iter}")
    assert (ref["iters"] == max_iter).any()


def test_no_early_termination(F, O, codes, torch_dev):
    code = codes["A"][0]
    llr = awgn(F, O, code, 0.0, 16)
    ref = model(code, llr, early_term=False)
    assert (ref["iters"] == 30).all()
    assert_same(run(F.LayeredDecoder(code, early_term=False), llr, torch_dev), ref, code.n, where="early_term=0")


def test_precheck(F, O, codes):
    """A passing channel syndrome returns 0 iterations with the channel decision and leaves the
    posteriors buffer untouched."""
    code = codes["A"][0]
    llr = awgn(F, O, code, 8.0, 32)
    ref = model(code, llr, precheck=True)
    pre = ref["prechecked"]
    assert pre.any() and not pre.all()
    assert (ref["iters"][pre] == 0).all() and (ref["iters"][~pre] >= 1).all()
    sentinel = np.full(llr.shape, -123456, np.int32)
    out = F.LayeredDecoder(code, precheck=True).decode_host(llr, post=sentinel.copy())
    assert_same(out, ref, code.n, check_post=False, where="precheck")
    assert (out["iters"][pre] == 0).all()
    assert (out["post"][pre] == -123456).all()
    assert (out["post"][~pre] == ref["post"][~pre]).all()


@pytest.mark.parametrize("frac,mask", [(2, 0x3F), (6, 0xFFF), (4, 0xF3)])
def test_arithmetic_parameters(F, O, codes, torch_dev, frac, mask):
    code = codes["A"][0]
    llr = awgn(F, O, code, 4.5, 16, frac=frac)
    ref = model(code, llr, frac_bits=frac, mask=mask)
    dec = F.LayeredDecoder(code, frac_bits=frac, width_mask=mask)
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"frac={frac} mask={mask:#x}")


def test_int16_and_int32_llr(F, case_a, torch_dev):
    code, llr, ref = case_a
    assert np.abs(llr).max() < 32768
    dec = F.LayeredDecoder(code)
    a, b = run(dec, llr, torch_dev, np.int16), run(dec, llr, torch_dev, np.int32)
    assert_same(a, ref, code.n, where="int16")
    for k in a:
        assert (a[k] == b[k]).all(), k


def test_batches(F, O, codes, torch_dev):
    """1, 3 and 2500 frames (50 distinct frames tiled: more than the resident grid, so workgroups
    pull several frames each)."""
    code = codes["A"][0]
    llr = awgn(F, O, code, 4.5, 50)
    ref = model(code, llr)
    dec = F.LayeredDecoder(code)
    grid = int(dec.describe().split("grid=")[1].split()[0])
    assert 0 < grid < 2500
    for b in (1, 3):
        assert_same(run(dec, llr[:b], torch_dev), {k: ref[k][:b] for k in ("iters", "hard", "syndrome_ok", "post")},
                    code.n, where=f"batch {b}")
    big = {k: np.tile(ref[k], (50,) + (1,) * (ref[k].ndim - 1)) for k in ("iters", "hard", "syndrome_ok", "post")}
    assert_same(run(dec, np.tile(llr, (50, 1)), torch_dev), big, code.n, where="batch 2500")


def test_counters(F, case_a, torch_dev):
    """bit_errors per frame and totals {bit errors, frames in error, frames, iteration sum} from the
    model's hard decisions; totals are added to across calls."""
    import torch
    code, llr, ref = case_a
    idx = np.arange(0, code.n, 3, dtype=np.int32)
    bits = (np.arange(len(idx)) % 5 == 0).astype(np.uint8)
    want = (ref["hard"][:, idx] != bits).sum(axis=1)
    dec = F.LayeredDecoder(code)
    dec.set_reference(idx, bits)
    tot = torch.zeros(4, dtype=torch.int64, device=torch_dev)
    out = None
    for _ in range(2):
        out = run(dec, llr, torch_dev, bit_errors=True, totals=tot)
    assert (out["bit_errors"] == want).all()
    one = np.array([want.sum(), (want > 0).sum(), len(llr), ref["iters"].sum()])
    assert (tot.cpu().numpy() == 2 * one).all(), (tot, one)
    host = dec.decode_host(llr, bit_errors=True, totals=np.array([1, 2, 3, 4]))
    assert (host["bit_errors"] == want).all() and (host["totals"] == one + [1, 2, 3, 4]).all()


def test_two_calls_on_a_stream(F, case_a, torch_dev):
    """Back to back on a non-default stream with nothing in between: the counter block resets itself."""
    import torch
    code, llr, ref = case_a
    dec = F.LayeredDecoder(code)
    t = torch.from_numpy(llr).to(torch_dev)
    s = torch.cuda.Stream(torch_dev)
    torch.cuda.synchronize()
    a = dec.decode_torch(t, post=True, stream=s)
    b = dec.decode_torch(t, post=True, stream=s)
    s.synchronize()
    for out in (a, b):
        assert_same({k: v.cpu().numpy() for k, v in out.items()}, ref, code.n, where="stream")
