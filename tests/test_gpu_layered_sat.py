"""The saturated layered decoder on the GPU (fpldpc_layered_create_sat, LayeredDecoder(post_bits=,
msg_bits=)) against the numpy model of its definition (tests/layered_sat_model.py): iterations, hard
decisions, syndrome flags and posteriors exactly, with int16 and int32 on-chip state, on every path of
the kernel -- A (exact degree, computed addresses), W (table in global memory and in LDS, layers wider
than a wave), R at 8 dB over several iterations (where the unsaturated decoder leaves int32) with its
c2v in either placement, every predicated width, small and irregular codes, every parameter.  The
model asserts the definition's bounds on every run, so no input is outside the envelope."""
import re

import numpy as np
import pytest

import layered_model as M
import layered_sat_model as S
from conftest import assert_same

pytestmark = pytest.mark.gpu
SEED = 123456789


def awgn(F, O, code, eb, frames, first=0, frac=4):
    snr, sigma = F.snr_sigma(eb, code.rate)
    return O.gen_llr(SEED, first, frames, code.n, snr, sigma, frac)


def rand(seed, frames, n, lim):
    return np.random.default_rng(seed).integers(-lim, lim, (frames, n)).astype(np.int32)


def model(code, llr, widths, L=0, **kw):
    return S.layered_sat_decode(M.ModelCode.from_code(code), llr, L or code.layering()[0], *widths, **kw)


def run(dec, llr, dev, dtype=np.int32, **kw):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(llr.astype(dtype))).to(dev)
    out = dec.decode_torch(t, post=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def case_a(F, O, codes):
    """The A frames most tests share, with their model results per widths (each computed once)."""
    code = codes["A"][0]
    llr = np.concatenate([awgn(F, O, code, 4.5, 24), awgn(F, O, code, 8.0, 8), rand(1, 8, code.n, 32768),
                          rand(3, 4, code.n, 3)])
    assert (llr[-4:] == 0).any() and np.abs(llr[32:40]).max() > 32000 and np.abs(llr).max() < 32768
    refs = {}

    def ref(widths):
        if widths not in refs:
            refs[widths] = model(code, llr, widths)
        return refs[widths]
    return code, llr, ref


@pytest.mark.parametrize("widths,state,lds", [((12, 10), "i16", 26526), ((16, 15), "i16", 26526), ((10, 8), "i16", 26526),
                                              ((20, 12), "i32", 53032)])
def test_a(F, case_a, torch_dev, widths, state, lds):
    """int16 state: 2209 posteriors (4420 B with the pad) + 16 B + c2v [47][235] int16; int32 state: today's 53032 B."""
    code, llr, ref = case_a
    r = ref(widths)
    dec = F.LayeredDecoder(code, post_bits=widths[0], msg_bits=widths[1])
    assert_same(run(dec, llr, torch_dev), r, code.n, where=f"A {widths}")
    d = dec.describe()
    assert d.startswith("layered_sat<DC=47,c2v=lds,addr=computed,deg=exact> L=47 layers=5 "), d
    assert d.endswith(f" sat={widths[0]}/{widths[1]} state={state}") and f" lds={lds} " in d, d
    assert 1 < r["iters"][:24].mean() < 30
    if widths == (12, 10):
        assert r["clipped"] > 0


def w_frames(F, O, code):
    return awgn(F, O, code, 2.0, 16)


@pytest.mark.parametrize("table", [None, "lds"])
def test_w(F, O, codes, torch_dev, monkeypatch, table):
    code = codes["W"][0]
    llr = w_frames(F, O, code)
    if table:
        monkeypatch.setenv("FPLDPC_LAYERED_TABLE", table)
    dec = F.LayeredDecoder(code, post_bits=12, msg_bits=10)
    if table:
        monkeypatch.delenv("FPLDPC_LAYERED_TABLE")
    d = dec.describe()
    assert d.startswith(f"layered_sat<DC=8,c2v=lds,addr={'table' if table else 'gtable'},deg=table> L=81 layers=12 "), d
    assert "threads=128" in d and d.endswith(" sat=12/10 state=i16"), d
    assert_same(run(dec, llr, torch_dev), model(code, llr, (12, 10)), code.n, where=f"W table={table}")


@pytest.fixture(scope="module")
def case_r(F, O, codes):
    code = codes["R"][0]
    llr = awgn(F, O, code, 8.0, 4)
    ref = model(code, llr, (12, 10), max_iter=3, early_term=False)
    assert ref["syndrome_ok"].all() and ref["clipped"] > 0
    return code, llr, ref


@pytest.mark.parametrize("c2v", [None, "global", "lds"])
def test_r(F, case_r, torch_dev, monkeypatch, c2v):
    """R at 8 dB, 3 iterations without early termination: outside int32 unsaturated
    (test_layered_sat_model.py).  Once as the placement rule has it (the global scratch: in LDS its
    int16 c2v, 110 KB, leaves one workgroup per CU), and with each placement forced."""
    code, llr, ref = case_r
    if c2v:
        monkeypatch.setenv("FPLDPC_LAYERED_C2V", c2v)
    dec = F.LayeredDecoder(code, max_iter=3, early_term=False, post_bits=12, msg_bits=10)
    if c2v:
        monkeypatch.delenv("FPLDPC_LAYERED_C2V")
    d = dec.describe()
    assert d.startswith(f"layered_sat<DC=47,c2v={c2v or 'global'},addr=computed,deg=exact> L=47 layers=24 "), d
    assert d.endswith(" sat=12/10 state=i16"), d
    if c2v == "lds":
        assert " lds=110468 " in d, d  # 4420 + 16 + 47 * 1128 * 2
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"R c2v={c2v}")


def test_forced_int32_state(F, case_a, torch_dev, monkeypatch):
    code, llr, ref = case_a
    monkeypatch.setenv("FPLDPC_LAYERED_STATE", "i32")
    dec = F.LayeredDecoder(code, post_bits=12, msg_bits=10)
    monkeypatch.delenv("FPLDPC_LAYERED_STATE")
    d = dec.describe()
    assert d.endswith(" sat=12/10 state=i32") and " lds=53032 " in d, d
    a = run(dec, llr, torch_dev)
    assert_same(a, ref((12, 10)), code.n, where="A forced int32 state")
    b = run(F.LayeredDecoder(code, post_bits=12, msg_bits=10), llr, torch_dev)
    for k in a:
        assert (a[k] == b[k]).all(), k


def irregular_alist(seed=11, n=24, m=12):
    """A seeded irregular non-quasi-cyclic code: check degrees 2..6, rows ascending."""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(n, int(rng.integers(2, 7)), replace=False)) for _ in range(m)]
    cols = [[c for c in range(m) if v in rows[c]] for v in range(n)]
    lines = [f"{n} {m}", f"{max(len(c) for c in cols)} {max(len(r) for r in rows)}",
             " ".join(str(len(c)) for c in cols), " ".join(str(len(r)) for r in rows)]
    lines += [" ".join(map(str, c)) for c in cols] + [" ".join(map(str, r)) for r in rows]
    return "\n".join(lines) + "\n"


def small_code(F, which):
    if which == "irregular":
        return F.Code.parse(irregular_alist()), 1
    return F.Code.array(*map(int, which[5:].split("x"))), 0


@pytest.mark.parametrize("c2v", [None, "global"])
@pytest.mark.parametrize("which", ["irregular", "array13x2", "array31x2", "array37x2", "array59x2"])
def test_small_codes(F, torch_dev, monkeypatch, which, c2v):
    """An irregular code (L = 1, table addressing, mixed degrees: DC = 8) and one array code per other
    predicated width: degrees 13, 31, 37 and 59 take DC = 16, 32, 48 and 64; p odd makes n odd, so the
    int16 posteriors end on half a word.  Random frames beyond S_p = 2047: every clamp acts.  Each with
    c2v in LDS and in the global scratch."""
    code, L = small_code(F, which)
    llr = rand(30, 8, code.n, 3000)
    ref = model(code, llr, (12, 10), L, max_iter=8)
    assert ref["clipped"] > 0
    if c2v:
        monkeypatch.setenv("FPLDPC_LAYERED_C2V", c2v)
    dec = F.LayeredDecoder(code, max_iter=8, layer_checks=L, post_bits=12, msg_bits=10)
    if c2v:
        monkeypatch.delenv("FPLDPC_LAYERED_C2V")
    d = dec.describe()
    dc = next(x for x in (8, 16, 32, 48, 64) if code.dc_max <= x)
    addr = "computed" if which != "irregular" else "table" if not c2v else "gtable"
    assert d.startswith(f"layered_sat<DC={dc},c2v={c2v or 'lds'},addr={addr},deg=table> ") and d.endswith("state=i16"), d
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"{which} c2v={c2v}")


def long_alist(q, cols=8, rows=2):
    """An array code cut to its first `cols` block columns: n = cols * q, m = rows * q, slot j of check
    c of block row i is variable j*q + c*(j+1+i) mod q (q prime: a block row's checks share no variable)."""
    chk = [[j * q + (c * (j + 1 + i)) % q for j in range(cols)] for i in range(rows) for c in range(q)]
    var = [[] for _ in range(cols * q)]
    for c, r in enumerate(chk):
        for v in r:
            var[v].append(c)
    lines = [f"{cols * q} {rows * q}", f"{rows} {cols}", " ".join([str(rows)] * (cols * q)), " ".join([str(cols)] * (rows * q))]
    lines += [" ".join(map(str, v)) for v in var] + [" ".join(map(str, r)) for r in chk]
    return "\n".join(lines) + "\n"


def test_code_longer_than_the_int32_state_allows(F, torch_dev):
    """n = 8 * 5147 = 41176: int32 posteriors (n <= 40956) do not fit LDS, int16 ones do; layers of 5147
    checks loop over the workgroup, and the c2v (165 KB) goes to the global scratch."""
    q = 5147
    assert all(q % d for d in range(2, 72))
    code = F.Code.parse(long_alist(q))
    assert code.n == 41176 and code.layering(q) == (q, 2)
    for kw in ({}, {"post_bits": 20, "msg_bits": 10}):
        with pytest.raises(F.FpldpcError) as e:
            F.LayeredDecoder(code, layer_checks=q, **kw)
        assert e.value.code == -4, e.value
    llr = rand(32, 3, code.n, 3000)
    ref = model(code, llr, (12, 10), q, max_iter=3)
    dec = F.LayeredDecoder(code, max_iter=3, layer_checks=q, post_bits=12, msg_bits=10)
    d = dec.describe()
    assert d.startswith(f"layered_sat<DC=8,c2v=global,addr=gtable,deg=table> L={q} layers=2 ") and "threads=256" in d, d
    assert_same(run(dec, llr, torch_dev), ref, code.n, where="n = 41176")


@pytest.mark.parametrize("frac,mask", [(2, 0x3F), (6, 0xFFF)])
def test_arithmetic_parameters(F, O, codes, torch_dev, frac, mask):
    code = codes["A"][0]
    llr = awgn(F, O, code, 4.5, 12, frac=frac)
    ref = model(code, llr, (12, 10), frac_bits=frac, mask=mask)
    dec = F.LayeredDecoder(code, frac_bits=frac, width_mask=mask, post_bits=12, msg_bits=10)
    assert_same(run(dec, llr, torch_dev), ref, code.n, where=f"frac={frac} mask={mask:#x}")


@pytest.mark.parametrize("precheck", [False, True])
def test_precheck(F, O, codes, precheck):
    """A passing channel syndrome (of the clamped LLRs: the same signs) returns 0 iterations with the
    channel decision and leaves the posteriors buffer untouched."""
    code = codes["A"][0]
    llr = awgn(F, O, code, 8.0, 16)
    ref = model(code, llr, (12, 10), precheck=precheck)
    pre = ref["prechecked"]
    assert pre.any() == precheck and not pre.all()
    sentinel = np.full(llr.shape, -123456, np.int32)
    out = F.LayeredDecoder(code, precheck=precheck, post_bits=12, msg_bits=10).decode_host(llr, post=sentinel.copy())
    assert_same(out, ref, code.n, check_post=False, where=f"precheck={precheck}")
    assert (out["iters"][pre] == 0).all() and (out["iters"][~pre] >= 1).all()
    assert (out["post"][pre] == -123456).all()
    assert (out["post"][~pre] == ref["post"][~pre]).all()


def test_max_iter_1(F, case_a, torch_dev):
    code, llr, _ = case_a
    ref = model(code, llr[:16], (12, 10), max_iter=1)
    dec = F.LayeredDecoder(code, max_iter=1, post_bits=12, msg_bits=10)
    assert_same(run(dec, llr[:16], torch_dev), ref, code.n, where="max_iter=1")
    assert (ref["iters"] == 1).all()


@pytest.mark.parametrize("widths", [(12, 10), (16, 15), (20, 12)])
def test_int16_and_int32_llr(F, case_a, torch_dev, widths):
    """The same frames as int16 and as int32 LLRs; then int32 LLRs beyond S_p and beyond int16 (65536 + x
    would narrow to x): the input clamp runs before the posteriors are stored."""
    code, llr, ref = case_a
    dec = F.LayeredDecoder(code, post_bits=widths[0], msg_bits=widths[1])
    a, b = run(dec, llr, torch_dev, np.int16), run(dec, llr, torch_dev, np.int32)
    assert_same(a, ref(widths), code.n, where="int16")
    for k in a:
        assert (a[k] == b[k]).all(), k
    big = llr[28:36].astype(np.int64) * 4097 + np.sign(llr[28:36]) * 65536
    assert np.abs(big).max() > 2 ** 23 and np.abs(big).max() < 2 ** 31
    big = big.astype(np.int32)
    assert_same(run(dec, big, torch_dev), model(code, big, widths), code.n, where="int32 beyond S_p")


def test_more_frames_than_the_grid(F, torch_dev):
    """The resident grid plus 3 frames on a small code: workgroups pull a second frame from the work counter."""
    code = F.Code.array(7, 3)
    dec = F.LayeredDecoder(code, max_iter=4, post_bits=12, msg_bits=10)
    grid = int(dec.describe().split("grid=")[1].split()[0])
    assert 0 < grid < 100000
    llr = rand(31, 64, code.n, 3000)
    ref = model(code, llr, (12, 10), max_iter=4)
    reps = -(-(grid + 3) // 64)
    sel = np.tile(np.arange(64), reps)[:grid + 3]
    big = {k: ref[k][sel] for k in ("iters", "hard", "syndrome_ok", "post")}
    assert_same(run(dec, llr[sel], torch_dev), big, code.n, where=f"batch {grid + 3}")


def test_two_calls_on_a_stream(F, case_a, torch_dev):
    import torch
    code, llr, ref = case_a
    dec = F.LayeredDecoder(code, post_bits=12, msg_bits=10)
    t = torch.from_numpy(llr).to(torch_dev)
    s = torch.cuda.Stream(torch_dev)
    torch.cuda.synchronize()
    a = dec.decode_torch(t, post=True, stream=s)
    b = dec.decode_torch(t, post=True, stream=s)
    s.synchronize()
    for out in (a, b):
        assert_same({k: v.cpu().numpy() for k, v in out.items()}, ref((12, 10)), code.n, where="stream")


def test_counters(F, case_a, torch_dev):
    """bit_errors per frame and totals {bit errors, frames in error, frames, iteration sum} from the
    model's hard decisions; totals are added to across calls."""
    import torch
    code, llr, ref = case_a
    r = ref((12, 10))
    idx = np.arange(0, code.n, 3, dtype=np.int32)
    bits = (np.arange(len(idx)) % 5 == 0).astype(np.uint8)
    want = (r["hard"][:, idx] != bits).sum(axis=1)
    dec = F.LayeredDecoder(code, post_bits=12, msg_bits=10)
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


def test_unsaturated_decoder_unchanged(F, codes):
    """fpldpc_layered_create keeps its kernel choice, LDS footprint and describe string."""
    d = F.LayeredDecoder(codes["A"][0]).describe()
    assert re.fullmatch(r"layered_generic<DC=47,c2v=lds,addr=computed,deg=exact> L=47 layers=5 grid=\d+ threads=64 "
                        r"lds=53032 device=0", d), d
    d = F.LayeredDecoder(codes["R"][0]).describe()
    assert re.fullmatch(r"layered_generic<DC=47,c2v=global,addr=computed,deg=exact> L=47 layers=24 grid=\d+ threads=64 "
                        r"lds=8852 device=0", d), d
