"""The stationary exit of the packed A kernel (flood_pk<ArrayChecks<47>, 3>, DESIGN.md "Stationary exit
(round 15)") against the oracle: a frame whose messages have stopped changing ends early and must
report exactly what max_iter iterations give -- iterations, hard bits, syndrome verdict, posteriors
and bit errors equal, not close.

The oracle itself says which frames are stationary: its edge RAM after k iterations holds the v2c
messages, and the first k whose edge arrays equal those after k + 1 is the frame's first stationary
iteration.  first_stationary() walks orc_decode_general_edges one iteration at a time over the kept edge
RAM (keep = 1 continues from what the array holds), which is the same sequence of states as calls
at max_iter = 1, 2, ... from scratch at a thirtieth of the work.

The kernel arms on equal posteriors of two consecutive updates and ends a frame when the c2v of two
consecutive updates are equal; a frame with first stationary iteration k passes that compare after
update k + 5 at the latest (up to three updates later when the frame sharing its lanes is at its own
last updates just then: the kernel arms only while the compare comes before either frame's end), so
every frame with k <= max_iter - 6 must end by the exit in these batches, and no frame the oracle
does not find stationary may.  A frame that ends by early termination is no exit.
"""
import math

import numpy as np
import pytest

from conftest import assert_same

pytestmark = pytest.mark.gpu

SEED = 123456789
A_KERNEL = "flood_array2<P=47,W=3>"
MAX_ITER = 30


@pytest.fixture(scope="module")
def acode(F, O):
    c = F.Code.array(47, 5)
    return c, O.OracleCode.from_alist_text(c.write_alist())


def _llr(O, code, eb, f0, frames):
    snr = 2 * math.pow(10.0, eb / 10) * code.rate
    return O.gen_llr(SEED, f0, frames, code.n, snr, math.sqrt(1 / snr), 4)


def first_stationary(O, ocode, llr, max_iter=MAX_ITER, frac_bits=4):
    """Per frame: the first k >= 1 with v2c(k) == v2c(k + 1), k + 1 <= max_iter; -1 if there is none or
    the syndrome passes first (the frame then ends by early termination)."""
    out = np.full(len(llr), -1, np.int32)
    fn = O.lib().orc_decode_general_edges
    for f, x in enumerate(llr):
        od = O.FSMDecoder(ocode, max_iter=1, frac_bits=frac_bits)
        prev = None
        for k in range(1, max_iter + 1):
            _, ok = od._run(fn, x, k > 1)
            if ok:
                break
            if prev is not None and (od.edge == prev).all():
                out[f] = k - 1
                break
            prev = od.edge.copy()
    return out


def _decode(dec, llr, torch_dev, **kw):
    import torch
    out = dec.decode_torch(torch.from_numpy(llr.astype(np.int16)).to(torch_dev), post=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bounds(k, max_iter=MAX_ITER):
    """(must exit, may exit) frame counts from the first stationary iterations."""
    return int(((k >= 1) & (k <= max_iter - 6)).sum()), int((k >= 1).sum())


@pytest.fixture(scope="module")
def pool0(O, acode):
    """Frames 0..1024 of the bench stream at 0 dB, their oracle decode, and the first stationary
    iteration of the first 256 (computed once, read only)."""
    code, ocode = acode
    llr = _llr(O, code, 0.0, 0, 1025)
    llr.setflags(write=False)
    ref = O.decode_batch(ocode, llr)
    return llr, ref, first_stationary(O, ocode, llr[:256])


def _sub(ref, sl):
    return {k: (v[sl] if v is not None else None) for k, v in ref.items()}


def test_stationary_frames_0db(F, O, acode, pool0, torch_dev):
    """Frames 0..255 at 0 dB: parity in every field, bit errors included; the exit count between the
    frames that must and the frames that may exit -- so the frames that cycle are not counted."""
    code, ocode = acode
    llr, ref, k = pool0
    llr, ref = llr[:256], _sub(ref, slice(0, 256))
    must, may = _bounds(k)
    print(f"0 dB: must {must}, may {may} of 256; first 96: must {_bounds(k[:96])[0]}; k mean {k[k >= 1].mean():.2f} max {k.max()}")
    assert _bounds(k[:96])[0] >= 90 and may < 256, (must, may)  # nearly all settle, and some frames cycle
    assert (ref["iters"] == MAX_ITER).all() and not ref["syndrome_ok"].any()
    dec = F.Decoder(code)
    assert dec.describe().startswith(A_KERNEL), dec.describe()
    rng = np.random.default_rng(3)
    idx = np.sort(rng.choice(code.n, size=code.n - code.rank, replace=False)).astype(np.int32)
    bits = rng.integers(0, 2, size=len(idx)).astype(np.uint8)
    dec.set_reference(idx, bits)
    gpu = _decode(dec, llr, torch_dev, bit_errors=True)
    n_exit = dec.stationary_exits()
    print(f"0 dB: {n_exit} exits")
    assert_same(gpu, ref, code.n, where="0 dB")
    assert (gpu["bit_errors"] == (ref["hard"][:, idx] != bits[None, :]).sum(axis=1)).all()
    assert dec.fallback_counts() == (0, 0)
    assert must <= n_exit <= may, (must, n_exit, may)
    # the first 96 on their own (one frame pair per workgroup, every second frame ends in the split tail)
    gpu = _decode(dec, llr[:96], torch_dev)
    assert_same(gpu, _sub(ref, slice(0, 96)), code.n, where="0 dB, 96 frames")
    m96, y96 = _bounds(k[:96])
    assert m96 <= dec.stationary_exits() <= y96, (m96, dec.stationary_exits(), y96)


@pytest.mark.parametrize("eb", [2.0, 3.0])
def test_no_stationary_frames(F, O, acode, torch_dev, eb):
    """Frames 0..47 at 2 dB and 3 dB: the oracle finds none stationary; no exit, parity."""
    code, ocode = acode
    llr = _llr(O, code, eb, 0, 48)
    k = first_stationary(O, ocode, llr)
    assert (k < 0).all(), k
    dec = F.Decoder(code)
    gpu = _decode(dec, llr, torch_dev)
    assert_same(gpu, O.decode_batch(ocode, llr), code.n, where=f"{eb} dB")
    assert dec.stationary_exits() == 0


def test_mixed_point_1db(F, O, acode, torch_dev):
    """Frames 0..47 at 1 dB: some frames settle late, some converge, some do neither."""
    code, ocode = acode
    llr = _llr(O, code, 1.0, 0, 48)
    k = first_stationary(O, ocode, llr)
    must, may = _bounds(k)
    print(f"1 dB: must {must}, may {may} of 48, k max {k.max()}")
    assert may >= 10 and k.max() >= 15, k
    dec = F.Decoder(code)
    gpu = _decode(dec, llr, torch_dev)
    n_exit = dec.stationary_exits()
    print(f"1 dB: {n_exit} exits")
    assert_same(gpu, O.decode_batch(ocode, llr), code.n, where="1 dB")
    assert must <= n_exit <= may, (must, n_exit, may)


@pytest.mark.parametrize("max_iter", [1, 2, 3, 4, 5, 8])
def test_small_max_iter_and_modes(F, O, acode, pool0, torch_dev, max_iter):
    """max_iter 1..5 and 8 (at the small values no verification can complete), early termination on
    and off, the pre-check on and off, posteriors requested: 0 dB frames and two that converge."""
    code, ocode = acode
    llr = np.concatenate([pool0[0][:14], _llr(O, code, 4.5, 0, 2)])
    k = first_stationary(O, ocode, llr, max_iter)
    for pre in (False, True):
        ref = O.decode_batch(ocode, llr, max_iter=max_iter, precheck=pre)
        for et in (True, False):
            dec = F.Decoder(code, max_iter=max_iter, precheck=pre, early_term=et)
            gpu = _decode(dec, llr, torch_dev)
            where = f"max_iter={max_iter} precheck={pre} early_term={et}"
            if et:
                assert_same(gpu, ref, code.n, check_post=not pre, where=where)
                assert dec.stationary_exits() <= _bounds(k, max_iter)[1], where
            else:
                # the oracle always stops at a passing syndrome: frames it ran to the cap compare in
                # full, the others must report the cap and the syndrome of their own hard decisions
                full = ref["iters"] == max_iter
                stopped0 = (ref["iters"] == 0) if pre else np.zeros(len(llr), bool)
                assert (gpu["iters"][~stopped0] == max_iter).all() and (gpu["iters"][stopped0] == 0).all(), where
                assert_same({k_: v[full] for k_, v in gpu.items()}, _sub(ref, full), code.n, where=where)
                hard = F.unpack_hard(gpu["hard"], code.n)
                assert [code.syndrome_ok(h) for h in hard] == [bool(o) for o in gpu["syndrome_ok"]], where
            if max_iter < 4:
                assert dec.stationary_exits() == 0, where


@pytest.mark.parametrize("split", ["1", "0"])
def test_batch_sizes_and_refills(F, O, acode, pool0, torch_dev, monkeypatch, split):
    """Batches of 1, 3 and 1025 frames on one workgroup per CU, the split tail on and off: halves are
    refilled, trigger on different steps, and lone frames meet the exit in the tail's form."""
    monkeypatch.setenv("FPLDPC_GRID_PER_CU", "1")
    monkeypatch.setenv("FPLDPC_SPLIT_TAIL", split)
    code, ocode = acode
    llr, ref, k = pool0
    dec = F.Decoder(code)
    assert dec.describe().startswith(A_KERNEL) and "grid=256" in dec.describe(), dec.describe()
    for B in (1, 3, 1025):
        gpu = _decode(dec, llr[:B], torch_dev)
        assert_same(gpu, _sub(ref, slice(0, B)), code.n, where=f"B={B} split={split}")
        n_exit = dec.stationary_exits()
        must, may = _bounds(k[:min(B, 256)])
        assert n_exit >= must and (B > 256 or n_exit <= may), (B, must, n_exit, may)
        assert n_exit <= B


def test_taint_path(F, O, acode, pool0, torch_dev):
    """0 dB frames interleaved with full-range random LLRs (+-32767): those are out of the int16 kernel's
    range from their load, and go to the fallback while their partners are being verified."""
    code, ocode = acode
    rng = np.random.default_rng(17)
    llr = np.array(pool0[0][:64])
    big = np.arange(1, 64, 2)
    llr[big] = rng.integers(-32767, 32768, (len(big), code.n))
    ref = O.decode_batch(ocode, llr)
    k = first_stationary(O, ocode, llr)
    dec = F.Decoder(code)
    gpu = _decode(dec, llr, torch_dev)
    fb, n_exit = dec.fallback_counts(), dec.stationary_exits()
    assert_same(gpu, ref, code.n, where=f"taint fallbacks={fb} exits={n_exit}")
    assert fb[0] >= len(big) and fb[1] == 0, fb
    assert n_exit <= _bounds(k)[1], (n_exit, _bounds(k))


def test_knob_off(F, O, acode, pool0, torch_dev, monkeypatch):
    """FPLDPC_STATIONARY_EXIT=0 at decoder creation: identical outputs, no exit."""
    code, ocode = acode
    llr = pool0[0][:256]
    on = F.Decoder(code)
    monkeypatch.setenv("FPLDPC_STATIONARY_EXIT", "0")
    off = F.Decoder(code)
    g_on, g_off = _decode(on, llr, torch_dev), _decode(off, llr, torch_dev)
    assert on.stationary_exits() > 0 and off.stationary_exits() == 0
    for key in g_on:
        assert (g_on[key] == g_off[key]).all(), key
    assert_same(g_off, _sub(pool0[1], slice(0, 256)), code.n, where="knob off")


def test_per_output_guard_variant(F, O, acode, torch_dev):
    """FRAC_WIDTH 8 (C = 160) selects the same kernel with the per-output range guard
    (ArrayChecksOutGuard), which has the exit too.  At -3 dB most of its frames settle (k = 3..14)."""
    code, ocode = acode
    snr = 2 * math.pow(10.0, -0.3) * code.rate
    llr = O.gen_llr(SEED, 0, 48, code.n, snr, math.sqrt(1 / snr), 8)
    k = first_stationary(O, ocode, llr, frac_bits=8)
    must, may = _bounds(k)
    assert must >= 20 and may < 48, k
    dec = F.Decoder(code, frac_bits=8, width_mask=0xFF)
    assert dec.describe().startswith(A_KERNEL), dec.describe()
    gpu = _decode(dec, llr, torch_dev)
    n_exit, fb = dec.stationary_exits(), dec.fallback_counts()
    print(f"frac 8, -3 dB: must {must}, may {may} of 48, {n_exit} exits, fallbacks {fb}")
    assert_same(gpu, O.decode_batch(ocode, llr, frac_bits=8, mask=0xFF), code.n, where="frac 8")
    assert fb == (0, 0) and must <= n_exit <= may, (must, n_exit, may, fb)
