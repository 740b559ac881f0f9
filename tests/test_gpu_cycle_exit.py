"""The cycle exit of the packed A kernel's split tail (flood_pk<ArrayChecks<47>, 3>, DESIGN.md "Cycle exit
(round 21)") against the oracle: a lone frame whose messages repeat with a period of 2 to 8 updates ends
early and must report exactly what max_iter iterations give -- iterations, hard bits, syndrome verdict,
posteriors and bit errors equal, not close.

The oracle itself says which frames cycle: its edge RAM after k iterations holds the v2c messages, and
first_cycle() walks orc_decode_general_edges one iteration at a time over the kept edge RAM (as
test_gpu_stationary.first_stationary does) until the edge RAM equals that of an earlier iteration j: the
frame has entered its cycle by update j, and k - j is its period.  The kernel compares the c2v messages,
which repeat from update j + 1 at the latest.

Oracle figures (seed 123456789, Q4.4, mask 0xff, printed by the tests):
  0 dB, frames 0..4095: 4056 become stationary; the other 40 cycle with period 3 (15 frames), 4 (4), 6 (17)
  or 8 (4), each inside its cycle by update 6.  The four single frames here: 20 (period 3), 1266 (4),
  1123 (6), 221 (8), entry <= 5.
  1 dB, frames 0..47: 36 periodic, 15 of them with a period of 2 or more; 2, 3 and 4.5 dB, frames 0..47: none.
  The arming predictor "every posterior of some check was left unchanged by the update" (first_cycle's
  `armed`): 1 dB 48 of 48 frames, 649 updates; 2 dB, 3 dB, 4.5 dB: no frame, no update.  The kernel's own
  form of it is weaker, the 15-bit XOR of a check's 47 posteriors, and small posteriors leave that XOR
  unchanged by chance: in the failing frames of 2 / 3 / 4.5 dB (24 / 48 / 35 frames, 696 / 1392 / 1014
  updates) some check's XOR repeats at 691 / 1118 / 236 updates, two checks of one wave at 575 / 352 / 8,
  eight checks of one wave at none; the 40 cyclers of 0 dB leave 30 and more checks, 11 and more in one wave,
  unchanged at every update from the third.  So the kernel arms on eight lanes of a wave.  The exit's
  result does not depend on the arming -- it only chooses when snapshots are taken -- so the tests assert
  the exits and the outputs, not the predictor.
"""
import math

import numpy as np
import pytest

from conftest import assert_same
from test_gpu_stationary import A_KERNEL, MAX_ITER, SEED, _bounds, _decode, _sub, first_stationary

pytestmark = pytest.mark.gpu

SINGLES = {20: 3, 1266: 4, 1123: 6, 221: 8}  # frame: period (0 dB)
CYCLERS = [20, 121, 191, 221, 383, 1056, 1123, 1141, 1192, 1266, 1525, 1575, 1683]  # 13 of the 40


@pytest.fixture(scope="module")
def acode(F, O):
    c = F.Code.array(47, 5)
    return c, O.OracleCode.from_alist_text(c.write_alist())


def _frames(O, code, eb, frames):
    """The LLRs of the listed frames of the bench stream at eb dB."""
    snr = 2 * math.pow(10.0, eb / 10) * code.rate
    return np.concatenate([O.gen_llr(SEED, int(f), 1, code.n, snr, math.sqrt(1 / snr), 4) for f in frames])


def first_cycle(O, ocode, llr, max_iter=MAX_ITER, frac_bits=4, armed=None):
    """Per frame (entry, period): the first k whose v2c equal those of an earlier iteration j gives entry j
    and period k - j (1: stationary); (-1, 0) if there is none within max_iter or the syndrome passes first.
    armed, a list, receives per frame the updates (2..) that left every posterior of some check unchanged."""
    out = np.zeros((len(llr), 2), np.int32)
    out[:, 0] = -1
    fn = O.lib().orc_decode_general_edges
    clist = ocode._clist - 1
    for f, x in enumerate(llr):
        od = O.FSMDecoder(ocode, max_iter=1, frac_bits=frac_bits)
        seen, post, arm = {}, None, []
        for k in range(1, max_iter + 1):
            _, ok = od._run(fn, x, k > 1)
            if ok:
                break
            if post is not None and not (od.post != post)[clist].any(axis=1).all():
                arm.append(k)
            post = od.post.copy()
            key = od.edge.tobytes()
            if key in seen:
                out[f] = seen[key], k - seen[key]
                break
            seen[key] = k
        if armed is not None:
            armed.append(arm)
    return out


@pytest.fixture(scope="module")
def singles(O, acode):
    """The four single frames at 0 dB, their LLRs and oracle cycles (computed once, read only)."""
    code, ocode = acode
    llr = _frames(O, code, 0.0, list(SINGLES))
    llr.setflags(write=False)
    cyc = first_cycle(O, ocode, llr)
    print("singles (entry, period):", dict(zip(SINGLES, cyc.tolist())))
    assert (cyc[:, 1] == list(SINGLES.values())).all() and (cyc[:, 0] >= 1).all() and (cyc[:, 0] <= 5).all(), cyc
    return llr, O.decode_batch(ocode, llr)


def _reference(code, seed=3):
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(code.n, size=code.n - code.rank, replace=False)).astype(np.int32)
    return idx, rng.integers(0, 2, size=len(idx)).astype(np.uint8)


@pytest.mark.parametrize("grid", ["1", None])
def test_single_frame_batches(F, O, acode, singles, torch_dev, monkeypatch, grid):
    """One-frame batches: the frame is in the split form from its first step, so the exit must fire (entry
    <= 5 and period <= 8: by update 24 of 30)."""
    if grid:
        monkeypatch.setenv("FPLDPC_GRID_PER_CU", grid)
    code, ocode = acode
    llr, ref = singles
    assert (ref["iters"] == MAX_ITER).all() and not ref["syndrome_ok"].any()
    dec = F.Decoder(code)
    assert dec.describe().startswith(A_KERNEL), dec.describe()
    idx, bits = _reference(code)
    dec.set_reference(idx, bits)
    for i, f in enumerate(SINGLES):
        gpu = _decode(dec, llr[i:i + 1], torch_dev, bit_errors=True)
        n_cyc, n_stat = dec.cycle_exits(), dec.stationary_exits()
        print(f"frame {f}: cycle exits {n_cyc}, stationary exits {n_stat}")
        assert_same(gpu, _sub(ref, slice(i, i + 1)), code.n, where=f"frame {f}")
        assert (gpu["bit_errors"] == (ref["hard"][i:i + 1, idx] != bits[None, :]).sum(axis=1)).all(), f
        assert (n_cyc, n_stat) == (1, 0), (f, n_cyc, n_stat)
        assert dec.fallback_counts() == (0, 0)


@pytest.mark.parametrize("max_iter", [9, 12, 17, 24, 30, 31, 32, 33, 35, 37, 40])
def test_max_iter_sweep(F, O, acode, singles, torch_dev, max_iter):
    """Every remainder of the updates left over the period, and caps where no window fits; early termination
    on and off, the pre-check on and off."""
    code, ocode = acode
    llr = singles[0]
    idx, bits = _reference(code)
    for pre in (False, True):
        ref = O.decode_batch(ocode, llr, max_iter=max_iter, precheck=pre)
        assert (ref["iters"] == max_iter).all()  # none converges: the oracle ran every frame to the cap
        for et in (True, False):
            dec = F.Decoder(code, max_iter=max_iter, precheck=pre, early_term=et)
            dec.set_reference(idx, bits)
            for i, f in enumerate(SINGLES):
                gpu = _decode(dec, llr[i:i + 1], torch_dev, bit_errors=True)
                where = f"frame {f} max_iter={max_iter} precheck={pre} early_term={et}"
                assert_same(gpu, _sub(ref, slice(i, i + 1)), code.n, where=where)
                assert (gpu["bit_errors"] == (ref["hard"][i:i + 1, idx] != bits[None, :]).sum(axis=1)).all(), where
                assert dec.cycle_exits() <= 1 and dec.stationary_exits() == 0, where


@pytest.fixture(scope="module")
def mixed(O, acode):
    """96 frames at 0 dB: 13 cyclers, each followed by neighbours of the same stream."""
    code, ocode = acode
    frames = []
    for i, f in enumerate(CYCLERS):
        frames += list(range(f, f + (8 if i < 5 else 7)))
    assert len(frames) == 96 and len(set(frames)) == 96
    llr = _frames(O, code, 0.0, frames)
    llr.setflags(write=False)
    return frames, llr, O.decode_batch(ocode, llr), first_stationary(O, ocode, llr), first_cycle(O, ocode, llr)


def test_mixed_batch(F, O, acode, mixed, torch_dev):
    """48 workgroups of two frames: the first frame to end sends its partner to the split form."""
    code, ocode = acode
    frames, llr, ref, k, cyc = mixed
    cyclers = int((cyc[:, 1] >= 2).sum())
    must, may = _bounds(k)
    print(f"mixed: {cyclers} cyclers (periods {sorted(cyc[cyc[:, 1] >= 2, 1].tolist())}), stationary must {must} may {may}")
    assert cyclers >= 13 and cyclers + may == 96, (cyclers, may)
    dec = F.Decoder(code)
    idx, bits = _reference(code)
    dec.set_reference(idx, bits)
    gpu = _decode(dec, llr, torch_dev, bit_errors=True)
    n_cyc, n_stat = dec.cycle_exits(), dec.stationary_exits()
    print(f"mixed: cycle exits {n_cyc}, stationary exits {n_stat}")
    assert_same(gpu, ref, code.n, where="mixed")
    assert (gpu["bit_errors"] == (ref["hard"][:, idx] != bits[None, :]).sum(axis=1)).all()
    assert dec.fallback_counts() == (0, 0)
    assert n_cyc <= cyclers, (n_cyc, cyclers)
    assert must <= n_stat <= may, (must, n_stat, may)


@pytest.mark.parametrize("eb", [2.0, 3.0, 4.5])
def test_other_snrs(F, O, acode, torch_dev, eb):
    """Frames 0..47 at 2, 3 and 4.5 dB: the oracle finds none periodic; no exit of either kind, parity."""
    code, ocode = acode
    llr = _frames(O, code, eb, range(48))
    armed = []
    cyc = first_cycle(O, ocode, llr, armed=armed)
    print(f"{eb} dB: periodic {int((cyc[:, 0] >= 0).sum())} of 48; frames the predictor arms {sum(1 for a in armed if a)}, "
          f"armed updates {sum(len(a) for a in armed)}")
    assert (cyc[:, 0] < 0).all(), cyc
    dec = F.Decoder(code)
    gpu = _decode(dec, llr, torch_dev)
    assert_same(gpu, O.decode_batch(ocode, llr), code.n, where=f"{eb} dB")
    assert dec.cycle_exits() == 0 and dec.stationary_exits() == 0


def test_range_fallback(F, O, acode, singles, torch_dev):
    """Each cycler paired with a full-range random frame (+-32767), which is out of the int16 kernel's range
    from its load and taints its partner: both go to the fallback."""
    code, ocode = acode
    rng = np.random.default_rng(17)
    llr = np.repeat(np.array(singles[0]), 2, axis=0)
    llr[1::2] = rng.integers(-32767, 32768, (len(SINGLES), code.n))
    ref = O.decode_batch(ocode, llr)
    dec = F.Decoder(code)
    gpu = _decode(dec, llr, torch_dev)
    fb, n_cyc = dec.fallback_counts(), dec.cycle_exits()
    assert_same(gpu, ref, code.n, where=f"range fallback={fb} cycle exits={n_cyc}")
    assert fb[0] >= len(SINGLES) and fb[1] == 0, fb
    assert n_cyc <= len(SINGLES)


def test_knob_off(F, O, acode, mixed, torch_dev, monkeypatch):
    """FPLDPC_CYCLE_EXIT=0 at decoder creation: identical outputs, no cycle exit, the stationary exit as before."""
    code, ocode = acode
    frames, llr, ref, k, cyc = mixed
    on = F.Decoder(code)
    monkeypatch.setenv("FPLDPC_CYCLE_EXIT", "0")
    off = F.Decoder(code)
    g_on, g_off = _decode(on, llr, torch_dev), _decode(off, llr, torch_dev)
    assert off.cycle_exits() == 0 and off.stationary_exits() >= _bounds(k)[0]
    for key in g_on:
        assert (g_on[key] == g_off[key]).all(), key
    assert_same(g_off, ref, code.n, where="knob off")
