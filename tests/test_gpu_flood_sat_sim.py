"""fpldpc_minsum_ber_sim and its harvest / source forms around a saturated flooding decoder (FloodSatDecoder): the
object is an fpldpc_minsum_t, so every simulation entry point of that family must run it, twin included.

Counters and the on_frame sequence against the frame loop restated in Python over a freshly created decoder: the
host channel's int16 LLRs, decode_host(bit_errors=True) in blocks and the ordered stop rule in numpy.  The widths
(10/8) are not the defaults: a twin built with defaults decodes the odd rounds differently (173 of the 1000
frames differ between 10/8 and 12/10 in the numpy model), and only the counters can show it.

Code.array(13, 2) at 4.0 dB, all-zero codeword, frames 37 .. 1036, max_iter 7, found on the CPU with
tests/flood_sat_model.py: 126 / 1000 frame errors, and the 25th frame error at frame 37 + 154, inside the third
chunk of 64.  The tests assert both properties on the GPU reference itself."""
import numpy as np
import pytest

import harvest_model as HM
from test_gpu_layered_sat import small_code
from test_gpu_sim_decoders import ordered, same

pytestmark = pytest.mark.gpu
SEED, INFO_SEED = 123456789, 24681357
FIRST, FRAMES, CHUNK, NEED, MAX_ITER, EB = 37, 1000, 64, 25, 7, 4.0
WIDTHS = dict(post_bits=10, msg_bits=8)
COUNTERS = ("bit_errors", "frame_errors", "frames", "iter_sum")


@pytest.fixture(scope="module")
def small(F):
    code = small_code(F, "array13x2")[0]
    return code, F.Encoder.from_code(code)


def make(F, code):
    dec = F.FloodSatDecoder(code, max_iter=MAX_ITER, **WIDTHS)
    assert dec.describe().endswith(" sat=10/8 state=i16"), dec.describe()
    return dec


def sim_args(F, small):
    code, enc = small
    snr, sigma = F.snr_sigma(EB, code.rate)
    return snr, sigma, dict(info_index=enc.info_index, info_bits=np.zeros(enc.k, np.uint8), seed=SEED, first_frame=FIRST,
                            max_frames=FRAMES)


@pytest.fixture(scope="module")
def reference(F, small):
    """(blkerror, iterations) of frames FIRST .. FIRST + FRAMES - 1 from the Python loop, computed once."""
    code, _ = small
    snr, sigma, kw = sim_args(F, small)
    dec = make(F, code)
    dec.set_reference(kw["info_index"], kw["info_bits"])
    blk, its = [], []
    for f0 in range(0, FRAMES, 256):
        llr = F.channel_llr(SEED, FIRST + f0, min(256, FRAMES - f0), code.n, snr, sigma, 4, dtype=np.int16)
        r = dec.decode_host(llr, bit_errors=True)
        blk.append(r["bit_errors"])
        its.append(r["iters"])
    out = (np.concatenate(blk), np.concatenate(its))
    for a in out:
        a.setflags(write=False)
    return out


def test_reference_is_a_fair_case(reference):
    """The frame error share is 5 % .. 50 % in both runs, and the stop frame lies strictly inside a chunk of round
    >= 2, so that rounds decoded by the twin are counted."""
    stop, _ = ordered(*reference, NEED)
    whole, _ = ordered(*reference, 0)
    for r in (stop, whole):
        print(r)
        assert 0.05 <= r["frame_errors"] / r["frames"] <= 0.5, r
    assert stop["frame_errors"] == NEED and whole["frames"] == FRAMES
    last = stop["frames"] - 1
    assert last // CHUNK >= 2 and 0 < last % CHUNK < CHUNK - 1, last


@pytest.mark.parametrize("device_channel", [False, True])
def test_counters_equal_the_python_loop(F, small, reference, device_channel):
    snr, sigma, kw = sim_args(F, small)
    seen = []
    r = make(F, small[0]).ber_sim(snr, sigma, max_frame_errors=NEED, chunk=CHUNK, device_channel=device_channel,
                                  on_frame=lambda *a: seen.append(a), **kw)
    same(r, seen, ordered(*reference, NEED), f"flood_sat device_channel={device_channel}")
    assert r["frames_decoded"] >= r["frames"]


def test_every_frame_counted(F, small, reference):
    """max_frame_errors = 0: all 1000 frames, the last chunk a short one."""
    snr, sigma, kw = sim_args(F, small)
    seen = []
    r = make(F, small[0]).ber_sim(snr, sigma, max_frame_errors=0, chunk=CHUNK, device_channel=True,
                                  on_frame=lambda *a: seen.append(a), **kw)
    same(r, seen, ordered(*reference, 0), "flood_sat every frame")


def restated(F, small, torch_dev, frames, source):
    """Frames FIRST .. of a random_info simulation decoded one call: hard decisions, codewords, blkerror, iterations."""
    import torch
    code, enc = small
    snr, sigma = F.snr_sigma(EB, code.rate)
    info = F.info_bits(INFO_SEED, FIRST, frames, enc.k)
    cw = enc.encode(info)
    llr, ovf = F.channel_llr_torch(SEED, FIRST, frames, code.n, snr, sigma, 4, cw=torch.from_numpy(cw).to(torch_dev),
                                   dtype=torch.int16, source=source)
    out = make(F, code).decode_torch(llr)
    torch.cuda.synchronize()
    assert int(ovf.cpu().sum()) == 0
    hard = F.unpack_hard(out["hard"].cpu().numpy(), code.n)
    return hard, cw, (hard[:, enc.info_index] != info).sum(axis=1), out["iters"].cpu().numpy()


@pytest.mark.parametrize("source,harvest", [("lehmer", None), ("lehmer", 8), ("philox", None)])
def test_random_info_harvest_and_philox(F, small, torch_dev, source, harvest):
    """random_info=True on the reference's noise stream, the same with harvest=8, and random_info on the counter-based
    source: each run to completion (256 frames, four chunks, the twin on the odd ones) against its restatement."""
    code, _ = small
    frames = 256
    snr, sigma = F.snr_sigma(EB, code.rate)
    hard, cw, blk, its = restated(F, small, torch_dev, frames, source)
    want, seq = ordered(blk, its, 0)
    assert 0 < want["frame_errors"] < frames
    seen = []
    more = {} if harvest is None else dict(harvest=harvest)
    r = make(F, code).ber_sim(snr, sigma, seed=SEED, first_frame=FIRST, max_frames=frames, max_frame_errors=0, chunk=CHUNK,
                              device_channel=True, random_info=True, info_seed=INFO_SEED, source=source,
                              on_frame=lambda *a: seen.append(a), **more)
    same(r, seen, (want, seq), f"flood_sat source={source} harvest={harvest}")
    if harvest is not None:
        want_hv = HM.harvest(hard, cw, code.lists()[3], its, blk, first_frame=FIRST, max_records=harvest)
        assert want_hv["counts"]["codeword_errors"] > harvest  # on the restatement alone: records are dropped
        HM.assert_equal(r["harvest"], want_hv, "flood_sat")
