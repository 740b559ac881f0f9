"""The harvest of a BER simulation (ber_sim(harvest=...), fpldpc_*_ber_sim_harvest) against the simulation
restated in Python -- the restatement of tests/test_gpu_sim_random_info.py (host information bits, the host
encoder, the device channel with a codeword per frame, decode_torch), kept to its hard decisions -- and
tests/harvest_model.py's statement of records, counts and classes on them.  p = 13, r = 2 at 4.0 dB, max_iter 7,
first_frame 37, chunks of 64, the three decoders of that file; A at 4.5 dB with flooding min-sum (70 hard words,
8 syndrome words).

What the restatements must show, asserted on them alone before anything is compared: detected and undetected
codeword errors on the small code for every decoder, detected ones on A.  (On one MI355X, 1000 frames of the
small code: 80 / 58 for flooding sxor, 114 / 41 for flooding min-sum, 130 / 45 for layered min-sum, the
undetected ones at weights 4, 6, 8 and 12; 500 frames of A with flooding min-sum: 11 detected, none undetected.)"""
import numpy as np
import pytest

import harvest_model as HM
import test_gpu_sim_random_info as RI
from test_gpu_layered_sat import small_code

pytestmark = pytest.mark.gpu
SEED, INFO_SEED, FIRST, CHUNK = RI.SEED, RI.INFO_SEED, RI.FIRST, RI.CHUNK
NAMES = list(RI.DECODERS)
COUNTERS = RI.COUNTERS


@pytest.fixture(scope="module")
def code_of(F):
    made = {}

    def get(which):
        if which not in made:
            code = F.Code.array(47, 5) if which == "A" else small_code(F, "array13x2")[0]
            made[which] = (code, F.Encoder.from_code(code), code.lists()[3])
        return made[which]
    return get


def make(F, code_of, which, name):
    cls, kw = RI.DECODERS[name]
    return getattr(F, cls)(code_of(which)[0], max_iter=RI.MAX_ITER, **kw)


@pytest.fixture(scope="module")
def restated(F, torch_dev, code_of):
    """(hard [frames][n], cw [frames][n], blkerror, iterations) of frames FIRST .. FIRST + frames - 1, each sent with
    its own information bits; computed once per (code, decoder, frames)."""
    import torch
    made = {}

    def get(which, name, eb, frames):
        key = (which, name, eb, frames)
        if key not in made:
            code, enc, _ = code_of(which)
            snr, sigma = F.snr_sigma(eb, code.rate)
            info = F.info_bits(INFO_SEED, FIRST, frames, enc.k)
            cw = enc.encode(info)
            cw_t = torch.from_numpy(cw).to(torch_dev)
            llr = torch.empty((frames, code.n), dtype=torch.int16, device=torch_dev)
            ovf = torch.zeros(1, dtype=torch.int32, device=torch_dev)
            F.channel_llr_ptrs(SEED, FIRST, frames, code.n, snr, sigma, 4, cw_t.data_ptr(), 1, llr.data_ptr(),
                               F.FPLDPC_LLR_I16, ovf.data_ptr(), torch.cuda.current_stream(torch_dev).cuda_stream)
            out = make(F, code_of, which, name).decode_torch(llr)
            torch.cuda.synchronize()
            assert int(ovf.cpu()[0]) == 0
            hard = F.unpack_hard(out["hard"].cpu().numpy(), code.n)
            blk = (hard[:, enc.info_index] != info).sum(axis=1)
            made[key] = (hard, cw, blk, out["iters"].cpu().numpy())
        return made[key]
    return get


def model(code_of, which, r, frames=None, max_records=1 << 20):
    hard, cw, blk, its = r
    k = len(hard) if frames is None else frames
    return HM.harvest(hard[:k], cw[:k], code_of(which)[2], its[:k], blk[:k], first_frame=FIRST, max_records=max_records)


def same_harvest(a, b):
    assert a.counts == b.counts and a.classes == b.classes
    for k in HM.FIELDS:
        assert (getattr(a, k) == getattr(b, k)).all(), k


def sim(F, dec, code, eb, frames, need, seen=None, **kw):
    return RI.sim(F, dec, code, eb, frames, need, seen, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_every_counted_frame(F, code_of, restated, name):
    """1000 frames, no error limit, nothing dropped: every record field, the counts and the classes; and the
    harvest against the result's own counters."""
    code = code_of("small")[0]
    r = restated("small", name, 4.0, 1000)
    want = model(code_of, "small", r)
    print(name, want["counts"], want["classes"])
    assert want["counts"]["detected"] > 0 and want["counts"]["undetected"] > 0  # on the restatement alone
    res = sim(F, make(F, code_of, "small", name), code, 4.0, 1000, 0, harvest=10000)
    hv = res["harvest"]
    HM.assert_equal(hv, want, name)
    assert hv.counts["dropped"] == 0 and hv.counts["frames"] == res["frames"] == 1000
    assert int((hv.info_errors > 0).sum()) == res["frame_errors"] > 0
    assert int(hv.info_errors.sum()) == res["bit_errors"]
    assert int(r[3].sum()) == res["iter_sum"]
    # the accessors: ascending positions, as many as the weights say
    for i in (0, len(hv.frame) - 1):
        e, s = hv.error_positions(i), hv.unsat_checks(i)
        assert len(e) == hv.weight[i] and len(s) == hv.unsat[i] and (np.diff(e) > 0).all() and (np.diff(s) > 0).all()
        f = int(hv.frame[i]) - FIRST
        assert e.tolist() == np.nonzero(r[0][f] != r[1][f])[0].tolist()


@pytest.mark.parametrize("name", NAMES)
def test_the_harvest_ends_at_the_stop_frame(F, code_of, restated, name):
    """25 frame errors: the stop frame lies past the second chunk with a third chunk in flight; the records end
    at the stop frame and no frame beyond it appears."""
    code = code_of("small")[0]
    r = restated("small", name, 4.0, 1000)
    counted, _ = RI.ordered(r[2], r[3], 25)
    stop = counted["frames"]
    assert 2 * CHUNK < stop < 1000 - 2 * CHUNK
    res = sim(F, make(F, code_of, "small", name), code, 4.0, 1000, 25, harvest=10000)
    assert {k: res[k] for k in COUNTERS} == counted and res["frames_decoded"] > stop
    hv = res["harvest"]
    HM.assert_equal(hv, model(code_of, "small", r, frames=stop), name)
    assert hv.counts["frames"] == stop and hv.frame.max() <= FIRST + stop - 1
    assert hv.frame[-1] == FIRST + stop - 1  # the stop frame is a frame error, so a codeword error: the last record


@pytest.mark.parametrize("name", NAMES)
def test_first_n_records(F, code_of, restated, name):
    code = code_of("small")[0]
    r = restated("small", name, 4.0, 1000)
    full = model(code_of, "small", r)
    total = full["counts"]["codeword_errors"]
    assert total > 7
    hv = sim(F, make(F, code_of, "small", name), code, 4.0, 1000, 0, harvest=7)["harvest"]
    HM.assert_equal(hv, model(code_of, "small", r, max_records=7), name)
    assert hv.counts["recorded"] == 7 and hv.counts["dropped"] == total - 7 and hv.classes == full["classes"]
    for k in HM.FIELDS:
        assert (getattr(hv, k) == full["records"][k][:7]).all(), k
    hv = sim(F, make(F, code_of, "small", name), code, 4.0, 1000, 0, harvest=0)["harvest"]
    HM.assert_equal(hv, model(code_of, "small", r, max_records=0), name)
    assert hv.counts == {**full["counts"], "recorded": 0, "dropped": total} and hv.classes == full["classes"]


@pytest.mark.parametrize("overlap", [None, "0"])
@pytest.mark.parametrize("name", NAMES)
def test_result_and_callbacks_do_not_know_of_the_harvest(F, code_of, restated, name, overlap, monkeypatch):
    code = code_of("small")[0]
    if overlap:
        monkeypatch.setenv("FPLDPC_SIM_OVERLAP", overlap)
    s0, s1 = [], []
    a = sim(F, make(F, code_of, "small", name), code, 4.0, 1000, 25, s0)
    b = sim(F, make(F, code_of, "small", name), code, 4.0, 1000, 25, s1, harvest=10000)
    assert {k: a[k] for k in COUNTERS} == {k: b[k] for k in COUNTERS} and a["frames_decoded"] == b["frames_decoded"]
    assert s0 == s1 and len(s0) == a["frames"]
    assert "harvest" not in a
    r = restated("small", name, 4.0, 1000)
    HM.assert_equal(b["harvest"], model(code_of, "small", r, frames=a["frames"]), name)


@pytest.mark.parametrize("chunk", [64, 50])
@pytest.mark.parametrize("name", NAMES)
def test_two_ranks_harvest_what_one_does(F, code_of, name, chunk):
    code = code_of("small")[0]
    snr, sigma = F.snr_sigma(4.0, code.rate)
    kw = dict(seed=SEED, first_frame=FIRST, max_frames=1000, max_frame_errors=25, chunk=chunk, device_channel=True,
              random_info=True, info_seed=INFO_SEED)
    s1, s2 = [], []
    single = make(F, code_of, "small", name).ber_sim(snr, sigma, on_frame=lambda *a: s1.append(a), harvest=10000, **kw)
    multi = F.ber_sim_multi([make(F, code_of, "small", name), make(F, code_of, "small", name)], snr, sigma,
                            collective=F.FPLDPC_COLL_HOST, on_frame=lambda *a: s2.append(a), harvest=10000, **kw)
    assert {k: single[k] for k in COUNTERS} == {k: multi[k] for k in COUNTERS} and s1 == s2
    assert multi["collective"] == F.FPLDPC_COLL_HOST and single["frames"] > 2 * chunk
    same_harvest(single["harvest"], multi["harvest"])
    assert single["harvest"].counts["frames"] == single["frames"] and single["harvest"].counts["codeword_errors"] >= 25


def fixed_codeword_case(F, torch_dev, code_of, name, device_channel, encoded, frames=300):
    """One codeword for every frame, all-zero (codeword NULL) or one encoded non-zero word, through the host or the
    device channel; the restatement is that channel, decode_torch and the count at the info positions."""
    import torch
    code, enc, clist = code_of("small")
    snr, sigma = F.snr_sigma(4.0, code.rate)
    if encoded:
        info = F.info_bits(INFO_SEED, 5, 1, enc.k)[0]
        cw = enc.encode(info)[0]
        assert cw.any() and code.syndrome_ok(cw)
    else:
        info, cw = np.zeros(enc.k, np.uint8), None
    if device_channel:
        llr, ovf = F.channel_llr_torch(SEED, FIRST, frames, code.n, snr, sigma,
                                       cw=None if cw is None else torch.from_numpy(cw).to(torch_dev))
        assert int(ovf.cpu()[0]) == 0
    else:
        llr = torch.from_numpy(F.channel_llr(SEED, FIRST, frames, code.n, snr, sigma, cw=cw)).to(torch_dev)
    out = make(F, code_of, "small", name).decode_torch(llr)
    torch.cuda.synchronize()
    hard = F.unpack_hard(out["hard"].cpu().numpy(), code.n)
    blk = (hard[:, enc.info_index] != info).sum(axis=1)
    want = HM.harvest(hard, cw, clist, out["iters"].cpu().numpy(), blk, first_frame=FIRST)
    assert want["counts"]["codeword_errors"] > 0
    res = make(F, code_of, "small", name).ber_sim(
        snr, sigma, info_index=enc.info_index, info_bits=info, codeword=cw, seed=SEED, first_frame=FIRST, max_frames=frames,
        max_frame_errors=0, chunk=CHUNK, device_channel=device_channel, harvest=10000)
    HM.assert_equal(res["harvest"], want, name)
    assert int(res["harvest"].info_errors.sum()) == res["bit_errors"] == int(blk.sum())


def test_host_channel_all_zero_codeword(F, torch_dev, code_of):
    fixed_codeword_case(F, torch_dev, code_of, "flood_minsum", device_channel=False, encoded=False)


def test_device_channel_one_encoded_codeword(F, torch_dev, code_of):
    fixed_codeword_case(F, torch_dev, code_of, "layered_minsum", device_channel=True, encoded=True)


def test_host_channel_one_encoded_codeword(F, torch_dev, code_of):
    """The host channel keeps its codeword on the host: the scan reads the simulation's own device copy of it."""
    fixed_codeword_case(F, torch_dev, code_of, "sxor", device_channel=False, encoded=True)


def test_a(F, code_of, restated):
    """A: 70 hard words with a one-bit tail, 8 syndrome words with an 11-bit tail, four 64-check steps."""
    code = code_of("A")[0]
    r = restated("A", "flood_minsum", 4.5, 500)
    want = model(code_of, "A", r)
    print(want["counts"], want["classes"])
    assert want["counts"]["detected"] > 0
    res = sim(F, make(F, code_of, "A", "flood_minsum"), code, 4.5, 500, 0, harvest=10000)
    hv = res["harvest"]
    assert (hv.hard_words, hv.syn_words) == (70, 8)
    HM.assert_equal(hv, want, "A")
    assert int((hv.info_errors > 0).sum()) == res["frame_errors"] and int(hv.info_errors.sum()) == res["bit_errors"]


def test_argument_rules(F, code_of):
    code = code_of("small")[0]
    other = F.Harvest(F.Code.array(13, 3), 10)      # another m
    backward = F.Harvest(F.Code.array(13, 2, forward=False), 10)  # the same n and m, other check lists
    for name in NAMES:
        dec = make(F, code_of, "small", name)
        for kw in (dict(count_mode=F._lib.FPLDPC_COUNT_ITERS, harvest=10), dict(harvest=other), dict(harvest=backward)):
            with pytest.raises(F.FpldpcError, match="harvest") as e:
                sim(F, dec, code, 4.0, 100, 0, **kw)
            assert e.value.code == -1
    # and a harvest is reusable: cleared when the next simulation starts
    hv = F.Harvest(code, 10000)
    dec = make(F, code_of, "small", "sxor")
    a = sim(F, dec, code, 4.0, 200, 0, harvest=hv)["harvest"]
    first = (a.counts, a.classes, a.frame.copy())
    b = sim(F, dec, code, 4.0, 200, 0, harvest=hv)["harvest"]
    assert b is hv and (b.counts, b.classes) == first[:2] and (b.frame == first[2]).all()
