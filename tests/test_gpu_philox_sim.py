"""The BER simulation on the counter-based noise source (ber_sim(source="philox"), fpldpc_*_ber_sim_source) against
the simulation restated in Python: host information bits, the host encoder, channel_llr_torch(source="philox")
with a codeword per frame (the kernel the simulation runs), decode_torch, numpy's count and the ordered stop rule.
Code.array(13, 2) (n = 169) at 5 dB, 4096 frames from frame 37, the three decoders of
tests/test_gpu_sim_random_info.py.  The result must not depend on the chunk size (64, 96), the number of decoders
(one, two with the host collective) or FPLDPC_SIM_OVERLAP=0; a harvest's frames replay from their frame index
alone; with a bias the weighted sums are the same bits in every variant; the host-channel form decodes the host
twin's LLRs; and the Lehmer source through the *_ber_sim_source entry points equals the entry points without one."""
import ctypes

import numpy as np
import pytest

import harvest_model as HM
import philox_model as PM
import test_gpu_bias_sim as BS
import test_gpu_sim_random_info as RI

pytestmark = pytest.mark.gpu
SEED, INFO_SEED, FIRST, EB, FRAMES, NEED = 2**40 + 7, RI.INFO_SEED, RI.FIRST, 5.0, 4096, 20
NAMES = list(RI.DECODERS)
COUNTERS = RI.COUNTERS
BIAS_POS, SHIFT = [3, 40, 41, 77, 120, 168], 0.5


@pytest.fixture(scope="module")
def small(F):
    code = F.Code.array(13, 2)
    assert code.n == 169
    return code, F.Encoder.from_code(code), code.lists()[3]


def make(F, small, name):
    cls, kw = RI.DECODERS[name]
    return getattr(F, cls)(small[0], max_iter=RI.MAX_ITER, **kw)


@pytest.fixture(scope="module")
def restated(F, torch_dev, small):
    """(hard, cw, blkerror, iterations, logw) of frames FIRST .. FIRST + FRAMES - 1 on the Philox channel, shifted by
    `bias` where there is one; computed once per decoder and bias."""
    import torch
    made = {}

    def get(name, bias=None):
        key = (name, bias is not None)
        if key not in made:
            code, enc, _ = small
            snr, sigma = F.snr_sigma(EB, code.rate)
            info = F.info_bits(INFO_SEED, FIRST, FRAMES, enc.k)
            cw = enc.encode(info)
            cw_t = torch.from_numpy(cw).to(torch_dev)
            if bias is None:
                llr, ovf = F.channel_llr_torch(SEED, FIRST, FRAMES, code.n, snr, sigma, 4, cw=cw_t, source="philox")
                logw = np.zeros(FRAMES)
            else:
                llr, lw, ovf = F.channel_llr_biased_torch(bias, SEED, FIRST, FRAMES, snr, sigma, 4, cw=cw_t, source="philox")
                logw = lw.cpu().numpy()
            out = make(F, small, name).decode_torch(llr)
            torch.cuda.synchronize()
            assert int(ovf.cpu()[0]) == 0
            hard = F.unpack_hard(out["hard"].cpu().numpy(), code.n)
            blk = (hard[:, enc.info_index] != info).sum(axis=1)
            assert (blk > 0).sum() > NEED  # the stop rule has something to stop at
            made[key] = (hard, cw, blk, out["iters"].cpu().numpy(), logw)
        return made[key]
    return get


@pytest.fixture(scope="module")
def bias(F, small):
    return F.Bias(small[0].n, BIAS_POS, SHIFT)


def variants(F, small, name, monkeypatch, need, **extra):
    """(label, result, on_frame sequence) of the same simulation run every way it can be run."""
    code = small[0]
    snr, sigma = F.snr_sigma(EB, code.rate)
    kw = dict(seed=SEED, first_frame=FIRST, max_frames=FRAMES, max_frame_errors=need, device_channel=True, random_info=True,
              info_seed=INFO_SEED, source="philox", **extra)
    for label, chunk, ranks, overlap in (("chunk 64", 64, 1, True), ("chunk 96", 96, 1, True), ("two ranks", 64, 2, True),
                                         ("one chunk at a time", 64, 1, False)):
        seen = []
        with monkeypatch.context() as m:
            if not overlap:
                m.setenv("FPLDPC_SIM_OVERLAP", "0")
            if ranks == 1:
                r = make(F, small, name).ber_sim(snr, sigma, chunk=chunk, on_frame=lambda *a: seen.append(a), **kw)
            else:
                r = F.ber_sim_multi([make(F, small, name) for _ in range(ranks)], snr, sigma, collective=F.FPLDPC_COLL_HOST,
                                    chunk=chunk, on_frame=lambda *a: seen.append(a), **kw)
                assert r["collective"] == F.FPLDPC_COLL_HOST
        yield label, r, seen


@pytest.mark.parametrize("need", [0, NEED])
@pytest.mark.parametrize("name", NAMES)
def test_simulation_equals_its_restatement(F, small, restated, name, need, monkeypatch):
    _, _, blk, its, _ = restated(name)
    want, seq = RI.ordered(blk, its, need)
    assert want["frame_errors"] == (need or want["frame_errors"]) and (need == 0 or 128 < want["frames"] < FRAMES)
    for label, r, seen in variants(F, small, name, monkeypatch, need):
        print(name, label, {k: r[k] for k in COUNTERS})
        assert {k: r[k] for k in COUNTERS} == want, label
        assert seen == seq, label  # the stop lands on the same frame


@pytest.mark.parametrize("name", NAMES)
def test_harvest_replays_from_the_frame_index(F, torch_dev, small, restated, name, monkeypatch):
    import torch
    code, enc, clist = small
    hard, cw, blk, its, _ = restated(name)
    stop = RI.ordered(blk, its, NEED)[0]["frames"]
    want = HM.harvest(hard[:stop], cw[:stop], clist, its[:stop], blk[:stop], first_frame=FIRST)
    first = None
    for label, r, _ in variants(F, small, name, monkeypatch, NEED, harvest=10000):
        HM.assert_equal(r["harvest"], want, (name, label))
        first = first or r["harvest"]
    # a record's frame index is enough: its bits, its codeword, its noise, its decode
    snr, sigma = F.snr_sigma(EB, code.rate)
    dec = make(F, small, name)
    assert first.counts["recorded"] >= NEED
    for i in range(0, first.counts["recorded"], 7):
        f = int(first.frame[i])
        info = F.info_bits(INFO_SEED, f, 1, enc.k)
        word = enc.encode(info)
        llr, _ = F.channel_llr_torch(SEED, f, 1, code.n, snr, sigma, 4, cw=torch.from_numpy(word).to(torch_dev), source="philox")
        out = dec.decode_torch(llr)
        torch.cuda.synchronize()
        again = F.unpack_hard(out["hard"].cpu().numpy(), code.n)[0]
        assert (np.nonzero(again ^ word[0])[0] == first.error_positions(i)).all()
        assert int(out["iters"].cpu()[0]) == first.iters[i]


@pytest.mark.parametrize("name", NAMES)
def test_weighted_sums_are_the_same_bits(F, small, restated, bias, name, monkeypatch):
    _, _, blk, its, logw = restated(name, bias)
    for need in (0, NEED):
        want, seq = RI.ordered(blk, its, need)
        sums = None
        for label, r, seen in variants(F, small, name, monkeypatch, need, bias=bias):
            assert {k: r[k] for k in COUNTERS} == want and seen == seq and r["bias"] is bias, label
            sums = sums or bias.sums
            assert bias.sums == sums, label  # bit for bit: python floats compare exactly
        BS.assert_sums(sums, BS.sums_of(blk, logw, want["frames"]))
    # and with a harvest beside the bias
    code, _, clist = small
    hard, cw = restated(name, bias)[:2]
    stop = want["frames"]
    for label, r, _ in variants(F, small, name, monkeypatch, NEED, bias=bias, harvest=10000):
        assert bias.sums == sums, label
        HM.assert_equal(r["harvest"], HM.harvest(hard[:stop], cw[:stop], clist, its[:stop], blk[:stop], first_frame=FIRST), label)
        break


@pytest.mark.parametrize("name", NAMES)
def test_host_channel_form(F, torch_dev, small, name):
    """device_channel = 0: one fixed codeword, forced positions, the LLRs of the host twin."""
    import torch
    code, enc, _ = small
    snr, sigma = F.snr_sigma(EB, code.rate)
    frames = 1000
    info = F.info_bits(INFO_SEED, 5, 1, enc.k)[0]
    cw = enc.encode(info[None])[0]
    forced = [int(x) for x in np.nonzero(cw == 0)[0][[0, 7]]]
    llr = F.channel_llr(SEED, FIRST, frames, code.n, snr, sigma, 4, cw, np.int16, source="philox")
    llr[:, forced] = 100
    out = make(F, small, name).decode_torch(torch.from_numpy(llr).to(torch_dev))
    torch.cuda.synchronize()
    hard = F.unpack_hard(out["hard"].cpu().numpy(), code.n)
    blk, its = (hard[:, enc.info_index] != info).sum(axis=1), out["iters"].cpu().numpy()
    assert (blk > 0).sum() > 3
    for need in (0, 3):
        want, seq = RI.ordered(blk, its, need)
        for chunk, ranks in ((64, 1), (96, 2)):
            seen = []
            kw = dict(info_index=enc.info_index, info_bits=info, codeword=cw, seed=SEED, first_frame=FIRST, max_frames=frames,
                      max_frame_errors=need, chunk=chunk, device_channel=False, forced_index=forced, forced_llr=100,
                      source="philox", on_frame=lambda *a: seen.append(a))
            if ranks == 1:
                r = make(F, small, name).ber_sim(snr, sigma, **kw)
            else:
                r = F.ber_sim_multi([make(F, small, name), make(F, small, name)], snr, sigma, collective=F.FPLDPC_COLL_HOST, **kw)
            assert {k: r[k] for k in COUNTERS} == want and seen == seq, (need, chunk, ranks)
    # the device channel on the same fixed codeword gives the host twin's frames too (off the boundary positions,
    # of which these 169,000 values have none: tests/philox_model.py, checked on the model)
    model = PM.channel(SEED, FIRST, frames, code.n, snr, sigma, 4, cw)
    assert not PM.boundary(model["x"], snr, sigma, 4).any()
    r = make(F, small, name).ber_sim(snr, sigma, info_index=enc.info_index, info_bits=info, codeword=cw, seed=SEED,
                                     first_frame=FIRST, max_frames=frames, max_frame_errors=0, chunk=64, device_channel=True,
                                     forced_index=forced, forced_llr=100, source="philox")
    assert {k: r[k] for k in COUNTERS} == RI.ordered(blk, its, 0)[0]


def source_call(F, decs, source, bias, harvest, snr, sigma, **kw):
    """<family>_ber_sim_source directly: (result fields, collective used)."""
    p, keep = F._lib.sim_params(snr, sigma, **kw)
    hs = (ctypes.c_void_p * len(decs))(*[d._h for d in decs])
    r, used = F._lib.SimResult(), ctypes.c_int32(0)
    if harvest is not None:
        harvest._refresh()
    st = decs[0]._fn("ber_sim_source")(hs, len(decs), ctypes.byref(p), F.FPLDPC_COLL_HOST, source,
                                       bias._h if bias is not None else None, harvest._h if harvest is not None else None,
                                       ctypes.byref(r), ctypes.byref(used))
    del keep
    return st, {k: getattr(r, k) for k, _ in F._lib.SimResult._fields_ if k != "seconds"}, used.value


@pytest.mark.parametrize("name", NAMES)
def test_lehmer_through_the_source_entry_points(F, small, bias, name):
    code, enc, _ = small
    snr, sigma = F.snr_sigma(EB, code.rate)
    kw = dict(seed=123456789, first_frame=FIRST, max_frames=FRAMES, max_frame_errors=10, chunk=64, device_channel=True,
              random_info=True, info_seed=INFO_SEED)
    fields = lambda r: {k: v for k, v in r.items() if k in COUNTERS + ("frames_decoded",)}
    L = F.FPLDPC_NOISE_LEHMER
    plain = make(F, small, name).ber_sim(snr, sigma, **kw)
    st, got, used = source_call(F, [make(F, small, name)], L, None, None, snr, sigma, **kw)
    assert st == 0 and fields(got) == fields(plain) and used == F.FPLDPC_COLL_HOST and plain["frame_errors"] == 10
    want = make(F, small, name).ber_sim(snr, sigma, harvest=10000, **kw)
    hv = F.Harvest(code, 10000)
    st, got, _ = source_call(F, [make(F, small, name)], L, None, hv, snr, sigma, **kw)
    assert st == 0 and fields(got) == fields(want)
    assert hv.counts == want["harvest"].counts and hv.classes == want["harvest"].classes
    for k in HM.FIELDS:
        assert (getattr(hv, k) == getattr(want["harvest"], k)).all(), k
    want = make(F, small, name).ber_sim(snr, sigma, bias=bias, **kw)
    sums = bias.sums
    st, got, _ = source_call(F, [make(F, small, name)], L, bias, None, snr, sigma, **kw)
    assert st == 0 and fields(got) == fields(want) and bias.sums == sums
    # the host channel too
    info = F.info_bits(INFO_SEED, 5, 1, enc.k)[0]
    hk = dict(info_index=enc.info_index, info_bits=info, codeword=enc.encode(info[None])[0], seed=123456789, first_frame=FIRST,
              max_frames=300, max_frame_errors=0, chunk=64, device_channel=False)
    want = make(F, small, name).ber_sim(snr, sigma, **hk)
    st, got, _ = source_call(F, [make(F, small, name)], L, None, None, snr, sigma, **hk)
    assert st == 0 and fields(got) == fields(want)


def test_argument_rules(F, small, bias):
    code, enc, _ = small
    snr, sigma = F.snr_sigma(EB, code.rate)
    kw = dict(first_frame=FIRST, max_frames=100, max_frame_errors=0, chunk=64, device_channel=True, random_info=True,
              info_seed=INFO_SEED)
    for name in NAMES:
        dec = make(F, small, name)
        st, _, _ = source_call(F, [dec], 2, None, None, snr, sigma, seed=1, **kw)
        assert st == -1 and b"source" in F.lib().fpldpc_last_error()
        st, _, _ = source_call(F, [dec], F.FPLDPC_NOISE_PHILOX, None, None, snr, sigma, seed=-1, **kw)
        assert st == -1 and b"philox" in F.lib().fpldpc_last_error()
        with pytest.raises(ValueError):
            dec.ber_sim(snr, sigma, seed=1, source="ranlux", **kw)
        with pytest.raises(ValueError):
            F.ber_sim_multi([dec], snr, sigma, seed=1, source=None, **kw)
        # seed 0 and a first frame beyond the Lehmer stream's 2^48 draws are Philox's to take
        # (on the all-zero codeword: random_info's information bits stay on their Lehmer stream and its limit)
        r = dec.ber_sim(snr, sigma, seed=0, source="philox", info_index=enc.info_index, info_bits=np.zeros(enc.k, np.uint8),
                        first_frame=2**50, max_frames=100, max_frame_errors=0, chunk=64, device_channel=True)
        assert r["frames"] == 100
        # a bias keeps its rules on either source
        with pytest.raises(F.FpldpcError, match="device_channel"):
            dec.ber_sim(snr, sigma, info_index=enc.info_index, info_bits=np.zeros(enc.k, np.uint8), seed=1, first_frame=FIRST,
                        max_frames=100, chunk=64, device_channel=False, bias=bias, source="philox")
