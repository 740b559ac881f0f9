"""A codeword per frame in the BER simulation (fpldpc_sim_params.random_info): the information-bit stream on
the device against the host's, and the whole pipeline restated in Python -- host information bits, the host
encoder, the device channel with a codeword per frame (the kernel the simulation runs, so the LLRs are
identical), decode_torch, numpy's count of the hard decisions at the encoder's info positions, the ordered stop
rule -- against ber_sim(random_info=True).

Eb/N0 (numpy models, all-zero codeword, max_iter 7): p = 13, r = 2 at 4.0 dB has 12 % .. 17 % frame errors;
A at 4.5 dB has 4 % (flooding min-sum), 20 % (flooding sxor) and 54 % (layered min-sum at 10 / 8 bits); at 8 dB
no model sees a frame error in 256 frames."""
import numpy as np
import pytest

from test_gpu_layered_sat import small_code

pytestmark = pytest.mark.gpu
SEED, INFO_SEED = 123456789, 24681357
FIRST, CHUNK, NEED, MAX_ITER = 37, 64, 10, 7
MS = dict(post_bits=10, msg_bits=8, scale_16=13, offset=3)
DECODERS = {
    "sxor": ("Decoder", {}),
    "flood_minsum": ("MinSumDecoder", MS),
    "layered_minsum": ("LayeredDecoder", dict(check="minsum", **MS)),
}
# code -> (frames, Eb/N0)
SHAPES = {"small": (1000, 4.0), "A": (500, 4.5)}
COUNTERS = ("bit_errors", "frame_errors", "frames", "iter_sum")


@pytest.fixture(scope="module")
def code_of(F):
    made = {}

    def get(which):
        if which not in made:
            code = F.Code.array(47, 5) if which == "A" else small_code(F, "array13x2")[0]
            made[which] = (code, F.Encoder.from_code(code))
        return made[which]
    return get


def make(F, code_of, which, name):
    cls, kw = DECODERS[name]
    return getattr(F, cls)(code_of(which)[0], max_iter=MAX_ITER, **kw)


@pytest.mark.parametrize("seed,first,frames,k", [(987654321, 37, 64, 144), (INFO_SEED, 37, 64, 1978), (5, 0, 7, 13),
                                                 (77, 1000003, 3, 1), (2**31 - 2, 2**30, 5, 1978), (9, 12, 1, 15),
                                                 (9, 12, 1, 16), (9, 12, 1, 17)])
def test_device_stream_equals_the_hosts(F, torch_dev, seed, first, frames, k):
    """Whole runs of 16 draws, a last run cut short (7 * 13 = 91, 15, 17 bits), k = 1, frames far into the stream."""
    import torch
    out = torch.full((frames * k + 64,), 0xAA, dtype=torch.uint8, device=torch_dev)
    F.info_bits_ptrs(seed, first, frames, k, out.data_ptr(), torch.cuda.current_stream(torch_dev).cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[frames * k:] == 0xAA).all()  # nothing past the last bit
    assert (got[:frames * k].reshape(frames, k) == F.info_bits(seed, first, frames, k)).all()


def ordered(blk, its, need):
    fe = np.cumsum(blk > 0)
    stop = len(blk) if need <= 0 or fe[-1] < need else int(np.argmax(fe >= need)) + 1
    b, i = blk[:stop].astype(np.int64), its[:stop].astype(np.int64)
    res = dict(bit_errors=int(b.sum()), frame_errors=int((b > 0).sum()), frames=stop, iter_sum=int(i.sum()))
    return res, [(FIRST + f, int(i[f]), int(b[f])) for f in range(stop)]


def restated(F, dev, dec, code, enc, eb, frames, info_seed=INFO_SEED):
    """(blkerror, iterations) of frames FIRST .. FIRST + frames - 1, each sent with its own information bits."""
    import torch
    snr, sigma = F.snr_sigma(eb, code.rate)
    info = F.info_bits(info_seed, FIRST, frames, enc.k)
    cw = enc.encode(info)
    assert all(code.syndrome_ok(c) for c in cw)  # codewords, every one
    assert (info[:CHUNK] != info[0]).any() and (cw[:CHUNK] != cw[0]).any()  # and not one codeword
    cw_t = torch.from_numpy(cw).to(dev)
    llr = torch.empty((frames, code.n), dtype=torch.int16, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    F.channel_llr_ptrs(SEED, FIRST, frames, code.n, snr, sigma, 4, cw_t.data_ptr(), 1, llr.data_ptr(), F.FPLDPC_LLR_I16,
                       ovf.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    out = dec.decode_torch(llr)
    torch.cuda.synchronize()
    assert int(ovf.cpu()[0]) == 0
    hard = F.unpack_hard(out["hard"].cpu().numpy(), code.n)
    blk = (hard[:, enc.info_index] != info).sum(axis=1)
    return blk, out["iters"].cpu().numpy()


def sim(F, dec, code, eb, frames, need, seen=None, info_seed=INFO_SEED, **kw):
    snr, sigma = F.snr_sigma(eb, code.rate)
    args = dict(seed=SEED, first_frame=FIRST, max_frames=frames, max_frame_errors=need, chunk=CHUNK, device_channel=True,
                random_info=True, info_seed=info_seed)
    args.update(kw)
    return dec.ber_sim(snr, sigma, on_frame=None if seen is None else (lambda *a: seen.append(a)), **args)


@pytest.mark.parametrize("name", list(DECODERS))
@pytest.mark.parametrize("which", list(SHAPES))
def test_pipeline_equals_its_restatement(F, torch_dev, code_of, which, name):
    code, enc = code_of(which)
    frames, eb = SHAPES[which]
    blk, its = restated(F, torch_dev, make(F, code_of, which, name), code, enc, eb, frames)
    want, seq = ordered(blk, its, NEED)
    assert want["frame_errors"] > 0  # the count has something to count
    seen = []
    r = sim(F, make(F, code_of, which, name), code, eb, frames, NEED, seen)
    print(which, name, {k: r[k] for k in COUNTERS}, "restated", want)
    assert {k: r[k] for k in COUNTERS} == want
    assert seen == seq
    if name == "flood_minsum":  # every frame; one chunk at a time; the iteration count as blkerror
        want, seq = ordered(blk, its, 0)
        seen = []
        r = sim(F, make(F, code_of, which, name), code, eb, frames, 0, seen)
        assert {k: r[k] for k in COUNTERS} == want and seen == seq and r["frames"] == frames
        r = sim(F, make(F, code_of, which, name), code, eb, frames, 0, count_mode=F._lib.FPLDPC_COUNT_ITERS)
        assert r["bit_errors"] == r["iter_sum"] == int(its.sum())


@pytest.mark.parametrize("name", list(DECODERS))
def test_one_chunk_at_a_time(F, torch_dev, code_of, name, monkeypatch):
    code, enc = code_of("small")
    blk, its = restated(F, torch_dev, make(F, code_of, "small", name), code, enc, 4.0, 300)
    monkeypatch.setenv("FPLDPC_SIM_OVERLAP", "0")
    seen = []
    r = sim(F, make(F, code_of, "small", name), code, 4.0, 300, NEED, seen)
    want, seq = ordered(blk, its, NEED)
    assert {k: r[k] for k in COUNTERS} == want and seen == seq


@pytest.mark.parametrize("name", list(DECODERS))
@pytest.mark.parametrize("which", list(SHAPES))
def test_noise_free(F, torch_dev, code_of, which, name):
    """At 8 dB nothing is in error: a count against the wrong positions or the wrong frame's bits fails on every
    frame (half the compared bits differ)."""
    code, enc = code_of(which)
    blk, _ = restated(F, torch_dev, make(F, code_of, which, name), code, enc, 8.0, 256)
    assert (blk == 0).all()
    r = sim(F, make(F, code_of, which, name), code, 8.0, 256, NEED)
    assert r["bit_errors"] == 0 and r["frame_errors"] == 0 and r["frames"] == 256


def test_argument_rules(F, code_of):
    code, enc = code_of("small")
    dec = make(F, code_of, "small", "flood_minsum")
    zeros = np.zeros(enc.k, np.uint8)
    for kw, rule in [(dict(device_channel=False), "device_channel"),
                     (dict(codeword=np.zeros(code.n, np.uint8)), "codeword"),
                     (dict(info_index=enc.info_index, info_bits=zeros), "info_index"),
                     (dict(forced_index=[0, 1], forced_llr=100), "forced"),
                     (dict(info_seed=0), "info_seed"), (dict(info_seed=2**31 - 1), "info_seed")]:
        for d in (dec, make(F, code_of, "small", "sxor")):
            with pytest.raises(F.FpldpcError, match=rule) as e:
                sim(F, d, code, 4.0, 100, NEED, **kw)
            assert e.value.code == -1 and "random_info" in str(e.value)


@pytest.mark.parametrize("name", list(DECODERS))
def test_random_info_off_ignores_the_seed(F, code_of, name):
    code, enc = code_of("small")
    snr, sigma = F.snr_sigma(4.0, code.rate)
    kw = dict(info_index=enc.info_index, info_bits=np.zeros(enc.k, np.uint8), seed=SEED, first_frame=FIRST,
              max_frames=300, max_frame_errors=NEED, chunk=CHUNK, device_channel=True)
    a = make(F, code_of, "small", name).ber_sim(snr, sigma, **kw)
    b = make(F, code_of, "small", name).ber_sim(snr, sigma, random_info=False, info_seed=12345, **kw)
    assert {k: a[k] for k in COUNTERS} == {k: b[k] for k in COUNTERS} and a["frame_errors"] > 0


def test_seeds_are_independent_streams(F, code_of):
    """Another info_seed sends other codewords through the same noise: other counters (on this code at this
    Eb/N0 over 1000 frames), the same number of frames."""
    code, _ = code_of("small")
    a = sim(F, make(F, code_of, "small", "sxor"), code, 4.0, 1000, 0)
    b = sim(F, make(F, code_of, "small", "sxor"), code, 4.0, 1000, 0, info_seed=INFO_SEED + 1)
    assert a["frames"] == b["frames"] == 1000 and a["frame_errors"] > 0 and b["frame_errors"] > 0
    assert (a["bit_errors"], a["iter_sum"]) != (b["bit_errors"], b["iter_sum"])


@pytest.mark.parametrize("chunk", [64, 50])
@pytest.mark.parametrize("name", list(DECODERS))
def test_multi_equals_single(F, code_of, name, chunk):
    code, _ = code_of("small")
    snr, sigma = F.snr_sigma(4.0, code.rate)
    kw = dict(seed=SEED, first_frame=FIRST, max_frames=1000, max_frame_errors=25, chunk=chunk, device_channel=True,
              random_info=True, info_seed=INFO_SEED)
    s1, s2 = [], []
    single = make(F, code_of, "small", name).ber_sim(snr, sigma, on_frame=lambda *a: s1.append(a), **kw)
    multi = F.ber_sim_multi([make(F, code_of, "small", name), make(F, code_of, "small", name)], snr, sigma,
                            collective=F.FPLDPC_COLL_HOST, on_frame=lambda *a: s2.append(a), **kw)
    assert {k: single[k] for k in COUNTERS} == {k: multi[k] for k in COUNTERS} and s1 == s2
    assert single["frame_errors"] == 25 and single["frames"] > 2 * chunk
