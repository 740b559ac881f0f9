"""The BER simulation on the shifted channel (ber_sim(bias=...), fpldpc_*_ber_sim_biased) against the simulation
restated in Python: tests/test_gpu_sim_random_info.py's restatement (host information bits, the host encoder,
decode_torch, numpy's count, the ordered stop rule) with channel_llr_biased_torch in place of the channel, and
numpy's accumulation of the weighted sums in frame order.  p = 13, r = 2 at 4.0 dB, max_iter 7, first_frame 37,
chunks of 64, the three decoders of that file.  The bias, shift 0.5, lies on the support of a low-weight
undetected error that a plain harvest of the flooding sxor decoder's restatement finds."""
import math

import numpy as np
import pytest

import harvest_model as HM
import test_gpu_sim_random_info as RI
from test_gpu_layered_sat import small_code

pytestmark = pytest.mark.gpu
SEED, INFO_SEED, FIRST, CHUNK = RI.SEED, RI.INFO_SEED, RI.FIRST, RI.CHUNK
NAMES = list(RI.DECODERS)
COUNTERS = RI.COUNTERS
EB, FRAMES, SHIFT = 4.0, 1000, 0.5
FLOATS = ("sum_w", "sum_w2", "sum_w_fe", "sum_w2_fe", "sum_w_be", "min_logw", "max_logw")


@pytest.fixture(scope="module")
def small(F):
    code = small_code(F, "array13x2")[0]
    return code, F.Encoder.from_code(code), code.lists()[3]


def make(F, small, name):
    cls, kw = RI.DECODERS[name]
    return getattr(F, cls)(small[0], max_iter=RI.MAX_ITER, **kw)


def sent(F, small, mode, frames):
    """(info, cw): a codeword per frame ("random"), one encoded word ("fixed") or the all-zero one ("zero")."""
    _, enc, _ = small
    if mode == "random":
        info = F.info_bits(INFO_SEED, FIRST, frames, enc.k)
        return info, enc.encode(info)
    if mode == "fixed":
        info = F.info_bits(INFO_SEED, 5, 1, enc.k)[0]
        return info, enc.encode(info[None])[0]
    return np.zeros(enc.k, np.uint8), None


@pytest.fixture(scope="module")
def restated(F, torch_dev, small):
    """(hard, cw, blkerror, iterations, logw) of frames FIRST .. FIRST + frames - 1 on the channel shifted by `bias`
    (None: the plain channel, logw 0); computed once per key."""
    import torch
    made = {}

    def get(name, bias, key, mode="random", frames=FRAMES):
        k = (name, key, mode, frames)
        if k not in made:
            code, enc, _ = small
            snr, sigma = F.snr_sigma(EB, code.rate)
            info, cw = sent(F, small, mode, frames)
            cw_t = None if cw is None else torch.from_numpy(cw).to(torch_dev)
            b = bias if bias is not None else F.Bias(code.n, [], [])
            llr, logw, ovf = F.channel_llr_biased_torch(b, SEED, FIRST, frames, snr, sigma, 4, cw=cw_t, device=torch_dev)
            out = make(F, small, name).decode_torch(llr)
            torch.cuda.synchronize()
            assert int(ovf.cpu()[0]) == 0
            hard = F.unpack_hard(out["hard"].cpu().numpy(), code.n)
            blk = (hard[:, enc.info_index] != info).sum(axis=1)
            made[k] = (hard, cw, blk, out["iters"].cpu().numpy(), logw.cpu().numpy())
        return made[k]
    return get


@pytest.fixture(scope="module")
def bias(F, small, restated):
    """On the support of the lowest-weight undetected error of the plain restatement, the first such record."""
    code, _, clist = small
    hard, cw, blk, its, _ = restated("sxor", None, "plain")
    want = HM.harvest(hard, cw, clist, its, blk, first_frame=FIRST)
    rec = want["records"]
    undetected = np.nonzero(rec["unsat"] == 0)[0]
    assert len(undetected) > 0  # the harvest found one, on the restatement alone
    i = undetected[np.argmin(rec["weight"][undetected])]
    assert rec["weight"][i] <= 12
    pos = np.nonzero(F.unpack_hard(rec["err"][i:i + 1], code.n)[0])[0]
    assert len(pos) == rec["weight"][i]
    print("bias on", pos.tolist())
    return F.Bias(code.n, pos, SHIFT)


def sums_of(blk, logw, stop):
    """numpy's accumulation in frame order over the first `stop` frames."""
    b, lw = blk[:stop].astype(np.int64), logw[:stop]
    w = np.exp(lw)
    fe = (b > 0).astype(np.float64)
    seq = lambda x: float(np.cumsum(x)[-1])  # one addition per frame, in order
    return dict(frames=stop, frame_errors=int((b > 0).sum()), bit_errors=int(b.sum()), sum_w=seq(w), sum_w2=seq(w * w),
                sum_w_fe=seq(w * fe), sum_w2_fe=seq(w * w * fe), sum_w_be=seq(w * b), min_logw=float(lw.min()),
                max_logw=float(lw.max()))


def assert_sums(got, want):
    for k in ("frames", "frame_errors", "bit_errors"):
        assert got[k] == want[k], (k, got, want)
    for k in FLOATS:  # host exp against numpy's: an ulp per frame, 1e-13 over a thousand frames
        assert abs(got[k] - want[k]) <= 1e-10 * abs(want[k]), (k, got[k], want[k])


def sim(F, dec, code, need, seen=None, frames=FRAMES, **kw):
    return RI.sim(F, dec, code, EB, frames, need, seen, **kw)


def inner_limit(blk):
    """A frame-error limit whose stop frame lies inside a chunk of round >= 2 with a further chunk in flight."""
    need = int((blk[:2 * CHUNK + 10] > 0).sum()) + 1
    stop = RI.ordered(blk, blk, need)[0]["frames"]
    assert 2 * CHUNK < stop < len(blk) - 2 * CHUNK and stop % CHUNK != 0
    return need, stop


@pytest.mark.parametrize("name", NAMES)
def test_simulation_equals_its_restatement(F, small, restated, bias, name):
    code = small[0]
    _, _, blk, its, logw = restated(name, bias, "bias")
    plain_blk = restated(name, None, "plain")[2]
    assert (blk > 0).sum() > (plain_blk > 0).sum() > 0  # the shift costs frames
    for need in (0, inner_limit(blk)[0]):
        want, seq = RI.ordered(blk, its, need)
        seen = []
        r = sim(F, make(F, small, name), code, need, seen, bias=bias)
        print(name, need, {k: r[k] for k in COUNTERS}, r["bias"].estimate(k=small[1].k))
        assert {k: r[k] for k in COUNTERS} == want and seen == seq
        assert r["bias"] is bias and (need == 0 or r["frames_decoded"] > r["frames"])
        assert_sums(bias.sums, sums_of(blk, logw, want["frames"]))
        est, s = bias.estimate(k=small[1].k), bias.sums
        assert est["fer"] == s["sum_w_fe"] / s["frames"] and est["ess"] == s["sum_w"] ** 2 / s["sum_w2"]
        assert est["ber"] == s["sum_w_be"] / (s["frames"] * small[1].k)
        assert est["fer_se"] == math.sqrt(max(s["sum_w2_fe"] / s["frames"] - est["fer"] ** 2, 0) / s["frames"])


@pytest.mark.parametrize("name", NAMES)
def test_sums_depend_on_neither_chunks_nor_ranks(F, small, restated, bias, name, monkeypatch):
    code = small[0]
    need, stop = inner_limit(restated(name, bias, "bias")[2])
    snr, sigma = F.snr_sigma(EB, code.rate)
    kw = dict(seed=SEED, first_frame=FIRST, max_frames=FRAMES, max_frame_errors=need, device_channel=True,
              random_info=True, info_seed=INFO_SEED)
    base = make(F, small, name).ber_sim(snr, sigma, chunk=CHUNK, bias=bias, **kw)
    first = bias.sums
    assert first["frames"] == stop == base["frames"]
    r = make(F, small, name).ber_sim(snr, sigma, chunk=96, bias=bias, **kw)
    assert bias.sums == first and {k: r[k] for k in COUNTERS} == {k: base[k] for k in COUNTERS}
    r = F.ber_sim_multi([make(F, small, name), make(F, small, name)], snr, sigma, collective=F.FPLDPC_COLL_HOST, chunk=CHUNK,
                        bias=bias, **kw)
    assert bias.sums == first and {k: r[k] for k in COUNTERS} == {k: base[k] for k in COUNTERS}
    assert r["collective"] == F.FPLDPC_COLL_HOST and r["bias"] is bias
    monkeypatch.setenv("FPLDPC_SIM_OVERLAP", "0")
    r = make(F, small, name).ber_sim(snr, sigma, chunk=CHUNK, bias=bias, **kw)
    assert bias.sums == first and {k: r[k] for k in COUNTERS} == {k: base[k] for k in COUNTERS}


@pytest.mark.parametrize("name", NAMES)
def test_with_a_harvest(F, small, restated, bias, name):
    code, _, clist = small
    hard, cw, blk, its, logw = restated(name, bias, "bias")
    need, stop = inner_limit(blk)
    sim(F, make(F, small, name), code, need, bias=bias)
    alone = bias.sums
    seen = []
    r = sim(F, make(F, small, name), code, need, seen, bias=bias, harvest=10000)
    assert bias.sums == alone and seen == RI.ordered(blk, its, need)[1]
    HM.assert_equal(r["harvest"], HM.harvest(hard[:stop], cw[:stop], clist, its[:stop], blk[:stop], first_frame=FIRST), name)
    # and from a record to the next bias
    hv = r["harvest"]
    nxt = F.Bias.from_harvest(hv, 0, 0.25)
    assert nxt.n == code.n and nxt.count == hv.weight[0] and (nxt.shifts == 0.25).all()
    assert (nxt.positions == hv.error_positions(0)).all()
    multi = F.ber_sim_multi([make(F, small, name), make(F, small, name)], *F.snr_sigma(EB, code.rate),
                            collective=F.FPLDPC_COLL_HOST, seed=SEED, first_frame=FIRST, max_frames=FRAMES,
                            max_frame_errors=need, chunk=CHUNK, device_channel=True, random_info=True, info_seed=INFO_SEED,
                            bias=bias, harvest=10000)
    assert bias.sums == alone and multi["harvest"].counts == r["harvest"].counts


@pytest.mark.parametrize("mode", ["fixed", "zero"])
@pytest.mark.parametrize("name", NAMES)
def test_other_codewords(F, small, restated, bias, name, mode):
    """One encoded codeword for every frame, and the all-zero one, without random_info."""
    code, enc, _ = small
    frames = 300
    info, cw = sent(F, small, mode, frames)
    _, _, blk, its, logw = restated(name, bias, "bias", mode, frames)
    want, seq = RI.ordered(blk, its, 0)
    assert want["frame_errors"] > 0
    snr, sigma = F.snr_sigma(EB, code.rate)
    seen = []
    r = make(F, small, name).ber_sim(snr, sigma, info_index=enc.info_index, info_bits=info, codeword=cw, seed=SEED,
                                     first_frame=FIRST, max_frames=frames, max_frame_errors=0, chunk=CHUNK,
                                     device_channel=True, bias=bias, on_frame=lambda *a: seen.append(a))
    assert {k: r[k] for k in COUNTERS} == want and seen == seq
    assert_sums(bias.sums, sums_of(blk, logw, frames))


@pytest.mark.parametrize("name", NAMES)
def test_zero_shift_and_no_side_effects(F, small, bias, name):
    """A bias of shift 0.0 is the plain simulation with unit weights; and a plain simulation returns the same
    before and after a biased one on the same decoder."""
    code = small[0]
    need = 25
    keys = COUNTERS + ("frames_decoded",)
    dec = make(F, small, name)
    before = sim(F, dec, code, need)
    zero = F.Bias(code.n, bias.positions, 0.0)
    r = sim(F, dec, code, need, bias=zero)
    assert {k: r[k] for k in keys} == {k: before[k] for k in keys}
    s = zero.sums
    assert s["sum_w"] == s["frames"] == r["frames"] and s["sum_w_fe"] == s["frame_errors"] == r["frame_errors"]
    assert s["sum_w_be"] == s["bit_errors"] == r["bit_errors"] and s["min_logw"] == s["max_logw"] == 0.0
    shifted = sim(F, dec, code, need, bias=bias)
    assert {k: shifted[k] for k in COUNTERS} != {k: before[k] for k in COUNTERS}
    after = sim(F, dec, code, need)
    assert {k: after[k] for k in keys} == {k: before[k] for k in keys} and "bias" not in after


def test_argument_rules(F, small, bias):
    code, enc, _ = small
    snr, sigma = F.snr_sigma(EB, code.rate)
    zeros = np.zeros(enc.k, np.uint8)
    fixed = dict(info_index=enc.info_index, info_bits=zeros, seed=SEED, first_frame=FIRST, max_frames=100, chunk=CHUNK)
    other = F.Bias(code.n + 1, bias.positions, SHIFT)
    outside = int(np.setdiff1d(np.arange(code.n), bias.positions)[0])
    for name in NAMES:
        dec = make(F, small, name)
        for kw, rule in [(dict(device_channel=False, bias=bias), "device_channel"),
                         (dict(device_channel=True, count_mode=F._lib.FPLDPC_COUNT_ITERS, bias=bias), "count_mode"),
                         (dict(device_channel=True, forced_index=[outside, int(bias.positions[-1])], forced_llr=100, bias=bias),
                          "forced position"),
                         (dict(device_channel=True, bias=other), "another n")]:
            with pytest.raises(F.FpldpcError, match=rule) as e:
                dec.ber_sim(snr, sigma, **fixed, **kw)
            assert e.value.code == -1 and "bias" in str(e.value)
        # a forced position beside the bias is fine
        dec.ber_sim(snr, sigma, device_channel=True, forced_index=[outside], forced_llr=100, bias=bias, **fixed)
        assert bias.sums["frames"] == 100
