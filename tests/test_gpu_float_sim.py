"""The ordered simulation around the float decoder (Decoder.ber_sim(float_bp=True), fpldpc_float_ber_sim_source)
against the frame loop it batches, restated in Python: the F64 channel, decode_float_host / decode_float_torch on a
freshly created decoder in blocks of 256, and the ordered stop rule in numpy (tests/test_gpu_sim_decoders.py's
ordered()).  Every comparison is exact unless said otherwise.  p = 13, r = 2 (n = 169: the generic float kernel),
max_iter 7, first frame 37, 1000 frames, chunks of 64, stop at the 25th frame error; W (bp_float_reg<8>) and A
(bp_float_reg<47>) once each.

Eb/N0: found on the CPU with the oracle's double decoder (oracle.decode_float_batch over oracle.gen_llr_f64,
all-zero codeword, frames 37 .. 1036, max_iter 7), so that the frame error share lies in 5 % .. 50 % and the 25th
frame error falls strictly inside a chunk of round >= 2:
  p = 13, r = 2 at 4.0 dB: 126 / 1000 frame errors, stop frame 37 + 146 (chunk 2, position 18)
                 (3.5 dB: 266, the stop in chunk 1; 4.5 dB: 47, below 5 %)
  W at 3.0 dB:             62 / 1000 frame errors, stop frame 37 + 348 (chunk 5, position 28)
                 (2.8 dB: 138, the stop in chunk 1; 3.2 dB: 21 frame errors, no 25th)
The tests assert both properties on the GPU reference loop itself."""
import numpy as np
import pytest

import test_gpu_bias_sim as BS
from test_gpu_layered_sat import small_code
from test_gpu_sim_decoders import CHUNK, FIRST, FRAMES, MAX_ITER, NEED, SEED, ordered

pytestmark = pytest.mark.gpu
INFO_SEED = 24681357
EB = {"small": 4.0, "W": 3.0, "A": 4.5}
COUNTERS = ("bit_errors", "frame_errors", "frames", "iter_sum")
BLOCK = 256


@pytest.fixture(scope="module")
def code_of(F):
    made = {}

    def get(which):
        if which not in made:
            code = {"small": lambda: small_code(F, "array13x2")[0], "W": F.Code.wifi_1944_r12,
                    "A": lambda: F.Code.array(47, 5)}[which]()
            made[which] = (code, F.Encoder.from_code(code))
        return made[which]
    return get


def make(F, code_of, which="small"):
    return F.Decoder(code_of(which)[0], max_iter=MAX_ITER)


@pytest.fixture(scope="module")
def loop(F, torch_dev, code_of):
    """The Python loop, once per key: dict(blk, its, hard [frames][hard_words] int32 on the device, cw, logw) of
    frames FIRST .. FIRST + frames - 1.  channel: "host" (channel_llr, decode_float_host) or "device"
    (channel_llr_torch / channel_llr_biased_torch, decode_float_torch); forced = (positions, double) written into the
    LLRs after the channel; random: a codeword per frame; bias: a Bias."""
    import torch
    made = {}

    def get(which="small", channel="device", frames=FRAMES, source="lehmer", forced=None, random=False, bias=None,
            key=None):
        k = (which, channel, frames, source, None if forced is None else (tuple(forced[0]), forced[1]), random, key)
        assert (bias is None) == (key is None)
        if k in made:
            return made[k]
        code, enc = code_of(which)
        snr, sigma = F.snr_sigma(EB[which], code.rate)
        dec = make(F, code_of, which)
        info = F.info_bits(INFO_SEED, FIRST, frames, enc.k) if random else np.zeros((frames, enc.k), np.uint8)
        cw = enc.encode(info) if random else None
        if not random:
            dec.set_reference(enc.info_index, info[0])
        blk, its, hard, logw = [], [], [], []
        for f0 in range(0, frames, BLOCK):
            b = min(BLOCK, frames - f0)
            if channel == "host":
                assert not random and bias is None
                llr = F.channel_llr(SEED, FIRST + f0, b, code.n, snr, sigma, 4, dtype=np.float64, source=source)
                if forced is not None:
                    llr[:, forced[0]] = forced[1]
                r = dec.decode_float_host(llr, post=False, bit_errors=True)
                h = torch.from_numpy(r["hard"].view(np.int32)).to(torch_dev)
                be, it = r["bit_errors"], r["iters"]
            else:
                cw_t = None if cw is None else torch.from_numpy(cw[f0:f0 + b]).to(torch_dev)
                if bias is not None:
                    llr, lw, _ = F.channel_llr_biased_torch(bias, SEED, FIRST + f0, b, snr, sigma, 4, cw=cw_t,
                                                            dtype=torch.float64, device=torch_dev, source=source)
                    logw.append(lw.cpu().numpy())
                else:
                    llr, _ = F.channel_llr_torch(SEED, FIRST + f0, b, code.n, snr, sigma, 4, cw=cw_t, dtype=torch.float64,
                                                 device=torch_dev, source=source)
                if forced is not None:
                    llr[:, torch.as_tensor(forced[0], device=torch_dev, dtype=torch.long)] = forced[1]
                r = dec.decode_float_torch(llr, bit_errors=not random)
                torch.cuda.synchronize()
                h, it = r["hard"], r["iters"].cpu().numpy()
                if random:
                    bits = F.unpack_hard(h.cpu().numpy(), code.n)
                    be = (bits[:, enc.info_index] != info[f0:f0 + b]).sum(axis=1).astype(np.int32)
                else:
                    be = r["bit_errors"].cpu().numpy()
            blk.append(be)
            its.append(it)
            hard.append(h)
        out = dict(blk=np.concatenate(blk), its=np.concatenate(its), hard=torch.cat(hard), cw=cw,
                   logw=np.concatenate(logw) if logw else None)
        out["blk"].setflags(write=False)
        out["its"].setflags(write=False)
        made[k] = out
        return out
    return get


def sim(F, code_of, dec, need=NEED, seen=None, which="small", frames=FRAMES, fixed_info=True, decoders=None, **kw):
    """ber_sim(float_bp=True) with the common settings; decoders: ber_sim_multi over them through host memory."""
    code, enc = code_of(which)
    snr, sigma = F.snr_sigma(EB[which], code.rate)
    args = dict(seed=SEED, first_frame=FIRST, max_frames=frames, max_frame_errors=need, chunk=CHUNK, float_bp=True,
                on_frame=None if seen is None else (lambda *a: seen.append(a)))
    if fixed_info:
        args.update(info_index=enc.info_index, info_bits=np.zeros(enc.k, np.uint8))
    args.update(kw)
    if decoders is not None:
        return F.ber_sim_multi(decoders, snr, sigma, collective=F.FPLDPC_COLL_HOST, **args)
    return dec.ber_sim(snr, sigma, **args)


def same(r, seen, ref, where):
    want, seq = ref
    print(where, {k: r[k] for k in want}, "reference", want)
    assert {k: r[k] for k in want} == want, where
    assert seen is None or seen == seq, where


def fair(ref, where):
    """The frame error share is 5 % .. 50 % up to the stop and over all frames, and the stop frame lies strictly
    inside a chunk of round >= 2, so that chunks decoded by the twin are counted."""
    stop, _ = ordered(ref["blk"], ref["its"], NEED)
    whole, _ = ordered(ref["blk"], ref["its"], 0)
    for r in (stop, whole):
        share = r["frame_errors"] / r["frames"]
        print(where, r, share)
        assert 0.05 <= share <= 0.5, (where, r)
    assert stop["frame_errors"] == NEED and whole["frames"] == len(ref["blk"])
    last = stop["frames"] - 1
    assert last // CHUNK >= 2 and 0 < last % CHUNK < CHUNK - 1, (where, last)


@pytest.mark.parametrize("channel", ["host", "device"])
def test_reference_is_a_fair_case(loop, channel):
    fair(loop(channel=channel), f"small {channel}")


@pytest.mark.parametrize("channel", ["host", "device"])
def test_counters_equal_the_python_loop(F, code_of, loop, channel):
    """1: counters and the on_frame sequence, host and device channel, both count modes."""
    ref = loop(channel=channel)
    seen = []
    r = sim(F, code_of, make(F, code_of), seen=seen, device_channel=channel == "device")
    same(r, seen, ordered(ref["blk"], ref["its"], NEED), f"float {channel}")
    assert r["frames_decoded"] >= r["frames"]
    seen = []
    r = sim(F, code_of, make(F, code_of), need=0, seen=seen, frames=200, fixed_info=False,
            count_mode=F._lib.FPLDPC_COUNT_ITERS, device_channel=channel == "device")
    its = ref["its"][:200]
    assert r["bit_errors"] == r["iter_sum"] == int(its.sum()) and r["frames"] == 200
    assert seen == [(FIRST + f, int(its[f]), int(its[f])) for f in range(200)]
    # and every frame, the last chunk a short one
    seen = []
    r = sim(F, code_of, make(F, code_of), need=0, seen=seen, device_channel=channel == "device")
    same(r, seen, ordered(ref["blk"], ref["its"], 0), f"float {channel} every frame")


@pytest.mark.parametrize("how", ["one_chunk_at_a_time", "chunk96", "chunk_auto", "two_decoders"])
def test_counters_depend_on_neither_chunks_nor_ranks(F, code_of, loop, how, monkeypatch):
    """2: FPLDPC_SIM_OVERLAP=0, chunk 96, chunk 0 (auto), two decoders on the one GPU through host memory."""
    ref = loop()
    want = ordered(ref["blk"], ref["its"], NEED)
    seen = []
    if how == "one_chunk_at_a_time":
        monkeypatch.setenv("FPLDPC_SIM_OVERLAP", "0")
        r = sim(F, code_of, make(F, code_of), seen=seen, device_channel=True)
    elif how == "two_decoders":
        r = sim(F, code_of, None, seen=seen, decoders=[make(F, code_of), make(F, code_of)], device_channel=True)
        assert r["collective"] == F.FPLDPC_COLL_HOST
        host = sim(F, code_of, None, decoders=[make(F, code_of), make(F, code_of)], device_channel=False)
        same(host, None, ordered(*[loop(channel="host")[k] for k in ("blk", "its")], NEED), "two decoders, host channel")
    else:
        r = sim(F, code_of, make(F, code_of), seen=seen, device_channel=True, chunk=96 if how == "chunk96" else 0)
    same(r, seen, want, how)


def test_random_info(F, code_of, loop):
    """3: info_bits, Encoder.encode, the F64 channel with a codeword per frame, decode_float_torch, numpy's count."""
    ref = loop(random=True)
    want = ordered(ref["blk"], ref["its"], NEED)
    assert want[0]["frame_errors"] == NEED and want[0]["frames"] > 2 * CHUNK
    seen = []
    r = sim(F, code_of, make(F, code_of), seen=seen, fixed_info=False, device_channel=True, random_info=True,
            info_seed=INFO_SEED)
    same(r, seen, want, "random_info")
    r = sim(F, code_of, make(F, code_of), need=0, fixed_info=False, device_channel=True, random_info=True,
            info_seed=INFO_SEED, count_mode=F._lib.FPLDPC_COUNT_ITERS)
    assert r["bit_errors"] == r["iter_sum"] == int(ref["its"].astype(np.int64).sum())


def shortened(code_of):
    return [int(i) for i in code_of("small")[1].info_index[::3]]


@pytest.mark.parametrize("frac_bits", [4, 2])
@pytest.mark.parametrize("channel", ["host", "device"])
def test_forced_positions(F, code_of, loop, channel, frac_bits):
    """4: a shortened set of information positions with forced_llr = 112: the doubles 112 / 2^frac_bits."""
    pos = shortened(code_of)
    ref = loop(channel=channel, forced=(pos, 112 / 2.0 ** frac_bits))
    plain = loop(channel=channel)
    differs = lambda a, b: not ((a["blk"] == b["blk"]).all() and (a["its"] == b["its"]).all())
    assert (ref["blk"] > 0).sum() > 0 and differs(ref, plain)  # shortening changes the decode
    if frac_bits == 2:  # and 28.0 is not 7.0
        assert differs(ref, loop(channel=channel, forced=(pos, 112 / 16.0)))
    want = ordered(ref["blk"], ref["its"], NEED)
    assert want[0]["frame_errors"] > 0 and want[0]["frames"] > 2 * CHUNK
    seen = []
    r = sim(F, code_of, make(F, code_of), seen=seen, device_channel=channel == "device", forced_index=pos,
            forced_llr=112, frac_bits=frac_bits)
    same(r, seen, want, f"forced {channel} frac_bits={frac_bits}")


def test_forced_positions_refused_as_now(F, code_of):
    code, enc = code_of("small")
    pos = shortened(code_of)
    bias = F.Bias(code.n, sorted(pos[:2] + [int(enc.parity_index[0])]), 0.5)
    with pytest.raises(F.FpldpcError, match="forced position is also a biased one") as e:
        sim(F, code_of, make(F, code_of), device_channel=True, forced_index=pos, forced_llr=112, bias=bias)
    assert e.value.code == -1
    with pytest.raises(F.FpldpcError, match="random_info: no forced positions") as e:
        sim(F, code_of, make(F, code_of), fixed_info=False, device_channel=True, random_info=True, forced_index=pos,
            forced_llr=112)
    assert e.value.code == -1


def expected_harvest(hv, ref, stop, max_records):
    """Harvest.scan_torch over the loop's hard decisions up to the stop frame, gathered as the harvest defines."""
    import torch
    cw = None if ref["cw"] is None else torch.from_numpy(ref["cw"][:stop]).to(ref["hard"].device)
    s = {k: v.cpu().numpy() for k, v in hv.scan_torch(ref["hard"][:stop].contiguous(), cw).items()}
    torch.cuda.synchronize()
    w, u = s["weight"], s["unsat"]
    bad = np.nonzero(w > 0)[0]
    keep = bad[:max_records]
    records = {"frame": (FIRST + keep).astype(np.int64), "iters": ref["its"][:stop].astype(np.int32)[keep],
               "info_errors": ref["blk"][:stop].astype(np.int32)[keep], "weight": w[keep], "unsat": u[keep],
               "err": s["err"][keep].view(np.uint32), "syn": s["syn"][keep].view(np.uint32)}
    counts = dict(frames=stop, codeword_errors=len(bad), detected=int((u[bad] > 0).sum()),
                  undetected=int((u[bad] == 0).sum()), recorded=len(keep), dropped=len(bad) - len(keep))
    classes = {}
    for a, b in sorted(zip(w[bad].tolist(), u[bad].tolist())):
        classes[(a, b)] = classes.get((a, b), 0) + 1
    return records, counts, classes


@pytest.mark.parametrize("random", [False, True])
@pytest.mark.parametrize("max_records", [8, 4096])
def test_harvest(F, code_of, loop, max_records, random):
    """5: counts, classes and records against scan_torch on the loop's hard decisions up to the stop frame."""
    ref = loop(random=random)
    want = ordered(ref["blk"], ref["its"], NEED)
    stop = want[0]["frames"]
    seen = []
    more = dict(fixed_info=False, random_info=True, info_seed=INFO_SEED) if random else {}
    r = sim(F, code_of, make(F, code_of), seen=seen, device_channel=True, harvest=max_records, **more)
    same(r, seen, want, f"harvest {max_records}")
    hv = r["harvest"]
    records, counts, classes = expected_harvest(hv, ref, stop, max_records)
    assert counts["codeword_errors"] >= NEED > 8 and (counts["dropped"] > 0) == (max_records == 8)
    assert hv.counts == counts
    assert hv.classes == classes and list(hv.classes) == sorted(classes)
    for k, w in records.items():
        g = getattr(hv, k)
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), k


@pytest.fixture(scope="module")
def bias(F, code_of, loop):
    """On the wrong bits of the lowest-weight codeword error of the plain loop."""
    code = code_of("small")[0]
    ref = loop()
    hv = F.Harvest(code, 0)
    w = hv.scan_torch(ref["hard"], None)
    weight = w["weight"].cpu().numpy()
    f = int(np.argmin(np.where(weight > 0, weight, 1 << 30)))
    pos = np.nonzero(F.unpack_hard(w["err"][f:f + 1].cpu().numpy(), code.n)[0])[0]
    assert 0 < len(pos) == weight[f]
    print("bias on", pos.tolist())
    return F.Bias(code.n, pos, 0.5)


def test_bias(F, code_of, loop, bias):
    """6: the weighted sums (tests/test_gpu_bias_sim.py's rule for them) and the counters on the shifted channel."""
    ref, plain = loop(bias=bias, key="bias"), loop()
    assert (ref["blk"] > 0).sum() > (plain["blk"] > 0).sum() > 0  # the shift costs frames
    for need in (0, NEED):
        want = ordered(ref["blk"], ref["its"], need)
        seen = []
        r = sim(F, code_of, make(F, code_of), need=need, seen=seen, device_channel=True, bias=bias)
        same(r, seen, want, f"bias need={need}")
        assert r["bias"] is bias
        BS.assert_sums(bias.sums, BS.sums_of(ref["blk"], ref["logw"], want[0]["frames"]))
        est = bias.estimate(k=code_of("small")[1].k)
        assert est["fer"] == bias.sums["sum_w_fe"] / bias.sums["frames"]
    # two decoders and another chunk: the same sums bit for bit
    first = bias.sums
    sim(F, code_of, None, decoders=[make(F, code_of), make(F, code_of)], device_channel=True, bias=bias, chunk=96)
    assert bias.sums == first


def test_empty_bias_is_the_unbiased_run(F, code_of, loop):
    ref = loop()
    keys = COUNTERS + ("frames_decoded",)
    s0, s1 = [], []
    plain = sim(F, code_of, make(F, code_of), seen=s0, device_channel=True)
    empty = F.Bias(code_of("small")[0].n, [], [])
    r = sim(F, code_of, make(F, code_of), seen=s1, device_channel=True, bias=empty)
    assert {k: r[k] for k in keys} == {k: plain[k] for k in keys} and s0 == s1
    same(r, s1, ordered(ref["blk"], ref["its"], NEED), "empty bias")
    s = empty.sums
    assert s["sum_w"] == s["sum_w2"] == s["frames"] == r["frames"] and s["sum_w_fe"] == s["frame_errors"] == NEED
    assert s["sum_w_be"] == s["bit_errors"] == r["bit_errors"] and s["min_logw"] == s["max_logw"] == 0.0


def test_philox(F, code_of, loop):
    """7: source="philox" on the device channel."""
    ref, lehmer = loop(source="philox"), loop()
    assert not (ref["blk"] == lehmer["blk"]).all()
    want = ordered(ref["blk"], ref["its"], NEED)
    assert want[0]["frame_errors"] == NEED and want[0]["frames"] > 2 * CHUNK
    seen = []
    r = sim(F, code_of, make(F, code_of), seen=seen, device_channel=True, source="philox")
    same(r, seen, want, "philox")


def test_w_register_kernel_and_its_twin(F, code_of, loop):
    """8: W at max_iter 7 runs bp_float_reg<8> on the caller's decoder and on the twin."""
    dec = make(F, code_of, "W")
    assert dec.float_describe().startswith("bp_float_reg<DC=8,predicated,table>"), dec.float_describe()
    ref = loop(which="W")
    fair(ref, "W")
    seen = []
    r = sim(F, code_of, make(F, code_of, "W"), seen=seen, which="W", device_channel=True)
    same(r, seen, ordered(ref["blk"], ref["its"], NEED), "W")
    assert r["frames_decoded"] > r["frames"]


def test_a_register_kernel(F, code_of, loop):
    """8: A, 300 frames, runs bp_float_reg<47>."""
    dec = make(F, code_of, "A")
    assert dec.float_describe().startswith("bp_float_reg<DC=47,regular,array>"), dec.float_describe()
    ref = loop(which="A", frames=300)
    want = ordered(ref["blk"], ref["its"], 0)
    assert 0 < want[0]["frame_errors"] < 300
    seen = []
    r = sim(F, code_of, make(F, code_of, "A"), need=0, seen=seen, which="A", frames=300, device_channel=True)
    same(r, seen, want, "A")


def star_alist(d):
    """One variable in d checks of degree 2: n = d + 1, m = d, check r = {0, r + 1}; variable degree d, check degree 2."""
    lines = [f"{d + 1} {d}", f"{d} 2", " ".join([str(d)] + ["1"] * d), " ".join(["2"] * d), " ".join(map(str, range(d)))]
    return "\n".join(lines + [str(v - 1) for v in range(1, d + 1)] + [f"0 {r + 1}" for r in range(d)]) + "\n"


@pytest.mark.parametrize("device_channel", [False, True])
def test_float_envelope_is_refused_before_any_frame(F, device_channel):
    """9: a code inside the flooding decoder's envelope (check degree 2, n = 301) and outside the float decoder's (a
    variable of degree 300 > 255): the Decoder exists, and the float simulation on it is FPLDPC_ERR_UNSUPPORTED with
    the float decoder's message before any frame is generated or decoded."""
    code = F.Code.parse(star_alist(300))
    assert (code.n, code.m, code.dv_max, code.dc_max) == (301, 300, 300, 2)
    dec = F.Decoder(code, max_iter=MAX_ITER)
    snr, sigma = F.snr_sigma(4.0, code.rate)
    seen = []
    kw = dict(max_frames=8, chunk=4, device_channel=device_channel, count_mode=F._lib.FPLDPC_COUNT_ITERS,
              on_frame=lambda *a: seen.append(a))
    with pytest.raises(F.FpldpcError, match="float decoder: variable degree > 255") as e:
        dec.ber_sim(snr, sigma, float_bp=True, **kw)
    assert e.value.code == -4 and seen == []
    with pytest.raises(F.FpldpcError, match="float decoder: variable degree > 255") as e:
        F.ber_sim_multi([dec, F.Decoder(code, max_iter=MAX_ITER)], snr, sigma, collective=F.FPLDPC_COLL_HOST, float_bp=True,
                        **kw)
    assert e.value.code == -4 and seen == []


def test_array_131_has_no_decoder(F):
    """9: Code.array(131, 2) (n = 17,161, check degree 131) is outside the float envelope too, but no Decoder exists
    for it: fpldpc_decoder_create refuses check degrees above 64, so the way to a float simulation ends there."""
    big = F.Code.array(131, 2)
    assert big.n == 17161 and big.dc_max == 131
    with pytest.raises(F.FpldpcError, match="check degree above 64") as e:
        F.Decoder(big, max_iter=MAX_ITER)
    assert e.value.code == -4


def test_three_argument_entry_point(F, code_of, loop):
    """fpldpc_float_ber_sim is fpldpc_float_ber_sim_source with ndev = 1, FPLDPC_COLL_HOST, FPLDPC_NOISE_LEHMER and no
    bias or harvest: test 1's counters and on_frame sequence from the C entry point itself."""
    import ctypes
    from fixedpointldpc_amd import _lib
    code, enc = code_of("small")
    ref = loop()
    snr, sigma = F.snr_sigma(EB["small"], code.rate)
    seen = []
    p, keep = _lib.sim_params(snr, sigma, info_index=enc.info_index, info_bits=np.zeros(enc.k, np.uint8), seed=SEED,
                              first_frame=FIRST, max_frames=FRAMES, max_frame_errors=NEED, chunk=CHUNK, device_channel=True,
                              on_frame=lambda *a: seen.append(a))
    r = _lib.SimResult()
    dec = make(F, code_of)
    assert F.lib().fpldpc_float_ber_sim(dec._h, ctypes.byref(p), ctypes.byref(r)) == 0
    del keep
    same({k: getattr(r, k) for k in COUNTERS}, seen, ordered(ref["blk"], ref["its"], NEED), "fpldpc_float_ber_sim")


def test_refusals(F, code_of):
    """9: the harvest's rules and the keyword's."""
    other = F.Harvest(small_code(F, "array13x3")[0], 16)
    with pytest.raises(F.FpldpcError, match="harvest was made from another code") as e:
        sim(F, code_of, make(F, code_of), device_channel=True, harvest=other)
    assert e.value.code == -1
    with pytest.raises(F.FpldpcError, match="a harvest needs count_mode") as e:
        sim(F, code_of, make(F, code_of), device_channel=True, harvest=16, count_mode=F._lib.FPLDPC_COUNT_ITERS)
    assert e.value.code == -1
    ms = F.MinSumDecoder(code_of("small")[0], max_iter=MAX_ITER)
    with pytest.raises(TypeError, match="float_bp=True needs Decoder objects"):
        sim(F, code_of, ms, device_channel=True)
    with pytest.raises(TypeError, match="float_bp=True needs Decoder objects"):
        sim(F, code_of, None, decoders=[make(F, code_of), ms], device_channel=True)


def test_one_decoder_both_ways(F, code_of, loop):
    """10: fixed, float, fixed on one object."""
    ref = loop()
    dec = make(F, code_of)
    keys = COUNTERS + ("frames_decoded",)

    def fixed():
        seen = []
        r = sim(F, code_of, dec, seen=seen, device_channel=True, float_bp=False)
        return {k: r[k] for k in keys}, seen
    before = fixed()
    seen = []
    r = sim(F, code_of, dec, seen=seen, device_channel=True)
    same(r, seen, ordered(ref["blk"], ref["its"], NEED), "float between two fixed runs")
    assert fixed() == before and before[0]["frame_errors"] == NEED
    assert before[1] != seen  # and the two decoders are not one
    # and the reverse: float, fixed, float
    r2 = sim(F, code_of, dec, device_channel=True)
    assert {k: r2[k] for k in keys} == {k: r[k] for k in keys}
