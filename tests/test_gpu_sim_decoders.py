"""fpldpc_layered_ber_sim / fpldpc_minsum_ber_sim (and their _multi forms) against the frame loop they batch,
restated in Python over a freshly created decoder of the same class and arguments: the host channel's int16
LLRs, decode_host(bit_errors=True) in blocks, and the ordered stop rule in numpy.  Counters and the on_frame
sequence must be equal.  The widths, scale and offset are not the defaults, and the kernel choice of some
cases depends on an environment switch that is gone when the simulation runs: a twin built with defaults, or
one that chose again, decodes the odd rounds differently, and only the counters can show it.

Eb/N0 per code: found once on the CPU with the numpy models of this directory (layered_model,
layered_sat_model, layered_minsum_model, minsum_model; all-zero codeword, frames 37 .. 1036, max_iter 7) so that
the frame error share lies in 5 % .. 50 % and the 25th frame error falls inside a chunk of round >= 2:
  p = 13, r = 2 at 4.0 dB: 121 / 1000 frame errors (sxor, all three layered kinds), 165 (layered min-sum),
                           149 (flooding min-sum); stop frames 37 + 154, 37 + 133, 37 + 133
  W at 3.2 dB:             96 / 1000 (flooding min-sum); stop frame 37 + 230
The tests assert both properties on the GPU reference itself."""
import numpy as np
import pytest

from test_gpu_layered_sat import small_code

pytestmark = pytest.mark.gpu
SEED = 123456789
FIRST, FRAMES, CHUNK, NEED, MAX_ITER = 37, 1000, 64, 25, 7
MS = dict(post_bits=10, msg_bits=8, scale_16=13, offset=3)
# name -> (code, Eb/N0, class, keywords, environment at creation only)
CASES = {
    "unsat": ("small", 4.0, "LayeredDecoder", {}, {}),
    "sat_i16": ("small", 4.0, "LayeredDecoder", dict(post_bits=12, msg_bits=10), {}),
    "sat_i32": ("small", 4.0, "LayeredDecoder", dict(post_bits=20, msg_bits=12), {}),
    "layered_minsum": ("small", 4.0, "LayeredDecoder", dict(check="minsum", **MS), {}),
    "flood_minsum": ("small", 4.0, "MinSumDecoder", MS, {}),
    "flood_minsum_w": ("W", 3.2, "MinSumDecoder", MS, {"FPLDPC_MINSUM_TABLE": "global"}),
    # the state in global memory, chosen by a switch that is read at creation
    "layered_minsum_global": ("small", 4.0, "LayeredDecoder", dict(check="minsum", **MS),
                              {"FPLDPC_LAYERED_MINSUM_STATE": "global"}),
    "flood_minsum_global": ("small", 4.0, "MinSumDecoder", MS, {"FPLDPC_MINSUM_STATE": "global"}),
}
LDS_OF = {"layered_minsum_global": "layered_minsum", "flood_minsum_global": "flood_minsum"}
ALL = list(CASES)
MAIN = [c for c in ALL if c not in LDS_OF]


@pytest.fixture(scope="module")
def code_of(F):
    made = {}

    def get(which):
        if which not in made:
            code = F.Code.wifi_1944_r12() if which == "W" else small_code(F, "array13x2")[0]
            made[which] = (code, F.Encoder.from_code(code).info_index.copy())
        return made[which]
    return get


def make(F, code_of, name):
    """A new decoder of the case; its environment switches are set for the creation only."""
    import os
    which, eb, cls, kw, env = CASES[name]
    code, _ = code_of(which)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        dec = getattr(F, cls)(code, max_iter=MAX_ITER, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    d = dec.describe()
    if name.endswith("_global"):
        assert "mem=global" in d and "scratch=" in d, d
    elif "minsum" in name:
        assert "mem=global" not in d, d
    if name == "flood_minsum_w":
        assert "addr=gtable" in d, d
    return dec


def sim_args(F, code_of, name):
    which, eb = CASES[name][:2]
    code, idx = code_of(which)
    snr, sigma = F.snr_sigma(eb, code.rate)
    return code, snr, sigma, dict(info_index=idx, info_bits=np.zeros(len(idx), np.uint8), seed=SEED, first_frame=FIRST,
                                  max_frames=FRAMES)


def ordered(blk, its, need, first=FIRST):
    """The serial loop's counters and on_frame sequence: frames in order, stopping after the frame that brings the
    frame errors to `need` (0: no such stop)."""
    fe = np.cumsum(blk > 0)
    stop = len(blk) if need <= 0 or fe[-1] < need else int(np.argmax(fe >= need)) + 1
    b, i = blk[:stop].astype(np.int64), its[:stop].astype(np.int64)
    res = dict(bit_errors=int(b.sum()), frame_errors=int((b > 0).sum()), frames=stop, iter_sum=int(i.sum()))
    return res, [(first + f, int(i[f]), int(b[f])) for f in range(stop)]


@pytest.fixture(scope="module")
def reference(F, code_of):
    """name -> (blkerror, iterations) of frames FIRST .. FIRST + FRAMES - 1 from the Python loop, computed once."""
    done = {}

    def get(name):
        if name not in done:
            code, snr, sigma, kw = sim_args(F, code_of, name)
            dec = make(F, code_of, name)
            dec.set_reference(kw["info_index"], kw["info_bits"])
            blk, its = [], []
            for f0 in range(0, FRAMES, 256):
                llr = F.channel_llr(SEED, FIRST + f0, min(256, FRAMES - f0), code.n, snr, sigma, 4, dtype=np.int16)
                r = dec.decode_host(llr, bit_errors=True)
                blk.append(r["bit_errors"])
                its.append(r["iters"])
            done[name] = (np.concatenate(blk), np.concatenate(its))
            done[name][0].setflags(write=False)
            done[name][1].setflags(write=False)
        return done[name]
    return get


def same(r, seen, ref, where):
    want, seq = ref
    print(where, {k: r[k] for k in want}, "reference", want)
    assert {k: r[k] for k in want} == want, where
    assert seen == seq, where


def run(F, code_of, dec, name, need, **more):
    _, snr, sigma, kw = sim_args(F, code_of, name)
    seen = []
    r = dec.ber_sim(snr, sigma, max_frame_errors=need, chunk=CHUNK, on_frame=lambda *a: seen.append(a), **kw, **more)
    return r, seen


@pytest.mark.parametrize("name", ALL)
def test_reference_is_a_fair_case(reference, name):
    """The frame error share is 5 % .. 50 % in both runs, and the stop frame lies strictly inside a chunk of
    round >= 2, so that rounds decoded by the twin are counted."""
    blk, its = reference(name)
    stop, _ = ordered(blk, its, NEED)
    whole, _ = ordered(blk, its, 0)
    for r in (stop, whole):
        share = r["frame_errors"] / r["frames"]
        print(name, r, share)
        assert 0.05 <= share <= 0.5, (name, r)
    assert stop["frame_errors"] == NEED and whole["frames"] == FRAMES
    last = stop["frames"] - 1
    assert last // CHUNK >= 2 and 0 < last % CHUNK < CHUNK - 1, (name, last)


@pytest.mark.parametrize("device_channel", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_counters_equal_the_python_loop(F, code_of, reference, name, device_channel):
    dec = make(F, code_of, name)
    r, seen = run(F, code_of, dec, name, NEED, device_channel=device_channel)
    same(r, seen, ordered(*reference(name), NEED), f"{name} device_channel={device_channel}")
    assert r["frames_decoded"] >= r["frames"]


@pytest.mark.parametrize("name", ALL)
def test_one_chunk_at_a_time(F, code_of, reference, name, monkeypatch):
    """FPLDPC_SIM_OVERLAP=0: no twin, the same counters."""
    dec = make(F, code_of, name)
    monkeypatch.setenv("FPLDPC_SIM_OVERLAP", "0")
    r, seen = run(F, code_of, dec, name, NEED, device_channel=True)
    same(r, seen, ordered(*reference(name), NEED), f"{name} one chunk at a time")


@pytest.mark.parametrize("name", list(LDS_OF))
def test_state_placement_is_not_semantics(reference, name):
    for a, b in zip(reference(name), reference(LDS_OF[name])):
        assert (a == b).all()


@pytest.mark.parametrize("name", MAIN)
def test_every_frame_counted(F, code_of, reference, name):
    """max_frame_errors = 0: all 1000 frames, the last chunk a short one."""
    dec = make(F, code_of, name)
    r, seen = run(F, code_of, dec, name, 0, device_channel=True)
    assert r["frames"] == FRAMES
    same(r, seen, ordered(*reference(name), 0), f"{name} every frame")


def test_count_iters(F, code_of, reference):
    """FPLDPC_COUNT_ITERS needs no reference bits: blkerror is the iteration count."""
    name = "sat_i16"
    code, snr, sigma, _ = sim_args(F, code_of, name)
    seen = []
    r = make(F, code_of, name).ber_sim(snr, sigma, seed=SEED, first_frame=FIRST, max_frames=200, max_frame_errors=0,
                                       count_mode=F._lib.FPLDPC_COUNT_ITERS, chunk=CHUNK,
                                       on_frame=lambda *a: seen.append(a))
    its = reference(name)[1][:200]
    assert r["bit_errors"] == r["iter_sum"] == int(its.sum()) and r["frames"] == 200
    assert seen == [(FIRST + f, int(its[f]), int(its[f])) for f in range(200)]


@pytest.mark.parametrize("chunk", [64, 50])
@pytest.mark.parametrize("name", ["sat_i16", "layered_minsum", "flood_minsum", "flood_minsum_global"])
def test_multi_equals_single(F, code_of, reference, name, chunk):
    decs = [make(F, code_of, name), make(F, code_of, name)]
    _, snr, sigma, kw = sim_args(F, code_of, name)
    seen = []
    r = F.ber_sim_multi(decs, snr, sigma, collective=F.FPLDPC_COLL_HOST, max_frame_errors=NEED, chunk=chunk,
                        device_channel=True, on_frame=lambda *a: seen.append(a), **kw)
    assert r["collective"] == F.FPLDPC_COLL_HOST
    single = decs[0].ber_sim(snr, sigma, max_frame_errors=NEED, chunk=chunk, device_channel=True, **kw)
    assert {k: r[k] for k in ("bit_errors", "frame_errors", "frames", "iter_sum")} == \
        {k: single[k] for k in ("bit_errors", "frame_errors", "frames", "iter_sum")}
    same(r, seen, ordered(*reference(name), NEED), f"{name} two decoders chunk={chunk}")


@pytest.mark.parametrize("name", ["sat_i16", "flood_minsum"])
def test_multi_refuses_what_it_cannot_run(F, code_of, name):
    _, snr, sigma, kw = sim_args(F, code_of, name)
    dec = make(F, code_of, name)
    with pytest.raises(F.FpldpcError, match="same decoder twice") as e:
        F.ber_sim_multi([dec, dec], snr, sigma, collective=F.FPLDPC_COLL_HOST, max_frame_errors=NEED, **kw)
    assert e.value.code == -1
    cls, args = CASES[name][2:4]
    other = getattr(F, cls)(small_code(F, "array13x3")[0], max_iter=MAX_ITER, **args)
    with pytest.raises(F.FpldpcError, match="different codes") as e:
        F.ber_sim_multi([dec, other], snr, sigma, collective=F.FPLDPC_COLL_HOST, max_frame_errors=NEED, **kw)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        F.ber_sim_multi([dec, F.Decoder(code_of("small")[0], max_iter=MAX_ITER)], snr, sigma, max_frame_errors=NEED, **kw)
    # the rules of the flooding decoder's simulation, word for word
    with pytest.raises(F.FpldpcError, match="needs max_frame_errors or max_frames"):
        dec.ber_sim(snr, sigma, **{**kw, "max_frames": 0}, max_frame_errors=0)
    with pytest.raises(F.FpldpcError, match="FPLDPC_COUNT_BITS needs info_index / info_bits"):
        dec.ber_sim(snr, sigma, max_frames=10)
