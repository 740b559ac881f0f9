"""The wide form of the two min-sum decoders (fpldpc_minsum_wide.hip: check degrees up to 255, run-time slot
loops, 8 + 4 W bytes of check state for W = ceil(dc_max / 32) sign words) against the widened numpy models
(tests/minsum_wide_model.py): iterations, hard decisions, syndrome flags and posteriors exactly.

  (i)   every code of the wide family (tests/wide_family.py) in both decoders with the table in LDS, the table
        global and the state global, at 14/16-2 and 16/16-0: families (a), (b), (d), (e) in one batch, family (c)
        with and without early termination, the pre-check on the constant frames; the whole describe() string
        pinned, lds= and scratch= from the layout the kernel's header states.
  (ii)  FPLDPC_MINSUM_FORM=wide on reg47, reg64 and mix of the shipped family: the shipped models and the bucket
        form, bit for bit.
  (iii) the flooding decoder at 16/15, plain min-sum, on reg129 with (a) // 4: the oracle's flooding decode at
        frac_bits = 0.
  (iv)  the global placement by size, no switch set.
  (v)   a simulation with its twin decoder, and a harvest, on Code.array(67, 3).
  (vi)  refusals: a check of degree 256; the sxor layered decoder on reg65.
What the inputs reach is pinned on the CPU in tests/test_minsum_wide_model.py, not here."""
import re

import numpy as np
import pytest

import degree_family as D
import harvest_model as HM
import minsum_wide_model as WM
import wide_family as W
from conftest import assert_same
from test_gpu_layered_sat import run

pytestmark = pytest.mark.gpu

KEYS = ("iters", "hard", "syndrome_ok", "post")
KINDS = ("fms", "lms")
PARAMS = ((12, 10, 14, 2), (12, 10, 16, 0))
PLACEMENTS = ("lds_table", "global_table", "global")
SWITCH = {
    "lms": {"lds_table": {"FPLDPC_LAYERED_TABLE": "lds"}, "global_table": {"FPLDPC_LAYERED_TABLE": "global"},
            "global": {"FPLDPC_LAYERED_MINSUM_STATE": "global"}},
    "fms": {"lds_table": {"FPLDPC_MINSUM_TABLE": "lds"}, "global_table": {"FPLDPC_MINSUM_TABLE": "global"},
            "global": {"FPLDPC_MINSUM_STATE": "global"}},
}


def up(x, to):
    return -(-x // to) * to


def expected_describe(kind, n, m, dc_max, L, layers, params, placement):
    """The describe() string of the wide form as a regular expression (grid and device are the machine's), and the
    bytes of a workgroup's slice (0: state in LDS).  The layout is the one fpldpc_minsum_wide.hip states:
    8 + 4 W bytes of state per check; the int16 vector to a whole word, 16 bytes of control words, the index table
    [dc_max][m] uint16 where it is in LDS, one byte per check of the degree table."""
    Wn = -(-dc_max // 32)
    state, vec16, flood = (8 + 4 * Wn) * m, up(2 * n, 4), kind == "fms"
    table = 2 * dc_max * m if placement == "lds_table" else 0
    addr = "table" if placement == "lds_table" else "gtable"
    mem, scratch = "", 0
    if placement == "global":
        lds, mem = vec16 + 16 + m, ",mem=global"
        scratch = up(state + (12 * n if flood else 0), 256)
    elif flood:
        lds = state + 12 * n + vec16 + 16 + table + m
    else:
        lds = vec16 + 16 + state + table + m
    tail = f" sat={params[0]}/{params[1]} ms={params[2]}/16-{params[3]} state=compressed"
    if flood:
        head = re.escape(f"flood_minsum_wide<DC={32 * Wn},addr={addr},deg=table{mem}>")
        want = rf"{head} grid=(\d+) threads={min(256, up(m, 64))} lds={lds} device=\d+{re.escape(tail)}"
    else:
        head = re.escape(f"layered_minsum_wide<DC={32 * Wn},addr={addr},deg=table{mem}>")
        want = rf"{head} L={L} layers={layers} grid=(\d+) threads={min(256, up(L, 64))} lds={lds} device=\d+{re.escape(tail)}"
    return want + (r" scratch=(\d+)" if scratch else ""), scratch


def test_describe_strings_the_issue_names():
    want, scratch = expected_describe("fms", 645, 15, 129, 5, 3, (12, 10, 14, 2), "lds_table")
    assert "flood_minsum_wide<DC=160,addr=table,deg=table>" in want.replace("\\", "") and scratch == 0
    assert f"lds={28 * 15 + 12 * 645 + 1292 + 16 + 2 * 129 * 15 + 15} " in want  # W = 5: 28 bytes per check
    want, scratch = expected_describe("lms", 645, 15, 129, 5, 3, (12, 10, 14, 2), "global")
    assert "layered_minsum_wide<DC=160,addr=gtable,deg=table,mem=global> L=5 layers=3 " in want.replace("\\", "")
    assert "lds=1323 " in want and scratch == 512


def make(F, monkeypatch, kind, code, L, params, env, **kw):
    """The decoder, the environment switches set around its creation only."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        ms = dict(post_bits=params[0], msg_bits=params[1], scale_16=params[2], offset=params[3])
        if kind == "fms":
            return F.MinSumDecoder(code, **ms, **kw)
        return F.LayeredDecoder(code, check="minsum", layer_checks=L, **ms, **kw)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def check_describe(dec, kind, params, placement, L=0):
    """The decoder's describe() string is the wide form's; returns the grid."""
    code = dec.code
    L, layers = (L, code.m // L) if L else (code.m, 1)
    want, slice_bytes = expected_describe(kind, code.n, code.m, code.dc_max, L, layers, params, placement)
    d = dec.describe()
    got = re.fullmatch(want, d)
    assert got, f"{d!r} is not {want!r}"
    grid = int(got.group(1))
    assert 0 < grid < 100000, d
    if slice_bytes:
        assert int(got.group(2)) == grid * slice_bytes, d
    return grid


_CODES = {}


def family_code(F, name):
    if name not in _CODES:
        _CODES[name] = F.Code.parse(W.alist_of(name) if name in W.CODES else D.alist_of(name))
    return _CODES[name]


def create(F, monkeypatch, name, kind, params, placement, **kw):
    dec = make(F, monkeypatch, kind, family_code(F, name), W.layer_size(name), params, SWITCH[kind][placement],
               **{"max_iter": W.MAX_ITER, **kw})
    check_describe(dec, kind, params, placement, W.layer_size(name) if kind == "lms" else 0)
    return dec


# ---- (i) every wide code, both decoders, every placement ----

@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", W.NAMES)
def test_form(F, torch_dev, monkeypatch, name, kind, placement):
    """Families (a), (b), (d) and (e) in one batch, at both parameter sets."""
    for params in PARAMS:
        dec = create(F, monkeypatch, name, kind, params, placement)
        assert_same(run(dec, W.inputs(name), torch_dev), W.reference(name, kind, params), dec.code.n,
                    where=f"{name} {kind} {params} {placement}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", W.NAMES)
def test_noisy_frames_with_early_termination(F, torch_dev, monkeypatch, name, kind):
    """Family (c): frames of one batch stop after different numbers of iterations."""
    dec = create(F, monkeypatch, name, kind, PARAMS[0], "lds_table")
    assert_same(run(dec, W.inputs(name, "c"), torch_dev), W.reference(name, kind, PARAMS[0], "c"), dec.code.n,
                where=f"{name} {kind} noisy")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", W.NAMES)
def test_noisy_frames_without_early_termination(F, torch_dev, monkeypatch, name, kind):
    """The same frames to the last iteration: converged frames go on through every slot."""
    dec = create(F, monkeypatch, name, kind, PARAMS[0], "global", early_term=False)
    assert_same(run(dec, W.inputs(name, "c"), torch_dev), W.reference(name, kind, PARAMS[0], "c", early_term=False),
                dec.code.n, where=f"{name} {kind} noisy, no early termination")


@pytest.mark.parametrize("placement", ("lds_table", "global"))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", W.NAMES)
def test_precheck_on_the_constant_frames(F, monkeypatch, name, kind, placement):
    """Family (e) with the channel pre-check: 0 iterations and untouched posteriors where it passes."""
    llr = W.inputs(name, "e")
    ref = W.reference(name, kind, PARAMS[0], "e", precheck=True)
    pre = ref["prechecked"]
    dec = create(F, monkeypatch, name, kind, PARAMS[0], placement, precheck=True)
    out = dec.decode_host(llr, post=np.full(llr.shape, -123456, np.int32))
    assert_same(out, ref, dec.code.n, check_post=False, where=f"{name} {kind} {placement} precheck")
    assert (out["iters"][pre] == 0).all() and (out["iters"][~pre] >= 1).all()
    assert (out["post"][pre] == -123456).all() and (out["post"][~pre] == ref["post"][~pre]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_mixw_more_frames_than_the_grid(F, torch_dev, monkeypatch, kind):
    """The resident grid plus 3 frames, state global: a workgroup's second frame starts from zero state in the
    slice its first one used."""
    dec = make(F, monkeypatch, kind, family_code(F, "mixw"), W.layer_size("mixw"), PARAMS[0], SWITCH[kind]["global"],
               max_iter=W.MAX_ITER)
    grid = check_describe(dec, kind, PARAMS[0], "global", W.layer_size("mixw") if kind == "lms" else 0)
    llr, ref = W.inputs("mixw"), W.reference("mixw", kind, PARAMS[0])
    sel = np.tile(np.arange(len(llr)), -(-(grid + 3) // len(llr)))[:grid + 3]
    assert_same(run(dec, llr[sel], torch_dev), {k: ref[k][sel] for k in KEYS}, dec.code.n, where=f"mixw {kind} batch {grid + 3}")


# ---- (ii) the wide form against the bucket form ----

@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ("reg47", "reg64", "mix"))
def test_forced_wide_form_is_the_bucket_form(F, torch_dev, monkeypatch, name, kind, placement):
    params = PARAMS[0]
    code, L = family_code(F, name), D.layer_size(name)
    wide = make(F, monkeypatch, kind, code, L, params, {**SWITCH[kind][placement], "FPLDPC_MINSUM_FORM": "wide"}, max_iter=D.MAX_ITER)
    check_describe(wide, kind, params, placement, L if kind == "lms" else 0)
    bucket = make(F, monkeypatch, kind, code, L, params, SWITCH[kind][placement], max_iter=D.MAX_ITER)
    assert "_wide<" not in bucket.describe() and bucket.describe().startswith(("flood_minsum<", "layered_minsum<"))
    for family in (None, "c"):
        llr, ref = D.inputs(name, kind, family), D.reference(name, kind, params, family)
        out = run(wide, llr, torch_dev)
        assert_same(out, ref, code.n, where=f"{name} {kind} {placement} forced wide, family {family}")
        other = run(bucket, llr, torch_dev)
        for k in KEYS:
            assert (out[k] == other[k]).all(), k


def test_any_other_value_of_the_form_switch_is_ignored(F, monkeypatch):
    for kind in KINDS:
        dec = make(F, monkeypatch, kind, family_code(F, "reg47"), 5, PARAMS[0], {"FPLDPC_MINSUM_FORM": "bucket"})
        assert "_wide<" not in dec.describe(), dec.describe()


# ---- (iii) flooding against the oracle ----

@pytest.mark.parametrize("placement", PLACEMENTS)
def test_plain_min_sum_is_the_reference_flooding_decoder(F, O, torch_dev, monkeypatch, placement):
    """16/15, plain min-sum, (a) // 4 on reg129: no clamp acts (test_minsum_wide_model.py), so the flooding min-sum
    decoder computes the reference's flooding decode with C = 0."""
    params = (16, 15, 16, 0)
    dec = create(F, monkeypatch, "reg129", "fms", params, placement)
    llr = W.inputs("reg129", "q")
    out = run(dec, llr, torch_dev)
    assert_same(out, W.reference("reg129", "fms", params, "q"), dec.code.n, where=f"reg129 16/15 {placement} vs the model")
    ocode = O.OracleCode.from_alist_text(W.alist_of("reg129"))
    assert_same(out, O.decode_batch(ocode, llr, W.MAX_ITER, 0, 0xFF), dec.code.n, where=f"reg129 16/15 {placement} vs the oracle")


# ---- (iv) the global placement by size ----

def test_flooding_goes_global_by_size(F, torch_dev):
    """Code.array(107, 3), n = 11,449, m = 321: three int32 accumulators and the int16 LLRs alone are 14 n =
    160,286 B, with any check state beyond 160 KiB.  A forward array code: its index table is built."""
    code = F.Code.array(107, 3)
    assert (code.n, code.m, code.dc_max) == (11449, 321, 107) and 14 * code.n + 32 + 17 * code.m > 160 * 1024
    dec = F.MinSumDecoder(code, post_bits=12, msg_bits=10, scale_16=12, max_iter=3)
    assert "mem=global" in dec.describe() and "addr=gtable" in dec.describe()
    check_describe(dec, "fms", (12, 10, 12, 0), "global")
    llr = np.concatenate([np.rint(np.random.default_rng(3).normal(60, 40, (4, code.n))),
                          np.random.default_rng(4).integers(-3000, 3001, (2, code.n))]).astype(np.int32)
    ref = WM.minsum_decode(WM.ModelCode.from_code(code), llr, 12, 10, 12, 0, max_iter=3)
    assert_same(run(dec, llr, torch_dev), ref, code.n, where="array(107, 3) flooding")


def test_layered_goes_global_by_size(F, torch_dev):
    """The partition code [100] * 600 in 4 layers: n = 60,000, m = 2,400, L = 600; 2 n + 16 + 19 m = 165,616 B
    is beyond 160 KiB for any check state of 18 bytes or more (W = 4: 24 bytes)."""
    profile, layers = [100] * 600, 4
    code = F.Code.parse(D.partition_alist(profile, layers))
    assert (code.n, code.m, code.dc_max) == (60000, 2400, 100) and 2 * code.n + 16 + 19 * code.m > 160 * 1024
    dec = F.LayeredDecoder(code, check="minsum", layer_checks=600, post_bits=12, msg_bits=10, scale_16=14, offset=2, max_iter=3)
    assert "mem=global" in dec.describe()
    check_describe(dec, "lms", (12, 10, 14, 2), "global", 600)
    llr = np.concatenate([np.rint(np.random.default_rng(5).normal(60, 40, (3, code.n))),
                          np.random.default_rng(6).integers(-3000, 3001, (2, code.n))]).astype(np.int32)
    ref = WM.layered_minsum_decode(WM.ModelCode.from_code(code), llr, 600, 12, 10, 14, 2, max_iter=3)
    assert_same(run(dec, llr, torch_dev), ref, code.n, where="[100] * 600 layered")


# ---- (v) simulation ----

SIM = dict(seed=123456789, first_frame=37, max_frames=256, max_frame_errors=0, chunk=64, device_channel=True,
           random_info=True, info_seed=24681357)


@pytest.fixture(scope="module")
def array67(F):
    code = F.Code.array(67, 3)
    return code, F.Encoder.from_code(code)


def sim_decoder(F, kind, code):
    ms = dict(post_bits=10, msg_bits=8, scale_16=13, offset=3, max_iter=7)
    dec = F.MinSumDecoder(code, **ms) if kind == "fms" else F.LayeredDecoder(code, check="minsum", **ms)
    assert "_minsum_wide<DC=96," in dec.describe(), dec.describe()
    return dec


@pytest.mark.parametrize("kind", KINDS)
def test_simulation_equals_its_restatement(F, torch_dev, array67, kind):
    """ber_sim on a p > 64 array code (two chunks in flight: the twin decoder copies the wide choice) against the same
    chunks decoded with decode_torch and counted against info_bits and the encoder; then once with a harvest."""
    import torch
    code, enc = array67
    eb, frames, first = 5.0, SIM["max_frames"], SIM["first_frame"]
    snr, sigma = F.snr_sigma(eb, code.rate)
    info = F.info_bits(SIM["info_seed"], first, frames, enc.k)
    cw = enc.encode(info)
    cw_t = torch.from_numpy(cw).to(torch_dev)
    llr = torch.empty((frames, code.n), dtype=torch.int16, device=torch_dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=torch_dev)
    F.channel_llr_ptrs(SIM["seed"], first, frames, code.n, snr, sigma, 4, cw_t.data_ptr(), 1, llr.data_ptr(), F.FPLDPC_LLR_I16,
                       ovf.data_ptr(), torch.cuda.current_stream(torch_dev).cuda_stream)
    out = sim_decoder(F, kind, code).decode_torch(llr)
    torch.cuda.synchronize()
    assert int(ovf.cpu()[0]) == 0
    hard = F.unpack_hard(out["hard"].cpu().numpy(), code.n)
    blk, its = (hard[:, enc.info_index] != info).sum(axis=1), out["iters"].cpu().numpy()
    want = dict(bit_errors=int(blk.sum()), frame_errors=int((blk > 0).sum()), frames=frames, iter_sum=int(its.sum()))
    seen = []
    r = sim_decoder(F, kind, code).ber_sim(snr, sigma, on_frame=lambda *a: seen.append(a), **SIM)
    print(kind, want)
    assert {k: r[k] for k in want} == want
    assert seen == [(first + f, int(its[f]), int(blk[f])) for f in range(frames)]
    res = sim_decoder(F, kind, code).ber_sim(snr, sigma, harvest=8, **SIM)
    assert {k: res[k] for k in want} == want
    want_hv = HM.harvest(hard, cw, code.lists()[3], its, blk, first_frame=first, max_records=8)
    assert want_hv["counts"]["codeword_errors"] > 8  # on the restatement alone: records are dropped
    HM.assert_equal(res["harvest"], want_hv, kind)


# ---- (vi) refusals ----

def test_degree_256_is_refused(F, torch_dev):
    from float_truth import star_alist
    code = F.Code.parse(star_alist([2, 256]))
    assert code.dc_max == 256
    for create_it in (lambda: F.MinSumDecoder(code), lambda: F.LayeredDecoder(code, check="minsum", layer_checks=1, post_bits=12, msg_bits=10)):
        with pytest.raises(F.FpldpcError, match="above 255") as e:
            create_it()
        assert e.value.code == -4, e.value
    ok = F.Code.parse(star_alist([2, 255]))
    assert "flood_minsum_wide<DC=256," in F.MinSumDecoder(ok).describe()


def test_sxor_layered_decoder_still_refuses_reg65(F, torch_dev):
    with pytest.raises(F.FpldpcError) as e:
        F.LayeredDecoder(family_code(F, "reg65"), layer_checks=5)
    assert e.value.code == -4, e.value
