"""Every check-degree edge and every addressing form of the five decoders built on fpldpc_layered_device.hpp --
layered_generic (unsaturated), layered_sat with int16 and with int32 state, layered_minsum, flood_minsum and
the two mem=global forms -- against the numpy models of their definitions: iterations, hard decisions,
syndrome flags and posteriors exactly.

The codes (tests/degree_family.py) put a degree at, below and above every bucket of the kernels' DC = 8 / 16 /
32 / 48 / 64 and the exact 47 into codes of a few hundred variables that are no array codes, so every one
reads the index table; `mix` holds all of them in one 16-lane layer.  Each runs in every form below, and each
form is pinned by its whole describe() string -- kernel, DC, c2v=, addr=, deg=, mem=, threads= and the LDS
bytes that the layout comment of its kernel gives -- so a silently substituted form fails the test.  What the
inputs reach (every slot the first minimum with either sign, the clamps, the iteration spread, int32) is
pinned on the CPU in tests/test_degree_family.py, not here.

Forms: the sxor decoders with c2v and the table in LDS, the table global, and c2v global; the two min-sum
decoders with the table in LDS, the table global, and the state global.  All decode families (a), (b), (d)
and (e) in one batch; family (c) runs with early termination on the first placement of each kind and, for the
saturating kinds, without it on the last.  At 16/15
with plain min-sum on (a) // 4 no clamp acts, and the flooding min-sum decoder must also give what the
oracle's restatement of the reference and the library's own flooding decoder give at frac_bits = 0."""
import re

import numpy as np
import pytest

import degree_family as D
from conftest import assert_same
from test_gpu_layered_sat import run

pytestmark = pytest.mark.gpu

KEYS = ("iters", "hard", "syndrome_ok", "post")
# id -> (kind, model parameters, switches besides the placement's)
FORMS = {
    "unsat": ("unsat", (), {}),
    "sat16": ("sat", (12, 10), {}),
    "sat32": ("sat", (20, 12), {}),
    "sat12as32": ("sat", (12, 10), {"FPLDPC_LAYERED_STATE": "i32"}),
    "lms14-2": ("lms", (12, 10, 14, 2), {}),
    "lms16-0": ("lms", (12, 10, 16, 0), {}),
    "fms14-2": ("fms", (12, 10, 14, 2), {}),
    "fms16-0": ("fms", (12, 10, 16, 0), {}),
}
# 16/15 with plain min-sum: no clamp acts on (a) // 4 (the flooding min-sum decoder against the oracle)
WIDE = {"fms16/15": ("fms", (16, 15, 16, 0), {})}
ONE_PER_KIND = ("unsat", "sat16", "sat32", "lms14-2", "fms14-2")
PLACEMENTS = ("lds_table", "global_table", "global")
SWITCH = {
    # (C2V=lds: a saturated decoder whose c2v leaves one workgroup per CU -- mix with int32 state, 82 KB -- would
    # else move it to the global scratch by its own rule)
    "sxor": {"lds_table": {"FPLDPC_LAYERED_C2V": "lds", "FPLDPC_LAYERED_TABLE": "lds"},
             "global_table": {"FPLDPC_LAYERED_C2V": "lds", "FPLDPC_LAYERED_TABLE": "global"},
             "global": {"FPLDPC_LAYERED_C2V": "global"}},
    "lms": {"lds_table": {"FPLDPC_LAYERED_TABLE": "lds"}, "global_table": {"FPLDPC_LAYERED_TABLE": "global"},
            "global": {"FPLDPC_LAYERED_MINSUM_STATE": "global"}},
    "fms": {"lds_table": {"FPLDPC_MINSUM_TABLE": "lds"}, "global_table": {"FPLDPC_MINSUM_TABLE": "global"},
            "global": {"FPLDPC_MINSUM_STATE": "global"}},
}


def up(x, to):
    return -(-x // to) * to


def kernel_of(name):
    """(DC, deg=) of the code's kernels: the straight-line 47 for a regular degree-47 code, else the first
    bucket that holds dc_max, predicated."""
    profile = D.CODES[name][0]
    if set(profile) == {47}:
        return 47, "exact"
    return next(x for x in (8, 16, 32, 48, 64) if max(profile) <= x), "table"


def test_kernels_the_issue_names():
    assert kernel_of("reg47") == (47, "exact") and kernel_of("near47") == kernel_of("reg48") == (48, "table")
    assert [kernel_of(f"reg{d}")[0] for d in D.REG_DEGREES] == [8, 8, 16, 16, 32, 32, 48, 47, 48, 64, 64, 64]
    assert kernel_of("mix") == (64, "table")


def expected_describe(name, form, placement):
    """The describe() string of the form, as a regular expression (grid and device are the machine's)."""
    kind, params, extra = {**FORMS, **WIDE}[form]
    profile, layers = D.CODES[name]
    n, L, m = sum(profile), len(profile), len(profile) * layers
    dc, deg = kernel_of(name)
    edges, degs = max(profile) * m, 0 if deg == "exact" else m
    vec16 = (2 * n + 3) // 4 * 4  # n int16, up to a whole word
    table = 2 * edges if placement == "lds_table" else 0
    addr = "table" if placement == "lds_table" else "gtable"
    scratch = ""
    if kind in ("unsat", "sat"):
        # post [n] | misc [4] | c2v [dc_max][m] | vidx [dc_max][m] uint16 | cdeg [m]
        state = 2 if kind == "sat" and params[0] <= 16 and not extra else 4
        lds = up(n * state, 4) + 16 + degs + (0 if placement == "global" else edges * state + table)
        kern = (f"layered_{'generic' if kind == 'unsat' else 'sat'}<DC={dc},c2v={'global' if placement == 'global' else 'lds'},"
                f"addr={addr},deg={deg}> L={L} layers={layers}")
        tail = "" if kind == "unsat" else f" sat={params[0]}/{params[1]} state={'i16' if state == 2 else 'i32'}"
        threads = 64
    else:
        flood = kind == "fms"
        tail = f" sat={params[0]}/{params[1]} ms={params[2]}/16-{params[3]} state=compressed"
        threads = min(256, up(m, 64)) if flood else 64
        mem = ""
        if placement == "global":
            # vec [n] int16 | misc [4] | cdeg [m]; a slice: state [m] uint4 (| acc [3][n] int32), to 256 bytes
            lds, mem = vec16 + 16 + degs, ",mem=global"
            scratch = up(16 * m + (12 * n if flood else 0), 256)
        elif flood:
            # state [m] uint4 | acc [3][n] int32 | llr [n] int16 | misc [4] | vidx | cdeg
            lds = 16 * m + 12 * n + vec16 + 16 + table + degs
        else:
            # post [n] int16 | misc [4] | (to 16 bytes) state [m] uint4 | vidx | cdeg
            lds = up(vec16 + 16, 16) + 16 * m + table + degs
        kern = f"{'flood' if flood else 'layered'}_minsum<DC={dc},addr={addr},deg={deg}{mem}>" + ("" if flood else f" L={L} layers={layers}")
    at = kern.index(" ") if " " in kern else len(kern)
    kern = re.escape(kern[:at]) + kern[at:]
    return rf"{kern} grid=(\d+) threads={threads} lds={lds} device=\d+{re.escape(tail)}" + (r" scratch=(\d+)" if scratch else ""), scratch


_CODES = {}


def family_code(F, name):
    if name not in _CODES:
        _CODES[name] = F.Code.parse(D.alist_of(name))
    return _CODES[name]


def create(F, monkeypatch, name, form, placement, **kw):
    """The decoder of the form, its switches set around creation only; its describe() string must be the form's.
    Returns the decoder and its grid."""
    kind, params, extra = {**FORMS, **WIDE}[form]
    env = {**SWITCH["sxor" if kind in ("unsat", "sat") else kind][placement], **extra}
    code = family_code(F, name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        if kind == "fms":
            dec = F.MinSumDecoder(code, post_bits=params[0], msg_bits=params[1], scale_16=params[2], offset=params[3],
                                  **{"max_iter": D.MAX_ITER, **kw})
        elif kind == "lms":
            dec = F.LayeredDecoder(code, check="minsum", layer_checks=D.layer_size(name), post_bits=params[0], msg_bits=params[1],
                                   scale_16=params[2], offset=params[3], **{"max_iter": D.MAX_ITER, **kw})
        elif kind == "sat":
            dec = F.LayeredDecoder(code, layer_checks=D.layer_size(name), post_bits=params[0], msg_bits=params[1],
                                   **{"max_iter": D.MAX_ITER, **kw})
        else:
            dec = F.LayeredDecoder(code, layer_checks=D.layer_size(name), **{"max_iter": D.MAX_ITER_UNSAT, **kw})
    finally:
        for k in env:
            monkeypatch.delenv(k)
    d = dec.describe()
    want, slice_bytes = expected_describe(name, form, placement)
    got = re.fullmatch(want, d)
    assert got, f"{name} {form} {placement}: {d!r} is not {want!r}"
    grid = int(got.group(1))
    assert 0 < grid < 100000, d
    if slice_bytes:
        assert int(got.group(2)) == grid * slice_bytes, d
    return dec, grid


def test_describe_strings_the_issue_names():
    """reg47: deg=exact through a table; near47 and reg48: the predicated DC = 48."""
    for placement, addr in (("lds_table", "addr=table"), ("global_table", "addr=gtable"), ("global", "addr=gtable")):
        for form in FORMS:
            assert "DC=47," in expected_describe("reg47", form, placement)[0]
            assert addr in expected_describe("reg47", form, placement)[0] and "deg=exact" in expected_describe("reg47", form, placement)[0]
            for name in ("near47", "reg48"):
                want = expected_describe(name, form, placement)[0]
                assert "DC=48," in want and "deg=table" in want and addr in want


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", D.NAMES)
def test_form(F, torch_dev, monkeypatch, name, form, placement):
    """Families (a), (b), (d) and (e) in one batch."""
    kind, params, _ = FORMS[form]
    dec, _ = create(F, monkeypatch, name, form, placement)
    ref = D.reference(name, kind, params)
    assert_same(run(dec, D.inputs(name, kind), torch_dev), ref, dec.code.n, where=f"{name} {form} {placement}")


@pytest.mark.parametrize("form", ONE_PER_KIND)
@pytest.mark.parametrize("name", D.NAMES)
def test_noisy_frames_with_early_termination(F, torch_dev, monkeypatch, name, form):
    """Family (c): frames of one batch stop after different numbers of iterations."""
    kind, params, _ = FORMS[form]
    dec, _ = create(F, monkeypatch, name, form, "lds_table")
    ref = D.reference(name, kind, params, "c")
    assert_same(run(dec, D.inputs(name, kind, "c"), torch_dev), ref, dec.code.n, where=f"{name} {form} noisy")


@pytest.mark.parametrize("form", [f for f in ONE_PER_KIND if f != "unsat"])
@pytest.mark.parametrize("name", D.NAMES)
def test_noisy_frames_without_early_termination(F, torch_dev, monkeypatch, name, form):
    """The same frames to the last iteration: converged frames go on through every slot.  (Not the unsaturated
    decoder: a converged frame's posteriors go on doubling with every layer, out of int32 on mix.)"""
    kind, params, _ = FORMS[form]
    dec, _ = create(F, monkeypatch, name, form, "global", early_term=False)
    ref = D.reference(name, kind, params, "c", early_term=False)
    assert_same(run(dec, D.inputs(name, kind, "c"), torch_dev), ref, dec.code.n, where=f"{name} {form} noisy, no early termination")


@pytest.fixture(scope="module")
def oracle_refs(O):
    """The oracle's flooding decode of (a) // 4 at frac_bits = 0, once per code."""
    made = {}

    def get(name):
        if name not in made:
            ocode = O.OracleCode.from_alist_text(D.alist_of(name))
            made[name] = O.decode_batch(ocode, D.inputs(name, "fms", "q"), D.MAX_ITER, 0, 0xFF)
        return made[name]
    return get


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", D.NAMES)
def test_plain_min_sum_is_the_reference_flooding_decoder(F, torch_dev, monkeypatch, oracle_refs, name, placement):
    """16/15, plain min-sum, (a) // 4: no clamp acts (test_degree_family.py), so the flooding min-sum decoder
    computes the reference's flooding decode with C = 0 -- the oracle's, and the library's flooding decoder's,
    which takes every code of the family."""
    dec, _ = create(F, monkeypatch, name, "fms16/15", placement)
    llr = D.inputs(name, "fms", "q")
    out = run(dec, llr, torch_dev)
    where = f"{name} 16/15 {placement}"
    assert_same(out, D.reference(name, "fms", WIDE["fms16/15"][1], "q"), dec.code.n, where=where + " vs the model")
    assert_same(out, oracle_refs(name), dec.code.n, where=where + " vs the oracle")
    if placement == PLACEMENTS[0]:
        flooding = F.Decoder(dec.code, max_iter=D.MAX_ITER, frac_bits=0)  # accepted: a creation error fails the test
        assert flooding.describe().startswith("flood_"), flooding.describe()
        assert_same(run(flooding, llr, torch_dev), oracle_refs(name), dec.code.n, where=where + ": flooding decoder vs the oracle")


# ---- mix only: the frame framework around the widest, most irregular kernel ----

@pytest.mark.parametrize("form", ONE_PER_KIND)
def test_mix_more_frames_than_the_grid(F, torch_dev, monkeypatch, form):
    """The resident grid plus 3 frames, state in global memory: a workgroup's second frame starts from zero
    state in the slice its first one used."""
    kind, params, _ = FORMS[form]
    dec, grid = create(F, monkeypatch, "mix", form, "global")
    llr, ref = D.inputs("mix", kind), D.reference("mix", kind, params)
    sel = np.tile(np.arange(len(llr)), -(-(grid + 3) // len(llr)))[:grid + 3]
    big = {k: ref[k][sel] for k in KEYS}
    assert_same(run(dec, llr[sel], torch_dev), big, dec.code.n, where=f"mix {form} batch {grid + 3}")


@pytest.mark.parametrize("form", ONE_PER_KIND)
def test_mix_two_calls_on_a_stream(F, torch_dev, monkeypatch, form):
    import torch
    kind, params, _ = FORMS[form]
    dec, _ = create(F, monkeypatch, "mix", form, "lds_table")
    t = torch.from_numpy(D.inputs("mix", kind)).to(torch_dev)
    s = torch.cuda.Stream(torch_dev)
    torch.cuda.synchronize()
    outs = [dec.decode_torch(t, post=True, stream=s), dec.decode_torch(t, post=True, stream=s)]
    s.synchronize()
    for out in outs:
        assert_same({k: v.cpu().numpy() for k, v in out.items()}, D.reference("mix", kind, params), dec.code.n, where=f"mix {form} stream")


@pytest.mark.parametrize("form", ONE_PER_KIND)
def test_mix_int16_and_int32_llr(F, torch_dev, monkeypatch, form):
    kind, params, _ = FORMS[form]
    dec, _ = create(F, monkeypatch, "mix", form, "global_table")
    llr = D.inputs("mix", kind)
    assert np.abs(llr).max() <= 32767
    a, b = run(dec, llr, torch_dev, np.int16), run(dec, llr, torch_dev, np.int32)
    assert_same(a, D.reference("mix", kind, params), dec.code.n, where=f"mix {form} int16")
    for k in KEYS:
        assert (a[k] == b[k]).all(), k
