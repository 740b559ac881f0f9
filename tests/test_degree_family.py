"""What tests/test_gpu_degree_edges.py rests on, pinned on the CPU with the numpy models alone: the family of
tests/degree_family.py parses as built, and its inputs reach what they are there for -- every slot of every
check degree becomes the first minimum k1 and carries both signs (so slot 32, the first bit of the sign
word's high half, slot 63, its top bit, and the last slot of every bucket hold live values), frames take
different numbers of iterations, the clamps act on family (b), the unsaturated decoder stays inside int32, and
at 16/15 no clamp acts, where the flooding min-sum decoder is the reference's flooding decoder with C = 0.
The GPU tests assert none of this on the code under test."""
import math

import numpy as np
import pytest

import degree_family as D
import layered_minsum_model as MS
import layered_model as M
import layered_sat_model as S
import minsum_model as FM

MS_PARAMS = (12, 10, 14, 2)
KEYS = ("iters", "hard", "syndrome_ok", "post")


@pytest.mark.parametrize("name", D.NAMES)
def test_code_is_what_the_builder_made(F, name):
    profile, layers = D.CODES[name]
    rows, L = D.rows_of(name), len(profile)
    code = F.Code.parse(D.alist_of(name))
    assert (code.n, code.m, code.dv_max, code.dc_max) == (sum(profile), L * layers, layers, max(profile))
    vdeg, cdeg, _, clist = code.lists()
    assert (vdeg == layers).all() and list(cdeg) == [len(r) for r in rows]
    assert list(cdeg[:L]) == profile and list(cdeg[L:2 * L]) == profile[::-1]
    for c, r in enumerate(rows):
        assert (np.diff(r) > 0).all() and list(clist[c, :len(r)]) == list(r), c
    assert code.layering(L) == (L, layers)
    assert code.regular_checks == (len(set(profile)) == 1)
    # a forward array code has n = p * p (detect_array, fpldpc_code.cpp); and no layer size is found for these
    assert math.isqrt(code.n) ** 2 != code.n and code.layering() == (1, code.m)
    mc, lib_mc = D.model_code(name), M.ModelCode.from_code(code)
    assert (mc.cdeg == lib_mc.cdeg).all() and (mc.pad == lib_mc.pad).all()


def test_the_family_is_the_one_of_the_issue():
    assert [n for n in D.NAMES if n.startswith("reg")] == [f"reg{d}" for d in (2, 8, 9, 16, 17, 32, 33, 47, 48, 49, 63, 64)]
    assert all(D.CODES[f"reg{d}"] == ([d] * 5, 3) for d in D.REG_DEGREES)
    assert D.CODES["near47"] == ([46, 47, 47, 46, 47], 3)
    profile, layers = D.CODES["mix"]
    assert profile == [2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64] and layers == 20
    assert (sum(profile), len(profile) * layers) == (444, 320)  # flooding: one full pass of 256 lanes and one of 64
    assert D.FRAMES["mix"] < 256 and all(D.FRAMES[n] == 256 for n in D.NAMES if n != "mix")


def covered(k1, s, d):
    return set(np.unique(k1).tolist()) == set(range(d)) and s.any(axis=(0, 1)).all() and (~s).any(axis=(0, 1)).all()


@pytest.mark.parametrize("name", D.NAMES)
def test_family_a_makes_every_slot_the_first_minimum(name, monkeypatch):
    """At S_m = 511, at the frame count the GPU tests use: in the flooding decoder's first step, and in the
    first iteration of the layered one (whose later layers read updated posteriors: recorded from the model)."""
    rows, llr = D.rows_of(name), D.uniform300(name)
    assert len(llr) == D.FRAMES[name]
    for d, (k1, s) in D.first_minima(rows, llr, 2047, 511).items():
        assert covered(k1, s, d), f"{name}: flooding, degree {d}"
    seen = {}
    update = MS.check_update

    def recording(t, scale_16, offset):
        new, state = update(t, scale_16, offset)
        seen.setdefault(t.shape[-1], []).append((state[2], state[3]))
        return new, state
    monkeypatch.setattr(MS, "check_update", recording)
    MS.layered_minsum_decode(D.model_code(name), llr, D.layer_size(name), *MS_PARAMS, max_iter=1)
    assert sorted(seen) == sorted(set(D.CODES[name][0]))
    for d, got in seen.items():
        k1, s = np.concatenate([g[0] for g in got], axis=1), np.concatenate([g[1] for g in got], axis=1)
        assert covered(k1, s, d), f"{name}: layered, degree {d}"
    if name == "mix":  # the smallest count in steps of 8: 16 frames miss a slot
        few = D.first_minima(rows, llr[:16], 2047, 511)
        assert not all(covered(k1, s, d) for d, (k1, s) in few.items())


@pytest.mark.parametrize("name", D.NAMES)
def test_family_a_takes_several_iterations_and_some_frame_fails(name):
    mc, llr = D.model_code(name), D.uniform300(name)[:64]
    for r in (MS.layered_minsum_decode(mc, llr, D.layer_size(name), *MS_PARAMS, max_iter=D.MAX_ITER),
              FM.minsum_decode(mc, llr, *MS_PARAMS, max_iter=D.MAX_ITER)):
        assert (r["iters"] > 1).any() and not r["syndrome_ok"].all()


def saturating(mc, llr, L):
    return {"sat 12/10": S.layered_sat_decode(mc, llr, L, 12, 10, max_iter=D.MAX_ITER),
            "sat 20/12": S.layered_sat_decode(mc, llr, L, 20, 12, max_iter=D.MAX_ITER),
            "layered min-sum": MS.layered_minsum_decode(mc, llr, L, *MS_PARAMS, max_iter=D.MAX_ITER),
            "flooding min-sum": FM.minsum_decode(mc, llr, *MS_PARAMS, max_iter=D.MAX_ITER)}


@pytest.mark.parametrize("name", D.NAMES)
def test_family_b_makes_the_clamps_act(name):
    """On 32 of its frames already, in every saturating model."""
    for what, r in saturating(D.model_code(name), D.uniform3000(name)[:32], D.layer_size(name)).items():
        assert r["clipped"] > 0, what


def test_family_a_alone_would_not():
    """Why (b) is there: at degree 32 the minimum of 32 values within +-300 is small, and no clamp at
    S_p = 2047 / S_m = 511 ever acts on family (a)."""
    r = saturating(D.model_code("reg32"), D.uniform300("reg32"), 5)
    assert [r[k]["clipped"] for k in ("sat 12/10", "layered min-sum", "flooding min-sum")] == [0, 0, 0]


@pytest.mark.parametrize("name", D.NAMES)
def test_unsaturated_decoder_stays_inside_int32(name):
    r = D.reference(name, "unsat")
    assert r["peak"] < 2 ** 31
    llr, where = D.batch(name, unsaturated=True)
    assert len(r["iters"]) == len(llr) and np.abs(llr[where["b"]]).max() > 2047
    if name == "mix":  # the two frames it does not get leave int32 inside the first iteration
        big = D.constants(name)[0][3:5]
        assert (np.abs(big) == 32767).all() and len(llr) == len(D.batch(name)[0]) - 2
        assert M.layered_decode(D.model_code(name), big, D.layer_size(name), max_iter=1)["peak"] >= 2 ** 31


@pytest.mark.parametrize("name", D.NAMES)
def test_plain_min_sum_at_16_15_is_the_reference_flooding_decoder_with_c_0(name):
    """Inputs (a) // 4, plain min-sum (16/16 - 0): no clamp acts, and then every output is that of the
    reference's flooding schedule over its own sxor at frac_bits = 0 (C = 0: sxor is the signed minimum)."""
    r = D.reference(name, "fms", (16, 15, 16, 0), "q")
    assert r["clipped"] == 0
    ref = M.flooding_decode(D.model_code(name), D.inputs(name, "fms", "q"), max_iter=D.MAX_ITER, frac_bits=0)
    for k in KEYS:
        assert (r[k] == ref[k]).all(), k
    assert ref["peak"] < 2 ** 15


@pytest.mark.parametrize("name", D.NAMES)
def test_noisy_family_spreads_the_iteration_counts(name):
    """Family (c) at the code's sigma: every decoder kind stops its frames after different numbers of iterations."""
    for kind, params in (("unsat", ()), ("sat", (12, 10)), ("sat", (20, 12)), ("lms", MS_PARAMS), ("fms", MS_PARAMS)):
        r = D.reference(name, kind, params, "c")
        it = r["iters"]
        assert kind != "unsat" or r["peak"] < 2 ** 31
        assert len(it) == D.NOISE_FRAMES and len(set(it.tolist())) >= 2, (kind, params, sorted(set(it.tolist())))
