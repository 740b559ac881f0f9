"""What tests/test_gpu_minsum_wide.py rests on, pinned on the CPU with the numpy models alone: the widened models
(tests/minsum_wide_model.py) are the shipped ones wherever those run, the wide family (tests/wide_family.py)
parses as built, and its inputs reach what they are there for -- on every regular code every slot becomes the
first minimum k1 and carries both signs (so the first and the last bit of every sign word hold live values),
the clamps act on family (b), and the noisy family stops its frames after different numbers of iterations in both
schedules.  The GPU tests assert none of this on the code under test."""
import numpy as np
import pytest

import degree_family as D
import layered_minsum_model as MS
import minsum_model as FM
import minsum_wide_model as WM
import wide_family as W

MS_PARAMS = (12, 10, 14, 2)
KEYS = ("iters", "hard", "syndrome_ok", "post", "clipped")


@pytest.mark.parametrize("name", ["reg47", "reg64", "near47", "mix"])
def test_widened_models_are_the_shipped_ones(name):
    mc, L = D.model_code(name), D.layer_size(name)
    llr = np.concatenate([D.uniform300(name)[:24], D.uniform3000(name)[:8], D.noisy(name)[:8], D.constants(name)[0]])
    for precheck in (False, True):
        a = MS.layered_minsum_decode(mc, llr, L, *MS_PARAMS, max_iter=D.MAX_ITER, precheck=precheck)
        b = WM.layered_minsum_decode(mc, llr, L, *MS_PARAMS, max_iter=D.MAX_ITER, precheck=precheck)
        c = FM.minsum_decode(mc, llr, *MS_PARAMS, max_iter=D.MAX_ITER, precheck=precheck)
        d = WM.minsum_decode(mc, llr, *MS_PARAMS, max_iter=D.MAX_ITER, precheck=precheck)
        for k in KEYS:
            assert (np.asarray(a[k]) == np.asarray(b[k])).all() and (np.asarray(c[k]) == np.asarray(d[k])).all(), k


def test_the_family_is_the_one_of_the_issue():
    assert [n for n in W.NAMES if n.startswith("reg")] == [f"reg{d}" for d in (
        65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 223, 224, 225, 254, 255)]
    assert all(W.CODES[f"reg{d}"] == ([d] * 5, 3) for d in W.REG_DEGREES)
    assert max(W.size(n) for n in W.NAMES if n.startswith("reg")) == 1275
    profile, layers = W.CODES["mixw"]
    assert min(profile) == 2 and max(profile) == 255 and sum(d <= 64 for d in profile) >= 5 and layers >= 3
    assert profile != profile[::-1]  # a lane's degree changes between layers
    # every sign-word count of the kernel occurs among the regular codes
    assert {-(-d // 32) for d in W.REG_DEGREES} == {3, 4, 5, 6, 7, 8}


@pytest.mark.parametrize("name", W.NAMES)
def test_code_is_what_the_builder_made(F, name):
    profile, layers = W.CODES[name]
    rows, L = W.rows_of(name), len(profile)
    code = F.Code.parse(W.alist_of(name))
    assert (code.n, code.m, code.dv_max, code.dc_max) == (sum(profile), L * layers, layers, max(profile))
    _, cdeg, _, clist = code.lists()
    assert list(cdeg) == [len(r) for r in rows] and list(cdeg[:L]) == profile and list(cdeg[L:2 * L]) == profile[::-1]
    for c, r in enumerate(rows):
        assert list(clist[c, :len(r)]) == list(r), c
    assert code.layering(L) == (L, layers)


def covered(k1, s, d):
    return set(np.unique(k1).tolist()) == set(range(d)) and s.any(axis=(0, 1)).all() and (~s).any(axis=(0, 1)).all()


@pytest.mark.parametrize("name", [n for n in W.NAMES if n.startswith("reg")])
def test_family_a_makes_every_slot_the_first_minimum(name, monkeypatch):
    """At S_m = 511 and 256 frames: in the flooding decoder's first step, and in the first iteration of the
    layered one (recorded from the model)."""
    rows, llr = W.rows_of(name), W.uniform300(name)
    assert len(llr) == 256
    for d, (k1, s) in D.first_minima(rows, llr, 2047, 511).items():
        assert covered(k1, s, d), f"{name}: flooding, degree {d}"
    seen = {}
    update = WM.check_update

    def recording(t, scale_16, offset):
        new, state = update(t, scale_16, offset)
        seen.setdefault(t.shape[-1], []).append((state[2], state[3]))
        return new, state
    monkeypatch.setattr(WM, "check_update", recording)
    WM.layered_minsum_decode(W.model_code(name), llr, W.layer_size(name), *MS_PARAMS, max_iter=1)
    assert sorted(seen) == sorted(set(W.CODES[name][0]))
    for d, got in seen.items():
        k1, s = np.concatenate([g[0] for g in got], axis=1), np.concatenate([g[1] for g in got], axis=1)
        assert covered(k1, s, d), f"{name}: layered, degree {d}"


@pytest.mark.parametrize("name", W.NAMES)
def test_family_b_makes_the_clamps_act(name):
    for kind in ("lms", "fms"):
        full = W.reference(name, kind, MS_PARAMS)
        assert full["clipped"] > 0, kind
    mc, llr = W.model_code(name), W.uniform3000(name)[:8]
    assert WM.layered_minsum_decode(mc, llr, W.layer_size(name), *MS_PARAMS, max_iter=2)["clipped"] > 0
    assert WM.minsum_decode(mc, llr, *MS_PARAMS, max_iter=2)["clipped"] > 0


@pytest.mark.parametrize("name", W.NAMES)
def test_noisy_family_spreads_the_iteration_counts(name):
    for kind in ("lms", "fms"):
        it = W.reference(name, kind, MS_PARAMS, "c")["iters"]
        assert len(it) == W.NOISE_FRAMES and len(set(it.tolist())) >= 2, (kind, sorted(set(it.tolist())))


@pytest.mark.parametrize("name", W.NAMES)
def test_constant_frames_meet_the_precheck(name):
    """Family (e): some frames pass the channel pre-check (0 iterations) and some do not."""
    for kind in ("lms", "fms"):
        pre = W.reference(name, kind, MS_PARAMS, "e", precheck=True)["prechecked"]
        assert pre.any() and not pre.all()


def test_plain_min_sum_at_16_15_clamps_nothing_on_reg129():
    assert W.reference("reg129", "fms", (16, 15, 16, 0), "q")["clipped"] == 0
