"""The packed A kernel's range guard from two chain values (fpldpc_flood_checks_array.hpp ArrayChecks::kChainGuard).

Property: with L = (deg - 1) // 2, F the forward and B the backward chain of the reference's fold,
    max_k |c2v_k| <= max(|F_{L-1}|, |B_{L+1}|) + (L + 1) * C,
which follows from |x [+] y| <= min(|x|, |y|) + C.  The kernel ORs (F_{L-1} + G) | (B_{L+1} + G), G =
(L + 1) C, into its range accumulator instead of every output magnitude; the bound is what makes that
flag every frame the per-output form flags.  CPU only (numpy), the fold as tests/layered_model.py's.
"""
import ctypes

import numpy as np
import pytest

from layered_model import sxor

PARAMS = [(10, 0xFF), (5, 0x3F), (160, 0xFF), (2560, 0xFFFF)]


def fold(t, C, mask):
    """t [rows][deg] v2c -> (fwd, bwd, c2v), the reference's serial forward / backward fold."""
    deg = t.shape[-1]
    fwd = np.empty_like(t)
    bwd = np.empty_like(t)
    fwd[:, 0] = t[:, 0]
    bwd[:, deg - 1] = t[:, deg - 1]
    for k in range(1, deg):
        fwd[:, k] = sxor(fwd[:, k - 1], t[:, k], C, mask)
        bwd[:, deg - 1 - k] = sxor(bwd[:, deg - k], t[:, deg - 1 - k], C, mask)
    new = np.empty_like(t)
    new[:, 0] = bwd[:, 1]
    new[:, deg - 1] = fwd[:, deg - 2]
    new[:, 1:deg - 1] = sxor(fwd[:, :deg - 2], bwd[:, 2:], C, mask)
    return fwd, bwd, new


def inputs(deg, rng):
    """Magnitudes in [0, 2^15) with random signs: uniform, small, all-equal rows, and rows that sit
    just under / at / over the A threshold 4096 and the other packed thresholds."""
    rows = [rng.integers(0, 1 << 15, (400, deg)), rng.integers(0, 64, (200, deg)), rng.integers(0, 700, (200, deg))]
    for v in (0, 1, 9, 10, 11, 255, 256, 4095, 4096, 32767):
        rows.append(np.full((1, deg), v))
    for thr in (512, 2048, 4096, 8192):
        rows.append(thr + rng.integers(-300, 301, (200, deg)))
        one = rng.integers(0, 40, (100, deg))  # one large input among small ones
        one[np.arange(100), rng.integers(0, deg, 100)] = thr + rng.integers(-5, 6, 100)
        rows.append(one)
    mag = np.concatenate(rows).astype(np.int64)
    sign = rng.choice([-1, 1], mag.shape)
    return mag * sign


@pytest.mark.parametrize("deg", [47, 8])
@pytest.mark.parametrize("C,mask", PARAMS)
def test_chain_values_bound_every_output(deg, C, mask):
    rng = np.random.default_rng(deg * 100003 + C)
    t = inputs(deg, rng)
    fwd, bwd, new = fold(t, C, mask)
    L = (deg - 1) // 2
    # the box-plus bound the derivation starts from, on every fold step taken
    assert (np.abs(fwd[:, 1:]) <= np.minimum(np.abs(fwd[:, :-1]), np.abs(t[:, 1:])) + C).all()
    assert (np.abs(bwd[:, :-1]) <= np.minimum(np.abs(bwd[:, 1:]), np.abs(t[:, :-1])) + C).all()
    bound = np.maximum(np.abs(fwd[:, L - 1]), np.abs(bwd[:, L + 1])) + (L + 1) * C
    worst = np.abs(new).max(axis=1)
    assert (worst <= bound).all(), (deg, C, mask, int((worst - bound).max()))
    # per side, as the derivation states it
    assert (np.abs(new[:, L:]).max(axis=1) <= np.abs(fwd[:, L - 1]) + (L + 1) * C).all()
    assert (np.abs(new[:, :L + 1]).max(axis=1) <= np.abs(bwd[:, L + 1]) + (L + 1) * C).all()


@pytest.mark.parametrize("deg", [47, 8])
@pytest.mark.parametrize("C,mask", PARAMS)
def test_guard_word_flags_whenever_an_output_does(deg, C, mask):
    """The flag as the kernel forms it, for every power-of-two threshold a packed kernel can have:
    (F + G) | (B + G) has a bit at or above 2^b whenever some |c2v| >= 2^b."""
    rng = np.random.default_rng(deg * 7919 + C)
    t = inputs(deg, rng)
    fwd, bwd, new = fold(t, C, mask)
    L = (deg - 1) // 2
    G = (L + 1) * C
    word = (np.abs(fwd[:, L - 1]) + G) | (np.abs(bwd[:, L + 1]) + G)
    worst = np.abs(new).max(axis=1)
    for b in range(9, 15):
        over = worst >= (1 << b)
        assert ((word >> b) != 0)[over].all(), (deg, C, b)
        if C == 10 and deg == 47 and b == 12:
            assert over.any() and (~over).any()  # the inputs sit on both sides of A's threshold


def test_chooser_rule(F):
    """choose_kernel's rule (fpldpc_testing_range_guard, no device needed): the chain guard while
    G = (L + 1) C <= (cmax + 1) / 8, the per-output form beyond."""
    lib = F.lib()

    def ask(dv, C, slots=24):
        cg = ctypes.c_int32(-1)
        cmax = lib.fpldpc_testing_range_guard(dv, C, slots, ctypes.byref(cg))
        return cmax, cg.value

    # A (p47 / r5: dv 5): cmax 4095; FRAC 4 / 3 take the chain guard, FRAC 8 and 12 do not
    assert ask(5, 10) == (4095, 1)
    assert ask(5, 5) == (4095, 1)
    assert ask(5, 160) == (4095, 0)
    assert ask(5, 2560)[1] == 0
    # p47 / r2 (dv 2): cmax 8191
    assert ask(2, 10) == (8191, 1)
    assert ask(2, 160) == (8191, 0)
    # the boundary itself: 24 * C <= 512 <=> C <= 21
    assert ask(5, 21)[1] == 1 and ask(5, 22)[1] == 0
    for dv in (1, 2, 5, 12, 24):
        for C in (1, 5, 10, 20, 21, 22, 40, 80, 160, 640, 2560):
            cmax, cg = ask(dv, C)
            assert cg == int(cmax > 0 and 24 * C <= (cmax + 1) // 8), (dv, C, cmax, cg)
