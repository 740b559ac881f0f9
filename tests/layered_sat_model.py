"""numpy model of the saturated layered schedule -- a test helper, not a test.

The definition (include/fpldpc.h, fpldpc_layered_create_sat; DESIGN.md "Saturated layered decoder"):
with S_p = 2^(post_bits-1) - 1, S_m = 2^(msg_bits-1) - 1, clamp(x, S) = min(max(x, -S), S), per frame
    post[v] = clamp(LLR[v], S_p);  c2v[c][k] = 0
    for it = 1 .. max_iter, for each check c in code order:
        t[k] = clamp(post[v_k] - c2v[c][k], S_m);  new = fold(t);  c2v[c][k] = new[k]
        post[v_k] = clamp(t[k] + new[k], S_p)
with the sxor, the fold and the code of layered_model.py, and everything else (hard decision,
syndrome, iterations, early termination, precheck on the clamped LLRs) as layered_decode there.
Defined for every input: every run asserts the bounds the definition gives, |c2v| and every fold value
<= S_m + C and |post| <= S_p, and in registers |post - c2v| <= S_p + S_m + C, |t + new| <= 2 S_m + C.
`clipped` counts the values a clamp changed, `c2v_peak` is the largest |c2v| (and fold value) seen.
"""
import numpy as np

from layered_model import ModelCode, check_update, constant, sxor  # noqa: F401 (sxor: the arithmetic this model runs on)


def limits(post_bits, msg_bits, frac_bits=4):
    """(S_p, S_m, C) after the creation rule of the library."""
    C = constant(frac_bits)
    assert 2 <= msg_bits < post_bits <= 24, (post_bits, msg_bits)
    Sp, Sm = (1 << (post_bits - 1)) - 1, (1 << (msg_bits - 1)) - 1
    assert Sp > Sm + C, (Sp, Sm, C)
    return Sp, Sm, C


def _clamp(x, S):
    y = np.clip(x, -S, S)
    return y, int((y != x).sum())


def layered_sat_decode(mc, llr, L, post_bits, msg_bits, max_iter=30, frac_bits=4, mask=0xFF, early_term=True,
                       precheck=False):
    Sp, Sm, C = limits(post_bits, msg_bits, frac_bits)
    llr = np.asarray(llr).astype(np.int64)
    B, m = llr.shape[0], mc.m
    assert llr.shape[1] == mc.n and L >= 1 and m % L == 0
    layers = []
    for lo in range(0, m, L):
        g = mc.groups(lo, lo + L)
        vs = np.concatenate([v.ravel() for _, _, v in g])
        assert len(np.unique(vs)) == len(vs), "a variable occurs twice inside a layer"
        layers.append(g)
    post, clipped = _clamp(llr, Sp)
    c2v = np.zeros((B, m, mc.clist.shape[1]), np.int64)
    iters = np.zeros(B, np.int32)
    pre = mc.syndrome_ok(post) if precheck else np.zeros(B, bool)
    act = ~pre
    c2v_peak = 0
    for it in range(1, max_iter + 1):
        idx = np.nonzero(act)[0]
        if not idx.size:
            break
        P, Cv = post[idx], c2v[idx]
        for g in layers:
            for rows, d, vs in g:
                raw = P[:, vs] - Cv[:, rows, :d]
                assert np.abs(raw).max() <= Sp + Sm + C
                t, n1 = _clamp(raw, Sm)
                new, pk = check_update(t, C, mask)
                assert pk <= Sm + C, (pk, Sm, C)  # every fold value and every c2v
                c2v_peak = max(c2v_peak, pk)
                Cv[:, rows, :d] = new
                q = t + new
                assert np.abs(q).max() <= 2 * Sm + C
                P[:, vs], n2 = _clamp(q, Sp)
                clipped += n1 + n2
        assert np.abs(P).max() <= Sp
        post[idx], c2v[idx] = P, Cv
        iters[idx] = it
        if early_term:
            act[idx[mc.syndrome_ok(P)]] = False
    assert np.abs(c2v).max() <= Sm + C and np.abs(post).max() <= Sp
    return {"iters": iters, "hard": (post <= 0).astype(np.uint8), "post": post,
            "syndrome_ok": mc.syndrome_ok(post).astype(np.uint8), "clipped": clipped, "c2v_peak": c2v_peak,
            "prechecked": pre}
