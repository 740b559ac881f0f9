"""numpy model of the saturated flooding decoder -- a test helper, not a test.

The definition (include/fpldpc.h, fpldpc_flood_create_sat; DESIGN.md "Saturated flooding decoder"): with
S_p = 2^(post_bits-1) - 1, S_m = 2^(msg_bits-1) - 1, clamp(x, S) = min(max(x, -S), S) and C the reference's
Constant, per frame
    L[v] = clamp(LLR[v], S_p);  post[v] = L[v];  c2v[c][k] = 0
    for it = 1 .. max_iter:
        for every check c, all reading the same post:
            t[k] = clamp(post[v_k] - c2v[c][k], S_m);  new = fold(t);  c2v[c][k] = new[k]
        for every variable v:  post[v] = clamp(L[v] + sum of c2v over v's edges, S_p)
        hard[v] = post[v] > 0 ? 0 : 1;  syndrome;  iters = it;  with early_term stop on a pass
with the sxor and the forward/backward fold of layered_model.check_update, the limits and the clamp of
layered_sat_model, and precheck on the clamped LLRs.  Vectorised over frames and over all checks of one degree;
frames that stop are frozen.

Every run asserts the four bounds the definition gives -- every fold value and every c2v at most S_m + C,
|post| <= S_p, |post - c2v| <= S_p + S_m + C, |L + sum| <= S_p + dv_max * (S_m + C).  `clipped` counts the
values a clamp changed: 0 means no clamp acted.
"""
import numpy as np

from layered_model import ModelCode, check_update  # noqa: F401 (callers build their codes through this module too)
from layered_sat_model import _clamp, limits


def flood_sat_decode(mc, llr, post_bits, msg_bits, max_iter=30, frac_bits=4, mask=0xFF, early_term=True, precheck=False):
    assert post_bits <= 16, post_bits
    Sp, Sm, C = limits(post_bits, msg_bits, frac_bits)
    llr = np.asarray(llr).astype(np.int64)
    B, m, dcm = llr.shape[0], mc.m, mc.clist.shape[1]
    assert llr.shape[1] == mc.n and dcm <= 64
    groups = mc.groups(0, m)
    dv_max = int(np.bincount(mc.clist[mc.clist >= 0].ravel(), minlength=mc.n).max())
    L, clipped = _clamp(llr, Sp)
    post = L.copy()
    c2v = np.zeros((B, m, dcm), np.int64)
    iters = np.zeros(B, np.int32)
    pre = mc.syndrome_ok(post) if precheck else np.zeros(B, bool)
    act = ~pre
    for it in range(1, max_iter + 1):
        idx = np.nonzero(act)[0]
        if not idx.size:
            break
        P, Cv = post[idx], c2v[idx]
        f = np.arange(len(idx))[:, None, None]
        acc = L[idx].copy()
        for rows, d, vs in groups:
            raw = P[:, vs] - Cv[:, rows, :d]
            assert np.abs(raw).max() <= Sp + Sm + C
            t, n1 = _clamp(raw, Sm)
            new, pk = check_update(t, C, mask)
            assert pk <= Sm + C, (pk, Sm, C)  # every fold value and every c2v
            Cv[:, rows, :d] = new
            np.add.at(acc, (f, vs[None]), new)
            clipped += n1
        assert np.abs(acc).max() <= Sp + dv_max * (Sm + C)
        P, n2 = _clamp(acc, Sp)
        clipped += n2
        post[idx], c2v[idx] = P, Cv
        iters[idx] = it
        if early_term:
            act[idx[mc.syndrome_ok(P)]] = False
    assert np.abs(c2v).max() <= Sm + C and np.abs(post).max() <= Sp
    return {"iters": iters, "hard": (post <= 0).astype(np.uint8), "post": post,
            "syndrome_ok": mc.syndrome_ok(post).astype(np.uint8), "clipped": clipped, "prechecked": pre}
