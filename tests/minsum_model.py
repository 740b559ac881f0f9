"""numpy model of the flooding min-sum decoder -- a test helper, not a test.

The definition (include/fpldpc.h, fpldpc_minsum_create; DESIGN.md "Flooding min-sum decoder"): with
S_p = 2^(post_bits-1) - 1, S_m = 2^(msg_bits-1) - 1, clamp(x, S) = min(max(x, -S), S) and
f(x) = max(((x * scale_16) >> 4) - offset, 0) for x >= 0, per frame
    L[v] = clamp(LLR[v], S_p);  post[v] = L[v];  c2v[c][k] = 0
    for it = 1 .. max_iter:
        for every check c, all reading the same post:
            t[k]   = clamp(post[v_k] - c2v[c][k], S_m)
            new[k] = the min-sum rule of layered_minsum_model.check_update;  c2v[c][k] = new[k]
        for every variable v:  post[v] = clamp(L[v] + sum of c2v over v's edges, S_p)
        hard[v] = post[v] > 0 ? 0 : 1;  syndrome;  iters = it;  with early_term stop on a pass
and precheck on the clamped LLRs.  Vectorised over frames and over all checks of one degree.

Every run asserts the bounds the definition gives -- |c2v| <= S_m, |post| <= S_p, |post - c2v| <= S_p + S_m,
|L + sum| <= S_p + dv_max * S_m -- and, on every check update, that the compressed state the kernel keeps,
(f(m1), f(m2), k1, sign word), rebuilds the stored messages (layered_minsum_model.rebuild).
`clipped` counts the values a clamp changed: 0 means no clamp acted.
"""
import numpy as np

from layered_minsum_model import _clamp, check_update, limits, rebuild
from layered_model import ModelCode  # noqa: F401 (callers build their codes through this module too)


def minsum_decode(mc, llr, post_bits, msg_bits, scale_16=16, offset=0, max_iter=30, early_term=True, precheck=False):
    Sp, Sm = limits(post_bits, msg_bits, scale_16, offset)
    llr = np.asarray(llr).astype(np.int64)
    B, m, dcm = llr.shape[0], mc.m, mc.clist.shape[1]
    assert llr.shape[1] == mc.n and dcm <= 64
    groups = mc.groups(0, m)
    dv_max = int(np.bincount(mc.clist[mc.clist >= 0].ravel(), minlength=mc.n).max())
    L, clipped = _clamp(llr, Sp)
    post = L.copy()
    c2v = np.zeros((B, m, dcm), np.int64)
    # the compressed state: all zero is the frame's initial state (every message rebuilds to 0)
    sM1, sM2, sk1 = (np.zeros((B, m), np.int64) for _ in range(3))
    ssg = np.zeros((B, m, dcm), bool)
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
            old = Cv[:, rows, :d]
            again = rebuild((sM1[idx][:, rows], sM2[idx][:, rows], sk1[idx][:, rows], ssg[idx][:, rows, :d]), d)
            assert (again == old).all(), "compressed state does not rebuild the stored messages"
            raw = P[:, vs] - old
            assert np.abs(raw).max() <= Sp + Sm
            t, n1 = _clamp(raw, Sm)
            new, (M1, M2, k1, s) = check_update(t, scale_16, offset)
            assert np.abs(new).max() <= Sm
            Cv[:, rows, :d] = new
            sM1[np.ix_(idx, rows)], sM2[np.ix_(idx, rows)], sk1[np.ix_(idx, rows)] = M1, M2, k1
            ssg[np.ix_(idx, rows, np.arange(d))] = s
            np.add.at(acc, (f, vs[None]), new)
            clipped += n1
        assert np.abs(acc).max() <= Sp + dv_max * Sm
        P, n2 = _clamp(acc, Sp)
        clipped += n2
        post[idx], c2v[idx] = P, Cv
        iters[idx] = it
        if early_term:
            act[idx[mc.syndrome_ok(P)]] = False
    assert np.abs(c2v).max() <= Sm and np.abs(post).max() <= Sp
    assert sM1.max() <= Sm and sM2.max() <= Sm and sM1.min() >= 0 and (sM1 <= sM2).all()
    return {"iters": iters, "hard": (post <= 0).astype(np.uint8), "post": post,
            "syndrome_ok": mc.syndrome_ok(post).astype(np.uint8), "clipped": clipped, "prechecked": pre}
