"""numpy models of the two min-sum decoders for check degrees above 64 -- a test helper, not a test.

The decode loops of tests/minsum_model.py (flooding) and tests/layered_minsum_model.py (layered) without their
`dcm <= 64` assertion, nothing else changed: the check rule (check_update), the rebuild of the messages from the
compressed state (rebuild), the parameter rule (limits) and the clamp are the shipped models' own, and none of
them depends on the degree.  tests/test_minsum_wide_model.py pins that these loops equal the shipped ones
wherever those run.
"""
import numpy as np

from layered_minsum_model import _clamp, check_update, limits, rebuild
from layered_model import ModelCode  # noqa: F401 (callers build their codes through this module too)


def minsum_decode(mc, llr, post_bits, msg_bits, scale_16=16, offset=0, max_iter=30, early_term=True, precheck=False):
    Sp, Sm = limits(post_bits, msg_bits, scale_16, offset)
    llr = np.asarray(llr).astype(np.int64)
    B, m, dcm = llr.shape[0], mc.m, mc.clist.shape[1]
    assert llr.shape[1] == mc.n
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


def layered_minsum_decode(mc, llr, L, post_bits, msg_bits, scale_16=16, offset=0, max_iter=30, early_term=True,
                          precheck=False):
    Sp, Sm = limits(post_bits, msg_bits, scale_16, offset)
    llr = np.asarray(llr).astype(np.int64)
    B, m, dcm = llr.shape[0], mc.m, mc.clist.shape[1]
    assert llr.shape[1] == mc.n and L >= 1 and m % L == 0
    layers = []
    for lo in range(0, m, L):
        g = mc.groups(lo, lo + L)
        vs = np.concatenate([v.ravel() for _, _, v in g])
        assert len(np.unique(vs)) == len(vs), "a variable occurs twice inside a layer"
        layers.append(g)
    post, clipped = _clamp(llr, Sp)
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
        St = [x[idx] for x in (sM1, sM2, sk1, ssg)]
        for g in layers:
            for rows, d, vs in g:
                old = Cv[:, rows, :d]
                again = rebuild((St[0][:, rows], St[1][:, rows], St[2][:, rows], St[3][:, rows, :d]), d)
                assert (again == old).all(), "compressed state does not rebuild the stored messages"
                raw = P[:, vs] - old
                assert np.abs(raw).max() <= Sp + Sm
                t, n1 = _clamp(raw, Sm)
                new, (M1, M2, k1, s) = check_update(t, scale_16, offset)
                assert np.abs(new).max() <= Sm
                Cv[:, rows, :d] = new
                St[0][:, rows], St[1][:, rows], St[2][:, rows] = M1, M2, k1
                St[3][:, rows, :d] = s
                q = t + new
                assert np.abs(q).max() <= 2 * Sm
                P[:, vs], n2 = _clamp(q, Sp)
                clipped += n1 + n2
        assert np.abs(P).max() <= Sp
        post[idx], c2v[idx] = P, Cv
        for dst, src in zip((sM1, sM2, sk1, ssg), St):
            dst[idx] = src
        iters[idx] = it
        if early_term:
            act[idx[mc.syndrome_ok(P)]] = False
    assert np.abs(c2v).max() <= Sm and np.abs(post).max() <= Sp
    assert sM1.max() <= Sm and sM2.max() <= Sm and sM1.min() >= 0 and (sM1 <= sM2).all()
    return {"iters": iters, "hard": (post <= 0).astype(np.uint8), "post": post,
            "syndrome_ok": mc.syndrome_ok(post).astype(np.uint8), "clipped": clipped, "prechecked": pre}
