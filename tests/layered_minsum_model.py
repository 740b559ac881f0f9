"""numpy model of the layered min-sum decoder -- a test helper, not a test.

The definition (include/fpldpc.h, fpldpc_layered_create_minsum; DESIGN.md "Layered min-sum decoder"):
with S_p = 2^(post_bits-1) - 1, S_m = 2^(msg_bits-1) - 1, clamp(x, S) = min(max(x, -S), S) and
f(x) = max(((x * scale_16) >> 4) - offset, 0) for x >= 0, per frame
    post[v] = clamp(LLR[v], S_p);  c2v[c][k] = 0
    for it = 1 .. max_iter, for each check c in code order:
        t[k]   = clamp(post[v_k] - c2v[c][k], S_m)
        s[k]   = t[k] <= 0
        m1     = min_k |t[k]|,  k1 = a slot attaining it,  m2 = min_{k != k1} |t[k]|
        mag[k] = f(k == k1 ? m2 : m1)
        new[k] = (parity of s[j] over j != k) ? -mag[k] : mag[k]
        c2v[c][k] = new[k];  post[v_k] = clamp(t[k] + new[k], S_p)
and everything else (hard decision, syndrome, iterations, early termination, precheck on the clamped
LLRs) as layered_model.layered_decode.  Vectorised over frames and the checks of a layer.

Every run asserts the bounds the definition gives -- |c2v| <= S_m, |post| <= S_p, |post - c2v| <=
S_p + S_m, |t + new| <= 2 S_m -- and runs a second path beside the direct one: the per-check state the
kernel keeps, (f(m1), f(m2), k1, sign word), from which every c2v[c][k] is rebuilt as magnitude
k == k1 ? f(m2) : f(m1) with sign parity ^ s[k]; the rebuilt messages must equal the stored ones.
"""
import numpy as np

from layered_model import ModelCode  # noqa: F401 (callers build their codes through this module too)


def limits(post_bits, msg_bits, scale_16=16, offset=0):
    """(S_p, S_m) after the creation rule of the library."""
    assert 2 <= msg_bits < post_bits <= 16, (post_bits, msg_bits)
    Sp, Sm = (1 << (post_bits - 1)) - 1, (1 << (msg_bits - 1)) - 1
    assert 1 <= scale_16 <= 16 and 0 <= offset <= Sm, (scale_16, offset)
    return Sp, Sm


def correct(x, scale_16, offset):
    """f(x) for x >= 0: 0 <= f(x) <= x."""
    y = np.maximum(((x * scale_16) >> 4) - offset, 0)
    assert (y >= 0).all() and (y <= x).all()
    return y


def check_update(t, scale_16, offset):
    """t [..., deg] -> (new [..., deg], state): state = (M1, M2, k1, s) with s [..., deg] the sign bits."""
    deg = t.shape[-1]
    assert deg >= 2
    a = np.abs(t)
    s = t <= 0
    k1 = a.argmin(axis=-1)  # the first slot attaining the minimum; any other changes nothing (then m2 = m1)
    m1 = np.take_along_axis(a, k1[..., None], -1)[..., 0]
    own = np.arange(deg) == k1[..., None]
    m2 = np.where(own, np.iinfo(np.int64).max, a).min(axis=-1)
    M1, M2 = correct(m1, scale_16, offset), correct(m2, scale_16, offset)
    mag = np.where(own, M2[..., None], M1[..., None])
    neg = (s.sum(axis=-1) & 1)[..., None] ^ s
    return np.where(neg, -mag, mag), (M1, M2, k1, s)


def rebuild(state, deg):
    """Every c2v of checks of degree deg from their compressed state."""
    M1, M2, k1, s = state
    mag = np.where(np.arange(deg) == k1[..., None], M2[..., None], M1[..., None])
    neg = (s.sum(axis=-1) & 1)[..., None] ^ s
    return np.where(neg, -mag, mag)


def _clamp(x, S):
    y = np.clip(x, -S, S)
    return y, int((y != x).sum())


def layered_minsum_decode(mc, llr, L, post_bits, msg_bits, scale_16=16, offset=0, max_iter=30, early_term=True,
                          precheck=False):
    Sp, Sm = limits(post_bits, msg_bits, scale_16, offset)
    llr = np.asarray(llr).astype(np.int64)
    B, m, dcm = llr.shape[0], mc.m, mc.clist.shape[1]
    assert llr.shape[1] == mc.n and L >= 1 and m % L == 0 and dcm <= 64
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
