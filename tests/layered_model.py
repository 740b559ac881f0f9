"""numpy model of the layered (row-serial) schedule -- a test helper, not a test.

The definition (include/fpldpc.h "layered decoder", DESIGN.md "Layered schedule"): per frame
post[v] = LLR[v], c2v[c][k] = 0; for every iteration and each check c in code order
    t[k] = post[v_k] - c2v[c][k];  new = fold(t);  c2v[c][k] = new[k];  post[v_k] = t[k] + new[k]
with the reference's sxor (oracle/fpldpc_oracle.c:56-67) and forward/backward fold (:117-129), then
hard = post > 0 ? 0 : 1 and the syndrome.  Vectorised over frames and over the checks of a layer (per
degree inside a layer), int64 throughout; frames that stop are frozen.  Every result carries `peak`,
the largest |value| seen: callers assert peak < 2^31, which is a condition on the inputs (the
definition holds while every intermediate fits int32), not a tolerance.
"""
import numpy as np


def constant(frac_bits):
    return int((5.0 / 8.0) * (1 << frac_bits))  # ArrayLDPCMacro.h:175


def sxor(x, y, C, mask):
    x = np.asarray(x, np.int64)
    y = np.asarray(y, np.int64)
    v1, v2 = np.abs(x), np.abs(y)
    part1 = np.maximum(C - (((v1 + v2) & mask) >> 2), 0)
    part2 = np.maximum(C - ((np.abs(v1 - v2) & mask) >> 2), 0)
    sg = np.where(x > 0, 1, -1) * np.where(y > 0, 1, -1)  # sgn(0) = -1
    return sg * (np.minimum(v1, v2) + part1 - part2)


def check_update(t, C, mask):
    """t [..., deg] v2c messages of checks of one degree -> (c2v [..., deg], largest |value|)."""
    deg = t.shape[-1]
    assert deg >= 2
    fwd = np.empty_like(t)
    bwd = np.empty_like(t)
    fwd[..., 0] = t[..., 0]
    bwd[..., deg - 1] = t[..., deg - 1]
    for k in range(1, deg):  # the two chains advance together, as in the reference's loop
        r = sxor(np.stack([fwd[..., k - 1], bwd[..., deg - k]]), np.stack([t[..., k], t[..., deg - 1 - k]]), C, mask)
        fwd[..., k] = r[0]
        bwd[..., deg - 1 - k] = r[1]
    new = np.empty_like(t)
    new[..., 0] = bwd[..., 1]
    new[..., deg - 1] = fwd[..., deg - 2]
    if deg > 2:
        new[..., 1:deg - 1] = sxor(fwd[..., :deg - 2], bwd[..., 2:], C, mask)
    return new, int(max(np.abs(fwd).max(), np.abs(bwd).max(), np.abs(new).max()))


class ModelCode:
    """clist / cdeg of a code (fixedpointldpc_amd.Code.lists()) with the per-degree check groups."""

    def __init__(self, n, cdeg, clist):
        self.n = int(n)
        self.cdeg = np.asarray(cdeg, np.int64)
        self.clist = np.asarray(clist, np.int64)
        self.m = len(self.cdeg)
        self.pad = np.where(self.clist < 0, self.n, self.clist)  # -> an always-0 extra hard bit

    @classmethod
    def from_code(cls, code):
        _, cdeg, _, clist = code.lists()
        return cls(code.n, cdeg, clist)

    def groups(self, lo, hi):
        """[(rows, deg, vars [rows][deg])] of the checks lo .. hi-1, one entry per check degree."""
        out = []
        for d in np.unique(self.cdeg[lo:hi]):
            rows = lo + np.nonzero(self.cdeg[lo:hi] == d)[0]
            out.append((rows, int(d), self.clist[rows, :d]))
        return out

    def syndrome_ok(self, post):
        hard = np.concatenate([post <= 0, np.zeros((post.shape[0], 1), bool)], axis=1)
        return ~(hard[:, self.pad].sum(axis=2) & 1).any(axis=1)


def layered_decode(mc, llr, L, max_iter=30, frac_bits=4, mask=0xFF, early_term=True, precheck=False):
    """The definition, with checks [l*L, (l+1)*L) updated at once (they must share no variable)."""
    C = constant(frac_bits)
    llr = np.asarray(llr).astype(np.int64)
    B, m = llr.shape[0], mc.m
    assert llr.shape[1] == mc.n and L >= 1 and m % L == 0
    layers = []
    for lo in range(0, m, L):
        g = mc.groups(lo, lo + L)
        vs = np.concatenate([v.ravel() for _, _, v in g])
        assert len(np.unique(vs)) == len(vs), "a variable occurs twice inside a layer"
        layers.append(g)
    post = llr.copy()
    c2v = np.zeros((B, m, mc.clist.shape[1]), np.int64)
    iters = np.zeros(B, np.int32)
    pre = mc.syndrome_ok(post) if precheck else np.zeros(B, bool)
    act = ~pre
    peak = int(np.abs(llr).max())
    for it in range(1, max_iter + 1):
        idx = np.nonzero(act)[0]
        if not idx.size:
            break
        P, Cv = post[idx], c2v[idx]
        for g in layers:
            for rows, d, vs in g:
                t = P[:, vs] - Cv[:, rows, :d]
                new, pk = check_update(t, C, mask)
                Cv[:, rows, :d] = new
                P[:, vs] = t + new
                peak = max(peak, pk, int(np.abs(t).max()), int(np.abs(P[:, vs]).max()))
        post[idx], c2v[idx] = P, Cv
        iters[idx] = it
        if early_term:
            act[idx[mc.syndrome_ok(P)]] = False
    return {"iters": iters, "hard": (post <= 0).astype(np.uint8), "post": post,
            "syndrome_ok": mc.syndrome_ok(post).astype(np.uint8), "peak": peak, "prechecked": pre}


def flooding_decode(mc, llr, max_iter=30, frac_bits=4, mask=0xFF):
    """The reference's flooding schedule (oracle/fpldpc_oracle.c:95-159) over the same check_update:
    pins the model's fold and sxor to the oracle."""
    C = constant(frac_bits)
    llr = np.asarray(llr).astype(np.int64)
    B = llr.shape[0]
    g = mc.groups(0, mc.m)
    v2c = [llr[:, vs] for _, _, vs in g]
    post = llr.copy()
    iters = np.zeros(B, np.int32)
    act = np.ones(B, bool)
    peak = int(np.abs(llr).max())
    f = np.arange(B)[:, None, None]
    for it in range(1, max_iter + 1):
        if not act.any():
            break
        c2v = []
        for x in v2c:
            new, pk = check_update(x, C, mask)
            c2v.append(new)
            peak = max(peak, pk)
        nxt = llr.copy()
        for (_, _, vs), new in zip(g, c2v):
            np.add.at(nxt, (f, vs[None]), new)
        post[act] = nxt[act]
        iters[act] = it
        v2c = [np.where(act[:, None, None], nxt[:, vs] - new, old) for (_, _, vs), new, old in zip(g, c2v, v2c)]
        peak = max(peak, int(np.abs(nxt[act]).max()))
        act &= ~mc.syndrome_ok(post)
    return {"iters": iters, "hard": (post <= 0).astype(np.uint8), "post": post,
            "syndrome_ok": mc.syndrome_ok(post).astype(np.uint8), "peak": peak}
