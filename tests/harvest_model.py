"""The harvest of a BER simulation (include/fpldpc.h, fpldpc_harvest_t) stated in numpy: for hard decisions
hard [B][n], the sent word(s) cw (None = all-zero, [n] shared, [B][n] per frame) and the code's clist [m][dc]
(-1 padded),
    e = hard XOR cw, weight = |e|;  s[k] = parity of hard over check k's clist, unsat = |s|
and from the frames in order: the records of the first max_records frames with weight > 0, the six counts and
the (weight, unsat) classes over all frames."""
import numpy as np

COUNTS = ("frames", "codeword_errors", "detected", "undetected", "recorded", "dropped")
FIELDS = ("frame", "iters", "info_errors", "weight", "unsat", "err", "syn")


def pack(bits):
    """[B][k] bits -> uint32 [B][ceil(k / 32)], bit v % 32 of word v // 32, bits at or above k zero."""
    bits = np.asarray(bits, np.uint8)
    B, k = bits.shape
    words = (k + 31) // 32
    padded = np.zeros((B, words * 32), np.uint8)
    padded[:, :k] = bits
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint32).reshape(B, words)


def scan(hard, cw, clist):
    """(weight [B], unsat [B], e [B][n], s [B][m]) of hard [B][n] bits."""
    hard = np.asarray(hard, np.uint8) & 1
    clist = np.asarray(clist)
    e = hard ^ (0 if cw is None else (np.asarray(cw, np.uint8) & 1))  # [n] broadcasts over the frames
    take = hard[:, np.where(clist < 0, 0, clist)]                     # [B][m][dc]
    s = (take * (clist >= 0)).sum(axis=2) & 1
    return e.sum(axis=1).astype(np.int32), s.sum(axis=1).astype(np.int32), e.astype(np.uint8), s.astype(np.uint8)


def harvest(hard, cw, clist, iters, blk, first_frame=0, max_records=1 << 20):
    """{records: {field: array}, counts: {name: int}, classes: {(weight, unsat): frames}} of the frames in order."""
    w, u, e, s = scan(hard, cw, clist)
    bad = np.nonzero(w > 0)[0]
    keep = bad[:max_records]
    records = {"frame": (first_frame + keep).astype(np.int64), "iters": np.asarray(iters, np.int32)[keep],
               "info_errors": np.asarray(blk, np.int32)[keep], "weight": w[keep], "unsat": u[keep],
               "err": pack(e[keep]), "syn": pack(s[keep])}
    counts = dict(frames=len(w), codeword_errors=len(bad), detected=int((u[bad] > 0).sum()),
                  undetected=int((u[bad] == 0).sum()), recorded=len(keep), dropped=len(bad) - len(keep))
    classes = {}
    for a, b in sorted(zip(w[bad].tolist(), u[bad].tolist())):
        classes[(a, b)] = classes.get((a, b), 0) + 1
    return {"records": records, "counts": counts, "classes": classes}


def assert_equal(hv, want, where=""):
    """A filled fixedpointldpc_amd.Harvest against harvest()'s result: every record field, counts, classes."""
    assert hv.counts == want["counts"], (where, hv.counts, want["counts"])
    got = hv.classes
    assert got == want["classes"] and list(got) == sorted(got), (where, got, want["classes"])
    for k in FIELDS:
        g, w = getattr(hv, k), want["records"][k]
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), (where, k)
