"""The degree-edge family of codes and inputs -- a test helper, not a test.

The kernels of the layered and min-sum decoders are instantiated per check-degree bucket (DC = 8 / 16 / 32 /
48 / 64, and the straight-line 47).  A "partition code" puts any list of check degrees into one layer: each
layer is a seeded random partition of the n = sum(profile) variables into len(profile) checks, check j of the
layer with degree profile[j] (the profile reversed on odd layers, so a lane's degree changes between layers),
rows ascending, every variable of degree `layers`.  L = len(profile) is a valid layer size by construction,
and no such code is a forward array code (n is no square), so every one is addressed through the index table.

CODES: reg<d> at every bucket edge and either side of it, near47 (dc_max 47, not regular: the predicated
DC = 48, not the exact 47) and mix, whose 16-lane layers hold every edge degree side by side and whose 320
checks make the flooding decoder's second pass a partial one.  tests/test_degree_family.py pins what the GPU
tests of tests/test_gpu_degree_edges.py rest on (every slot of every degree becomes k1, clamps act, ...).
"""
import numpy as np

SEED = 7
MIX_PROFILE = [2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
REG_DEGREES = (2, 8, 9, 16, 17, 32, 33, 47, 48, 49, 63, 64)
# name -> (profile, layers)
CODES = {f"reg{d}": ([d] * 5, 3) for d in REG_DEGREES}
CODES["near47"] = ([46, 47, 47, 46, 47], 3)
CODES["mix"] = (MIX_PROFILE, 20)
NAMES = tuple(CODES)

# Frames of the random families: 256 on the small codes.  mix: the fewest (in steps of 8) at which family (a)
# still makes every slot of every degree the first minimum in both schedules (test_degree_family.py rechecks it).
FRAMES = {name: 256 for name in CODES}
FRAMES["mix"] = 24
# Family (c): sigma of rint(N(60, sigma)) per code, found on the CPU with the numpy models alone (the grid 10, 14,
# 18, 22, 26, 30, 35, 40, 50, 60, 80 at 32 frames: a sigma at which the iteration counts of every decoder kind
# take at least two values); test_degree_family.py asserts that spread.
NOISE_FRAMES = 32
SIGMA = {"reg2": 80, "reg8": 35, "reg9": 35, "reg16": 30, "reg17": 30, "reg32": 26, "reg33": 26, "reg47": 22,
         "reg48": 26, "reg49": 26, "reg63": 26, "reg64": 26, "near47": 26, "mix": 40}


def partition_rows(profile, layers, seed=SEED):
    """The checks of the partition code, layer after layer: ascending int arrays."""
    n = sum(profile)
    rs = np.random.default_rng(seed)
    rows = []
    for l in range(layers):
        perm = rs.permutation(n)
        at = 0
        for d in (profile[::-1] if l & 1 else profile):
            rows.append(np.sort(perm[at:at + d]))
            at += d
        assert at == n
    return rows


def partition_alist(profile, layers, seed=SEED):
    """alist text (0-based, as Code.parse reads it) of the partition code."""
    n, rows = sum(profile), partition_rows(profile, layers, seed)
    cols = [[] for _ in range(n)]
    for c, r in enumerate(rows):
        for v in r:
            cols[int(v)].append(c)
    assert all(len(c) == layers for c in cols)
    lines = [f"{n} {len(rows)}", f"{layers} {max(profile)}", " ".join([str(layers)] * n), " ".join(str(len(r)) for r in rows)]
    lines += [" ".join(map(str, c)) for c in cols] + [" ".join(map(str, r)) for r in rows]
    return "\n".join(lines) + "\n"


def rows_of(name):
    return partition_rows(*CODES[name])


def alist_of(name):
    return partition_alist(*CODES[name])


def layer_size(name):
    return len(CODES[name][0])


def _rng(name, family):
    return np.random.default_rng([SEED, NAMES.index(name), ord(family)])


def uniform300(name):
    """(a) uniform in +-300, zeros present."""
    n = sum(CODES[name][0])
    x = _rng(name, "a").integers(-300, 301, (FRAMES[name], n)).astype(np.int32)
    assert (x == 0).any()
    return x


def uniform3000(name):
    """(b) uniform in +-3000: beyond S_p = 2047 and S_m = 511, every clamp acts."""
    n = sum(CODES[name][0])
    return _rng(name, "b").integers(-3000, 3001, (FRAMES[name], n)).astype(np.int32)


def noisy(name, sigma=None):
    """(c) the all-zero codeword at LLR 60 in Gaussian noise, rounded."""
    n = sum(CODES[name][0])
    return np.rint(_rng(name, "c").normal(60, SIGMA[name] if sigma is None else sigma, (NOISE_FRAMES, n))).astype(np.int32)


TIE_SCALES = (1, 3, 40, 300, 1500)


def ties(name):
    """(d) values from {-2 .. 2} * s, s per frame from TIE_SCALES: most minima are attained more than once."""
    n, frames = sum(CODES[name][0]), FRAMES[name]
    s = np.array(TIE_SCALES)[np.arange(frames) % len(TIE_SCALES)]
    return (_rng(name, "d").integers(-2, 3, (frames, n)) * s[:, None]).astype(np.int32)


def constants(name, big=True):
    """(e) constant frames: 0, -5, +5, (big) -32767, +32767, and per check degree of the code one frame that is
    +40 but -40 exactly on the first check of that degree.  Returns the frames and, per frame, a label."""
    profile, _ = CODES[name]
    n, rows = sum(profile), rows_of(name)
    vals = [0, -5, 5] + ([-32767, 32767] if big else [])
    out, label = [np.full(n, v, np.int32) for v in vals], [f"all {v}" for v in vals]
    for d in sorted(set(profile)):
        x = np.full(n, 40, np.int32)
        x[next(r for r in rows if len(r) == d)] = -40
        out.append(x)
        label.append(f"check of degree {d} negative")
    return np.stack(out), label


def first_minima(rows, llr, Sp, Sm):
    """Per check degree d: (k1 [frames][checks of degree d], s [frames][checks][d]) of the first update of a
    flooding step, t = clamp(clamp(LLR, S_p), S_m) -- and of the first layer of a layered one."""
    out = {}
    post = np.clip(np.asarray(llr, np.int64), -Sp, Sp)
    for d in sorted({len(r) for r in rows}):
        vs = np.stack([r for r in rows if len(r) == d])
        t = np.clip(post[:, vs], -Sm, Sm)
        out[d] = (np.abs(t).argmin(axis=-1), t <= 0)
    return out


# ---- the batch every form decodes, and its model results ----

def model_code(name):
    """The code as the numpy models read it, from the builder's rows (no library involved)."""
    from layered_model import ModelCode
    rows = rows_of(name)
    clist = np.full((len(rows), max(map(len, rows))), -1, np.int64)
    for c, r in enumerate(rows):
        clist[c, :len(r)] = r
    return ModelCode(sum(CODES[name][0]), [len(r) for r in rows], clist)


def batch(name, unsaturated=False):
    """Families (a), (b), (d) and (e) in one batch, and the slice of each.  The unsaturated decoder is defined
    while every intermediate fits int32 and a constant frame doubles with every layer until its first syndrome,
    so on mix (20 layers: 32767 * 2^20 > 2^31) it gets (e) without the two frames at +-32767."""
    parts = {"a": uniform300(name), "b": uniform3000(name), "d": ties(name),
             "e": constants(name, big=not (unsaturated and name == "mix"))[0]}
    at, where = 0, {}
    for k, x in parts.items():
        where[k] = slice(at, at + len(x))
        at += len(x)
    return np.concatenate(list(parts.values())), where


MAX_ITER = 8        # the saturating decoders
MAX_ITER_UNSAT = 4  # the unsaturated one: posteriors stay far inside int32 (test_degree_family.py)
_REFS = {}


def reference(name, kind, params=(), family=None, **kw):
    """The numpy model's result, computed once and kept read-only.  kind / params: "unsat" (), "sat" (post_bits,
    msg_bits), "lms" / "fms" (post_bits, msg_bits, scale_16, offset): the layered / flooding min-sum decoder.
    family None: batch(name); "c": noisy(name); "q": uniform300(name) // 4."""
    import layered_minsum_model as MS
    import layered_model as M
    import layered_sat_model as S
    import minsum_model as FM
    key = (name, kind, tuple(params), family, tuple(sorted(kw.items())))
    if key not in _REFS:
        mc, L = model_code(name), layer_size(name)
        llr = inputs(name, kind, family)
        if kind == "unsat":
            r = M.layered_decode(mc, llr, L, **{"max_iter": MAX_ITER_UNSAT, **kw})
        elif kind == "sat":
            r = S.layered_sat_decode(mc, llr, L, *params, **{"max_iter": MAX_ITER, **kw})
        elif kind == "lms":
            r = MS.layered_minsum_decode(mc, llr, L, *params, **{"max_iter": MAX_ITER, **kw})
        else:
            assert kind == "fms", kind
            r = FM.minsum_decode(mc, llr, *params, **{"max_iter": MAX_ITER, **kw})
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def inputs(name, kind, family=None):
    if family == "c":
        return noisy(name)
    if family == "q":
        return uniform300(name) // 4
    assert family is None, family
    return batch(name, kind == "unsat")[0]
