"""The wide degree family: partition codes (tests/degree_family.py's builder, imported) with check degrees above
64, and their inputs -- a test helper, not a test.

The wide form of the min-sum decoders (fpldpc_minsum_wide.hip) walks a check 32 slots -- one sign word -- at a
time, so the edges are the multiples of 32: reg<d>, profile [d] * 5 in 3 layers, for every d at, below and above
each sign-word edge from 65 to 255 (n = 1275 at most), and mixw, whose 25-lane layers hold degrees from 2 to
255 side by side (degrees <= 64 among them), the profile reversed on odd layers so a lane's degree changes
between layers.  The input families are degree_family's (a) .. (e), drawn here for these codes.
tests/test_minsum_wide_model.py pins what tests/test_gpu_minsum_wide.py rests on.
"""
import numpy as np

import degree_family as D
import minsum_wide_model as WM
from layered_model import ModelCode

SEED = 11
REG_DEGREES = (65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 223, 224, 225, 254, 255)
MIXW_PROFILE = [2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 223, 224, 225, 254, 255]
# name -> (profile, layers)
CODES = {f"reg{d}": ([d] * 5, 3) for d in REG_DEGREES}
CODES["mixw"] = (MIXW_PROFILE, 4)
NAMES = tuple(CODES)
# frames of family (a): 256 on the regular codes (every slot the first minimum, test_minsum_wide_model.py);
# families (b) and (d), which have no slot to reach, take a quarter of them
FRAMES = {name: 256 for name in CODES}
FRAMES["mixw"] = 16
NOISE_FRAMES = 32
SIGMA = 22  # family (c): rint(N(60, SIGMA)); test_minsum_wide_model.py asserts the spread of the iteration counts
MAX_ITER = 8


def rows_of(name):
    return D.partition_rows(*CODES[name])


def alist_of(name):
    return D.partition_alist(*CODES[name])


def layer_size(name):
    return len(CODES[name][0])


def size(name):
    return sum(CODES[name][0])


def _rng(name, family):
    return np.random.default_rng([SEED, NAMES.index(name), ord(family)])


def uniform300(name):
    """(a) uniform in +-300, zeros present."""
    x = _rng(name, "a").integers(-300, 301, (FRAMES[name], size(name))).astype(np.int32)
    assert (x == 0).any()
    return x


def uniform3000(name):
    """(b) uniform in +-3000: beyond S_p = 2047 and S_m = 511."""
    return _rng(name, "b").integers(-3000, 3001, (FRAMES[name] // 4, size(name))).astype(np.int32)


def noisy(name):
    """(c) the all-zero codeword at LLR 60 in Gaussian noise, rounded."""
    return np.rint(_rng(name, "c").normal(60, SIGMA, (NOISE_FRAMES, size(name)))).astype(np.int32)


def ties(name):
    """(d) values from {-2 .. 2} * s, s per frame from degree_family.TIE_SCALES."""
    frames = FRAMES[name] // 4
    s = np.array(D.TIE_SCALES)[np.arange(frames) % len(D.TIE_SCALES)]
    return (_rng(name, "d").integers(-2, 3, (frames, size(name))) * s[:, None]).astype(np.int32)


def constants(name):
    """(e) constant frames 0, -5, +5, -32767, +32767, and per check degree one frame that is +40 but -40 exactly on
    the first check of that degree."""
    n, rows = size(name), rows_of(name)
    out = [np.full(n, v, np.int32) for v in (0, -5, 5, -32767, 32767)]
    for d in sorted(set(CODES[name][0])):
        x = np.full(n, 40, np.int32)
        x[next(r for r in rows if len(r) == d)] = -40
        out.append(x)
    return np.stack(out)


def batch(name):
    """Families (a), (b), (d) and (e) in one batch."""
    return np.concatenate([uniform300(name), uniform3000(name), ties(name), constants(name)])


def inputs(name, family=None):
    if family == "c":
        return noisy(name)
    if family == "e":
        return constants(name)
    if family == "q":
        return uniform300(name) // 4
    assert family is None, family
    return batch(name)


def model_code(name):
    """The code as the numpy models read it, from the builder's rows (no library involved)."""
    rows = rows_of(name)
    clist = np.full((len(rows), max(map(len, rows))), -1, np.int64)
    for c, r in enumerate(rows):
        clist[c, :len(r)] = r
    return ModelCode(size(name), [len(r) for r in rows], clist)


_REFS = {}


def reference(name, kind, params, family=None, **kw):
    """The widened model's result, computed once and kept read-only.  kind "lms" / "fms": the layered / flooding
    min-sum decoder with params (post_bits, msg_bits, scale_16, offset); family as inputs()."""
    key = (name, kind, tuple(params), family, tuple(sorted(kw.items())))
    if key not in _REFS:
        mc, llr = model_code(name), inputs(name, family)
        if kind == "lms":
            r = WM.layered_minsum_decode(mc, llr, layer_size(name), *params, **{"max_iter": MAX_ITER, **kw})
        else:
            assert kind == "fms", kind
            r = WM.minsum_decode(mc, llr, *params, **{"max_iter": MAX_ITER, **kw})
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]
