"""A plain high-precision model of the floating-point BP decoder (fpldpc_decode_float), in mpmath at
50 digits: the truth that tests/test_float_truth.py holds the oracle to and tests/test_gpu_float_paths.py
the kernels.

The flooding schedule of decode_general / orc_decode_float for any code, from Code.lists(): edge init
v2c = LLR; check update; post = LLR + sum of c2v, v2c = post - c2v; hard = post > 0 ? 0 : 1; the
syndrome of the hard decisions after every iteration ends the frame.

The check update is the closed form, not a box-plus chain: the sign of c2v_k is the product over the
other edges of (v > 0 ? +1 : -1) and its magnitude 2 atanh(prod_{j != k} tanh(|v_j| / 2)).  With
phi(x) = -log tanh(x / 2) = 2 atanh(exp(-x)), its own inverse, that magnitude is
phi(sum_{j != k} phi(|v_j|)): the same prefix and suffix products, carried as sums of logarithms.  As
products they could not be evaluated for the inputs these tests use -- tanh(345) is 1 to 50 digits (and
tanh(5e29) to any number of digits), so a check whose other inputs are all large would give atanh(1)
-- while exp(-1e30) is an ordinary mpf (its exponent is an unbounded integer).  check_update_chain is
the reference's forward / backward box-plus chain in the same arithmetic; test_float_truth.py holds the
two to 1e-40 of each other.
"""
import numpy as np
from mpmath import mp, mpf

DPS = 50
BIG = 690.0  # the kernels fold a check holding a message of this magnitude in the log domain


def phi(x):
    """-log tanh(x / 2) for x >= 0, accurate in both tails; phi(0) = +inf, phi(+inf) = 0."""
    if x == 0:
        return mp.inf
    if x == mp.inf:
        return mpf(0)
    return 2 * mp.atanh(mp.exp(-x)) if x >= 1 else -mp.log(mp.tanh(x / 2))


def check_update(v):
    """c2v of one check from its v2c inputs (a list of mpf, degree >= 2), in closed form."""
    d = len(v)
    neg = [0 if x > 0 else 1 for x in v]  # sgn(0) = -1
    par = sum(neg) & 1
    p = [phi(abs(x)) for x in v]
    pre, suf = [mpf(0)] * (d + 1), [mpf(0)] * (d + 1)  # pre[k] = p_0 + .. + p_{k-1}, suf[k] = p_k + .. + p_{d-1}
    for k in range(d):
        pre[k + 1] = pre[k] + p[k]
        suf[d - 1 - k] = suf[d - k] + p[d - 1 - k]
    out = []
    for k in range(d):
        mag = phi(pre[k] + suf[k + 1])
        out.append(-mag if par ^ neg[k] else mag)
    return out


def boxplus(x, y):
    """sxor(double, double) of the reference in mpmath: sgn sgn (min + log(1 + e^-(|x|+|y|)) - log(1 + e^-||x|-|y||))."""
    a, b = abs(x), abs(y)
    r = min(a, b) + mp.log1p(mp.exp(-(a + b))) - mp.log1p(mp.exp(-abs(a - b)))
    return r if (x > 0) == (y > 0) else -r


def check_update_chain(v):
    """The same c2v as the reference folds them: c2v_k = F_{k-1} [+] B_{k+1}."""
    d = len(v)
    F, B = [None] * d, [None] * d
    F[0], B[d - 1] = v[0], v[d - 1]
    for k in range(1, d):
        F[k] = boxplus(F[k - 1], v[k])
        B[d - 1 - k] = boxplus(B[d - k], v[d - 1 - k])
    return [B[1]] + [boxplus(F[k - 1], B[k + 1]) for k in range(1, d - 1)] + [F[d - 2]]


class Graph:
    """The edges of a code from Code.lists(): edge e = off[c] + k is slot k of check c (clist order)."""

    def __init__(self, lists):
        vdeg, cdeg, vlist, clist = lists
        self.n, self.m = len(vdeg), len(cdeg)
        self.cdeg = [int(d) for d in cdeg]
        self.cvars = [[int(x) for x in clist[c, :self.cdeg[c]]] for c in range(self.m)]
        self.off = np.concatenate([[0], np.cumsum(self.cdeg)]).astype(int)
        slot = {}
        for c, vs in enumerate(self.cvars):
            for k, x in enumerate(vs):
                slot[(c, x)] = int(self.off[c]) + k
        # the edges of variable v in vlist order (the order the reference sums them in)
        self.vedges = [[slot[(int(c), v)] for c in vlist[v, :int(vdeg[v])]] for v in range(self.n)]


def decode(graph, llr, max_iter, early_term=True):
    """One frame.  Returns post (mpf list) and post64 (rounded to float64), hard, iters, syndrome_ok,
    min_abs_post (the smallest |post| seen at any syndrome check), big[it] (the set of checks holding an
    input of magnitude >= BIG in iteration it) and history[it] = (post, hard, syndrome_ok) after it + 1
    iterations: while no syndrome passes, a run with a smaller max_iter ends at history[max_iter - 1]."""
    with mp.workdps(DPS):
        g = graph
        L = [mpf(float(x)) for x in llr]
        v2c = [None] * int(g.off[-1])
        for c, vs in enumerate(g.cvars):
            for k, x in enumerate(vs):
                v2c[g.off[c] + k] = L[x]
        c2v = [None] * len(v2c)
        it, ok, min_abs, big, history = 0, False, mp.inf, [], []
        post, hard = L, [0 if x > 0 else 1 for x in L]
        while it < max_iter:
            big.append(set())
            for c in range(g.m):
                a, b = int(g.off[c]), int(g.off[c + 1])
                if max(abs(x) for x in v2c[a:b]) >= BIG:
                    big[-1].add(c)
                c2v[a:b] = check_update(v2c[a:b])
            post = [None] * g.n
            for v in range(g.n):
                acc = mpf(0)
                for e in g.vedges[v]:
                    acc += c2v[e]
                post[v] = acc + L[v]
                for e in g.vedges[v]:
                    v2c[e] = post[v] - c2v[e]
            it += 1
            hard = [0 if x > 0 else 1 for x in post]
            min_abs = min(min_abs, min(abs(x) for x in post))
            ok = not any(sum(hard[x] for x in vs) & 1 for vs in g.cvars)
            history.append((post, np.array(hard, np.uint8), ok))
            if ok and early_term:
                break
        return {"post": post, "post64": np.array([float(x) for x in post]), "hard": np.array(hard, np.uint8), "iters": it,
                "syndrome_ok": ok, "min_abs_post": float(min_abs), "big": big, "history": history}


def E(x, truth):
    """max_v |x_v - truth_v| / (2^-52 max(1, |truth_v|)): the error of float64 posteriors x in ulps of the
    truth (of 1 below 1)."""
    with mp.workdps(DPS):
        u = mpf(2) ** -52
        return float(max(abs(mpf(float(a)) - t) / (u * max(1, abs(t))) for a, t in zip(x, truth)))


# ---------------------------------------------------------------------------------------------------
# The codes and input families of tests/test_float_truth.py and tests/test_gpu_float_paths.py, and their
# truth, computed once per session.

def star_alist(degs):
    """alist text of disjoint checks of the given degrees over consecutive variables (dv = 1)."""
    n, m = sum(degs), len(degs)
    off = np.concatenate([[0], np.cumsum(degs)])
    rows = [range(off[c], off[c + 1]) for c in range(m)]
    lines = [f"{n} {m}", f"1 {max(degs)}", " ".join(["1"] * n), " ".join(map(str, degs))]
    lines += [str(c) for c in range(m) for _ in rows[c]] + [" ".join(map(str, r)) for r in rows]
    return "\n".join(lines) + "\n"


def _irregular(F):
    from test_gpu_layered_sat import irregular_alist
    return F.Code.parse(irregular_alist())


def _rand_deg60(F):
    from test_gpu_codes import CODES
    return CODES["rand_deg60"](F)


# name: (builder, the kernel form Decoder.float_describe() must name, a star code)
CODES = {
    "star47": (lambda F: F.Code.array(47, 1), "bp_float_reg<DC=47,regular,array>", True),
    "array47x2": (lambda F: F.Code.array(47, 2), "bp_float_reg<DC=47,regular,array>", False),
    "array47x2b": (lambda F: F.Code.array(47, 2, forward=False), "bp_float_reg<DC=47,regular,table>", False),
    "star47t": (lambda F: F.Code.parse(star_alist([47] * 6)), "bp_float_reg<DC=47,regular,table>", True),
    "star_small": (lambda F: F.Code.parse(star_alist([2, 3, 4, 5, 6, 7, 8] * 3)), "bp_float_reg<DC=8,predicated,table>", True),
    "irregular": (_irregular, "bp_float_reg<DC=8,predicated,table>", False),
    # (degrees 129 and 255 would suit the float kernel, but no Decoder exists for a check degree above 64)
    "star_generic": (lambda F: F.Code.parse(star_alist([2, 3, 9, 16, 17, 33, 46, 47, 48, 64])), "bp_float_kernel", True),
    "array13x2": (lambda F: F.Code.array(13, 2), "bp_float_kernel", False),
    "rand_deg60": (_rand_deg60, "bp_float_kernel", False),
}
FAMILIES = "abcd"
FRAMES = 4     # per code and family
MAX_ITER = 3   # the truth of a case holds 1, 2 and 3 iterations (history)
_codes, _truth = {}, {}


def get_code(F, name):
    """(Code, Graph, the form's prefix) of a named code."""
    if name not in _codes:
        code = CODES[name][0](F)
        _codes[name] = (code, Graph(code.lists()), CODES[name][1])
    return _codes[name]


def _signs(rng, shape):
    return np.where(rng.integers(0, 2, shape) == 1, 1.0, -1.0)


def _log_uniform(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), shape))


def family_frame(rng, name, family, graph, f):
    """Frame f of FRAMES of one input family (N(mean, variance), every sign random):
      a  N(0, 4);
      b  magnitudes log-uniform in [1e-12, 600];
      c  N(0, 4) with about 1/60 of the entries -- 1/8 on the stars of small degrees, at least one a frame --
         replaced by magnitudes log-uniform in [690, 1e30].  (The two degree-47 stars keep 1/60: at 1/8
         only 0.2 % of their checks would hold no large input, and the case is to run both folds.);
      d  N(0, 20) with planted 0.0, -0.0 (at most 0.5 % of the case's variables), 5e-324, 1e-300, and
         pairs in the first two slots of a check -- where the reference's chain adds and subtracts their
         magnitudes -- that sum to, or differ by, 36.75 and its two neighbours, or are both 690 or one of
         its two neighbours; in every second frame a check with such a sum or difference also holds an 800,
         which sends the register kernels' check to the log-domain fold that has the 36.75 cut."""
    n = graph.n
    if family == "a":
        return rng.normal(0, 2, n)
    if family == "b":
        return _signs(rng, n) * _log_uniform(rng, 1e-12, 600, n)
    if family == "c":
        x = rng.normal(0, 2, n)
        frac = 1 / 8 if CODES[name][2] and min(graph.cdeg) != 47 else 1 / 60
        idx = rng.choice(n, max(1, round(n * frac)), replace=False)
        x[idx] = _signs(rng, len(idx)) * _log_uniform(rng, 690, 1e30, len(idx))
        return x
    x = rng.normal(0, np.sqrt(20), n)
    lo36, hi36 = np.nextafter(36.75, -np.inf), np.nextafter(36.75, np.inf)
    lo690, hi690 = np.nextafter(690.0, -np.inf), np.nextafter(690.0, np.inf)
    kinds = [("sum", t) for t in (lo36, 36.75, hi36)] + [("diff", t) for t in (lo36, 36.75, hi36)] + \
            [("both", t) for t in (lo690, 690.0, hi690)]
    zeros = min(int(0.005 * FRAMES * n), 8)
    used = set()

    def plant(v, val):
        x[v] = val * (1.0 if rng.integers(0, 2) else -1.0) if val != 0 else val
        used.add(v)
    # every kind in every frame where the code has the checks for it, else dealt over the frames
    mine = kinds if graph.m >= 40 else [k for i, k in enumerate(kinds) if i % FRAMES == f] + \
        [k for i, k in enumerate(kinds) if (i + 2) % FRAMES == f and i >= 6]
    checks = iter(rng.permutation(graph.m))
    for kind, t in mine:
        vs = next(graph.cvars[c] for c in checks if not used & set(graph.cvars[c][:2]))
        a = float(rng.integers(2**20, 2**24)) * 2.0**-20  # in [1, 16), a multiple of 2^-20: a + t, t - a exact
        b = {"sum": t - a, "diff": a + t, "both": t}[kind]
        a = t if kind == "both" else a
        assert {"sum": a + b, "diff": b - a, "both": b}[kind] == t
        plant(vs[0], a)
        plant(vs[1], b)
        if kind != "both" and f % 2 == 1 and len(vs) >= 3 and vs[2] not in used:
            plant(vs[2], 800.0)
    singles = [5e-324, 1e-300] if n >= 100 or f == 0 else []
    singles += [(0.0, -0.0)[(f + i) % 2] for i in range(zeros // FRAMES + (1 if f < zeros % FRAMES else 0))]
    # each in a variable that some check reads, no two in one check (each would make the other's posterior ~0)
    taken = set()
    for v in rng.permutation(n):
        if not singles:
            break
        checks = {c for c in range(graph.m) if v in graph.cvars[c]}
        if v not in used and checks and not checks & taken:
            plant(v, singles.pop())
            taken |= checks
    assert not singles
    return x


def truth_case(F, name, family):
    """(frames [FRAMES][n], [decode(...) per frame at MAX_ITER]) of a code and family, computed once.
    Every frame runs MAX_ITER iterations in the truth: random signs leave the large codes no chance of a
    passing syndrome, but belief propagation satisfies a lone check of small degree in one iteration more
    often than not (it flips the least reliable bit), so a draw whose truth passes a syndrome is drawn again."""
    import zlib
    key = (name, family)
    if key not in _truth:
        _, graph, _ = get_code(F, name)
        rng = np.random.default_rng([FAMILIES.index(family), zlib.crc32(name.encode())])
        xs, ts = [], []
        for f in range(FRAMES):
            for _ in range(200):
                x = family_frame(rng, name, family, graph, f)
                t = decode(graph, x, MAX_ITER)
                if t["iters"] == MAX_ITER and not t["syndrome_ok"]:
                    break
            else:
                raise AssertionError(f"{name} ({family}): no frame that runs {MAX_ITER} iterations in 200 draws")
            xs.append(x)
            ts.append(t)
        _truth[key] = (np.array(xs), ts)
    return _truth[key]


def oracle_code(O, code):
    return O.OracleCode.from_alist_text(code.write_alist())
