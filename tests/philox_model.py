"""The counter-based noise source (include/fpldpc.h, FPLDPC_NOISE_PHILOX) stated in numpy, vectorised over pairs:
Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85), and for seed S,
frame f and position i
    key = (S & 0xffffffff, S >> 32),  counter = (i >> 1, 0, f & 0xffffffff, f >> 32)
    a = (r0 | r1 << 32) >> 11,  b = (r2 | r3 << 32) >> 11,  u1 = (a + 1) 2^-53,  u2 = b 2^-53
    rad = sqrt(-2 ln u1),  z = rad cos(2 pi u2) at even i,  rad sin(2 pi u2) at odd i
    nrm = 0.0 + sigma z,  LLR = (2 snr) ((1 - 2 c[i]) + nrm),  LLR_fp = (int)(LLR 2^frac_bits)
and, at a biased position i = pos[j], the shifted channel of tests/bias_model.py on the same z.

ln, sin and cos are numpy's here, the C library's in the host twin and the device library's in the kernels: the
transform is defined as the mathematical value, and this file also holds the rule by which any two of the three are
compared (f64_bound, boundary, assert_fixed_equal)."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(ctr, key):
    """Philox4x32-10 of counters [..., 4] under key (k0, k1): uint32 [..., 4]."""
    c = np.asarray(ctr, np.uint64)
    c0, c1, c2, c3 = (c[..., i] & _LO for i in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # < 2^64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words(seed, frame, pairs):
    """The four output words of each pair in `pairs` of frame `frame`: uint32 [len(pairs)][4]."""
    pairs = np.asarray(pairs, np.uint64).reshape(-1)
    ctr = np.zeros((len(pairs), 4), np.uint64)
    ctr[:, 0] = pairs
    ctr[:, 2] = frame & 0xFFFFFFFF
    ctr[:, 3] = frame >> 32
    return philox4x32(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def variates(seed, first_frame, frames, n):
    """z [frames][n]."""
    ppf = (n + 1) // 2
    ctr = np.zeros((frames, ppf, 4), np.uint64)
    ctr[:, :, 0] = np.arange(ppf, dtype=np.uint64)[None, :]
    f = [first_frame + k for k in range(frames)]  # python integers: up to 2^63
    ctr[:, :, 2] = np.array([x & 0xFFFFFFFF for x in f], np.uint64)[:, None]
    ctr[:, :, 3] = np.array([x >> 32 for x in f], np.uint64)[:, None]
    r = philox4x32(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.uint64)
    a = (r[..., 0] | r[..., 1] << _S32) >> np.uint64(11)
    b = (r[..., 2] | r[..., 3] << _S32) >> np.uint64(11)
    u1 = (a + np.uint64(1)).astype(np.float64) * 2.0**-53
    u2 = b.astype(np.float64) * 2.0**-53
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = (2.0 * np.pi) * u2
    z = np.empty((frames, 2 * ppf))
    z[:, 0::2] = rad * np.cos(ang)
    z[:, 1::2] = rad * np.sin(ang)
    return z[:, :n]


def channel(seed, first_frame, frames, n, snr, sigma, frac_bits=4, cw=None, pos=(), shift=()):
    """{llr: float64 [frames][n], x: llr * 2^frac_bits (float64, before truncation), fp: int64 trunc(x), logw:
    float64 [frames], abs_terms: float64 [frames] (sum_j |term_j|)} of the channel, shifted on pos by shift."""
    pos = np.asarray(pos, np.int64).reshape(-1)
    a = np.broadcast_to(np.asarray(shift, np.float64), pos.shape)
    nrm = 0.0 + sigma * variates(seed, first_frame, frames, n)
    c = np.zeros((frames, n), np.int64) if cw is None else np.broadcast_to(np.asarray(cw, np.int64) & 1, (frames, n))
    s = (1 - 2 * c).astype(np.float64)
    mean = s.copy()
    mean[:, pos] = s[:, pos] * (1 - a)
    llr = (2 * snr) * (mean + nrm)
    term = a * (2 * s[:, pos] * nrm[:, pos] - a) / (2 * sigma * sigma)
    logw, abs_terms = np.zeros(frames), np.zeros(frames)
    for j in range(len(pos)):  # ascending j, one addition each
        logw = logw + term[:, j]
        abs_terms = abs_terms + np.abs(term[:, j])
    x = llr * float(1 << frac_bits)
    return {"llr": llr, "x": x, "fp": np.trunc(x).astype(np.int64), "logw": logw, "abs_terms": abs_terms}


# ---- the comparison rule, wherever two implementations meet (model, host twin, device)

def f64_bound(snr, sigma):
    """|x - y| of two F64 outputs: a few ulps of ln / sin / cos on |z| <= 8.6 come to about 1e-15 * 10 in z; a
    hundred times that, scaled as the LLR is."""
    return 1e-12 * 2 * snr * (1 + 9 * sigma)


def boundary(x, snr, sigma, frac_bits):
    """The boundary positions of model values x = LLR * 2^frac_bits: within g of an integer, where truncation may
    fall to either side.  Everywhere else two implementations must store the same integer."""
    g = 1e-10 * 2 * snr * (1 + 9 * sigma) * float(1 << frac_bits)
    return np.abs(x - np.rint(x)) <= g


class Budget:
    """At most `cap` boundary positions over all the values a test module compares (about 1e6: the expected share
    is 2 g, about 1e-8).  Counted on the model alone, before the other side is looked at."""

    def __init__(self, cap=2):
        self.cap, self.seen, self.values = cap, 0, 0

    def take(self, mask):
        self.seen += int(mask.sum())
        self.values += mask.size
        assert self.seen <= self.cap, (self.seen, self.values)


def assert_fixed_equal(budget, model, got, snr, sigma, frac_bits, where=""):
    """A quantised output (I32, or I16 without overflow) against the model's by the rule above."""
    edge = boundary(model["x"], snr, sigma, frac_bits)
    budget.take(edge)
    d = np.asarray(got, np.int64) - model["fp"]
    assert (d[~edge] == 0).all(), (where, np.argwhere((d != 0) & ~edge)[:4])
    assert (np.abs(d[edge]) <= 1).all(), where


def assert_fixed_pair(budget, model, a, b, snr, sigma, frac_bits, where=""):
    """Two quantised outputs of other implementations against each other: equal off the model's boundary
    positions (already counted or not: the caller says which by budget = None), within one on them."""
    edge = boundary(model["x"], snr, sigma, frac_bits)
    if budget is not None:
        budget.take(edge)
    d = np.asarray(a, np.int64) - np.asarray(b, np.int64)
    assert (d[~edge] == 0).all(), (where, np.argwhere((d != 0) & ~edge)[:4])
    assert (np.abs(d[edge]) <= 1).all(), where
