"""Mean-shift importance sampling (include/fpldpc.h, fpldpc_bias_t) stated in numpy: the draw stream
(s = s * 48271 mod 2^31 - 1, draw D's state is seed * 48271^(D + 1)), the Odeh-Evans variate of a state, and for
frame f, position i, s = 1 - 2 c[i], nrm = 0.0 + sigma * z of draw f * n + i:
    LLR     = (2 snr) (s (1 - a[j]) + nrm)  at i = pos[j],   2 snr (s + nrm)  elsewhere
    LLR_fp  = (int)(LLR * 2^frac_bits)
    term_j  = a[j] (2 s nrm - a[j]) / (2 sigma sigma),   logw[f] = sum_j term_j  in ascending j
Every operation is one IEEE double operation, as in the library's host channel (no contraction); log is
math.log, the C library's, so that the double outputs can be compared exactly."""
import math

import numpy as np

M, A = 2**31 - 1, 48271
_BLOCK = 4096
_TAB = None


def states(seed, first_draw, count):
    """Lehmer states of draws first_draw .. first_draw + count - 1, uint64 [count]."""
    global _TAB
    if _TAB is None:
        _TAB = np.empty(_BLOCK, np.uint64)
        x = 1
        for k in range(_BLOCK):  # s = s * 48271 mod 2^31 - 1
            x = x * A % M
            _TAB[k] = x
    out = np.empty(count, np.uint64)
    s = seed * pow(A, first_draw, M) % M  # the state after first_draw draws
    for o in range(0, count, _BLOCK):
        k = min(_BLOCK, count - o)
        out[o:o + k] = (np.uint64(s) * _TAB[:k]) % np.uint64(M)  # < 2^62
        s = int(out[o + k - 1])
    return out


_log = np.frompyfunc(math.log, 1, 1)


def variates(s):
    """Odeh & Evans: Normal(0, 1) of each Lehmer state."""
    u = s.astype(np.float64) / float(M)
    p0, q0 = 0.322232431088, 0.099348462606
    p1, q1 = 1.0, 0.588581570495
    p2, q2 = 0.342242088547, 0.531103462366
    p3, q3 = 0.204231210245e-1, 0.103537752850
    p4, q4 = 0.453642210148e-4, 0.385607006340e-2
    low = u < 0.5
    t = np.sqrt(-2.0 * _log(np.where(low, u, 1.0 - u)).astype(np.float64))
    p = p0 + t * (p1 + t * (p2 + t * (p3 + t * p4)))
    q = q0 + t * (q1 + t * (q2 + t * (q3 + t * q4)))
    return np.where(low, (p / q) - t, t - (p / q))


def channel(seed, first_frame, frames, n, snr, sigma, frac_bits=4, cw=None, pos=(), shift=()):
    """{llr: float64 [frames][n], fp: int64 [frames][n] (the truncated fixed-point value before any narrowing),
    logw: float64 [frames], abs_terms: float64 [frames] (sum_j |term_j|)} of the shifted channel."""
    pos = np.asarray(pos, np.int64).reshape(-1)
    a = np.broadcast_to(np.asarray(shift, np.float64), pos.shape)
    z = variates(states(seed, first_frame * n, frames * n)).reshape(frames, n)
    nrm = 0.0 + sigma * z
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
    fp = np.trunc(llr * float(1 << frac_bits)).astype(np.int64)
    return {"llr": llr, "fp": fp, "logw": logw, "abs_terms": abs_terms}


def weights(seed, first_frame, frames, n, sigma, cw=None, pos=(), shift=()):
    """(logw [frames], sum_j |term_j| [frames]) alone: channel()'s, with the variates formed on the biased draws only."""
    pos = np.asarray(pos, np.int64).reshape(-1)
    a = np.broadcast_to(np.asarray(shift, np.float64), pos.shape)
    st = states(seed, first_frame * n, frames * n).reshape(frames, n)[:, pos]
    nrm = 0.0 + sigma * variates(st.reshape(-1)).reshape(frames, len(pos))
    c = np.zeros((frames, n), np.int64) if cw is None else np.broadcast_to(np.asarray(cw, np.int64) & 1, (frames, n))
    s = (1 - 2 * c[:, pos]).astype(np.float64)
    term = a * (2 * s * nrm - a) / (2 * sigma * sigma)
    logw, abs_terms = np.zeros(frames), np.zeros(frames)
    for j in range(len(pos)):
        logw = logw + term[:, j]
        abs_terms = abs_terms + np.abs(term[:, j])
    return logw, abs_terms


def logw_bound(abs_terms):
    """|logw - model| <= 1e-12 (sum_j |term_j| + 1): (count - 1) 2^-53 relative summation error at count <= 256
    is below 3e-14, a few ulps in z between the C libraries add the same order; 1e-12 leaves a tenfold margin."""
    return 1e-12 * (abs_terms + 1)
