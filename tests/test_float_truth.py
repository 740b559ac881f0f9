"""The high-precision model of the float decoder (tests/float_truth.py) kept honest, on the CPU.

Its closed-form check update equals the reference's box-plus chain evaluated in the same 50-digit
arithmetic, and the oracle (orc_decode_float: the reference's double arithmetic) stays within
E(oracle) <= 8 of it -- E in ulps of the posterior, of 1 below 1 -- on every code and input family that
tests/test_gpu_float_paths.py gives the kernels, over 1 to 3 iterations.  The GPU test's bound is a
multiple of this E(oracle), so a model that drifted from the reference would show here first.
"""
import numpy as np
import pytest
from mpmath import mp, mpf

import float_truth as T

ORACLE_E_MAX = 8


def _checks(rng, deg):
    """Three checks of one degree: ordinary values; magnitudes over the families' whole range with some
    beyond 690; and ordinary values with a zero and a denormal."""
    a = rng.normal(0, 4, deg)
    b = T._signs(rng, deg) * T._log_uniform(rng, 1e-12, 600, deg)
    b[rng.integers(deg)] = rng.choice([-1.0, 1.0]) * T._log_uniform(rng, 690, 1e30, 1)[0]
    c = rng.normal(0, 4, deg)
    c[rng.integers(deg)] = rng.choice([0.0, -0.0, 5e-324, -1e-300])
    return a, b, c


def test_closed_form_equals_box_plus_chain():
    rng = np.random.default_rng(7)
    worst = 0.0
    with mp.workdps(T.DPS):
        for deg in range(2, 65):
            for x in _checks(rng, deg):
                v = [mpf(float(t)) for t in x]
                closed, chain = T.check_update(v), T.check_update_chain(v)
                for k, (p, q) in enumerate(zip(closed, chain)):
                    err = abs(p - q) / max(1, abs(q))
                    worst = max(worst, float(err))
                    assert err <= mpf("1e-40"), (deg, k, x.tolist(), p, q)
                    if abs(q) > mpf("1e-40"):  # above the chain's own rounding (and sgn(0) = -1 only ever multiplies a zero)
                        assert (p > 0) == (q > 0), (deg, k, x.tolist())
    print(f"closed form against box-plus chain, degrees 2..64: worst scaled difference {worst:.3g}")


def test_phi_is_its_own_inverse_in_both_tails():
    with mp.workdps(T.DPS):
        for x in ("5e-324", "1e-300", "1e-12", "0.5", "1", "36.75", "690", "1e30"):
            x = mpf(x)
            assert abs(T.phi(T.phi(x)) - x) <= mpf("1e-45") * x, x
        assert T.phi(mpf(0)) == mp.inf and T.phi(mp.inf) == 0


@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("name", list(T.CODES))
def test_oracle_within_bound_of_truth(F, O, name, family):
    code, graph, _ = T.get_code(F, name)
    x, truth = T.truth_case(F, name, family)
    assert all(t["iters"] == T.MAX_ITER and not t["syndrome_ok"] for t in truth)
    ocode = T.oracle_code(O, code)
    worst = 0.0
    for k in range(1, T.MAX_ITER + 1):
        ref = O.decode_float_batch(ocode, x, max_iter=k)
        assert (ref["iters"] == k).all()
        for f, t in enumerate(truth):
            worst = max(worst, T.E(ref["post"][f], t["history"][k - 1][0]))
    print(f"{name} ({family}): E(oracle) {worst:.2f}")
    assert worst <= ORACLE_E_MAX, f"{name} ({family}): E(oracle) {worst:.2f}"


def test_family_d_plants_what_it_says(F):
    """The edge inputs of family (d) are in the frames, bit for bit."""
    _, graph, _ = T.get_code(F, "array47x2")
    x, _ = T.truth_case(F, "array47x2", "d")
    near36 = {np.nextafter(36.75, -np.inf), 36.75, np.nextafter(36.75, np.inf)}
    near690 = {np.nextafter(690.0, -np.inf), 690.0, np.nextafter(690.0, np.inf)}
    for row in x:
        first2 = np.abs(np.array([[row[vs[0]], row[vs[1]]] for vs in graph.cvars]))
        assert near36 <= set(first2.sum(axis=1)) and near36 <= set(np.abs(first2[:, 1] - first2[:, 0]))
        assert near690 <= {a for a, b in first2 if a == b}
        assert 5e-324 in np.abs(row) and 1e-300 in np.abs(row)
        zeros = row[row == 0]
        assert 0 < len(zeros) <= 0.005 * graph.n
    assert {bool(np.signbit(z)) for row in x for z in row[row == 0]} == {False, True}
