"""Every kernel form of the float decoder (fpldpc_decode_float), and the log-domain fold inside the
register forms, against the high-precision model tests/float_truth.py.

The forms (Decoder.float_describe() names the one a decoder launches; every test asserts it):
  bp_float_reg<DC=47,regular,array>    star47, array47x2
  bp_float_reg<DC=47,regular,table>    array47x2b, star47t
  bp_float_reg<DC=8,predicated,table>  star_small (degrees 2..8), irregular (2..6)
  bp_float_kernel                      star_generic, array13x2, rand_deg60
and, in the register forms, the log-domain fold of a check that holds a message of magnitude >= 690.

The measure is E(x) = max_v |x_v - truth_v| / (2^-52 max(1, |truth_v|)) and the bound
E(gpu) <= 4 max(E(oracle), 1), the oracle's own E computed on the same frames (it is at most 8:
tests/test_float_truth.py).  Why 4: a float64 emulation of the tanh fold has 0.5 to 2.2 times the
oracle's E on such frames and the device exp, log and division are each within an ulp, so 4 leaves
about a factor 2; a plumbing error (wrong slot, wrong sign, stale c2v, the wrong side of a threshold)
is at least 1e10 in this unit.  Hard decisions must equal the truth's wherever the bound on the
posterior leaves its sign no choice, |truth| > 4 max(E(oracle), 1) 2^-52 max(1, |truth|) -- every
variable with |truth| > 1e-9 and more: family (b) has magnitudes from 1e-12, a fifth of its posteriors
lie below 1e-9, and they are compared too -- and at most 1 % of a case's variables may lie below that.

Measured on an MI355X (-s prints each case): see DESIGN.md, "Float decoder against the high-precision model".
"""
import numpy as np
import pytest

import float_truth as T

pytestmark = pytest.mark.gpu
SEED = 123456789
BOUND = 4
ULP = 2.0 ** -52


def _decode(F, torch_dev, dec, x):
    import torch
    out = dec.decode_float_torch(torch.from_numpy(np.ascontiguousarray(x)).to(torch_dev), post=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(F, out, n):
    return F.unpack_hard(out["hard"], n)


def _oracle_E(O, ocode, x, want, max_iter):
    """E(oracle) over the frames x against want = [(post, hard, ok, iters)], with the oracle run as the GPU is."""
    ref = O.decode_float_batch(ocode, x, max_iter=max_iter)
    return max(T.E(ref["post"][f], w[0]) for f, w in enumerate(want))


def _compare(F, code, out, want, e_oracle, where, frames=None):
    """GPU frames `frames` of out (default: all, in order) against want = [(post, hard, ok, iters)]: E within
    the bound, hard decisions, iteration counts, and the syndrome verdict against the GPU's own bits.
    Returns E(gpu)."""
    frames = range(len(want)) if frames is None else frames
    bound = BOUND * max(e_oracle, 1.0)
    bits = _bits(F, out, code.n)
    e_gpu, left_out = 0.0, 0
    for f, (post, hard, ok, iters) in zip(frames, want):
        e = T.E(out["post"][f], post)
        e_gpu = max(e_gpu, e)
        assert e <= bound, f"{where} frame {f}: E(gpu) {e:.3g} > {BOUND} * max(E(oracle) {e_oracle:.3g}, 1)"
        t = np.abs(np.array([float(p) for p in post]))
        sure = t > bound * ULP * np.maximum(1.0, t)
        left_out += int((~sure).sum())
        bad = np.nonzero(sure & (bits[f] != hard))[0]
        assert bad.size == 0, f"{where} frame {f}: hard decisions differ at {bad[:8]}"
        assert out["iters"][f] == iters, f"{where} frame {f}: {out['iters'][f]} iterations, truth {iters}"
        assert bool(out["syndrome_ok"][f]) == code.syndrome_ok(bits[f]), f"{where} frame {f}: syndrome verdict"
    assert left_out <= 0.01 * len(want) * code.n, f"{where}: {left_out} posteriors too close to zero to decide"
    return e_gpu


def _same(a, b):
    return all((a[k].view(np.uint8) == b[k].view(np.uint8)).all() for k in ("post", "hard", "iters", "syndrome_ok"))


@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("name", list(T.CODES))
def test_every_form_every_family(F, O, torch_dev, name, family):
    """Test 1: 1, 2 and 3 iterations of four frames that no syndrome ends, early termination on and off."""
    code, graph, form = T.get_code(F, name)
    x, truth = T.truth_case(F, name, family)
    assert all(t["iters"] == T.MAX_ITER and not t["syndrome_ok"] for t in truth)
    if family == "c":  # every frame, every iteration: checks for the log-domain fold and checks for the tanh fold
        assert all(0 < len(b) < graph.m for t in truth for b in t["big"]), [[len(b) for b in t["big"]] for t in truth]
    ocode = T.oracle_code(O, code)
    worst_gpu = worst_oracle = 0.0
    for k in range(1, T.MAX_ITER + 1):
        want = [(*t["history"][k - 1], k) for t in truth]
        e_oracle = _oracle_E(O, ocode, x, want, k)
        outs = []
        for early_term in (True, False):
            dec = F.Decoder(code, max_iter=k, early_term=early_term)
            assert dec.float_describe().startswith(form), dec.float_describe()
            outs.append(_decode(F, torch_dev, dec, x))
        assert _same(*outs), f"{name} ({family}) {k} iterations: early termination changes the outputs"
        assert not outs[0]["syndrome_ok"].any()
        e_gpu = _compare(F, code, outs[0], want, e_oracle, f"{name} ({family}) {k} iterations")
        worst_gpu, worst_oracle = max(worst_gpu, e_gpu), max(worst_oracle, e_oracle)
    print(f"{name} ({family}) [{form}]: E(gpu) {worst_gpu:.2f} E(oracle) {worst_oracle:.2f}")


# Eb/N0 at which the truth's iteration counts of 16 all-zero-codeword AWGN frames (rate max(R, 0.3)) spread
# over at least three values below max_iter = 8 and some frames fail: chosen on the CPU, from the truth
CONVERGING = {"array13x2": 3.0, "rand_deg60": 4.0, "irregular": 2.0}


def _awgn(F, O, code, ebn0, frames):
    snr, sigma = F.snr_sigma(ebn0, max(code.rate, 0.3))
    return O.gen_llr_f64(SEED, 0, frames, code.n, snr, sigma)


@pytest.mark.parametrize("name", list(CONVERGING))
def test_converging_frames(F, O, torch_dev, name):
    """Test 2: early termination, frame by frame: iterations, hard decisions and verdicts equal the truth's."""
    code, graph, form = T.get_code(F, name)
    x = _awgn(F, O, code, CONVERGING[name], 16)
    truth = [T.decode(graph, row, 8) for row in x]
    its = [t["iters"] for t in truth]
    assert len({i for i, t in zip(its, truth) if t["syndrome_ok"]}) >= 3 and not all(t["syndrome_ok"] for t in truth), its
    keep = [f for f, t in enumerate(truth) if t["min_abs_post"] >= 1e-9]
    assert len(keep) >= 15
    dec = F.Decoder(code, max_iter=8)
    assert dec.float_describe().startswith(form), dec.float_describe()
    out = _decode(F, torch_dev, dec, x)
    want = [(truth[f]["post"], truth[f]["hard"], truth[f]["syndrome_ok"], truth[f]["iters"]) for f in keep]
    ref = O.decode_float_batch(T.oracle_code(O, code), x, max_iter=8)
    same = [f for f in keep if ref["iters"][f] == truth[f]["iters"]]
    e_oracle = max(T.E(ref["post"][f], truth[f]["post"]) for f in same)
    e_gpu = _compare(F, code, out, want, e_oracle, f"{name} {CONVERGING[name]} dB", frames=keep)
    bits = _bits(F, out, code.n)
    for f in keep:
        assert (bits[f] == truth[f]["hard"]).all() and bool(out["syndrome_ok"][f]) == truth[f]["syndrome_ok"], f
    print(f"{name} {CONVERGING[name]} dB [{form}]: iterations {sorted(its)}, E(gpu) {e_gpu:.2f} E(oracle) {e_oracle:.2f}")


# Eb/N0 at which the first two AWGN frames converge within 3 iterations (the truth asserts it)
BATCH_CODES = {"array47x2": 7.0, "array47x2b": 7.0, "irregular": 6.0, "array13x2": 6.0}


@pytest.mark.parametrize("name", list(BATCH_CODES))
def test_more_frames_than_the_grid(F, O, torch_dev, monkeypatch, name):
    """Test 3: grid + 3 frames on a grid of one workgroup per CU, so workgroups decode a second frame over the
    scratch of their first (never cleared: the `first` flag of the register forms, the edge init of the generic
    kernel), and a frame that converged early is followed by one that does not."""
    monkeypatch.setenv("FPLDPC_FLOAT_WG_PER_CU", "1")
    code, graph, form = T.get_code(F, name)
    dec = F.Decoder(code, max_iter=T.MAX_ITER)
    desc = dec.float_describe()
    assert desc.startswith(form), desc
    grid = int(desc.split("grid=")[1].split()[0])
    assert 0 < grid <= 1024, desc  # one workgroup on each CU
    awgn = _awgn(F, O, code, BATCH_CODES[name], 2)
    t_awgn = [T.decode(graph, row, T.MAX_ITER) for row in awgn]
    assert all(t["syndrome_ok"] for t in t_awgn)
    xs, truth = [awgn], t_awgn
    for family in "acd":
        x, t = T.truth_case(F, name, family)
        xs.append(x[:2])
        truth += t[:2]
    distinct = np.concatenate(xs)  # 2 AWGN, 2 of (a), 2 of (c), 2 of (d)
    order = np.random.default_rng(3).permutation(grid + 3) % 8
    out = _decode(F, torch_dev, dec, distinct[order])
    want8 = [(t["post"], t["hard"], t["syndrome_ok"], t["iters"]) for t in truth]
    e_oracle = _oracle_E(O, T.oracle_code(O, code), distinct, want8, T.MAX_ITER)
    first = [int(np.nonzero(order == i)[0][0]) for i in range(8)]
    e_gpu = _compare(F, code, out, want8, e_oracle, f"{name} batch of {grid + 3}", frames=first)
    for i in range(8):  # every copy bit-identical to the first, which is compared with the truth
        for f in np.nonzero(order == i)[0]:
            assert all(out[k][f].tobytes() == out[k][first[i]].tobytes() for k in ("post", "hard", "iters", "syndrome_ok")), f"{name}: frame {f}, a copy of {first[i]}, differs"
    print(f"{name} [{desc}] batch {grid + 3}: E(gpu) {e_gpu:.2f} E(oracle) {e_oracle:.2f}")


def test_two_calls_on_one_stream(F, O, torch_dev):
    """Test 4: two calls of one decoder back to back on one stream (the second launch's counter reset and
    scratch follow the first's in stream order); both equal the truth."""
    import torch
    code, graph, form = T.get_code(F, "star_generic")
    dec = F.Decoder(code, max_iter=T.MAX_ITER)
    assert dec.float_describe().startswith(form), dec.float_describe()
    cases = [T.truth_case(F, "star_generic", family) for family in "ac"]
    dev_in = [torch.from_numpy(x).to(torch_dev) for x, _ in cases]
    torch.cuda.synchronize()
    outs = [dec.decode_float_torch(x, post=True) for x in dev_in]  # no synchronisation in between
    torch.cuda.synchronize()
    ocode = T.oracle_code(O, code)
    for (x, truth), out, tag in zip(cases, outs, "ac"):
        want = [(t["post"], t["hard"], t["syndrome_ok"], t["iters"]) for t in truth]
        out = {k: v.cpu().numpy() for k, v in out.items()}
        e_oracle = _oracle_E(O, ocode, x, want, T.MAX_ITER)
        e_gpu = _compare(F, code, out, want, e_oracle, f"star_generic ({tag}), call on a shared stream")
        print(f"star_generic ({tag}) two calls: E(gpu) {e_gpu:.2f} E(oracle) {e_oracle:.2f}")


def test_check_degree_above_64_has_no_decoder(F, torch_dev):
    """Why star_generic stops at degree 64: the float kernel takes check degrees up to 255, but a Decoder
    is created with its fixed-point kernel, and there is none above 64."""
    code = F.Code.parse(T.star_alist([2, 3, 129, 255]))
    with pytest.raises(F.FpldpcError) as e:
        F.Decoder(code)
    assert e.value.code == -4
