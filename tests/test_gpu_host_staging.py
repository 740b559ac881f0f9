"""The host form of every decoder (fpldpc_decode_host, fpldpc_layered_decode_host for the unsaturated and the
min-sum decoder, fpldpc_minsum_decode_host, fpldpc_decode_float_host) with every subset of its six optional
outputs, through the library itself: the Python wrappers always pass hard, iters and syndrome_ok.

Array code p = 13, r = 3 (n = 169: six hard words, no buffer a multiple of 256 bytes; m = 39), 5 iterations (float:
3).  One decoder object per kind decodes batches of 3, 300 and 2 frames in that order, so that its staging block
grows and a larger block is then reused.  Within a batch every output a call asks for equals the same output of
the call that asks for all six on the same LLRs, and the totals add up across the calls from the caller's
starting values.  The fixed-point decoders run with the pre-check and a noiseless first frame, whose seeded
posteriors come back untouched.  Without reference bits a call that asks for bit_errors fails with its own
family's text."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, R, N, HW = 13, 3, 169, 6
BATCHES = (3, 300, 2)
OUTS = ("hard", "iters", "syndrome_ok", "post", "bit_errors", "totals")
TOT0 = np.array([5, 70, 900, 11000], np.int64)

# kind: (decoder, entry point, LLR dtypes, the set_reference its error text names)
KINDS = {
    "flood": (lambda F, c: F.Decoder(c, max_iter=5, precheck=True), "fpldpc_decode_host", (np.int16, np.int32),
              "fpldpc_set_reference"),
    "layered": (lambda F, c: F.LayeredDecoder(c, max_iter=5, precheck=True), "fpldpc_layered_decode_host",
                (np.int16, np.int32), "fpldpc_layered_set_reference"),
    "layered-minsum": (lambda F, c: F.LayeredDecoder(c, max_iter=5, precheck=True, post_bits=12, msg_bits=10, check="minsum"),
                       "fpldpc_layered_decode_host", (np.int16, np.int32), "fpldpc_layered_set_reference"),
    "minsum": (lambda F, c: F.MinSumDecoder(c, max_iter=5, precheck=True), "fpldpc_minsum_decode_host",
               (np.int16, np.int32), "fpldpc_minsum_set_reference"),
    "float": (lambda F, c: F.Decoder(c, max_iter=3), "fpldpc_decode_float_host", (np.float64,), "fpldpc_set_reference"),
}


@pytest.fixture(scope="module")
def setup(F):
    code = F.Code.array(P, R)
    assert (code.n, code.m) == (N, 39)
    snr, sigma = F.snr_sigma(3.0, code.rate)
    llr = F.channel_llr(20261021, 0, max(BATCHES), N, snr, sigma, dtype=np.int16)
    llr[0] = 40  # noiseless all-zero codeword: the pre-check passes
    return code, llr, F.Encoder.from_code(code).info_index


def _llr(llr16, B, dt):
    """The first B frames as int16 / int32 fixed-point LLRs (4 fraction bits) or as float64 LLRs."""
    return np.ascontiguousarray(llr16[:B] / 16.0 if dt == np.float64 else llr16[:B], dt)


def _call(F, dec, entry, llr, bufs):
    ptr = [None if b is None else b.ctypes.data_as(ctypes.c_void_p) for b in bufs]
    args = [dec._h, llr.ctypes.data_as(ctypes.c_void_p)]
    if llr.dtype != np.float64:
        args.append(F.FPLDPC_LLR_I16 if llr.dtype == np.int16 else F.FPLDPC_LLR_I32)
    return getattr(F.lib(), entry)(*args, llr.shape[0], *ptr)


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_output_subset(F, setup, kind):
    code, llr16, info_index = setup
    make, entry, dtypes, ref_name = KINDS[kind]
    dec = make(F, code)
    fixed = kind != "float"
    post_t = np.int32 if fixed else np.float64
    # bit_errors without reference bits: the family's own text, whatever else is asked for
    be = np.zeros(3, np.int32)
    assert _call(F, dec, entry, _llr(llr16, 3, dtypes[0]), [None, None, None, None, be, None]) == -1
    assert F.lib().fpldpc_last_error().decode().endswith("bit_errors requested without " + ref_name)
    dec.set_reference(info_index, np.zeros(len(info_index), np.uint8))
    for dt in dtypes:
        for B in BATCHES:
            llr = _llr(llr16, B, dt)
            seed = (np.arange(B * N).reshape(B, N) % 251 - 125).astype(post_t)
            running, after, got = TOT0.copy(), {}, {}
            for mask in range(64):  # 63, the last, asks for everything
                want = [bool(mask >> i & 1) for i in range(6)]
                bufs = [np.full((B, HW), 0xA5A5A5A5, np.uint32), np.full(B, -7, np.int32), np.full(B, 9, np.uint8), seed.copy(),
                        np.full(B, -3, np.int32), running]
                bufs = [b if w else None for b, w in zip(bufs, want)]
                assert _call(F, dec, entry, llr, bufs) == 0, (mask, F.lib().fpldpc_last_error().decode())
                got[mask] = bufs
                if want[5]:
                    after[mask] = running.copy()
            full = dict(zip(OUTS, got[63]))
            where = f"{kind} {np.dtype(dt).name} batch {B}"
            # the all-outputs call itself: totals are this batch's sums on top of the 31 calls before it
            delta = np.array([full["bit_errors"].sum(), (full["bit_errors"] > 0).sum(), B, full["iters"].sum()], np.int64)
            assert (full["iters"] >= 0).all() and (full["iters"] <= (5 if fixed else 3)).all(), where
            assert set(np.unique(full["syndrome_ok"])) <= {0, 1} and full["syndrome_ok"][0] == 1, where
            assert not (full["hard"][0] != 0).any(), where
            assert (full["post"][1:] != seed[1:]).any(), where
            if fixed:  # frame 0 passes the pre-check: its seeded posteriors stay
                assert (full["post"][0] == seed[0]).all(), where
            calls = 0
            for mask in range(64):
                for name, b in zip(OUTS[:5], got[mask][:5]):
                    if b is not None:
                        assert np.array_equal(b, full[name]), f"{where}: {name} of subset {mask:06b}"
                if mask in after:
                    calls += 1
                    assert np.array_equal(after[mask], TOT0 + calls * delta), f"{where}: totals after subset {mask:06b}"
            assert calls == 32


# (entry point, LLR dtype, frames): the fixed-point and the float host decode of one flooding decoder in turn
SHARED_CALLS = (("fpldpc_decode_host", np.int16, 3), ("fpldpc_decode_float_host", np.float64, 300),
                ("fpldpc_decode_host", np.int32, 300), ("fpldpc_decode_float_host", np.float64, 2),
                ("fpldpc_decode_host", np.int16, 2))


def test_fixed_and_float_share_one_block(F, setup):
    """The two host decodes of one flooding decoder object share its staging block and stream: the block is grown
    by one family and reused by the other, with other element sizes and so other region offsets.  One decoder
    (3 iterations, pre-check on, so the fixed-point calls' seeded posteriors of the noiseless frame must survive
    what the float call left in the block) takes SHARED_CALLS in order, all six outputs each; every call's outputs
    equal those of the same call on a fresh decoder of its own."""
    code, llr16, info_index = setup

    def make():
        dec = F.Decoder(code, max_iter=3, precheck=True)
        dec.set_reference(info_index, np.zeros(len(info_index), np.uint8))
        return dec

    def call(dec, entry, dt, B):
        seed = (np.arange(B * N).reshape(B, N) % 251 - 125).astype(np.float64 if dt == np.float64 else np.int32)
        bufs = [np.full((B, HW), 0xA5A5A5A5, np.uint32), np.full(B, -7, np.int32), np.full(B, 9, np.uint8), seed.copy(),
                np.full(B, -3, np.int32), TOT0.copy()]
        assert _call(F, dec, entry, _llr(llr16, B, dt), bufs) == 0, F.lib().fpldpc_last_error().decode()
        return dict(zip(OUTS, bufs)), seed

    shared = make()
    for i, (entry, dt, B) in enumerate(SHARED_CALLS):
        where = f"call {i + 1}: {entry} {np.dtype(dt).name} batch {B}"
        (got, seed), (want, _) = call(shared, entry, dt, B), call(make(), entry, dt, B)
        # the fresh decoder's call did its work: every output written, its totals this batch's sums
        assert (want["iters"] >= 0).all() and (want["iters"] <= 3).all() and (want["bit_errors"] >= 0).all(), where
        assert want["syndrome_ok"][0] == 1 and (want["post"][1:] != seed[1:]).any(), where
        assert np.array_equal(want["totals"] - TOT0, [want["bit_errors"].sum(), (want["bit_errors"] > 0).sum(), B,
                                                      want["iters"].sum()]), where
        for name in OUTS:
            assert np.array_equal(got[name], want[name]), f"{where}: {name}"
