"""fpldpc_minsum_ber_sim and its harvest / source forms around a saturated flooding decoder in the global form
(FloodSatDecoder(state="global")): the simulation's twin copies the choice and allocates a scratch of its own, so
every entry point of the family must run the global form with nothing else changed.

The case of tests/test_gpu_flood_sat_sim.py -- Code.array(13, 2) at 4.0 dB, frames 37 .. 1036, chunks of 64, stop at
25 frame errors, widths 10/8, max_iter 7 -- run by a global-form decoder and by an LDS-form decoder with the same
arguments: counters and the on_frame sequence must be equal.  The twin decodes the odd rounds, so a twin that lost
the placement (an LDS launch with the global form's LDS bytes) or the scratch shows up in the counters."""
import pytest

import harvest_model as HM
from test_gpu_flood_sat_sim import CHUNK, COUNTERS, INFO_SEED, MAX_ITER, NEED, WIDTHS, sim_args, small  # noqa: F401

pytestmark = pytest.mark.gpu


def make(F, code, state):
    dec = F.FloodSatDecoder(code, max_iter=MAX_ITER, state=state, **WIDTHS)
    d = dec.describe()
    if state == "global":
        assert d.startswith("flood_sat<DC=16,addr=gtable,deg=table,mem=global> ") and " sat=10/8 state=i16 scratch=" in d, d
    else:
        assert d.startswith("flood_sat<DC=16,addr=computed,deg=table> ") and d.endswith(" sat=10/8 state=i16"), d
    return dec


def both(F, small, **kw):  # noqa: F811
    """(result, on_frame sequence) of the same ber_sim call on a global-form and on an LDS-form decoder."""
    snr, sigma, base = sim_args(F, small)
    if kw.get("random_info"):  # the simulation owns the information bits
        base = {k: v for k, v in base.items() if k not in ("info_index", "info_bits")}
    out = []
    for state in ("global", "lds"):
        seen = []
        r = make(F, small[0], state).ber_sim(snr, sigma, chunk=CHUNK, on_frame=lambda *a: seen.append(a), **{**base, **kw})
        out.append((r, seen))
    return out


def assert_equal_runs(g, l, where):
    (rg, sg), (rl, sl) = g, l
    print(where, {k: rg[k] for k in COUNTERS}, "lds", {k: rl[k] for k in COUNTERS})
    assert {k: rg[k] for k in COUNTERS} == {k: rl[k] for k in COUNTERS}, where
    assert sg == sl and len(sg) == rg["frames"], where


@pytest.mark.parametrize("device_channel", [False, True])
def test_plain_run_stops_inside_a_later_chunk(F, small, device_channel):  # noqa: F811
    g, l = both(F, small, max_frame_errors=NEED, device_channel=device_channel)
    assert_equal_runs(g, l, f"global device_channel={device_channel}")
    r = g[0]
    # a fair case: the stop frame lies strictly inside a chunk of round >= 2, so rounds of the twin are counted
    last = r["frames"] - 1
    assert r["frame_errors"] == NEED and last // CHUNK >= 2 and 0 < last % CHUNK < CHUNK - 1, r
    assert 0.05 <= r["frame_errors"] / r["frames"] <= 0.5 and r["iter_sum"] > r["frames"], r


@pytest.mark.parametrize("source,harvest", [("lehmer", 16), ("philox", None)])
def test_harvest_and_philox(F, small, source, harvest):  # noqa: F811
    """random_info on 256 frames (four chunks, the twin on the odd ones) run to completion: with harvest=16 on the
    reference's noise stream, and on the counter-based source."""
    more = {} if harvest is None else dict(harvest=harvest)
    g, l = both(F, small, max_frames=256, max_frame_errors=0, device_channel=True, random_info=True, info_seed=INFO_SEED,
                source=source, **more)
    assert_equal_runs(g, l, f"global source={source} harvest={harvest}")
    assert g[0]["frames"] == 256 and 0 < g[0]["frame_errors"] < 256, g[0]
    if harvest is not None:
        hg, hl = g[0]["harvest"], l[0]["harvest"]
        assert hg.counts["codeword_errors"] > 0 and len(hg.frame) > 0
        HM.assert_equal(hg, {"counts": hl.counts, "classes": hl.classes, "records": {k: getattr(hl, k) for k in HM.FIELDS}},
                        "global against lds")
