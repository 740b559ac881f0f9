#!/usr/bin/env python3
"""What the run-time slot loop of the wide min-sum form costs, and what the two min-sum decoders do on array
codes with p > 64, which only the wide form decodes: one JSON line per (code, point, decoder) and one ratio
line per pair.  A record, not a gate; bench.py stays the flagship measurement.

Part 1, --config A W: the flooding and the layered min-sum decoder (widths 12/10, scale 12/16, max_iter 30) in
their bucket form and forced into the wide form (FPLDPC_MINSUM_FORM=wide, set around creation only), the four
alternating step by step inside one timed window on the frames of tools/bench_layered.py (A: 4096 frames at 0
and 4.5 dB; W: 8192 frames at -2 and 2 dB).  Decoded frames and iteration sums must be equal; the ratio lines
give wide / bucket of the same decoder.

Part 2, --array P,R,EBN0 ...: Code.array(P, R) at one Eb/N0 each with early termination, both decoders as the
placement rule chooses them, with grid, LDS and scratch in `describe`.

Timing as tools/bench_minsum_long.py: device events around each decode call with every output and the totals,
after a warm-up; the median step is reported.

usage: tools/bench_minsum_wide.py [--config A W] [--array 67,5,4.6 97,5,5.0 127,3,5.8] [--array-frames 2048]
                                  [--steps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_layered import CONFIGS, SEED, Leg, git_head  # noqa: E402
from bench_minsum_long import WIDTHS, measure  # noqa: E402

DECODERS = ("flood_minsum", "layered_minsum")
FORM = "FPLDPC_MINSUM_FORM"


def create(F, which, code, wide):
    if wide:
        os.environ[FORM] = "wide"
    try:
        if which == "flood_minsum":
            return F.MinSumDecoder(code, max_iter=30, **WIDTHS)
        return F.LayeredDecoder(code, max_iter=30, check="minsum", **WIDTHS)
    finally:
        os.environ.pop(FORM, None)


def array_point(text):
    p, r, eb = text.split(",")
    return int(p), int(r), float(eb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="*", default=["A", "W"], choices=["A", "W"])
    ap.add_argument("--array", type=array_point, nargs="*", metavar="P,R,EBN0",
                    default=[(67, 5, 4.6), (97, 5, 5.0), (127, 3, 5.8)])
    ap.add_argument("--array-frames", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--min-warmup-s", type=float, default=0.5)
    ap.add_argument("--git-head", default=None, help="recorded as git_head where the tree is not a git checkout")
    args = ap.parse_args()
    assert args.steps >= 20, "at least 20 timed steps"

    import torch

    import fixedpointldpc_amd as F
    if not torch.cuda.is_available():
        sys.exit("bench_minsum_wide.py needs the GPU (there is no CPU path)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    common = {"git_head": git_head(args.git_head), "device": torch.cuda.get_device_name(dev), "steps": args.steps,
              "widths": "12/10", "ms": "12/16-0", "timing": "device events, median step"}

    for cfg in args.config:
        mk, batch, rate, points = CONFIGS[cfg]
        code = mk(F)
        for ebn0 in points:
            snr, sigma = F.snr_sigma(ebn0, rate or code.rate)
            llr = torch.from_numpy(F.channel_llr(SEED, 0, batch, code.n, snr, sigma, 4, None, np.int16, nthreads=16)).to(dev)
            legs = {f"{which}{'_wide' if wide else ''}": Leg(torch, create(F, which, code, wide), code, batch, dev)
                    for which in DECODERS for wide in (False, True)}
            rows = measure(torch, F, legs, llr, stream, dev, args)
            for row in rows.values():
                print(json.dumps({"config": cfg, "ebn0_db": ebn0, **row, **common}), flush=True)
            for which in DECODERS:
                w, b = rows[which + "_wide"], rows[which]
                assert "_wide<" in w["describe"] and "_wide<" not in b["describe"]
                assert (w["decoded_frames"], w["mean_iters"]) == (b["decoded_frames"], b["mean_iters"])
                print(json.dumps({"config": cfg, "ebn0_db": ebn0, "ratio": f"{which}_wide / {which}",
                                  "median_ms": [w["median_ms"], b["median_ms"]],
                                  "step_time": round(w["median_ms"] / b["median_ms"], 4), "mean_iters": w["mean_iters"],
                                  "describe": w["describe"], **common}), flush=True)

    for p, r, ebn0 in args.array:
        code = F.Code.array(p, r)
        batch = args.array_frames
        snr, sigma = F.snr_sigma(ebn0, code.rate)
        llr = torch.from_numpy(F.channel_llr(SEED, 0, batch, code.n, snr, sigma, 4, None, np.int16, nthreads=16)).to(dev)
        legs = {which: Leg(torch, create(F, which, code, False), code, batch, dev) for which in DECODERS}
        rows = measure(torch, F, legs, llr, stream, dev, args)
        for row in rows.values():
            assert "_wide<" in row["describe"]
            print(json.dumps({"config": f"array_p{p}_r{r}", "n": code.n, "m": code.m, "ebn0_db": ebn0, **row, **common}),
                  flush=True)


if __name__ == "__main__":
    main()
