#!/usr/bin/env python3
"""What leaving the chip costs the saturated flooding decoder, and what it does on codes that only fit off chip:
one JSON line per (code, point, placement) and one ratio line per pair.  A record, not a gate; bench.py stays
the flagship measurement.

Part 1, --config A W: FloodSatDecoder (widths 12/10, max_iter 30) in its LDS form and forced into the global
form (state="global"), the two alternating step by step inside one timed window on the frames of
tools/bench_layered.py (A: 4096 frames at 0 and 4.5 dB; W: 8192 frames at -2 and 2 dB).  Decoded frames and
iteration sums of the two must be equal; the ratio lines give global / lds.

Part 2, --long Q ... and --array P R: the global form alone (state="auto", which must choose it) on the array
code cut to 8 block columns and 2 block rows that the long-code tests use (n = 8q, m = 2q, degree 8; frames of
rint(normal(60, 28)) int16 LLRs) and on Code.array(P, R) (rint(normal(60, 24))), with grid, LDS and scratch in
`describe`.  The LDS form refuses these codes, so there is nothing to compare them with.

Timing as tools/bench_minsum_long.py: device events around each decode call with every output and the totals,
after a warm-up; the median step is reported.  --out appends the lines to a file as well.

usage: tools/bench_flood_sat_long.py [--config A W] [--long 1123 8191] [--array 61 30] [--long-frames 1024]
                                     [--steps 30] [--warmup 5] [--out profiles/flood_sat_long/bench.jsonl]
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
from bench_minsum_long import long_alist, measure  # noqa: E402

WIDTHS = {"post_bits": 12, "msg_bits": 10}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="*", default=["A", "W"], choices=["A", "W"])
    ap.add_argument("--long", type=int, nargs="*", default=[1123, 8191], metavar="Q")
    ap.add_argument("--array", type=int, nargs="*", default=[61, 30], metavar="N", help="P R of a Code.array, or nothing")
    ap.add_argument("--long-frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--min-warmup-s", type=float, default=0.5)
    ap.add_argument("--out", default=None, help="append every line to this file too")
    ap.add_argument("--git-head", default=None, help="recorded as git_head where the tree is not a git checkout")
    args = ap.parse_args()
    assert args.steps >= 20, "at least 20 timed steps"
    assert len(args.array) in (0, 2), "--array takes P R"

    import torch

    import fixedpointldpc_amd as F
    if not torch.cuda.is_available():
        sys.exit("bench_flood_sat_long.py needs the GPU (there is no CPU path)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    common = {"git_head": git_head(args.git_head), "device": torch.cuda.get_device_name(dev), "steps": args.steps,
              "widths": "12/10", "timing": "device events, median step"}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(row):
        line = json.dumps({**row, **common})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for cfg in args.config:
        mk, batch, rate, points = CONFIGS[cfg]
        code = mk(F)
        for ebn0 in points:
            snr, sigma = F.snr_sigma(ebn0, rate or code.rate)
            llr = torch.from_numpy(F.channel_llr(SEED, 0, batch, code.n, snr, sigma, 4, None, np.int16, nthreads=16)).to(dev)
            legs = {f"flood_sat{'_global' if state == 'global' else ''}":
                    Leg(torch, F.FloodSatDecoder(code, max_iter=30, state=state, **WIDTHS), code, batch, dev)
                    for state in ("lds", "global")}
            rows = measure(torch, F, legs, llr, stream, dev, args)
            for row in rows.values():
                emit({"config": cfg, "ebn0_db": ebn0, **row})
            g, l = rows["flood_sat_global"], rows["flood_sat"]
            assert "mem=global" in g["describe"] and "mem=global" not in l["describe"]
            assert (g["decoded_frames"], g["mean_iters"]) == (l["decoded_frames"], l["mean_iters"]), (g, l)
            emit({"config": cfg, "ebn0_db": ebn0, "ratio": "flood_sat_global / flood_sat",
                  "median_ms": [g["median_ms"], l["median_ms"]], "step_time": round(g["median_ms"] / l["median_ms"], 4),
                  "mean_iters": g["mean_iters"], "decoded_frames": g["decoded_frames"], "describe": g["describe"]})

    long_codes = [(f"long_q{q}", lambda q=q: F.Code.parse(long_alist(q)), 28) for q in args.long]
    if args.array:
        p, r = args.array
        long_codes.append((f"array_{p}x{r}", lambda: F.Code.array(p, r), 24))
    for name, mk, sigma in long_codes:
        code = mk()
        batch = args.long_frames
        llr = np.rint(np.random.default_rng(5).normal(60, sigma, (batch, code.n))).astype(np.int16)
        llr = torch.from_numpy(llr).to(dev)
        legs = {"flood_sat_global": Leg(torch, F.FloodSatDecoder(code, max_iter=30, state="auto", **WIDTHS), code, batch, dev)}
        rows = measure(torch, F, legs, llr, stream, dev, args)
        for row in rows.values():
            assert "mem=global" in row["describe"], row["describe"]
            emit({"config": name, "n": code.n, "m": code.m, "dc_max": code.dc_max,
                  "llr": f"rint(normal(60, {sigma})), seed 5", **row})


if __name__ == "__main__":
    main()
