#!/usr/bin/env python3
"""What leaving the chip costs the two min-sum decoders, and what they do on codes that only fit off chip:
one JSON line per (code, point, decoder) and one ratio line per pair.  A record, not a gate; bench.py stays
the flagship measurement.

Part 1, --config A W: the flooding and the layered min-sum decoder (widths 12/10, scale 12/16, max_iter 30)
in their LDS form and forced into the global form (FPLDPC_MINSUM_STATE / FPLDPC_LAYERED_MINSUM_STATE =
global, set around creation only), the four alternating step by step inside one timed window on the frames
of tools/bench_layered.py (A: 4096 frames at 0 and 4.5 dB; W: 8192 frames at -2 and 2 dB).  The ratio
lines give global / lds of the same decoder.

Part 2, --long Q ...: the array code cut to 8 block columns and 2 block rows that the long-code tests use
(n = 8q, m = 2q, degree 8; layers of q checks), frames of rint(normal(60, 28)) int16 LLRs: both decoders as
the placement rule chooses them (q = 1123: flooding global, layered LDS; q = 8191: both global), with grid,
LDS and scratch in `describe`.

Timing as tools/bench_layered.py: device events around each decode call with every output and the totals,
after a warm-up; the median step is reported.

usage: tools/bench_minsum_long.py [--config A W] [--long 1123 8191] [--long-frames 1024] [--steps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_layered import CONFIGS, SEED, Leg, git_head  # noqa: E402

WIDTHS = {"post_bits": 12, "msg_bits": 10, "scale_16": 12, "offset": 0}
SWITCH = {"flood_minsum": "FPLDPC_MINSUM_STATE", "layered_minsum": "FPLDPC_LAYERED_MINSUM_STATE"}


def long_alist(q, cols=8, rows=2):
    """Slot j of check c of block row i is variable j*q + c*(j+1+i) mod q (q prime)."""
    chk = [[j * q + (c * (j + 1 + i)) % q for j in range(cols)] for i in range(rows) for c in range(q)]
    var = [[] for _ in range(cols * q)]
    for c, r in enumerate(chk):
        for v in r:
            var[v].append(c)
    lines = [f"{cols * q} {rows * q}", f"{rows} {cols}", " ".join([str(rows)] * (cols * q)), " ".join([str(cols)] * (rows * q))]
    lines += [" ".join(map(str, v)) for v in var] + [" ".join(map(str, r)) for r in chk]
    return "\n".join(lines) + "\n"


def create(F, which, code, layer_checks, forced):
    if forced:
        os.environ[SWITCH[which]] = "global"
    try:
        if which == "flood_minsum":
            return F.MinSumDecoder(code, max_iter=30, **WIDTHS)
        return F.LayeredDecoder(code, max_iter=30, layer_checks=layer_checks, check="minsum", **WIDTHS)
    finally:
        os.environ.pop(SWITCH[which], None)


def measure(torch, F, legs, llr, stream, dev, args):
    """The legs alternate inside one window; returns name -> row."""
    t_w, n_w = time.perf_counter(), 0
    while n_w < args.warmup or time.perf_counter() - t_w < args.min_warmup_s:
        for leg in legs.values():
            leg.step(llr, F, stream)
        n_w += 1
        torch.cuda.synchronize(dev)
    for leg in legs.values():
        leg.totals.zero_()
    torch.cuda.synchronize(dev)
    ev = []
    for _ in range(args.steps):
        for name, leg in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            leg.step(llr, F, stream)
            e1.record(stream)
            ev.append((name, e0, e1))
    torch.cuda.synchronize(dev)
    for name, e0, e1 in ev:
        legs[name].ms.append(e0.elapsed_time(e1))
    rows = {}
    for name, leg in legs.items():
        tot = leg.totals.cpu().numpy()
        assert int(tot[2]) == leg.batch * args.steps
        med = float(np.median(leg.ms))
        decoded = int(leg.ok.sum().item())  # frames whose output satisfies H
        rows[name] = {"decoder": name, "frames": leg.batch, "max_iter": 30, "describe": leg.dec.describe(),
                      "median_ms": round(med, 4), "min_ms": round(float(np.min(leg.ms)), 4),
                      "max_ms": round(float(np.max(leg.ms)), 4), "frames_per_s": round(leg.batch / med * 1e3, 1),
                      "decoded_frames": decoded, "decoded_frames_per_s": round(decoded / med * 1e3, 1),
                      "mean_iters": round(float(tot[3]) / float(tot[2]), 3)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="*", default=["A", "W"], choices=["A", "W"])
    ap.add_argument("--long", type=int, nargs="*", default=[1123, 8191], metavar="Q")
    ap.add_argument("--long-frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--min-warmup-s", type=float, default=0.5)
    ap.add_argument("--git-head", default=None, help="recorded as git_head where the tree is not a git checkout")
    args = ap.parse_args()
    assert args.steps >= 20, "at least 20 timed steps"

    import torch

    import fixedpointldpc_amd as F
    if not torch.cuda.is_available():
        sys.exit("bench_minsum_long.py needs the GPU (there is no CPU path)")
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
            legs = {f"{which}{'_global' if forced else ''}": Leg(torch, create(F, which, code, 0, forced), code, batch, dev)
                    for which in SWITCH for forced in (False, True)}
            rows = measure(torch, F, legs, llr, stream, dev, args)
            for row in rows.values():
                print(json.dumps({"config": cfg, "ebn0_db": ebn0, **row, **common}), flush=True)
            for which in SWITCH:
                g, l = rows[which + "_global"], rows[which]
                assert "mem=global" in g["describe"] and "mem=global" not in l["describe"]
                assert (g["decoded_frames"], g["mean_iters"]) == (l["decoded_frames"], l["mean_iters"])
                print(json.dumps({"config": cfg, "ebn0_db": ebn0, "ratio": f"{which}_global / {which}",
                                  "median_ms": [g["median_ms"], l["median_ms"]],
                                  "step_time": round(g["median_ms"] / l["median_ms"], 4), "mean_iters": g["mean_iters"],
                                  "describe": g["describe"], **common}), flush=True)

    for q in args.long:
        code = F.Code.parse(long_alist(q))
        batch = args.long_frames
        llr = np.rint(np.random.default_rng(5).normal(60, 28, (batch, code.n))).astype(np.int16)
        llr = torch.from_numpy(llr).to(dev)
        legs = {which: Leg(torch, create(F, which, code, q, False), code, batch, dev) for which in SWITCH}
        rows = measure(torch, F, legs, llr, stream, dev, args)
        for row in rows.values():
            print(json.dumps({"config": f"long_q{q}", "n": code.n, "m": code.m, "llr": "rint(normal(60, 28)), seed 5",
                              **row, **common}), flush=True)


if __name__ == "__main__":
    main()
