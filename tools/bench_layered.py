#!/usr/bin/env python3
"""Layered against flooding at equal SNR: one JSON line per (config, Eb/N0, schedule) and one ratio
line per point.  bench.py stays the flagship measurement; this tool answers what the layered
schedule costs and buys on the same frames.

For A (4096 frames) and W (8192 frames), reference-harness frames from seed 123456789, int16 LLRs
resident in HBM: the flooding Decoder and the LayeredDecoder at 0 dB / -2 dB (no frame converges:
all 30 iterations) and at 4.5 dB / 2 dB (the waterfall, early termination).  Timing as bench.py:
device events around each decode call with every output and the totals, after a warm-up; the two
schedules alternate step by step inside one timed window, and the median step is reported.

--post-bits / --msg-bits add a third decoder to the same window: the saturated layered decoder
(fpldpc_layered_create_sat) at those widths.  R (4096 frames, 6.5 dB) is measured on request
(--config R): its unsaturated layered line is only as good as int32 holds at that SNR.
--minsum SCALE16 OFFSET (with the two widths) adds the layered min-sum decoder with compressed check
state (fpldpc_layered_create_minsum) as a further leg; every point then ends with one line that sets its
step time against the saturated sxor decoder's.  --flood-minsum SCALE16 OFFSET (with the two widths) adds the
flooding min-sum decoder (fpldpc_minsum_create) to the same window, on the same frames with the same outputs
and totals, and a line that sets it against layered min-sum when both run.  --flood-sat POST MSG adds the saturated flooding
decoder (fpldpc_flood_create_sat: the flooding Decoder's schedule and check rule at those widths, which are its own:
it needs no --post-bits / --msg-bits) to the same window.  The FPLDPC_LAYERED_* switches apply to the decoders this tool creates, as to any other.

usage: tools/bench_layered.py [--config A W] [--steps 30] [--warmup 5] [--layer-checks 0]
                              [--post-bits 12 --msg-bits 10 [--minsum 12 0] [--flood-minsum 12 0]] [--flood-sat 12 10]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 123456789
CONFIGS = {
    # name: (code, batch, rate of the harness, (Eb/N0 where nothing converges, waterfall Eb/N0))
    "A": (lambda F: F.Code.array(47, 5), 4096, None, (0.0, 4.5)),
    "W": (lambda F: F.Code.wifi_1944_r12(), 8192, 0.5, (-2.0, 2.0)),  # the WiFi harness hard-codes R = 0.5
    "R": (lambda F: F.Code.array(47, 24), 4096, None, (6.5,)),
}


def git_head(arg):
    if arg:
        return arg
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], check=True, capture_output=True,
                              text=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


class Leg:
    """One decoder with its own output buffers and totals."""

    def __init__(self, torch, dec, code, batch, dev):
        k = code.n - code.rank
        dec.set_reference(np.arange(k, dtype=np.int32), np.zeros(k, np.uint8))  # the all-zero codeword
        self.dec, self.k, self.batch = dec, k, batch
        self.hard = torch.empty((batch, dec.hard_words), dtype=torch.int32, device=dev)
        self.iters = torch.empty(batch, dtype=torch.int32, device=dev)
        self.ok = torch.empty(batch, dtype=torch.uint8, device=dev)
        self.bit_err = torch.empty(batch, dtype=torch.int32, device=dev)
        self.totals = torch.zeros(4, dtype=torch.int64, device=dev)
        self.ms = []

    def step(self, llr, F, stream):
        self.dec.decode_ptrs(llr.data_ptr(), F.FPLDPC_LLR_I16, self.batch, self.hard.data_ptr(), self.iters.data_ptr(),
                             self.ok.data_ptr(), 0, self.bit_err.data_ptr(), self.totals.data_ptr(), stream.cuda_stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["A", "W"], choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--min-warmup-s", type=float, default=0.5)
    ap.add_argument("--layer-checks", type=int, default=0)
    ap.add_argument("--post-bits", type=int, default=0, help="with --msg-bits: also time the saturated layered decoder")
    ap.add_argument("--msg-bits", type=int, default=0)
    ap.add_argument("--minsum", type=int, nargs=2, metavar=("SCALE16", "OFFSET"),
                    help="with --post-bits / --msg-bits: also time the layered min-sum decoder")
    ap.add_argument("--flood-minsum", type=int, nargs=2, metavar=("SCALE16", "OFFSET"),
                    help="with --post-bits / --msg-bits: also time the flooding min-sum decoder")
    ap.add_argument("--flood-sat", type=int, nargs=2, metavar=("POST", "MSG"),
                    help="also time the saturated flooding decoder at these widths")
    ap.add_argument("--git-head", default=None, help="recorded as git_head where the tree is not a git checkout")
    args = ap.parse_args()
    assert args.steps >= 20, "at least 20 timed steps"
    assert not args.minsum or (args.post_bits and args.msg_bits), "--minsum needs --post-bits and --msg-bits"
    assert not args.flood_minsum or (args.post_bits and args.msg_bits), "--flood-minsum needs --post-bits and --msg-bits"

    import torch

    import fixedpointldpc_amd as F
    if not torch.cuda.is_available():
        sys.exit("bench_layered.py needs the GPU (there is no CPU path)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    common = {"kernel_build_id": F.lib().fpldpc_kernel_build_id().decode(), "git_head": git_head(args.git_head),
              "device": torch.cuda.get_device_name(dev), "steps": args.steps, "timing": "device events, median step"}
    for cfg in args.config:
        mk, batch, rate, points = CONFIGS[cfg]
        code = mk(F)
        for ebn0 in points:
            snr, sigma = F.snr_sigma(ebn0, rate or code.rate)
            llr = torch.from_numpy(F.channel_llr(SEED, 0, batch, code.n, snr, sigma, 4, None, np.int16, nthreads=16)).to(dev)
            legs = {"flooding": Leg(torch, F.Decoder(code, max_iter=30), code, batch, dev),
                    "layered": Leg(torch, F.LayeredDecoder(code, max_iter=30, layer_checks=args.layer_checks), code,
                                   batch, dev)}
            if args.post_bits or args.msg_bits:
                legs["layered_sat"] = Leg(torch, F.LayeredDecoder(code, max_iter=30, layer_checks=args.layer_checks,
                                                                  post_bits=args.post_bits, msg_bits=args.msg_bits),
                                          code, batch, dev)
            if args.minsum:
                legs["layered_minsum"] = Leg(torch, F.LayeredDecoder(code, max_iter=30, layer_checks=args.layer_checks,
                                                                     check="minsum", post_bits=args.post_bits,
                                                                     msg_bits=args.msg_bits, scale_16=args.minsum[0],
                                                                     offset=args.minsum[1]), code, batch, dev)
            if args.flood_minsum:
                legs["flood_minsum"] = Leg(torch, F.MinSumDecoder(code, max_iter=30, post_bits=args.post_bits,
                                                                  msg_bits=args.msg_bits, scale_16=args.flood_minsum[0],
                                                                  offset=args.flood_minsum[1]), code, batch, dev)
            if args.flood_sat:
                legs["flood_sat"] = Leg(torch, F.FloodSatDecoder(code, max_iter=30, post_bits=args.flood_sat[0],
                                                                 msg_bits=args.flood_sat[1]), code, batch, dev)
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
            for _ in range(args.steps):  # the decoders alternate inside one window
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
                med = float(np.median(leg.ms))
                decoded = int(leg.ok.sum().item())  # frames whose output satisfies H
                rows[name] = {
                    "config": cfg, "ebn0_db": ebn0, "schedule": name, "frames": batch, "max_iter": 30, "early_term": 1,
                    "describe": leg.dec.describe(), "median_ms": round(med, 4), "min_ms": round(float(np.min(leg.ms)), 4),
                    "max_ms": round(float(np.max(leg.ms)), 4), "info_mbps": round(leg.k * batch / med / 1e3, 1),
                    "frames_per_s": round(batch / med * 1e3, 1), "decoded_frames": decoded,
                    "decoded_frames_per_s": round(decoded / med * 1e3, 1), "mean_iters": round(float(tot[3]) / float(tot[2]), 3),
                    "frame_errors": int(tot[1]) // args.steps, "bit_errors": int(tot[0]) // args.steps, **common}
                assert int(tot[2]) == batch * args.steps
            f = rows["flooding"]
            for name, row in rows.items():  # every layered line carries its ratio to flooding (None: flooding decodes no frame)
                if name != "flooding":
                    row["decoded_frames_per_s_vs_flooding"] = (round(row["decoded_frames_per_s"] / f["decoded_frames_per_s"], 4)
                                                               if f["decoded_frames"] else None)
                print(json.dumps(row), flush=True)
            for name in list(legs)[1:]:
                l = rows[name]
                print(json.dumps({
                    "config": cfg, "ebn0_db": ebn0, "ratio": f"{name} / flooding", "describe": l["describe"],
                    "frames_per_s": round(l["frames_per_s"] / f["frames_per_s"], 4),
                    "decoded_frames_per_s": (round(l["decoded_frames_per_s"] / f["decoded_frames_per_s"], 4)
                                             if f["decoded_frames"] else None),
                    "mean_iters": round(l["mean_iters"] / f["mean_iters"], 4),
                    "frame_errors": [l["frame_errors"], f["frame_errors"]], **common}), flush=True)
            if args.minsum:  # the yardstick of the min-sum kernel: the saturated sxor decoder at the same widths
                ms, sx = rows["layered_minsum"], rows["layered_sat"]
                print(json.dumps({
                    "config": cfg, "ebn0_db": ebn0, "ratio": "layered_minsum / layered_sat", "describe": ms["describe"],
                    "median_ms": [ms["median_ms"], sx["median_ms"]], "step_time": round(ms["median_ms"] / sx["median_ms"], 4),
                    "mean_iters": [ms["mean_iters"], sx["mean_iters"]],
                    "ms_per_iteration": [round(ms["median_ms"] / ms["mean_iters"], 4), round(sx["median_ms"] / sx["mean_iters"], 4)],
                    "decoded_frames_per_s_vs_flooding": [ms["decoded_frames_per_s_vs_flooding"],
                                                         sx["decoded_frames_per_s_vs_flooding"]], **common}), flush=True)
            if args.flood_minsum and args.minsum:  # the same check rule on the two schedules
                fm, lm = rows["flood_minsum"], rows["layered_minsum"]
                print(json.dumps({
                    "config": cfg, "ebn0_db": ebn0, "ratio": "flood_minsum / layered_minsum", "describe": fm["describe"],
                    "median_ms": [fm["median_ms"], lm["median_ms"]], "step_time": round(fm["median_ms"] / lm["median_ms"], 4),
                    "mean_iters": [fm["mean_iters"], lm["mean_iters"]],
                    "ms_per_iteration": [round(fm["median_ms"] / fm["mean_iters"], 4), round(lm["median_ms"] / lm["mean_iters"], 4)],
                    "frame_errors": [fm["frame_errors"], lm["frame_errors"]],
                    "decoded_frames_per_s_vs_flooding": [fm["decoded_frames_per_s_vs_flooding"],
                                                         lm["decoded_frames_per_s_vs_flooding"]], **common}), flush=True)


if __name__ == "__main__":
    main()
