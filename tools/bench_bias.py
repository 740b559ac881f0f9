#!/usr/bin/env python3
"""What mean-shift importance sampling costs a BER simulation and what it gives (ber_sim(bias=...)).

cost: A (p = 47, r = 5) at 4.5 dB, MinSumDecoder(scale_16=12), device channel, a codeword per frame, chunks of
16,384.  Interleaved runs, each in a process of its own, of: an earlier revision's library (--parent-lib, through
FPLDPC_LIB_PATH; left out and marked "not measured" without one), this build without a bias, and this build with
a bias of shift 0.5 on 8 and on 64 evenly spaced positions.  A shift changes what the decoder is given, so a
fifth mode, 64 positions at shift 0.0, runs the patch kernel on the plain channel's frames: the kernel's cost
alone.  The no-bias range must overlap the parent's.

use: on A at the highest Eb/N0 of --ebn0 where a plain harvest of --frames frames (2^24) still finds codeword
errors, the first record of the most frequent (weight, unsat) class becomes a bias; the biased simulation runs at
shifts 0.25 and 0.5 and its fer, fer_se, ess and error-frame counts stand beside the plain run's.  The same on
p = 13, r = 2 at an Eb/N0 where the plain run resolves the rate, with the z-score between the two estimates.
These numbers are recorded, not asserted.

Prints one JSON line per run and a summary line per part; --out appends them to a file (the committed copy is
profiles/bias/bench.jsonl).

usage: tools/bench_bias.py cost [--parent-lib LIB] [--seconds S] [--repeat N] [--out FILE]
       tools/bench_bias.py use [--frames N] [--ebn0 6.5,6.0,5.5,5.0] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EB, CHUNK = 4.5, 16384
MODES = ("parent", "off", "bias8", "bias64", "zero64")


def decoder(F, code):
    return F.MinSumDecoder(code, scale_16=12)


def one_run(mode, frames):
    """One timed simulation after a warm-up one, in this process; prints its JSON line."""
    import numpy as np

    import fixedpointldpc_amd as F
    code = F.Code.array(47, 5)
    dec = decoder(F, code)
    snr, sigma = F.snr_sigma(EB, code.rate)
    kw = dict(max_frame_errors=0, chunk=CHUNK, device_channel=True, random_info=True)
    if mode.startswith(("bias", "zero")):
        count = int(mode[4:])
        pos = np.unique(np.linspace(0, code.n - 1, count).astype(np.int64))
        kw["bias"] = F.Bias(code.n, pos, 0.5 if mode.startswith("bias") else 0.0)
    dec.ber_sim(snr, sigma, max_frames=16 * CHUNK, **kw)  # warm-up
    r = dec.ber_sim(snr, sigma, max_frames=frames, **kw)
    r.pop("bias", None)
    print(json.dumps({"part": "cost", "mode": mode, "frames": r["frames"], "frame_errors": r["frame_errors"],
                      "bit_errors": r["bit_errors"], "iter_sum": r["iter_sum"], "seconds": round(r["seconds"], 4),
                      "frames_per_s": round(r["frames"] / r["seconds"]),
                      "kernel_build_id": F.lib().fpldpc_kernel_build_id().decode()}), flush=True)


def worker(mode, frames, parent_lib):
    env = dict(os.environ)
    env.pop("FPLDPC_LIB_PATH", None)
    if mode == "parent":
        env["FPLDPC_LIB_PATH"] = parent_lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "one", "--mode", "off" if mode == "parent" else mode,
                        "--frames", str(frames)], env=env, capture_output=True, text=True, timeout=600)
    if p.returncode:
        raise RuntimeError(f"{mode}: exit {p.returncode}\n{p.stderr[-2000:]}")
    d = json.loads(p.stdout.strip().splitlines()[-1])
    d["mode"] = mode
    return d


def cost(a, emit):
    modes = [m for m in MODES if m != "parent" or a.parent_lib]
    cal = worker("off", 64 * CHUNK, "")
    frames = max(64, int(a.seconds * cal["frames_per_s"] / CHUNK)) * CHUNK
    runs = {m: [] for m in modes}
    for rep in range(a.repeat):
        for m in modes:  # interleaved: drift of the machine falls on every mode alike
            d = worker(m, frames, a.parent_lib)
            d["rep"] = rep
            runs[m].append(d)
            emit(d)
    s = {"part": "cost", "summary": True, "code": "A", "ebn0_db": EB, "decoder": "MinSumDecoder(scale_16=12)",
         "frames": frames, "chunk": CHUNK, "repeat": a.repeat}
    for m, rs in runs.items():
        fps = [d["frames_per_s"] for d in rs]
        s[f"{m}_frames_per_s"] = {"median": statistics.median(fps), "min": min(fps), "max": max(fps)}
    off = s["off_frames_per_s"]
    if "parent" in runs:
        par = s["parent_frames_per_s"]
        s["off_overlaps_parent"] = off["min"] <= par["max"] and par["min"] <= off["max"]
        s["off_over_parent_median"] = round(off["median"] / par["median"], 4)
        assert all(d["bit_errors"] == runs["off"][0]["bit_errors"] and d["iter_sum"] == runs["off"][0]["iter_sum"]
                   for m in ("parent", "off", "zero64") for d in runs[m]), "the plain counters moved"
    else:
        s["parent_frames_per_s"] = "not measured"
    for m in modes:
        if m not in ("parent", "off"):
            s[f"{m}_slowdown"] = round(1 - s[f"{m}_frames_per_s"]["median"] / off["median"], 4)
    emit(s)


def harvest_bias_runs(F, name, code, eb, frames, emit):
    """A plain harvest, then the biased simulation at two shifts on its most frequent class's first record."""
    dec = decoder(F, code)
    k = F.Encoder.from_code(code).k
    snr, sigma = F.snr_sigma(eb, code.rate)
    kw = dict(max_frame_errors=0, max_frames=frames, chunk=CHUNK, device_channel=True, random_info=True)
    r = dec.ber_sim(snr, sigma, harvest=4096, **kw)
    hv = r.pop("harvest")
    classes = hv.classes
    plain = {"part": "use", "code": name, "ebn0_db": eb, "mode": "plain", "frames": r["frames"], "frame_errors": r["frame_errors"],
             "bit_errors": r["bit_errors"], "seconds": round(r["seconds"], 3), "harvest_counts": hv.counts,
             "classes": {f"{w},{u}": c for (w, u), c in classes.items()}}
    p = r["frame_errors"] / r["frames"]
    plain["fer"], plain["fer_se"] = p, math.sqrt(p * (1 - p) / r["frames"])
    emit(plain)
    if not classes or hv.counts["recorded"] == 0:
        return plain, []
    (w, u), _ = max(classes.items(), key=lambda kv: kv[1])
    match = [i for i in range(len(hv.frame)) if (hv.weight[i], hv.unsat[i]) == (w, u)]
    if not match:
        return plain, []
    pos = hv.error_positions(match[0])
    out = []
    for shift in (0.25, 0.5):
        b = F.Bias.from_harvest(hv, match[0], shift)
        r = dec.ber_sim(snr, sigma, bias=b, **kw)
        est = b.estimate(k=k)
        d = {"part": "use", "code": name, "ebn0_db": eb, "mode": "biased", "shift": shift, "class": f"{w},{u}",
             "record_frame": int(hv.frame[match[0]]), "positions": [int(x) for x in pos], "frames": r["frames"],
             "frame_errors": r["frame_errors"], "bit_errors": r["bit_errors"], "seconds": round(r["seconds"], 3), **est,
             "sums": b.sums}
        if plain["fer_se"] > 0:
            d["z_against_plain"] = (est["fer"] - plain["fer"]) / math.hypot(est["fer_se"], plain["fer_se"])
        out.append(d)
        emit(d)
    return plain, out


def use(a, emit):
    import fixedpointldpc_amd as F
    A = F.Code.array(47, 5)
    tried = []
    for eb in [float(x) for x in a.ebn0.split(",")]:  # descending: the first with codeword errors is the highest
        dec = decoder(F, A)
        r = dec.ber_sim(*F.snr_sigma(eb, A.rate), harvest=0, max_frame_errors=0, max_frames=a.frames, chunk=CHUNK,
                        device_channel=True, random_info=True)
        n = r["harvest"].counts["codeword_errors"]
        tried.append({"ebn0_db": eb, "codeword_errors": n, "frame_errors": r["frame_errors"]})
        if n > 0:
            harvest_bias_runs(F, "A", A, eb, a.frames, emit)
            break
    emit({"part": "use", "summary": True, "code": "A", "frames": a.frames, "searched": tried})
    harvest_bias_runs(F, "array13x2", F.Code.array(13, 2), a.small_ebn0, a.small_frames, emit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["cost", "use", "one"])
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--seconds", type=float, default=3.0, help="cost: about this long per run")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1 << 24)
    ap.add_argument("--ebn0", default="6.5,6.0,5.5,5.0")
    ap.add_argument("--small-ebn0", type=float, default=5.0)
    ap.add_argument("--small-frames", type=int, default=1 << 22)
    ap.add_argument("--mode", default="off")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.part == "one":
        return one_run(a.mode, a.frames)
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    (cost if a.part == "cost" else use)(a, emit)


if __name__ == "__main__":
    main()
