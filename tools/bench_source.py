#!/usr/bin/env python3
"""What the counter-based noise source costs and gives (source="philox", include/fpldpc.h FPLDPC_NOISE_PHILOX),
beside the reference's Lehmer stream.

kernel: the Lehmer channel kernel (fpldpc_channel_llr) and the Philox channel kernel (fpldpc_channel_llr_src)
alternating in one process on A (n = 2209) and W (n = 1944) at 16,384 and 65,536 frames, int16 output, a
codeword per frame; device events after a warm-up, five timings each; G LLR / s and written GB / s with the spread.
sim: A (p = 47, r = 5) at 4.5 dB, MinSumDecoder(scale_16=12), device channel, a codeword per frame, chunks of
16,384, 31,539,200 frames (tools/bench_bias.py cost's count).  Interleaved runs, each in a process of its own, of
an earlier revision's library (--parent-lib, through FPLDPC_LIB_PATH; "not measured" without one), this build with
source="lehmer" and this build with source="philox".  The Lehmer range must overlap the parent's.
fer: p = 13, r = 2 at 5 dB, 4,194,304 frames on each source, the same decoder: the two frame error rates and the
z-score of their difference against their binomial errors.  Recorded, not asserted.

Prints one JSON line per run and a summary line per part; --out appends them to a file (the committed copy is
profiles/source/bench.jsonl).

usage: tools/bench_source.py kernel [--out FILE]
       tools/bench_source.py sim [--parent-lib LIB] [--repeat N] [--out FILE]
       tools/bench_source.py fer [--frames N] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EB, CHUNK, SIM_FRAMES = 4.5, 16384, 31539200
MODES = ("parent", "lehmer", "philox")


def decoder(F, code):
    return F.MinSumDecoder(code, scale_16=12)


def kernel(a, emit):
    import torch

    import fixedpointldpc_amd as F
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    for name, code in (("A", F.Code.array(47, 5)), ("W", F.Code.wifi_1944_r12())):
        n = code.n
        snr, sigma = F.snr_sigma(EB, code.rate)
        for frames in (16384, 65536):
            cw = torch.randint(0, 2, (frames, n), dtype=torch.uint8, device=dev)
            out = torch.empty((frames, n), dtype=torch.int16, device=dev)
            ovf = torch.zeros(1, dtype=torch.int32, device=dev)

            def launch(source):
                F.channel_llr_ptrs(123456789, 0, frames, n, snr, sigma, 4, cw.data_ptr(), 1, out.data_ptr(), F.FPLDPC_LLR_I16,
                                   ovf.data_ptr(), stream, source=source)
            ms = {"lehmer": [], "philox": []}
            for rep in range(-2, 5):  # two warm-up rounds, then five timed ones, the sources alternating
                for source in ms:
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    launch(source)
                    t1.record()
                    t1.synchronize()
                    if rep >= 0:
                        ms[source].append(t0.elapsed_time(t1))
            assert int(ovf.cpu()[0]) == 0
            d = {"part": "kernel", "code": name, "n": n, "frames": frames, "out": "int16", "cw": "per frame",
                 "kernel_build_id": F.lib().fpldpc_kernel_build_id().decode()}
            for source, t in ms.items():
                med = statistics.median(t)
                d[source] = {"ms": {"median": round(med, 4), "min": round(min(t), 4), "max": round(max(t), 4)},
                             "gllr_per_s": round(frames * n / med / 1e6, 2), "gb_per_s_written": round(frames * n * 2 / med / 1e6, 1)}
            d["philox_over_lehmer_time"] = round(d["philox"]["ms"]["median"] / d["lehmer"]["ms"]["median"], 4)
            emit(d)


def one_run(mode, frames):
    """One timed simulation after a warm-up one, in this process; prints its JSON line."""
    import fixedpointldpc_amd as F
    code = F.Code.array(47, 5)
    dec = decoder(F, code)
    snr, sigma = F.snr_sigma(EB, code.rate)
    kw = dict(max_frame_errors=0, chunk=CHUNK, device_channel=True, random_info=True)
    if mode != "parent":  # the parent's library has no source argument: its one stream
        kw["source"] = mode
    dec.ber_sim(snr, sigma, max_frames=16 * CHUNK, **kw)  # warm-up
    r = dec.ber_sim(snr, sigma, max_frames=frames, **kw)
    print(json.dumps({"part": "sim", "mode": mode, "frames": r["frames"], "frame_errors": r["frame_errors"],
                      "bit_errors": r["bit_errors"], "iter_sum": r["iter_sum"], "seconds": round(r["seconds"], 4),
                      "frames_per_s": round(r["frames"] / r["seconds"]),
                      "kernel_build_id": F.lib().fpldpc_kernel_build_id().decode()}), flush=True)


def worker(mode, frames, parent_lib):
    env = dict(os.environ)
    env.pop("FPLDPC_LIB_PATH", None)
    if mode == "parent":
        env["FPLDPC_LIB_PATH"] = parent_lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "one", "--mode", mode, "--frames", str(frames)], env=env,
                       capture_output=True, text=True, timeout=600)
    if p.returncode:
        raise RuntimeError(f"{mode}: exit {p.returncode}\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def sim(a, emit):
    modes = [m for m in MODES if m != "parent" or a.parent_lib]
    runs = {m: [] for m in modes}
    for rep in range(a.repeat):
        for m in modes:  # interleaved: drift of the machine falls on every mode alike
            d = worker(m, a.frames, a.parent_lib)
            d["rep"] = rep
            runs[m].append(d)
            emit(d)
    s = {"part": "sim", "summary": True, "code": "A", "ebn0_db": EB, "decoder": "MinSumDecoder(scale_16=12)",
         "frames": a.frames, "chunk": CHUNK, "repeat": a.repeat}
    for m, rs in runs.items():
        fps = [d["frames_per_s"] for d in rs]
        s[f"{m}_frames_per_s"] = {"median": statistics.median(fps), "min": min(fps), "max": max(fps)}
        s[f"{m}_iter_sum"] = rs[0]["iter_sum"]
    leh = s["lehmer_frames_per_s"]
    if "parent" in runs:
        par = s["parent_frames_per_s"]
        s["lehmer_overlaps_parent"] = leh["min"] <= par["max"] and par["min"] <= leh["max"]
        s["lehmer_over_parent_median"] = round(leh["median"] / par["median"], 4)
        assert all(d["bit_errors"] == runs["lehmer"][0]["bit_errors"] and d["iter_sum"] == runs["lehmer"][0]["iter_sum"]
                   for m in ("parent", "lehmer") for d in runs[m]), "the Lehmer counters moved"
    else:
        s["parent_frames_per_s"] = "not measured"
    s["philox_over_lehmer_median"] = round(s["philox_frames_per_s"]["median"] / leh["median"], 4)
    emit(s)


def fer(a, emit):
    import fixedpointldpc_amd as F
    code = F.Code.array(13, 2)
    snr, sigma = F.snr_sigma(5.0, code.rate)
    got = {}
    for source in ("lehmer", "philox"):
        r = decoder(F, code).ber_sim(snr, sigma, max_frame_errors=0, max_frames=a.frames, chunk=CHUNK, device_channel=True,
                                     random_info=True, source=source)
        p = r["frame_errors"] / r["frames"]
        got[source] = (p, math.sqrt(p * (1 - p) / r["frames"]))
        emit({"part": "fer", "code": "array13x2", "ebn0_db": 5.0, "source": source, "frames": r["frames"],
              "frame_errors": r["frame_errors"], "bit_errors": r["bit_errors"], "iter_sum": r["iter_sum"], "fer": p,
              "fer_se": got[source][1], "seconds": round(r["seconds"], 3)})
    (pl, sl), (pp, sp) = got["lehmer"], got["philox"]
    emit({"part": "fer", "summary": True, "lehmer_fer": pl, "philox_fer": pp, "z": (pp - pl) / math.hypot(sl, sp)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernel", "sim", "fer", "one"])
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--mode", default="lehmer")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    a.frames = a.frames or (1 << 22 if a.part == "fer" else SIM_FRAMES)
    if a.part == "one":
        return one_run(a.mode, a.frames)

    def emit(d):
        print(json.dumps(d), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    {"kernel": kernel, "sim": sim, "fer": fer}[a.part](a, emit)


if __name__ == "__main__":
    main()
