#!/usr/bin/env python3
"""What the simulation around the float decoder (Decoder.ber_sim(float_bp=True), fpldpc_float_ber_sim_source) runs
at, beside two other figures on the same frames:

  float_sim   ber_sim(float_bp=True): device channel, a codeword per frame (random_info), chunks of 16,384;
  fixed_sim   the fixed-point Decoder.ber_sim with the same arguments (frame f receives the same noise);
  bare_float  decode_float_torch alone over pre-generated F64 LLRs of the same frames (fpldpc_info_bits, the device
              encoder and the F64 channel with a codeword per frame), 16,384 frames a call on one decoder and one
              stream.  The LLRs of a few seconds of decoding do not fit the device, so they are made --block chunks
              at a time with the clock stopped; the clock runs from a block's first decode call to the
              synchronisation after its last.

A (p = 47, r = 5) at 4.5 dB and W (802.11n, n = 1944, rate 1/2) at 2 dB, max_iter 30, noise source --source
(default "philox": the runs are longer than the Lehmer stream serves).  The frame count per code is
set from a warm-up call of the float simulation so that one call runs about --seconds (a whole number of blocks).
After the warm-up the three figures are taken in turn, --repeat times (default 3).  The bare loop's iteration sum
and frame errors must equal the float simulation's: the same frames.  Nothing is asserted about speed.

Prints one JSON line per call and a summary line per code; --out appends them to a file (the committed copy is
profiles/float_sim/bench.jsonl).

usage: tools/bench_float_sim.py [--seconds S] [--repeat N] [--block CHUNKS] [--source S] [--codes A,W] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK, SEED, INFO_SEED, FIRST = 16384, 123456789, 987654321, 0
CASES = {"A": (lambda F: F.Code.array(47, 5), 4.5), "W": (lambda F: F.Code.wifi_1944_r12(), 2.0)}


def pregenerate(F, torch, dev, code, enc, snr, sigma, first, frames, source):
    """Per chunk: (F64 LLRs [b][n], information bits [b][k]) of frames first .. first + frames - 1 on the device."""
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = []
    for f0 in range(first, first + frames, CHUNK):
        b = min(CHUNK, first + frames - f0)
        info = torch.empty((b, enc.k), dtype=torch.uint8, device=dev)
        F.info_bits_ptrs(INFO_SEED, f0, b, enc.k, info.data_ptr(), stream)
        cw = enc.encode_torch(info)
        llr, _ = F.channel_llr_torch(SEED, f0, b, code.n, snr, sigma, 4, cw=cw, dtype=torch.float64, device=dev,
                                     source=source)
        out.append((llr, info))
    torch.cuda.synchronize()
    return out


def bare(F, torch, dev, dec, code, enc, snr, sigma, frames, block, source, idx):
    """decode_float_torch over the frames, a block of chunks at a time; the frame errors are counted with the clock
    stopped, from the hard decisions at the encoder's info positions."""
    word, bit = (idx >> 5), (idx & 31).to(torch.int32)
    dt, gen, its, fe = 0.0, 0.0, 0, 0
    for first in range(FIRST, FIRST + frames, block * CHUNK):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chunks = pregenerate(F, torch, dev, code, enc, snr, sigma, first, min(block * CHUNK, FIRST + frames - first), source)
        gen += time.perf_counter() - t0  # what the simulation does per chunk and this loop's clock leaves out
        t0 = time.perf_counter()
        outs = [dec.decode_float_torch(llr) for llr, _ in chunks]
        torch.cuda.synchronize()
        dt += time.perf_counter() - t0
        for o, (_, info) in zip(outs, chunks):
            its += int(o["iters"].sum())
            got = (o["hard"][:, word] >> bit) & 1
            fe += int((got != info).any(dim=1).sum())
        del chunks, outs
    return {"seconds": dt, "iter_sum": its, "frame_errors": fe, "frames": frames, "generate_seconds": gen}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--block", type=int, default=24)
    ap.add_argument("--source", default="philox")
    ap.add_argument("--codes", default="A,W")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    import fixedpointldpc_amd as F
    dev = torch.device("cuda:0")

    def emit(d):
        print(json.dumps(d), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    for name in a.codes.split(","):
        mk, eb = CASES[name]
        code = mk(F)
        enc = F.Encoder.from_code(code)
        snr, sigma = F.snr_sigma(eb, code.rate)
        dec = F.Decoder(code)
        kw = dict(seed=SEED, first_frame=FIRST, max_frame_errors=0, chunk=CHUNK, device_channel=True, random_info=True,
                  info_seed=INFO_SEED, source=a.source)
        # warm-up of both simulations (tables, the twin's first decode) and the frame count from the float one's rate
        dec.ber_sim(snr, sigma, max_frames=2 * CHUNK, **kw)
        dec.ber_sim(snr, sigma, max_frames=2 * CHUNK, float_bp=True, **kw)
        w = dec.ber_sim(snr, sigma, max_frames=4 * CHUNK, float_bp=True, **kw)
        per = a.block * CHUNK
        frames = max(per, int(a.seconds * w["frames"] / w["seconds"]) // per * per)
        idx = torch.from_numpy(enc.info_index).to(dev).long()
        bare_dec = F.Decoder(code)
        bare_args = (F, torch, dev, bare_dec, code, enc, snr, sigma)
        bare(*bare_args, per, a.block, a.source, idx)  # warm-up
        base = {"code": name, "n": code.n, "ebn0_db": eb, "max_iter": 30, "frames": frames, "chunk": CHUNK, "source": a.source,
                "bare_block_chunks": a.block,
                "describe": bare_dec.float_describe(), "kernel_build_id": F.lib().fpldpc_kernel_build_id().decode()}
        runs = {"float_sim": [], "fixed_sim": [], "bare_float": []}
        for rep in range(a.repeat):
            for mode in runs:  # in turn: drift of the machine falls on every figure alike
                if mode == "bare_float":
                    r = bare(*bare_args, frames, a.block, a.source, idx)
                else:
                    r = dec.ber_sim(snr, sigma, max_frames=frames, float_bp=mode == "float_sim", **kw)
                d = dict(base, mode=mode, rep=rep, frame_errors=r["frame_errors"], iter_sum=r["iter_sum"],
                         fer=r["frame_errors"] / frames, seconds=round(r["seconds"], 4),
                         frames_per_s=round(frames / r["seconds"]))
                assert r["frames"] == frames
                if mode == "bare_float":  # generation alone (allocation included), not in `seconds`
                    d["generate_seconds"] = round(r["generate_seconds"], 4)
                runs[mode].append(d)
                emit(d)
        f0 = runs["float_sim"][0]
        assert all(d["iter_sum"] == f0["iter_sum"] and d["frame_errors"] == f0["frame_errors"]
                   for d in runs["float_sim"] + runs["bare_float"]), "the bare loop did not decode the simulation's frames"
        s = dict(base, summary=True, repeat=a.repeat, machines=1)
        for mode, rs in runs.items():
            fps = [d["frames_per_s"] for d in rs]
            s[mode] = {"frames_per_s": {"median": statistics.median(fps), "min": min(fps), "max": max(fps)},
                       "fer": rs[0]["fer"], "frame_errors": rs[0]["frame_errors"]}
        bf, fs = s["bare_float"]["frames_per_s"], s["float_sim"]["frames_per_s"]
        s["float_sim_over_bare_median"] = round(fs["median"] / bf["median"], 4)
        s["bare_spread"] = bf["max"] - bf["min"]
        s["bare_seconds_median"] = statistics.median(d["seconds"] for d in runs["bare_float"])
        s["bare_generate_seconds_median"] = statistics.median(d["generate_seconds"] for d in runs["bare_float"])
        s["float_sim_seconds_median"] = statistics.median(d["seconds"] for d in runs["float_sim"])
        s["float_sim_below_bare_by_more_than_its_spread"] = bf["median"] - fs["median"] > s["bare_spread"]
        s["float_sim_over_fixed_sim_median"] = round(fs["median"] / s["fixed_sim"]["frames_per_s"]["median"], 4)
        emit(s)


if __name__ == "__main__":
    main()
