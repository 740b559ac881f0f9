#!/usr/bin/env python3
"""What a harvest costs a BER simulation (ber_sim(harvest=...)): A (p = 47, r = 5) at 4.5 dB with the flooding
sxor decoder -- the fastest decoder, so the worst case for the relative overhead -- device channel, a codeword
per frame.  Interleaved runs of the same simulation with the harvest off, on with max_records = 0 (scan only)
and on with max_records = 4096 (scan, compaction and the record buffer's copy until 4096 records are held), REPEAT
of each; and one chunk's kernels timed with events: source (information bits, encoder, channel), decode, scan
without and with rows, compaction -- and the harvest kernels' share of a chunk of the harvest-off runs.

Prints one JSON line per run and a summary line; --out also writes them to a file (the committed copy is
profiles/harvest/bench_harvest.json).  --modes off runs the harvest-less simulation alone (for a library of
an earlier revision through FPLDPC_LIB_PATH).

usage: tools/bench_harvest.py [--frames N] [--chunk N] [--repeat N] [--modes off,0,4096] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EB, MAX_ITER = 4.5, 30


def timed(torch, fn, reps=20):
    """Median milliseconds of fn() on the current stream, by events, after two warm-up calls."""
    fn()
    fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def chunk_times(F, code, dec, chunk, cap):
    """One chunk's stages on one stream, each timed alone.  The harvest's kernels run on preallocated buffers
    through the pointer entry points, so that an interval holds the launches and nothing else: the scan as a
    chunk without rows runs it (weight and unsat only: max_records = 0, or a harvest that is full), the scan
    with err / syn rows, and the compaction."""
    import torch
    dev = torch.device("cuda:0")
    enc = F.Encoder.from_code(code)
    hv = F.Harvest(code, cap)
    snr, sigma = F.snr_sigma(EB, code.rate)
    stream = torch.cuda.current_stream(dev).cuda_stream
    info = torch.empty((chunk, enc.k), dtype=torch.uint8, device=dev)
    llr = torch.empty((chunk, code.n), dtype=torch.int16, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    state = {}

    def source():
        F.info_bits_ptrs(987654321, 0, chunk, enc.k, info.data_ptr(), stream)
        state["cw"] = enc.encode_torch(info)
        F.channel_llr_ptrs(123456789, 0, chunk, code.n, snr, sigma, 4, state["cw"].data_ptr(), 1, llr.data_ptr(),
                           F.FPLDPC_LLR_I16, ovf.data_ptr(), stream)

    def decode():
        state["out"] = dec.decode_torch(llr)

    out = {"source_ms": timed(torch, source), "decode_ms": timed(torch, decode)}
    hard, cw = state["out"]["hard"], state["cw"]
    weight = torch.empty(chunk, dtype=torch.int32, device=dev)
    unsat = torch.empty(chunk, dtype=torch.int32, device=dev)
    err = torch.empty((chunk, hv.hard_words), dtype=torch.int32, device=dev)
    syn = torch.empty((chunk, hv.syn_words), dtype=torch.int32, device=dev)

    def scan(rows):
        hv.scan_ptrs(hard.data_ptr(), cw.data_ptr(), 1, chunk, weight.data_ptr(), unsat.data_ptr(),
                     err.data_ptr() if rows else 0, syn.data_ptr() if rows else 0, stream)

    out["scan_ms"] = timed(torch, lambda: scan(False))
    out["scan_rows_ms"] = timed(torch, lambda: scan(True))
    rows = torch.cat([err, syn], dim=1).contiguous()
    pos = torch.empty(chunk, dtype=torch.int32, device=dev)
    rec = torch.empty((min(cap, chunk), rows.shape[1]), dtype=torch.int32, device=dev)
    c = ctypes.c_void_p

    def compact():
        F.lib().fpldpc_testing_harvest_compact(c(weight.data_ptr()), c(rows.data_ptr()), rows.shape[1], chunk,
                                               min(cap, chunk), c(pos.data_ptr()), c(rec.data_ptr()), c(stream))

    out["compact_ms"] = timed(torch, compact)
    out["codeword_errors_in_chunk"] = int((weight > 0).sum().cpu())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=0, help="frames per run (0: about 4 s, from a calibration run)")
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--modes", default="off,0,4096")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import fixedpointldpc_amd as F
    code = F.Code.array(47, 5)
    dec = F.Decoder(code, max_iter=MAX_ITER)
    snr, sigma = F.snr_sigma(EB, code.rate)
    kw = dict(max_frame_errors=0, chunk=a.chunk, device_channel=True, random_info=True)
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    frames = a.frames
    if frames <= 0:
        r = dec.ber_sim(snr, sigma, max_frames=16 * a.chunk, **kw)  # also the warm-up
        r = dec.ber_sim(snr, sigma, max_frames=64 * a.chunk, **kw)
        frames = max(64, int(4.0 * r["frames"] / r["seconds"] / a.chunk)) * a.chunk
    modes = a.modes.split(",")
    runs = {m: [] for m in modes}
    for rep in range(a.repeat):
        for m in modes:  # interleaved: drift of the machine falls on every mode alike
            r = dec.ber_sim(snr, sigma, max_frames=frames, **kw, **({} if m == "off" else {"harvest": int(m)}))
            hv = r.pop("harvest", None)
            d = {"mode": m, "rep": rep, "frames": r["frames"], "frame_errors": r["frame_errors"], "bit_errors": r["bit_errors"],
                 "seconds": round(r["seconds"], 4), "frames_per_s": round(r["frames"] / r["seconds"])}
            if hv is not None:
                d["harvest_counts"] = hv.counts
            runs[m].append(d)
            emit(d)
    summary = {"summary": True, "code": "A", "ebn0_db": EB, "decoder": dec.describe(), "frames": frames, "chunk": a.chunk,
               "library": os.environ.get("FPLDPC_LIB_PATH", "in-tree"), "kernel_build_id": F.lib().fpldpc_kernel_build_id().decode()}
    for m, rs in runs.items():
        fps = [d["frames_per_s"] for d in rs]
        summary[f"{m}_frames_per_s"] = {"median": statistics.median(fps), "min": min(fps), "max": max(fps)}
    if "off" in runs:
        off = summary["off_frames_per_s"]
        summary["off_spread"] = round((off["max"] - off["min"]) / off["median"], 4)
        for m in modes:
            if m != "off":
                summary[f"{m}_slowdown"] = round(1 - summary[f"{m}_frames_per_s"]["median"] / off["median"], 4)
        assert all(d["frame_errors"] == runs["off"][0]["frame_errors"] and d["bit_errors"] == runs["off"][0]["bit_errors"]
                   for rs in runs.values() for d in rs), "the counters depend on the harvest"
    if any(m != "off" for m in modes):
        t = chunk_times(F, code, dec, a.chunk, 4096)
        summary["chunk_times"] = {k: round(v, 4) if isinstance(v, float) else v for k, v in t.items()}
        if "off" in runs:  # the kernels' share of what a chunk takes the harvest-less simulation, two chunks in flight
            chunk_ms = 1e3 * a.chunk / summary["off_frames_per_s"]["median"]
            summary["off_chunk_ms"] = round(chunk_ms, 4)
            summary["scan_share_of_chunk"] = round(t["scan_ms"] / chunk_ms, 4)
            summary["scan_rows_compact_share_of_chunk"] = round((t["scan_rows_ms"] + t["compact_ms"]) / chunk_ms, 4)
    emit(summary)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(d) for d in lines) + "\n")


if __name__ == "__main__":
    main()
