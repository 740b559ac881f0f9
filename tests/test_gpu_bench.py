"""bench.py's own N-rank launch on the GPU box: `bench.py --gpus 2 --backend gloo` with no outer
torchrun starts two ranks (sharing the box's one GPU), each decoding its own frame range of the
reference channel stream; rank 0 prints one line for the whole job."""
import json
import os
import subprocess
import sys

import pytest

from conftest import stale_profile_ok, ROOT

pytestmark = pytest.mark.gpu


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=240, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_self_launches_two_ranks():
    """The N > 1 line: parity on rank 0's sample (checked after the timed region while rank 1
    waits), no CPU baseline (timed at N = 1 only, the bench contract's rule), and the VALU-issue
    roofline (the committed counters of the per-GPU workload, configs[1]'s 4096 frames, apply to
    every rank's launch)."""
    r = _bench("--full", "--gpus", "2", "--backend", "gloo", "--steps", "2", "--warmup", "1", "--min-warmup-s", "0",
               "--cpu-frames", "256")
    assert r["n_gpus"] == 2 and r["config"]["global_batch"] == 8192 and r["config"]["parallelism"] == "dp2"
    assert r["parity_vs_cpu_oracle"] is True and r["parity_sample"]["last"] == 4095
    assert r["ber"]["frames"] == 2 * 4096 * 2 and r["ber"]["avg_iters"] == 30.0
    assert r["value"] > 0 and r["collective"]["backend"] == "gloo" and r["collective"]["world"] == 2
    assert r["cpu_baseline"] is None and r["cpu_baseline_all_cores"] is None
    assert (r["roofline"]["frac"] is not None and 0 < r["roofline"]["frac"] < 1) or stale_profile_ok(r), r["roofline"]


def test_bench_one_rank_rccl():
    """bench.py under torchrun at one rank: the process group is RCCL (`nccl`) and the counter
    all-reduce runs through it (a 1-rank communicator), as every rank of an 8-GPU run does."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
                        "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(ROOT, "bench.py"),
                        "--full", "--batch", "1024", "--steps", "2", "--warmup", "1", "--no-cpu"],
                       capture_output=True, text=True, timeout=240, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["collective"] == {"backend": "nccl", "world": 1, "ops": r["collective"]["ops"]}
    assert r["n_gpus"] == 1 and r["parity_vs_cpu_oracle"] is True
    assert r["ber"]["frames"] == 1024 * 2 and r["ber"]["avg_iters"] == 30.0


def test_bench_single_gpu_line():
    r = _bench("--full", "--batch", "1024", "--steps", "2", "--warmup", "1", "--cpu-frames", "256", "--inflight-steps",
               "2")
    assert r["n_gpus"] == 1 and r["config"]["global_batch"] == 1024 and r["parity_vs_cpu_oracle"] is True
    # the CPU baseline (N = 1): 1 core, the port calibrated against the reference's own decoder
    # (BASELINE.md CPU-baseline plan, tools/cpu_calibrate.py): bit-exact, within +-15 % of its time
    assert r["cpu_baseline"]["value"] > 0 and r["cpu_baseline"]["cores"] == 1
    cal = r["cpu_baseline"]["calibration"]
    assert cal is not None and cal["bit_exact"] is True, r["cpu_baseline"]
    assert 0.85 <= cal["port_over_reference_time"] <= 1.15, cal
    assert r["cpu_baseline_all_cores"]["value"] > 0
    t = r["two_in_flight"]  # the supplementary two-streams measurement: same decodes, same results
    assert t["batches_in_flight"] == 2 and t["steps"] == 2 and t["iters_equal_headline"] is True and t["value"] > 0


def test_bench_two_in_flight_early_termination():
    """At 4.5 dB (frames stop at different iterations) both decoders of the two-streams
    measurement reproduce the headline's per-frame iteration counts."""
    r = _bench("--full", "--ebn0", "4.5", "--steps", "4", "--warmup", "2", "--no-cpu", "--inflight-steps", "4")
    assert r["parity_vs_cpu_oracle"] is True and r["ber"]["avg_iters"] < 10
    assert r["two_in_flight"]["iters_equal_headline"] is True


def test_bench_plain_run_dumps_last_step(F, torch_dev, tmp_path):
    """A plain run (no --full) times its --steps launches and nothing else: the measurements and
    checks of --full are absent from its line.  --dump-outputs writes what the last timed step
    returned, from the fixed channel stream: equal to an in-process decode of the same frames."""
    import math

    import numpy as np
    import torch
    batch, steps = 300, 3
    r = _bench("--batch", str(batch), "--steps", str(steps), "--warmup", "1", "--min-warmup-s", "0", "--ebn0", "4.5",
               "--dump-outputs", str(tmp_path / "out"))
    assert r["full"] is False and r["steps"] == steps and r["warmup_steps_run"] == 1
    assert r["value"] > 0 and r["ms_per_step"] > 0 and r["dtype"] == "int16" and r["unit"] == "Mb/s"
    # value and ms_per_step are one measurement (the line rounds ms_per_step to 1e-4 ms, value to 1e-3)
    assert math.isclose(r["value"], batch * 1978 / (r["ms_per_step"] * 1e-3) / 1e6,
                        rel_tol=5e-5 / r["ms_per_step"] + 1e-6)
    for k in ("parity_vs_cpu_oracle", "parity_sample", "cpu_baseline", "cpu_baseline_all_cores", "h2d", "two_in_flight"):
        assert r[k] is None, k
    assert r["ber"]["frames"] == batch * steps
    out = {k: np.load(tmp_path / "out" / f"{k}.npy") for k in r["outputs_dumped"]}
    assert sorted(out) == ["bit_errors", "hard", "hard_frames", "iters", "syndrome_ok", "totals"]
    assert all(a.dtype == (np.float64 if k == "totals" else np.float32) for k, a in out.items())
    assert sum(a.nbytes for a in out.values()) <= 64e6
    code = F.Code.array(47, 5)
    snr, sigma = F.snr_sigma(4.5, code.rate)
    llr = F.channel_llr(123456789, 0, batch, code.n, snr, sigma, 4, None, np.int16)
    ref = F.Decoder(code, max_iter=30, width_mask=0xFF).decode_torch(torch.from_numpy(llr).to(torch_dev))
    hard = F.unpack_hard(ref["hard"].cpu().numpy(), code.n)
    assert (out["hard_frames"] == np.arange(batch)).all() and (out["hard"] == hard).all()
    assert (out["iters"] == ref["iters"].cpu().numpy()).all() and out["iters"].min() < 30  # early termination seen
    assert (out["syndrome_ok"] == ref["syndrome_ok"].cpu().numpy()).all()
    assert (out["bit_errors"] == hard[:, :1978].sum(axis=1)).all()  # against the all-zero codeword's info bits
    assert out["totals"].tolist() == [steps * out["bit_errors"].sum(), steps * (out["bit_errors"] > 0).sum(),
                                      steps * batch, steps * out["iters"].sum()]
