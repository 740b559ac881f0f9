"""bench.py's roofline bookkeeping (CPU): committed PMC summaries are matched to a run by workload,
kernel build id, frames per launch, Eb/N0 and kernel variant (find_profile), never by key alone;
GPUs are counted from the KFD topology without touching HIP (count_gpus)."""
import importlib.util
import json
import os

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_find_profile_matches_the_exact_workload(tmp_path, monkeypatch):
    b = _bench()
    d = tmp_path / "profiles" / "r9"
    d.mkdir(parents=True)
    base = {"kernel_build_id": "abc", "describe": "flood_array2<P=47,W=3>", "profiled_ebn0_db": 0.0}
    entries = {
        "A": dict(base, workload="A", profiled_frames=4096, sq={"SQ_INSTS_VALU": 1}),
        "A_b8192": dict(base, workload="A", profiled_frames=8192, sq={"SQ_INSTS_VALU": 2}),
        "A_4.5dB": dict(base, workload="A", profiled_frames=4096, profiled_ebn0_db=4.5, sq={"SQ_INSTS_VALU": 3}),
        "A_float": dict(base, workload="A_float", profiled_frames=4096, describe="bp_float", sq={"SQ_INSTS_VALU": 4}),
    }
    (d / "pmc_traffic.json").write_text(json.dumps(entries))
    monkeypatch.setattr(b, "ROOT", str(tmp_path))
    f = lambda *a: (b.find_profile(*a) or {}).get("sq", {}).get("SQ_INSTS_VALU")
    assert f("A", "abc", 4096, 0.0, "flood_array2<P=47,W=3>") == 1
    assert f("A", "abc", 8192, 0.0, "flood_array2<P=47,W=3>") == 2
    assert f("A", "abc", 4096, 4.5, "flood_array2<P=47,W=3>") == 3
    assert f("A_float", "abc", 4096, 0.0, "bp_float") == 4
    assert f("A", "other-build", 4096, 0.0, "flood_array2<P=47,W=3>") is None   # another kernel build
    assert f("A", "abc", 2048, 0.0, "flood_array2<P=47,W=3>") is None           # another batch
    assert f("A", "abc", 4096, 0.0, "flood_array<P=47>") is None                # another variant
    assert b.find_profile("A", "abc", 4096, 0.0, "flood_array2<P=47,W=3>")["file"] == os.path.join("profiles", "r9",
                                                                                              "pmc_traffic.json")


def test_count_gpus_from_kfd_topology(monkeypatch, tmp_path):
    b = _bench()
    nodes = []
    for i, simds in enumerate([0, 1024, 1024, 0]):  # a CPU node, two GPU nodes, another CPU node
        p = tmp_path / f"{i}_properties"
        p.write_text(f"cpu_cores_count 0\nsimd_count {simds}\n")
        nodes.append(str(p))
    monkeypatch.setattr("glob.glob", lambda pattern: nodes)
    for v in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(v, raising=False)
    assert b.count_gpus() == 2
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "1")
    assert b.count_gpus() == 1


def test_committed_profile_is_of_the_shipped_build(F):
    """The newest committed PMC summary was measured on the kernels the in-tree library carries
    (the library's own fpldpc_kernel_build_id, a host function: no GPU needed).  A kernel change
    without a new profiling pass would leave every bench line without its roofline fraction; this
    reports it on the CPU.  A freshness rule for evidence, not a correctness property: a
    kernel edit awaiting its profiling pass, or a hipcc that emits different bytes, skips with the
    ids named instead of failing the suite; one summary must still hold one build's counters."""
    import glob
    import pytest
    import re
    summaries = glob.glob(os.path.join(ROOT, "profiles", "r*", "pmc_traffic.json"))
    newest = max(summaries, key=lambda p: int(re.fullmatch(r"r(\d+)", os.path.basename(os.path.dirname(p))).group(1)))
    ids = {e.get("kernel_build_id") for e in json.load(open(newest)).values()}
    assert len(ids) == 1, (newest, ids)
    built = F.lib().fpldpc_kernel_build_id().decode()
    if ids != {built}:
        pytest.skip(f"{os.path.relpath(newest, ROOT)} profiles kernel build {ids.pop()}, the in-tree library is {built}: "
                    "re-run tools/gpu_round.sh PHASE=prof before quoting a roofline fraction")


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: float32 / float64 .npy files; the hard decisions whole while they fit the
    byte budget, else the frames of a fixed (seeded) sorted sample, the same from run to run."""
    import numpy as np
    b = _bench()
    n, batch = 70, 50
    rs = np.random.default_rng(5)
    words = rs.integers(-2**31, 2**31, (batch, 3), dtype=np.int64).astype(np.int32)
    per = [rs.integers(0, 31, batch).astype(np.int32), rs.integers(0, 2, batch).astype(np.uint8),
           rs.integers(0, n, batch).astype(np.int32)]
    totals = np.array([2**40 + 1, 7, batch, 900], np.int64)
    bits = np.unpackbits(words.view(np.uint8).reshape(batch, -1), axis=1, bitorder="little")[:, :n]

    def unpack(w, nn):
        return np.unpackbits(np.ascontiguousarray(w).view(np.uint8).reshape(len(w), -1), axis=1, bitorder="little")[:, :nn]

    shapes = b.dump_outputs(str(tmp_path / "whole"), n, words, *per, totals, unpack)
    got = {k: np.load(tmp_path / "whole" / f"{k}.npy") for k in shapes}
    assert shapes["hard"] == [batch, n] and (got["hard"] == bits).all() and (got["hard_frames"] == np.arange(batch)).all()
    assert (got["iters"] == per[0]).all() and (got["syndrome_ok"] == per[1]).all() and (got["bit_errors"] == per[2]).all()
    assert got["totals"].dtype == np.float64 and got["totals"].tolist() == totals.tolist()
    assert all(a.dtype == np.float32 for k, a in got.items() if k != "totals")
    monkeypatch.setattr(b, "DUMP_HARD_BYTES", 20 * n * 4 + 8)  # room for 20 frames
    for d in ("s1", "s2"):
        assert b.dump_outputs(str(tmp_path / d), n, words, *per, totals, unpack)["hard"] == [20, n]
    s1, s2 = ({k: np.load(tmp_path / d / f"{k}.npy") for k in shapes} for d in ("s1", "s2"))
    rows = s1["hard_frames"].astype(int)
    assert len(set(rows)) == 20 and (np.diff(rows) > 0).all() and (s1["hard"] == bits[rows]).all()
    assert (s1["iters"] == per[0]).all() and all((s1[k] == s2[k]).all() for k in shapes)
