"""What a simulation's rank threads share through host memory (fpldpc_sim_exchange.hpp: the barrier that a failed
rank can break, and the all-gather / all-reduce of the ranks' counters on it) and the weighted sums' frame step
(bias_sums_add, fpldpc_bias.hpp), on the CPU: tests/cpp/sim_exchange_test.cpp, a program of its own, built plain,
with the address and undefined-behaviour sanitizers, and with the thread sanitizer."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

BUILDS = {"plain": ["-O2"],
          "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
          "threads": ["-O1", "-g", "-fsanitize=thread"]}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("build", list(BUILDS))
def test_barrier_exchange_and_bias_sums(tmp_path, build):
    exe = str(tmp_path / "sim_exchange_test")
    subprocess.run(["g++", "-std=c++17", *BUILDS[build], "-pthread", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "fixedpointldpc_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "sim_exchange_test.cpp")], check=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert " 0 mismatches" in p.stdout
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
