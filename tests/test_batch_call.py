"""The layout builder of the batch calls (vilo::CallLayout, cerberus_amd/csrc/batch_call.hpp) on a CPU.

tests/host_check/batch_call_check.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers, lays out the
blocks of a gradient-like call and of the gyroscope-bias alignment at W = 1 without landmarks, at a small odd shape and at W = 32768 with
6.5 M landmarks (the alignment's record copies alone are past 4 GiB there) and checks: every offset a multiple of 256, the blocks in order
and disjoint, nothing taken for a block that is not wanted or empty, the totals."""
import os
import subprocess

from conftest import ROOT


def test_call_layout(tmp_path):
    exe = str(tmp_path / "batch_call_check")
    src = os.path.join(ROOT, "tests", "host_check", "batch_call_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe],
                   check=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.strip() == "ok", p.stdout
