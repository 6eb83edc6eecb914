"""CPU check of k_om3wt's per-task helpers (csrc/ba_om3_task.hpp).

The kernel runs exactly these helpers.  tests/native/om3_task_check.cpp runs
them on the host: the closed-form lane tables (om3_lane_tables) against the
per-member definitions in Om3LaneOffsets for every la, the root majorities in
32-bit halves (Om3RootHalves) for their unit-to-lane mapping -- every (word,
receiver, half) covered exactly once, nothing outside R1T or the A image --
and against a bit-by-bit majority on random images.  Built with hipcc as host
code the way tests/test_byte_slice.py builds its check, plain and with the
host address / undefined-behaviour sanitizers (a stand-alone executable: no
device, nothing loaded into Python).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "om3_task_check.cpp")
HIPCC = "/opt/rocm/bin/hipcc"
SANITIZE = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
            "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc absent")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1"] + SANITIZE], ids=["plain", "asan_ubsan"])
def test_task_helpers_match_their_definitions(tmp_path, flags):
    exe = tmp_path / "om3_task_check"
    subprocess.run([HIPCC, *flags, "-std=c++17", "-Wall", "-o", str(exe), SRC], check=True,
                   capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "om3_task_check ok" in r.stdout, r.stdout + r.stderr
