"""CPU check of the 8x8 bit-matrix helpers behind k_om3wt's byte-sliced staging
and pick-out (csrc/ba_bitslice.hpp).

The kernel runs exactly these helpers.  tests/native/byte_slice_check.cpp runs
them on the host: transpose8x8 against a bit-by-bit transpose (and as its own
inverse), stage_load + stage_pack against the per-trial definition of
stage_slice (all 256 order bytes, mask bits >= N, every valid count 0..8 of a
lane, buffers of exactly `batch` elements at the C ABI's element alignment),
and pick_out against the per-trial bit() of wave_epilogue's phase 2 (L = 9 and
every other L up to 16).  Built with hipcc as host code the way
tests/test_philox_split.py builds its check, plain and with the host address /
undefined-behaviour sanitizers (a stand-alone executable: no device, nothing
loaded into Python).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "byte_slice_check.cpp")
HIPCC = "/opt/rocm/bin/hipcc"
SANITIZE = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
            "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc absent")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1"] + SANITIZE], ids=["plain", "asan_ubsan"])
def test_byte_slice_helpers_match_the_per_trial_definitions(tmp_path, flags):
    exe = tmp_path / "byte_slice_check"
    subprocess.run([HIPCC, *flags, "-std=c++17", "-Wall", "-o", str(exe), SRC], check=True,
                   capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "byte_slice_check ok" in r.stdout, r.stdout + r.stderr
