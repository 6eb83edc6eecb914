"""CPU check of the Philox rounds 0-1 split behind k_om3wt's pair table.

A lie call's counter is {pair, level, gw_lo, gw_hi}.  ba_device.hpp restates
rounds 0-1 of Philox4x32-10 as a pair-only entry (philox_pair_entry: what the
lanes of a wave share through LDS), per-(word, level) constants
(philox_word_consts) and a two-xor finish (philox_finish01); the kernel runs
exactly these helpers.  tests/native/philox_split_check.cpp compares them with
philox10 on the host over random pairs, words and keys, levels 0-5 and gw_hi in
{0, 1, random}.  It is built here with hipcc as host code, the way
tests/test_lib.py builds csa_check.cpp, plain and with the host address /
undefined-behaviour sanitizers (a stand-alone executable: no device, nothing
loaded into Python).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "philox_split_check.cpp")
HIPCC = "/opt/rocm/bin/hipcc"
SANITIZE = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
            "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc absent")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1"] + SANITIZE], ids=["plain", "asan_ubsan"])
def test_philox_split_matches_philox10(tmp_path, flags):
    exe = tmp_path / "philox_split_check"
    subprocess.run([HIPCC, *flags, "-std=c++17", "-Wall", "-o", str(exe), SRC], check=True,
                   capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "philox_split_check ok" in r.stdout, r.stdout + r.stderr
