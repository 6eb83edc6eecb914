"""tests/wave_shape.py mirrors launch_wave (csrc/ba_wave.hpp): the constants it copies
are read back from the sources, and the shapes the GPU tests rely on are pinned."""
import os
import re

import pytest

import wave_shape as WS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "byzantine-agreement_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_are_the_sources():
    wave, eng, api = _src("ba_wave.hpp"), _src("ba_engine.hpp"), _src("ba_api.cpp")
    assert int(re.search(r"constexpr int kWaveThreads = (\d+);", eng).group(1)) == 64 * WS.WAVES_PER_BLOCK
    assert int(re.search(r"#define BA_OM4W_BLOCKS_PER_CU (\d+)", wave).group(1)) == WS.OM4W_BPC
    assert "static constexpr int BPC = BA_OM4W_BLOCKS_PER_CU;" in wave
    assert f"static constexpr int BPC = {WS.OM3W_BPC};" in wave
    assert int(re.search(r"uint32_t cu_count = (\d+);", api).group(1)) == WS.CU_COUNT
    # the launch arithmetic itself
    for line in ("tasks = (words + G::W - 1) / G::W;", "uint64_t blocks = (tasks + wpb - 1) / wpb;",
                 "uint64_t cap = (uint64_t)G::BPC * a.cu_count;", "if (c >= 1 && c < cap) cap = c;",
                 "tasks <= blocks * wpb"):
        assert line in wave, line


@pytest.mark.parametrize("n", range(6, 15))
def test_om4w_shapes_of_the_gpu_tests(n):
    W = WS.om4w_words(n)
    # the batch test_om4_wave_vs_oracle keeps for the default grid: no loop under any cap
    for cap in (None, "1", "2"):
        s = WS.wave_shape(W, 64 * 13 + 37, cap)
        assert s.words == 14 and s.tasks <= 3 and not s.persistent
    # its capped batch, and test_om4w's
    for cap, waves in (("1", 4), ("2", 8)):
        s = WS.wave_shape(W, 64 * W * 11 + 37, cap)
        assert (s.tasks, 4 * s.blocks, s.persistent) == (12, waves, True)
    assert WS.wave_shape(W, 64 * W * 11 + 37).persistent is False
    s = WS.wave_shape(W, 64 * W * 3 + 11)
    assert (s.tasks, 4 * s.blocks, s.persistent) == (4, 4, False)
    s = WS.wave_shape(W, 64 * W * 9 + 11, "1")
    assert (s.tasks, 4 * s.blocks, s.persistent) == (10, 4, True)


def test_cap_rules():
    assert WS.wave_shape(8, 64 * 8 * 5000, None, 256, WS.OM3W_BPC).blocks == 512  # BPC x CUs
    assert WS.wave_shape(8, 64 * 8 * 5000, "0", 256, WS.OM3W_BPC).blocks == 512   # 0: ignored
    assert WS.wave_shape(8, 64 * 8 * 5000, "512", 256, WS.OM3W_BPC).blocks == 512  # not below the cap
    assert WS.wave_shape(8, 64 * 8 * 5000, "0x10", 256, WS.OM3W_BPC).blocks == 16  # strtoull base 0
    assert WS.wave_shape(8, 1).tasks == 1 and WS.wave_shape(8, 0).tasks == 0
