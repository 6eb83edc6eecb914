"""CPU check of the register windows of the generated Philox asm.

tools/gen_philox_asm.py emits every group size G = 2..5 of philox_r29_asm_vkm
in window 0 (fixed pairs v[0, 6G)) and, as philox_r29_asm_vkm_w1 / _w2 / _w3, in
windows 1..3 (v[6G w, 6G (w + 1))), which the depth-3 WAVE rounds rotate through
so that a group's y, w outputs are not overwritten by the next groups.  Every
specialisation is interpreted against a plain Philox4x32-10 with the helpers of
test_philox_asm.py, its fixed registers must lie inside its window, and the
committed header must be what the generator prints now.
"""
import random
import re
import subprocess
import sys

import pytest

from test_philox_asm import GEN, HDR, M0, M1, MASK, W0, W1, parse, philox_rounds, run_asm

GS = (2, 3, 4, 5)
WINDOWS = (0, 1, 2, 3)


def fname(win):
    return "philox_r29_asm_vkm" + (f"_w{win}" if win else "")


def test_header_holds_exactly_these_specialisations():
    src = open(HDR).read()
    found = sorted(re.findall(r"^__device__ __forceinline__ void (philox_r29_asm_vkm\w*)<(\d)>\(",
                              src, re.M))
    assert found == sorted((fname(w), str(g)) for w in WINDOWS for g in GS)
    out = subprocess.run([sys.executable, GEN], capture_output=True, text=True, check=True).stdout
    assert out == src, "ba_philox_asm.hpp is stale: rerun tools/gen_philox_asm.py"


@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("G", GS)
def test_window_rounds_match_philox(G, win):
    lines, outs, ins = parse(G, fname(win))
    # every fixed register (asm text, pinned outputs, clobbers) lies in the window
    src = open(HDR).read()
    body = re.search(r"%s<%d>\(.*?asm volatile\((.*?)\);\n}" % (fname(win), G), src, re.S).group(1)
    regs = {int(r) for r in re.findall(r"\bv(\d+)\b", body)}
    for lo, hi in re.findall(r"v\[(\d+):(\d+)\]", body):
        regs |= {int(lo), int(hi)}
    assert regs and min(regs) >= 6 * G * win and max(regs) < 6 * G * (win + 1), (min(regs), max(regs))
    rng = random.Random(99 + 10 * win + G)
    for _ in range(25):
        k0, k1 = rng.getrandbits(32), rng.getrandbits(32)
        ctrs = [[rng.getrandbits(32) for _ in range(4)] for _ in range(G)]
        r2 = [philox_rounds(c, k0, k1, 0, 2) for c in ctrs]
        want = [philox_rounds(c, k0, k1, 0, 10) for c in ctrs]
        env = {"m0": M0, "m1": M1}
        for g in range(G):
            env[f"x[{g}]"], env[f"yi[{g}]"], env[f"z[{g}]"], env[f"wi[{g}]"] = r2[g]
        for i in range(8):
            env[f"k0[{i}]"] = (k0 + (2 + i) * W0) & MASK
            env[f"k1[{i}]"] = (k1 + (2 + i) * W1) & MASK
        got = run_asm(lines, outs, ins, env)
        for g in range(G):
            assert [got[f"x[{g}]"], got[f"y[{g}]"], got[f"z[{g}]"], got[f"w[{g}]"]] == want[g]
