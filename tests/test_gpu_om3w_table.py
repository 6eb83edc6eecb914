"""GPU parity of k_om3wt (n = 10, m = 3: the wave-shared Philox pair table).

k_om3wt takes the pair-only half of Philox rounds 0-1 of a round's 21 leaf
calls from a per-wave table in LDS (csrc/ba_wave.hpp, Om3PairTable) instead of
computing it in every lane.  The lie stream may not move by a bit: decisions,
per-trial outcome bytes and all 12 run counters are compared with oracle_c.run,
with staged inputs (gen_inputs_device buffers, GIVEN mode) and in-kernel draws.

Batches: 1, 65, one task (512), one task plus a trial, and five tasks plus 37
trials under BA_WAVE_MAX_BLOCKS=1, where one wave rebuilds the table across
its tasks.  first_trial: 64*9; 64*(2^32 + 16), where the table holds gw_hi = 1;
64*(2^32 - 4) with 1,029 trials, which straddles a multiple of 2^32 trial words
and must fall back to k_om3w and still match.  profile_read shows which kernel
ran.  n = 11 stays on k_om3w.
"""
import ctypes

import numpy as np
import pytest

import oracle_c
from test_gpu import same
from test_gpu_om3w_trim import run_staged

pytestmark = pytest.mark.gpu

N, M, W = 10, 3, 8  # Om3W<10>::W = 8 words = 512 trials per task
FT_LOW, FT_HI1, FT_STRADDLE = 64 * 9, 64 * (2**32 + 16), 64 * (2**32 - 4)


def kw_for(first_trial, seed=0x7AB1E):
    from ba_amd import lib as L
    return dict(seed=seed, faulty_mode=L.FAULTY_RANDOM, f=4, order_mode=L.ORDER_RANDOM,
                first_trial=first_trial)


def check_case(n, B, kw, want_kernel, tag):
    """Drawn and staged runs of one case against the oracle, on a fresh engine
    whose profile names the kernel that ran."""
    from ba_amd import lib as L
    od, oo, ocnt = oracle_c.run(n, M, B, **kw)
    e = L.Engine(0)
    try:
        e.profile(True)
        res = e.run(n, M, B, **kw)
        same(res.decisions, od, "decisions, drawn " + tag)
        same(res.outcome, oo, "outcome, drawn " + tag)
        assert {k: res.counters[k] for k in ocnt} == ocnt, "drawn " + tag
        dec, out, cnt = run_staged(e, n, M, B, kw)
        same(dec, od, "decisions, staged " + tag)
        same(out, oo, "outcome, staged " + tag)
        assert cnt == list(ocnt.values()), "staged " + tag
        prof = e.profile_read()
    finally:
        e.close()
    ran = {k: v[0] for k, v in prof.items() if k.startswith("k_om3w")}
    assert ran == {want_kernel: 2}, (tag, prof)


@pytest.mark.parametrize("B,cap", [(1, None), (65, None), (64 * W, None), (64 * W + 1, None),
                                   (64 * W * 5 + 37, "1")])
def test_table_batches_vs_oracle(monkeypatch, B, cap):
    monkeypatch.delenv("BA_OM3W_TABLE", raising=False)
    if cap:
        monkeypatch.setenv("BA_WAVE_MAX_BLOCKS", cap)
    else:
        monkeypatch.delenv("BA_WAVE_MAX_BLOCKS", raising=False)
    check_case(N, B, kw_for(FT_LOW), "k_om3wt", f"B={B} cap={cap}")


@pytest.mark.parametrize("first_trial,B,kernel", [(FT_LOW, 64 * W + 1, "k_om3wt"),
                                                  (FT_HI1, 64 * W * 2 + 5, "k_om3wt"),
                                                  (FT_STRADDLE, 1029, "k_om3w")])
def test_first_trial_picks_the_kernel(monkeypatch, first_trial, B, kernel):
    """gw_hi = 0, gw_hi = 1 (both on the table path) and a launch whose words
    straddle 2^32 (the fallback), each against the oracle."""
    monkeypatch.delenv("BA_OM3W_TABLE", raising=False)
    monkeypatch.delenv("BA_WAVE_MAX_BLOCKS", raising=False)
    check_case(N, B, kw_for(first_trial, seed=0x51DE + (first_trial >> 38)), kernel,
               f"first_trial={first_trial} B={B}")


def test_switch_off_gives_identical_outputs(monkeypatch):
    """BA_OM3W_TABLE=0 forces k_om3w; outputs are those of the default."""
    from ba_amd import lib as L
    B, kw = 64 * W * 3 + 11, kw_for(FT_LOW, seed=0xAB)
    got = {}
    for tag, val, kernel in (("table", None, "k_om3wt"), ("off", "0", "k_om3w")):
        if val is None:
            monkeypatch.delenv("BA_OM3W_TABLE", raising=False)
        else:
            monkeypatch.setenv("BA_OM3W_TABLE", val)
        e = L.Engine(0)
        try:
            e.profile(True)
            res = e.run(N, M, B, **kw)
            prof = e.profile_read()
        finally:
            e.close()
        assert [k for k in prof if k.startswith("k_om3w")] == [kernel], prof
        got[tag] = res
    same(got["table"].decisions, got["off"].decisions, "decisions")
    same(got["table"].outcome, got["off"].outcome, "outcome")
    assert got["table"].counters == got["off"].counters
    od, oo, ocnt = oracle_c.run(N, M, B, **kw)
    same(got["table"].decisions, od, "decisions vs oracle")
    same(got["table"].outcome, oo, "outcome vs oracle")


def test_every_general_faulty_given_inputs(monkeypatch):
    """Given inputs with every general faulty: every relay takes its lie bit, so
    every word of every leaf call reaches the outputs."""
    from ba_amd import lib as L
    monkeypatch.delenv("BA_OM3W_TABLE", raising=False)
    monkeypatch.delenv("BA_WAVE_MAX_BLOCKS", raising=False)
    B = 64 * W * 2 + 3
    fm = np.full(B, (1 << N) - 1, np.uint32)
    oc = np.random.default_rng(10).choice([0, 1, 2], B).astype(np.uint8)
    od, oo, ocnt = oracle_c.run(N, M, B, seed=77, faulty=fm, order=oc, first_trial=FT_HI1)
    assert ocnt["faulty_total"] == N * B
    e = L.Engine(0)
    try:
        e.profile(True)
        res = e.run(N, M, B, seed=77, faulty=fm, order=oc, first_trial=FT_HI1)
        prof = e.profile_read()
    finally:
        e.close()
    assert "k_om3wt" in prof and "k_om3w" not in prof, prof
    same(res.decisions, od, "decisions")
    same(res.outcome, oo, "outcome")
    assert {k: res.counters[k] for k in ocnt} == ocnt


def test_n11_stays_on_k_om3w(monkeypatch):
    monkeypatch.delenv("BA_OM3W_TABLE", raising=False)
    monkeypatch.delenv("BA_WAVE_MAX_BLOCKS", raising=False)
    check_case(11, 64 * 7 + 1, kw_for(FT_LOW, seed=0xB11), "k_om3w", "n=11")


def test_three_blocks_per_cu_resident():
    """The staged kernel at its launch shape (256 threads, the four waves' LDS
    images) is resident three blocks per CU, as k_om3w is: the kernel is loaded
    from the library's own code object as a module and asked through
    hipModuleOccupancyMaxActiveBlocksPerMultiprocessor (nothing is launched)."""
    import re

    import codeobj
    from ba_amd import lib as L
    L.load()
    hip = ctypes.CDLL(_loaded_hip_runtime())  # the runtime the library itself runs on
    assert hip.hipSetDevice(0) == 0
    name, image = None, None
    for co in codeobj.code_objects():
        m = re.search(rb"_ZN2ba7k_om3wtILi10ELb1EE\w+", co)
        if m:
            name, image = m.group(0).decode(), co
    assert name is not None
    lds_dynamic = 4 * 8 * (1472 + 176)  # Om3WT<10>::words per wave (csrc/ba_wave.hpp)
    mod, fn, nb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int(0)
    buf = ctypes.create_string_buffer(image, len(image))
    assert hip.hipModuleLoadData(ctypes.byref(mod), buf) == 0
    try:
        assert hip.hipModuleGetFunction(ctypes.byref(fn), mod, name.encode()) == 0
        assert hip.hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(
            ctypes.byref(nb), fn, ctypes.c_int(256), ctypes.c_size_t(lds_dynamic)) == 0
    finally:
        hip.hipModuleUnload(mod)
    print("k_om3wt<10, staged>: blocks per CU =", nb.value)
    assert nb.value >= 3, nb.value


def _loaded_hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return line.split()[-1]
    raise AssertionError("the HIP runtime is not loaded")
