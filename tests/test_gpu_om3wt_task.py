"""GPU parity of k_om3wt's per-task code around the rounds (n = 10, m = 3;
csrc/ba_om3_task.hpp and k_om3wt in csrc/ba_wave.hpp): the lane tables from
their closed forms, the task's LDS addresses without the `act` selects, the
root majorities in 32-bit halves into a dense A image, which the byte-sliced
epilogue reads.  None of it may move a bit: decisions, per-trial outcome bytes
and all 12 run counters are compared with oracle_c.run and with k_om3w
(BA_OM3W_TABLE=0), which keeps the per-member tables and the 64-bit roots.

Batches: three full tasks and a ragged one (64*8*3 + 37), one trial, one full
task; each as launched and under BA_WAVE_MAX_BLOCKS=1, where one wave walks
every task, so whatever a task leaves behind in registers or LDS meets the next
one.  first_trial 64*9, and 64*(2^32 + 16) where the pair table holds gw_hi = 1.
Inputs: in-kernel draws and staged buffers (check_case), and given faulty masks
drawn uniformly from all 2^10 sets -- most of them beyond m = 3 traitors -- with
given orders.  profile_read names the kernel that ran.
"""
import numpy as np
import pytest

import oracle_c
from test_gpu import same
from test_gpu_om3w_table import FT_HI1, FT_LOW, check_case, kw_for

pytestmark = pytest.mark.gpu

N, M, W = 10, 3, 8
TASK = 64 * W
BATCHES = [3 * TASK + 37, 1, TASK]
CAPS = [None, "1"]
FIRST = [FT_LOW, FT_HI1]


def set_cap(monkeypatch, cap):
    if cap:
        monkeypatch.setenv("BA_WAVE_MAX_BLOCKS", cap)
    else:
        monkeypatch.delenv("BA_WAVE_MAX_BLOCKS", raising=False)


@pytest.mark.parametrize("first_trial", FIRST, ids=["ft_low", "ft_hi1"])
@pytest.mark.parametrize("cap", CAPS, ids=["grid", "one_block"])
@pytest.mark.parametrize("B", BATCHES)
def test_drawn_and_staged_vs_oracle(monkeypatch, B, cap, first_trial):
    monkeypatch.delenv("BA_OM3W_TABLE", raising=False)
    set_cap(monkeypatch, cap)
    check_case(N, B, kw_for(first_trial, seed=0x7A5C + B), "k_om3wt",
               f"B={B} cap={cap} first_trial={first_trial}")


def run_both_ways(e, B, kw, fm, oc):
    """(drawn, given) results of one engine: in-kernel inputs, then given masks
    and orders."""
    drawn = e.run(N, M, B, **kw)
    given = e.run(N, M, B, seed=kw["seed"], faulty=fm, order=oc, first_trial=kw["first_trial"])
    return drawn, given


@pytest.mark.parametrize("first_trial", FIRST, ids=["ft_low", "ft_hi1"])
@pytest.mark.parametrize("cap", CAPS, ids=["grid", "one_block"])
@pytest.mark.parametrize("B", BATCHES)
def test_equals_k_om3w_and_oracle_on_any_faulty_set(monkeypatch, B, cap, first_trial):
    from ba_amd import lib as L
    set_cap(monkeypatch, cap)
    kw = kw_for(first_trial, seed=0xF00D + B)
    rng = np.random.default_rng(B + (first_trial >> 30))
    fm = rng.integers(0, 1 << N, B, dtype=np.uint64).astype(np.uint32)
    fm[0] = (1 << N) - 1                      # every general a traitor
    oc = rng.choice([0, 1, 2], B).astype(np.uint8)
    assert B == 1 or (np.array([bin(x).count("1") for x in fm]) > M).any()
    got = {}
    for tag, val, kernel in (("new", None, "k_om3wt"), ("old", "0", "k_om3w")):
        if val is None:
            monkeypatch.delenv("BA_OM3W_TABLE", raising=False)
        else:
            monkeypatch.setenv("BA_OM3W_TABLE", val)
        e = L.Engine(0)
        try:
            e.profile(True)
            got[tag] = run_both_ways(e, B, kw, fm, oc)
            prof = e.profile_read()
        finally:
            e.close()
        ran = {k: v[0] for k, v in prof.items() if k.startswith("k_om3w")}
        assert ran == {kernel: 2}, (tag, prof)
    want = (oracle_c.run(N, M, B, **kw),
            oracle_c.run(N, M, B, seed=kw["seed"], faulty=fm, order=oc, first_trial=first_trial))
    for k, what in enumerate(("drawn", "given")):
        new, old = got["new"][k], got["old"][k]
        od, oo, ocnt = want[k]
        assert len(ocnt) == 12
        same(new.decisions, old.decisions, f"decisions vs k_om3w, {what}")
        same(new.outcome, old.outcome, f"outcome vs k_om3w, {what}")
        assert new.counters == old.counters, what
        same(new.decisions, od, f"decisions vs oracle, {what}")
        same(new.outcome, oo, f"outcome vs oracle, {what}")
        assert {c: new.counters[c] for c in ocnt} == ocnt, what
