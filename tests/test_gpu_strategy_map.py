"""GPU tests that tie OM(m)'s three adversaries to one relay tree (docs/SEMANTICS.md §8,
"Coins, policies and tables as strategies").  The coin engines are anchored outside this
project (the C oracle, and through it ba.py's transcripts); k_adv and k_enum are otherwise
compared only with models written beside them.  Here a coin trial, a scripted policy and a
ba.py coin table are each mapped to one strategy index S by the library's own slot list
(tests/strategy_map.py: slot lists and closed forms, no tree evaluation) and k_enum must
compute at S what the other kernel computed:

  1. coin trial t == k_enum at S_coin(t), after the engines agree with each other and
     with oracle_c.run;
  2. k_adv under a policy == k_enum at S_policy;
  3. at m = 1, k_table on one row per strategy == k_enum over the whole space, in
     decisions, outcome bytes, all 12 counters and the witness.

Identities 1 and 2 hold on the loyal lieutenants' decisions and outcome bits 2-5; with at
most one faulty general (no dead slot) on both words in full.  Every comparison is exact.
Depth 4 with a faulty lieutenant needs B = 64 at n = 6, out of k_enum's reach: (7, 4) and
(10, 3) are commander-only.  B = 45 at (7, 2) puts S above 2^32.  The file makes
102 * 3 * 16 + 102 * 3 * 3 + 107 = 5,921 run_enum calls."""
import numpy as np
import pytest

import enum_model as E
import oracle_c
import strategy_map as M
from test_gpu import _engines, same

pytestmark = pytest.mark.gpu

SEED = 0x5157ED0123456789
FIRST = 64 * 5
BATCH = 64
PICKED = (0, 1, 31, 32, 63, 5, 9, 14, 20, 27, 38, 41, 46, 50, 55, 60)  # 16 of the 64 trials
ORDERS = (0, 1, 2)


def describe(n, m, F, o, what, S, got, want):
    from ba_amd import lib as L
    return (f"n={n} m={m} F={F:#b} o={o} {what} S={S}: strategy {L.decode_strategy(n, m, F, S)}; "
            f"decisions {int(got[0]):#x} / k_enum {int(want[0]):#x}, "
            f"outcome {int(got[1]):#04x} / k_enum {int(want[1]):#04x}")


def enum_at(engine, n, m, F, o, S):
    """(decisions, outcome) of strategy S: the 64-strategy word that holds it."""
    from ba_amd import lib as L
    first = S & ~63
    res = engine.run_enum(n, m, F, o, first=first, count=min(64, (1 << L.enum_bits(n, m, F)) - first),
                          want_decisions=True, want_outcome=True)
    return res.decisions[S & 63], res.outcome[S & 63]


def check_reach(n, m, F):
    from ba_amd import lib as L
    assert L.load().ba_tree_slots(n, m) <= E.MAX_SLOTS, (n, m)
    B = L.enum_bits(n, m, F)
    assert B == E.bits(n, m, F) <= E.MAX_BITS, (n, m, F)
    return B


def coin_launches(engine, n, m, F, o):
    """One 64-trial coin launch of the case on AUTO and on every engine of (n, m), each
    equal to the oracle; at (10, 3) also k_om3w in place of k_om3wt."""
    from ba_amd import lib as L
    kw = dict(seed=SEED, first_trial=FIRST, faulty=np.full(BATCH, F, np.uint32),
              order=np.full(BATCH, o, np.uint8))
    od, oo, ocnt = oracle_c.run(n, m, BATCH, **kw)
    for eng in [L.ENGINE_AUTO] + _engines(n, m):
        res = engine.run(n, m, BATCH, engine=eng, **kw)
        what = f"n={n} m={m} F={F:#b} o={o} engine={eng}"
        same(res.decisions, od, what + " decisions vs oracle")
        same(res.outcome, oo, what + " outcome vs oracle")
        assert {k: res.counters[k] for k in ocnt} == ocnt, what
    return od, oo


def wave_kernel_launch(monkeypatch, switch, kernel, F, o):
    """(10, 3) on a fresh engine whose profile names the wave kernel that ran."""
    from ba_amd import lib as L
    if switch is None:
        monkeypatch.delenv("BA_OM3W_TABLE", raising=False)
    else:
        monkeypatch.setenv("BA_OM3W_TABLE", switch)
    e = L.Engine(0)
    try:
        e.profile(True)
        res = e.run(10, 3, BATCH, seed=SEED, first_trial=FIRST, faulty=np.full(BATCH, F, np.uint32),
                    order=np.full(BATCH, o, np.uint8))
        prof = e.profile_read()
    finally:
        e.close()
    assert [k for k in prof if k.startswith("k_om3w")] == [kernel], prof
    return res


@pytest.mark.parametrize("o", ORDERS)
@pytest.mark.parametrize("n,m", sorted(M.CASES))
def test_coin_trial_is_a_strategy(engine, monkeypatch, n, m, o):
    """Identity 1, for 16 of the 64 trials of every case."""
    calls = 0
    for F in M.CASES[n, m]:
        B = check_reach(n, m, F)
        dec, out = coin_launches(engine, n, m, F, o)
        if (n, m) == (10, 3):
            for switch, kernel in ((None, "k_om3wt"), ("0", "k_om3w")):
                res = wave_kernel_launch(monkeypatch, switch, kernel, F, o)
                same(res.decisions, dec, kernel + " decisions vs oracle")
                same(res.outcome, out, kernel + " outcome vs oracle")
        for i in PICKED:
            t = FIRST + i
            S = M.s_coin(n, m, F, SEED, t)
            assert 0 <= S < 1 << B
            got, want = (dec[i], out[i]), enum_at(engine, n, m, F, o, S)
            calls += 1
            assert M.agree(n, F, *got, *want), describe(n, m, F, o, f"t={t}", S, got, want)
    print(f"({n},{m}) o={o}: {calls} run_enum calls")


def test_strategies_above_2_to_the_32_are_reached():
    """(7, 2) F = {1, 2, 3}: 45 bits, so the coin strategies exercise k_enum's 64-bit word
    index; all 16 picked trials lie above 2^32 and are distinct."""
    S = {M.s_coin(7, 2, 0b1110, SEED, FIRST + i) for i in PICKED}
    assert len(PICKED) == len(set(PICKED)) == len(S) == 16 and min(S) >> 32 and max(S) >> 44


@pytest.mark.parametrize("n,m", sorted(M.CASES))
def test_policy_is_a_strategy(engine, n, m):
    """Identity 2: one k_adv launch per policy over every (F, o) of the shape."""
    rows = [(F, o) for F in M.CASES[n, m] for o in ORDERS]
    fm = np.array([r[0] for r in rows], np.uint32)
    oc = np.array([r[1] for r in rows], np.uint8)
    for F in M.CASES[n, m]:
        check_reach(n, m, F)
    calls = 0
    for policy in M.POLICIES:
        res = engine.run_adv(n, m, len(rows), policy, faulty=fm, order=oc)
        assert res.counters["trials"] == len(rows)
        for i, (F, o) in enumerate(rows):
            S = M.s_policy(n, m, F, o, policy)
            got, want = (res.decisions[i], res.outcome[i]), enum_at(engine, n, m, F, o, S)
            calls += 1
            assert M.agree(n, F, *got, *want), describe(n, m, F, o, f"policy={policy}", S, got, want)
    print(f"({n},{m}): {calls} run_enum calls")


def check_table_case(engine, n, F, o):
    """Identity 3 for one case: every output of k_table on the strategies' rows equals
    k_enum's (and the oracle's table mode, the anchor)."""
    from ba_amd import lib as L
    B = check_reach(n, 1, F)
    T = 1 << B
    tab = M.table_rows(n, F, np.arange(T, dtype=np.uint64))
    kw = dict(lie_mode=L.LIE_TABLE, faulty=np.full(T, F, np.uint32), order=np.full(T, o, np.uint8),
              table=tab)
    res = engine.run(n, 1, T, **kw)
    od, oo, ocnt = oracle_c.run(n, 1, T, **kw)
    what = f"n={n} m=1 F={F:#b} o={o}"
    same(res.decisions, od, what + " table decisions vs oracle")
    same(res.outcome, oo, what + " table outcome vs oracle")
    assert {k: res.counters[k] for k in ocnt} == ocnt, what
    en = engine.run_enum(n, 1, F, o, want_decisions=True, want_outcome=True)
    bad = np.nonzero((en.decisions != res.decisions) | (en.outcome != res.outcome))[0]
    if len(bad):
        S = int(bad[0])
        raise AssertionError(f"{len(bad)} strategies differ, first: " + describe(
            n, 1, F, o, "table", S, (res.decisions[S], res.outcome[S]), (en.decisions[S], en.outcome[S])))
    assert len(en.counters) == 12 and en.counters == res.counters, what
    out = res.outcome.astype(np.int64)
    viol = np.nonzero(~(((out >> 2) & 1 == 1) & (((out >> 3) & 1 == 0) | ((out >> 4) & 1 == 1))))[0]
    assert en.witness == (int(viol[0]) if len(viol) else None), what


@pytest.mark.parametrize("n", sorted(M.TABLE_CASES))
def test_table_mode_carries_the_whole_space(engine, n):
    for F in M.TABLE_CASES[n]:
        for o in ORDERS:
            check_table_case(engine, n, F, o)


@pytest.mark.parametrize("o", [1, 0])
def test_table_mode_carries_262144_strategies(engine, o):
    """(10, 1) with three faulty lieutenants: B = 18, one k_table launch and one k_enum run."""
    from ba_amd import lib as L
    assert L.enum_bits(10, 1, 0b1110) == 18
    check_table_case(engine, 10, 0b1110, o)
