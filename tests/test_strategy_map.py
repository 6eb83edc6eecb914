"""CPU tests that tie OM(m)'s three adversaries to one relay tree (docs/SEMANTICS.md §8,
"Coins, policies and tables as strategies"): a coin trial, a scripted policy and a ba.py
coin table are each one strategy of §8's space, under the library's own slot list
(tests/strategy_map.py).  Here the identities are checked on the CPU models
(oracle/ba_oracle.py, tests/adv_model.py, tests/enum_model.py); tests/test_gpu_strategy_map.py
holds the kernels to them.  Also `encode_strategy`, the inverse of `decode_strategy`."""
import functools
import random

import numpy as np
import pytest

import adv_model as A
import ba_oracle as O
import enum_model as E
import strategy_map as M

SEED = 0xBA5EED
ORDERS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def model_index(n, m, F):
    """The enumeration model's own numbering of the free slots (not the library's)."""
    return {key: i for i, key in enumerate(E.free_slots(n, m, F))}


def word(dec):
    return sum(d << (2 * r) for r, d in enumerate(dec))


def enum_side(n, m, F, o, S):
    dec = E.decisions_rec(n, m, F, int(o == O.ATTACK), S, model_index(n, m, F))
    return word(dec), O.trial_outcome(n, m, F, o, dec)


def coin_side(n, m, F, o, t):
    dec = O.om_decisions(n, m, SEED, t, F, int(o == O.ATTACK))
    return word(dec), O.trial_outcome(n, m, F, o, dec)


def policy_side(n, m, F, o, policy):
    dec = A.decisions_rec(n, m, policy, F, int(o == O.ATTACK))
    return word(dec), O.trial_outcome(n, m, F, o, dec)


def test_case_list_is_within_k_enums_reach():
    from ba_amd import lib as L
    for (n, m), masks in M.CASES.items():
        assert L.load().ba_tree_slots(n, m) <= E.MAX_SLOTS, (n, m)
        for F in masks:
            assert L.enum_bits(n, m, F) == E.bits_formula(n, m, F) <= E.MAX_BITS, (n, m, F)
    assert E.bits_formula(7, 2, 0b1110) == 45 and E.bits_formula(6, 3, 0b11) == 44
    assert E.bits_formula(6, 4, 0b10) == 64  # depth 4 with one faulty lieutenant: out of reach
    assert sum(len(v) for v in M.CASES.values()) == 102


def test_loyal_mask_and_dead_slots():
    assert M.loyal_mask(4, 0) == 0b111111 and M.loyal_mask(4, 0b0001) == 0b111111
    assert M.loyal_mask(4, 0b0100) == 0b110011 and M.loyal_mask(4, 0b1110) == 0
    assert M.loyal_mask(1, 0) == 0
    for (n, m), masks in M.CASES.items():
        for F in masks:
            assert M.no_dead_slot(n, F) == (E.dead_slots(n, m, F) == 0), (n, m, F)


@pytest.mark.parametrize("n,m", sorted(M.CASES))
def test_coin_trial_is_a_strategy_on_the_models(n, m):
    """Identity 1: the oracle's coin trial t and the enumeration model at S_coin(t)."""
    for F in M.CASES[n, m]:
        for o in ORDERS:
            for t in range(320, 326):
                S = M.s_coin(n, m, F, SEED, t)
                a, b = coin_side(n, m, F, o, t), enum_side(n, m, F, o, S)
                assert M.agree(n, F, *a, *b), (n, m, F, o, t, S, a, b)


@pytest.mark.parametrize("n,m", sorted(M.CASES))
def test_policy_is_a_strategy_on_the_models(n, m):
    """Identity 2: the policy model's trial and the enumeration model at S_policy."""
    for F in M.CASES[n, m]:
        for o in ORDERS:
            for policy in M.POLICIES:
                S = M.s_policy(n, m, F, o, policy)
                a, b = policy_side(n, m, F, o, policy), enum_side(n, m, F, o, S)
                assert M.agree(n, F, *a, *b), (n, m, F, o, policy, S, a, b)


def test_table_mode_carries_the_whole_space_on_the_models():
    """Identity 3: ba.py's OM(1) on the table rows of every strategy equals the
    enumeration model in decisions, outcome bytes and all 12 counters; the smallest
    violating row is the witness."""
    from ba_amd import lib as L
    triples = 0
    for n, masks in M.TABLE_CASES.items():
        for F in masks:
            B = L.enum_bits(n, 1, F)
            tab = M.table_rows(n, F, np.arange(1 << B, dtype=np.uint64))
            assert tab.shape == (1 << B, L.table_stride(n))
            count = O.canonical_coin_count(n, F)
            assert count == len(M.table_order(n, F)) == B + E.dead_slots(n, 1, F)
            coins = [M.row_coins(row, count) for row in tab]
            for o in ORDERS:
                dec, out, cnt = O.run(n, 1, lie_mode=O.LIE_TABLE, batch=1 << B, faulty=[F] * (1 << B),
                                      order=[o] * (1 << B), table=coins)
                edec, eout, ecnt, wit = E.run(n, 1, F, o)
                assert (dec, out, cnt) == (edec, eout, ecnt), (n, F, o)
                bad = [S for S, x in enumerate(out) if E.violated(x)]
                assert wit == (bad[0] if bad else E.NO_WITNESS), (n, F, o)
                triples += 1 << B
    assert triples == 16461


ROUND_TRIP = [(4, 1, 0), (4, 1, 0b0011), (5, 2, 0b00110), (6, 3, 0b000011), (7, 2, 0b0001110)]


def test_encode_strategy_inverts_decode_strategy():
    from ba_amd import lib as L
    rng = random.Random(7)
    seen = set()
    for n, m, F in ROUND_TRIP:
        B = L.enum_bits(n, m, F)
        seen.add(B)
        for S in {0, (1 << B) - 1} | {rng.getrandbits(B) for _ in range(8)}:
            d = L.decode_strategy(n, m, F, S)
            assert len(d) == B and L.encode_strategy(n, m, F, d) == S, (n, m, F, S)
    assert {0, 45} <= seen
    assert L.encode_strategy(4, 1, 0, {}) == 0
    # (4, 1) F = {0, 1}: the witness of tests/test_enum_model.py, written by hand
    assert L.encode_strategy(4, 1, 0b0011, {(1,): 1, (2,): 0, (0, 1): 1, (0, 2): 0}) == 5
    assert L.encode_strategy(4, 1, 0b0011, {(0, 2): 0, (2,): 0, (0, 1): 1, (1,): 1}) == 5  # any key order


def test_encode_strategy_rejects_what_is_not_a_strategy():
    from ba_amd import lib as L
    good = {(1,): 1, (2,): 0, (0, 1): 1, (0, 2): 0}
    for bad in ({k: v for k, v in good.items() if k != (0, 2)},   # a free slot is missing
                {**good, (0,): 0},                                # a dead slot
                {**good, (1, 2): 1},                              # a truth slot
                {**good, (3,): 1},                                # no such lieutenant
                {**good, (1,): 2},                                # not a bit
                {}):
        with pytest.raises(ValueError):
            L.encode_strategy(4, 1, 0b0011, bad)
    with pytest.raises(ValueError):
        L.encode_strategy(4, 1, 0, {(0,): 1})  # no traitor: no free slot


def _mismatches_under_reversed_bits(n, m):
    """(coin mismatches, coin comparisons, policy mismatches, policy comparisons) of a
    shape when the strategy's bit order is reversed before it is evaluated."""
    from ba_amd import lib as L
    coin = coins = pol = pols = 0
    for F in M.CASES[n, m]:
        B = L.enum_bits(n, m, F)
        for o in (0, 1):
            for t in range(320, 336):
                S = M.reverse_bits(M.s_coin(n, m, F, SEED, t), B)
                coin += not M.agree(n, F, *coin_side(n, m, F, o, t), *enum_side(n, m, F, o, S))
                coins += 1
            for policy in M.POLICIES:
                S = M.reverse_bits(M.s_policy(n, m, F, o, policy), B)
                pol += not M.agree(n, F, *policy_side(n, m, F, o, policy), *enum_side(n, m, F, o, S))
                pols += 1
    return coin, coins, pol, pols


# shape -> (coin mismatches, coin comparisons, policy mismatches) with the bit order reversed
REVERSED = {(4, 1): (34, 512, 12), (5, 2): (408, 1024, 60), (5, 3): (424, 1024, 45),
            (6, 1): (25, 96, 6), (6, 2): (61, 192, 9), (6, 3): (16, 128, 4), (7, 2): (67, 224, 14)}


@pytest.mark.parametrize("n,m", M.SENSITIVE)
def test_case_list_tells_a_wrong_map_from_a_right_one(n, m):
    """With bit i and bit B-1-i of S swapped, identities 1 and 2 must each fail somewhere in
    every shape that has a faulty lieutenant: otherwise the list could not see a wrong
    free-slot order.  Orders retreat and attack, seed 0xBA5EED, trials 320..335.  The
    models give (coin mismatches / comparisons, policy mismatches):
      (4,1) 34/512, 12   (5,2) 408/1024, 60   (5,3) 424/1024, 45   (6,1) 25/96, 6
      (6,2) 61/192, 9    (6,3) 16/128, 4      (7,2) 67/224, 14
    The counts are those of the models, which do not change; the condition is at least one
    of each.  (7, 4) and (10, 3) have a faulty commander only and are blind to the order of
    the bits, as is every commander-only case: each loyal lieutenant takes a majority over
    the same L level-0 bits.  They stay in the list for the full-word equality."""
    coin, coins, pol, pols = _mismatches_under_reversed_bits(n, m)
    print(f"({n},{m}) reversed bit order: coin {coin}/{coins}, policy {pol}/{pols}")
    assert coin >= 1 and pol >= 1
    assert (coin, coins, pol) == REVERSED[n, m]


def test_commander_only_cases_are_blind_to_the_bit_order():
    for n, m in ((7, 4), (10, 3)):
        assert M.CASES[n, m] == (1,)
        for o, t in ((0, 320), (1, 321)):
            S = M.s_coin(n, m, 1, SEED, t)
            assert enum_side(n, m, 1, o, M.reverse_bits(S, n - 1)) == enum_side(n, m, 1, o, S) \
                == coin_side(n, m, 1, o, t)
