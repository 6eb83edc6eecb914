"""Coin trials, scripted policies and ba.py's coin tables as strategies of §8's space
(docs/SEMANTICS.md §8, "Coins, policies and tables as strategies").

TEST INFRASTRUCTURE ONLY (not a test file).  The slot list is the library's
(`lib.enum_slots`, `lib.path_of_rank`, both host-only), never enum_model's, so the map
under test is the one a user of `decode_strategy` gets.  Nothing here evaluates a relay
tree: the strategy bits are a coin per slot, a closed form of the slot's path, or a table
position.
"""
from __future__ import annotations

import numpy as np

import ba_oracle as O
from ba_amd import lib as L

SPLIT, FLIP, ANTI = 0, 1, 2
POLICIES = (SPLIT, FLIP, ANTI)

# The cases of identities 1 and 2: shape -> faulty masks.  Every case has B <= 48 and at
# most 4,096 tree slots.  Depth 4 with a faulty lieutenant needs B = 64 at n = 6 and is out
# of k_enum's reach, so (7, 4) and (10, 3) are commander-only.
CASES = {
    (4, 1): tuple(range(16)),
    (5, 2): tuple(range(32)),
    (5, 3): tuple(range(32)),
    (6, 1): (0b000111, 0b001110, 0b000110),
    (6, 2): (1, 2, 3, 6, 7, 0b1010),
    (6, 3): (1, 2, 3, 0b10000),
    (7, 2): (1, 2, 3, 6, 7, 0b1110, 0b101000),
    (7, 4): (1,),
    (10, 3): (1,),
}
# The shapes whose cases can tell a wrong bit order from a right one.  In the other two
# only the commander is faulty: every loyal lieutenant takes a majority over the same L
# level-0 bits, whatever their order.
SENSITIVE = ((4, 1), (5, 2), (5, 3), (6, 1), (6, 2), (6, 3), (7, 2))

# The cases of identity 3 (m = 1): n -> faulty masks.
TABLE_CASES = {
    3: tuple(range(8)),
    4: tuple(range(16)),
    5: (1, 2, 3, 6, 7, 0b01110, 0b11111),
    6: (0b000111, 0b001110),
    7: (0b0001110, 0b0000111),
}


def paths(n, m, F):
    """Relay paths of free bits 0..B-1, by the library's slot list."""
    return [L.path_of_rank(n, k, x) for k, x in L.enum_slots(n, m, F)]


def loyal_mask(n, F):
    """Bits [2(r-1), 2(r-1)+1] of a decisions word for every loyal lieutenant r."""
    return sum(3 << (2 * (r - 1)) for r in range(1, n) if not (F >> r) & 1)


def no_dead_slot(n, F):
    """At most one general is faulty: no message goes from a traitor to a traitor."""
    return bin(F & ((1 << n) - 1)).count("1") <= 1


def agree(n, F, dec_a, out_a, dec_b, out_b):
    """Identities 1 and 2: two runs of one strategy agree on the loyal lieutenants'
    decisions and on outcome bits 2-5; with no dead slot, on both words in full."""
    if no_dead_slot(n, F):
        return int(dec_a) == int(dec_b) and int(out_a) == int(out_b)
    lm = loyal_mask(n, F)
    return int(dec_a) & lm == int(dec_b) & lm and int(out_a) & 0x3C == int(out_b) & 0x3C


def s_coin(n, m, F, seed, t):
    """The strategy coin trial t plays: bit i is §3's coin of free slot i."""
    return sum(O.lie(seed, t, k, x) << i for i, (k, x) in enumerate(L.enum_slots(n, m, F)))


def policy_bit(policy, F, ob, tau):
    """What a scripted traitor puts into the free slot tau = (j_0, .., j_k), by tau alone."""
    k = len(tau) - 1
    if policy == SPLIT:
        return tau[-1] & 1
    if policy == FLIP:  # every faulty sender of the chain flips once
        senders = [0] + [j + 1 for j in tau[:-1]]
        return ob ^ (sum((F >> g) & 1 for g in senders) & 1)
    if policy == ANTI:
        if k == 0:
            return tau[0] & 1
        return 1 - ((tau[-1] & 1) if F & 1 else ob)
    raise ValueError(policy)


def s_policy(n, m, F, order, policy):
    """The strategy a scripted policy plays in the case (n, m, F, order)."""
    ob = int(order == O.ATTACK)
    return sum(policy_bit(policy, F, ob, tau) << i for i, tau in enumerate(paths(n, m, F)))


def reverse_bits(S, B):
    """Bit i <-> bit B-1-i: a wrong map the case list must be able to tell from the right one."""
    return sum(((S >> i) & 1) << (B - 1 - i) for i in range(B))


def table_order(n, F):
    """Free-bit index of every coin of ba.py's canonical draw order at m = 1 (§3), -1 for a
    coin whose recipient is faulty (a dead slot): level 0 with r ascending when the
    commander is faulty, then receiver-major, r ascending, faulty j ascending, j != r."""
    bit = {tau: i for i, tau in enumerate(paths(n, 1, F))}
    order = []
    if F & 1:
        order += [bit.get((r - 1,), -1) for r in range(1, n)]
    for r in range(1, n):
        order += [bit.get((j - 1, r - 1), -1) for j in range(1, n) if j != r and (F >> j) & 1]
    assert sorted(i for i in order if i >= 0) == list(range(len(bit)))  # every free bit once
    return order


def table_rows(n, F, strategies):
    """Table-mode rows (uint32 [len(strategies)][table_stride(n)]) that carry the given
    strategies of the case (n, 1, F): coin c is the strategy bit of its slot, 0 (retreat)
    in a dead slot."""
    S = np.asarray(strategies, np.uint64)
    tab = np.zeros((len(S), L.table_stride(n)), np.uint32)
    for c, i in enumerate(table_order(n, F)):
        if i >= 0:
            tab[:, c >> 5] |= (((S >> np.uint64(i)) & np.uint64(1)) << np.uint64(c & 31)).astype(np.uint32)
    return tab


def row_coins(row, count):
    """The first `count` coins of a table row as a list (for the CPU oracle)."""
    return [(int(row[c >> 5]) >> (c & 31)) & 1 for c in range(count)]
