"""Reference model of OM(m) against every traitor strategy (docs/SEMANTICS.md §8).

TEST INFRASTRUCTURE ONLY (not a test file).  Two implementations written apart
from each other and from the HIP kernel:

  recursion form -- §2.3's resolve_r / val_r recursion, one strategy and one
                    lieutenant at a time; the free slots are numbered by sorting
                    their (level, path rank) keys.
  level form     -- §2.3's arrays L_k and R_p in lexicographic path rank, every
                    strategy of the range at once (one numpy column per strategy);
                    the free slots are numbered by a counter that runs along the
                    arrays.  `run` uses this one by default.

The quorum and the outcome byte come from oracle/ba_oracle.py (`trial_outcome`);
the counters are ba_oracle's list.
"""
from __future__ import annotations

import itertools
import math

import numpy as np

import ba_oracle as O

MAX_BITS = 48
MAX_SLOTS = 4096
NO_WITNESS = (1 << 64) - 1
TRUTH, FREE, DEAD = "truth", "free", "dead"


def _mask(n, F):
    return F & ((1 << n) - 1)


def bits_formula(n, m, F):
    """B = [F_0](L - f_L) + f_L (L - f_L) sum_{k=1..me} P(L-2, k-1)."""
    F = _mask(n, F)
    L, me = n - 1, O.effective_depth(n, m)
    fl = bin(F >> 1).count("1")
    chains = sum(math.perm(L - 2, k - 1) for k in range(1, me + 1))
    return (F & 1) * (L - fl) + fl * (L - fl) * chains


def slot_class(F, tau):
    """Class of the slot L_k[tau]: by its sender and its recipient."""
    sender = 0 if len(tau) == 1 else tau[-2] + 1
    if not (F >> sender) & 1:
        return TRUTH
    return DEAD if (F >> (tau[-1] + 1)) & 1 else FREE


def free_slots(n, m, F):
    """[(level, path rank)] of free bits 0..B-1: (level, rank) ascending."""
    F = _mask(n, F)
    L, me = n - 1, O.effective_depth(n, m)
    if L == 0:
        return []
    keys = [(k, O.path_rank(tau, L)) for k in range(me + 1)
            for tau in itertools.permutations(range(L), k + 1) if slot_class(F, tau) == FREE]
    return sorted(keys)


def dead_slots(n, m, F):
    F = _mask(n, F)
    L, me = n - 1, O.effective_depth(n, m)
    return sum(1 for k in range(me + 1) for tau in itertools.permutations(range(L), k + 1)
               if slot_class(F, tau) == DEAD) if L else 0


def bits(n, m, F):
    return len(free_slots(n, m, F))


# ---------------------------------------------------------------------------
# recursion form
# ---------------------------------------------------------------------------
def decisions_rec(n, m, F, ob, S, index=None):
    """Root decisions of lieutenant ranks 0..L-1 under strategy S."""
    F = _mask(n, F)
    L, me = n - 1, O.effective_depth(n, m)
    if index is None:
        index = {key: i for i, key in enumerate(free_slots(n, m, F))}

    def level(tau):  # L_k[tau], k = len(tau) - 1
        k = len(tau) - 1
        cls = slot_class(F, tau)
        if cls == TRUTH:
            return ob if k == 0 else level(tau[:-1])
        if cls == DEAD:
            return 0
        return (S >> index[(k, O.path_rank(tau, L))]) & 1

    def resolve(sigma, r):
        v = level(sigma + (r,))  # val_r(sigma)
        if len(sigma) == me:
            return v
        a, c = v, 1
        for j in range(L):
            if j in sigma or j == r:
                continue
            a += resolve(sigma + (j,), r)
            c += 1
        if not sigma:
            return O.ATTACK if 2 * a > c else (O.RETREAT if 2 * a < c else O.UNDEFINED)
        return 1 if 2 * a > c else 0

    return [resolve((), r) for r in range(L)]


# ---------------------------------------------------------------------------
# level form: arrays [slots of the level][strategies]
# ---------------------------------------------------------------------------
def decisions_levels(n, m, F, ob, strategies):
    """Root decisions [strategy][lieutenant rank] of a list of strategies."""
    F = _mask(n, F)
    L, me = n - 1, O.effective_depth(n, m)
    T = len(strategies)
    if L == 0:
        return [[] for _ in range(T)]
    S = np.asarray(strategies, np.uint64)
    faulty = np.array([(F >> g) & 1 for g in range(n)], bool)
    nxt = [0]  # the next free bit: levels in order, slots of a level in array order

    def fill(truth, snd_faulty, rcp_faulty):
        out = np.empty_like(truth)
        for x in range(truth.shape[0]):
            if not snd_faulty[x]:
                out[x] = truth[x]
            elif rcp_faulty[x]:
                out[x] = 0
            else:
                out[x] = ((S >> np.uint64(nxt[0])) & np.uint64(1)).astype(np.uint8)
                nxt[0] += 1
        return out

    truth0 = np.full((L, T), ob, np.uint8)
    levels = [fill(truth0, np.full(L, faulty[0]), faulty[1:])]
    last = np.arange(L)                      # last lieutenant of each slot's path
    free = ~np.eye(L, dtype=bool)            # lieutenants not on the slot's path
    for _ in range(1, me + 1):
        rows, cols = np.nonzero(free)        # children in lexicographic path rank
        levels.append(fill(levels[-1][rows], faulty[last[rows] + 1], faulty[cols + 1]))
        free = free[rows]
        free[np.arange(len(cols)), cols] = False
        last = cols
    # majorities, leaves up: R_p[sr s + b] over L_p[sr s + b] and R_{p+1}[(sr s + a)(s-1) + b - [b > a]]
    R = levels[me].astype(np.int16)
    for p in range(me - 1, -1, -1):
        s = L - p
        Rn = R.reshape(-1, s, s - 1, T)      # [sr][a][child rank][strategy]
        cnt = levels[p].reshape(-1, s, T).astype(np.int16)
        for b in range(s):
            for a in range(s):
                if a != b:
                    cnt[:, b] += Rn[:, a, b - (1 if b > a else 0)]
        if p == 0:
            R = np.where(2 * cnt > s, O.ATTACK, np.where(2 * cnt < s, O.RETREAT, O.UNDEFINED))
        else:
            R = (2 * cnt > s).astype(np.int16)
        R = R.reshape(-1, T)
    return [[int(R[r, t]) for r in range(L)] for t in range(T)]


# ---------------------------------------------------------------------------
# the run
# ---------------------------------------------------------------------------
def violated(out: int) -> bool:
    """IC1 fails, or IC2 is applicable and fails, in a trial with this outcome byte."""
    return not ((out >> 2) & 1 and (not (out >> 3) & 1 or (out >> 4) & 1))


def run(n, m, F, order, first=0, count=None, form="levels"):
    """(decisions, outcomes, counters dict, witness) of strategies [first, first + count);
    count=None: up to the end of the space.  witness: the smallest violating strategy of
    the range, NO_WITNESS when there is none."""
    F = _mask(n, F)
    B = bits(n, m, F)
    assert first % 64 == 0 and B <= MAX_BITS
    if count is None:
        count = (1 << B) - first
    assert 0 <= count and first + count <= 1 << B
    ob = int(order == O.ATTACK)
    strategies = list(range(first, first + count))
    if form == "levels":
        decs = decisions_levels(n, m, F, ob, strategies) if count else []
    else:
        index = {key: i for i, key in enumerate(free_slots(n, m, F))}
        decs = [decisions_rec(n, m, F, ob, S, index) for S in strategies]
    decisions, outcomes = [], []
    cnt = dict.fromkeys(O.COUNTERS, 0)
    witness = NO_WITNESS
    for S, dec in zip(strategies, decs):
        word = 0
        for r, d in enumerate(dec):
            word |= d << (2 * r)
        out = O.trial_outcome(n, m, F, order, dec)
        decisions.append(word)
        outcomes.append(out)
        agree, appl, valid, inb = (out >> 2) & 1, (out >> 3) & 1, (out >> 4) & 1, (out >> 5) & 1
        cnt["trials"] += 1
        cnt["agreement"] += agree
        cnt["validity_applicable"] += appl
        cnt["validity"] += valid
        cnt[["quorum_retreat", "quorum_attack", "quorum_undetermined"][out & 3]] += 1
        cnt["undefined_decisions"] += sum(1 for d in dec if d == O.UNDEFINED)
        cnt["attack_decisions"] += sum(1 for d in dec if d == O.ATTACK)
        cnt["in_bound"] += inb
        cnt["bound_violations"] += int(inb and violated(out))
        cnt["faulty_total"] += bin(F).count("1")
        if violated(out) and S < witness:
            witness = S
    return decisions, outcomes, cnt, witness


def violations(outcomes) -> int:
    return sum(1 for o in outcomes if violated(int(o)))
