"""Reference model of OM(m) under scripted traitor policies (docs/SEMANTICS.md §7).

TEST INFRASTRUCTURE ONLY (not a test file).  Two implementations written apart
from each other and from the HIP kernel:

  recursion form -- §2.3's resolve_r / val_r recursion, one trial and one
                    lieutenant at a time, with §7's face rule in place of the coin.
  level form     -- §2.3's arrays L_k and R_p in lexicographic path rank, every
                    trial of the batch at once (one numpy column per trial).
                    `run` uses this one by default.

Synthetic inputs, the quorum and the outcome byte come from oracle/ba_oracle.py
(`gen`, `quorum` via `trial_outcome`); the counters are ba_oracle's list.
"""
from __future__ import annotations

import itertools

import numpy as np

import ba_oracle as O

SPLIT, FLIP, ANTI = 0, 1, 2
POLICIES = (SPLIT, FLIP, ANTI)
POLICY_NAMES = {SPLIT: "split", FLIP: "flip", ANTI: "anti"}
PATH_CAP = 1 << 24


def paths(n: int, m: int) -> int:
    """P(L-1, me): the leaf chains one receiver resolves (ba_adv_paths)."""
    if n < 1 or n > 32 or m > 8:
        return 0
    p = 1
    for i in range(O.effective_depth(n, m)):
        p *= n - 2 - i
    return p


# ---------------------------------------------------------------------------
# recursion form
# ---------------------------------------------------------------------------
def decisions_rec(n, m, policy, fmask, ob):
    """Root decisions of lieutenant ranks 0..L-1 in one trial."""
    L, me = n - 1, O.effective_depth(n, m)

    def faulty(g):
        return (fmask >> g) & 1

    def face(k, j, truth):
        if policy == SPLIT:
            return j & 1
        if policy == FLIP:
            return 1 - truth
        return j & 1 if k == 0 else 1 - level((j,))  # ANTI

    def level(tau):  # L_k[tau], k = len(tau) - 1
        k = len(tau) - 1
        sender = 0 if k == 0 else tau[-2] + 1
        truth = ob if k == 0 else level(tau[:-1])
        return face(k, tau[-1], truth) if faulty(sender) else truth

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
# level form: arrays [slots of the level][trials]
# ---------------------------------------------------------------------------
def decisions_levels(n, m, policy, fmasks, obs):
    """Root decisions [trial][lieutenant rank] of a batch of trials."""
    L, me = n - 1, O.effective_depth(n, m)
    B = len(fmasks)
    if L == 0:
        return [[] for _ in range(B)]
    fm = np.asarray(fmasks, np.uint64)
    F = np.stack([((fm >> np.uint64(g)) & np.uint64(1)).astype(np.uint8) for g in range(n)])  # [n][B]
    ob = np.asarray(obs, np.uint8)
    odd = (np.arange(L) & 1).astype(np.uint8)[:, None]
    # level 0: slot r; the sender is the commander
    truth = np.broadcast_to(ob, (L, B))
    lie0 = (1 - truth) if policy == FLIP else np.broadcast_to(odd, (L, B))
    L0 = np.where(F[0][None, :] == 1, lie0, truth).astype(np.uint8)
    levels = [L0]
    last = np.arange(L)                      # last lieutenant of each slot's path
    free = ~np.eye(L, dtype=bool)            # lieutenants not on the slot's path
    for k in range(1, me + 1):
        rows, cols = np.nonzero(free)        # children in lexicographic path rank
        truth = levels[-1][rows]
        Fs = F[last[rows] + 1]
        if policy == SPLIT:
            lie = np.broadcast_to(odd[cols], truth.shape)
        elif policy == FLIP:
            lie = 1 - truth
        else:
            lie = 1 - L0[cols]
        levels.append(np.where(Fs == 1, lie, truth).astype(np.uint8))
        free = free[rows]
        free[np.arange(len(cols)), cols] = False
        last = cols
    # majorities, leaves up: R_p[sr s + b] over L_p[sr s + b] and R_{p+1}[(sr s + a)(s-1) + b - [b > a]]
    R = levels[me].astype(np.int16)
    for p in range(me - 1, -1, -1):
        s = L - p
        Rn = R.reshape(-1, s, s - 1, B)      # [sr][a][child rank][trial]
        cnt = levels[p].reshape(-1, s, B).astype(np.int16)
        for b in range(s):
            for a in range(s):
                if a != b:
                    cnt[:, b] += Rn[:, a, b - (1 if b > a else 0)]
        if p == 0:
            R = np.where(2 * cnt > s, O.ATTACK, np.where(2 * cnt < s, O.RETREAT, O.UNDEFINED))
        else:
            R = (2 * cnt > s).astype(np.int16)
        R = R.reshape(-1, B)
    return [[int(R[r, t]) for r in range(L)] for t in range(B)]


# ---------------------------------------------------------------------------
# the run
# ---------------------------------------------------------------------------
def inputs(n, seed, faulty_mode, f, order_mode, order_value, t, i, faulty, order):
    gm, go = O.gen(n, seed, faulty_mode, f, order_mode, order_value, t)
    fmask = (faulty[i] if faulty_mode == O.FAULTY_GIVEN else gm) & ((1 << n) - 1)
    oc = order[i] if order_mode == O.ORDER_GIVEN else go
    return int(fmask), int(oc)


def run(n, m, policy, seed=0, faulty_mode=O.FAULTY_GIVEN, f=0, order_mode=O.ORDER_GIVEN,
        order_value=O.ATTACK, first_trial=0, batch=1, faulty=None, order=None, form="levels"):
    """(decisions, outcomes, counters dict) of trials [first_trial, + batch), like ba_oracle.run."""
    assert policy in POLICIES and first_trial % 64 == 0
    ins = [inputs(n, seed, faulty_mode, f, order_mode, order_value, first_trial + i, i, faulty,
                  order) for i in range(batch)]
    if form == "levels":
        decs = decisions_levels(n, m, policy, [fm for fm, _ in ins],
                                [int(oc == O.ATTACK) for _, oc in ins]) if batch else []
    else:
        decs = [decisions_rec(n, m, policy, fm, int(oc == O.ATTACK)) for fm, oc in ins]
    decisions, outcomes = [], []
    cnt = dict.fromkeys(O.COUNTERS, 0)
    for (fmask, oc), dec in zip(ins, decs):
        word = 0
        for r, d in enumerate(dec):
            word |= d << (2 * r)
        out = O.trial_outcome(n, m, fmask, oc, dec)
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
        cnt["bound_violations"] += int(inb and not (agree and (not appl or valid)))
        cnt["faulty_total"] += bin(fmask).count("1")
    return decisions, outcomes, cnt


def violated(out: int) -> bool:
    """IC1 or IC2 fails in a trial with this outcome byte."""
    return not ((out >> 2) & 1 and (not (out >> 3) & 1 or (out >> 4) & 1))


def census(n, m, policy, f, orders=(O.RETREAT, O.ATTACK), form="levels"):
    """(cases, violations, violating (mask, order) rows) over every f-subset of the n
    generals x the given orders."""
    rows = [(sum(1 << g for g in c), oc) for c in itertools.combinations(range(n), f)
            for oc in orders]
    _, outs, _ = run(n, m, policy, batch=len(rows), faulty=[r[0] for r in rows],
                     order=[r[1] for r in rows], form=form)
    bad = [r for r, o in zip(rows, outs) if violated(o)]
    return len(rows), len(bad), bad
