"""Reference model of RAND against the stalling adversary (docs/SEMANTICS.md §15).

TEST INFRASTRUCTURE ONLY (not a test file).  Two implementations written apart from
each other and from the HIP kernel:

  message form -- one trial at a time: the phases are rand_model.phase_step's, which is
                  handed §15's messages as callables (0 for a dead report, None for a
                  dead proposal).  What the traitors need to know, the loyal preferences
                  and the loyal proposals, is counted general by general from the
                  messages themselves.  `run` uses this form.
  plane form   -- 64 trials per word: planes x, D, V, F per general; the loyal attack
                  count a, a traitor's rank and the loyal proposal counts P1, P0 are
                  bit-sliced ripple counters, "rank(j) < t" is the bit-sliced comparison
                  a + rank(j) < floor(n/2), "P1 > P0" a bit-sliced comparison of two
                  counters.  Neither form knows that all loyal generals count alike.

Synthetic inputs and the outcome byte come from king_model and rand_model; the tosses
are rand_model's c(3p, 33 i) or c(3p, 0).  No message coin is drawn.  Both forms always
run all R phases: the kernel's early finish has to be invisible against them.
`stall_strategy` gives the play of one trial as a strategy of §14's space.
"""
from __future__ import annotations

import ba_oracle as O
import king_model as K
import rand_model as RM
import renum_model as RN

RAND_LOCAL, RAND_COMMON = RM.RAND_LOCAL, RM.RAND_COMMON
MAX_PHASES = 250
UNDECIDED, UNSAFE = RM.UNDECIDED, RM.UNSAFE
_M64 = (1 << 64) - 1


def coin_calls(n: int, phases: int, coin: int) -> int:
    """Philox calls per 64-trial word when every toss is drawn: R (n or 1); 0 for bad
    arguments."""
    if n < 1 or n > 32 or phases < 1 or phases > MAX_PHASES or coin not in (RAND_LOCAL, RAND_COMMON):
        return 0
    return phases * (n if coin == RAND_LOCAL else 1)


def rank(fmask: int, j: int) -> int:
    """The number of faulty generals with an index below j."""
    return bin(fmask & ((1 << j) - 1)).count("1")


# ---------------------------------------------------------------------------
# message form
# ---------------------------------------------------------------------------
def stall_phase(n, m, fmask, x, D, V, toss):
    """One phase of §15 on the state (x, D, V: lists of n): (x, D, V, t, value), where t
    is the number of traitors that report attack and value what they all propose."""
    def faulty(g):
        return (fmask >> g) & 1

    loyal = [g for g in range(n) if not faulty(g)]
    f = n - len(loyal)
    a = sum(x[g] for g in loyal)
    t = min(max(n // 2 - a, 0), f)

    def report(j, i):
        return 0 if faulty(i) else int(rank(fmask, j) < t)

    # the loyal generals' proposals, each from the n messages it is shown
    P = [0, 0]
    for i in loyal:
        c1 = sum(x[j] if j == i or not faulty(j) else report(j, i) for j in range(n))
        if 2 * c1 > n + m:
            P[1] += 1
        elif 2 * (n - c1) > n + m:
            P[0] += 1
    value = 0 if P[1] > P[0] else 1

    def propose(j, i):
        return None if faulty(i) else value

    x, D, V = RM.phase_step(n, m, fmask, x, D, V, report, propose, toss)
    return x, D, V, t, value


def round0(n, fmask, ob):
    """A faulty commander shows a loyal lieutenant r the bit r & 1, a faulty one retreat."""
    return RM.round0(n, fmask, ob, lambda r: 0 if (fmask >> r) & 1 else r & 1)


def play_message(n, m, R, coin, coins: RM.Coins, t, fmask, ob):
    """(states (x, D, V) of all n generals at the end of phases 0..R, [(t_p, value_p)]
    of phases 1..R)."""
    x = round0(n, fmask, ob)
    D, V = [0] * n, [0] * n
    hist, shown = [(list(x), list(D), list(V))], []
    for p in range(1, R + 1):
        x, D, V, tp, value = stall_phase(n, m, fmask, x, D, V,
                                         lambda i: coins(t, 3 * p, RM.toss_slot(coin, i)))
        hist.append((list(x), list(D), list(V)))
        shown.append((tp, value))
    return hist, shown


def history_message(n, m, R, coin, coins: RM.Coins, t, fmask, ob):
    return play_message(n, m, R, coin, coins, t, fmask, ob)[0]


def stall_strategy(coin, n, m, R, fmask, ob, seed, t):
    """Trial t of a STALL run with `seed` as a strategy S of §14's case (coin, n, m, R,
    fmask, order ob): reports [rank(j) < t_p], proposals (1, value_p), round 0 r & 1,
    and the seed's tosses."""
    coins = RM.Coins(seed)
    shown = play_message(n, m, R, coin, coins, t, fmask, ob)[1]

    def bit(q, j, i):
        return i & 1 if q == 0 else int(rank(fmask, j) < shown[(q + 2) // 3 - 1][0])

    return RN.strategy_of(coin, n, m, R, fmask, bit, lambda q, j, i: (1, shown[(q + 1) // 3 - 1][1]),
                          lambda p, g: coins(t, 3 * p, RM.toss_slot(coin, 0 if g is None else g)))


# ---------------------------------------------------------------------------
# plane form: 64 trials per word
# ---------------------------------------------------------------------------
def _tally(planes_in, width=6):
    cnt = [0] * width  # ripple counter, up to 32 in six planes
    for x in planes_in:
        for b in range(width):
            cnt[b], x = cnt[b] ^ x, cnt[b] & x
    return cnt


def _add(p, q):
    """Bit-sliced sum of two six-plane counters: seven planes."""
    out, carry = [], 0
    for a, b in zip(p, q):
        out.append(a ^ b ^ carry)
        carry = (a & b) | (carry & (a ^ b))
    return out + [carry]


def _greater(p, q):
    """Word of the trials whose counter p is above counter q."""
    gt, eq = 0, _M64
    for a, b in zip(reversed(p), reversed(q)):
        gt |= eq & a & ~b & _M64
        eq &= ~(a ^ b) & _M64
    return gt


def history_plane_word(n, m, R, coin, coins: RM.Coins, w, fmasks, obs):
    """Planes (x, D, V) at the end of phases 0..R for the trials 64 w + b, b < len(fmasks)."""
    nb = len(fmasks)
    F = [sum(((fmasks[b] >> g) & 1) << b for b in range(nb)) for g in range(n)]
    L = [~F[g] & _M64 for g in range(n)]
    OB = sum((obs[b] & 1) << b for b in range(nb))
    ge = K._count_ge
    T = (n + m) // 2 + 1  # 2 c > n + m  <=>  c >= T
    ranks = [_tally(F[:j]) for j in range(n)]

    x = [OB] + [(OB & ~F[0] & _M64) | (F[0] & L[r] & (_M64 if r & 1 else 0)) for r in range(1, n)]
    D, V = [0] * n, [0] * n
    hist = [(list(x), list(D), list(V))]
    for p in range(1, R + 1):
        a = _tally(x[g] & L[g] for g in range(n))
        # rank(j) < t = min(max(n/2 - a, 0), f)  <=>  a + rank(j) < n/2 for a faulty j
        attack = [~ge(_add(a, ranks[j]), n // 2) & _M64 for j in range(n)]
        A, Rt = [], []
        for i in range(n):
            c1 = _tally(x[j] if j == i else (x[j] & L[j]) | (F[j] & L[i] & attack[j]) for j in range(n))
            A.append(ge(c1, T))
            Rt.append(~ge(c1, n - T + 1) & _M64 if T <= n else 0)  # c0 >= T  <=>  c1 <= n - T
        more1 = _greater(_tally(A[g] & L[g] for g in range(n)), _tally(Rt[g] & L[g] for g in range(n)))
        nx = []
        for i in range(n):
            d1 = _tally(A[j] if j == i else (A[j] & L[j]) | (F[j] & L[i] & ~more1 & _M64) for j in range(n))
            d0 = _tally(Rt[j] if j == i else (Rt[j] & L[j]) | (F[j] & L[i] & more1) for j in range(n))
            v0 = ge(d0, m + 1)
            v1 = ge(d1, m + 1) & ~v0 & _M64
            has = v0 | v1
            new = ((v0 & ge(d0, T)) | (v1 & ge(d1, T))) & ~D[i] & _M64
            V[i] = (V[i] & ~new & _M64) | (new & v1)
            D[i] |= new
            slot = RM.toss_slot(coin, i)
            nx.append(v1 | (~has & coins.words(w, 3 * p, slot >> 1)[slot & 1] & _M64))
        x = nx
        hist.append((list(x), list(D), list(V)))
    return hist


# ---------------------------------------------------------------------------
# per-trial results and the run
# ---------------------------------------------------------------------------
def run(n, m, R, coin=RAND_COMMON, seed=0, faulty_mode=O.FAULTY_GIVEN, f=0, order_mode=O.ORDER_GIVEN,
        order_value=O.ATTACK, first_trial=0, batch=1, faulty=None, order=None, form="message"):
    """(decisions, outcomes, decided, counters dict) of trials [first_trial, + batch)."""
    assert first_trial % 64 == 0 and coin in (RAND_LOCAL, RAND_COMMON) and 1 <= R <= MAX_PHASES
    coins = RM.Coins(seed)
    ins = [K.inputs(n, seed, faulty_mode, f, order_mode, order_value, first_trial + i, i, faulty,
                    order) for i in range(batch)]
    if form == "message":
        hists = [history_message(n, m, R, coin, coins, first_trial + i, fm, int(oc == O.ATTACK))
                 for i, (fm, oc) in enumerate(ins)]
    else:
        hists = []
        for i0 in range(0, batch, 64):
            part = ins[i0:i0 + 64]
            hw = history_plane_word(n, m, R, coin, coins, (first_trial + i0) >> 6,
                                    [p[0] for p in part], [int(p[1] == O.ATTACK) for p in part])
            hists += [[tuple([(pl >> b) & 1 for pl in planes] for planes in ph) for ph in hw]
                      for b in range(len(part))]
    decisions, outcomes, decided = [], [], []
    cnt = dict.fromkeys(O.COUNTERS, 0)
    for (fmask, oc), hist in zip(ins, hists):
        dec = hist[-1][0][1:]
        out = RM.trial_outcome(n, m, fmask, oc, dec)
        decisions.append(sum(d << (2 * r) for r, d in enumerate(dec)))
        outcomes.append(out)
        decided.append(RM.decided_of(n, fmask, int(oc == O.ATTACK), hist))
        agree, appl, valid, inb = (out >> 2) & 1, (out >> 3) & 1, (out >> 4) & 1, (out >> 5) & 1
        cnt["trials"] += 1
        cnt["agreement"] += agree
        cnt["validity_applicable"] += appl
        cnt["validity"] += valid
        cnt[["quorum_retreat", "quorum_attack", "quorum_undetermined"][out & 3]] += 1
        cnt["attack_decisions"] += sum(dec)
        cnt["in_bound"] += inb
        cnt["bound_violations"] += int(inb and not (agree and (not appl or valid)))
        cnt["faulty_total"] += bin(fmask).count("1")
    return decisions, outcomes, decided, cnt
