"""Reference model of randomized agreement: Ben-Or rounds with a local or a common
coin (docs/SEMANTICS.md §13).

TEST INFRASTRUCTURE ONLY (not a test file).  Two implementations written apart
from each other and from the HIP kernel:

  message form -- one trial at a time: every report and proposal is an explicit
                  message (None = no proposal), every tally an explicit integer, the
                  rules as §13 writes them.  One phase is `phase_step`, which takes
                  the traitors' messages and the coins as callables, so that a test
                  can walk every one of them.  `run` uses this form.
  plane form   -- 64 trials per word: planes x, D, V per general, ripple counters
                  over the senders' planes and the threshold form (c >= (n+m)/2 + 1,
                  d >= m + 1).

Synthetic inputs, the quorum and the outcome byte come from oracle/ba_oracle.py and
tests/king_model.py; the coins are this protocol's own, c(q, x) = coin(256 + q, x),
with the Philox block of (word, q, pair) cached.  Both forms always run all R
phases: the kernel's early finish has to be invisible against them.
"""
from __future__ import annotations

import ba_oracle as O
import king_model as K

RAND_TAG = 256  # ctr word 1 of the draws: c(q, x) = coin(256 + q, x)
KING_COIN, KING_SPLIT = K.KING_COIN, K.KING_SPLIT
RAND_LOCAL, RAND_COMMON = 0, 1
MAX_PHASES = 64
UNDECIDED, UNSAFE = 255, 254
MAX_M = 10
_M64 = (1 << 64) - 1


class Coins:
    """c(q, x) of §13 for one seed: ba_oracle.lie(seed, t, 256 + q, x)."""

    def __init__(self, seed: int):
        self.seed = seed
        self.key = (seed & O.M32, seed >> 32)
        self.blocks = {}

    def words(self, w: int, q: int, pair: int):
        """The 64-trial coin words of x = 2 pair and x = 2 pair + 1."""
        key = (w, q, pair)
        b = self.blocks.get(key)
        if b is None:
            o = O.philox4x32_10((pair, RAND_TAG + q, w & O.M32, w >> 32), self.key)
            b = self.blocks[key] = (o[1] << 32 | o[0], o[3] << 32 | o[2])
        return b

    def __call__(self, t: int, q: int, x: int) -> int:
        return (self.words(t >> 6, q, x >> 1)[x & 1] >> (t & 63)) & 1


def coin_calls(n: int, phases: int, coin: int) -> int:
    """Philox calls per 64-trial word when every sender is faulty in the word and
    every toss is drawn: ceil(n/2) (1 + 2 n R) + R (n or 1); 0 for bad arguments."""
    if n < 1 or n > 32 or phases < 1 or phases > MAX_PHASES or coin not in (RAND_LOCAL, RAND_COMMON):
        return 0
    return ((n + 1) // 2) * (1 + 2 * n * phases) + phases * (n if coin == RAND_LOCAL else 1)


def toss_slot(coin: int, i: int) -> int:
    """x of general i's toss c(3p, x): its own slot 33 i, or the one common slot 0."""
    return 33 * i if coin == RAND_LOCAL else 0


# ---------------------------------------------------------------------------
# message form
# ---------------------------------------------------------------------------
def phase_step(n, m, fmask, x, D, V, lie_report, lie_propose, toss):
    """One phase on the state (x, D, V: lists of n).  lie_report(j, i) and
    lie_propose(j, i) give the bit a faulty j shows i != j; toss(i) gives general
    i's coin of the phase and is called only where i has no value v."""
    def faulty(g):
        return (fmask >> g) & 1

    prop = []
    for i in range(n):
        c1 = sum(x[j] if j == i or not faulty(j) else lie_report(j, i) for j in range(n))
        c0 = n - c1
        prop.append(1 if 2 * c1 > n + m else (0 if 2 * c0 > n + m else None))
    nx, nD, nV = [], list(D), list(V)
    for i in range(n):
        d = [0, 0]
        for j in range(n):
            shown = prop[j] if j == i or not faulty(j) else lie_propose(j, i)
            if shown is not None:
                d[shown] += 1
        v = 0 if d[0] > m else (1 if d[1] > m else None)
        if v is None:
            nx.append(toss(i))
        else:
            nx.append(v)
            if 2 * d[v] > n + m and not nD[i]:
                nD[i], nV[i] = 1, v
    return nx, nD, nV


def round0(n, fmask, ob, lie0):
    """Preferences after the commander's send; lie0(r): what a faulty commander shows r."""
    return [ob] + [lie0(r) if fmask & 1 else ob for r in range(1, n)]


def history_message(n, m, R, policy, coin, coins: Coins, t, fmask, ob):
    """States (x, D, V) of all n generals at the end of phases 0..R."""
    def lie(q):
        return lambda j, r: r & 1 if policy == KING_SPLIT else coins(t, q, 32 * j + r)

    x = round0(n, fmask, ob, lambda r: lie(0)(0, r))
    D, V = [0] * n, [0] * n
    hist = [(list(x), list(D), list(V))]
    for p in range(1, R + 1):
        x, D, V = phase_step(n, m, fmask, x, D, V, lie(3 * p - 2), lie(3 * p - 1),
                             lambda i: coins(t, 3 * p, toss_slot(coin, i)))
        hist.append((list(x), list(D), list(V)))
    return hist


def unsafe_state(n, fmask, ob, x, D, V) -> bool:
    """§13's three unsafe conditions on the state at the end of one phase."""
    loyal = [g for g in range(n) if not (fmask >> g) & 1]
    dec = [g for g in loyal if D[g]]
    if len({V[g] for g in dec}) > 1:
        return True
    if any(x[g] != V[g] for g in dec):
        return True
    return bool(not fmask & 1 and any(V[g] != ob for g in dec))


def decided_of(n, fmask, ob, hist) -> int:
    """decided[t]: 254 if some phase ended unsafe, else the first phase at whose end
    every loyal general has D set (1 when there is none), else 255."""
    loyal = [g for g in range(n) if not (fmask >> g) & 1]
    first = UNDECIDED
    for p in range(1, len(hist)):
        x, D, V = hist[p]
        if unsafe_state(n, fmask, ob, x, D, V):
            return UNSAFE
        if first == UNDECIDED and all(D[g] for g in loyal):
            first = p
    return first


# ---------------------------------------------------------------------------
# plane form: 64 trials per word
# ---------------------------------------------------------------------------
def _tally(planes_in):
    cnt = [0] * 6  # ripple counter, up to 32
    for x in planes_in:
        for b in range(6):
            cnt[b], x = cnt[b] ^ x, cnt[b] & x
    return cnt


def history_plane_word(n, m, R, policy, coin, coins: Coins, w, fmasks, obs):
    """Planes (x, D, V) at the end of phases 0..R for the trials 64 w + b, b < len(fmasks)."""
    nb = len(fmasks)
    F = [sum(((fmasks[b] >> g) & 1) << b for b in range(nb)) for g in range(n)]
    OB = sum((obs[b] & 1) << b for b in range(nb))
    ge = K._count_ge
    T = (n + m) // 2 + 1  # 2 c > n + m  <=>  c >= T

    def word(q, xslot):
        return coins.words(w, q, xslot >> 1)[xslot & 1]

    def shown(q, j, r, truth, flip=False):
        if j == r or not F[j]:
            return truth
        c = (_M64 if r & 1 else 0) if policy == KING_SPLIT else word(q, 32 * j + r)
        if flip:
            c = ~c & _M64
        return (truth & ~F[j] & _M64) | (F[j] & c)

    x = [OB] + [shown(0, 0, r, OB) for r in range(1, n)]
    D, V = [0] * n, [0] * n
    hist = [(list(x), list(D), list(V))]
    for p in range(1, R + 1):
        A, Rt = [], []
        for i in range(n):
            c1 = _tally(shown(3 * p - 2, j, i, x[j]) for j in range(n))
            A.append(ge(c1, T))
            Rt.append(~ge(c1, n - T + 1) & _M64 if T <= n else 0)  # c0 >= T  <=>  c1 <= n - T
        nx = []
        for i in range(n):
            d1 = _tally(shown(3 * p - 1, j, i, A[j]) for j in range(n))
            d0 = _tally(shown(3 * p - 1, j, i, Rt[j], flip=True) for j in range(n))
            v0 = ge(d0, m + 1)
            v1 = ge(d1, m + 1) & ~v0 & _M64
            has = v0 | v1
            strong = (v0 & ge(d0, T)) | (v1 & ge(d1, T))
            new = strong & ~D[i] & _M64
            V[i] = (V[i] & ~new & _M64) | (new & v1)
            D[i] |= new
            c = word(3 * p, toss_slot(coin, i))
            nx.append(v1 | (~has & c & _M64))
        x = nx
        hist.append((list(x), list(D), list(V)))
    return hist


# ---------------------------------------------------------------------------
# per-trial results and the run
# ---------------------------------------------------------------------------
def trial_outcome(n, m, fmask, order_code, dec):
    """king_model's outcome byte with this protocol's in-bound rule: |F| <= m and n > 3m."""
    out = K.trial_outcome(n, m, fmask, order_code, dec) & ~32
    return out | int(bin(fmask).count("1") <= m and n > 3 * m) << 5


def run(n, m, R, policy=KING_COIN, coin=RAND_COMMON, seed=0, faulty_mode=O.FAULTY_GIVEN, f=0,
        order_mode=O.ORDER_GIVEN, order_value=O.ATTACK, first_trial=0, batch=1, faulty=None,
        order=None, form="message"):
    """(decisions, outcomes, decided, counters dict) of trials [first_trial, + batch)."""
    assert first_trial % 64 == 0 and policy in (KING_COIN, KING_SPLIT)
    assert coin in (RAND_LOCAL, RAND_COMMON) and 1 <= R <= MAX_PHASES
    coins = Coins(seed)
    ins = [K.inputs(n, seed, faulty_mode, f, order_mode, order_value, first_trial + i, i, faulty,
                    order) for i in range(batch)]
    if form == "message":
        hists = [history_message(n, m, R, policy, coin, coins, first_trial + i, fm, int(oc == O.ATTACK))
                 for i, (fm, oc) in enumerate(ins)]
    else:
        hists = []
        for i0 in range(0, batch, 64):
            part = ins[i0:i0 + 64]
            hw = history_plane_word(n, m, R, policy, coin, coins, (first_trial + i0) >> 6,
                                    [p[0] for p in part], [int(p[1] == O.ATTACK) for p in part])
            hists += [[tuple([(pl >> b) & 1 for pl in planes] for planes in ph) for ph in hw]
                      for b in range(len(part))]
    decisions, outcomes, decided = [], [], []
    cnt = dict.fromkeys(O.COUNTERS, 0)
    for (fmask, oc), hist in zip(ins, hists):
        dec = hist[-1][0][1:]
        dword = 0
        for r, d in enumerate(dec):
            dword |= d << (2 * r)
        out = trial_outcome(n, m, fmask, oc, dec)
        decisions.append(dword)
        outcomes.append(out)
        decided.append(decided_of(n, fmask, int(oc == O.ATTACK), hist))
        agree, appl, valid, inb = (out >> 2) & 1, (out >> 3) & 1, (out >> 4) & 1, (out >> 5) & 1
        cnt["trials"] += 1
        cnt["agreement"] += agree
        cnt["validity_applicable"] += appl
        cnt["validity"] += valid
        cnt[["quorum_retreat", "quorum_attack", "quorum_undetermined"][out & 3]] += 1
        cnt["attack_decisions"] += sum(1 for d in dec if d == O.ATTACK)
        cnt["in_bound"] += inb
        cnt["bound_violations"] += int(inb and not (agree and (not appl or valid)))
        cnt["faulty_total"] += bin(fmask).count("1")
    return decisions, outcomes, decided, cnt


def reachable(n, m, R, coin, fmask, ob):
    """Every state (x, D, V, unsafe so far) the loyal generals can be in after R
    phases, over every message of the traitors in `fmask` (rounds 0, 3p-2, 3p-1:
    one bit per faulty sender and loyal recipient) and every coin outcome (LOCAL:
    one bit per loyal general that tosses; COMMON: one bit per phase).  A faulty
    general's own state reaches nobody and is left out (kept at 0)."""
    import itertools
    loyal = [g for g in range(n) if not (fmask >> g) & 1]
    bad = [g for g in range(n) if (fmask >> g) & 1]
    pairs = [(j, i) for j in bad for i in loyal]

    def scrub(x, D, V):  # drop the faulty generals' own state
        return tuple(tuple(0 if (fmask >> g) & 1 else s[g] for g in range(n)) for s in (x, D, V))

    starts = set()
    for bits in itertools.product((0, 1), repeat=len(loyal) if fmask & 1 else 0):
        shown = dict(zip(loyal, bits))
        x = round0(n, fmask, ob, lambda r: shown.get(r, 0))
        starts.add(scrub(x, [0] * n, [0] * n) + (False,))
    states = starts
    for _ in range(R):
        nxt = set()
        for x, D, V, was_unsafe in states:
            for rb in itertools.product((0, 1), repeat=len(pairs)):
                rep = dict(zip(pairs, rb))
                for pb in itertools.product((0, 1), repeat=len(pairs)):
                    prp = dict(zip(pairs, pb))
                    ncoin = len(loyal) if coin == RAND_LOCAL else 1
                    seen = set()
                    for cb in itertools.product((0, 1), repeat=ncoin):
                        asked = []

                        def toss(i):
                            if (fmask >> i) & 1:
                                return 0
                            k = loyal.index(i) if coin == RAND_LOCAL else 0
                            asked.append(k)
                            return cb[k]

                        st = scrub(*phase_step(n, m, fmask, list(x), list(D), list(V),
                                               lambda j, i: rep.get((j, i), 0),
                                               lambda j, i: prp.get((j, i), 0), toss))
                        if st in seen:
                            continue
                        seen.add(st)
                        nxt.add(st + (was_unsafe or unsafe_state(n, fmask, ob, *st),))
                        if not asked:
                            break  # no general tossed: the coins change nothing
        states = nxt
    return states
