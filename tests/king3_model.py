"""Reference model of the three-round King algorithm (Berman, Garay, Perry;
docs/SEMANTICS.md §10).

TEST INFRASTRUCTURE ONLY (not a test file).  Two implementations written apart
from each other and from the HIP kernel:

  message form -- one trial at a time: every message of the value, propose and king
                  rounds is an explicit bit or trit (None = no proposal), every
                  tally an explicit integer, the rules as §10 writes them.  `run`
                  uses this one.
  plane form   -- 64 trials per word: one preference plane per general, ripple
                  counters over the senders' planes and the threshold form
                  (c1 >= n-m, c1 <= m, d0 >= m+1, d1 >= m+1, the `sure` select).

Synthetic inputs, the quorum, `settled` and the outcome byte come from
oracle/ba_oracle.py and tests/king_model.py; the coins are this protocol's own,
c(q, x) = coin(192 + q, x), with the Philox block of (word, q, pair) cached.
"""
from __future__ import annotations

import ba_oracle as O
import king_model as K

KING3_TAG = 192  # ctr word 1 of KING3 draws: c(q, x) = coin(192 + q, x)
KING_COIN, KING_SPLIT = K.KING_COIN, K.KING_SPLIT
UNSETTLED = K.UNSETTLED
MAX_M = 10
_M64 = (1 << 64) - 1


class Coins:
    """c(q, x) of §10 for one seed: ba_oracle.lie(seed, t, 192 + q, x)."""

    def __init__(self, seed: int):
        self.seed = seed
        self.key = (seed & O.M32, seed >> 32)
        self.blocks = {}

    def words(self, w: int, q: int, pair: int):
        """The 64-trial coin words of x = 2 pair and x = 2 pair + 1."""
        key = (w, q, pair)
        b = self.blocks.get(key)
        if b is None:
            o = O.philox4x32_10((pair, KING3_TAG + q, w & O.M32, w >> 32), self.key)
            b = self.blocks[key] = (o[1] << 32 | o[0], o[3] << 32 | o[2])
        return b

    def __call__(self, t: int, q: int, x: int) -> int:
        return (self.words(t >> 6, q, x >> 1)[x & 1] >> (t & 63)) & 1


def phases(n: int, m: int) -> int:
    """P = min(m, n - 1) + 1 (0 for n outside 1..32 or m > 10)."""
    if n < 1 or n > 32 or m < 0 or m > MAX_M:
        return 0
    return min(m, n - 1) + 1


def coin_calls(n: int, m: int) -> int:
    """Philox calls per 64-trial word: ceil(n/2) (1 + P (2n + 1))."""
    P = phases(n, m)
    if P == 0:
        return 0
    return ((n + 1) // 2) * (1 + P * (2 * n + 1))


# ---------------------------------------------------------------------------
# message form
# ---------------------------------------------------------------------------
def history_message(n, m, policy, coins: Coins, t, fmask, ob):
    """Preferences of all n generals at the end of phases 0..P: list of P+1 lists."""
    P = phases(n, m)

    def faulty(g):
        return (fmask >> g) & 1

    def lie(q, j, r):
        return r & 1 if policy == KING_SPLIT else coins(t, q, 32 * j + r)

    pref = [ob] + [lie(0, 0, r) if faulty(0) else ob for r in range(1, n)]
    hist = [list(pref)]
    for p in range(1, P + 1):
        k = p - 1
        # value round
        prop = []
        for i in range(n):
            c1 = sum(pref[j] if j == i or not faulty(j) else lie(3 * p - 2, j, i) for j in range(n))
            c0 = n - c1
            prop.append(0 if c0 >= n - m else (1 if c1 >= n - m else None))
        # propose round: a trit per message
        x, sure = [], []
        for i in range(n):
            d = [0, 0]
            for j in range(n):
                trit = prop[j] if j == i or not faulty(j) else lie(3 * p - 1, j, i)
                if trit is not None:
                    d[trit] += 1
            xi = 0 if d[0] > m else (1 if d[1] > m else pref[i])
            x.append(xi)
            sure.append(d[xi] >= n - m)
        # king round
        w = x[k]
        pref = [x[i] if sure[i] or i == k else (lie(3 * p, k, i) if faulty(k) else w)
                for i in range(n)]
        hist.append(list(pref))
    return hist


# ---------------------------------------------------------------------------
# plane form: 64 trials per word
# ---------------------------------------------------------------------------
def _tally(planes_in):
    cnt = [0] * 6  # ripple counter, up to 32
    for x in planes_in:
        for b in range(6):
            cnt[b], x = cnt[b] ^ x, cnt[b] & x
    return cnt


def history_plane_word(n, m, policy, coins: Coins, w, fmasks, obs):
    """Preference planes at the end of phases 0..P for the trials 64 w + b,
    b < len(fmasks): list of P+1 lists of n words."""
    P = phases(n, m)
    nb = len(fmasks)
    F = [sum(((fmasks[b] >> g) & 1) << b for b in range(nb)) for g in range(n)]
    OB = sum((obs[b] & 1) << b for b in range(nb))
    ge = K._count_ge

    def coin(q, j, r):
        if policy == KING_SPLIT:
            return _M64 if r & 1 else 0
        return coins.words(w, q, 16 * j + (r >> 1))[r & 1]

    def shown(q, j, r, truth, flip=False):
        """Plane of what j shows r: the truth where j is loyal (or j = r), else the
        coin (its complement for the retreat half of a proposal)."""
        if j == r or not F[j]:
            return truth
        c = coin(q, j, r)
        if flip:
            c = ~c & _M64
        return (truth & ~F[j] & _M64) | (F[j] & c)

    pref = [OB] + [shown(0, 0, r, OB) for r in range(1, n)]
    hist = [list(pref)]
    for p in range(1, P + 1):
        k = p - 1
        A, R = [], []  # who proposes attack / retreat
        for i in range(n):
            c1 = _tally(shown(3 * p - 2, j, i, pref[j]) for j in range(n))
            r0 = ~ge(c1, m + 1) & _M64  # c0 >= n - m  <=>  c1 <= m
            R.append(r0)
            A.append(ge(c1, n - m) & ~r0 & _M64)  # retreat wins when both hold
        x, sure = [], []
        for i in range(n):
            d1 = _tally(shown(3 * p - 1, j, i, A[j]) for j in range(n))
            d0 = _tally(shown(3 * p - 1, j, i, R[j], flip=True) for j in range(n))
            x0, x1 = ge(d0, m + 1), ge(d1, m + 1)
            xi = ~x0 & (x1 | pref[i]) & _M64
            x.append(xi)
            sure.append((xi & ge(d1, n - m)) | (~xi & ge(d0, n - m) & _M64))
        pref = [(sure[i] & x[i]) | (~sure[i] & shown(3 * p, k, i, x[k]) & _M64) for i in range(n)]
        hist.append(list(pref))
    return hist


# ---------------------------------------------------------------------------
# per-trial results and the run
# ---------------------------------------------------------------------------
def trial_outcome(n, m, fmask, order_code, dec):
    """king_model's outcome byte with this protocol's in-bound rule: |F| <= m and n > 3m."""
    out = K.trial_outcome(n, m, fmask, order_code, dec) & ~32
    return out | int(bin(fmask).count("1") <= m and n > 3 * m) << 5


def run(n, m, policy=KING_COIN, seed=0, faulty_mode=O.FAULTY_GIVEN, f=0,
        order_mode=O.ORDER_GIVEN, order_value=O.ATTACK, first_trial=0, batch=1, faulty=None,
        order=None, form="message"):
    """(decisions, outcomes, settled, counters dict) of trials [first_trial, + batch)."""
    assert first_trial % 64 == 0 and policy in (KING_COIN, KING_SPLIT)
    coins = Coins(seed)
    ins = [K.inputs(n, seed, faulty_mode, f, order_mode, order_value, first_trial + i, i, faulty,
                    order) for i in range(batch)]
    if form == "message":
        hists = [history_message(n, m, policy, coins, first_trial + i, fm, int(oc == O.ATTACK))
                 for i, (fm, oc) in enumerate(ins)]
    else:
        hists = []
        for i0 in range(0, batch, 64):
            part = ins[i0:i0 + 64]
            hw = history_plane_word(n, m, policy, coins, (first_trial + i0) >> 6,
                                    [p[0] for p in part], [int(p[1] == O.ATTACK) for p in part])
            hists += [[[(pl >> b) & 1 for pl in ph] for ph in hw] for b in range(len(part))]
    decisions, outcomes, settled = [], [], []
    cnt = dict.fromkeys(O.COUNTERS, 0)
    for (fmask, oc), hist in zip(ins, hists):
        dec = hist[-1][1:]
        dword = 0
        for r, d in enumerate(dec):
            dword |= d << (2 * r)
        out = trial_outcome(n, m, fmask, oc, dec)
        decisions.append(dword)
        outcomes.append(out)
        settled.append(K.settled_of(n, fmask, hist))
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
    return decisions, outcomes, settled, cnt


violations = K.violations
unsettled = K.unsettled
