"""Reference model of Phase King agreement (Berman, Garay, Perry; docs/SEMANTICS.md §9).

TEST INFRASTRUCTURE ONLY (not a test file).  Two implementations written apart
from each other and from the HIP kernel:

  message form -- one trial at a time: every message of every round is an explicit
                  bit, every tally an explicit integer, and the update is §9's
                  (maj, mult, strong) rule.  `run` uses this one.
  plane form   -- 64 trials per word: one preference plane per general, ripple
                  counters over the senders' planes and the two-threshold form of
                  the update (c1 >= S -> 1, c1 <= n - S -> 0, else the king).

Coins, synthetic inputs and the quorum come from oracle/ba_oracle.py (`lie`,
`gen`, `quorum`); the Philox blocks behind `lie` are cached per (word, q, pair)
so n = 32 stays within seconds.
"""
from __future__ import annotations

import ba_oracle as O

KING_TAG = 128  # ctr word 1 of Phase King draws: c(q, x) = coin(128 + q, x)
KING_COIN, KING_SPLIT = 0, 1
UNSETTLED = 255
_M64 = (1 << 64) - 1


class Coins:
    """c(q, x) of §9 for one seed: ba_oracle.lie(seed, t, 128 + q, x), with the
    Philox block of (trial word, q, pair) computed once."""

    def __init__(self, seed: int):
        self.seed = seed
        self.key = (seed & O.M32, seed >> 32)
        self.blocks = {}

    def words(self, w: int, q: int, pair: int):
        """The 64-trial coin words of x = 2 pair and x = 2 pair + 1."""
        key = (w, q, pair)
        b = self.blocks.get(key)
        if b is None:
            o = O.philox4x32_10((pair, KING_TAG + q, w & O.M32, w >> 32), self.key)
            b = self.blocks[key] = (o[1] << 32 | o[0], o[3] << 32 | o[2])
        return b

    def __call__(self, t: int, q: int, x: int) -> int:
        return (self.words(t >> 6, q, x >> 1)[x & 1] >> (t & 63)) & 1


def phases(n: int, m: int) -> int:
    """P = min(m, n - 1) + 1 (0 for n outside 1..32 or m > 8)."""
    if n < 1 or n > 32 or m < 0 or m > 8:
        return 0
    return min(m, n - 1) + 1


def coin_calls(n: int, m: int) -> int:
    """Philox calls per 64-trial word: ceil(n/2) (1 + P (n + 1))."""
    P = phases(n, m)
    if P == 0:
        return 0
    return ((n + 1) // 2) * (1 + P * (n + 1))


# ---------------------------------------------------------------------------
# message form
# ---------------------------------------------------------------------------
def history_message(n, m, policy, coins: Coins, t, fmask, ob):
    """Preferences of all n generals at the end of phases 0..P: list of P+1 lists."""
    P = phases(n, m)

    def faulty(g):
        return (fmask >> g) & 1

    def msg(q, j, r, truth):
        if j == r or not faulty(j):
            return truth
        if policy == KING_SPLIT:
            return r & 1
        return coins(t, q, 32 * j + r)

    pref = [ob] + [msg(0, 0, r, ob) for r in range(1, n)]
    hist = [list(pref)]
    for p in range(1, P + 1):
        k = p - 1
        maj, strong = [], []
        for i in range(n):
            received = [msg(2 * p - 1, j, i, pref[j]) for j in range(n)]
            c1 = sum(received)
            c0 = n - c1
            mj = 1 if 2 * c1 > n else 0
            mult = c1 if mj else c0
            maj.append(mj)
            strong.append(2 * mult > n + 2 * m)
        new = []
        for i in range(n):
            km = maj[k] if i == k else msg(2 * p, k, i, maj[k])
            new.append(maj[i] if strong[i] else km)
        pref = new
        hist.append(list(pref))
    return hist


# ---------------------------------------------------------------------------
# plane form: 64 trials per word
# ---------------------------------------------------------------------------
def _count_ge(planes, T):
    """Word of the trials whose bit-sliced count (planes[i] = bit i) is >= T."""
    if T <= 0:
        return _M64
    if T >= 1 << len(planes):
        return 0
    gt, eq = 0, _M64
    for i in range(len(planes) - 1, -1, -1):
        if (T >> i) & 1:
            eq &= planes[i]
        else:
            gt |= eq & planes[i]
            eq &= ~planes[i] & _M64
    return gt | eq


def history_plane_word(n, m, policy, coins: Coins, w, fmasks, obs):
    """Preference planes at the end of phases 0..P for the trials 64 w + b,
    b < len(fmasks): list of P+1 lists of n words."""
    P = phases(n, m)
    nb = len(fmasks)
    F = [sum(((fmasks[b] >> g) & 1) << b for b in range(nb)) for g in range(n)]
    OB = sum((obs[b] & 1) << b for b in range(nb))
    S = (n + 2 * m) // 2 + 1

    def shown(q, j, r, truth):  # plane of what j shows r
        if j == r or not F[j]:
            return truth
        if policy == KING_SPLIT:
            c = _M64 if r & 1 else 0
        else:
            c = coins.words(w, q, 16 * j + (r >> 1))[r & 1]
        return (truth & ~F[j] & _M64) | (F[j] & c)

    pref = [OB] + [shown(0, 0, r, OB) for r in range(1, n)]
    hist = [list(pref)]
    for p in range(1, P + 1):
        k = p - 1
        hi, lo, maj = [], [], []
        for i in range(n):
            cnt = [0] * 6  # ripple counter, up to 32
            for j in range(n):
                x = shown(2 * p - 1, j, i, pref[j])
                for b in range(6):
                    cnt[b], x = cnt[b] ^ x, cnt[b] & x
            hi.append(_count_ge(cnt, S))
            lo.append(~_count_ge(cnt, n - S + 1) & _M64)  # c1 <= n - S
            maj.append(_count_ge(cnt, n // 2 + 1))
        new = []
        for i in range(n):
            km = shown(2 * p, k, i, maj[k])
            new.append(hi[i] | (~lo[i] & km & _M64))
        pref = new
        hist.append(list(pref))
    return hist


# ---------------------------------------------------------------------------
# per-trial results and the run
# ---------------------------------------------------------------------------
def settled_of(n, fmask, hist) -> int:
    """Smallest p such that the loyal generals hold one preference at the end of
    phase p and of every later phase; 255 if they differ at the end."""
    loyal = [g for g in range(n) if not (fmask >> g) & 1]
    s = UNSETTLED
    for p, pref in enumerate(hist):
        if len({pref[g] for g in loyal}) <= 1:
            if s == UNSETTLED:
                s = p
        else:
            s = UNSETTLED
    return s


def trial_outcome(n, m, fmask, order_code, dec):
    """Outcome byte: §2.4 with the Phase King in-bound rule |F| <= m and n > 4m."""
    q = O.quorum(n, order_code, dec)[0]
    loyal = [dec[r - 1] for r in range(1, n) if not (fmask >> r) & 1]
    agree = int(len(set(loyal)) <= 1)
    appl = int(not fmask & 1)
    want = O.ATTACK if order_code == O.ATTACK else O.RETREAT
    valid = int(appl and all(d == want for d in loyal))
    inb = int(bin(fmask).count("1") <= m and n > 4 * m)
    return q | agree << 2 | appl << 3 | valid << 4 | inb << 5


def inputs(n, seed, faulty_mode, f, order_mode, order_value, t, i, faulty, order):
    gm, go = O.gen(n, seed, faulty_mode, f, order_mode, order_value, t)
    fmask = (faulty[i] if faulty_mode == O.FAULTY_GIVEN else gm) & ((1 << n) - 1)
    oc = order[i] if order_mode == O.ORDER_GIVEN else go
    return int(fmask), int(oc)


def run(n, m, policy=KING_COIN, seed=0, faulty_mode=O.FAULTY_GIVEN, f=0,
        order_mode=O.ORDER_GIVEN, order_value=O.ATTACK, first_trial=0, batch=1, faulty=None,
        order=None, form="message"):
    """(decisions, outcomes, settled, counters dict) of trials [first_trial, + batch)."""
    assert first_trial % 64 == 0 and policy in (KING_COIN, KING_SPLIT)
    coins = Coins(seed)
    ins = [inputs(n, seed, faulty_mode, f, order_mode, order_value, first_trial + i, i, faulty,
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
        settled.append(settled_of(n, fmask, hist))
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


def violations(outcomes) -> int:
    """Trials in which IC1 or IC2 fails."""
    return sum(1 for o in outcomes if not ((o >> 2) & 1 and (not (o >> 3) & 1 or (o >> 4) & 1)))


def unsettled(settled) -> int:
    return sum(1 for s in settled if s == UNSETTLED)
