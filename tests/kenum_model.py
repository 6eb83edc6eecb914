"""Reference model of Phase King and KING3 against every traitor strategy of one case
(docs/SEMANTICS.md §11).

TEST INFRASTRUCTURE ONLY (not a test file).  Two implementations written apart from
each other and from the HIP kernel:

  message form -- one strategy at a time: S is decoded into one explicit bit (or trit,
                  None = no proposal) per free message, every message of every round is
                  looked up by (q, sender, recipient), every tally is an explicit integer
                  and the updates are §9's (maj, mult, strong) rule and §10's rules as
                  written.
  plane form   -- a whole space at once: a plane is a Python integer of 2^B bits, bit S
                  = the value under strategy S; ripple counters over all n senders'
                  planes and the threshold forms of the updates.  Good up to B of about 22.

Both walk all n senders of a round one by one; neither shares the loyal senders' tally
among recipients or ranks the traitors, which is how k_kenum finds a free bit.  The
slot order is built here from §11's sentence, not taken from the library.  `phases`,
`trial_outcome` and the quorum are king_model's / king3_model's.
"""
from __future__ import annotations

import functools

import ba_oracle as O
import king3_model as K3
import king_model as K

KING, KING3 = 0, 1
MAX_BITS = 48


def phases(proto, n, m):
    return K.phases(n, m) if proto == KING else K3.phases(n, m)


def trial_outcome(proto, n, m, fmask, order_code, dec):
    return (K if proto == KING else K3).trial_outcome(n, m, fmask, order_code, dec)


def rounds(proto, n, m):
    """[(q, kind, senders)] of the protocol's rounds in q order; kind is "send", "vote"
    (exchange / value), "propose" or "king"."""
    out = [(0, "send", [0])]
    for p in range(1, phases(proto, n, m) + 1):
        if proto == KING:
            out += [(2 * p - 1, "vote", list(range(n))), (2 * p, "king", [p - 1])]
        else:
            out += [(3 * p - 2, "vote", list(range(n))), (3 * p - 1, "propose", list(range(n))),
                    (3 * p, "king", [p - 1])]
    return out


@functools.lru_cache(maxsize=64)
def _slots(proto, n, m, fmask):
    out = []
    for q, kind, senders in rounds(proto, n, m):
        for j in senders:
            if not (fmask >> j) & 1:
                continue
            for i in range(n):
                if (fmask >> i) & 1:
                    continue  # j = i, or a dead message
                out += [(q, j, i, 0), (q, j, i, 1)] if kind == "propose" else [(q, j, i, 0)]
    return tuple(out)


def slots(proto, n, m, fmask):
    """[(q, sender, recipient, part)] of free bits 0..B-1: q ascending, sender ascending,
    recipient ascending, lo (part 0) before hi (part 1)."""
    return list(_slots(proto, n, m, fmask & ((1 << n) - 1)))


def bits_formula(proto, n, m, fmask):
    """§11's closed form of B."""
    fmask &= (1 << n) - 1
    P = phases(proto, n, m)
    nf = bin(fmask).count("1")
    ell = n - nf
    fK = bin(fmask & ((1 << P) - 1)).count("1")
    return (fmask & 1) * ell + (1 if proto == KING else 3) * P * nf * ell + fK * ell


def messages_of(proto, n, m, fmask, S):
    """{(q, sender, recipient): 0 / 1 / None} of strategy S."""
    msgs = {}
    for b, (q, j, i, part) in enumerate(slots(proto, n, m, fmask)):
        v = (S >> b) & 1
        if part == 0:
            msgs[(q, j, i)] = v
        else:  # hi: read only when lo = 1
            msgs[(q, j, i)] = v if msgs[(q, j, i)] else None
    return msgs


def strategy_of(proto, n, m, fmask, bit_of, propose_of):
    """S whose one-bit message (q, j, i) is bit_of(q, j, i) and whose proposal (q, j, i)
    is the pair (lo, hi) = propose_of(q, j, i)."""
    S = 0
    kinds = {qq: kind for qq, kind, _ in rounds(proto, n, m)}
    for b, (q, j, i, part) in enumerate(slots(proto, n, m, fmask)):
        v =propose_of(q, j, i)[part] if kinds[q] == "propose" else bit_of(q, j, i)
        S |= (v & 1) << b
    return S


def split_strategy(proto, n, m, fmask):
    """BA_KING_SPLIT (§9, §10) as a strategy: every free message is recipient & 1, and a
    faulty sender always proposes."""
    return strategy_of(proto, n, m, fmask, lambda q, j, i: i & 1, lambda q, j, i: (1, i & 1))


def coin_strategy(proto, n, m, fmask, seed, t):
    """Trial t of a BA_KING_COIN run with `seed` as a strategy: free message (q, j, i) is
    the coin c(q, 32 j + i) of the protocol's own stream; (lo, hi) = (1, coin)."""
    coins = (K if proto == KING else K3).Coins(seed)

    def bit(q, j, i):
        return coins(t, q, 32 * j + i)

    return strategy_of(proto, n, m, fmask, bit, lambda q, j, i: (1, bit(q, j, i)))


# ---------------------------------------------------------------------------
# message form: one strategy
# ---------------------------------------------------------------------------
def history_message(proto, n, m, fmask, ob, msgs):
    """Preferences of all n generals at the end of phases 0..P under the free messages
    `msgs` ({(q, sender, recipient): 0 / 1 / None})."""
    fmask &= (1 << n) - 1

    def faulty(g):
        return (fmask >> g) & 1

    def shown(q, j, i, truth, dead=0):
        if j == i or not faulty(j):
            return truth
        if faulty(i):
            return dead
        return msgs[(q, j, i)]

    pref = [ob] + [shown(0, 0, i, ob) for i in range(1, n)]
    hist = [list(pref)]
    for p in range(1, phases(proto, n, m) + 1):
        k = p - 1
        if proto == KING:
            maj, strong = [], []
            for i in range(n):
                c1 = sum(shown(2 * p - 1, j, i, pref[j]) for j in range(n))
                mj = 1 if 2 * c1 > n else 0
                maj.append(mj)
                strong.append(2 * (c1 if mj else n - c1) > n + 2 * m)
            pref = [maj[i] if strong[i] else shown(2 * p, k, i, maj[k]) for i in range(n)]
        else:
            prop = []
            for i in range(n):
                c1 = sum(shown(3 * p - 2, j, i, pref[j]) for j in range(n))
                prop.append(0 if n - c1 >= n - m else (1 if c1 >= n - m else None))
            x, sure = [], []
            for i in range(n):
                d = [0, 0]
                for j in range(n):
                    trit = shown(3 * p - 1, j, i, prop[j], dead=None)
                    if trit is not None:
                        d[trit] += 1
                xi = 0 if d[0] > m else (1 if d[1] > m else pref[i])
                x.append(xi)
                sure.append(d[xi] >= n - m)
            pref = [x[i] if sure[i] else shown(3 * p, k, i, x[k]) for i in range(n)]
        hist.append(list(pref))
    return hist


def violates(out: int) -> bool:
    """IC1 fails, or IC2 is applicable and fails."""
    return not ((out >> 2) & 1 and (not (out >> 3) & 1 or (out >> 4) & 1))


def run_message(proto, n, m, fmask, order, first, count):
    """(decisions, outcomes, counters dict, witness or None) of strategies
    [first, first + count), one at a time."""
    fmask &= (1 << n) - 1
    decisions, outcomes, wit = [], [], None
    cnt = dict.fromkeys(O.COUNTERS, 0)
    for S in range(first, first + count):
        hist = history_message(proto, n, m, fmask, int(order == O.ATTACK),
                               messages_of(proto, n, m, fmask, S))
        dec = hist[-1][1:]
        out = trial_outcome(proto, n, m, fmask, order, dec)
        decisions.append(sum(d << (2 * r) for r, d in enumerate(dec)))
        outcomes.append(out)
        agree, appl, valid, inb = (out >> 2) & 1, (out >> 3) & 1, (out >> 4) & 1, (out >> 5) & 1
        cnt["trials"] += 1
        cnt["agreement"] += agree
        cnt["validity_applicable"] += appl
        cnt["validity"] += valid
        cnt[["quorum_retreat", "quorum_attack", "quorum_undetermined"][out & 3]] += 1
        cnt["attack_decisions"] += sum(dec)
        cnt["in_bound"] += inb
        cnt["bound_violations"] += int(inb and violates(out))
        cnt["faulty_total"] += bin(fmask).count("1")
        if wit is None and violates(out):
            wit = S
    return decisions, outcomes, cnt, wit


# ---------------------------------------------------------------------------
# plane form: the whole space, one Python integer per plane
# ---------------------------------------------------------------------------
class Space:
    """The 2^B strategies of one case as bit positions of big integers."""

    def __init__(self, proto, n, m, fmask):
        self.proto, self.n, self.m = proto, n, m
        self.fmask = fmask & ((1 << n) - 1)
        self.slots = slots(proto, n, m, self.fmask)
        self.B = len(self.slots)
        assert self.B <= 24, "the plane form holds 2^B-bit integers"
        self.size = 1 << self.B
        self.ones = (1 << self.size) - 1
        self.index = {s: b for b, s in enumerate(self.slots)}
        self.planes = {}

    def plane(self, b):
        """Bit S = bit b of S: 2^b zeros, then 2^b ones, repeated (by doubling)."""
        x = self.planes.get(b)
        if x is None:
            run = 1 << b
            x, width = ((1 << run) - 1) << run, 2 * run
            while width < self.size:
                x |= x << width
                width *= 2
            self.planes[b] = x
        return x

    def faulty(self, g):
        return (self.fmask >> g) & 1

    def shown(self, q, j, i, truth):
        """Plane of the one-bit message j shows i in round q."""
        if j == i or not self.faulty(j):
            return truth
        if self.faulty(i):
            return 0
        return self.plane(self.index[(q, j, i, 0)])

    def proposal(self, q, j, i, A, R):
        """Planes (attack, retreat) of the proposal j shows i; A, R: j's own."""
        if j == i or not self.faulty(j):
            return A, R
        if self.faulty(i):
            return 0, 0
        lo, hi = self.plane(self.index[(q, j, i, 0)]), self.plane(self.index[(q, j, i, 1)])
        return lo & hi, lo & ~hi & self.ones

    def tally(self, planes_in):
        cnt = [0] * 6
        for x in planes_in:
            for b in range(6):
                cnt[b], x = cnt[b] ^ x, cnt[b] & x
        return cnt

    def ge(self, cnt, T):
        if T <= 0:
            return self.ones
        if T >= 1 << len(cnt):
            return 0
        gt, eq = 0, self.ones
        for b in range(len(cnt) - 1, -1, -1):
            if (T >> b) & 1:
                eq &= cnt[b]
            else:
                gt |= eq & cnt[b]
                eq &= ~cnt[b] & self.ones
        return gt | eq

    def final_planes(self, ob):
        """The n preference planes after the last phase."""
        n, m, ones = self.n, self.m, self.ones
        OB = ones if ob else 0
        pref = [OB] + [self.shown(0, 0, i, OB) for i in range(1, n)]
        for p in range(1, phases(self.proto, n, m) + 1):
            k = p - 1
            if self.proto == KING:
                S = (n + 2 * m) // 2 + 1
                c1 = [self.tally(self.shown(2 * p - 1, j, i, pref[j]) for j in range(n)) for i in range(n)]
                majk = self.ge(c1[k], n // 2 + 1)
                pref = [self.ge(c1[i], S) |
                        (self.ge(c1[i], n - S + 1) & self.shown(2 * p, k, i, majk))  # not (c1 <= n - S)
                        for i in range(n)]
            else:
                A, R = [], []
                for i in range(n):
                    c1 = self.tally(self.shown(3 * p - 2, j, i, pref[j]) for j in range(n))
                    r0 = ~self.ge(c1, m + 1) & ones
                    R.append(r0)
                    A.append(self.ge(c1, n - m) & ~r0 & ones)
                x, sure = [], []
                for i in range(n):
                    shown = [self.proposal(3 * p - 1, j, i, A[j], R[j]) for j in range(n)]
                    d1 = self.tally(a for a, _ in shown)
                    d0 = self.tally(r for _, r in shown)
                    xi = ~self.ge(d0, m + 1) & (self.ge(d1, m + 1) | pref[i]) & ones
                    x.append(xi)
                    sure.append((xi & self.ge(d1, n - m)) | (~xi & self.ge(d0, n - m) & ones))
                pref = [(sure[i] & x[i]) | (~sure[i] & self.shown(3 * p, k, i, x[k]) & ones)
                        for i in range(n)]
        return pref

    def run(self, order):
        """(final planes, counters dict, witness or None) over the whole space."""
        n, fmask, ones = self.n, self.fmask, self.ones
        pref = self.final_planes(int(order == O.ATTACK))
        loyal = [pref[r] for r in range(1, n) if not self.faulty(r)]
        allA = allR = ones
        for pl in loyal:
            allA &= pl
            allR &= ~pl & ones
        agree = allA | allR
        appl = not fmask & 1
        valid = (allA if order == O.ATTACK else allR) if appl else 0
        viol = ones & ~(agree & (valid if appl else ones))
        pop = lambda x: bin(x).count("1")  # noqa: E731
        nf = pop(fmask)
        inb = trial_outcome(self.proto, n, self.m, fmask, order, [0] * (n - 1)) >> 5 & 1
        cnt = dict.fromkeys(O.COUNTERS, 0)
        cnt["trials"] = self.size
        cnt["agreement"] = pop(agree)
        cnt["validity_applicable"] = self.size if appl else 0
        cnt["validity"] = pop(valid)
        cnt["attack_decisions"] = sum(pop(pref[r]) for r in range(1, n))
        cnt["in_bound"] = self.size if inb else 0
        cnt["bound_violations"] = pop(viol) if inb else 0
        cnt["faulty_total"] = nf * self.size
        # the quorum depends on the number of attack decisions alone: the oracle's
        # code for each count, times the strategies with that count
        na = self.tally(pref[1:])
        for a in range(n):
            has = self.ge(na, a) & ~self.ge(na, a + 1) & ones
            q = O.quorum(n, order, [1] * a + [0] * (n - 1 - a))[0]
            cnt[["quorum_retreat", "quorum_attack", "quorum_undetermined"][q]] += pop(has)
        wit = (viol & -viol).bit_length() - 1 if viol else None
        return pref, cnt, wit

    def trial(self, pref, order, S):
        """(decisions word, outcome byte) of strategy S out of the final planes."""
        dec = [(pref[r] >> S) & 1 for r in range(1, self.n)]
        return (sum(d << (2 * r) for r, d in enumerate(dec)),
                trial_outcome(self.proto, self.n, self.m, self.fmask, order, dec))
