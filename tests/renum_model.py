"""Reference model of RAND against every traitor strategy and every coin outcome of one
case (docs/SEMANTICS.md §14).

TEST INFRASTRUCTURE ONLY (not a test file).  Two implementations written apart from
each other and from the HIP kernel:

  message form -- one strategy at a time: S is decoded into one explicit value per free
                  message (None = no proposal) and one bit per toss, and the phases are
                  rand_model.phase_step's, which is handed the messages and the tosses
                  as callables; `decided` is rand_model.decided_of, the outcome byte
                  rand_model.trial_outcome.
  plane form   -- a whole space at once: a plane is a Python integer of 2^B bits, bit S
                  = the value under strategy S; ripple counters over all n senders'
                  planes and §13's threshold forms.  Good up to B of about 24.

Both walk all n senders of a round one by one; neither shares the loyal senders' tally
among recipients or ranks the traitors, which is how k_renum finds a free bit.  The
slot order is built here from §14's sentence, not taken from the library.
"""
from __future__ import annotations

import functools

import ba_oracle as O
import rand_model as RM

LOCAL, COMMON = RM.RAND_LOCAL, RM.RAND_COMMON
MAX_BITS = 48
MAX_PHASES = 16
TOSS = 2           # a slot's part: a toss bit
COMMON_COIN = 0xFFFFFFFF  # sender and recipient of the common coin's slot
UNDECIDED, UNSAFE = RM.UNDECIDED, RM.UNSAFE


def _mask(n, fmask):
    return fmask & ((1 << n) - 1)


@functools.lru_cache(maxsize=64)
def _slots(coin, n, m, R, fmask):
    loyal = [g for g in range(n) if not (fmask >> g) & 1]
    bad = [g for g in range(n) if (fmask >> g) & 1]
    out = [(0, 0, i, 0) for i in loyal] if fmask & 1 else []
    for p in range(1, R + 1):
        out += [(3 * p - 2, j, i, 0) for j in bad for i in loyal]
        out += [(3 * p - 1, j, i, part) for j in bad for i in loyal for part in (0, 1)]
        out += [(3 * p, COMMON_COIN, COMMON_COIN, TOSS)] if coin == COMMON else [(3 * p, i, i, TOSS) for i in loyal]
    return tuple(out)


def slots(coin, n, m, R, fmask):
    """[(q, sender, recipient, part)] of free bits 0..B-1: round 0, then per phase the
    reports, the proposals (lo = part 0 before hi = part 1) and the tosses (part 2)."""
    return list(_slots(coin, n, m, R, _mask(n, fmask)))


def bits_formula(coin, n, m, R, fmask):
    """§14's closed form of B."""
    fmask = _mask(n, fmask)
    nf = bin(fmask).count("1")
    ell = n - nf
    return (fmask & 1) * ell + R * (3 * nf * ell + (ell if coin == LOCAL else 1))


def messages_of(coin, n, m, R, fmask, S):
    """{"messages": {(q, sender, recipient): 0 / 1 / None}, "coins": {(p, general or None): bit}}."""
    msgs, coins = {}, {}
    for b, (q, j, i, part) in enumerate(slots(coin, n, m, R, fmask)):
        v = (S >> b) & 1
        if part == TOSS:
            coins[(q // 3, None if j == COMMON_COIN else j)] = v
        elif part == 0:
            msgs[(q, j, i)] = v
        else:  # hi: read only when lo = 1
            msgs[(q, j, i)] = v if msgs[(q, j, i)] else None
    return {"messages": msgs, "coins": coins}


def strategy_of(coin, n, m, R, fmask, bit_of, propose_of, toss_of):
    """S whose one-bit message (q, j, i) is bit_of(q, j, i), whose proposal is the pair
    (lo, hi) = propose_of(q, j, i) and whose toss of phase p is toss_of(p, general or None)."""
    S = 0
    for b, (q, j, i, part) in enumerate(slots(coin, n, m, R, fmask)):
        if part == TOSS:
            v = toss_of(q // 3, None if j == COMMON_COIN else j)
        elif q and q % 3 == 2:
            v = propose_of(q, j, i)[part]
        else:
            v = bit_of(q, j, i)
        S |= (v & 1) << b
    return S


def _rand_trial(coin, n, m, R, fmask, seed, t, split):
    coins = RM.Coins(seed)

    def bit(q, j, i):
        return i & 1 if split else coins(t, q, 32 * j + i)

    return strategy_of(coin, n, m, R, fmask, bit, lambda q, j, i: (1, bit(q, j, i)),
                       lambda p, g: coins(t, 3 * p, RM.toss_slot(coin, 0 if g is None else g)))


def coin_strategy(coin, n, m, R, fmask, seed, t):
    """Trial t of a BA_KING_COIN k_rand run with `seed` as a strategy (§14)."""
    return _rand_trial(coin, n, m, R, fmask, seed, t, False)


def split_strategy(coin, n, m, R, fmask, seed, t):
    """Trial t of a BA_KING_SPLIT k_rand run: the messages are recipient & 1, the tosses
    are still the seed's."""
    return _rand_trial(coin, n, m, R, fmask, seed, t, True)


# ---------------------------------------------------------------------------
# message form: one strategy
# ---------------------------------------------------------------------------
def history_message(coin, n, m, R, fmask, ob, play):
    """States (x, D, V) of all n generals at the end of phases 0..R under `play`
    (messages_of's dict)."""
    fmask = _mask(n, fmask)
    msgs, coins = play["messages"], play["coins"]

    def faulty(g):
        return (fmask >> g) & 1

    x = RM.round0(n, fmask, ob, lambda r: 0 if faulty(r) else msgs[(0, 0, r)])
    D, V = [0] * n, [0] * n
    hist = [(list(x), list(D), list(V))]
    for p in range(1, R + 1):
        def report(j, i, q=3 * p - 2):
            return 0 if faulty(i) else msgs[(q, j, i)]  # dead: retreat

        def propose(j, i, q=3 * p - 1):
            return None if faulty(i) else msgs[(q, j, i)]  # dead: no proposal

        def toss(i, p=p):
            if coin == COMMON:
                return coins[(p, None)]
            return 0 if faulty(i) else coins[(p, i)]  # a faulty general's own toss is dead

        x, D, V = RM.phase_step(n, m, fmask, x, D, V, report, propose, toss)
        hist.append((list(x), list(D), list(V)))
    return hist


def violates(out: int) -> bool:
    """IC1 fails, or IC2 is applicable and fails."""
    return not ((out >> 2) & 1 and (not (out >> 3) & 1 or (out >> 4) & 1))


def new_stats():
    return {"unsafe": 0, "undecided": 0, "unsafe_witness": None, "undecided_witness": None,
            "decided_in": [0] * (MAX_PHASES + 1)}


def run_message(coin, n, m, R, fmask, order, first, count):
    """(decisions, outcomes, decided, counters dict, witness or None, stats dict) of
    strategies [first, first + count), one at a time."""
    fmask = _mask(n, fmask)
    ob = int(order == O.ATTACK)
    decisions, outcomes, decided, wit = [], [], [], None
    cnt = dict.fromkeys(O.COUNTERS, 0)
    st = new_stats()
    for S in range(first, first + count):
        hist = history_message(coin, n, m, R, fmask, ob, messages_of(coin, n, m, R, fmask, S))
        dec = hist[-1][0][1:]
        out = RM.trial_outcome(n, m, fmask, order, dec)
        dcd = RM.decided_of(n, fmask, ob, hist)
        decisions.append(sum(d << (2 * r) for r, d in enumerate(dec)))
        outcomes.append(out)
        decided.append(dcd)
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
        if dcd == UNSAFE:
            st["unsafe"] += 1
            if st["unsafe_witness"] is None:
                st["unsafe_witness"] = S
        elif dcd == UNDECIDED:
            st["undecided"] += 1
            if st["undecided_witness"] is None:
                st["undecided_witness"] = S
        else:
            st["decided_in"][dcd] += 1
    return decisions, outcomes, decided, cnt, wit, st


# ---------------------------------------------------------------------------
# plane form: the whole space, one Python integer per plane
# ---------------------------------------------------------------------------
class Space:
    """The 2^B strategies of one case as bit positions of big integers."""

    def __init__(self, coin, n, m, R, fmask):
        self.coin, self.n, self.m, self.R = coin, n, m, R
        self.fmask = _mask(n, fmask)
        self.slots = slots(coin, n, m, R, self.fmask)
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

    def toss(self, p, i):
        if self.coin == COMMON:
            return self.plane(self.index[(3 * p, COMMON_COIN, COMMON_COIN, TOSS)])
        return 0 if self.faulty(i) else self.plane(self.index[(3 * p, i, i, TOSS)])

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

    def walk(self, ob):
        """(final x planes, unsafe plane, [plane of "first all-loyal-decided at phase p"]
        indexed by p) after R phases."""
        n, m, ones = self.n, self.m, self.ones
        OB = ones if ob else 0
        T = (n + m) // 2 + 1
        loyal = [g for g in range(n) if not self.faulty(g)]
        x = [OB] + [self.shown(0, 0, i, OB) for i in range(1, n)]
        D, V = [0] * n, [0] * n
        bad, seen, first = 0, 0, [0] * (self.R + 1)
        for p in range(1, self.R + 1):
            A, Rt = [], []
            for i in range(n):
                c1 = self.tally(self.shown(3 * p - 2, j, i, x[j]) for j in range(n))
                A.append(self.ge(c1, T))
                Rt.append(~self.ge(c1, n - T + 1) & ones if T <= n else 0)  # c0 >= T  <=>  c1 <= n - T
            nx = []
            for i in range(n):
                shown = [self.proposal(3 * p - 1, j, i, A[j], Rt[j]) for j in range(n)]
                d1 = self.tally(a for a, _ in shown)
                d0 = self.tally(r for _, r in shown)
                v0 = self.ge(d0, m + 1)
                v1 = self.ge(d1, m + 1) & ~v0 & ones
                strong = (v0 & self.ge(d0, T)) | (v1 & self.ge(d1, T))
                new = strong & ~D[i] & ones
                V[i] = (V[i] & ~new & ones) | (new & v1)
                D[i] |= new
                nx.append(v1 | (~(v0 | v1) & ones & self.toss(p, i)))
            x = nx
            # §13's three unsafe conditions, over the loyal generals
            a1 = a0 = moved = 0
            allD = ones
            for g in loyal:
                a1 |= D[g] & V[g]
                a0 |= D[g] & ~V[g] & ones
                moved |= D[g] & (x[g] ^ V[g])
                allD &= D[g]
            bad |= (a1 & a0) | moved
            if not self.fmask & 1:
                bad |= (a1 & ~OB & ones) | (a0 & OB)
            first[p] = allD & ~seen & ones
            seen |= allD
        return x, bad, first

    def run(self, order):
        """(x planes, decided planes (bad, first), counters dict, witness or None, stats
        dict) over the whole space."""
        n, fmask, ones = self.n, self.fmask, self.ones
        x, bad, first = self.walk(int(order == O.ATTACK))
        loyal = [x[r] for r in range(1, n) if not self.faulty(r)]
        allA = allR = ones
        for pl in loyal:
            allA &= pl
            allR &= ~pl & ones
        agree = allA | allR
        appl = not fmask & 1
        valid = (allA if order == O.ATTACK else allR) if appl else 0
        viol = ones & ~(agree & (valid if appl else ones))
        pop = lambda v: bin(v).count("1")  # noqa: E731
        low = lambda v: (v & -v).bit_length() - 1 if v else None  # noqa: E731
        nf = pop(fmask)
        inb = RM.trial_outcome(n, self.m, fmask, order, [0] * (n - 1)) >> 5 & 1
        cnt = dict.fromkeys(O.COUNTERS, 0)
        cnt["trials"] = self.size
        cnt["agreement"] = pop(agree)
        cnt["validity_applicable"] = self.size if appl else 0
        cnt["validity"] = pop(valid)
        cnt["attack_decisions"] = sum(pop(x[r]) for r in range(1, n))
        cnt["in_bound"] = self.size if inb else 0
        cnt["bound_violations"] = pop(viol) if inb else 0
        cnt["faulty_total"] = nf * self.size
        na = self.tally(x[1:])
        for a in range(n):
            has = self.ge(na, a) & ~self.ge(na, a + 1) & ones
            q = O.quorum(n, order, [1] * a + [0] * (n - 1 - a))[0]
            cnt[["quorum_retreat", "quorum_attack", "quorum_undetermined"][q]] += pop(has)
        st = new_stats()
        seen = 0
        for p in range(1, self.R + 1):
            seen |= first[p]
            st["decided_in"][p] = pop(first[p] & ~bad)
        und = ones & ~bad & ~seen
        st["unsafe"], st["undecided"] = pop(bad), pop(und)
        st["unsafe_witness"], st["undecided_witness"] = low(bad), low(und)
        return x, (bad, first), cnt, low(viol), st

    def trial(self, x, dplanes, order, S):
        """(decisions word, outcome byte, decided byte) of strategy S out of run's planes."""
        bad, first = dplanes
        dec = [(x[r] >> S) & 1 for r in range(1, self.n)]
        dcd = UNDECIDED
        for p in range(1, self.R + 1):
            if (first[p] >> S) & 1:
                dcd = p
        if (bad >> S) & 1:
            dcd = UNSAFE
        return (sum(d << (2 * r) for r, d in enumerate(dec)),
                RM.trial_outcome(self.n, self.m, self.fmask, order, dec), dcd)
