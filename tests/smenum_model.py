"""Reference model of SM(m) against every strategy of a traitor coalition that shares
its signatures (docs/SEMANTICS.md §12).

TEST INFRASTRUCTURE ONLY (not a test file).  Two implementations written apart from
each other and from the HIP kernel:

  chain form -- one strategy at a time, explicit signed messages: a message is a value
                plus the chain of its signers, the commander first.  Loyal generals log
                what they sign; the coalition builds a chain for every message it wants
                to deliver (`find_chain`: its own members first, a loyal signer only
                where the log has that very prefix), and every recipient verifies what it
                is handed.  Nothing here knows which messages are "dead": a send outside
                the coded rounds is simply tried (`extra`).
  plane form -- a whole space at once: a plane is a Python integer of 2^B bits, bit S =
                the value under strategy S; has / fresh planes per lieutenant, every
                recipient ORing over the loyal senders one by one.  Good up to B of
                about 22.

k_smenum keeps one "some loyal lieutenant is fresh" plane per value instead; neither
form here does.  The slot order is built from §12's sentence, not taken from the
library.  `choice`, `trial_outcome`, the coins and the pair index are sm_model's.
"""
from __future__ import annotations

import functools
import itertools

import ba_oracle as O
from sm_model import Coins, choice, pair_index, trial_outcome

MESSAGES, COALITION = 0, 1
ANY = 0xFFFFFFFF  # the sender of a coalition-form relay slot: any traitor
MAX_BITS = 48


def shape(n, m, fmask):
    """(F, c, loyal lieutenants, faulty lieutenants, me, K) of a case."""
    F = fmask & ((1 << n) - 1)
    loyal = [r for r in range(1, n) if not (F >> r) & 1]
    faulty = [r for r in range(1, n) if (F >> r) & 1]
    me = O.effective_depth(n, m)
    return F, F & 1, loyal, faulty, me, min(me, len(faulty))


@functools.lru_cache(maxsize=256)
def _slots(form, n, m, fmask, ob):
    F, c, loyal, faulty, me, K = shape(n, m, fmask)
    values = (0, 1) if c else (ob,)
    out = []
    if c:
        out += [(0, 0, r, v) for r in loyal for v in values]
    for k in range(1, K + 1):
        for j in (faulty if form == MESSAGES else [ANY]):
            out += [(k, j, r, v) for r in loyal for v in values]
    return tuple(out)


def slots(form, n, m, fmask, order):
    """[(k, sender, recipient, v)] of free bits 0..B-1: k ascending, sender ascending,
    recipient ascending, retreat before attack."""
    return list(_slots(form, n, m, fmask & ((1 << n) - 1), int(order == O.ATTACK)))


def bits_formula(form, n, m, fmask):
    """§12's closed form of B."""
    F, c, loyal, faulty, me, K = shape(n, m, fmask)
    ell, fL = len(loyal), len(faulty)
    return c * 2 * ell + K * (fL if form == MESSAGES else 1) * ell * (1 + c)


def messages_of(form, n, m, fmask, order, S):
    """The sorted list of the messages (k, sender, recipient, v) sent under strategy S."""
    return sorted(s for b, s in enumerate(slots(form, n, m, fmask, order)) if (S >> b) & 1)


def strategy_of(form, n, m, fmask, order, messages):
    """S that sends exactly `messages` (each a free bit of the case)."""
    index = {s: b for b, s in enumerate(slots(form, n, m, fmask, order))}
    return sum(1 << index[tuple(msg)] for msg in set(messages))


def project(n, m, fmask, order, S):
    """Message-form S -> the coalition-form S' whose bit (k, r, v) is the OR over the
    senders j of S's bits (k, j, r, v)."""
    sent = {(k, 0 if k == 0 else ANY, r, v) for k, _, r, v in messages_of(MESSAGES, n, m, fmask, order, S)}
    return strategy_of(COALITION, n, m, fmask, order, sent)


def violates(out: int) -> bool:
    """IC1 fails, or IC2 is applicable and fails."""
    return not ((out >> 2) & 1 and (not (out >> 3) & 1 or (out >> 4) & 1))


# ---------------------------------------------------------------------------
# chain form: one strategy, explicit signed messages
# ---------------------------------------------------------------------------
def vsets_chain(n, m, fmask, ob, sends, delivered=None):
    """{lieutenant: V} under the coalition's send attempts `sends`, an iterable of (k,
    sender, recipient, v): sender a faulty general, or ANY for "whoever of the coalition
    can".  An attempt delivers only if a valid chain can be put together; `delivered`
    (a list) collects (k, sender, recipient, v, chain) of the relay-round ones that do."""
    F, c, loyal, faulty, me, K = shape(n, m, fmask)
    lts = range(1, n)
    is_faulty = lambda g: (F >> g) & 1  # noqa: E731
    signed = {g: set() for g in range(n) if not is_faulty(g)}  # loyal g -> {(v, chain ending in g)}
    V = {r: set() for r in lts}

    def verify(k, r, v, chain):
        """What recipient r checks of a round-k message: k + 1 distinct signers, the
        commander first, r itself absent, and a loyal signer only where it really
        signed that prefix.  A faulty recipient is kept honest on what loyal senders
        show it: its own signature on a loyal relay's chain does not hide the value."""
        if len(chain) != k + 1 or chain[0] != 0 or len(set(chain)) != len(chain):
            return False
        if any(not 0 <= g < n for g in chain):
            return False
        if r in chain and not is_faulty(r):
            return False
        return all(is_faulty(g) or (v, chain[:p + 1]) in signed[g] for p, g in enumerate(chain))

    def find_chain(k, j, r, v):
        """A valid chain for a round-k message of value v from traitor j to r, or None:
        the commander, k - 1 further lieutenants, j last; the coalition's own first."""
        others = [g for g in faulty if g not in (j, r)] + [g for g in loyal if g != r]
        for mid in itertools.permutations(others, k - 1):
            chain = (0,) + mid + (j,)
            if verify(k, r, v, chain):
                return chain
        return None

    by_round = {}
    for k, j, r, v in sorted(sends):
        by_round.setdefault(k, []).append((j, r, v))
    inbox = {r: [] for r in lts}
    if not c:
        signed[0].add((ob, (0,)))
        for r in lts:
            inbox[r].append((ob, (0,)))
    else:
        for j, r, v in by_round.get(0, []):
            assert j == 0
            inbox[r].append((v, (0,)))
    for k in range(me + 1):
        relay = []
        for r in lts:
            for v, chain in inbox[r]:
                if verify(k, r, v, chain) and v not in V[r]:
                    V[r].add(v)
                    if not is_faulty(r):
                        relay.append((r, v, chain + (r,)))  # r signs; relays next round
        if k == me:
            break
        inbox = {r: [] for r in lts}
        for j, v, chain in relay:  # a loyal relay goes to every other lieutenant
            signed[j].add((v, chain))
            for r in lts:
                if r != j:
                    inbox[r].append((v, chain))
        for j, r, v in by_round.get(k + 1, []):
            for sender in (faulty if j == ANY else [j]):
                assert is_faulty(sender) and not is_faulty(r)
                chain = find_chain(k + 1, sender, r, v)
                if chain is not None:
                    inbox[r].append((v, chain))
                    if delivered is not None:
                        delivered.append((k + 1, sender, r, v, chain))
                    break
    return V


def decide_chain(n, m, fmask, order, sends):
    """(decision codes by lieutenant rank, outcome byte) of one set of send attempts."""
    V = vsets_chain(n, m, fmask, int(order == O.ATTACK), sends)
    dec = [choice(V[r]) for r in range(1, n)]
    return dec, trial_outcome(n, m, fmask & ((1 << n) - 1), order, dec)


def run_chain(form, n, m, fmask, order, first, count):
    """(decisions, outcomes, counters dict, witness or None) of strategies
    [first, first + count), one at a time."""
    fmask &= (1 << n) - 1
    decisions, outcomes, wit = [], [], None
    cnt = dict.fromkeys(O.COUNTERS, 0)
    for S in range(first, first + count):
        dec, out = decide_chain(n, m, fmask, order, messages_of(form, n, m, fmask, order, S))
        decisions.append(sum(d << (2 * r) for r, d in enumerate(dec)))
        outcomes.append(out)
        agree, appl, valid, inb = (out >> 2) & 1, (out >> 3) & 1, (out >> 4) & 1, (out >> 5) & 1
        cnt["trials"] += 1
        cnt["agreement"] += agree
        cnt["validity_applicable"] += appl
        cnt["validity"] += valid
        cnt[["quorum_retreat", "quorum_attack", "quorum_undetermined"][out & 3]] += 1
        cnt["attack_decisions"] += sum(1 for d in dec if d == O.ATTACK)
        cnt["in_bound"] += inb
        cnt["bound_violations"] += int(inb and violates(out))
        cnt["faulty_total"] += bin(fmask).count("1")
        if wit is None and violates(out):
            wit = S
    return decisions, outcomes, cnt, wit


# ---------------------------------------------------------------------------
# a k_sm coin trial as one strategy
# ---------------------------------------------------------------------------
def coin_sends(n, m, fmask, ob, coins: Coins, t):
    """The messages (k, j, r, v), k <= K, that a faulty general j really sent a loyal
    lieutenant r in trial t of a coin run (§6): a faulty commander on its round-0
    coins, a faulty lieutenant what it accepted a round ago and its coin allows."""
    F, c, loyal, faulty, me, K = shape(n, m, fmask)
    L = n - 1
    has = {r: set() for r in range(1, n)}
    fresh = {r: set() for r in range(1, n)}
    sent = set()
    for r in range(1, n):
        for v in (0, 1):
            if (coins(t, 0, 2 * (r - 1) + v) if c else v == ob):
                fresh[r].add(v)
                if c and r in loyal:
                    sent.add((0, 0, r, v))
        has[r] |= fresh[r]
    for k in range(1, me + 1):
        recv = {r: set() for r in range(1, n)}
        for j in range(1, n):
            for v in fresh[j]:
                for r in range(1, n):
                    if r == j:
                        continue
                    if j in loyal or coins(t, k, 2 * pair_index(j - 1, r - 1, L) + v):
                        recv[r].add(v)
                        if j in faulty and r in loyal and k <= K:
                            sent.add((k, j, r, v))
        for r in range(1, n):
            fresh[r] = recv[r] - has[r]
            has[r] |= fresh[r]
    return sent


def coin_strategy(form, n, m, fmask, order, seed, t, coins=None):
    """Trial t of a k_sm coin run with `seed`, faulty set and order given, as a strategy:
    the free bit of (k, j, r, v) is 1 iff faulty j sent v to loyal r in round k <= K
    (what it sends later is dead).  The coalition form takes the projection.  coins: a
    Coins(seed) to share its cached draws between calls."""
    S = strategy_of(MESSAGES, n, m, fmask, order,
                    coin_sends(n, m, fmask, int(order == O.ATTACK), coins or Coins(seed), t))
    return S if form == MESSAGES else project(n, m, fmask, order, S)


# ---------------------------------------------------------------------------
# plane form: the whole space, one Python integer per plane
# ---------------------------------------------------------------------------
class Space:
    """The 2^B strategies of one case as bit positions of big integers."""

    def __init__(self, form, n, m, fmask, order):
        self.form, self.n, self.m, self.order = form, n, m, order
        self.fmask, self.c, self.loyal, self.faulty, self.me, self.K = shape(n, m, fmask)
        self.slots = slots(form, n, m, self.fmask, order)
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

    def free(self, k, r, v):
        """Plane of "the coalition delivers v to loyal r in round k"."""
        x = 0
        for j in ([0] if k == 0 else self.faulty if self.form == MESSAGES else [ANY]):
            b = self.index.get((k, j, r, v))
            if b is not None:
                x |= self.plane(b)
        return x

    def final_planes(self):
        """has[v][r] of every lieutenant r after round me."""
        n, ones = self.n, self.ones
        ob = int(self.order == O.ATTACK)
        has = [{}, {}]
        fresh = [{}, {}]
        for r in range(1, n):
            for v in (0, 1):
                if not self.c:
                    x = ones if v == ob else 0
                else:
                    x = self.free(0, r, v) if r in self.loyal else 0
                has[v][r] = fresh[v][r] = x
        for k in range(1, self.me + 1):
            new = [{}, {}]
            for r in range(1, n):
                for v in (0, 1):
                    recv = 0
                    for j in self.loyal:
                        if j != r:
                            recv |= fresh[v][j]
                    if r in self.loyal and k <= self.K:
                        recv |= self.free(k, r, v)
                    new[v][r] = recv & ~has[v][r] & ones
            for v in (0, 1):
                for r in range(1, n):
                    fresh[v][r] = new[v][r]
                    has[v][r] |= new[v][r]
        return has

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

    def run(self):
        """(attack-decision planes by lieutenant rank, counters dict, witness or None)
        over the whole space."""
        n, fmask, ones, order = self.n, self.fmask, self.ones, self.order
        has = self.final_planes()
        dec = [has[1][r] & ~has[0][r] & ones for r in range(1, n)]  # choice(V) = attack iff V = {1}
        allA = allR = ones
        for r in self.loyal:
            allA &= dec[r - 1]
            allR &= ~dec[r - 1] & ones
        agree = allA | allR
        appl = not self.c
        valid = (allA if order == O.ATTACK else allR) if appl else 0
        viol = ones & ~(agree & (valid if appl else ones))
        pop = lambda x: bin(x).count("1")  # noqa: E731
        nf = pop(fmask)
        inb = nf <= self.m
        cnt = dict.fromkeys(O.COUNTERS, 0)
        cnt["trials"] = self.size
        cnt["agreement"] = pop(agree)
        cnt["validity_applicable"] = self.size if appl else 0
        cnt["validity"] = pop(valid)
        cnt["attack_decisions"] = sum(pop(d) for d in dec)
        cnt["in_bound"] = self.size if inb else 0
        cnt["bound_violations"] = pop(viol) if inb else 0
        cnt["faulty_total"] = nf * self.size
        # the quorum depends on the number of attack decisions alone: the oracle's
        # code for each count, times the strategies with that count
        na = self.tally(dec)
        for a in range(n):
            hit = self.ge(na, a) & ~self.ge(na, a + 1) & ones
            q = O.quorum(n, order, [1] * a + [0] * (n - 1 - a))[0]
            cnt[["quorum_retreat", "quorum_attack", "quorum_undetermined"][q]] += pop(hit)
        wit = (viol & -viol).bit_length() - 1 if viol else None
        return dec, cnt, wit

    def violating(self):
        """(number of violating strategies, the smallest or None)."""
        dec, _, wit = self.run()
        allA = allR = self.ones
        for r in self.loyal:
            allA &= dec[r - 1]
            allR &= ~dec[r - 1] & self.ones
        ok = (allA | allR) if self.c else (allA if self.order == O.ATTACK else allR)
        return bin(self.ones & ~ok).count("1"), wit

    def trial(self, dec, S):
        """(decisions word, outcome byte) of strategy S out of the decision planes."""
        d = [(x >> S) & 1 for x in dec]
        return (sum(v << (2 * r) for r, v in enumerate(d)),
                trial_outcome(self.n, self.m, self.fmask, self.order, d))
