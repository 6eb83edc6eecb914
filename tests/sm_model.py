"""Reference model of SM(m), Lamport's signed-messages algorithm (docs/SEMANTICS.md §6).

TEST INFRASTRUCTURE ONLY (not a test file).  Two implementations written apart
from each other and from the HIP kernel:

  chain form  -- the textbook one: explicit signed messages, each a value plus
                 the chain of lieutenants that signed it after the commander.
                 One trial at a time.  `run` uses this one.
  plane form  -- the fresh/has bit planes of §6 over a 64-trial word, no chains.

Coins, synthetic inputs and the quorum come from oracle/ba_oracle.py (`lie`,
`gen`, `quorum`); the Philox blocks behind `lie` are cached per (word, k, pair)
so n = 32 stays within seconds.
"""
from __future__ import annotations

import ba_oracle as O

SM_TAG = 64  # ctr word 1 of SM draws: c(k, x) = coin(64 + k, x)
_M64 = (1 << 64) - 1


class Coins:
    """c(k, x) of §6 for one seed: ba_oracle.lie(seed, t, 64 + k, x), with the
    Philox block of (trial word, k, pair) computed once."""

    def __init__(self, seed: int):
        self.seed = seed
        self.key = (seed & O.M32, seed >> 32)
        self.blocks = {}

    def words(self, w: int, k: int, pair: int):
        """(retreat half, attack half) = the 64-trial coin words of x = 2 pair, 2 pair + 1."""
        key = (w, k, pair)
        b = self.blocks.get(key)
        if b is None:
            o = O.philox4x32_10((pair, SM_TAG + k, w & O.M32, w >> 32), self.key)
            b = self.blocks[key] = (o[1] << 32 | o[0], o[3] << 32 | o[2])
        return b

    def __call__(self, t: int, k: int, x: int) -> int:
        return (self.words(t >> 6, k, x >> 1)[x & 1] >> (t & 63)) & 1


def pair_index(j: int, r: int, L: int) -> int:
    """Index of the ordered (sender j, recipient r) pair, r != j."""
    return j * (L - 1) + r - (1 if r > j else 0)


def coin_calls(n: int, m: int) -> int:
    """Philox calls per 64-trial word: L + me L (L - 1)."""
    if n < 1:
        return 0
    L, me = n - 1, O.effective_depth(n, m)
    return L + me * L * (L - 1)


# ---------------------------------------------------------------------------
# chain form
# ---------------------------------------------------------------------------
def vsets_chain(n, m, coins: Coins, t, fmask, ob):
    """V_r of every lieutenant rank r, as a list of sets, by explicit messages."""
    L, me = n - 1, O.effective_depth(n, m)
    V = [set() for _ in range(L)]

    def faulty(g):
        return (fmask >> g) & 1

    # round 0: the commander signs and sends; message = (value, chain of relayers)
    inbox = [[] for _ in range(L)]
    for r in range(L):
        if faulty(0):
            for v in (0, 1):
                if coins(t, 0, 2 * r + v):
                    inbox[r].append((v, ()))
        else:
            inbox[r].append((ob, ()))
    for k in range(me + 1):
        relay = []
        for r in range(L):
            for v, chain in inbox[r]:
                # k lieutenants signed after the commander; all distinct; never the recipient
                assert len(chain) == k and len(set(chain)) == k and r not in chain
                if v not in V[r]:
                    V[r].add(v)
                    relay.append((r, v, chain + (r,)))  # r signs; relays next round
        if k == me:
            break
        inbox = [[] for _ in range(L)]
        for j, v, chain in relay:
            for r in range(L):
                if r in chain:  # signers already hold v (j itself included)
                    continue
                if not faulty(j + 1) or coins(t, k + 1, 2 * pair_index(j, r, L) + v):
                    inbox[r].append((v, chain))
    return V


# ---------------------------------------------------------------------------
# plane form: 64 trials per word, no chains
# ---------------------------------------------------------------------------
def vsets_plane_word(n, m, coins: Coins, w, fmasks, obs):
    """V sets of the trials 64 w + b, b < len(fmasks): list (per trial) of lists of sets."""
    L, me = n - 1, O.effective_depth(n, m)
    nb = len(fmasks)
    F = [sum(((fmasks[b] >> g) & 1) << b for b in range(nb)) for g in range(n)]
    OB = sum((obs[b] & 1) << b for b in range(nb))
    has = [[0] * L, [0] * L]  # has[v][r]
    fresh = [[0] * L, [0] * L]
    for r in range(L):
        c = coins.words(w, 0, r) if F[0] else (0, 0)
        recv = [(F[0] & c[0]) | (~F[0] & ~OB & _M64), (F[0] & c[1]) | (~F[0] & OB)]
        for v in (0, 1):
            fresh[v][r] = recv[v]
            has[v][r] = recv[v]
    for k in range(1, me + 1):
        recv = [[0] * L, [0] * L]
        for j in range(L):
            if not (fresh[0][j] | fresh[1][j]):
                continue
            Fj = F[j + 1]
            for r in range(L):
                if r == j:
                    continue
                c = coins.words(w, k, pair_index(j, r, L)) if Fj else (0, 0)
                for v in (0, 1):
                    recv[v][r] |= fresh[v][j] & ((~Fj & _M64) | c[v])
        for v in (0, 1):
            for r in range(L):
                fresh[v][r] = recv[v][r] & ~has[v][r] & _M64
                has[v][r] |= fresh[v][r]
    return [[{v for v in (0, 1) if (has[v][r] >> b) & 1} for r in range(L)] for b in range(nb)]


# ---------------------------------------------------------------------------
# per-trial results and the run
# ---------------------------------------------------------------------------
def choice(V) -> int:
    return O.ATTACK if V == {1} else O.RETREAT


def trial_outcome(n, m, fmask, order_code, dec):
    """Outcome byte: §2.4 with the SM in-bound rule |F| <= m."""
    q = O.quorum(n, order_code, dec)[0]
    loyal = [dec[r - 1] for r in range(1, n) if not (fmask >> r) & 1]
    agree = int(len(set(loyal)) <= 1)
    appl = int(not fmask & 1)
    want = O.ATTACK if order_code == O.ATTACK else O.RETREAT
    valid = int(appl and all(d == want for d in loyal))
    inb = int(bin(fmask).count("1") <= m)
    return q | agree << 2 | appl << 3 | valid << 4 | inb << 5


def inputs(n, seed, faulty_mode, f, order_mode, order_value, t, i, faulty, order):
    gm, go = O.gen(n, seed, faulty_mode, f, order_mode, order_value, t)
    fmask = (faulty[i] if faulty_mode == O.FAULTY_GIVEN else gm) & ((1 << n) - 1)
    oc = order[i] if order_mode == O.ORDER_GIVEN else go
    return int(fmask), int(oc)


def run(n, m, seed=0, faulty_mode=O.FAULTY_GIVEN, f=0, order_mode=O.ORDER_GIVEN,
        order_value=O.ATTACK, first_trial=0, batch=1, faulty=None, order=None, form="chain"):
    """(decisions, outcomes, vsets, counters dict) of trials [first_trial, + batch)."""
    assert first_trial % 64 == 0
    coins = Coins(seed)
    ins = [inputs(n, seed, faulty_mode, f, order_mode, order_value, first_trial + i, i, faulty,
                  order) for i in range(batch)]
    if form == "chain":
        Vs = [vsets_chain(n, m, coins, first_trial + i, fm, int(oc == O.ATTACK))
              for i, (fm, oc) in enumerate(ins)]
    else:
        Vs = []
        for i0 in range(0, batch, 64):
            part = ins[i0:i0 + 64]
            Vs += vsets_plane_word(n, m, coins, (first_trial + i0) >> 6, [p[0] for p in part],
                                   [int(p[1] == O.ATTACK) for p in part])
    decisions, outcomes, vsets = [], [], []
    cnt = dict.fromkeys(O.COUNTERS, 0)
    for (fmask, oc), V in zip(ins, Vs):
        dec = [choice(v) for v in V]
        dword = vword = 0
        for r, (d, v) in enumerate(zip(dec, V)):
            dword |= d << (2 * r)
            vword |= (int(1 in v) | int(0 in v) << 1) << (2 * r)
        out = trial_outcome(n, m, fmask, oc, dec)
        decisions.append(dword)
        outcomes.append(out)
        vsets.append(vword)
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
    return decisions, outcomes, vsets, cnt


def violations(outcomes) -> int:
    """Trials in which IC1 or IC2 fails."""
    return sum(1 for o in outcomes if not ((o >> 2) & 1 and (not (o >> 3) & 1 or (o >> 4) & 1)))


def two_valued(vsets) -> int:
    """Trials in which some lieutenant holds both values."""
    return sum(1 for v in vsets if v & (v >> 1) & 0x5555555555555555)
