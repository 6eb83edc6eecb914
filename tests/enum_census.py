"""Census of the enumeration kernels' instantiations on LIVE free bits.

TEST INFRASTRUCTURE ONLY (not a test file; CPU only, nothing here touches the GPU).

k_kenum<PROTO, N>, k_renum<COMMON, N> and k_enum<ME> are instantiated per shape, and a
comparison with the model at strategy S says something about free bit b only if b is
LIVE at S: the model's outputs at S and at S ^ (1 << b) differ.  Inside the protocols'
bounds almost every sampled strategy is dead in every bit (that is the theorem), so the
strategies are searched for, not sampled.  This module

  evaluate(case, S)        the model's per-strategy output, from the one-strategy forms
                           of kenum_model / renum_model / enum_model
  candidates(family, sel)  the cases of one instantiation within the 48-bit cap
  search(case, budget, seed)  [(S, [bits shown live at S])], seeded and deterministic
  select(family, sel)      one to three cases per instantiation, searched in full

and `python tests/enum_census.py --write` regenerates tests/golden/enum_census.json, which
tests/test_enum_census.py (CPU) and tests/test_gpu_enum_census.py (GPU) read; neither
searches.
"""
from __future__ import annotations

import collections
import functools
import json
import math
import os
import random
import sys
import zlib

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(os.path.dirname(_HERE), "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ba_oracle as O  # noqa: E402
import enum_model as EM  # noqa: E402
import kenum_model as KM  # noqa: E402
import rand_model as RAND  # noqa: E402
import renum_model as RM  # noqa: E402

FIXTURE = os.path.join(_HERE, "golden", "enum_census.json")
SEED = 0xCE75
PROBE = 6      # strategies per candidate when the cases of an instantiation are ranked
BUDGET = 32    # strategies per shortlisted case
SHORT = 3      # cases per role that get the full search, by each of two orders
CAP = 48       # BA_ENUM_MAX_BITS
MAX_SLOTS = EM.MAX_SLOTS  # k_enum's slot map
KING, KING3, LOCAL, COMMON, OM = "king", "king3", "local", "common", "om"
FAMILIES = (KING, KING3, LOCAL, COMMON, OM)
PROTO = {KING: KM.KING, KING3: KM.KING3}
COIN = {LOCAL: RM.LOCAL, COMMON: RM.COMMON}
MAX_M = {KING: 8, KING3: 10, LOCAL: 10, COMMON: 10}
MAX_N = 16      # k_kenum / k_renum keep one plane per general in registers
OM_NS = tuple(range(2, 18)) + (25, 32)  # k_enum's n is a run-time value: every n to 17, then two up to its limit
OM_DEPTHS = 9   # k_enum<0..8>

# family: kenum / renum / om; R = 0 outside RAND; F: the faulty mask; o: the order code
Case = collections.namedtuple("Case", "family n m R F o")


def kernel_name(family, sel):
    return {KING: "k_kenum<KING,%d>", KING3: "k_kenum<KING3,%d>", LOCAL: "k_renum<LOCAL,%d>",
            COMMON: "k_renum<COMMON,%d>", OM: "k_enum<%d>"}[family] % sel


def instantiations():
    """Every (family, sel) the dispatch tables hold: N = 1..16, ME = 0..8."""
    out = [(f, N) for f in (KING, KING3, LOCAL, COMMON) for N in range(1, MAX_N + 1)]
    return out + [(OM, me) for me in range(OM_DEPTHS)]


def sel_of(case):
    return O.effective_depth(case.n, case.m) if case.family == OM else case.n


def tree_slots(n, m):
    return sum(math.perm(n - 1, k + 1) for k in range(O.effective_depth(n, m) + 1))


def bits(case):
    """B by the model's closed form."""
    f, n, m, R, F, _ = case
    if f in PROTO:
        return KM.bits_formula(PROTO[f], n, m, F)
    if f in COIN:
        return RM.bits_formula(COIN[f], n, m, R, F)
    return EM.bits_formula(n, m, F)


def groups(case):
    """The free bits by (round, part) -- by level for OM(m) -- in bit order."""
    f, n, m, R, F, _ = case
    if f in PROTO:
        keys = [(q, part) for q, _, _, part in KM.slots(PROTO[f], n, m, F)]
    elif f in COIN:
        keys = [(q, part) for q, _, _, part in RM.slots(COIN[f], n, m, R, F)]
    else:
        keys = [k for k, _ in EM.free_slots(n, m, F)]
    out = collections.OrderedDict()
    for b, key in enumerate(keys):
        out.setdefault(key, []).append(b)
    return list(out.values())


@functools.lru_cache(maxsize=16)
def _om_index(n, m, F):
    return {key: i for i, key in enumerate(EM.free_slots(n, m, F))}


def _word(dec):
    return sum(d << (2 * r) for r, d in enumerate(dec))


def evaluate(case, S):
    """The model's whole output at strategy S: (decisions word, outcome byte) and, for
    RAND, the `decided` byte."""
    f, n, m, R, F, o = case
    ob = int(o == O.ATTACK)
    if f in PROTO:
        p = PROTO[f]
        dec = KM.history_message(p, n, m, F, ob, KM.messages_of(p, n, m, F, S))[-1][1:]
        return _word(dec), KM.trial_outcome(p, n, m, F, o, dec)
    if f in COIN:
        c = COIN[f]
        hist = RM.history_message(c, n, m, R, F, ob, RM.messages_of(c, n, m, R, F, S))
        dec = hist[-1][0][1:]
        return _word(dec), RAND.trial_outcome(n, m, F, o, dec), RAND.decided_of(n, F, ob, hist)
    dec = EM.decisions_rec(n, m, F, ob, S, _om_index(n, m, F))
    return _word(dec), O.trial_outcome(n, m, F, o, dec)


def live_bits(case, S, B=None):
    """The free bits that decide the output at S."""
    base = evaluate(case, S)
    return [b for b in range(bits(case) if B is None else B) if evaluate(case, S ^ (1 << b)) != base]


# ---------------------------------------------------------------------------
# the cases of an instantiation
# ---------------------------------------------------------------------------
def fault_sets(n):
    """|F| = 0..n-1, traitors lowest-index-first and highest-index-first, with and
    without the commander: the lowest set holds the commander and the kings of the first
    phases, the highest holds neither (while it can), and the two mixed sets hold one."""
    out = []
    for nf in range(n):
        low = (1 << nf) - 1
        sets = [low, low << (n - nf), (low << 1) & ((1 << n) - 1)]
        if nf >= 1:
            sets.append(1 | (((1 << (nf - 1)) - 1) << (n - nf + 1)))
        for F in sets:
            if F not in out and bin(F).count("1") == nf:
                out.append(F)
    return out


def candidates(family, sel):
    """The cases of instantiation (family, sel) within the cap (and, for OM(m), the slot
    map): m over the entry's range, R = 1..3 for RAND, F over fault_sets, both orders."""
    out = []
    if family == OM:
        shapes = [(n, sel, 0) for n in OM_NS if n >= sel + 2 and tree_slots(n, sel) <= MAX_SLOTS]
    else:
        Rs = (1, 2, 3) if family in COIN else (0,)
        shapes = [(sel, m, R) for m in range(MAX_M[family] + 1) for R in Rs]
    for n, m, R in shapes:
        for F in fault_sets(n):
            for o in (O.ATTACK, O.RETREAT):
                case = Case(family, n, m, R, F, o)
                if bits(case) <= CAP:
                    out.append(case)
    return out


# ---------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------
DENSITIES = (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0)


def _rng(case, seed):
    return random.Random(zlib.crc32(repr((seed,) + tuple(case)).encode()))


def search(case, budget, seed=SEED):
    """[(S, bits first shown live at S)] over `budget` strategies.  A strategy is drawn
    with one random density per (round, part); every other draw instead re-draws one
    group of the strategy that served the most bits so far, which stays near the
    thresholds that one sits at.  One S is kept for as many bits as it serves."""
    B = bits(case)
    if B == 0:
        return []
    grp = groups(case)
    rng = _rng(case, seed)
    found, shown, tried, best = [], set(), set(), None

    def draw(S, which):
        for g in which:
            d = rng.choice(DENSITIES)
            for b in g:
                S &= ~(1 << b)
                if rng.random() < d:
                    S |= 1 << b
        return S

    for it in range(budget):
        if len(shown) == B:
            break
        S = draw(best[1], [rng.choice(grp)]) if best and it & 1 else draw(0, grp)
        if S in tried:
            continue
        tried.add(S)
        live = live_bits(case, S, B)
        if best is None or len(live) > best[0]:
            best = (len(live), S)
        new = [b for b in live if b not in shown]
        if new:
            shown.update(new)
            found.append((S, new))
    return found


def shown_live(found):
    return sorted({b for _, bs in found for b in bs})


# ---------------------------------------------------------------------------
# the selection
# ---------------------------------------------------------------------------
def _nf(case):
    return bin(case.F).count("1")


def select(family, sel, seed=SEED, probe=PROBE, budget=BUDGET):
    """One to three cases of the instantiation, each with its full search:
      best    B >= 24 from N = 5 on; then at least half of B shown live, then a live
              bit >= 38, then the most live bits
      ranks   |F| >= 2 traitors and >= 2 loyal generals, where rf * l + rl runs with
              rf > 0 and rl > 0 (one loyal general where the cap leaves no more: rf > 0
              alone); m >= 1 and B >= 39 preferred
      phases  RAND only: R >= 2, with traitors present where the cap allows it
    Every candidate is probed with `probe` strategies; the SHORT best of a role by the
    probe get the full search and the role takes the best of those by its result.
    [(role, case, found)]; a role the cap leaves no case for is absent."""
    probed = {case: _measure(case, search(case, probe, seed)) for case in candidates(family, sel)}
    big = family == OM or sel >= 5

    def k_best(case, B, nl, hi):
        return (B >= 24 or not big, 2 * nl >= B, hi > 0, nl, B)

    def k_ranks(case, B, nl, hi):
        return (case.m >= 1, 2 * nl >= B, B >= 39, hi > 0, nl)

    def k_phases(case, B, nl, hi):
        return (nl, B)

    roles = [("best", k_best, lambda c: True),
             ("ranks", k_ranks, lambda c: _nf(c) >= 2 and c.n - _nf(c) >= 2),
             ("phases", k_phases, lambda c: c.R >= 2 and _nf(c) >= 1)]
    out, taken = [], set()
    for role, key, ok in roles:
        if role == "phases" and family not in COIN:
            continue
        pool = [c for c in probed if ok(c) and c not in taken]
        if role == "phases" and not pool:
            # no traitor fits under the cap with two phases: the loop over the phases
            # still runs twice with F empty, where only whole windows can be compared
            pool = [c for c in probed if c.R >= 2 and c not in taken]
        if role == "ranks" and not pool:
            # the cap leaves two traitors only beside one loyal general: rf > 0 still runs
            pool = [c for c in probed if _nf(c) >= 2 and c.n - _nf(c) >= 1 and c not in taken]
        if not pool:
            continue
        # sorted is stable: equals stay in candidates' order
        short = sorted(pool, key=lambda c: key(c, *probed[c]), reverse=True)[:SHORT]
        short += [c for c in sorted(pool, key=lambda c: probed[c][1], reverse=True)[:SHORT] if c not in short]
        full = {c: search(c, budget, seed) for c in short}
        top = max(short, key=lambda c: key(c, *_measure(c, full[c])))
        if role == "ranks" and not full[top]:
            continue
        taken.add(top)
        out.append((role, top, full[top]))
    return out


def _measure(case, found):
    live = shown_live(found)
    return bits(case), len(live), sum(1 for b in live if b >= 38)


def records(family, sel, seed=SEED):
    """The fixture's entries of one instantiation."""
    out = []
    for role, case, found in select(family, sel, seed):
        out.append({"kernel": kernel_name(family, sel), "family": family, "sel": sel, "role": role,
                    "n": case.n, "m": case.m, "R": case.R, "F": case.F, "o": case.o, "B": bits(case),
                    "live": [[S, bs] for S, bs in found]})
    return out


def case_of(rec):
    return Case(rec["family"], rec["n"], rec["m"], rec["R"], rec["F"], rec["o"])


def reachable():
    """The instantiations some case within the limits reaches."""
    return [(f, s) for f, s in instantiations() if candidates(f, s)]


def generate(seed=SEED):
    cases = []
    for f, s in reachable():
        cases += records(f, s, seed)
    return {"seed": seed, "probe": PROBE, "budget": BUDGET, "cases": cases}


def dumps(doc):
    """One case per line."""
    head = {k: v for k, v in doc.items() if k != "cases"}
    lines = [json.dumps(c, separators=(",", ":")) for c in doc["cases"]]
    return json.dumps(head)[:-1] + ', "cases": [\n' + ",\n".join(lines) + "\n]}\n"


def load():
    with open(FIXTURE) as fh:
        return json.load(fh)


def table(doc):
    """instantiation, case, B, live bits: one row per recorded case."""
    rows = []
    for rec in doc["cases"]:
        live = shown_live(rec["live"])
        what = f"({rec['n']},{rec['m']})" + (f" R={rec['R']}" if rec["R"] else "")
        rows.append(f"{rec['kernel']:<20} {rec['role']:<6} {what:<12} F={rec['F']:#06x} o={rec['o']} "
                    f"B={rec['B']:>2} live={len(live):>2} low={sum(b < 6 for b in live)} "
                    f"mid={sum(6 <= b < 38 for b in live):>2} high={sum(b >= 38 for b in live):>2} "
                    f"S={len(rec['live'])}")
    return "\n".join(rows)


def table_markdown(doc):
    """DESIGN.md's table: one row per instantiation, its cases as `(n,m[,R]) F o: live/B`
    with the live bits >= 38 in brackets."""
    rows = collections.OrderedDict()
    for rec in doc["cases"]:
        live = shown_live(rec["live"])
        what = f"({rec['n']},{rec['m']}" + (f",R={rec['R']}" if rec["R"] else "") + ")"
        high = sum(b >= 38 for b in live)
        rows.setdefault(rec["kernel"], []).append(
            f"{what} F={rec['F']:#x} o={rec['o']}: {len(live)}/{rec['B']}" + (f" [{high}]" if high else ""))
    out = ["| instantiation | cases: live bits / B [of them >= 38] |", "|---|---|"]
    return "\n".join(out + [f"| `{k}` | {'; '.join(v)} |" for k, v in rows.items()])


if __name__ == "__main__":
    if "--write" in sys.argv[1:]:
        doc = generate()
        with open(FIXTURE, "w") as fh:
            fh.write(dumps(doc))
    print(table_markdown(load()) if "--markdown" in sys.argv[1:] else table(load()))
