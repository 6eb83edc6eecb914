"""The OM(m) shape lattice and the engines' dispatch rule, restated.

Test infrastructure, host only.  ba_run_trials picks among several dozen kernel
instantiations by (n, m_eff, engine, batch words) alone.  This module lists every shape
the sweep runs (LATTICE), restates the dispatch as plain functions -- from include/ba.h,
DESIGN.md and the launch code (ba_api.cpp run_trials_device_impl, ba_fused.hip
launch_fused / plan_fused, ba_wave3.hip, ba_levels.hip launch_levels_chunk, ba_tail.hip,
ba_cascade.hip) -- and builds the inputs both test files use.  Nothing here calls the
library: tests/test_om_lattice.py compares the rule with ba_engine_for on the host, and
tests/test_gpu_om_lattice.py with the kernel profile on the device."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

MAX_N, MAX_DEPTH = 32, 8

# Two conditions that keep scratch and oracle cost small (not measurements): the
# two-word batch runs every shape whose tree has at most SLOTS_SMALL slots, the
# eighteen-word batch those with at most SLOTS_WIDE.
SLOTS_SMALL = 1 << 22
SLOTS_WIDE = 1 << 19

B_SMALL = 70            # two 64-trial words, ragged
B_WIDE = 64 * 17 + 5    # eighteen words, ragged
B_LARGE = 64 ** 3 + 37  # 4097 words: 65 groups of 64 words (the big-batch epilogues)
BATCHES = (B_SMALL, B_WIDE)


def words_of(batch):
    return (batch + 63) // 64


# ---------------------------------------------------------------------------
# geometry, closed form
# ---------------------------------------------------------------------------
def m_eff(n, m):
    return 0 if n < 2 else min(m, n - 2)


def perm(L, k):
    """P(L, k) = L (L-1) .. (L-k+1); 0 when k > L."""
    p = 1
    for i in range(k):
        p *= max(0, L - i)
    return p


def level_slots(n, me, k):
    """|L_k| = P(n-1, k+1), k = 0..me."""
    return perm(n - 1, k + 1)


def tree_slots(n, me):
    return sum(level_slots(n, me, k) for k in range(me + 1))


# ---------------------------------------------------------------------------
# the lattice
# ---------------------------------------------------------------------------
def _lattice():
    out = []
    for n in range(1, MAX_N + 1):
        for me in range(0, m_eff(n, MAX_DEPTH) + 1):
            if tree_slots(n, me) <= SLOTS_SMALL:
                out.append((n, me))  # m = m_eff: one m per distinct effective depth
    return out


LATTICE = _lattice()
# m > m_eff: must equal the twin (n, m_eff) bit for bit
ALIASES = [(1, 3), (2, 5), (3, 8), (4, 5), (9, 8)]


def shapes_of(n):
    return [(nn, me) for nn, me in LATTICE if nn == n]


def aliases_of(n):
    return [(nn, m) for nn, m in ALIASES if nn == n]


def batches_of(n, me):
    """The batches of the sweep a shape runs at (the slot caps)."""
    s = tree_slots(n, me)
    return [b for b, cap in ((B_SMALL, SLOTS_SMALL), (B_WIDE, SLOTS_WIDE)) if s <= cap]


# ---------------------------------------------------------------------------
# the dispatch, restated
# ---------------------------------------------------------------------------
K_LEAF_MAX_S = 12          # k_leaf / k_leaf_up / k_fused are instantiated for S = n - m_eff in 2..12
K_FUSED_MAX_DEPTH = 6
K_FUSED_LDS_WORDS = 39 * 1024 // 8
K_TOP_MAX = 6              # k_relay_top<K>, K = 0..6
K_TOP_FUSE_WORDS = 2       # inputs bit-sliced inside k_relay_top up to two words
K_TAIL_MAX_WORDS = 16
CASCADE_SHAPES = {(16, 5), (16, 4), (16, 3), (10, 3), (9, 4), (8, 5)}  # BA_CASC_SHAPES
CASCADE_CO_WORDS = 4

# every ProfScope name of the OM(m) engines
NAMES = frozenset(["k_om3w", "k_om3wt", "k_om4w", "k_fused", "k_cascade", "k_cascade_co",
                   "k_cascade_units", "k_cascade_mtop", "k_cascade_wtop", "k_cascade_top",
                   "k_input", "k_relay_top", "k_relay_inner", "k_relay_leaf", "k_leaf",
                   "k_leaf_up", "k_majority_inner", "k_majority_leaf", "k_tail", "k_epilogue"])


def normalise(profile_names):
    """Profile names as the rule names them: the units launch of the two-launch cascade
    picks its latency mode by the chip's size, which the rule does not restate."""
    return {"k_cascade_units" if k == "k_cascade_units_lat" else k for k in profile_names}


def planes_for(s):
    """Bit-sliced counter planes for a count up to s: the smallest p with 2^p > s."""
    p = 1
    while (1 << p) <= s:
        p += 1
    return p


def leaf_supported(n, me):
    return me >= 2 and 2 <= n - me <= K_LEAF_MAX_S


def wave_supported(n, me):
    return (me == 3 and 5 <= n <= 14) or (me == 4 and 6 <= n <= 14)


def plan_fused(n, me):
    """k_fused keeps one trial word's tree in LDS: F[n] OB OO VAL, L_0..L_{me-2},
    R_1..R_{me-1} (and 2L root words at depth 2), within 39 KiB."""
    if not leaf_supported(n, me) or me > K_FUSED_MAX_DEPTH:
        return False
    o = n + 3
    o += sum(level_slots(n, me, k) for k in range(0, me - 1))
    o += sum(level_slots(n, me, p) for p in range(1, me))
    if me == 2:
        o += 2 * (n - 1)
    o = (o + 1) & ~1
    return o <= K_FUSED_LDS_WORDS


def engine_for(n, me):
    """What ENGINE_AUTO picks: 'FUSED' (a WAVE kernel or k_fused) or 'LEVELS'."""
    return "FUSED" if wave_supported(n, me) or plan_fused(n, me) else "LEVELS"


Expect = namedtuple("Expect", "names inst")
"""names: the kernel names the profile must show -- every other name of NAMES is
forbidden; inst: the instantiations (kernel, template argument...) the run lands on."""


def levels_kernels(n, me, leaf, words, no_in=False, no_up=False, no_tail=False, epi_w=True):
    """The multi-launch LEVELS pipeline (ba_levels.hip launch_levels_chunk) over one chunk
    of `words` trial words; leaf: L_{me-1} and L_me generated by k_leaf, not stored."""
    L = n - 1
    names, inst = set(), set()
    fuse = not no_in and words <= K_TOP_FUSE_WORDS
    ktop = me - 2 if leaf else me
    kf = ktop if (leaf or me == 0) else me - 1
    if not fuse or kf > K_TOP_MAX:
        names.add("k_input")
    if kf <= K_TOP_MAX:
        names.add("k_relay_top")
        inst.add(("k_relay_top", kf))
        k_first = kf + 1
    else:
        inst.add(("k_relay_fallback",))
        k_first = 0
    for k in range(k_first, ktop + 1):
        names.add("k_relay_leaf" if k == me else "k_relay_inner")
    up = leaf and me >= 3 and not no_up
    if leaf:
        names.add("k_leaf_up" if up else "k_leaf")
        inst.add(("k_leaf_up" if up else "k_leaf", n - me))
    pdeep = me - ((3 if up else 2) if leaf else 1)
    tail = (not no_tail and pdeep >= 1 and words <= K_TAIL_MAX_WORDS and me >= 2 and 4 <= n <= 16)
    for p in range(pdeep, (2 if tail else 1) - 1, -1):
        names.add("k_majority_leaf" if p + 1 == me else "k_majority_inner")
        inst.add(("k_majority", planes_for(L - p)))
    if tail:
        names.add("k_tail")
        inst.add(("k_tail", n))
        return Expect(names, inst)
    names.add("k_epilogue")
    if (words + 63) // 64 >= 64 and 4 <= n <= 16 and me >= 1:  # 64 groups of 64 words
        inst.add(("k_epilogue_w", n) if epi_w else ("k_epilogue_bs", 4 if planes_for(n) <= 4 else 5))
    else:
        inst.add(("k_epilogue", planes_for(L)))
    return Expect(names, inst)


def cascade_kernels(n, me, words):
    inst = {("k_cascade", n, me)}
    if me < 4:
        return Expect({"k_cascade"}, inst)
    if words <= CASCADE_CO_WORDS:
        return Expect({"k_cascade_co"}, inst)
    return Expect({"k_cascade_units", "k_cascade_mtop"}, inst)


def fused_kernels(n, me, generic=False, pair_table=True):
    if wave_supported(n, me) and not generic:
        if me == 4:
            return Expect({"k_om4w"}, {("k_om4w", n)})
        if n == 10 and pair_table:
            return Expect({"k_om3wt"}, {("k_om3wt", 10)})
        return Expect({"k_om3w"}, {("k_om3w", n)})
    assert plan_fused(n, me), (n, me)
    return Expect({"k_fused"}, {("k_fused", n - me, me)})


# How each variant is run (tests/test_gpu_om_lattice.py) and what it must launch.
#   V1  ENGINE_AUTO, default environment
#   V2  ENGINE_LEVELS with BA_NO_CASCADE=1: the pipeline with leaf kernels
#   V3  ENGINE_LEVELS on an Engine created under BA_NO_LEAF_FUSION=1: materialised leaves
#   V4  ENGINE_FUSED with BA_FUSED_KIND=2: the generic k_fused on a WAVE shape
#   V5  ENGINE_AUTO with BA_OM3W_TABLE=0 at (10, 3): k_om3w<10> (k_om3wt is the default there)
#   LEVELS  ENGINE_LEVELS, default environment (the cascade where it applies); not part of
#           the sweep: tests/test_gpu_cascade.py asserts it
VARIANTS = ("V1", "V2", "V3", "V4", "V5")


def applies(variant, n, me):
    if variant in ("V1", "V2", "LEVELS"):
        return True
    if variant == "V3":
        return leaf_supported(n, me)
    if variant == "V4":
        return wave_supported(n, me) and plan_fused(n, me)
    if variant == "V5":
        return (n, me) == (10, 3)
    raise ValueError(variant)


def use_cascade(n, me):
    return leaf_supported(n, me) and me >= 3 and (n, me) in CASCADE_SHAPES


def expect(n, me, variant, words, **switches):
    """Expect of one ba_run_trials call of `words` trial words (one chunk: every batch of
    the sweep fits one).  switches: levels_kernels' (the BA_NO_* environment)."""
    assert applies(variant, n, me), (variant, n, me)
    if variant in ("V1", "V5"):
        if engine_for(n, me) == "FUSED":
            return fused_kernels(n, me, pair_table=variant == "V1")
        variant = "LEVELS"
    if variant == "V4":
        return fused_kernels(n, me, generic=True)
    if variant == "LEVELS" and use_cascade(n, me):
        return cascade_kernels(n, me, words)
    return levels_kernels(n, me, leaf_supported(n, me) and variant != "V3", words, **switches)


# The large-batch leg beside the lattice: B_LARGE, m = 1, ENGINE_LEVELS, given inputs.
LARGE_EPI = [(n, 1, epi_w) for n in range(4, 17) for epi_w in (True, False)]
LARGE_PER_TRIAL = [(n, 1) for n in (2, 3, 17, 18, 31, 32)] + [(17, 2)]


def reach():
    """Every instantiation the sweep lands on: lattice x variants x batches, and the
    large-batch leg."""
    got = set()
    for n, me in LATTICE:
        for v in VARIANTS:
            if applies(v, n, me):
                for b in batches_of(n, me):
                    got |= expect(n, me, v, words_of(b)).inst
    for n, m, epi_w in LARGE_EPI:
        got |= expect(n, m_eff(n, m), "LEVELS", words_of(B_LARGE), epi_w=epi_w).inst
    for n, m in LARGE_PER_TRIAL:
        got |= expect(n, m_eff(n, m), "LEVELS", words_of(B_LARGE)).inst
    return got


def reachable():
    """Every instantiation ANY call can reach: all 1 <= n <= 32, 0 <= m_eff <= 8 whose
    levels stay below the engines' 2^31-slot limit, every variant, one to 4097 words,
    every BA_NO_* switch."""
    got = set()
    for n in range(1, MAX_N + 1):
        for me in range(0, m_eff(n, MAX_DEPTH) + 1):
            if level_slots(n, me, me) > 1 << 31:
                continue
            for v in VARIANTS:
                if not applies(v, n, me):
                    continue
                for w in (1, 2, 3, 4, 5, 16, 17, 18, words_of(B_LARGE)):
                    got |= expect(n, me, v, w).inst
                    if v in ("V2", "V3"):
                        for sw in (dict(no_up=True), dict(no_tail=True), dict(epi_w=False),
                                   dict(no_up=True, no_tail=True)):
                            got |= expect(n, me, v, w, **sw).inst
    return got


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def drawn_kw(n, me):
    """The drawn leg: faulty sets and orders drawn in the kernel, a non-zero first trial."""
    return dict(seed=0x0D1A77 + 977 * n + me, faulty_mode=1, f=(n - 1) // 3 + 1, order_mode=1,
                first_trial=64 * (1000 + n))


def given_kw(n, me, batch):
    """The given leg: trial t cycles through
         t % 4 == 0  only the commander faulty: every lieutenant relays what it got, so an
                     even number of lieutenants ties whenever the commander's coins split
                     evenly (the root-tie path);
         t % 4 == 1  a dense faulty set (each general faulty with probability 1/2);
         t % 4 == 2  a sparse one (probability 1/8);
         t % 4 == 3  the commander and a sparse set of lieutenants;
       trial 1 is the all-faulty mask; orders are uniform over retreat / attack / OTHER."""
    rng = np.random.default_rng([n, batch])
    full = (1 << n) - 1

    def draw():
        return rng.integers(0, 1 << n, batch, dtype=np.uint64)

    dense, sparse, sparse2 = draw(), draw() & draw() & draw(), draw() & draw() & draw()
    t = np.arange(batch)
    fm = np.where(t % 4 == 0, np.uint64(1),
                  np.where(t % 4 == 1, dense, np.where(t % 4 == 2, sparse, sparse2 | np.uint64(1))))
    if batch > 1:
        fm[1] = full
    order = rng.choice([0, 1, 2], batch).astype(np.uint8)
    return dict(seed=0x61BE4 + n, first_trial=64 * (7 + n), faulty=(fm & np.uint64(full)).astype(np.uint32),
                order=order)
